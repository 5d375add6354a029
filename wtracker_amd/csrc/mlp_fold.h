// The two parameter layouts of a ResMLP and the one function that turns the first into the second, for host and device.
//   state  the trainer's unfolded parameters of one model (MlpTrainLayerDev: state_layout in mlp_train.hip): per layer W [out][in], b, [gamma, beta],
//          then per BatchNorm layer running_mean, running_var
//   blob   what mlp_kernel reads (MlpLayerDev): per layer W [out_pad][in_pad], in_pad = ceil4(in), out_pad = ceil16(out), zero padded, then b [out_pad];
//          the whole rounded up to 4 floats (the kernels copy it to LDS as float4)
// mlp_fold_row is resmlp._fold bit for bit: float64 arithmetic cast to float32 at the end, s = gamma / sqrt(var + 1e-5), W' = W s,
// b' = (b - mean) s + beta with the product and the sum rounded separately (numpy does not fuse them; contraction is switched off in the function itself).
#pragma once
#include "wtk_kernels.h"

#include <cmath>
#include <cstdint>

namespace wtk {

struct MlpTrainLayerDev {
    int in_dim, out_dim, relu, bn;
    int w_off, b_off, g_off, be_off; // float offsets in the state: trainable section
    int rm_off, rv_off;              // ... and in the buffer section behind it (bn only)
    int pad_[2];
};

__host__ __device__ inline int mlp_in_pad(int in_dim) { return (in_dim + 3) / 4 * 4; }
__host__ __device__ inline int mlp_out_pad(int out_dim) { return (out_dim + 15) / 16 * 16; }
__host__ __device__ inline int mlp_layer_blob_floats(int in_dim, int out_dim) { return mlp_out_pad(out_dim) * mlp_in_pad(in_dim) + mlp_out_pad(out_dim); }
__host__ __device__ inline int mlp_blob_round(int floats) { return (floats + 3) / 4 * 4; }

// Layer i of the blob, given the float offset `off` at which it starts; returns the offset of the next layer.
__host__ __device__ inline int mlp_blob_layer(MlpLayerDev &l, int in_dim, int out_dim, int relu, int off) {
    l.in_dim = in_dim, l.out_dim = out_dim;
    l.in_pad = mlp_in_pad(in_dim), l.out_pad = mlp_out_pad(out_dim);
    l.relu = relu;
    l.w_off = off;
    l.b_off = off + l.out_pad * l.in_pad;
    l.pad_ = 0;
    return l.b_off + l.out_pad;
}

// The blob layout of a structure (Layer: anything with in_dim, out_dim, relu) with wtk_mlp_create's refusals, in its order: the blob's floats, or -1 with
// *why naming the reason.  L (nullable): the n_layers table entries.
template <class Layer>
inline int64_t mlp_blob_layout(const Layer *layers, int n_layers, int n_blocks, int layers_per_block, MlpLayerDev *L, const char **why) {
    const char *dummy;
    if (!why) why = &dummy;
    if (!layers) return *why = "null argument", -1;
    if (n_layers != 2 + n_blocks * layers_per_block) return *why = "n_layers != 2 + n_blocks*layers_per_block", -1;
    if (n_layers > kMlpMaxLayers) return *why = "too many layers", -1;
    if (n_layers < 2) return *why = "n_layers != 2 + n_blocks*layers_per_block", -1;
    const int per = layers_per_block > 1 ? layers_per_block : 1;
    int off = 0;
    for (int i = 0; i < n_layers; ++i) {
        const Layer &s = layers[i];
        if (s.in_dim <= 0 || s.out_dim <= 0 || s.in_dim > kMlpMaxDim || s.out_dim > kMlpMaxDim) return *why = "layer dim out of range", -1;
        if (i > 0) {
            const bool block_first = (i - 1) % per == 0 && i < n_layers - 1;
            const int prev_out = (block_first || i == n_layers - 1) ? layers[0].out_dim : layers[i - 1].out_dim;
            if (s.in_dim != prev_out) return *why = "layer dims do not chain", -1;
        }
        MlpLayerDev l;
        off = mlp_blob_layer(l, s.in_dim, s.out_dim, s.relu, off);
        if (L) L[i] = l;
    }
    for (int b = 0; b < n_blocks; ++b) // every block must return to the residual width
        if (layers[layers_per_block * (b + 1)].out_dim != layers[0].out_dim) return *why = "block output dim != residual dim", -1;
    return mlp_blob_round(off);
}

// Row o (< out_pad) of layer i of one model: its in_pad weights and its bias, from the model's state into its blob.  `w_off`: where the layer starts in
// the blob (mlp_blob_layer).  Rows and columns of the padding are written as 0.
__host__ __device__ inline void mlp_fold_row(const MlpTrainLayerDev &T, int w_off, int o, const float *state, float *blob) {
#pragma clang fp contract(off)
    const int in_pad = mlp_in_pad(T.in_dim), out_pad = mlp_out_pad(T.out_dim);
    float *W = blob + w_off + (size_t)o * in_pad;
    float *b = blob + w_off + (size_t)out_pad * in_pad + o;
    if (o >= T.out_dim) {
        for (int k = 0; k < in_pad; ++k) W[k] = 0.f;
        *b = 0.f;
        return;
    }
    const float *w = state + T.w_off + (size_t)o * T.in_dim;
    if (T.bn) {
        const double s = (double)state[T.g_off + o] / sqrt((double)state[T.rv_off + o] + 1e-5);
        for (int k = 0; k < T.in_dim; ++k) W[k] = (float)((double)w[k] * s);
        const double t = ((double)state[T.b_off + o] - (double)state[T.rm_off + o]) * s;
        *b = (float)(t + (double)state[T.be_off + o]);
    } else {
        for (int k = 0; k < T.in_dim; ++k) W[k] = w[k];
        *b = state[T.b_off + o];
    }
    for (int k = T.in_dim; k < in_pad; ++k) W[k] = 0.f;
}

} // namespace wtk
