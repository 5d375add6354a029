// The ResMLP forward arithmetic, stated once for mlp_kernel (mlp.hip) and the population kernel (mlp_population.hip): one wavefront owns 16 samples whose
// activations ping-pong between two LDS buffers of [16][kLdAct] while the residual stream lives in a third.  Every Linear is the k-ordered
// v_mfma_f32_16x16x4_f32 chain of mlp_layer, per sample an fp32 fma chain: a sample's result does not depend on which tile, wave or workgroup computes it.
#pragma once
#include "wtk_device.h"

namespace wtk {

constexpr int kLdAct = kMlpMaxDim + 4; // LDS row stride (floats), +4 breaks the power-of-two stride
constexpr int kMlpLdsParams = 32768 - 64; // floats of the parameter blob staged in LDS (the fast path may read 63 floats past the blob)

// y[16][out_pad] = act(W x + b); src/dst are LDS [16][kLdAct]
// FAST (parameters in LDS): all fragments of a 64-deep K slice are fetched first — 32 LDS reads in flight instead of a
// read -> wait -> MFMA round trip per k step — then the MFMA chain runs (same k order: bit-identical results).  Reads past
// in_pad stay inside the activation row / the LDS parameter array and are never multiplied.
template <bool FAST, typename P> // P: const float * into LDS or global memory
__device__ __forceinline__ void mlp_layer(P params, const MlpLayerDev &L, const float *src, float *dst, int lane) {
    const int r = lane & 15, g = lane >> 4;
    P W = params + L.w_off;
    P bvec = params + L.b_off;
    for (int n0 = 0; n0 < L.out_pad; n0 += 16) {
        floatx4 acc = {0.f, 0.f, 0.f, 0.f};
        P wrow = W + (n0 + r) * L.in_pad;
        if constexpr (FAST) {
            for (int kb = 0; kb < L.in_pad; kb += 64) {
                float xa[16], wb[16];
#pragma unroll
                for (int ks = 0; ks < 16; ++ks) {
                    xa[ks] = src[r * kLdAct + kb + 4 * ks + g];
                    wb[ks] = wrow[kb + 4 * ks + g];
                }
#pragma unroll
                for (int ks = 0; ks < 16; ++ks)
                    if (kb + 4 * ks < L.in_pad) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[ks], wb[ks], acc, 0, 0, 0);
            }
        } else {
            for (int k0 = 0; k0 < L.in_pad; k0 += 4) {
                const float xa = src[r * kLdAct + k0 + g]; // A[row = sample r][k = k0 + g]
                const float wb = wrow[k0 + g];             // B[k = k0 + g][col = out n0 + r]
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xa, wb, acc, 0, 0, 0);
            }
        }
        // lane holds D[row = 4g + i][col = r]: sample 4g+i, out n0+r
        const float b = bvec[n0 + r];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float v = acc[i] + b;
            if (L.relu) v = fmaxf(v, 0.f);
            dst[(4 * g + i) * kLdAct + n0 + r] = v;
        }
    }
}

// The network over one tile of 16 samples: the input rows are in bufA (zero padded), the output rows end up in bufA.  Every wave of the workgroup
// calls it the same number of times (the barriers are the workgroup's); the three buffers are the calling wave's own.
template <bool FAST, typename P>
__device__ __forceinline__ void mlp_forward_tile(P params, const MlpLayerDev *layers, int n_blocks, int layers_per_block, float *bufA, float *bufB, float *bufH,
                                                 int lane) {
    int li = 0;
    // input layer -> h
    mlp_layer<FAST>(params, layers[li++], bufA, bufH, lane);
    __syncthreads();
    for (int b = 0; b < n_blocks; ++b) {
        const float *src = bufH;
        float *dst = bufA;
        for (int l = 0; l < layers_per_block; ++l) {
            mlp_layer<FAST>(params, layers[li++], src, dst, lane);
            __syncthreads();
            src = dst;
            dst = (dst == bufA) ? bufB : bufA;
        }
        // h <- h + block(h)
        for (int i = lane; i < 16 * kLdAct; i += 64) bufH[i] += src[i];
        __syncthreads();
    }
    mlp_layer<FAST>(params, layers[li], bufH, bufA, lane);
    __syncthreads();
}

// The batched form of MLPController.provide_movement_vector's input (wtracker/sim/sim_controllers/mlp_controllers.py:38-56) for ONE sample: the n_in boxes
// of the float32 track at t + input_frames[j], x / y made relative to the first box's corner, into row[0 .. 4 n_in).  Returns 0, with the row's in_dim
// floats zeroed, where a frame lies outside the track or a box is not finite.
__device__ __forceinline__ int mlp_gather_sample(const float *track, int n_frames, int t, const int *input_frames, int n_in, int in_dim, float *row) {
    int ok = 1;
    float x0 = 0.f, y0 = 0.f;
    for (int j = 0; j < n_in; ++j) {
        const int f = t + input_frames[j];
        if (f < 0 || f >= n_frames) {
            ok = 0;
            break;
        }
        const float4 b = *reinterpret_cast<const float4 *>(track + (long long)f * 4);
        if (!(isfinite(b.x) && isfinite(b.y) && isfinite(b.z) && isfinite(b.w))) {
            ok = 0;
            break;
        }
        if (j == 0) {
            x0 = b.x;
            y0 = b.y;
        }
        float *d = &row[j * 4];
        d[0] = b.x - x0;
        d[1] = b.y - y0;
        d[2] = b.z;
        d[3] = b.w;
    }
    if (!ok)
        for (int k = 0; k < in_dim; ++k) row[k] = 0.f;
    return ok;
}

} // namespace wtk
