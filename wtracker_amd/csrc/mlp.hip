// ResMLP trajectory predictor (wtracker/neural/mlp.py:144-188, eval mode) as small exact-fp32
// MFMA GEMMs.  One wavefront owns 16 samples; every Linear(+folded BatchNorm1d)+ReLU is
// D[16 samples x 16 outs] += X[16 x 4] * W^T[4 x 16] with v_mfma_f32_16x16x4_f32, which is
// bit-for-bit a k-ordered fp32 fma chain, so results stay within the reference's own
// batch-size variance (abs 2e-4 + rel 1e-5).  Activations ping-pong between two
// LDS buffers; the residual stream h lives in a third (h <- h + block(h), mlp.py:185-187).
// The whole parameter blob (33 KB / 105 KB for the two shipped predictors) and the layer table are copied
// into LDS first: the kernel is one dependent chain of ~20 tiny GEMMs, and fetching each weight element from
// global memory inside that chain cost ~10 % of a call (59 -> 54 us for the 26-layer predictor; the rest is the
// dependent MFMA / LDS / barrier chain itself: interleaving several output tiles per layer measured slower, 54 -> 70 us).
//
// The optional gather front-end is the batched form of MLPController.provide_movement_vector
// (wtracker/sim/sim_controllers/mlp_controllers.py:38-56): 7 boxes of the track at
// anchor + input_frames, NaN / out-of-range guard, x/y made relative to the first box's corner.
#include "mlp_forward.h"

namespace wtk {

__global__ __launch_bounds__(64) void mlp_kernel(const MlpArgs a) {
    __shared__ float bufA[16 * kLdAct];
    __shared__ float bufB[16 * kLdAct];
    __shared__ float bufH[16 * kLdAct];
    __shared__ int s_valid[16];
    __shared__ __attribute__((aligned(16))) float wlds[kMlpLdsParams + 64];
    __shared__ MlpLayerDev s_layers[kMlpMaxLayers];
    const int lane = threadIdx.x;
    const int s0 = blockIdx.x * 16;
    const bool in_lds = a.n_params <= kMlpLdsParams; // block uniform
    if (in_lds) {
        const float4 *src4 = reinterpret_cast<const float4 *>(a.params); // hipMalloc'd: 16-byte aligned; blob padded to 4 floats
        float4 *dst4 = reinterpret_cast<float4 *>(wlds);
        for (int i = lane; i < (a.n_params + 3) / 4; i += 64) dst4[i] = src4[i];
    }
    for (int i = lane; i < a.n_layers * (int)(sizeof(MlpLayerDev) / sizeof(int)); i += 64)
        reinterpret_cast<int *>(s_layers)[i] = reinterpret_cast<const int *>(a.layers)[i];

    // ---- stage the 16 input rows (zero-padded) into bufA
    for (int i = lane; i < 16 * kLdAct; i += 64) bufA[i] = 0.f;
    __syncthreads();
    if (a.x) {
        for (int i = lane; i < 16 * a.in_dim; i += 64) {
            const int s = i / a.in_dim, k = i - s * a.in_dim;
            if (s0 + s < a.B) bufA[s * kLdAct + k] = a.x[(long long)(s0 + s) * a.in_dim + k];
        }
    } else {
        if (lane < 16) {
            const int s = s0 + lane;
            int ok = s < a.B;
            if (ok) ok = mlp_gather_sample(a.track, a.n_frames, a.anchor_frames[s], a.input_frames, a.n_in, a.in_dim, &bufA[lane * kLdAct]);
            s_valid[lane] = ok;
        }
    }
    __syncthreads();

    if (in_lds)
        mlp_forward_tile<true>(static_cast<const float *>(wlds), s_layers, a.n_blocks, a.layers_per_block, bufA, bufB, bufH, lane);
    else
        mlp_forward_tile<false>(a.params, s_layers, a.n_blocks, a.layers_per_block, bufA, bufB, bufH, lane);
    for (int i = lane; i < 16 * a.out_dim; i += 64) {
        const int s = i / a.out_dim, k = i - s * a.out_dim;
        if (s0 + s < a.B) {
            float v = bufA[s * kLdAct + k];
            if (!a.x && !s_valid[s]) v = 0.f;
            a.y[(long long)(s0 + s) * a.out_dim + k] = v;
        }
    }
    if (!a.x && a.valid && lane < 16 && s0 + lane < a.B) a.valid[s0 + lane] = s_valid[lane];
}

hipError_t launch_mlp(const MlpArgs &a, hipStream_t stream) {
    if (a.B <= 0) return hipSuccess;
    if (a.in_dim > kMlpMaxDim || a.out_dim > kMlpMaxDim) return hipErrorInvalidValue;
    if (a.n_layers != 2 + a.n_blocks * a.layers_per_block || a.n_layers > kMlpMaxLayers) return hipErrorInvalidValue;
    if (!a.x && (a.n_in <= 0 || a.n_in > kMlpMaxInputFrames || a.n_in * 4 != a.in_dim)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mlp_kernel, dim3((a.B + 15) / 16), dim3(64), 0, stream, a);
    return hipGetLastError();
}

} // namespace wtk
