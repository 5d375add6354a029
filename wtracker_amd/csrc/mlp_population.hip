// The per-cycle ResMLP targets of a whole POPULATION of models (E folded parameter blobs of one structure, on the device) over one track in ONE call, in
// the layout replay.hip's scan reads for WTK_REPLAY_MLP: for every (cycle c, model e) what Replay.mlp computes with model e —
// the gather front end and the forward arithmetic of mlp_kernel (mlp_forward.h: the same functions, so the same bits whatever the tiling), the float32
// clip of the prediction, the float64 corner of the first box.
//
// mlp_kernel gives every 16-sample tile a workgroup of its own, which stages the whole blob into LDS again: E x ceil(C / 16) stagings for a population.
// Here one workgroup belongs to one model and a run of tiles: the blob is staged once, and `waves` wavefronts (as many as fit next to the blob: three
// activation buffers of [16][kLdAct] each, 24.75 KiB per wave; 2 for the 105 KB blob of the 26-layer predictor, 5 for the 33 KB one, 6 when the blob is
// read from global memory) each walk `trips` tiles.  Every wave makes the same number of trips, so the barriers of mlp_forward_tile are the workgroup's; a tile
// behind the last cycle computes zero rows and stores nothing.  The layer table is built in LDS from the structure's dims, passed by value: the call
// allocates nothing.  A blob above kMlpLdsParams floats is read from global memory, as in mlp_kernel.
// A nullable stop flag (the ctrl word of a search) turns the launch into a no-op.
#include "wtk_internal.h"
#include "mlp_fold.h"
#include "mlp_forward.h"

using namespace wtk;

namespace {

constexpr int kPopMaxWaves = 8;
constexpr int kPopBufFloats = 16 * kLdAct;                  // one activation buffer
constexpr int kPopWaveFloats = 3 * kPopBufFloats;           // bufA, bufB, bufH of a wave
constexpr int kPopLdsBytes = 160 * 1024;                    // LDS of a CU: one workgroup may take all of it
constexpr int kPopTargetGroups = 512;                       // workgroups wanted in flight (256 CUs, 2 each where they fit)

struct MlpPopArgs {
    const float *blob; // [E][blob_floats]
    int blob_floats, E;
    const float *track32; // [n_track][4]
    const double *track;  // [n_track][4]
    int n_track;
    const int *anchors; // [C]
    int C;
    int input_frames[kMlpMaxInputFrames];
    int n_in;
    float bound;
    const float *bounds; // [C] (nullable: `bound` for every cycle)
    double *a, *b; // [C][E][2]
    int *valid;    // [C][E]
    const int *stop;
    int n_layers, n_blocks, layers_per_block, in_dim;
    int waves, trips, in_lds;
    unsigned char l_in[kMlpMaxLayers], l_out[kMlpMaxLayers], l_relu[kMlpMaxLayers]; // dims - 1 (1 .. 128 in a byte), relu
};

__global__ __launch_bounds__(kPopMaxWaves * 64) void mlp_population_kernel(const MlpPopArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[]; // the blob (+ 64 floats the fast path may read past it), then the waves' buffers
    __shared__ MlpLayerDev s_layers[kMlpMaxLayers];
    __shared__ int s_valid[kPopMaxWaves * 16];
    if (a.stop && *a.stop) return; // block uniform
    const int e = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, T = a.waves * 64;
    const float *gparams = a.blob + (size_t)e * a.blob_floats;
    const int n_lds = a.in_lds ? a.blob_floats + 64 : 0;
    if (a.in_lds) {
        const float4 *src4 = reinterpret_cast<const float4 *>(gparams); // blob_floats is a multiple of 4 and the base 16-byte aligned (checked by the host)
        float4 *dst4 = reinterpret_cast<float4 *>(lds);
        for (int i = tid; i < a.blob_floats / 4; i += T) dst4[i] = src4[i];
        for (int i = tid; i < 64; i += T) lds[a.blob_floats + i] = 0.f;
    }
    if (tid < a.n_layers) { // the layer table of the blob: mlp_blob_layer, offsets by a prefix sum over the dims
        int off = 0;
        for (int j = 0; j < tid; ++j) off += mlp_layer_blob_floats(a.l_in[j] + 1, a.l_out[j] + 1);
        MlpLayerDev l;
        mlp_blob_layer(l, a.l_in[tid] + 1, a.l_out[tid] + 1, a.l_relu[tid], off);
        s_layers[tid] = l;
    }
    float *bufA = lds + n_lds + wave * kPopWaveFloats, *bufB = bufA + kPopBufFloats, *bufH = bufB + kPopBufFloats;
    int *ok = s_valid + wave * 16;
    __syncthreads();

    for (int trip = 0; trip < a.trips; ++trip) {
        const int s0 = ((blockIdx.y * a.trips + trip) * a.waves + wave) * 16; // may lie behind the last cycle: zero rows, nothing stored
        for (int i = lane; i < kPopBufFloats; i += 64) bufA[i] = 0.f;
        __syncthreads();
        if (lane < 16) {
            const int s = s0 + lane;
            int v = s < a.C;
            if (v) v = mlp_gather_sample(a.track32, a.n_track, a.anchors[s], a.input_frames, a.n_in, a.in_dim, &bufA[lane * kLdAct]);
            ok[lane] = v;
        }
        __syncthreads();
        if (a.in_lds)
            mlp_forward_tile<true>(static_cast<const float *>(lds), s_layers, a.n_blocks, a.layers_per_block, bufA, bufB, bufH, lane);
        else
            mlp_forward_tile<false>(gparams, s_layers, a.n_blocks, a.layers_per_block, bufA, bufB, bufH, lane);
        if (lane < 32 && s0 + (lane >> 1) < a.C) { // lane = 2 sample + axis
            const int r = lane >> 1, k = lane & 1, s = s0 + r;
            const size_t ce = (size_t)s * a.E + e;
            // torch.clamp: min(max(x, -bound), bound) with NaN kept (fmaxf / fminf would drop it)
            const float bound = a.bounds ? a.bounds[s] : a.bound;
            float v = bufA[r * kLdAct + k];
            v = v < -bound ? -bound : v;
            v = v > bound ? bound : v;
            a.a[2 * ce + k] = ok[r] ? (double)v : 0.0;
            long long first = (long long)a.anchors[s] + a.input_frames[0];
            first = first < 0 ? 0 : (first > a.n_track - 1 ? a.n_track - 1 : first);
            a.b[2 * ce + k] = a.track[4 * first + k];
            if (k == 0) a.valid[ce] = ok[r];
        }
        __syncthreads(); // bufA and ok are free again
    }
}

// the kernel's dynamic LDS limit: what its static arrays leave of the CU's
constexpr int kPopDynBytes = kPopLdsBytes - (int)(sizeof(MlpLayerDev) * kMlpMaxLayers + sizeof(int) * kPopMaxWaves * 16);
// waves per workgroup next to `lds_floats` of parameters; 0: not even one fits
int pop_waves(int lds_floats) {
    const int w = (kPopDynBytes - lds_floats * 4) / (kPopWaveFloats * 4);
    return w < kPopMaxWaves ? w : kPopMaxWaves;
}

} // namespace

namespace {

// both forms of the entry point: one bound for every cycle, or bounds_dev [n_cycles]
int mlp_targets(const char *who, const wtk_mlp_train_layer *layers, int32_t n_layers, int32_t n_blocks, int32_t layers_per_block, const float *blob_dev, int32_t E,
                const float *track32_dev, const double *track_dev, int32_t n_track, const int32_t *anchors_dev, int32_t n_cycles, const int32_t *input_frames_host,
                int32_t n_in, float bound, const float *bounds_dev, double *a_dev, double *b_dev, int32_t *valid_dev, const int32_t *stop_dev, void *stream) {
    if (!layers || !blob_dev || !track32_dev || !track_dev || !anchors_dev || !input_frames_host || !a_dev || !b_dev || !valid_dev)
        return fail(std::string(who) + ": null argument");
    const char *why = "";
    const int64_t F = mlp_blob_layout(layers, n_layers, n_blocks, layers_per_block, nullptr, &why);
    if (F < 0) return fail(std::string(who) + ": " + why);
    if (layers[n_layers - 1].out_dim != 2) return fail(std::string(who) + ": the replay takes predictors of out_dim 2 (one predicted frame)");
    if (n_in < 1 || n_in > kMlpMaxInputFrames || n_in * 4 != layers[0].in_dim) return fail(std::string(who) + ": n_in must be in [1, 16] and n_in*4 must equal the model's input dim");
    if (E < 1 || E > 65535) return fail(std::string(who) + ": need 1 <= E <= 65535 models");
    if (n_cycles < 1 || n_track < 1) return fail(std::string(who) + ": need n_cycles >= 1 and n_track >= 1");
    if (reinterpret_cast<uintptr_t>(blob_dev) % 16 || reinterpret_cast<uintptr_t>(track32_dev) % 16) return fail(std::string(who) + ": blob and float32 track must be 16-byte aligned");
    MlpPopArgs a = {};
    a.blob = blob_dev, a.blob_floats = (int)F, a.E = E, a.track32 = track32_dev, a.track = track_dev, a.n_track = n_track, a.anchors = anchors_dev, a.C = n_cycles;
    for (int i = 0; i < kMlpMaxInputFrames; ++i) a.input_frames[i] = i < n_in ? input_frames_host[i] : 0;
    a.n_in = n_in, a.bound = bound, a.bounds = bounds_dev, a.a = a_dev, a.b = b_dev, a.valid = valid_dev, a.stop = stop_dev;
    a.n_layers = n_layers, a.n_blocks = n_blocks, a.layers_per_block = layers_per_block, a.in_dim = layers[0].in_dim;
    for (int i = 0; i < n_layers; ++i) a.l_in[i] = (unsigned char)(layers[i].in_dim - 1), a.l_out[i] = (unsigned char)(layers[i].out_dim - 1), a.l_relu[i] = layers[i].relu ? 1 : 0;
    a.in_lds = F <= kMlpLdsParams;
    const int lds_floats = a.in_lds ? (int)F + 64 : 0;
    const int tiles = (n_cycles + 15) / 16;
    int waves = pop_waves(lds_floats);
    if (waves < 1) return fail(std::string(who) + ": the blob leaves no room for a wave's buffers in LDS"); // (cannot happen below kMlpLdsParams)
    if (waves > tiles) waves = tiles;
    // groups of tiles per model: enough workgroups to fill the device, no more than there are runs of `waves` tiles
    int groups = (kPopTargetGroups + E - 1) / E;
    const int max_groups = (tiles + waves - 1) / waves;
    if (groups > max_groups) groups = max_groups;
    a.trips = (tiles + groups * waves - 1) / (groups * waves);
    groups = (tiles + a.trips * waves - 1) / (a.trips * waves);
    a.waves = waves;
    const size_t dyn = ((size_t)lds_floats + (size_t)waves * kPopWaveFloats) * sizeof(float);
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&mlp_population_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kPopDynBytes));
    hipLaunchKernelGGL(mlp_population_kernel, dim3((unsigned)E, (unsigned)groups), dim3(waves * 64), dyn, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

} // namespace

extern "C" int wtk_replay_mlp_targets(const wtk_mlp_train_layer *layers, int32_t n_layers, int32_t n_blocks, int32_t layers_per_block, const float *blob_dev, int32_t E,
                                      const float *track32_dev, const double *track_dev, int32_t n_track, const int32_t *anchors_dev, int32_t n_cycles,
                                      const int32_t *input_frames_host, int32_t n_in, float bound, double *a_dev, double *b_dev, int32_t *valid_dev,
                                      const int32_t *stop_dev, void *stream) {
    return mlp_targets("wtk_replay_mlp_targets", layers, n_layers, n_blocks, layers_per_block, blob_dev, E, track32_dev, track_dev, n_track, anchors_dev, n_cycles,
                       input_frames_host, n_in, bound, nullptr, a_dev, b_dev, valid_dev, stop_dev, stream);
}

extern "C" int wtk_replay_mlp_targets_bounds(const wtk_mlp_train_layer *layers, int32_t n_layers, int32_t n_blocks, int32_t layers_per_block, const float *blob_dev,
                                             int32_t E, const float *track32_dev, const double *track_dev, int32_t n_track, const int32_t *anchors_dev,
                                             int32_t n_cycles, const int32_t *input_frames_host, int32_t n_in, const float *bounds_dev, double *a_dev,
                                             double *b_dev, int32_t *valid_dev, const int32_t *stop_dev, void *stream) {
    if (!bounds_dev) return fail("wtk_replay_mlp_targets_bounds: null argument");
    return mlp_targets("wtk_replay_mlp_targets_bounds", layers, n_layers, n_blocks, layers_per_block, blob_dev, E, track32_dev, track_dev, n_track, anchors_dev,
                       n_cycles, input_frames_host, n_in, 0.f, bounds_dev, a_dev, b_dev, valid_dev, stop_dev, stream);
}

extern "C" int32_t wtk_replay_mlp_targets_waves(int64_t blob_floats) {
    if (blob_floats < 0) return -1;
    return pop_waves(blob_floats <= kMlpLdsParams ? (int)blob_floats + 64 : 0);
}
