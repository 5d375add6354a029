// Training of the ResMLP predictor (wtracker/neural/training.py:267-333, MLPTrainer over RMLP in train mode, wtracker/neural/mlp.py:51-188):
// a POPULATION of E models of one structure, one workgroup per model (blockIdx.x = e).  A workgroup never waits for another one, there is no grid-wide
// barrier and no cooperative launch; every loop runs to a bound the host validated.
//
// One batch = gather -> forward (train mode: batch statistics) -> loss -> backward -> optimizer step.  Every matrix product is the exact-fp32 MFMA of
// mlp.hip (v_mfma_f32_16x16x4_f32, a k-ordered fma chain): a wave owns whole 16 x 16 output tiles and walks K in ascending order, so
//   forward   z  = a W^T      K = the layer's inputs
//   dW        = dz^T a        K = the batch's samples, ascending
//   dx        = dz W          K = the layer's outputs
// need no cross-wave reduction, and the BatchNorm / bias / loss sums over the samples are taken in a fixed two-level order (chan_sums in the kernel).
// A model's bits therefore depend on nothing but its own parameters, data, order and hyper-parameters: not on E, its index, its neighbours or the run.
//
// The unfolded parameter set ("state": per layer W, b, [gamma, beta]; then per BatchNorm running_mean, running_var) stays in LDS for the whole launch while
// it fits kTrainLdsFloats (the notebook's model: 35 488 floats = 139 KiB of 160 KiB) and is read and updated in global memory above that; both paths run
// the same code through flat pointers, so they give the same bits.  Operand loads are masked (row, column and k bounds), so no buffer needs padding and no
// load leaves its allocation.  Activations saved for backward, gradients and optimizer moments live in per-model global scratch owned by the handle.
#include "wtk_internal.h"

#include <cmath>
#include <string>
#include <vector>

namespace wtk {

typedef float floatx4 __attribute__((ext_vector_type(4)));

constexpr int kTrainLd = kMlpMaxDim;       // row stride (floats) of every activation buffer
constexpr int kTrainThreads = 1024;        // one workgroup = 16 waves
constexpr int kTrainMaxBatch = 1024;       // samples of one batch (the loss partials are one per thread)
constexpr int kTrainLdsFloats = 36864;     // 144 KiB of parameters in LDS; ~14 KiB of static LDS next to them
constexpr float kBnEps = 1e-5f, kBnMomentum = 0.1f;
enum { TRAIN_STEP = 0, TRAIN_GRAD = 1, TRAIN_EVAL = 2 };
enum { LOSS_MSE = 0, LOSS_L1 = 1 };
enum { OPT_ADAM = 0, OPT_ADAMW = 1, OPT_SGD = 2, OPT_RMSPROP = 3 };
enum { BUF_X = 0, BUF_Y = 1, BUF_DH = 2, BUF_DZ = 3, BUF_DX = 4, BUF_FIRST_ACT = 5 };

struct MlpTrainLayerDev {
    int in_dim, out_dim, relu, bn;
    int w_off, b_off, g_off, be_off; // float offsets in the state: trainable section
    int rm_off, rv_off;              // ... and in the buffer section behind it (bn only)
    int pad_[2];
};

struct MlpTrainArgs {
    float *state, *best;      // [E][n_state]
    float *grad;              // [E][n_train]
    float *m, *v;             // [E][n_train] optimizer moments
    float *scratch;           // [E][scratch_floats]
    int *steps, *best_steps;  // [E] optimizer steps taken (= batches trained), and the count at the best state
    float *best_loss;         // [E] early stopping (training.py:119-128)
    int *has_best, *no_improve;
    const MlpTrainLayerDev *layers;
    int n_layers, n_blocks, layers_per_block, n_state, n_train, max_batch;
    long long scratch_floats;
    int loss_kind, opt_kind, in_dim, out_dim;
    int use_lds;
    // the call
    int mode;
    const float *x, *y; // [n][in_dim], [n][out_dim]
    const int *order;   // [E][n] sample order of each model, or null: 0 .. n - 1
    int n, batch_size, n_batches;
    const double *lr, *wd; // [E]
    int *active;           // [E] or null
    float *loss_out;       // [E][n_batches]
    int *nc_out;           // [E][n_batches]
    float *pred_out;       // TRAIN_EVAL: [E][n][out_dim] or null
    int patience;          // TRAIN_EVAL: > 0 clears active[e] after this many epochs without improvement
    int reset_best;        // TRAIN_EVAL: forget the early-stopping state of earlier epochs first
};

// One 16 x 16 tile of D = A B, D[m][n] = sum_{k < K} A(m, k) B(k, n) in ascending k: A(m, k) = A[m * a_rs + k * a_ks], B(k, n) = B[k * b_ks + n * b_cs].
// Loads outside m < M, n < N, k < K are replaced by 0 (their address is clamped to element 0 of the row / column).  The lane holds D[m0 + 4 g + i][n0 + r].
__device__ __forceinline__ floatx4 train_tile(const float *A, int a_rs, int a_ks, int M, const float *B, int b_ks, int b_cs, int N, int K, int m0, int n0, int lane) {
    const int r = lane & 15, g = lane >> 4;
    const bool a_ok = m0 + r < M, b_ok = n0 + r < N;
    const float *ap = A + (size_t)(a_ok ? m0 + r : 0) * a_rs;
    const float *bp = B + (size_t)(b_ok ? n0 + r : 0) * b_cs;
    floatx4 acc = {0.f, 0.f, 0.f, 0.f};
    // the operands of four k steps are fetched before their MFMAs (eight loads in flight instead of a load -> wait -> MFMA round trip per step); same k order
    for (int k0 = 0; k0 < K; k0 += 16) {
        float av[4], bv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = k0 + 4 * u + g;
            const bool k_ok = k < K;
            const int kc = k_ok ? k : 0;
            const float x = ap[(size_t)kc * a_ks], w = bp[(size_t)kc * b_ks];
            av[u] = (a_ok && k_ok) ? x : 0.f;
            bv[u] = (b_ok && k_ok) ? w : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (k0 + 4 * u < K) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bv[u], acc, 0, 0, 0);
    }
    return acc;
}

__global__ __launch_bounds__(kTrainThreads) void mlp_train_kernel(const MlpTrainArgs a) {
    extern __shared__ __attribute__((aligned(16))) float wlds[];
    __shared__ MlpTrainLayerDev s_layers[kMlpMaxLayers];
    __shared__ float s_part[kTrainMaxBatch];
    __shared__ int s_flag[kTrainMaxBatch];
    __shared__ float s_part2[64];
    __shared__ int s_flag2[64];
    __shared__ float s_c0[kMlpMaxDim], s_c1[kMlpMaxDim];
    __shared__ double s_opt[4];
    __shared__ int s_improved;
    const int e = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int T = kTrainThreads, kWaves = kTrainThreads / 64;
    if (a.active && a.active[e] == 0) return; // block uniform: a stopped model costs nothing

    float *gstate = a.state + (size_t)e * a.n_state;
    float *P = a.use_lds ? wlds : gstate;
    if (a.use_lds)
        for (int i = tid; i < a.n_state; i += T) wlds[i] = gstate[i];
    for (int i = tid; i < a.n_layers * (int)(sizeof(MlpTrainLayerDev) / sizeof(int)); i += T)
        reinterpret_cast<int *>(s_layers)[i] = reinterpret_cast<const int *>(a.layers)[i];

    float *S = a.scratch + (size_t)e * a.scratch_floats;
    const size_t bsz = (size_t)a.max_batch * kTrainLd;
    const int nl = a.n_layers, lpb = a.layers_per_block;
    auto buf = [&](int k) { return S + (size_t)k * bsz; };
    auto act = [&](int i) { return buf(BUF_FIRST_ACT + i); };          // output of layer i (after BatchNorm and ReLU)
    auto xhat = [&](int i) { return buf(BUF_FIRST_ACT + nl + i); };    // z, then x^ of a BatchNorm layer
    auto hres = [&](int b) { return b == 0 ? act(0) : buf(BUF_FIRST_ACT + 2 * nl + b - 1); }; // residual stream in front of block b
    auto input_of = [&](int i) { return i == 0 ? buf(BUF_X) : (i == nl - 1 ? hres(a.n_blocks) : ((i - 1) % lpb == 0 ? hres((i - 1) / lpb) : act(i - 1))); };
    float *stat = S + (size_t)(BUF_FIRST_ACT + 2 * nl + a.n_blocks) * bsz; // [n_layers][kMlpMaxDim] 1 / sqrt(var + eps) of the batch
    float *XB = buf(BUF_X), *YB = buf(BUF_Y), *DH = buf(BUF_DH), *DZ = buf(BUF_DZ), *DX = buf(BUF_DX);
    float *G = a.grad ? a.grad + (size_t)e * a.n_train : nullptr;
    float *Mo = a.m ? a.m + (size_t)e * a.n_train : nullptr, *Vo = a.v ? a.v + (size_t)e * a.n_train : nullptr;
    const bool train = a.mode != TRAIN_EVAL;
    // chan_sums: a sum over the batch's samples per channel is taken by kChanParts threads per channel — thread (part j, channel c) adds samples j, j + 8, ...
    // in ascending order — and the kChanParts partial sums are added in the order j = 0 .. 7: a fixed order, whatever E is
    constexpr int kChanParts = kTrainThreads / kMlpMaxDim;
    const int cch = tid & (kMlpMaxDim - 1), cpart = tid / kMlpMaxDim;
    float *s_part1 = reinterpret_cast<float *>(s_flag); // second partial-sum array (the loss phase's flags are not live then)
    auto chan_total = [&](const float *part, int c) {
        float t = 0.f;
#pragma unroll
        for (int j = 0; j < kChanParts; ++j) t += part[j * kMlpMaxDim + c];
        return t;
    };
    int step_t = a.steps[e];
    float eval_sum = 0.f; // thread 0: fp32 sum of the batch losses of an eval epoch, in batch order
    __syncthreads();

    for (int bi = 0; bi < a.n_batches; ++bi) {
        const int b0 = bi * a.batch_size;
        const int B = min(a.batch_size, a.n - b0);
        // ---- optimizer scalars of this step (torch computes them in double on the host) and the batch's rows
        if (tid == 0 && a.mode == TRAIN_STEP) {
            const double lr = a.lr[e], t = (double)(step_t + 1);
            if (a.opt_kind == OPT_ADAM || a.opt_kind == OPT_ADAMW) {
                const double bc1 = 1.0 - pow(0.9, t), bc2 = 1.0 - pow(0.999, t);
                s_opt[0] = lr / bc1;  // step_size
                s_opt[1] = sqrt(bc2); // bias_correction2_sqrt
            } else {
                s_opt[0] = lr;
                s_opt[1] = 1.0;
            }
            s_opt[2] = a.wd[e];
            s_opt[3] = 1.0 - lr * a.wd[e]; // adamw: decoupled decay
        }
        for (int i = tid; i < B * a.in_dim; i += T) {
            const int s = i / a.in_dim, k = i - s * a.in_dim;
            int row = a.order ? a.order[(size_t)e * a.n + b0 + s] : b0 + s;
            row = min(max(row, 0), a.n - 1);
            XB[s * kTrainLd + k] = a.x[(size_t)row * a.in_dim + k];
        }
        for (int i = tid; i < B * a.out_dim; i += T) {
            const int s = i / a.out_dim, k = i - s * a.out_dim;
            int row = a.order ? a.order[(size_t)e * a.n + b0 + s] : b0 + s;
            row = min(max(row, 0), a.n - 1);
            YB[s * kTrainLd + k] = a.y[(size_t)row * a.out_dim + k];
        }
        __syncthreads();

        // ---- forward
        for (int i = 0; i < nl; ++i) {
            const MlpTrainLayerDev L = s_layers[i];
            const float *in = input_of(i);
            const float *W = P + L.w_off;
            const bool bn_batch = L.bn && train; // batch statistics: z goes to xhat(i) first
            float *zdst = bn_batch ? xhat(i) : act(i);
            const int tm = (B + 15) / 16, tn = (L.out_dim + 15) / 16;
            for (int t = wave; t < tm * tn; t += kWaves) {
                const int m0 = (t / tn) * 16, n0 = (t % tn) * 16;
                const floatx4 acc = train_tile(in, kTrainLd, 1, B, W, 1, L.in_dim, L.out_dim, L.in_dim, m0, n0, lane);
                const int o = n0 + (lane & 15);
                if (o < L.out_dim) {
                    const float bias = P[L.b_off + o];
                    float sc = 1.f, sh = 0.f, mu = 0.f, ga = 1.f;
                    if (L.bn && !train) { // eval: running statistics, in the order of the reference's modules
                        mu = P[L.rm_off + o];
                        sc = sqrtf(P[L.rv_off + o] + kBnEps);
                        ga = P[L.g_off + o];
                        sh = P[L.be_off + o];
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int s = m0 + 4 * (lane >> 4) + j;
                        if (s < B) {
                            float v = acc[j] + bias;
                            if (L.bn && !train) v = (v - mu) / sc * ga + sh;
                            if (!bn_batch && L.relu) v = fmaxf(v, 0.f);
                            zdst[s * kTrainLd + o] = v;
                        }
                    }
                }
            }
            __syncthreads();
            if (bn_batch) {
                float *Z = xhat(i);
                // mean, then the biased variance around it: kChanParts threads per channel (chan_sums)
                {
                    float p = 0.f;
                    if (cch < L.out_dim)
                        for (int s = cpart; s < B; s += kChanParts) p += Z[s * kTrainLd + cch];
                    s_part[cpart * kMlpMaxDim + cch] = p;
                }
                __syncthreads();
                const float mean = chan_total(s_part, cch) / (float)B; // every thread of a channel adds the same partial sums in the same order
                __syncthreads();
                {
                    float p = 0.f;
                    if (cch < L.out_dim)
                        for (int s = cpart; s < B; s += kChanParts) {
                            const float d = Z[s * kTrainLd + cch] - mean;
                            p += d * d;
                        }
                    s_part[cpart * kMlpMaxDim + cch] = p;
                }
                __syncthreads();
                if (tid < L.out_dim) {
                    const float sq = chan_total(s_part, tid);
                    const float var = sq / (float)B;
                    const float inv = 1.f / sqrtf(var + kBnEps);
                    s_c0[tid] = mean;
                    s_c1[tid] = inv;
                    stat[i * kMlpMaxDim + tid] = inv;
                    if (a.mode == TRAIN_STEP) { // running_var takes the unbiased variance (torch.nn.BatchNorm1d)
                        const float unb = sq / (float)(B - 1);
                        P[L.rm_off + tid] = (1.f - kBnMomentum) * P[L.rm_off + tid] + kBnMomentum * mean;
                        P[L.rv_off + tid] = (1.f - kBnMomentum) * P[L.rv_off + tid] + kBnMomentum * unb;
                    }
                }
                __syncthreads();
                float *Aout = act(i);
                for (int idx = tid; idx < B * L.out_dim; idx += T) {
                    const int s = idx / L.out_dim, o = idx - s * L.out_dim;
                    const float xh = (Z[s * kTrainLd + o] - s_c0[o]) * s_c1[o];
                    Z[s * kTrainLd + o] = xh;
                    float v = xh * P[L.g_off + o] + P[L.be_off + o];
                    if (L.relu) v = fmaxf(v, 0.f);
                    Aout[s * kTrainLd + o] = v;
                }
                __syncthreads();
            }
            if (i >= 1 && i < nl - 1 && (i - 1) % lpb == lpb - 1) { // h <- h + block(h)
                const int b = (i - 1) / lpb;
                const float *h0 = hres(b), *blk = act(i);
                float *h1 = hres(b + 1);
                for (int idx = tid; idx < B * L.out_dim; idx += T) {
                    const int s = idx / L.out_dim, o = idx - s * L.out_dim;
                    h1[s * kTrainLd + o] = h0[s * kTrainLd + o] + blk[s * kTrainLd + o];
                }
                __syncthreads();
            }
        }

        // ---- loss, num_correct (training.py:317) and the gradient of the loss into DZ
        {
            const float *Pr = act(nl - 1);
            const float inv_n = 1.f / (float)(B * a.out_dim);
            if (tid < B) {
                float sum = 0.f, n2 = 0.f;
                for (int o = 0; o < a.out_dim; ++o) {
                    const float d = Pr[tid * kTrainLd + o] - YB[tid * kTrainLd + o];
                    n2 += d * d;
                    sum += a.loss_kind == LOSS_MSE ? d * d : fabsf(d);
                    if (train) DZ[tid * kTrainLd + o] = a.loss_kind == LOSS_MSE ? 2.f * d * inv_n : (d > 0.f ? inv_n : (d < 0.f ? -inv_n : 0.f));
                }
                s_part[tid] = sum;
                s_flag[tid] = sqrtf(n2) < 1.0f ? 1 : 0;
                if (a.pred_out)
                    for (int o = 0; o < a.out_dim; ++o) {
                        int row = a.order ? a.order[(size_t)e * a.n + b0 + tid] : b0 + tid;
                        row = min(max(row, 0), a.n - 1);
                        a.pred_out[((size_t)e * a.n + row) * a.out_dim + o] = Pr[tid * kTrainLd + o];
                    }
            }
            __syncthreads();
            if (tid < 64) { // fixed two-level order: 64 runs of 16 samples, then the 64 partial sums
                float sum = 0.f;
                int cnt = 0;
                for (int j = 0; j < 16; ++j) {
                    const int s = tid * 16 + j;
                    if (s < B) {
                        sum += s_part[s];
                        cnt += s_flag[s];
                    }
                }
                s_part2[tid] = sum;
                s_flag2[tid] = cnt;
            }
            __syncthreads();
            if (tid == 0) {
                float sum = 0.f;
                int cnt = 0;
                for (int j = 0; j < 64; ++j) {
                    sum += s_part2[j];
                    cnt += s_flag2[j];
                }
                const float loss = sum * inv_n;
                a.loss_out[(size_t)e * a.n_batches + bi] = loss;
                if (a.nc_out) a.nc_out[(size_t)e * a.n_batches + bi] = cnt;
                eval_sum += loss;
            }
        }
        if (!train) {
            __syncthreads();
            continue;
        }

        // ---- backward: layer i turns the gradient of its output (src) into dz (DZ), then into dW, db and the gradient of its input
        for (int i = nl - 1; i >= 0; --i) {
            const MlpTrainLayerDev L = s_layers[i];
            const bool is_out = i == nl - 1, is_in = i == 0;
            const int l_in_block = (is_out || is_in) ? -1 : (i - 1) % lpb;
            if (!is_out) {
                const float *src = (is_in || l_in_block == lpb - 1) ? DH : DX;
                const float *Aout = act(i);
                if (L.bn) {
                    const float *Xh = xhat(i);
                    {
                        float pg = 0.f, pb = 0.f;
                        if (cch < L.out_dim)
                            for (int s = cpart; s < B; s += kChanParts) {
                                float d = src[s * kTrainLd + cch];
                                if (L.relu && !(Aout[s * kTrainLd + cch] > 0.f)) d = 0.f;
                                pg += d * Xh[s * kTrainLd + cch];
                                pb += d;
                            }
                        s_part[cpart * kMlpMaxDim + cch] = pg;
                        s_part1[cpart * kMlpMaxDim + cch] = pb;
                    }
                    __syncthreads();
                    if (tid < L.out_dim) {
                        const float dg = chan_total(s_part, tid), db = chan_total(s_part1, tid);
                        G[L.g_off + tid] = dg;
                        G[L.be_off + tid] = db;
                        s_c0[tid] = dg;
                        s_c1[tid] = db;
                    }
                    __syncthreads();
                    const float fB = (float)B;
                    for (int idx = tid; idx < B * L.out_dim; idx += T) {
                        const int s = idx / L.out_dim, o = idx - s * L.out_dim;
                        float d = src[s * kTrainLd + o];
                        if (L.relu && !(Aout[s * kTrainLd + o] > 0.f)) d = 0.f;
                        const float k = P[L.g_off + o] * stat[i * kMlpMaxDim + o] / fB;
                        DZ[s * kTrainLd + o] = k * (fB * d - s_c1[o] - Xh[s * kTrainLd + o] * s_c0[o]);
                    }
                } else {
                    for (int idx = tid; idx < B * L.out_dim; idx += T) {
                        const int s = idx / L.out_dim, o = idx - s * L.out_dim;
                        float d = src[s * kTrainLd + o];
                        if (L.relu && !(Aout[s * kTrainLd + o] > 0.f)) d = 0.f;
                        DZ[s * kTrainLd + o] = d;
                    }
                }
                __syncthreads();
            }
            const float *in = input_of(i);
            const float *W = P + L.w_off;
            const int to = (L.out_dim + 15) / 16, tk = (L.in_dim + 15) / 16, tm = (B + 15) / 16;
            const int n_dw = to * tk, n_dx = is_in ? 0 : tm * tk;
            { // db[o] = sum_s dz[s][o] (chan_sums); its totals are added while the tile loop runs
                float p = 0.f;
                if (cch < L.out_dim)
                    for (int s = cpart; s < B; s += kChanParts) p += DZ[s * kTrainLd + cch];
                s_part[cpart * kMlpMaxDim + cch] = p;
            }
            __syncthreads();
            if (tid < L.out_dim) G[L.b_off + tid] = chan_total(s_part, tid);
            for (int t = wave; t < n_dw + n_dx; t += kWaves) {
                if (t < n_dw) { // dW[o][k] = sum_s dz[s][o] a[s][k]
                    const int m0 = (t / tk) * 16, n0 = (t % tk) * 16;
                    const floatx4 acc = train_tile(DZ, 1, kTrainLd, L.out_dim, in, kTrainLd, 1, L.in_dim, B, m0, n0, lane);
                    const int k = n0 + (lane & 15);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int o = m0 + 4 * (lane >> 4) + j;
                        if (o < L.out_dim && k < L.in_dim) G[L.w_off + o * L.in_dim + k] = acc[j];
                    }
                } else { // dx[s][k] = sum_o dz[s][o] W[o][k]
                    const int u = t - n_dw;
                    const int m0 = (u / tk) * 16, n0 = (u % tk) * 16;
                    const floatx4 acc = train_tile(DZ, kTrainLd, 1, B, W, L.in_dim, 1, L.in_dim, L.out_dim, m0, n0, lane);
                    const int k = n0 + (lane & 15);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int s = m0 + 4 * (lane >> 4) + j;
                        if (s < B && k < L.in_dim) {
                            if (is_out)
                                DH[s * kTrainLd + k] = acc[j];
                            else if (l_in_block == 0)
                                DH[s * kTrainLd + k] += acc[j]; // the residual sum: dh = dh + d(block input)
                            else
                                DX[s * kTrainLd + k] = acc[j];
                        }
                    }
                }
            }
            __syncthreads();
        }
        if (a.mode == TRAIN_GRAD) continue;

        // ---- optimizer step (torch.optim defaults but lr and weight_decay: neural/config.py:28-33)
        {
            const float step_size = (float)s_opt[0], bc2s = (float)s_opt[1], wd = (float)s_opt[2], decay = (float)s_opt[3], lr = (float)s_opt[0];
            for (int i = tid; i < a.n_train; i += T) {
                float p = P[i], g = G[i];
                if (a.opt_kind == OPT_ADAMW) {
                    p = p * decay;
                } else if (wd != 0.f) {
                    // grad.add(param, alpha = weight_decay) is ONE fma in torch.  Where g ~ -wd p the sum cancels, and the second rounding of a separate
                    // multiply (half a unit in the last place of wd p, any fraction of what is left) is what Adam / RMSprop then normalise into the step
                    g = fmaf(wd, p, g);
                }
                if (a.opt_kind == OPT_ADAM || a.opt_kind == OPT_ADAMW) {
                    float m = Mo[i], v = Vo[i];
                    m = m + (g - m) * 0.1f;               // exp_avg.lerp_(grad, 1 - beta1)
                    v = v * 0.999f + (0.001f * g) * g;     // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
                    Mo[i] = m;
                    Vo[i] = v;
                    const float denom = sqrtf(v) / bc2s + 1e-8f;
                    p = p - step_size * (m / denom);
                } else if (a.opt_kind == OPT_SGD) {
                    p = p - lr * g;
                } else { // rmsprop: alpha 0.99, eps 1e-8, no momentum, not centered
                    float v = Vo[i];
                    v = v * 0.99f + (0.01f * g) * g;
                    Vo[i] = v;
                    p = p - lr * (g / (sqrtf(v) + 1e-8f));
                }
                P[i] = p;
            }
            step_t += 1;
            __syncthreads();
        }
    }

    if (a.mode == TRAIN_STEP) {
        if (a.use_lds)
            for (int i = tid; i < a.n_state; i += T) gstate[i] = wlds[i];
        if (tid == 0) a.steps[e] = step_t;
    } else if (a.mode == TRAIN_EVAL && a.best) {
        // early stopping, training.py:119-128: curr = fp32 sum of the batch losses in batch order / n_batches, strict <, the best state kept on the device
        if (tid == 0) {
            const float curr = eval_sum / (float)a.n_batches;
            if (a.reset_best) a.has_best[e] = 0, a.no_improve[e] = 0; // the first test epoch of a fit: best_val_loss = None
            int improved = 0;
            if (!a.has_best[e] || curr < a.best_loss[e]) {
                a.best_loss[e] = curr;
                a.has_best[e] = 1;
                a.no_improve[e] = 0;
                a.best_steps[e] = step_t;
                improved = 1;
            } else {
                const int k = a.no_improve[e] + 1;
                a.no_improve[e] = k;
                if (a.patience > 0 && k >= a.patience && a.active) a.active[e] = 0;
            }
            s_improved = improved;
        }
        __syncthreads();
        if (s_improved) {
            float *bst = a.best + (size_t)e * a.n_state;
            for (int i = tid; i < a.n_state; i += T) bst[i] = P[i];
        }
    }
}

} // namespace wtk

// =====================================================================================================================================================
// C ABI
// =====================================================================================================================================================
using namespace wtk;

struct wtk_mlp_trainer {
    int device = 0;
    int n_models = 0, n_layers = 0, n_blocks = 0, layers_per_block = 0, max_batch = 0;
    int n_state = 0, n_train = 0, any_bn = 0;
    long long scratch_floats = 0;
    MlpTrainArgs base{};
    std::vector<void *> allocs;
};

static int trainer_alloc(wtk_mlp_trainer *h, void **p, size_t bytes, bool zero) {
    HIP_TRY(hipMalloc(p, bytes ? bytes : 4));
    h->allocs.push_back(*p);
    if (zero) HIP_TRY(hipMemset(*p, 0, bytes ? bytes : 4));
    return 0;
}

extern "C" int64_t wtk_mlp_trainer_state_floats(const wtk_mlp_trainer_desc *d, int64_t *n_train_out) {
    if (!d || !d->layers || d->n_layers <= 0) return -1;
    int64_t n_train = 0, n_buf = 0;
    for (int i = 0; i < d->n_layers; ++i) {
        const wtk_mlp_train_layer &s = d->layers[i];
        n_train += (int64_t)s.out_dim * s.in_dim + s.out_dim + (s.batch_norm ? 2 * s.out_dim : 0);
        n_buf += s.batch_norm ? 2 * s.out_dim : 0;
    }
    if (n_train_out) *n_train_out = n_train;
    return n_train + n_buf;
}

extern "C" void wtk_mlp_trainer_destroy(wtk_mlp_trainer *h) {
    if (!h) return;
    for (void *p : h->allocs) (void)hipFree(p);
    delete h;
}

extern "C" int wtk_mlp_trainer_create(wtk_mlp_trainer **out, const wtk_mlp_trainer_desc *d) {
    const char *who = "wtk_mlp_trainer_create";
    if (!out || !d || !d->layers || !d->state) return fail(std::string(who) + ": null argument");
    if (d->n_models <= 0) return fail(std::string(who) + ": n_models must be positive");
    if (d->n_layers > kMlpMaxLayers) return fail(std::string(who) + ": more than kMlpMaxLayers = 64 layers");
    if (d->n_blocks < 0 || (d->n_blocks > 0 && d->layers_per_block <= 0) || d->n_layers != 2 + d->n_blocks * d->layers_per_block)
        return fail(std::string(who) + ": n_layers != 2 + n_blocks * layers_per_block");
    if (d->loss != LOSS_MSE && d->loss != LOSS_L1) return fail(std::string(who) + ": loss must be mse (0) or l1 (1)");
    if (d->optimizer < OPT_ADAM || d->optimizer > OPT_RMSPROP) return fail(std::string(who) + ": optimizer must be adam (0), adamw (1), sgd (2) or rmsprop (3)");
    if (d->max_batch < 1 || d->max_batch > kTrainMaxBatch) return fail(std::string(who) + ": batch_size must be in [1, 1024]");
    std::vector<MlpTrainLayerDev> L(d->n_layers);
    int off = 0, any_bn = 0;
    for (int i = 0; i < d->n_layers; ++i) {
        const wtk_mlp_train_layer &s = d->layers[i];
        if (s.in_dim <= 0 || s.out_dim <= 0 || s.in_dim > kMlpMaxDim || s.out_dim > kMlpMaxDim) return fail(std::string(who) + ": layer width outside [1, kMlpMaxDim = 128]");
        if (s.relu != 0 && s.relu != 1) return fail(std::string(who) + ": activation must be ReLU (1) or none (0)");
        if (i > 0) {
            const bool block_first = i < d->n_layers - 1 && (i - 1) % d->layers_per_block == 0;
            const int prev_out = (block_first || i == d->n_layers - 1) ? L[0].out_dim : L[i - 1].out_dim;
            if (s.in_dim != prev_out) return fail(std::string(who) + ": layer dims do not chain");
        }
        if (i == d->n_layers - 1 && (s.batch_norm || s.relu)) return fail(std::string(who) + ": the output layer is a plain Linear");
        MlpTrainLayerDev &l = L[i];
        l = MlpTrainLayerDev{};
        l.in_dim = s.in_dim, l.out_dim = s.out_dim, l.relu = s.relu, l.bn = s.batch_norm ? 1 : 0;
        any_bn |= l.bn;
        l.w_off = off, off += s.out_dim * s.in_dim;
        l.b_off = off, off += s.out_dim;
        if (l.bn) {
            l.g_off = off, off += s.out_dim;
            l.be_off = off, off += s.out_dim;
        }
    }
    const int n_train = off;
    for (auto &l : L)
        if (l.bn) {
            l.rm_off = off, off += l.out_dim;
            l.rv_off = off, off += l.out_dim;
        }
    const int n_state = off;
    for (int b = 0; b < d->n_blocks; ++b)
        if (L[d->layers_per_block * (b + 1)].out_dim != L[0].out_dim) return fail(std::string(who) + ": block output dim != residual dim");
    if (wtk_device_count() <= d->device || d->device < 0) return fail(std::string(who) + ": no such HIP device (is a GPU visible?)");
    DEVICE_GUARD(d);
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&mlp_train_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kTrainLdsFloats * (int)sizeof(float)));
    wtk_mlp_trainer *h = new wtk_mlp_trainer();
    h->device = d->device;
    h->n_models = d->n_models, h->n_layers = d->n_layers, h->n_blocks = d->n_blocks, h->layers_per_block = d->layers_per_block, h->max_batch = d->max_batch;
    h->n_state = n_state, h->n_train = n_train, h->any_bn = any_bn;
    h->scratch_floats = (long long)(BUF_FIRST_ACT + 2 * d->n_layers + d->n_blocks) * d->max_batch * kTrainLd + (long long)d->n_layers * kMlpMaxDim;
    MlpTrainArgs &a = h->base;
    const size_t E = (size_t)d->n_models;
    void *layers = nullptr;
    if (trainer_alloc(h, (void **)&a.state, E * n_state * 4, false) || trainer_alloc(h, (void **)&a.best, E * n_state * 4, false) ||
        trainer_alloc(h, (void **)&a.grad, E * n_train * 4, true) || trainer_alloc(h, (void **)&a.m, E * n_train * 4, true) ||
        trainer_alloc(h, (void **)&a.v, E * n_train * 4, true) || trainer_alloc(h, (void **)&a.scratch, E * (size_t)h->scratch_floats * 4, true) ||
        trainer_alloc(h, (void **)&a.steps, E * 4, true) || trainer_alloc(h, (void **)&a.best_steps, E * 4, true) ||
        trainer_alloc(h, (void **)&a.best_loss, E * 4, true) || trainer_alloc(h, (void **)&a.has_best, E * 4, true) ||
        trainer_alloc(h, (void **)&a.no_improve, E * 4, true) || trainer_alloc(h, &layers, L.size() * sizeof(MlpTrainLayerDev), false)) {
        wtk_mlp_trainer_destroy(h);
        return 1;
    }
    hipError_t err;
    if ((err = hipMemcpy(a.state, d->state, E * n_state * 4, hipMemcpyHostToDevice)) != hipSuccess ||
        (err = hipMemcpy(a.best, d->state, E * n_state * 4, hipMemcpyHostToDevice)) != hipSuccess ||
        (err = hipMemcpy(layers, L.data(), L.size() * sizeof(MlpTrainLayerDev), hipMemcpyHostToDevice)) != hipSuccess) {
        wtk_mlp_trainer_destroy(h);
        return fail_hip(who, err);
    }
    a.layers = (const MlpTrainLayerDev *)layers;
    a.n_layers = d->n_layers, a.n_blocks = d->n_blocks, a.layers_per_block = d->layers_per_block;
    a.n_state = n_state, a.n_train = n_train, a.max_batch = d->max_batch, a.scratch_floats = h->scratch_floats;
    a.loss_kind = d->loss, a.opt_kind = d->optimizer, a.in_dim = L[0].in_dim, a.out_dim = L.back().out_dim;
    a.use_lds = n_state <= kTrainLdsFloats;
    *out = h;
    return 0;
}

// the checks every call shares; `who` names the entry point
static int trainer_launch(wtk_mlp_trainer *h, const char *who, MlpTrainArgs a, hipStream_t stream) {
    if (a.n <= 0) return fail(std::string(who) + ": no samples");
    if (a.batch_size < 1 || a.batch_size > h->max_batch)
        return fail(std::string(who) + ": batch_size must be in [1, " + std::to_string(h->max_batch) + "] (the handle's max_batch; at most 1024)");
    a.n_batches = (a.n + a.batch_size - 1) / a.batch_size;
    if (a.mode != TRAIN_EVAL && h->any_bn && (a.batch_size == 1 || a.n % a.batch_size == 1))
        return fail(std::string(who) + ": a batch of one sample (batch_size 1, or the last, partial batch): train-mode BatchNorm expects more than 1 value per channel");
    DEVICE_GUARD(h);
    hipLaunchKernelGGL(mlp_train_kernel, dim3(h->n_models), dim3(kTrainThreads), a.use_lds ? (size_t)a.n_state * sizeof(float) : 0, stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int wtk_mlp_trainer_grad(wtk_mlp_trainer *h, const float *x_dev, const float *y_dev, int32_t batch, float *grad_dev, float *loss_dev, void *stream) {
    if (!h || !x_dev || !y_dev || !grad_dev || !loss_dev) return fail("wtk_mlp_trainer_grad: null argument");
    MlpTrainArgs a = h->base;
    a.mode = TRAIN_GRAD, a.x = x_dev, a.y = y_dev, a.n = batch, a.batch_size = batch, a.grad = grad_dev, a.loss_out = loss_dev;
    return trainer_launch(h, "wtk_mlp_trainer_grad", a, (hipStream_t)stream);
}

extern "C" int wtk_mlp_trainer_train_epoch(wtk_mlp_trainer *h, const float *x_dev, const float *y_dev, int32_t n, const int32_t *order_dev, int32_t batch_size,
                                           const double *lr_dev, const double *weight_decay_dev, int32_t *active_dev, float *loss_dev, int32_t *num_correct_dev,
                                           void *stream) {
    if (!h || !x_dev || !y_dev || !lr_dev || !weight_decay_dev || !loss_dev) return fail("wtk_mlp_trainer_train_epoch: null argument");
    MlpTrainArgs a = h->base;
    a.mode = TRAIN_STEP, a.x = x_dev, a.y = y_dev, a.n = n, a.order = order_dev, a.batch_size = batch_size, a.lr = lr_dev, a.wd = weight_decay_dev;
    a.active = active_dev, a.loss_out = loss_dev, a.nc_out = num_correct_dev;
    return trainer_launch(h, "wtk_mlp_trainer_train_epoch", a, (hipStream_t)stream);
}

extern "C" int wtk_mlp_trainer_step(wtk_mlp_trainer *h, const float *x_dev, const float *y_dev, int32_t batch, const double *lr_dev, const double *weight_decay_dev,
                                    float *loss_dev, int32_t *num_correct_dev, void *stream) {
    if (!h || !x_dev || !y_dev || !lr_dev || !weight_decay_dev || !loss_dev) return fail("wtk_mlp_trainer_step: null argument");
    MlpTrainArgs a = h->base;
    a.mode = TRAIN_STEP, a.x = x_dev, a.y = y_dev, a.n = batch, a.batch_size = batch, a.lr = lr_dev, a.wd = weight_decay_dev;
    a.loss_out = loss_dev, a.nc_out = num_correct_dev;
    return trainer_launch(h, "wtk_mlp_trainer_step", a, (hipStream_t)stream);
}

extern "C" int wtk_mlp_trainer_eval_epoch(wtk_mlp_trainer *h, const float *x_dev, const float *y_dev, int32_t n, int32_t batch_size, int32_t patience,
                                          int32_t track_best, int32_t *active_dev, float *loss_dev, int32_t *num_correct_dev, float *pred_dev, void *stream) {
    if (!h || !x_dev || !y_dev || !loss_dev) return fail("wtk_mlp_trainer_eval_epoch: null argument");
    MlpTrainArgs a = h->base;
    a.mode = TRAIN_EVAL, a.x = x_dev, a.y = y_dev, a.n = n, a.batch_size = batch_size, a.patience = patience, a.active = active_dev;
    a.loss_out = loss_dev, a.nc_out = num_correct_dev, a.pred_out = pred_dev;
    if (track_best < 0 || track_best > 2) return fail("wtk_mlp_trainer_eval_epoch: track_best must be 0, 1 or 2");
    if (!track_best) a.best = nullptr;
    a.reset_best = track_best == 2;
    return trainer_launch(h, "wtk_mlp_trainer_eval_epoch", a, (hipStream_t)stream);
}

extern "C" int wtk_mlp_trainer_get_state(wtk_mlp_trainer *h, int32_t which, float *state_host, int32_t *steps_host, void *stream) {
    if (!h || !state_host) return fail("wtk_mlp_trainer_get_state: null argument");
    if (which < 0 || which > 3) return fail("wtk_mlp_trainer_get_state: which must be 0 (state), 1 (best state), 2 (first moment) or 3 (second moment)");
    DEVICE_GUARD(h);
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    const MlpTrainArgs &a = h->base;
    const float *src = which == 0 ? a.state : which == 1 ? a.best : which == 2 ? a.m : a.v;
    const size_t per = which <= 1 ? h->n_state : h->n_train;
    HIP_TRY(hipMemcpy(state_host, src, (size_t)h->n_models * per * 4, hipMemcpyDeviceToHost));
    if (steps_host) HIP_TRY(hipMemcpy(steps_host, which == 1 ? a.best_steps : a.steps, (size_t)h->n_models * 4, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int wtk_mlp_trainer_get_stopping(wtk_mlp_trainer *h, float *best_loss_host, int32_t *has_best_host, int32_t *no_improve_host, void *stream) {
    if (!h || !best_loss_host || !has_best_host || !no_improve_host) return fail("wtk_mlp_trainer_get_stopping: null argument");
    DEVICE_GUARD(h);
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    const MlpTrainArgs &a = h->base;
    HIP_TRY(hipMemcpy(best_loss_host, a.best_loss, (size_t)h->n_models * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(has_best_host, a.has_best, (size_t)h->n_models * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(no_improve_host, a.no_improve, (size_t)h->n_models * 4, hipMemcpyDeviceToHost));
    return 0;
}
