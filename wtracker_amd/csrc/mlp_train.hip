// Training of the ResMLP predictor (wtracker/neural/training.py:267-333, MLPTrainer over RMLP in train mode, wtracker/neural/mlp.py:51-188):
// a POPULATION of E models of one structure, one workgroup per model (blockIdx.x = e).  A workgroup never waits for another one, there is no grid-wide
// barrier and no cooperative launch; every loop runs to a bound the host validated.
//
// mlp_train_kernel is a driver over named phases, each a __device__ __forceinline__ function of one TrainCtx.  One batch =
//   gather_batch -> forward_layer per layer (linear_forward, batchnorm_train, residual_add) -> loss_and_seed -> backward_layer per layer, last to first
//   (activation_backward into dz, then db, dW and dx) -> optimizer_step;   after the last batch: the state write-back, or early_stopping.
// What the phases share is stated once: TrainScratch (the per-model scratch layout), ResTopology (which layer feeds which), state_layout (the parameter
// layout, host side), batch_row, chan_sum / chan_sum2, relu_masked, and train_tile with its element visitor tile_each.
//
// Every matrix product is the exact-fp32 MFMA of mlp.hip (v_mfma_f32_16x16x4_f32, a k-ordered fma chain): a wave owns whole 16 x 16 output tiles and
// walks K in ascending order, so
//   forward   z  = a W^T      K = the layer's inputs
//   dW        = dz^T a        K = the batch's samples, ascending
//   dx        = dz W          K = the layer's outputs
// need no cross-wave reduction, and the BatchNorm / bias / loss sums over the samples are taken in a fixed two-level order (chan_sum).
// A model's bits therefore depend on nothing but its own parameters, data, order and hyper-parameters: not on E, its index, its neighbours or the run.
//
// The unfolded parameter set ("state", state_layout) stays in LDS for the whole launch while it fits kTrainLdsFloats (the notebook's model: 35 488 floats
// = 139 KiB of 160 KiB) and is read and updated in global memory above that; both paths run the same code through flat pointers, so they give the same
// bits.  Operand loads are masked (row, column and k bounds), so no buffer needs padding and no load leaves its allocation.  Activations saved for
// backward, gradients and optimizer moments live in per-model global scratch owned by the handle.  Each phase states the workgroup barriers it executes:
// a BatchNorm layer 6 forward and 5 backward, the notebook's model 198 per training step and 26 per eval batch.
#include "wtk_device.h"
#include "wtk_internal.h"
#include "mlp_fold.h" // MlpTrainLayerDev, the blob layout, mlp_fold_row

#include <cmath>
#include <string>
#include <vector>

namespace wtk {

constexpr int kTrainLd = kMlpMaxDim;       // row stride (floats) of every activation buffer
constexpr int kTrainThreads = 1024;        // one workgroup = 16 waves
constexpr int kTrainWaves = kTrainThreads / 64;
constexpr int kTrainMaxBatch = 1024;       // samples of one batch (the loss partials are one per thread)
constexpr int kTrainLdsFloats = 36864;     // 144 KiB of parameters in LDS; ~14 KiB of static LDS next to them
constexpr int kChanParts = kTrainThreads / kMlpMaxDim; // threads per channel of chan_sum
constexpr float kBnEps = 1e-5f, kBnMomentum = 0.1f;
enum { TRAIN_STEP = 0, TRAIN_GRAD = 1, TRAIN_EVAL = 2 };
enum { LOSS_MSE = 0, LOSS_L1 = 1 };
enum { OPT_ADAM = 0, OPT_ADAMW = 1, OPT_SGD = 2, OPT_RMSPROP = 3 };

// Which layer feeds which: layer 0 is the input layer, layer n_layers - 1 the output layer (a plain Linear on the residual stream), and the layers
// between them form blocks of layers_per_block, each block adding its last layer's output to the residual stream it read: h <- h + block(h).
struct ResTopology {
    int n_layers, layers_per_block;
    __host__ __device__ bool is_input(int i) const { return i == 0; }
    __host__ __device__ bool is_output(int i) const { return i == n_layers - 1; }
    __host__ __device__ bool in_block(int i) const { return !is_input(i) && !is_output(i); }
    __host__ __device__ int block_of(int i) const { return (i - 1) / layers_per_block; } // of a layer in a block
    __host__ __device__ int place(int i) const { return (i - 1) % layers_per_block; }    // ... and its place in that block
    __host__ __device__ bool block_first(int i) const { return in_block(i) && place(i) == 0; }
    __host__ __device__ bool block_last(int i) const { return in_block(i) && place(i) == layers_per_block - 1; }
};

// The scratch of one model, as float offsets: buffers of [max_batch][kTrainLd], then stat [n_layers][kMlpMaxDim].
struct TrainScratch {
    int n_layers, n_blocks, max_batch;
    __host__ __device__ size_t buf(int k) const { return (size_t)k * ((size_t)max_batch * kTrainLd); }
    __host__ __device__ size_t x() const { return buf(0); }  // the batch's rows of x and y
    __host__ __device__ size_t y() const { return buf(1); }
    __host__ __device__ size_t dh() const { return buf(2); } // gradient of the residual stream
    __host__ __device__ size_t dz() const { return buf(3); } // gradient of the current layer's Linear output
    __host__ __device__ size_t dx() const { return buf(4); } // gradient of the current layer's input inside a block
    __host__ __device__ size_t act(int i) const { return buf(5 + i); }             // output of layer i (after BatchNorm and ReLU)
    __host__ __device__ size_t xhat(int i) const { return buf(5 + n_layers + i); } // z, then x^ of a BatchNorm layer
    __host__ __device__ size_t hres(int b) const { return b == 0 ? act(0) : buf(5 + 2 * n_layers + b - 1); } // residual stream in front of block b
    __host__ __device__ size_t stat() const { return buf(5 + 2 * n_layers + n_blocks); } // 1 / sqrt(var + eps) of the batch
    __host__ __device__ long long floats() const { return (long long)stat() + (long long)n_layers * kMlpMaxDim; }
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

// What the phases work on, built once at kernel entry.
struct TrainCtx {
    const MlpTrainArgs &a;
    int e, tid, lane, wave;
    int cch, cpart;                 // chan_sum: this thread's channel and which of its kChanParts partial sums it takes
    bool train;                     // batch statistics and a backward pass (not TRAIN_EVAL)
    float *P;                       // the model's state, in LDS or in global memory
    float *G, *Mo, *Vo;             // its gradient and optimizer moments
    float *S;                       // its scratch, laid out by sc
    TrainScratch sc;
    float *XB, *YB, *DH, *DZ, *DX, *stat; // ... of which the buffers every layer uses: S + sc.x(), y(), dh(), dz(), dx(), stat()
    ResTopology net;
    const MlpTrainLayerDev *layers; // in LDS, as all that follows
    float *part, *part1, *c0, *c1;  // chan_sum's partial sums (part also: per-sample losses), per-channel values of a BatchNorm pass
    int *flag;                      // per-sample num_correct
    float *part2;                   // second level of the loss sum and of num_correct
    int *flag2;
    double *opt;                    // optimizer scalars of the step
    int *improved;
    __host__ __device__ size_t input_of(int i) const { // residual stream in front of the layer's block (output layer: behind the last block), or layer i - 1
        return net.is_input(i) ? sc.x() : (net.is_output(i) ? sc.hres(sc.n_blocks) : (net.block_first(i) ? sc.hres(net.block_of(i)) : sc.act(i - 1)));
    }
};

// One 16 x 16 tile of D = A B, D[m][n] = sum_{k < K} A(m, k) B(k, n) in ascending k: A(m, k) = A[m * a_rs + k * a_ks], B(k, n) = B[k * b_ks + n * b_cs].
// Loads outside m < M, n < N, k < K are replaced by 0 (their address is clamped to element 0 of the row / column).  The lane holds D[m0 + 4 g + i][n0 + r],
// r = lane & 15, g = lane >> 4: tile_col, and tile_each's rows.
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
__device__ __forceinline__ int tile_col(int n0, int lane) { return n0 + (lane & 15); }
template <class F> __device__ __forceinline__ void tile_each(const floatx4 &acc, int m0, int n0, int lane, F f) { // f(row, col, value) for the lane's four elements
#pragma unroll
    for (int j = 0; j < 4; ++j) f(m0 + 4 * (lane >> 4) + j, tile_col(n0, lane), acc[j]);
}

// chan_sum: a sum over the batch's samples per channel is taken by kChanParts threads per channel — thread (part j, channel c) adds the terms of samples
// j, j + 8, ... in ascending order — and the kChanParts partial sums are added in the order j = 0 .. 7: a fixed order, whatever E is.  term(at) is the
// sample's term, at = s * kTrainLd + c.  One barrier, between the partial sums and the total; the caller's next barrier frees the partial sums again.
// The total of channel c.cch comes back in all of its threads (to_all_parts: each adds the same partial sums in the same order) or in thread c alone.
__device__ __forceinline__ float chan_total(const float *part, int ch) {
    float t = 0.f;
#pragma unroll
    for (int j = 0; j < kChanParts; ++j) t += part[j * kMlpMaxDim + ch];
    return t;
}
template <class F> __device__ __forceinline__ float chan_sum(const TrainCtx &c, int n_ch, int B, bool to_all_parts, F term) {
    float p = 0.f;
    if (c.cch < n_ch)
        for (int s = c.cpart; s < B; s += kChanParts) p += term(s * kTrainLd + c.cch);
    c.part[c.cpart * kMlpMaxDim + c.cch] = p;
    __syncthreads();
    return (to_all_parts || c.tid < n_ch) ? chan_total(c.part, c.cch) : 0.f;
}
template <class F> __device__ __forceinline__ void chan_sum2(const TrainCtx &c, int n_ch, int B, float &t0, float &t1, F term) { // two sums; totals in thread c
    float p0 = 0.f, p1 = 0.f;
    if (c.cch < n_ch)
        for (int s = c.cpart; s < B; s += kChanParts) term(s * kTrainLd + c.cch, p0, p1);
    c.part[c.cpart * kMlpMaxDim + c.cch] = p0;
    c.part1[c.cpart * kMlpMaxDim + c.cch] = p1;
    __syncthreads();
    if (c.tid < n_ch) t0 = chan_total(c.part, c.tid), t1 = chan_total(c.part1, c.tid);
}

// the sample that position i of model e's epoch stands for
__device__ __forceinline__ int batch_row(const MlpTrainArgs &a, int e, int i) {
    const int row = a.order ? a.order[(size_t)e * a.n + i] : i;
    return min(max(row, 0), a.n - 1);
}
// the gradient src[at] of a layer's output, taken behind its ReLU: 0 where the output aout[at] is not positive
__device__ __forceinline__ float relu_masked(const float *src, const float *aout, int at, int relu) {
    float d = src[at];
    if (relu && !(aout[at] > 0.f)) d = 0.f;
    return d;
}

// ---- the batch's rows of x and y.  1 barrier
__device__ __forceinline__ void gather_rows(const TrainCtx &c, const float *src, int dim, float *dst, int b0, int B) {
    for (int i = c.tid; i < B * dim; i += kTrainThreads) {
        const int s = i / dim, k = i - s * dim;
        dst[s * kTrainLd + k] = src[(size_t)batch_row(c.a, c.e, b0 + s) * dim + k];
    }
}
__device__ __forceinline__ void gather_batch(const TrainCtx &c, int b0, int B) {
    gather_rows(c, c.a.x, c.a.in_dim, c.XB, b0, B);
    gather_rows(c, c.a.y, c.a.out_dim, c.YB, b0, B);
    __syncthreads();
}

// ---- forward.  z = in W^T + b, finished into act(i), or as z into xhat(i) where batch statistics follow.  1 barrier
__device__ __forceinline__ void linear_forward(const TrainCtx &c, int i, const MlpTrainLayerDev &L, int B, bool bn_batch) {
    const float *P = c.P, *in = c.S + c.input_of(i), *W = P + L.w_off;
    const bool train = c.train;
    float *zdst = c.S + (bn_batch ? c.sc.xhat(i) : c.sc.act(i));
    const int tm = (B + 15) / 16, tn = (L.out_dim + 15) / 16;
    for (int t = c.wave; t < tm * tn; t += kTrainWaves) {
        const int m0 = (t / tn) * 16, n0 = (t % tn) * 16;
        const floatx4 acc = train_tile(in, kTrainLd, 1, B, W, 1, L.in_dim, L.out_dim, L.in_dim, m0, n0, c.lane);
        const int o = tile_col(n0, c.lane);
        if (o < L.out_dim) {
            const float bias = P[L.b_off + o];
            float sc = 1.f, sh = 0.f, mu = 0.f, ga = 1.f;
            if (L.bn && !train) { // eval: running statistics, in the order of the reference's modules
                mu = P[L.rm_off + o];
                sc = sqrtf(P[L.rv_off + o] + kBnEps);
                ga = P[L.g_off + o];
                sh = P[L.be_off + o];
            }
            tile_each(acc, m0, n0, c.lane, [&](int s, int, float z) {
                if (s < B) {
                    float v = z + bias;
                    if (L.bn && !train) v = (v - mu) / sc * ga + sh;
                    if (!bn_batch && L.relu) v = fmaxf(v, 0.f);
                    zdst[s * kTrainLd + o] = v;
                }
            });
        }
    }
    __syncthreads();
}
// BatchNorm1d on the batch's statistics: the mean, then the biased variance around it, x^ over z in xhat(i), act(gamma x^ + beta) into act(i).  5 barriers
__device__ __forceinline__ void batchnorm_train(const TrainCtx &c, int i, const MlpTrainLayerDev &L, int B) {
    float *P = c.P, *Z = c.S + c.sc.xhat(i), *Aout = c.S + c.sc.act(i);
    const int tid = c.tid;
    const float mean = chan_sum(c, L.out_dim, B, true, [&](int at) { return Z[at]; }) / (float)B;
    __syncthreads();
    const float sq = chan_sum(c, L.out_dim, B, false, [&](int at) {
        const float d = Z[at] - mean;
        return d * d;
    });
    if (tid < L.out_dim) {
        const float var = sq / (float)B;
        const float inv = 1.f / sqrtf(var + kBnEps);
        c.c0[tid] = mean;
        c.c1[tid] = inv;
        c.stat[i * kMlpMaxDim + tid] = inv;
        if (c.a.mode == TRAIN_STEP) { // running_var takes the unbiased variance (torch.nn.BatchNorm1d)
            const float unb = sq / (float)(B - 1);
            P[L.rm_off + tid] = (1.f - kBnMomentum) * P[L.rm_off + tid] + kBnMomentum * mean;
            P[L.rv_off + tid] = (1.f - kBnMomentum) * P[L.rv_off + tid] + kBnMomentum * unb;
        }
    }
    __syncthreads();
    for (int idx = tid; idx < B * L.out_dim; idx += kTrainThreads) {
        const int s = idx / L.out_dim, o = idx - s * L.out_dim;
        const float xh = (Z[s * kTrainLd + o] - c.c0[o]) * c.c1[o];
        Z[s * kTrainLd + o] = xh;
        float v = xh * P[L.g_off + o] + P[L.be_off + o];
        if (L.relu) v = fmaxf(v, 0.f);
        Aout[s * kTrainLd + o] = v;
    }
    __syncthreads();
}
// h <- h + block(h) behind the last layer of a block.  1 barrier
__device__ __forceinline__ void residual_add(const TrainCtx &c, int i, int width, int B) {
    const int b = c.net.block_of(i);
    const float *h0 = c.S + c.sc.hres(b), *blk = c.S + c.sc.act(i);
    float *h1 = c.S + c.sc.hres(b + 1);
    for (int idx = c.tid; idx < B * width; idx += kTrainThreads) {
        const int s = idx / width, o = idx - s * width;
        h1[s * kTrainLd + o] = h0[s * kTrainLd + o] + blk[s * kTrainLd + o];
    }
    __syncthreads();
}
__device__ __forceinline__ void forward_layer(const TrainCtx &c, int i, int B) {
    const MlpTrainLayerDev L = c.layers[i];
    const bool bn_batch = L.bn && c.train;
    linear_forward(c, i, L, B, bn_batch);
    if (bn_batch) batchnorm_train(c, i, L, B);
    if (c.net.block_last(i)) residual_add(c, i, L.out_dim, B);
}

// ---- loss, num_correct (training.py:317) and the gradient of the loss into dz.  2 barriers
__device__ __forceinline__ void loss_and_seed(const TrainCtx &c, int bi, int b0, int B, float &eval_sum) {
    const MlpTrainArgs &a = c.a;
    const int tid = c.tid;
    const float *Pr = c.S + c.sc.act(a.n_layers - 1), *YB = c.YB;
    float *DZ = c.DZ;
    const float inv_n = 1.f / (float)(B * a.out_dim);
    if (tid < B) {
        float sum = 0.f, n2 = 0.f;
        for (int o = 0; o < a.out_dim; ++o) {
            const float d = Pr[tid * kTrainLd + o] - YB[tid * kTrainLd + o];
            n2 += d * d;
            sum += a.loss_kind == LOSS_MSE ? d * d : fabsf(d);
            if (c.train) DZ[tid * kTrainLd + o] = a.loss_kind == LOSS_MSE ? 2.f * d * inv_n : (d > 0.f ? inv_n : (d < 0.f ? -inv_n : 0.f));
        }
        c.part[tid] = sum;
        c.flag[tid] = sqrtf(n2) < 1.0f ? 1 : 0;
        if (a.pred_out)
            for (int o = 0; o < a.out_dim; ++o) a.pred_out[((size_t)c.e * a.n + batch_row(a, c.e, b0 + tid)) * a.out_dim + o] = Pr[tid * kTrainLd + o];
    }
    __syncthreads();
    if (tid < 64) { // fixed two-level order: 64 runs of 16 samples, then the 64 partial sums
        float sum = 0.f;
        int cnt = 0;
        for (int j = 0; j < 16; ++j) {
            const int s = tid * 16 + j;
            if (s < B) {
                sum += c.part[s];
                cnt += c.flag[s];
            }
        }
        c.part2[tid] = sum;
        c.flag2[tid] = cnt;
    }
    __syncthreads();
    if (tid == 0) {
        float sum = 0.f;
        int cnt = 0;
        for (int j = 0; j < 64; ++j) {
            sum += c.part2[j];
            cnt += c.flag2[j];
        }
        const float loss = sum * inv_n;
        a.loss_out[(size_t)c.e * a.n_batches + bi] = loss;
        if (a.nc_out) a.nc_out[(size_t)c.e * a.n_batches + bi] = cnt;
        eval_sum += loss;
    }
}

// ---- backward.  The gradient src of layer i's output, through its ReLU and BatchNorm (the batch statistics take part; dgamma, dbeta), into dz.
// 1 barrier, + 2 with BatchNorm
__device__ __forceinline__ void activation_backward(const TrainCtx &c, int i, const MlpTrainLayerDev &L, int B, const float *src) {
    const float *P = c.P, *Aout = c.S + c.sc.act(i);
    float *DZ = c.DZ;
    if (L.bn) {
        const float *Xh = c.S + c.sc.xhat(i), *stat = c.stat;
        float dg = 0.f, db = 0.f;
        chan_sum2(c, L.out_dim, B, dg, db, [&](int at, float &pg, float &pb) {
            const float d = relu_masked(src, Aout, at, L.relu);
            pg += d * Xh[at];
            pb += d;
        });
        if (c.tid < L.out_dim) {
            c.G[L.g_off + c.tid] = dg;
            c.G[L.be_off + c.tid] = db;
            c.c0[c.tid] = dg;
            c.c1[c.tid] = db;
        }
        __syncthreads();
        const float fB = (float)B;
        for (int idx = c.tid; idx < B * L.out_dim; idx += kTrainThreads) {
            const int s = idx / L.out_dim, o = idx - s * L.out_dim;
            const float d = relu_masked(src, Aout, s * kTrainLd + o, L.relu);
            const float k = P[L.g_off + o] * stat[i * kMlpMaxDim + o] / fB;
            DZ[s * kTrainLd + o] = k * (fB * d - c.c1[o] - Xh[s * kTrainLd + o] * c.c0[o]);
        }
    } else {
        for (int idx = c.tid; idx < B * L.out_dim; idx += kTrainThreads) {
            const int s = idx / L.out_dim, o = idx - s * L.out_dim;
            DZ[s * kTrainLd + o] = relu_masked(src, Aout, s * kTrainLd + o, L.relu);
        }
    }
    __syncthreads();
}
// Layer i turns the gradient of its output (the loss's seed in dz, dh behind a block or the input layer, dx inside a block) into dz, then into db, dW and
// the gradient of its input: dh behind the output layer, added to dh in front of a block (dh = dh + d(block input)), dx inside one.  2 barriers + the above
__device__ __forceinline__ void backward_layer(const TrainCtx &c, int i, int B) {
    const MlpTrainLayerDev L = c.layers[i];
    const bool is_out = c.net.is_output(i), is_in = c.net.is_input(i), first = c.net.block_first(i);
    float *DH = c.DH, *DZ = c.DZ, *DX = c.DX, *G = c.G;
    if (!is_out) activation_backward(c, i, L, B, (is_in || c.net.block_last(i)) ? DH : DX);
    const float *in = c.S + c.input_of(i), *W = c.P + L.w_off;
    const int to = (L.out_dim + 15) / 16, tk = (L.in_dim + 15) / 16, tm = (B + 15) / 16;
    const int n_dw = to * tk, n_dx = is_in ? 0 : tm * tk;
    // db[o] = sum_s dz[s][o]; its totals are added while the tile loop runs, whose barrier frees the partial sums
    const float db = chan_sum(c, L.out_dim, B, false, [&](int at) { return DZ[at]; });
    if (c.tid < L.out_dim) G[L.b_off + c.tid] = db;
    for (int t = c.wave; t < n_dw + n_dx; t += kTrainWaves) {
        if (t < n_dw) { // dW[o][k] = sum_s dz[s][o] a[s][k]
            const int m0 = (t / tk) * 16, n0 = (t % tk) * 16;
            const floatx4 acc = train_tile(DZ, 1, kTrainLd, L.out_dim, in, kTrainLd, 1, L.in_dim, B, m0, n0, c.lane);
            tile_each(acc, m0, n0, c.lane, [&](int o, int k, float v) {
                if (o < L.out_dim && k < L.in_dim) G[L.w_off + o * L.in_dim + k] = v;
            });
        } else { // dx[s][k] = sum_o dz[s][o] W[o][k]
            const int u = t - n_dw;
            const int m0 = (u / tk) * 16, n0 = (u % tk) * 16;
            const floatx4 acc = train_tile(DZ, kTrainLd, 1, B, W, L.in_dim, 1, L.in_dim, L.out_dim, m0, n0, c.lane);
            tile_each(acc, m0, n0, c.lane, [&](int s, int k, float v) {
                if (s < B && k < L.in_dim) {
                    if (is_out)
                        DH[s * kTrainLd + k] = v;
                    else if (first)
                        DH[s * kTrainLd + k] += v;
                    else
                        DX[s * kTrainLd + k] = v;
                }
            });
        }
    }
    __syncthreads();
}

// ---- optimizer (torch.optim defaults but lr and weight_decay: neural/config.py:28-33).  The scalars of step t + 1, which torch computes in double on
// the host, by thread 0 in front of gather_batch's barrier; the step itself: 1 barrier
__device__ __forceinline__ void optimizer_scalars(const TrainCtx &c, int step_t) {
    if (c.tid != 0) return;
    const double lr = c.a.lr[c.e], t = (double)(step_t + 1);
    if (c.a.opt_kind == OPT_ADAM || c.a.opt_kind == OPT_ADAMW) {
        const double bc1 = 1.0 - pow(0.9, t), bc2 = 1.0 - pow(0.999, t);
        c.opt[0] = lr / bc1;  // step_size
        c.opt[1] = sqrt(bc2); // bias_correction2_sqrt
    } else {
        c.opt[0] = lr;
        c.opt[1] = 1.0;
    }
    c.opt[2] = c.a.wd[c.e];
    c.opt[3] = 1.0 - lr * c.a.wd[c.e]; // adamw: decoupled decay
}
__device__ __forceinline__ void optimizer_step(const TrainCtx &c) {
    const int opt_kind = c.a.opt_kind;
    float *P = c.P, *G = c.G, *Mo = c.Mo, *Vo = c.Vo;
    const float step_size = (float)c.opt[0], bc2s = (float)c.opt[1], wd = (float)c.opt[2], decay = (float)c.opt[3], lr = (float)c.opt[0];
    for (int i = c.tid; i < c.a.n_train; i += kTrainThreads) {
        float p = P[i], g = G[i];
        if (opt_kind == OPT_ADAMW) {
            p = p * decay;
        } else if (wd != 0.f) {
            // grad.add(param, alpha = weight_decay) is ONE fma in torch.  Where g ~ -wd p the sum cancels, and the second rounding of a separate
            // multiply (half a unit in the last place of wd p, any fraction of what is left) is what Adam / RMSprop then normalise into the step
            g = fmaf(wd, p, g);
        }
        if (opt_kind == OPT_ADAM || opt_kind == OPT_ADAMW) {
            float m = Mo[i], v = Vo[i];
            m = m + (g - m) * 0.1f;               // exp_avg.lerp_(grad, 1 - beta1)
            v = v * 0.999f + (0.001f * g) * g;     // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
            Mo[i] = m;
            Vo[i] = v;
            const float denom = sqrtf(v) / bc2s + 1e-8f;
            p = p - step_size * (m / denom);
        } else if (opt_kind == OPT_SGD) {
            p = p - lr * g;
        } else { // rmsprop: alpha 0.99, eps 1e-8, no momentum, not centered
            float v = Vo[i];
            v = v * 0.99f + (0.01f * g) * g;
            Vo[i] = v;
            p = p - lr * (g / (sqrtf(v) + 1e-8f));
        }
        P[i] = p;
    }
    __syncthreads();
}

// ---- early stopping, training.py:119-128: curr = fp32 sum of the batch losses in batch order / n_batches, strict <, the best state kept on the device
__device__ __forceinline__ void early_stopping(const TrainCtx &c, float eval_sum, int step_t) {
    const MlpTrainArgs &a = c.a;
    const int e = c.e;
    if (c.tid == 0) {
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
        *c.improved = improved;
    }
    __syncthreads();
    if (*c.improved) {
        float *bst = a.best + (size_t)e * a.n_state;
        for (int i = c.tid; i < a.n_state; i += kTrainThreads) bst[i] = c.P[i];
    }
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
    const int e = blockIdx.x, tid = threadIdx.x;
    constexpr int T = kTrainThreads;
    if (a.active && a.active[e] == 0) return; // block uniform: a stopped model costs nothing

    float *gstate = a.state + (size_t)e * a.n_state;
    if (a.use_lds)
        for (int i = tid; i < a.n_state; i += T) wlds[i] = gstate[i];
    for (int i = tid; i < a.n_layers * (int)(sizeof(MlpTrainLayerDev) / sizeof(int)); i += T)
        reinterpret_cast<int *>(s_layers)[i] = reinterpret_cast<const int *>(a.layers)[i];
    float *s_part1 = reinterpret_cast<float *>(s_flag); // second partial-sum array (the loss phase's flags are not live then)
    float *S = a.scratch + (size_t)e * a.scratch_floats;
    const TrainScratch sc{a.n_layers, a.n_blocks, a.max_batch};
    const TrainCtx c = {a, e, tid, tid & 63, tid >> 6, tid & (kMlpMaxDim - 1), tid / kMlpMaxDim, a.mode != TRAIN_EVAL,
                        a.use_lds ? wlds : gstate, a.grad ? a.grad + (size_t)e * a.n_train : nullptr, a.m ? a.m + (size_t)e * a.n_train : nullptr,
                        a.v ? a.v + (size_t)e * a.n_train : nullptr, S, sc, S + sc.x(), S + sc.y(), S + sc.dh(), S + sc.dz(), S + sc.dx(), S + sc.stat(),
                        ResTopology{a.n_layers, a.layers_per_block}, s_layers, s_part, s_part1, s_c0, s_c1, s_flag, s_part2, s_flag2, s_opt, &s_improved};
    int step_t = a.steps[e];
    float eval_sum = 0.f; // thread 0: fp32 sum of the batch losses of an eval epoch, in batch order
    __syncthreads();

    for (int bi = 0; bi < a.n_batches; ++bi) {
        const int b0 = bi * a.batch_size;
        const int B = min(a.batch_size, a.n - b0);
        if (a.mode == TRAIN_STEP) optimizer_scalars(c, step_t);
        gather_batch(c, b0, B);
        for (int i = 0; i < a.n_layers; ++i) forward_layer(c, i, B);
        loss_and_seed(c, bi, b0, B, eval_sum);
        if (!c.train) {
            __syncthreads();
            continue;
        }
        for (int i = a.n_layers - 1; i >= 0; --i) backward_layer(c, i, B);
        if (a.mode == TRAIN_GRAD) continue;
        optimizer_step(c);
        step_t += 1;
    }

    if (a.mode == TRAIN_STEP) {
        if (a.use_lds)
            for (int i = tid; i < a.n_state; i += T) gstate[i] = wlds[i];
        if (tid == 0) a.steps[e] = step_t;
    } else if (a.mode == TRAIN_EVAL && a.best) {
        early_stopping(c, eval_sum, step_t);
    }
}

// ---- the inference blob of every model from its state (mlp_fold.h): one workgroup per (model, layer), one thread per padded output row
__global__ __launch_bounds__(kMlpMaxDim) void mlp_fold_kernel(const float *state, int n_state, const MlpTrainLayerDev *layers, int n_layers, float *blob, int blob_floats) {
    const int e = blockIdx.x, i = blockIdx.y, o = threadIdx.x;
    int off = 0;
    for (int j = 0; j < i; ++j) off += mlp_layer_blob_floats(layers[j].in_dim, layers[j].out_dim);
    const MlpTrainLayerDev T = layers[i];
    float *dst = blob + (size_t)e * blob_floats;
    if (o < mlp_out_pad(T.out_dim)) mlp_fold_row(T, off, o, state + (size_t)e * n_state, dst);
    if (i == n_layers - 1 && o == 0) // the blob's round-up to 4 floats
        for (int k = off + mlp_layer_blob_floats(T.in_dim, T.out_dim); k < blob_floats; ++k) dst[k] = 0.f;
}

// ---- the best state by a caller's score: a finite score[e] strictly below the stored one (or the first one) copies the state and the step count.
// NaN and +-inf never win, a tie keeps the earlier state.  One workgroup per model; the decision is read by every thread before thread 0 stores it.
__global__ __launch_bounds__(256) void mlp_keep_scored_kernel(const float *state, int n_state, const int *steps, const double *score, const int *active, float *scored,
                                                              int *scored_steps, double *best_score, int *has_score) {
    const int e = blockIdx.x;
    if (active && active[e] == 0) return; // block uniform
    const double s = score[e];
    const bool take = isfinite(s) && (!has_score[e] || s < best_score[e]);
    __syncthreads();
    if (!take) return;
    for (int i = threadIdx.x; i < n_state; i += 256) scored[(size_t)e * n_state + i] = state[(size_t)e * n_state + i];
    if (threadIdx.x == 0) best_score[e] = s, has_score[e] = 1, scored_steps[e] = steps[e];
}

} // namespace wtk

// =====================================================================================================================================================
// C ABI
// =====================================================================================================================================================
using namespace wtk;

struct wtk_mlp_trainer {
    int device = 0;
    int n_models = 0, max_batch = 0;
    int n_state = 0, n_train = 0, any_bn = 0;
    MlpTrainArgs base{};
    std::vector<void *> allocs;
    // the state kept by a caller's score (wtk_mlp_trainer_keep_scored): allocated by the first call, the initial state until a score wins
    std::vector<float> initial; // host, [n_models][n_state]
    std::vector<wtk_mlp_train_layer> structure;
    float *scored = nullptr;
    int *scored_steps = nullptr, *has_score = nullptr;
    double *best_score = nullptr;
    int64_t blob_floats = 0;
};

static int trainer_alloc(wtk_mlp_trainer *h, void **p, size_t bytes, bool zero) {
    HIP_TRY(hipMalloc(p, bytes ? bytes : 4));
    h->allocs.push_back(*p);
    if (zero) HIP_TRY(hipMemset(*p, 0, bytes ? bytes : 4));
    return 0;
}

// The unfolded state of a model, in floats: per layer W [out][in], b, [gamma, beta] (the n_train trainable floats; gradients and optimizer moments
// have this section alone), then per BatchNorm layer running_mean, running_var.  Returns n_state; with L, writes each layer's offsets.
static int64_t state_layout(const wtk_mlp_train_layer *layers, int n_layers, int64_t *n_train, MlpTrainLayerDev *L) {
    int64_t off = 0;
    auto place = [&](int i, int MlpTrainLayerDev::*field, int64_t n) {
        if (L) L[i].*field = (int)off;
        off += n;
    };
    for (int i = 0; i < n_layers; ++i) {
        const wtk_mlp_train_layer &s = layers[i];
        place(i, &MlpTrainLayerDev::w_off, (int64_t)s.out_dim * s.in_dim);
        place(i, &MlpTrainLayerDev::b_off, s.out_dim);
        if (s.batch_norm) place(i, &MlpTrainLayerDev::g_off, s.out_dim), place(i, &MlpTrainLayerDev::be_off, s.out_dim);
    }
    if (n_train) *n_train = off;
    for (int i = 0; i < n_layers; ++i)
        if (layers[i].batch_norm) place(i, &MlpTrainLayerDev::rm_off, layers[i].out_dim), place(i, &MlpTrainLayerDev::rv_off, layers[i].out_dim);
    return off;
}

extern "C" int64_t wtk_mlp_trainer_state_floats(const wtk_mlp_trainer_desc *d, int64_t *n_train_out) {
    if (!d || !d->layers || d->n_layers <= 0) return -1;
    return state_layout(d->layers, d->n_layers, n_train_out, nullptr);
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
    const ResTopology net{d->n_layers, d->layers_per_block};
    std::vector<MlpTrainLayerDev> L(d->n_layers);
    int any_bn = 0;
    for (int i = 0; i < d->n_layers; ++i) {
        const wtk_mlp_train_layer &s = d->layers[i];
        if (s.in_dim <= 0 || s.out_dim <= 0 || s.in_dim > kMlpMaxDim || s.out_dim > kMlpMaxDim) return fail(std::string(who) + ": layer width outside [1, kMlpMaxDim = 128]");
        if (s.relu != 0 && s.relu != 1) return fail(std::string(who) + ": activation must be ReLU (1) or none (0)");
        // a layer reads the residual stream (as wide as the input layer's output) or the layer before it: TrainCtx::input_of
        if (!net.is_input(i) && s.in_dim != ((net.block_first(i) || net.is_output(i)) ? L[0].out_dim : L[i - 1].out_dim)) return fail(std::string(who) + ": layer dims do not chain");
        if (net.is_output(i) && (s.batch_norm || s.relu)) return fail(std::string(who) + ": the output layer is a plain Linear");
        L[i] = MlpTrainLayerDev{};
        L[i].in_dim = s.in_dim, L[i].out_dim = s.out_dim, L[i].relu = s.relu, L[i].bn = s.batch_norm ? 1 : 0;
        any_bn |= L[i].bn;
    }
    int64_t n_train64 = 0;
    const int n_state = (int)state_layout(d->layers, d->n_layers, &n_train64, L.data()), n_train = (int)n_train64;
    for (int i = 0; i < d->n_layers; ++i)
        if (net.block_last(i) && L[i].out_dim != L[0].out_dim) return fail(std::string(who) + ": block output dim != residual dim");
    if (wtk_device_count() <= d->device || d->device < 0) return fail(std::string(who) + ": no such HIP device (is a GPU visible?)");
    DEVICE_GUARD(d);
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&mlp_train_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kTrainLdsFloats * (int)sizeof(float)));
    wtk_mlp_trainer *h = new wtk_mlp_trainer();
    h->device = d->device;
    h->n_models = d->n_models, h->max_batch = d->max_batch;
    h->n_state = n_state, h->n_train = n_train, h->any_bn = any_bn;
    MlpTrainArgs &a = h->base;
    a.scratch_floats = TrainScratch{d->n_layers, d->n_blocks, d->max_batch}.floats();
    const size_t E = (size_t)d->n_models;
    void *layers = nullptr;
    if (trainer_alloc(h, (void **)&a.state, E * n_state * 4, false) || trainer_alloc(h, (void **)&a.best, E * n_state * 4, false) ||
        trainer_alloc(h, (void **)&a.grad, E * n_train * 4, true) || trainer_alloc(h, (void **)&a.m, E * n_train * 4, true) ||
        trainer_alloc(h, (void **)&a.v, E * n_train * 4, true) || trainer_alloc(h, (void **)&a.scratch, E * (size_t)a.scratch_floats * 4, true) ||
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
    a.n_state = n_state, a.n_train = n_train, a.max_batch = d->max_batch;
    a.loss_kind = d->loss, a.opt_kind = d->optimizer, a.in_dim = L[0].in_dim, a.out_dim = L.back().out_dim;
    a.use_lds = n_state <= kTrainLdsFloats;
    h->initial.assign(d->state, d->state + E * n_state);
    h->structure.assign(d->layers, d->layers + d->n_layers);
    h->blob_floats = mlp_blob_layout(d->layers, d->n_layers, d->n_blocks, d->layers_per_block, nullptr, nullptr);
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
    if (which < 0 || which > 4)
        return fail("wtk_mlp_trainer_get_state: which must be 0 (state), 1 (best state), 2 (first moment), 3 (second moment) or 4 (best state by score)");
    DEVICE_GUARD(h);
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    const MlpTrainArgs &a = h->base;
    if (which == 4 && !h->scored) { // no score yet: the initial state
        std::memcpy(state_host, h->initial.data(), h->initial.size() * sizeof(float));
        if (steps_host) std::memset(steps_host, 0, (size_t)h->n_models * 4);
        return 0;
    }
    const float *src = which == 0 ? a.state : which == 1 ? a.best : which == 2 ? a.m : which == 3 ? a.v : h->scored;
    const size_t per = (which <= 1 || which == 4) ? h->n_state : h->n_train;
    HIP_TRY(hipMemcpy(state_host, src, (size_t)h->n_models * per * 4, hipMemcpyDeviceToHost));
    if (steps_host) HIP_TRY(hipMemcpy(steps_host, which == 1 ? a.best_steps : which == 4 ? h->scored_steps : a.steps, (size_t)h->n_models * 4, hipMemcpyDeviceToHost));
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

// =====================================================================================================================================================
// Folding a population for inference, and keeping the best state by a caller's score
// =====================================================================================================================================================
extern "C" int64_t wtk_mlp_folded_floats(const wtk_mlp_train_layer *layers, int32_t n_layers, int32_t n_blocks, int32_t layers_per_block) {
    return mlp_blob_layout(layers, n_layers, n_blocks, layers_per_block, nullptr, nullptr);
}

extern "C" int wtk_mlp_fold_state_host(const wtk_mlp_train_layer *layers, int32_t n_layers, int32_t n_blocks, int32_t layers_per_block, const float *state_host,
                                       float *blob_host) {
    if (!layers || !state_host || !blob_host) return fail("wtk_mlp_fold_state_host: null argument");
    const char *why = "";
    std::vector<MlpLayerDev> B(n_layers > 0 ? n_layers : 0);
    const int64_t F = mlp_blob_layout(layers, n_layers, n_blocks, layers_per_block, B.data(), &why);
    if (F < 0) return fail(std::string("wtk_mlp_fold_state_host: ") + why);
    std::vector<MlpTrainLayerDev> T(n_layers);
    for (int i = 0; i < n_layers; ++i) T[i] = MlpTrainLayerDev{}, T[i].in_dim = layers[i].in_dim, T[i].out_dim = layers[i].out_dim, T[i].bn = layers[i].batch_norm ? 1 : 0;
    state_layout(layers, n_layers, nullptr, T.data());
    for (int i = 0; i < n_layers; ++i)
        for (int o = 0; o < B[i].out_pad; ++o) mlp_fold_row(T[i], B[i].w_off, o, state_host, blob_host);
    for (int64_t k = B[n_layers - 1].b_off + B[n_layers - 1].out_pad; k < F; ++k) blob_host[k] = 0.f;
    return 0;
}

extern "C" int wtk_mlp_trainer_fold(wtk_mlp_trainer *h, int32_t which, float *blob_dev, void *stream) {
    if (!h || !blob_dev) return fail("wtk_mlp_trainer_fold: null argument");
    if (which != 0 && which != 1 && which != 4) return fail("wtk_mlp_trainer_fold: which must be 0 (state), 1 (best state) or 4 (best state by score)");
    if (h->blob_floats < 0) return fail("wtk_mlp_trainer_fold: the structure has no inference blob (wtk_mlp_folded_floats)");
    if (which == 4 && !h->scored) return fail("wtk_mlp_trainer_fold: no state was kept by score yet (wtk_mlp_trainer_keep_scored)");
    DEVICE_GUARD(h);
    const MlpTrainArgs &a = h->base;
    const float *src = which == 0 ? a.state : which == 1 ? a.best : h->scored;
    hipLaunchKernelGGL(mlp_fold_kernel, dim3(h->n_models, a.n_layers), dim3(kMlpMaxDim), 0, (hipStream_t)stream, src, h->n_state, a.layers, a.n_layers, blob_dev,
                       (int)h->blob_floats);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int wtk_mlp_trainer_keep_scored(wtk_mlp_trainer *h, const double *score_dev, const int32_t *active_dev, void *stream) {
    if (!h || !score_dev) return fail("wtk_mlp_trainer_keep_scored: null argument");
    DEVICE_GUARD(h);
    const size_t E = (size_t)h->n_models;
    if (!h->scored) { // the first call allocates the slot and fills it with the initial state
        float *scored = nullptr;
        if (trainer_alloc(h, (void **)&scored, E * h->n_state * 4, false) || trainer_alloc(h, (void **)&h->scored_steps, E * 4, true) ||
            trainer_alloc(h, (void **)&h->has_score, E * 4, true) || trainer_alloc(h, (void **)&h->best_score, E * 8, true))
            return 1;
        HIP_TRY(hipMemcpy(scored, h->initial.data(), E * h->n_state * 4, hipMemcpyHostToDevice));
        h->scored = scored;
    }
    const MlpTrainArgs &a = h->base;
    hipLaunchKernelGGL(mlp_keep_scored_kernel, dim3(h->n_models), dim3(256), 0, (hipStream_t)stream, a.state, h->n_state, a.steps, score_dev, active_dev, h->scored,
                       h->scored_steps, h->best_score, h->has_score);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int wtk_mlp_trainer_get_scores(wtk_mlp_trainer *h, double *best_score_host, int32_t *has_score_host, void *stream) {
    if (!h || !best_score_host || !has_score_host) return fail("wtk_mlp_trainer_get_scores: null argument");
    DEVICE_GUARD(h);
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    if (!h->scored) {
        for (int e = 0; e < h->n_models; ++e) best_score_host[e] = NAN, has_score_host[e] = 0;
        return 0;
    }
    HIP_TRY(hipMemcpy(best_score_host, h->best_score, (size_t)h->n_models * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(has_score_host, h->has_score, (size_t)h->n_models * 4, hipMemcpyDeviceToHost));
    for (int e = 0; e < h->n_models; ++e)
        if (!has_score_host[e]) best_score_host[e] = NAN; // no score stored yet
    return 0;
}
