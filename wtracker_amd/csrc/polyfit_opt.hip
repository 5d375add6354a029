// Weight search for the polynomial-fit controller on the device: the reference's WeightEvaluator (wtracker/sim/sim_controllers/
// polyfit_controller.py:87-221: dataset of per-cycle head centres, mean absolute error of a weighted fit extrapolated to the target time) for MANY
// weight vectors per call, and the step of a particle swarm over them (what polyfit_optimizer.ipynb asks mealpy for).
//
// Dataset   one block walks the candidate cycles of a track 1024 at a time: flag (times in range, 2N + 2 finite centres, speed window) ->
//           block scan -> scatter, so the kept cycles land in cycle order behind the *count_dev series that are already there.
// MAE       all series share one time axis, so fit-then-extrapolate is ONE linear functional per weight vector w and degree d:
//           y_pred[m] = sum_n g_n y_input[n][m],  g = v(t_pred)^T pinv(diag(w) V / scl) diag(w) / scl  (V the Vandermonde matrix of the sample
//           times, scl its weighted column norms), from polyfit_solve.h's N x (d + 1) factor with numpy's cut (singular values <= N eps s_max dropped).
//             rows kernel    one thread per candidate: g[16] (all NaN when the weights are not finite or the solver did not converge)
//             mae kernel     block (chunk s, candidate p): sum over the chunk's kMaeChunk series of |y_target - sum_n g_n y_input[n]|, g from LDS,
//                            reads coalesced along the series axis, lane-serial partial sums, then a fixed tree
//             finish kernel  one thread per candidate adds the chunk partials in index order and divides by M  (M = 0: 0 / 0 = NaN, np.mean's)
//           No floating-point atomics and no dependence on P or on the block schedule: the same weights give the same bits in every call.
// Swarm     one single-block launch per epoch: personal bests (strict <), global best (lowest particle index among equals), the stall counter and
//           the stop flag, then the inertia-weight velocity / position update from host-supplied random numbers.  Once the stop flag is up the
//           evaluation kernels and the step return at once, so all epochs can be enqueued back to back without a host round trip.
#include "wtk_internal.h"
#include "polyfit_solve.h"

#include <climits>
#include <cmath>

using namespace wtk;

namespace {

constexpr int kDsThreads = 1024;  // candidate cycles per pass of the dataset block
constexpr int kMaeThreads = 256;
constexpr int kMaeChunk = 4096;   // series per block of the mae kernel: the FIXED chunking of the reduction
constexpr int kSwarmThreads = 256;

struct DatasetArgs {
    const void *track; // [n_frames][4] xywh, float or double
    int n_frames, cycle_frame_num;
    int times[kTrackMaxTimes]; // sorted input offsets from the start of a cycle
    int n_times, pred_offset;
    double min_speed, max_speed;
    double *y_input;  // [n_times][ld]
    double *y_target; // [ld]
    long long ld;     // row stride of y_input in doubles (= 2 * capacity in cycles)
    int capacity;     // cycles the buffers hold
    int *count;       // in: cycles already in the buffers; out: + the cycles kept here (may exceed capacity: nothing is written past it)
};

struct RowsArgs {
    const double *weights; // [P][n_times]
    int P, n_times, degree;
    int times[kTrackMaxTimes];
    double t_pred;
    double *g; // [P][kTrackMaxTimes]
    const int *stop;
};

struct MaeArgs {
    const double *g;       // [P][kTrackMaxTimes]
    const double *y_input; // [n_times][ld]
    const double *y_target;
    long long ld;
    int M, n_times, P, S;
    double *partial; // [P][S]
    double *mae;     // [P]
    const int *stop;
};

struct SwarmArgs {
    const double *mae;  // [P]
    const double *rand; // [2][P][N] of this epoch, uniform in [0, 1)
    int P, N, epoch, max_early_stop;
    double w, c1, c2, lb, ub, vmax;
    double *pos, *vel, *pbest_pos, *pbest_val; // [P][N] x 3, [P]
    double *gbest_pos, *gbest_val;             // [N], [1]
    int *ctrl;                                 // [4]: stop flag, epochs since the last improvement, epochs run, particle of the global best
    double *history;                           // [epoch] = best MAE so far
};

template <typename T> __device__ __forceinline__ void center_of(const T *track, long long f, double &cx, double &cy) {
    const double x = (double)track[4 * f + 0], y = (double)track[4 * f + 1], w = (double)track[4 * f + 2], h = (double)track[4 * f + 3];
    cx = x + w / 2; // BoxUtils.center
    cy = y + h / 2;
}

// WeightEvaluator._extract_positions (polyfit_controller.py:145-188), cycles in order
template <typename T> __global__ __launch_bounds__(kDsThreads) void polyfit_dataset_kernel(const DatasetArgs a) {
    __shared__ int wave_sum[kDsThreads / 64];
    __shared__ int base;
    const T *track = reinterpret_cast<const T *>(a.track);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long n_cycles = ((long long)a.n_frames + a.cycle_frame_num - 1) / a.cycle_frame_num;
    if (threadIdx.x == 0) base = *a.count;
    __syncthreads();
    for (long long c0 = 0; c0 < n_cycles; c0 += kDsThreads) { // block-uniform trip count
        const long long c = c0 + threadIdx.x, start = c * a.cycle_frame_num, ft = start + a.pred_offset;
        bool keep = c < n_cycles && ft >= 0 && ft < a.n_frames;
        for (int j = 0; keep && j < a.n_times; ++j) {
            const long long f = start + a.times[j];
            keep = f >= 0 && f < a.n_frames; // f >= n_frames cannot happen for the offsets the entry point admits; never read past the track
        }
        double px[kTrackMaxTimes], py[kTrackMaxTimes], tx = 0.0, ty = 0.0;
        if (keep) {
            center_of(track, ft, tx, ty);
            keep = isfinite(tx) && isfinite(ty);
            for (int j = 0; j < a.n_times; ++j) {
                center_of(track, start + a.times[j], px[j], py[j]);
                keep = keep && isfinite(px[j]) && isfinite(py[j]);
            }
        }
        if (keep) { // np.linalg.norm(target - first input) / (pred offset - first offset): x * x + y * y, no contraction (-ffp-contract=off)
            const double dx = tx - px[0], dy = ty - py[0];
            const double speed = sqrt(dx * dx + dy * dy) / (double)(a.pred_offset - a.times[0]);
            keep = speed >= a.min_speed && speed <= a.max_speed;
        }
        // exclusive scan of the flags in thread (= cycle) order: ballot inside the wave, the 16 wave totals through LDS
        const unsigned long long mask = __ballot(keep);
        const int before = __popcll(mask & ((1ull << lane) - 1ull));
        if (lane == 0) wave_sum[wave] = __popcll(mask);
        __syncthreads();
        int offset = base, total = 0;
        for (int wv = 0; wv < kDsThreads / 64; ++wv) {
            const int s = wave_sum[wv];
            offset += wv < wave ? s : 0;
            total += s;
        }
        const long long slot = (long long)offset + before;
        if (keep && slot < a.capacity) {
            for (int j = 0; j < a.n_times; ++j) a.y_input[j * a.ld + 2 * slot] = px[j], a.y_input[j * a.ld + 2 * slot + 1] = py[j];
            a.y_target[2 * slot] = tx, a.y_target[2 * slot + 1] = ty;
        }
        __syncthreads(); // every thread has read base and wave_sum
        if (threadIdx.x == 0) base += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) *a.count = base;
}

// numpy.polynomial.polynomial.polyfit(x, ., deg, w) followed by polyval at t_pred, as the row g the data are multiplied with: polyfit_solve.h's factor,
// then the functional instead of a right-hand side
__global__ __launch_bounds__(64) void polyfit_rows_kernel(const RowsArgs a) {
    if (a.stop && *a.stop) return;
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= a.P) return;
    const int n = a.n_times, K = a.degree + 1;
    double *g = a.g + (long long)p * kTrackMaxTimes;
    double tt[kTrackMaxTimes], ww[kTrackMaxTimes];
    bool finite = true;
    for (int j = 0; j < n; ++j) tt[j] = (double)a.times[j], ww[j] = a.weights[(long long)p * n + j], finite = finite && isfinite(ww[j]);
    PolyfitFactor fit;
    if (!finite || !polyfit_factor(fit, tt, ww, n, K)) { // no silent number: the candidate's MAE becomes NaN
        for (int j = 0; j < kTrackMaxTimes; ++j) g[j] = nan("");
        return;
    }
    // z_e = (v(t_pred) / scl) . V[:, e] / s_e^2 for the directions numpy keeps; g_j = w_j sum_e L_rot[j][e] z_e
    double z[kTrackMaxCoef];
    for (int e = 0; e < K; ++e) {
        z[e] = 0.0;
        if (!polyfit_keeps(fit.s2[e], fit.s2max, n)) continue;
        double tp = 1.0, acc = 0.0;
        for (int q = 0; q < K; ++q) acc += fit.V[q][e] * (tp / fit.scl[q]), tp *= a.t_pred;
        z[e] = acc / fit.s2[e];
    }
    for (int j = 0; j < kTrackMaxTimes; ++j) {
        double acc = 0.0;
        if (j < n)
            for (int e = 0; e < K; ++e) acc += fit.L[j][e] * z[e];
        g[j] = j < n ? ww[j] * acc : 0.0;
    }
}

__global__ __launch_bounds__(kMaeThreads) void polyfit_mae_kernel(const MaeArgs a) {
    __shared__ double gs[kTrackMaxTimes];
    __shared__ double red[kMaeThreads];
    if (a.stop && *a.stop) return; // block-uniform
    const int p = blockIdx.y, s = blockIdx.x;
    if (threadIdx.x < kTrackMaxTimes) gs[threadIdx.x] = a.g[(long long)p * kTrackMaxTimes + threadIdx.x];
    __syncthreads();
    double acc = 0.0;
    const long long m0 = (long long)s * kMaeChunk;
    for (int i = 0; i < kMaeChunk / kMaeThreads; ++i) {
        const long long m = m0 + (long long)i * kMaeThreads + threadIdx.x;
        if (m < a.M) {
            double pred = 0.0;
            for (int n = 0; n < a.n_times; ++n) pred += gs[n] * a.y_input[n * a.ld + m];
            acc += fabs(a.y_target[m] - pred);
        }
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int half = kMaeThreads / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) red[threadIdx.x] += red[threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x == 0) a.partial[(long long)p * a.S + s] = red[0];
}

__global__ __launch_bounds__(64) void polyfit_mae_finish_kernel(const MaeArgs a) {
    if (a.stop && *a.stop) return;
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p >= a.P) return;
    double sum = 0.0;
    for (int s = 0; s < a.S; ++s) sum += a.partial[(long long)p * a.S + s];
    a.mae[p] = sum / (double)a.M; // M = 0: 0 / 0 = NaN, as np.mean of an empty array
}

__global__ __launch_bounds__(kSwarmThreads) void polyfit_swarm_step_kernel(const SwarmArgs a) {
    __shared__ double best_v[kSwarmThreads];
    __shared__ int best_i[kSwarmThreads];
    __shared__ int stop_now;
    if (a.ctrl[0]) return; // stopped in an earlier epoch (block-uniform)
    const int tid = threadIdx.x;
    // personal bests: strictly lower only, so a NaN never replaces anything
    double bv = INFINITY;
    int bi = INT_MAX;
    for (int p = tid; p < a.P; p += kSwarmThreads) {
        const double v = a.mae[p];
        if (v < a.pbest_val[p]) {
            a.pbest_val[p] = v;
            for (int j = 0; j < a.N; ++j) a.pbest_pos[(long long)p * a.N + j] = a.pos[(long long)p * a.N + j];
        }
        const double pb = a.pbest_val[p];
        if (pb < bv) bv = pb, bi = p; // ascending p: the lowest index among equals stays
    }
    best_v[tid] = bv, best_i[tid] = bi;
    __syncthreads();
    for (int half = kSwarmThreads / 2; half > 0; half >>= 1) {
        if (tid < half) {
            const double ov = best_v[tid + half];
            const int oi = best_i[tid + half];
            if (ov < best_v[tid] || (ov == best_v[tid] && oi < best_i[tid])) best_v[tid] = ov, best_i[tid] = oi;
        }
        __syncthreads();
    }
    if (tid == 0) {
        int since = a.ctrl[1] + 1;
        if (best_v[0] < *a.gbest_val) {
            *a.gbest_val = best_v[0];
            a.ctrl[3] = best_i[0];
            for (int j = 0; j < a.N; ++j) a.gbest_pos[j] = a.pbest_pos[(long long)best_i[0] * a.N + j];
            since = 0;
        }
        a.ctrl[1] = since;
        a.ctrl[2] = a.epoch + 1;
        a.history[a.epoch] = *a.gbest_val;
        stop_now = since >= a.max_early_stop ? 1 : 0;
        if (stop_now) a.ctrl[0] = 1;
    }
    __syncthreads();
    if (stop_now) return;
    // v <- clamp(w v + c1 r1 (pbest - x) + c2 r2 (gbest - x), +-vmax);  x <- clip(x + v, lb, ub)   (no contraction: a numpy replay gives the same bits)
    const long long PN = (long long)a.P * a.N;
    for (long long i = tid; i < PN; i += kSwarmThreads) {
        const int j = (int)(i % a.N);
        const double x = a.pos[i];
        double v = a.w * a.vel[i] + (a.c1 * a.rand[i]) * (a.pbest_pos[i] - x);
        v = v + (a.c2 * a.rand[PN + i]) * (a.gbest_pos[j] - x);
        v = fmin(fmax(v, -a.vmax), a.vmax);
        a.vel[i] = v;
        a.pos[i] = fmin(fmax(x + v, a.lb), a.ub);
    }
}

int check_axis(const char *who, const int32_t *times_host, int32_t n_times) {
    if (!times_host) return fail(std::string(who) + ": null argument");
    if (check_fit_shape(who, n_times, 0)) return 1; // the axis alone: the dataset has no degree, wtk_polyfit_weight_mae checks its own next
    for (int i = 1; i < n_times; ++i)
        if (times_host[i] < times_host[i - 1]) return fail(std::string(who) + ": the sample times must be sorted");
    return 0;
}

} // namespace

extern "C" int wtk_polyfit_dataset(const void *track_dev, int32_t track_is_f64, int32_t n_frames, int32_t cycle_frame_num, const int32_t *input_offsets_host,
                                   int32_t n_times, int32_t pred_time_offset, double min_speed, double max_speed, double *y_input_dev, double *y_target_dev,
                                   int32_t capacity, int32_t *count_dev, void *stream) {
    if (!track_dev || !y_input_dev || !y_target_dev || !count_dev) return fail("wtk_polyfit_dataset: null argument");
    if (check_axis("wtk_polyfit_dataset", input_offsets_host, n_times)) return 1;
    if (n_frames < 0 || capacity < 0) return fail("wtk_polyfit_dataset: negative size");
    if (cycle_frame_num <= 0) return fail("wtk_polyfit_dataset: cycle_frame_num must be positive");
    if (pred_time_offset < input_offsets_host[n_times - 1])
        return fail("wtk_polyfit_dataset: the largest input offset lies beyond pred_time_offset (the input frames of the last cycles would lie past the end of the log)");
    if (pred_time_offset <= input_offsets_host[0]) return fail("wtk_polyfit_dataset: pred_time_offset must lie after the first input offset (the speed is measured over that span)");
    DatasetArgs a;
    a.track = track_dev, a.n_frames = n_frames, a.cycle_frame_num = cycle_frame_num, a.n_times = n_times, a.pred_offset = pred_time_offset;
    for (int i = 0; i < kTrackMaxTimes; ++i) a.times[i] = i < n_times ? input_offsets_host[i] : 0;
    a.min_speed = min_speed, a.max_speed = max_speed, a.y_input = y_input_dev, a.y_target = y_target_dev, a.ld = 2ll * capacity, a.capacity = capacity;
    a.count = count_dev;
    if (track_is_f64)
        hipLaunchKernelGGL(polyfit_dataset_kernel<double>, dim3(1), dim3(kDsThreads), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(polyfit_dataset_kernel<float>, dim3(1), dim3(kDsThreads), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int64_t wtk_polyfit_mae_scratch_doubles(int32_t P, int32_t M) {
    if (P < 0 || M < 0) return -1;
    return (int64_t)P * (kTrackMaxTimes + ((int64_t)M + kMaeChunk - 1) / kMaeChunk);
}

extern "C" int wtk_polyfit_weight_mae(const double *y_input_dev, const double *y_target_dev, int64_t ld, int32_t M, const int32_t *sample_times_host,
                                      int32_t n_times, int32_t pred_time_offset, int32_t degree, const double *weights_dev, int32_t P, double *mae_dev,
                                      double *scratch_dev, int64_t scratch_doubles, const int32_t *stop_dev, void *stream) {
    if (!weights_dev || !mae_dev || !scratch_dev) return fail("wtk_polyfit_weight_mae: null argument");
    if (check_axis("wtk_polyfit_weight_mae", sample_times_host, n_times)) return 1;
    if (check_fit_shape("wtk_polyfit_weight_mae", n_times, degree)) return 1;
    if (P < 0 || M < 0 || ld < M) return fail("wtk_polyfit_weight_mae: need P >= 0, M >= 0 and a row stride ld >= M");
    if (M > 0 && (!y_input_dev || !y_target_dev)) return fail("wtk_polyfit_weight_mae: null dataset");
    if (P > 65535) return fail("wtk_polyfit_weight_mae: at most 65535 weight vectors per call");
    if (scratch_doubles < wtk_polyfit_mae_scratch_doubles(P, M)) return fail("wtk_polyfit_weight_mae: scratch smaller than wtk_polyfit_mae_scratch_doubles(P, M)");
    if (P == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    RowsArgs r;
    r.weights = weights_dev, r.P = P, r.n_times = n_times, r.degree = degree, r.t_pred = (double)pred_time_offset, r.g = scratch_dev, r.stop = stop_dev;
    for (int i = 0; i < kTrackMaxTimes; ++i) r.times[i] = i < n_times ? sample_times_host[i] : 0;
    MaeArgs m;
    m.g = scratch_dev, m.y_input = y_input_dev, m.y_target = y_target_dev, m.ld = ld, m.M = M, m.n_times = n_times, m.P = P;
    m.S = (int)(((long long)M + kMaeChunk - 1) / kMaeChunk);
    m.partial = scratch_dev + (long long)P * kTrackMaxTimes, m.mae = mae_dev, m.stop = stop_dev;
    const dim3 per_candidate((unsigned)((P + 63) / 64));
    hipLaunchKernelGGL(polyfit_rows_kernel, per_candidate, dim3(64), 0, s, r);
    if (m.S > 0) hipLaunchKernelGGL(polyfit_mae_kernel, dim3((unsigned)m.S, (unsigned)P), dim3(kMaeThreads), 0, s, m);
    hipLaunchKernelGGL(polyfit_mae_finish_kernel, per_candidate, dim3(64), 0, s, m);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int wtk_polyfit_swarm_step(const double *mae_dev, const double *rand_dev, int32_t P, int32_t N, int32_t epoch, int32_t max_early_stop, double w,
                                      double c1, double c2, double lb, double ub, double vmax, double *pos_dev, double *vel_dev, double *pbest_pos_dev,
                                      double *pbest_val_dev, double *gbest_pos_dev, double *gbest_val_dev, int32_t *ctrl_dev, double *history_dev,
                                      void *stream) {
    if (!mae_dev || !rand_dev || !pos_dev || !vel_dev || !pbest_pos_dev || !pbest_val_dev || !gbest_pos_dev || !gbest_val_dev || !ctrl_dev || !history_dev)
        return fail("wtk_polyfit_swarm_step: null argument");
    if (P <= 0 || P > 65535 || N <= 0 || N > kTrackMaxTimes) return fail("wtk_polyfit_swarm_step: need 1 <= P <= 65535 particles of 1..16 weights");
    if (epoch < 0 || max_early_stop <= 0) return fail("wtk_polyfit_swarm_step: epoch must be >= 0 and max_early_stop positive");
    if (!(lb < ub) || !(vmax > 0.0) || !std::isfinite(lb) || !std::isfinite(ub)) return fail("wtk_polyfit_swarm_step: need finite bounds lb < ub and vmax > 0");
    SwarmArgs a;
    a.mae = mae_dev, a.rand = rand_dev, a.P = P, a.N = N, a.epoch = epoch, a.max_early_stop = max_early_stop;
    a.w = w, a.c1 = c1, a.c2 = c2, a.lb = lb, a.ub = ub, a.vmax = vmax;
    a.pos = pos_dev, a.vel = vel_dev, a.pbest_pos = pbest_pos_dev, a.pbest_val = pbest_val_dev, a.gbest_pos = gbest_pos_dev, a.gbest_val = gbest_val_dev;
    a.ctrl = ctrl_dev, a.history = history_dev;
    hipLaunchKernelGGL(polyfit_swarm_step_kernel, dim3(1), dim3(kSwarmThreads), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}
