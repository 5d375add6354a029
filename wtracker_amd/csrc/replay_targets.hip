// The per-cycle Polyfit targets of a whole POPULATION of weight vectors (the weight search's position buffer, on the device) in ONE call, in the layout
// replay.hip's scan reads.  The <= 16 x 8 SVD of a fit depends on the weights and on WHICH samples of the cycle are finite only, so
// the cycles are grouped by that set (a <= 16-bit mask; the caller derives the classes from the track once): pass A solves one SVD per (class, particle)
// and keeps the rotated matrix, V, s^2, scl and the compacted weights particle-minor in scratch; pass B, one thread per (cycle, particle), reads its
// class's record and the cycle's centres (LDS: one cycle per block) and solves and evaluates.  Both passes call the functions track_polyfit_kernel calls
// (polyfit_solve.h: polyfit_factor, polyfit_eval_axes), so the targets have that kernel's bits.
// A nullable stop flag (the swarm's ctrl word) turns both launches into no-ops.
#include "wtk_internal.h"
#include "polyfit_solve.h"

using namespace wtk;

namespace {

struct PopArgs {
    const double *track; // [n_track][4] xywh
    int n_track, L;
    const double *weights; // [P][n_times]
    int P, C, n_times, degree, n_classes;
    int times[kTrackMaxTimes];
    double t_eval;
    const int *cycle_class; // [C]
    const int *class_mask;  // [n_classes]: bit j = sample j of the cycle is inside the track and has a finite centre
    double *rec;            // [n_classes][pop_record(n_times, K)][P]
    double *a;              // [C][P][2]
    int *valid;             // [C][P]
    const int *stop;
};

// fields of a (class, particle) record, each P doubles apart: L_rot [n_times][K], V [K][K], s2 [K], scl [K], compacted weights [n_times], converged
__host__ __device__ inline int pop_off_V(int n_times, int K) { return n_times * K; }
__host__ __device__ inline int pop_off_s2(int n_times, int K) { return n_times * K + K * K; }
__host__ __device__ inline int pop_off_scl(int n_times, int K) { return n_times * K + K * K + K; }
__host__ __device__ inline int pop_off_w(int n_times, int K) { return n_times * K + K * K + 2 * K; }
__host__ __device__ inline int pop_off_ok(int n_times, int K) { return n_times * K + K * K + 2 * K + n_times; }
__host__ __device__ inline int pop_record(int n_times, int K) { return n_times * K + K * K + 2 * K + n_times + 1; }

// a (class, particle) record as polyfit_eval_axes reads it; r points at the particle's first field
struct PopRecordView {
    const double *r;
    long long P;
    int n_times, K;
    __device__ __forceinline__ double L(int j, int e) const { return r[(j * K + e) * P]; }
    __device__ __forceinline__ double V(int q, int e) const { return r[(pop_off_V(n_times, K) + q * K + e) * P]; }
    __device__ __forceinline__ double s2(int e) const { return r[(pop_off_s2(n_times, K) + e) * P]; }
    __device__ __forceinline__ double scl(int q) const { return r[(pop_off_scl(n_times, K) + q) * P]; }
    __device__ __forceinline__ double w(int j) const { return r[(pop_off_w(n_times, K) + j) * P]; }
};

// Pass A of the population targets: one thread per (class, particle).  The factor of the samples the class keeps; the record is written particle-minor
// (a wave of consecutive particles writes consecutive addresses).
__global__ __launch_bounds__(64) void replay_polyfit_solve_kernel(const PopArgs a) {
    if (a.stop && *a.stop) return;
    const int PB = (a.P + 63) / 64;
    const int k = blockIdx.x / PB, p = (blockIdx.x - k * PB) * 64 + threadIdx.x;
    if (p >= a.P) return;
    const int K = a.degree + 1;
    const unsigned mask = (unsigned)a.class_mask[k] & ((1u << a.n_times) - 1u);
    double tt[kTrackMaxTimes], ww[kTrackMaxTimes];
    int n = 0;
    for (int j = 0; j < a.n_times; ++j)
        if ((mask >> j) & 1u) tt[n] = (double)a.times[j], ww[n] = a.weights[(long long)p * a.n_times + j], ++n;
    if (n == 0) return; // no sample: pass B writes valid = 0 without looking at the record
    double *r = a.rec + (long long)k * pop_record(a.n_times, K) * a.P + p; // field f of this record: r[f * P]
    const long long P = a.P;
    PolyfitFactor fit;
    const bool ok = polyfit_factor(fit, tt, ww, n, K);
    r[pop_off_ok(a.n_times, K) * P] = ok ? 1.0 : 0.0;
    if (!ok) return; // every cycle of this class and particle: valid = 0
    for (int e = 0; e < K; ++e) {
        r[(pop_off_s2(a.n_times, K) + e) * P] = fit.s2[e];
        r[(pop_off_scl(a.n_times, K) + e) * P] = fit.scl[e];
    }
    for (int j = 0; j < n; ++j) {
        r[(pop_off_w(a.n_times, K) + j) * P] = ww[j];
        for (int e = 0; e < K; ++e) r[(j * K + e) * P] = fit.L[j][e];
    }
    for (int q = 0; q < K; ++q)
        for (int e = 0; e < K; ++e) r[(pop_off_V(a.n_times, K) + q * K + e) * P] = fit.V[q][e];
}

// Pass B: one thread per (cycle, particle), one cycle per block, so the cycle's centres are read once into LDS.  The samples found in the track are
// compared with the class's mask: a cycle whose class does not describe it (a class table of another track) gets valid = 0, never a fit of the wrong samples.
__global__ __launch_bounds__(64) void replay_polyfit_eval_kernel(const PopArgs a) {
    __shared__ double px[kTrackMaxTimes], py[kTrackMaxTimes];
    __shared__ int stale;
    if (a.stop && *a.stop) return; // block-uniform
    const int PB = (a.P + 63) / 64;
    const int c = blockIdx.x / PB, p = (blockIdx.x - c * PB) * 64 + threadIdx.x;
    const int K = a.degree + 1;
    const int k = a.cycle_class[c];
    const bool known = k >= 0 && k < a.n_classes;
    const unsigned mask = known ? (unsigned)a.class_mask[k] & ((1u << a.n_times) - 1u) : 0u;
    if (threadIdx.x == 0) stale = known ? 0 : 1;
    __syncthreads();
    if ((int)threadIdx.x < a.n_times) {
        const int j = threadIdx.x;
        const long long f = (long long)c * a.L + a.times[j];
        double cx = 0.0, cy = 0.0;
        bool finite = f >= 0 && f < a.n_track;
        if (finite) {
            const double x = a.track[4 * f + 0], y = a.track[4 * f + 1], w = a.track[4 * f + 2], h = a.track[4 * f + 3];
            cx = x + w / 2; // BoxUtils.center
            cy = y + h / 2;
            finite = isfinite(cx) && isfinite(cy);
        }
        if (finite != (((mask >> j) & 1u) != 0u)) {
            stale = 1; // every writer writes the same value
        } else if (finite) {
            const int slot = __popc(mask & ((1u << j) - 1u)); // the compaction: samples in time order
            px[slot] = cx, py[slot] = cy;
        }
    }
    __syncthreads();
    if (p >= a.P) return;
    const long long P = a.P, cp = (long long)c * P + p;
    const int n = __popc(mask);
    const double *r = a.rec + (long long)(known ? k : 0) * pop_record(a.n_times, K) * P + p;
    if (stale || n == 0 || r[pop_off_ok(a.n_times, K) * P] == 0.0) {
        a.a[2 * cp] = a.a[2 * cp + 1] = 0.0;
        a.valid[cp] = 0;
        return;
    }
    double x, y;
    polyfit_eval_axes(PopRecordView{r, P, a.n_times, K}, px, py, n, K, a.t_eval, x, y);
    a.a[2 * cp] = x;
    a.a[2 * cp + 1] = y;
    a.valid[cp] = 1;
}

} // namespace

extern "C" int64_t wtk_replay_polyfit_targets_scratch_doubles(int32_t n_classes, int32_t P, int32_t n_times, int32_t degree) {
    if (n_classes < 0 || P < 0 || n_times < 1 || n_times > kTrackMaxTimes || degree < 0 || degree + 1 > kTrackMaxCoef) return -1;
    return (int64_t)n_classes * pop_record(n_times, degree + 1) * P;
}

extern "C" int wtk_replay_polyfit_targets(const double *track_dev, int32_t n_track, int32_t n_cycles, int32_t cycle_frame_num, const double *weights_dev,
                                          int32_t P, const int32_t *sample_times_host, int32_t n_times, int32_t degree, double t_eval,
                                          const int32_t *cycle_class_dev, const int32_t *class_mask_dev, int32_t n_classes, double *a_dev,
                                          int32_t *valid_dev, double *scratch_dev, int64_t scratch_doubles, const int32_t *stop_dev, void *stream) {
    if (!track_dev || !weights_dev || !sample_times_host || !cycle_class_dev || !class_mask_dev || !a_dev || !valid_dev || !scratch_dev)
        return fail("wtk_replay_polyfit_targets: null argument");
    if (check_fit_shape("wtk_replay_polyfit_targets", n_times, degree)) return 1;
    if (P < 1 || P > 65535) return fail("wtk_replay_polyfit_targets: need 1 <= P <= 65535 weight vectors");
    if (n_track < 0 || n_cycles < 1 || cycle_frame_num <= 0) return fail("wtk_replay_polyfit_targets: need n_track >= 0, n_cycles >= 1 and a positive cycle_frame_num");
    if (n_classes < 1 || n_classes > n_cycles) return fail("wtk_replay_polyfit_targets: need 1 <= n_classes <= n_cycles");
    if (scratch_doubles < wtk_replay_polyfit_targets_scratch_doubles(n_classes, P, n_times, degree))
        return fail("wtk_replay_polyfit_targets: scratch smaller than wtk_replay_polyfit_targets_scratch_doubles(n_classes, P, n_times, degree)");
    const long long PB = (P + 63) / 64;
    if (PB * n_cycles > INT32_MAX) return fail("wtk_replay_polyfit_targets: too many (cycle, particle) blocks for one launch");
    PopArgs a = {};
    a.track = track_dev, a.n_track = n_track, a.L = cycle_frame_num, a.weights = weights_dev, a.P = P, a.C = n_cycles, a.n_times = n_times, a.degree = degree;
    a.n_classes = n_classes, a.t_eval = t_eval, a.cycle_class = cycle_class_dev, a.class_mask = class_mask_dev, a.rec = scratch_dev, a.a = a_dev;
    a.valid = valid_dev, a.stop = stop_dev;
    for (int i = 0; i < kTrackMaxTimes; ++i) a.times[i] = i < n_times ? sample_times_host[i] : 0;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(replay_polyfit_solve_kernel, dim3((unsigned)(PB * n_classes)), dim3(64), 0, st, a);
    hipLaunchKernelGGL(replay_polyfit_eval_kernel, dim3((unsigned)(PB * n_cycles)), dim3(64), 0, st, a);
    HIP_TRY(hipGetLastError());
    return 0;
}
