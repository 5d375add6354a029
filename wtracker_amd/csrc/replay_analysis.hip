// The reference's analysis of a replayed population on the device: what DataAnalyzer.initialize / clean / change_unit / describe /
// calc_anomalies / print_stats (wtracker/eval/data_analyzer.py:54-107, 121-159, 178-213, 326-416) and the Plotter's per-cycle and per-cycle-step
// aggregates (wtracker/eval/plotter.py:164-168, 203-213, 237-245) compute from ONE log with pandas, for every experiment of a scan at once.
//
// Nothing of size [E][R][columns] is ever stored.  A row's columns are a few dozen flops away from the scan's pos / move (replay_row,
// row_bbox_error: the functions the rows kernel calls), so every kernel recomputes the value where it consumes it:
//   last     one block per experiment: the largest cycle number among the rows that survive imaging_only and bounds.  trim_cycles drops cycle 0 and THAT
//            cycle (DataAnalyzer.clean takes data["cycle"].max() after the first two filters), so the mask of a row is final only once this is known.
//   segment  the hot path: one workgroup per (experiment, column, segment), the segment being the whole experiment (describe) or one cycle step
//            (the distributions of plot_cycle_error).  Count, mean and std (two passes, about the computed mean) in a FIXED order: thread t adds the
//            segment's rows t, t + 512, ... in order, then a binary tree in LDS; the order depends on the row count alone, so an experiment gives the same
//            bits alone and in any population.  Order statistics, two ways that return the same bits:
//              sort    the kept non-NaN values as order-preserving 64-bit keys in dynamic LDS (up to 160 KiB: 19960 keys beside the tree's buffer), a
//                      bitonic network in which every comparator sends the smaller key to the lower index: with the indices >= n imagined to hold
//                      +infinity no comparator ever moves one of them, so leaving out the comparators that touch them sorts any n, a power of two or not.
//                      Then min, max and every requested rank are reads.
//              select  for segments longer than the LDS holds: a most-significant-digit radix select, 8 passes of 8 bits over the recomputed values,
//                      all ranks (min, max, both neighbours of every percentile) at once, a 256-bin histogram per rank in static LDS (integer atomics:
//                      the counts do not depend on the order of arrival).  It finds the key of each rank exactly.
//            The way is chosen on the host from the segment's row count (an upper bound of the kept count), so it is uniform over a launch.
//   cycle    one thread per (experiment, cycle, column): max and mean (rows in order) of the kept non-NaN values: groupby(["log_num", "cycle"]).
//   flags    one block per experiment: calc_anomalies' six masks per kept row (bit flags, optionally written out), their counts, print_stats' figures.
//            Integer counts only.
// Every value is written with plain C++ stores.  Everything relies on -ffp-contract=off and on HIP's float64 sqrt and division being the correctly
// rounded ones (they are without fast-math flags: OCML's sqrt refines the hardware estimate to the IEEE result).
// The statements of a row, of the sums and of the order statistics live in replay_analysis_device.h: the analysis of a set of logs calls them too.
#include "wtk_internal.h"
#include "replay_analysis_device.h"

#include <algorithm>
#include <cmath>

using namespace wtk;

namespace {

__global__ __launch_bounds__(kAnaThreads) void analysis_last_cycle_kernel(const AnaArgs a) {
    __shared__ int best[kAnaThreads];
    const int e = blockIdx.x;
    if (!a.c.use_bounds) { // imaging_only alone keeps step 0 of every cycle (block-uniform)
        if (threadIdx.x == 0) a.last_cycle[e] = a.v.n_log - 1;
        return;
    }
    int mine = -1;
    for (long long r = threadIdx.x; r < a.v.R; r += kAnaThreads) {
        const AnaRow w = ana_row(a, e, r);
        if (w.pre) mine = max(mine, w.c);
    }
    best[threadIdx.x] = mine;
    __syncthreads();
    for (int half = kAnaThreads / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) best[threadIdx.x] = max(best[threadIdx.x], best[threadIdx.x + half]);
        __syncthreads();
    }
    if (threadIdx.x == 0) a.last_cycle[e] = best[0];
}

// a (experiment, column, segment) workgroup's share of the work
struct Segment {
    int e, j, col, seg, last;
    long long n_rows; // rows of the segment, kept or not
    __device__ __forceinline__ long long row(long long k, int L) const { return seg < 0 ? k : seg + k * L; }
};

__device__ __forceinline__ Segment segment_of(const AnaArgs &a) {
    Segment s;
    const int n_seg = a.by_step ? a.v.g.L : 1;
    const int idx = blockIdx.x;
    const int sg = idx % n_seg;
    s.j = (idx / n_seg) % a.n_cols, s.e = idx / (n_seg * a.n_cols);
    s.col = a.cols[s.j], s.seg = a.by_step ? sg : -1;
    s.n_rows = a.by_step ? (a.v.R > sg ? (a.v.R - sg + a.v.g.L - 1) / a.v.g.L : 0) : a.v.R;
    s.last = a.c.trim_cycles ? a.last_cycle[s.e] : -1;
    return s;
}

// the k-th row of the segment: its value where the row is kept and the value is not NaN
__device__ __forceinline__ bool segment_value(const AnaArgs &a, const Segment &s, long long k, double &v) {
    const long long r = s.row(k, a.v.g.L);
    const AnaRow w = ana_row(a, s.e, r);
    if (!ana_keep(a, w, s.last)) return false;
    v = ana_value(a, w, r, s.col);
    return !isnan(v);
}

// thread 0 writes the segment's results: count, mean, std, min, percentiles, max (describe) or percentiles and count (cycle steps)
__device__ __forceinline__ void write_segment(const AnaArgs &a, const Segment &s, long long n, double mean, double ss, double vmin, double vmax, const double *pct) {
    const double nanv = __builtin_nan("");
    if (!a.by_step) {
        double *o = a.describe + ((long long)s.e * a.n_cols + s.j) * (5 + a.Q);
        o[0] = (double)n;
        o[1] = n > 0 ? mean : nanv;
        o[2] = n > 1 ? sqrt(ss / (double)(n - 1)) : nanv;
        o[3] = n > 0 ? vmin : nanv;
        for (int i = 0; i < a.Q; ++i) o[4 + i] = n > 0 ? pct[i] : nanv;
        o[4 + a.Q] = n > 0 ? vmax : nanv;
    } else {
        const long long at = ((long long)s.e * a.v.g.L + s.seg) * a.n_cols + s.j;
        if (a.step_count) a.step_count[at] = (int)n;
        if (a.step_q)
            for (int i = 0; i < a.Q; ++i) a.step_q[at * a.Q + i] = n > 0 ? pct[i] : nanv;
    }
}

// count, mean and the sum of squares about the mean of the segment, each thread over its rows in order.  kKeys: the values also go to LDS as keys.
template <bool kKeys>
__device__ __forceinline__ void segment_moments(const AnaArgs &a, const Segment &s, double *red, unsigned long long *keys, int *key_count, int max_keys,
                                                long long &n, double &mean, double &ss) {
    double sum = 0.0, cnt = 0.0;
    for (long long k = threadIdx.x; k < s.n_rows; k += kAnaThreads) {
        double v;
        if (!segment_value(a, s, k, v)) continue;
        sum += v, cnt += 1.0;
        if (kKeys) {
            const int at = atomicAdd(key_count, 1); // the order of arrival does not matter: the keys are sorted next
            if (at < max_keys) keys[at] = to_key(v);
        }
    }
    n = (long long)block_sum(red, cnt); // exact: counts are small integers
    mean = block_sum(red, sum) / (double)n;
    double part = 0.0;
    if (n > 1) {
        for (long long k = threadIdx.x; k < s.n_rows; k += kAnaThreads) {
            double v;
            if (segment_value(a, s, k, v)) part += (v - mean) * (v - mean);
        }
    }
    ss = block_sum(red, part);
}

__global__ __launch_bounds__(kAnaThreads) void analysis_segment_sort_kernel(const AnaArgs a, const int max_keys) {
    extern __shared__ unsigned long long lds64[];
    int *key_count = reinterpret_cast<int *>(lds64);
    double *red = reinterpret_cast<double *>(lds64 + kAnaHeaderWords);
    unsigned long long *keys = lds64 + kAnaHeaderWords + kAnaThreads;
    const Segment s = segment_of(a);
    if (threadIdx.x == 0) *key_count = 0;
    __syncthreads();
    long long n;
    double mean, ss;
    segment_moments<true>(a, s, red, keys, key_count, max_keys, n, mean, ss);
    const int m = min((int)n, max_keys); // n <= n_rows <= max_keys: the host chose this kernel for that
    for (int k = 2; (k >> 1) < m; k <<= 1) { // the bitonic network (replay_analysis_device.h)
        for (int i = threadIdx.x; i < m; i += kAnaThreads) bitonic_compare(keys, i, i ^ (k - 1), m);
        __syncthreads();
        for (int j = k >> 2; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < m; i += kAnaThreads) bitonic_compare(keys, i, i ^ j, m);
            __syncthreads();
        }
    }
    if (threadIdx.x == 0) {
        double pct[kMaxQ];
        for (int i = 0; i < a.Q && m > 0; ++i) {
            long long lo, hi;
            double t;
            percentile_rank(a.q[i], m, lo, hi, t);
            pct[i] = lerp_linear(from_key(keys[lo]), from_key(keys[hi]), t);
        }
        write_segment(a, s, m, mean, ss, m > 0 ? from_key(keys[0]) : 0.0, m > 0 ? from_key(keys[m - 1]) : 0.0, pct);
    }
}

__global__ __launch_bounds__(kAnaThreads) void analysis_segment_select_kernel(const AnaArgs a) {
    __shared__ double red[kAnaThreads];
    __shared__ unsigned hist[kMaxRanks][256];
    __shared__ unsigned long long prefix[kMaxRanks]; // the digits found so far, in place
    __shared__ long long remain[kMaxRanks];          // the rank among the values that share the prefix
    const Segment s = segment_of(a);
    long long n;
    double mean, ss;
    segment_moments<false>(a, s, red, nullptr, nullptr, 0, n, mean, ss);
    const int n_ranks = 2 + 2 * a.Q;
    if (n > 0) { // block-uniform; the radix select (replay_analysis_device.h)
        if ((int)threadIdx.x < n_ranks) radix_start(prefix, remain, a.q, n);
        for (int shift = 56; shift >= 0; shift -= 8) {
            for (int i = threadIdx.x; i < n_ranks * 256; i += kAnaThreads) hist[i >> 8][i & 255] = 0u;
            __syncthreads();
            for (long long k = threadIdx.x; k < s.n_rows; k += kAnaThreads) {
                double v;
                if (!segment_value(a, s, k, v)) continue;
                const unsigned long long key = to_key(v);
                const unsigned digit = (unsigned)(key >> shift) & 255u;
                for (int i = 0; i < n_ranks; ++i)
                    if (shift == 56 || ((key ^ prefix[i]) >> (shift + 8)) == 0ull) atomicAdd(&hist[i][digit], 1u);
            }
            __syncthreads();
            if ((int)threadIdx.x < n_ranks) radix_digit(hist, prefix, remain, shift);
            __syncthreads();
        }
    }
    if (threadIdx.x == 0) {
        double pct[kMaxQ];
        for (int i = 0; i < a.Q && n > 0; ++i) {
            long long lo, hi;
            double t;
            percentile_rank(a.q[i], n, lo, hi, t);
            pct[i] = lerp_linear(from_key(prefix[2 + 2 * i]), from_key(prefix[3 + 2 * i]), t);
        }
        write_segment(a, s, n, mean, ss, n > 0 ? from_key(prefix[0]) : 0.0, n > 0 ? from_key(prefix[1]) : 0.0, pct);
    }
}

// groupby(["log_num", "cycle"]) max / mean of every requested column over the kept rows: NaN where the cycle has no kept non-NaN value
__global__ __launch_bounds__(256) void analysis_cycle_kernel(const AnaArgs a) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)a.v.E * a.v.n_log * a.n_cols) return;
    const int j = (int)(idx % a.n_cols), c = (int)((idx / a.n_cols) % a.v.n_log), e = (int)(idx / ((long long)a.n_cols * a.v.n_log));
    const int last = a.c.trim_cycles ? a.last_cycle[e] : -1;
    double vmax = 0.0, sum = 0.0;
    int n = 0;
    for (int step = 0; step < a.v.g.L; ++step) {
        const long long r = (long long)c * a.v.g.L + step;
        const AnaRow w = ana_row(a, e, r);
        if (!ana_keep(a, w, last)) continue;
        const double v = ana_value(a, w, r, a.cols[j]);
        if (isnan(v)) continue;
        vmax = n == 0 ? v : fmax(vmax, v);
        sum += v, ++n;
    }
    const double nanv = __builtin_nan("");
    if (a.cycle_max) a.cycle_max[idx] = n > 0 ? vmax : nanv;
    if (a.cycle_mean) a.cycle_mean[idx] = n > 0 ? sum / (double)n : nanv;
}

// calc_anomalies and print_stats over the kept rows of one experiment; counts are integers, added with LDS atomics
__global__ __launch_bounds__(kAnaThreads) void analysis_flags_kernel(const AnaArgs a) {
    __shared__ int cnt[12]; // [0..5] the six anomaly kinds, [6] any, [7] kept rows, [8] no-pred rows, [9] rows with bbox_error > 1e-7, [10] cycles with a kept row
    const int e = blockIdx.x;
    if (threadIdx.x < 12) cnt[threadIdx.x] = 0;
    __syncthreads();
    const int last = a.c.trim_cycles ? a.last_cycle[e] : -1;
    for (long long r = threadIdx.x; r < a.v.R; r += kAnaThreads) {
        const AnaRow w = ana_row(a, e, r);
        unsigned bits = 0u;
        if (ana_keep(a, w, last)) {
            // on the values calc_anomalies sees: after change_unit; a comparison with NaN is false
            bits |= w.sp * a.c.speed_factor >= a.c.min_speed ? 1u : 0u;
            bits |= w.err >= a.c.min_bbox_error ? 2u : 0u;
            bits |= w.dev * a.c.dist_factor >= a.c.min_dist_error ? 4u : 0u;
            bits |= w.ww * a.c.dist_factor >= a.c.min_width ? 8u : 0u;
            bits |= w.wh * a.c.dist_factor >= a.c.min_height ? 16u : 0u;
            const bool finite = isfinite(w.wx) && isfinite(w.wy) && isfinite(w.ww) && isfinite(w.wh);
            bits |= (a.c.no_preds && !finite) ? 32u : 0u;
            for (int k = 0; k < 6; ++k)
                if ((bits >> k) & 1u) atomicAdd(&cnt[k], 1);
            if (bits) atomicAdd(&cnt[6], 1);
            atomicAdd(&cnt[7], 1);
            if (isnan(w.wx) || isnan(w.wy) || isnan(w.ww) || isnan(w.wh)) atomicAdd(&cnt[8], 1);
            if (w.err > 1e-7) atomicAdd(&cnt[9], 1);
        }
        if (a.anomaly_mask) a.anomaly_mask[(long long)e * a.v.R + r] = (uint8_t)bits;
    }
    for (int c = threadIdx.x; c < a.v.n_log; c += kAnaThreads) {
        bool any = false;
        for (int step = 0; step < a.v.g.L && !any; ++step) any = ana_keep(a, ana_row(a, e, (long long)c * a.v.g.L + step), last);
        if (any) atomicAdd(&cnt[10], 1);
    }
    __syncthreads();
    if (threadIdx.x < 7 && a.anomaly_counts) a.anomaly_counts[(long long)e * 7 + threadIdx.x] = cnt[threadIdx.x];
    if (threadIdx.x == 0 && a.stats) {
        long long *o = a.stats + (long long)e * 4;
        o[0] = a.v.R - cnt[7], o[1] = cnt[8], o[2] = cnt[10], o[3] = cnt[9];
    }
}

} // namespace

extern "C" int64_t wtk_replay_analysis_scratch_doubles(int32_t E, int64_t R, int32_t n_cols, int32_t Q) {
    if (E < 0 || R < 0 || n_cols < 0 || Q < 0) return -1;
    return ((int64_t)E + 1) / 2; // [E] int32: the last surviving cycle of every experiment
}

extern "C" int wtk_replay_analyze(const wtk_replay_config *cfg, const wtk_replay_analysis_config *acfg, int32_t E, int32_t n_cycles,
                                  const double *track_dev, int32_t n_track, const double *share_dev, const int32_t *pos_dev, const int32_t *move_dev,
                                  const double *precise_pair_dev, const int32_t *columns_host, int32_t n_cols, const double *percentiles_host, int32_t Q,
                                  int32_t max_lds_rows, double *describe_dev, double *cycle_max_dev, double *cycle_mean_dev, double *step_quantiles_dev,
                                  int32_t *step_count_dev, int64_t *anomaly_counts_dev, uint8_t *anomaly_mask_dev, int64_t *stats_dev, double *scratch_dev,
                                  int64_t scratch_doubles, void *stream) {
    const std::string w("wtk_replay_analyze");
    AnaArgs a = {};
    if (!acfg) return fail(w + ": null argument");
    if (replay_view("wtk_replay_analyze", cfg, WTK_REPLAY_OPTIMAL, E, n_cycles, track_dev, n_track, share_dev, pos_dev, move_dev, a.v)) return 1;
    if (!scratch_dev) return fail(w + ": null argument");
    if (analysis_spec(w, acfg, columns_host, n_cols, percentiles_host, Q, max_lds_rows, precise_pair_dev != nullptr, "precise_pair_dev", a.cols, a.q)) return 1;
    if (a.v.R > INT32_MAX || (long long)E * n_cols * a.v.g.L > INT32_MAX || ((long long)E * a.v.n_log * n_cols + 255) / 256 > INT32_MAX)
        return fail(w + ": too many blocks for one launch");
    if (scratch_doubles < wtk_replay_analysis_scratch_doubles(E, a.v.R, n_cols, Q)) return fail(w + ": scratch smaller than wtk_replay_analysis_scratch_doubles(E, R, n_cols, Q)");
    a.pair = precise_pair_dev, a.c = *acfg, a.n_cols = n_cols, a.Q = Q, a.last_cycle = reinterpret_cast<int *>(scratch_dev);
    a.describe = describe_dev, a.cycle_max = cycle_max_dev, a.cycle_mean = cycle_mean_dev, a.step_q = step_quantiles_dev, a.step_count = step_count_dev;
    a.anomaly_counts = reinterpret_cast<long long *>(anomaly_counts_dev), a.anomaly_mask = anomaly_mask_dev, a.stats = reinterpret_cast<long long *>(stats_dev);
    hipStream_t st = (hipStream_t)stream;
    const int max_keys = max_lds_rows == 0 ? kAnaMaxKeys : std::min((int)max_lds_rows, kAnaMaxKeys);
    const bool segments = describe_dev || step_quantiles_dev || step_count_dev;
    // above 64 KiB of dynamic LDS a kernel needs the attribute (per device, so it is set at every call: a host-side table write)
    if (segments) HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&analysis_segment_sort_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kAnaLdsBytes));
    if (a.c.trim_cycles) hipLaunchKernelGGL(analysis_last_cycle_kernel, dim3((unsigned)E), dim3(kAnaThreads), 0, st, a);
    for (int by_step = 0; by_step < 2; ++by_step) {
        if (by_step ? !(step_quantiles_dev || step_count_dev) : !describe_dev) continue;
        a.by_step = by_step;
        const long long seg_rows = by_step ? (long long)a.v.n_log : a.v.R; // the longest segment's rows: an upper bound of its kept values
        const unsigned grid = (unsigned)((long long)E * n_cols * (by_step ? a.v.g.L : 1));
        if (seg_rows <= max_keys) {
            const size_t lds = (size_t)(kAnaHeaderWords + kAnaThreads + std::max(seg_rows, 1ll)) * 8;
            hipLaunchKernelGGL(analysis_segment_sort_kernel, dim3(grid), dim3(kAnaThreads), lds, st, a, (int)std::max(seg_rows, 1ll));
        } else {
            hipLaunchKernelGGL(analysis_segment_select_kernel, dim3(grid), dim3(kAnaThreads), 0, st, a);
        }
    }
    a.by_step = 0;
    if ((cycle_max_dev || cycle_mean_dev) && a.v.n_log > 0)
        hipLaunchKernelGGL(analysis_cycle_kernel, dim3((unsigned)(((long long)E * a.v.n_log * n_cols + 255) / 256)), dim3(256), 0, st, a);
    if (anomaly_counts_dev || anomaly_mask_dev || stats_dev) hipLaunchKernelGGL(analysis_flags_kernel, dim3((unsigned)E), dim3(kAnaThreads), 0, st, a);
    HIP_TRY(hipGetLastError());
    return 0;
}
