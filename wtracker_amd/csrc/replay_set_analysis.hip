// The analysis of a population replayed on a SET of T tracks: what the reference's Plotter computes from several logs at once
// (wtracker/eval/plotter.py:37-40: every log through its own DataAnalyzer.initialize / clean / change_unit, the cleaned frames concatenated with a log_num
// column), for every experiment of a set scan.  Log (t, e) is replay_analysis.hip's experiment e on track t's ReplayView (built from the track table as
// replay_set_rows_kernel builds it) through replay_analysis_device.h's statements: frame, cycle and cycle_step count from the track's own row 0, the
// speed's diff(period) never reaches across a track boundary, and clean trims with THAT log's last surviving cycle.  Two results:
//   per track  every array of wtk_replay_analyze on the track alone, bit for bit, for any E, any T and any place of the track in the set
//   pooled     the same statistics over the concatenation of the T cleaned logs of experiment e, in track order
// Kernels (a fixed number of launches whatever T is):
//   prefix   one thread: row0[t] = the rows, log0[t] = the logged cycles of the tracks before t (the packed per-track outputs' offsets)
//   last     one block per (track, experiment): analysis_last_cycle_kernel on the track's view
//   segment  one workgroup per (track, experiment, column, segment), or (pooled) per (experiment, column, segment).  The workgroup walks its tracks in
//            order (one, or all T).  sum_t and n_t of track t as analysis_segment_*_kernel takes them (thread i adds the track's rows i, i + 512, ... in
//            order, then the binary tree); S = (...((sum_0 + sum_1) + sum_2)...) from the FIRST track that keeps a value (not from 0.0: one track keeps
//            the sign of a -0.0 sum), N = the sum of n_t, mean = S / N; ss_t about that pooled mean in the same order and chained the same way;
//            std = sqrt(SS / (N - 1)).  One track: wtk_replay_analyze's bits.  Order statistics over the union of the kept non-NaN values: all tracks'
//            keys in ONE LDS sort where the segment's rows of all tracks fit the key buffer, else the radix select over the recomputed values of all
//            tracks; both return the same bits.  The way is chosen on the host, uniform per launch: by the longest track for the per-track launches,
//            by the sum over the tracks for the pooled ones.
//   cycle    one thread per (experiment, logged cycle of any track, column): groupby(["log_num", "cycle"]) max and mean
//   flags    one block per (track, experiment): calc_anomalies' masks and counts, print_stats' figures;  pool: their integer sums over the tracks
// No floating-point atomics; every value is written with plain C++ stores.
#include "wtk_internal.h"
#include "replay_analysis_device.h"
#include "replay_set_device.h"

#include <algorithm>

using namespace wtk;

namespace {

constexpr int kFlagCounts = 11; // analysis_flags_kernel's counters: six anomaly kinds, any, kept rows, no-pred rows, rows with bbox_error > 1e-7, cycles kept

struct SetAnaArgs {
    SetArgs s;              // the view of the scanned set
    const double *err;      // [E][rows] precise error of every row, NaN = no value (nullable): wtk_replay_set_precise's err_dev
    long long rows, logs;   // logged rows and logged cycles of all tracks
    wtk_replay_analysis_config c;
    int n_cols, Q;
    int cols[kMaxCols];
    double q[kMaxQ];
    int by_step, pooled;    // the segment launch: one segment per cycle step / over all tracks
    long long *row0, *log0; // [T + 1] scratch: prefix sums of R and n_log
    int *last_cycle;        // [T][E] scratch
    long long *flag_counts; // [T][E][kFlagCounts] scratch
    // per track, packed over the tracks
    double *t_describe;             // [T][E][n_cols][5 + Q]
    double *cycle_max, *cycle_mean; // [E][logs][n_cols]: track t's cycles from log0[t]
    double *t_step_q;               // [T][E][L][n_cols][Q]
    int *t_step_count;              // [T][E][L][n_cols]
    long long *t_anomaly_counts;    // [T][E][7]
    uint8_t *anomaly_mask;          // [E][rows]: track t's rows from row0[t]
    long long *t_stats;             // [T][E][4]
    // pooled
    double *describe;          // [E][n_cols][5 + Q]
    double *step_q;            // [E][L][n_cols][Q]
    int *step_count;           // [E][L][n_cols]
    long long *anomaly_counts; // [E][7]
    long long *stats;          // [E][4]
};

__global__ void set_analysis_prefix_kernel(const SetAnaArgs a) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    long long rows = 0, logs = 0;
    for (int t = 0; t < a.s.T; ++t) {
        a.row0[t] = rows, a.log0[t] = logs;
        rows += a.s.tracks[t].R, logs += a.s.tracks[t].n_log;
    }
    a.row0[a.s.T] = rows, a.log0[a.s.T] = logs;
}

// track t (entry `tr`) as wtk_replay_analyze's arguments: its view and the spec (the statements of a row read nothing else).  With a geometry table
// the spec's change_unit factors are the track's own: every statement below that converts a value reads them from here, never from a.c.
__device__ __forceinline__ AnaArgs track_args(const SetAnaArgs &a, int t, const wtk_replay_set_track &tr) {
    AnaArgs p = {};
    p.v = track_view(a.s, t, tr), p.pair = nullptr, p.c = a.c;
    if (a.s.geom) {
        const wtk_replay_set_geometry tg = a.s.geom[t];
        p.c.time_factor = tg.time_factor, p.c.dist_factor = tg.dist_factor, p.c.speed_factor = tg.speed_factor;
    }
    return p;
}

// row r of log (track, e); the precise error comes from the set's per-row buffer, unrounded (the track's rows start at row0)
__device__ __forceinline__ AnaRow set_row(const SetAnaArgs &a, const AnaArgs &p, long long row0, int e, long long r) {
    AnaRow w = ana_row(p, e, r);
    if (a.err) w.precise = a.err[(long long)e * a.rows + row0 + r];
    return w;
}

__global__ __launch_bounds__(kAnaThreads) void set_analysis_last_cycle_kernel(const SetAnaArgs a) {
    __shared__ int best[kAnaThreads];
    const int t = blockIdx.x / a.s.E, e = blockIdx.x - t * a.s.E;
    const wtk_replay_set_track tr = a.s.tracks[t];
    if (!a.c.use_bounds) { // imaging_only alone keeps step 0 of every cycle (block-uniform)
        if (threadIdx.x == 0) a.last_cycle[blockIdx.x] = tr.n_log - 1;
        return;
    }
    const AnaArgs p = track_args(a, t, tr);
    int mine = -1;
    for (long long r = threadIdx.x; r < p.v.R; r += kAnaThreads) {
        const AnaRow w = ana_row(p, e, r); // (the precise error is no part of clean)
        if (w.pre) mine = max(mine, w.c);
    }
    best[threadIdx.x] = mine;
    __syncthreads();
    for (int half = kAnaThreads / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) best[threadIdx.x] = max(best[threadIdx.x], best[threadIdx.x + half]);
        __syncthreads();
    }
    if (threadIdx.x == 0) a.last_cycle[blockIdx.x] = best[0];
}

// a workgroup's share of a segment launch: experiment, column, segment, and the tracks [t0, t1) it walks (one track, or all of them)
struct SetSegment {
    int e, j, col, seg, t0, t1;
};

__device__ __forceinline__ SetSegment set_segment_of(const SetAnaArgs &a) {
    SetSegment s;
    const int n_seg = a.by_step ? a.s.g.L : 1;
    const int idx = blockIdx.x;
    const int sg = idx % n_seg;
    s.j = (idx / n_seg) % a.n_cols, s.e = (idx / (n_seg * a.n_cols)) % a.s.E;
    const int t = idx / (n_seg * a.n_cols * a.s.E); // (0 in a pooled launch: its grid holds no track)
    s.col = a.cols[s.j], s.seg = a.by_step ? sg : -1;
    s.t0 = a.pooled ? 0 : t, s.t1 = a.pooled ? a.s.T : t + 1;
    return s;
}

// one track's part of a segment
struct TrackPart {
    AnaArgs p;
    long long row0, n_rows; // the track's first global row; rows of the segment in this track, kept or not
    int last;
};

__device__ __forceinline__ TrackPart track_part(const SetAnaArgs &a, const SetSegment &s, int t) {
    const wtk_replay_set_track tr = a.s.tracks[t];
    TrackPart tp;
    tp.p = track_args(a, t, tr), tp.row0 = a.row0[t];
    tp.n_rows = s.seg < 0 ? tr.R : (tr.R > s.seg ? (tr.R - s.seg + a.s.g.L - 1) / a.s.g.L : 0);
    tp.last = a.c.trim_cycles ? a.last_cycle[(long long)t * a.s.E + s.e] : -1;
    return tp;
}

// the k-th row of the segment in track part tp: its value where the row is kept and the value is not NaN
__device__ __forceinline__ bool part_value(const SetAnaArgs &a, const SetSegment &s, const TrackPart &tp, long long k, double &v) {
    const long long r = s.seg < 0 ? k : s.seg + k * a.s.g.L;
    const AnaRow w = set_row(a, tp.p, tp.row0, s.e, r);
    if (!ana_keep(tp.p, w, tp.last)) return false;
    v = ana_value(tp.p, w, r, s.col);
    return !isnan(v);
}

// Count, mean and the sum of squares about the mean over the segment's tracks in order (the chain the head of this file states).  kKeys: the values
// also go to LDS as keys.  Every trip count and every branch around a barrier is block-uniform.
template <bool kKeys>
__device__ __forceinline__ void set_moments(const SetAnaArgs &a, const SetSegment &s, double *red, unsigned long long *keys, int *key_count, int max_keys,
                                            long long &n, double &mean, double &ss) {
    double S = 0.0;
    long long N = 0;
    for (int t = s.t0; t < s.t1; ++t) {
        const TrackPart tp = track_part(a, s, t);
        double sum = 0.0, cnt = 0.0;
        for (long long k = threadIdx.x; k < tp.n_rows; k += kAnaThreads) {
            double v;
            if (!part_value(a, s, tp, k, v)) continue;
            sum += v, cnt += 1.0;
            if (kKeys) {
                const int at = atomicAdd(key_count, 1); // the order of arrival does not matter: the keys are sorted next
                if (at < max_keys) keys[at] = to_key(v);
            }
        }
        const long long n_t = (long long)block_sum(red, cnt); // exact: counts are small integers
        const double sum_t = block_sum(red, sum);
        if (n_t > 0) S = N == 0 ? sum_t : S + sum_t, N += n_t; // a track without a kept value is no link of the chain
    }
    n = N, mean = S / (double)N;
    double SS = 0.0;
    if (N > 1) {
        for (int t = s.t0; t < s.t1; ++t) {
            const TrackPart tp = track_part(a, s, t);
            double part = 0.0;
            for (long long k = threadIdx.x; k < tp.n_rows; k += kAnaThreads) {
                double v;
                if (part_value(a, s, tp, k, v)) part += (v - mean) * (v - mean);
            }
            const double ss_t = block_sum(red, part);
            SS = t == s.t0 ? ss_t : SS + ss_t; // (an empty track adds +0.0 to a sum of squares: the same bits as leaving it out)
        }
    }
    ss = SS;
}

// thread 0 writes the segment's results where analysis_segment_*_kernel's write_segment writes them, per track or pooled
__device__ __forceinline__ void write_set_segment(const SetAnaArgs &a, const SetSegment &s, long long n, double mean, double ss, double vmin, double vmax,
                                                  const double *pct) {
    const double nanv = __builtin_nan("");
    const long long te = a.pooled ? (long long)s.e : (long long)s.t0 * a.s.E + s.e;
    {
        const bool to_pooled = a.pooled;
        if (!a.by_step) {
            double *o = (to_pooled ? a.describe : a.t_describe) + (te * a.n_cols + s.j) * (5 + a.Q); // (the host launches only where it is asked for)
            o[0] = (double)n;
            o[1] = n > 0 ? mean : nanv;
            o[2] = n > 1 ? sqrt(ss / (double)(n - 1)) : nanv;
            o[3] = n > 0 ? vmin : nanv;
            for (int i = 0; i < a.Q; ++i) o[4 + i] = n > 0 ? pct[i] : nanv;
            o[4 + a.Q] = n > 0 ? vmax : nanv;
        } else {
            const long long at = (te * a.s.g.L + s.seg) * a.n_cols + s.j;
            int *count = to_pooled ? a.step_count : a.t_step_count;
            double *sq = to_pooled ? a.step_q : a.t_step_q;
            if (count) count[at] = (int)n;
            if (sq)
                for (int i = 0; i < a.Q; ++i) sq[at * a.Q + i] = n > 0 ? pct[i] : nanv;
        }
    }
}

__global__ __launch_bounds__(kAnaThreads) void set_analysis_segment_sort_kernel(const SetAnaArgs a, const int max_keys) {
    extern __shared__ unsigned long long lds64[];
    int *key_count = reinterpret_cast<int *>(lds64);
    double *red = reinterpret_cast<double *>(lds64 + kAnaHeaderWords);
    unsigned long long *keys = lds64 + kAnaHeaderWords + kAnaThreads;
    const SetSegment s = set_segment_of(a);
    if (threadIdx.x == 0) *key_count = 0;
    __syncthreads();
    long long n;
    double mean, ss;
    set_moments<true>(a, s, red, keys, key_count, max_keys, n, mean, ss);
    const int m = min((int)n, max_keys); // n <= the segment's rows of all its tracks <= max_keys: the host chose this kernel for that
    for (int k = 2; (k >> 1) < m; k <<= 1) { // the bitonic network (replay_analysis_device.h); m is block-uniform
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
        write_set_segment(a, s, m, mean, ss, m > 0 ? from_key(keys[0]) : 0.0, m > 0 ? from_key(keys[m - 1]) : 0.0, pct);
    }
}

// (waves per SIMD pinned at 4, i.e. at most 128 VGPRs, which is what the kernel took before the geometry table's pointer and factors: left to itself
// the compiler now spills more scalars into vector lanes, ends at 135 and halves the workgroups per CU; with the pin it ends at 125, no scratch)
__global__ __launch_bounds__(kAnaThreads) __attribute__((amdgpu_waves_per_eu(4, 4))) void set_analysis_segment_select_kernel(const SetAnaArgs a) {
    __shared__ double red[kAnaThreads];
    __shared__ unsigned hist[kMaxRanks][256];
    __shared__ unsigned long long prefix[kMaxRanks]; // the digits found so far, in place
    __shared__ long long remain[kMaxRanks];          // the rank among the values that share the prefix
    const SetSegment s = set_segment_of(a);
    long long n;
    double mean, ss;
    set_moments<false>(a, s, red, nullptr, nullptr, 0, n, mean, ss);
    const int n_ranks = 2 + 2 * a.Q;
    if (n > 0) { // block-uniform; the radix select (replay_analysis_device.h)
        if ((int)threadIdx.x < n_ranks) radix_start(prefix, remain, a.q, n);
        for (int shift = 56; shift >= 0; shift -= 8) {
            for (int i = threadIdx.x; i < n_ranks * 256; i += kAnaThreads) hist[i >> 8][i & 255] = 0u;
            __syncthreads();
            for (int t = s.t0; t < s.t1; ++t) {
                const TrackPart tp = track_part(a, s, t);
                for (long long k = threadIdx.x; k < tp.n_rows; k += kAnaThreads) {
                    double v;
                    if (!part_value(a, s, tp, k, v)) continue;
                    const unsigned long long key = to_key(v);
                    const unsigned digit = (unsigned)(key >> shift) & 255u;
                    for (int i = 0; i < n_ranks; ++i)
                        if (shift == 56 || ((key ^ prefix[i]) >> (shift + 8)) == 0ull) atomicAdd(&hist[i][digit], 1u);
                }
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
        write_set_segment(a, s, n, mean, ss, n > 0 ? from_key(prefix[0]) : 0.0, n > 0 ? from_key(prefix[1]) : 0.0, pct);
    }
}

// groupby(["log_num", "cycle"]) max / mean: analysis_cycle_kernel's thread on the cycle's track; the output index is the thread's
__global__ __launch_bounds__(256) void set_analysis_cycle_kernel(const SetAnaArgs a) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)a.s.E * a.logs * a.n_cols) return;
    const int j = (int)(idx % a.n_cols), e = (int)(idx / ((long long)a.n_cols * a.logs));
    const long long gc = (idx / a.n_cols) % a.logs;
    int lo = 0, hi = a.s.T - 1; // the last track whose first logged cycle is <= gc (a track without one shares its log0 with the next and is never found)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.log0[mid] <= gc) lo = mid;
        else hi = mid - 1;
    }
    const AnaArgs p = track_args(a, lo, a.s.tracks[lo]);
    const long long row0 = a.row0[lo];
    const int c = (int)(gc - a.log0[lo]);
    const int last = a.c.trim_cycles ? a.last_cycle[(long long)lo * a.s.E + e] : -1;
    double vmax = 0.0, sum = 0.0;
    int n = 0;
    for (int step = 0; step < a.s.g.L; ++step) {
        const long long r = (long long)c * a.s.g.L + step;
        const AnaRow w = set_row(a, p, row0, e, r);
        if (!ana_keep(p, w, last)) continue;
        const double v = ana_value(p, w, r, a.cols[j]);
        if (isnan(v)) continue;
        vmax = n == 0 ? v : fmax(vmax, v);
        sum += v, ++n;
    }
    const double nanv = __builtin_nan("");
    if (a.cycle_max) a.cycle_max[idx] = n > 0 ? vmax : nanv;
    if (a.cycle_mean) a.cycle_mean[idx] = n > 0 ? sum / (double)n : nanv;
}

// calc_anomalies and print_stats over the kept rows of one (track, experiment); counts are integers, added with LDS atomics
__global__ __launch_bounds__(kAnaThreads) void set_analysis_flags_kernel(const SetAnaArgs a) {
    __shared__ int cnt[12]; // analysis_flags_kernel's
    const int t = blockIdx.x / a.s.E, e = blockIdx.x - t * a.s.E;
    if (threadIdx.x < 12) cnt[threadIdx.x] = 0;
    __syncthreads();
    const AnaArgs p = track_args(a, t, a.s.tracks[t]);
    const long long row0 = a.row0[t];
    const int last = a.c.trim_cycles ? a.last_cycle[blockIdx.x] : -1;
    for (long long r = threadIdx.x; r < p.v.R; r += kAnaThreads) {
        const AnaRow w = ana_row(p, e, r); // (no flag reads the precise error)
        unsigned bits = 0u;
        if (ana_keep(p, w, last)) {
            // analysis_flags_kernel's statements, on the values calc_anomalies sees: after change_unit; a comparison with NaN is false
            bits |= w.sp * p.c.speed_factor >= a.c.min_speed ? 1u : 0u;
            bits |= w.err >= a.c.min_bbox_error ? 2u : 0u;
            bits |= w.dev * p.c.dist_factor >= a.c.min_dist_error ? 4u : 0u;
            bits |= w.ww * p.c.dist_factor >= a.c.min_width ? 8u : 0u;
            bits |= w.wh * p.c.dist_factor >= a.c.min_height ? 16u : 0u;
            const bool finite = isfinite(w.wx) && isfinite(w.wy) && isfinite(w.ww) && isfinite(w.wh);
            bits |= (a.c.no_preds && !finite) ? 32u : 0u;
            for (int k = 0; k < 6; ++k)
                if ((bits >> k) & 1u) atomicAdd(&cnt[k], 1);
            if (bits) atomicAdd(&cnt[6], 1);
            atomicAdd(&cnt[7], 1);
            if (isnan(w.wx) || isnan(w.wy) || isnan(w.ww) || isnan(w.wh)) atomicAdd(&cnt[8], 1);
            if (w.err > 1e-7) atomicAdd(&cnt[9], 1);
        }
        if (a.anomaly_mask) a.anomaly_mask[(long long)e * a.rows + row0 + r] = (uint8_t)bits;
    }
    for (int c = threadIdx.x; c < p.v.n_log; c += kAnaThreads) {
        bool any = false;
        for (int step = 0; step < a.s.g.L && !any; ++step) any = ana_keep(p, ana_row(p, e, (long long)c * a.s.g.L + step), last);
        if (any) atomicAdd(&cnt[10], 1);
    }
    __syncthreads();
    if (threadIdx.x < kFlagCounts) a.flag_counts[(long long)blockIdx.x * kFlagCounts + threadIdx.x] = cnt[threadIdx.x];
    if (threadIdx.x < 7 && a.t_anomaly_counts) a.t_anomaly_counts[(long long)blockIdx.x * 7 + threadIdx.x] = cnt[threadIdx.x];
    if (threadIdx.x == 0 && a.t_stats) {
        long long *o = a.t_stats + (long long)blockIdx.x * 4;
        o[0] = p.v.R - cnt[7], o[1] = cnt[8], o[2] = cnt[10], o[3] = cnt[9];
    }
}

// the pooled counts: integer sums over the tracks (distinct (log_num, cycle) pairs are the sum of the tracks' distinct cycles)
__global__ __launch_bounds__(256) void set_analysis_pool_kernel(const SetAnaArgs a) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= a.s.E) return;
    long long sum[kFlagCounts];
    for (int k = 0; k < kFlagCounts; ++k) sum[k] = 0;
    for (int t = 0; t < a.s.T; ++t)
        for (int k = 0; k < kFlagCounts; ++k) sum[k] += a.flag_counts[((long long)t * a.s.E + e) * kFlagCounts + k];
    if (a.anomaly_counts)
        for (int k = 0; k < 7; ++k) a.anomaly_counts[(long long)e * 7 + k] = sum[k];
    if (a.stats) {
        long long *o = a.stats + (long long)e * 4;
        o[0] = a.rows - sum[7], o[1] = sum[8], o[2] = sum[10], o[3] = sum[9];
    }
}

// the scratch in doubles from its start: row0 and log0 [T + 1] int64 each, the flags' counters [T][E][11] int64, the last cycles [T][E] int32
inline long long set_ana_off_flags(long long T) { return 2 * (T + 1); }
inline long long set_ana_off_last(long long T, long long E) { return set_ana_off_flags(T) + T * E * kFlagCounts; }
inline long long set_ana_scratch(long long T, long long E) { return set_ana_off_last(T, E) + (T * E + 1) / 2; }

} // namespace

extern "C" int64_t wtk_replay_set_analysis_scratch_doubles(const wtk_replay_set_track *tracks_host, int32_t T, int32_t cycle_frame_num, int32_t E, int32_t n_cols,
                                                           int32_t Q) {
    if (!tracks_host || T < 1 || cycle_frame_num < 1 || E < 0 || n_cols < 0 || Q < 0) return -1;
    for (int t = 0; t < T; ++t)
        if (tracks_host[t].n_log < 0) return -1;
    return set_ana_scratch(T, E);
}

extern "C" int wtk_replay_set_analyze_geom(const wtk_replay_config *cfg, const wtk_replay_analysis_config *acfg, const wtk_replay_set_track *tracks_host,
                                           const wtk_replay_set_track *tracks_dev, const wtk_replay_set_geometry *geom_host,
                                           const wtk_replay_set_geometry *geom_dev, int32_t T, int32_t guard_cycles, int32_t E, const double *track_dev,
                                           int32_t n_super, const double *share_dev, const int32_t *pos_dev, const int32_t *move_dev,
                                           const double *precise_rows_dev, const int32_t *columns_host, int32_t n_cols, const double *percentiles_host,
                                           int32_t Q, int32_t max_lds_rows, double *track_describe_dev, double *cycle_max_dev, double *cycle_mean_dev,
                                           double *track_step_quantiles_dev, int32_t *track_step_count_dev, int64_t *track_anomaly_counts_dev,
                                           uint8_t *anomaly_mask_dev, int64_t *track_stats_dev, double *describe_dev, double *step_quantiles_dev,
                                           int32_t *step_count_dev, int64_t *anomaly_counts_dev, int64_t *stats_dev, double *scratch_dev,
                                           int64_t scratch_doubles, void *stream) {
    const char *who = geom_host || geom_dev ? "wtk_replay_set_analyze_geom" : "wtk_replay_set_analyze";
    const std::string w(who);
    SetAnaArgs a = {};
    int min_log = 0;
    if (!acfg) return fail(w + ": null argument");
    if (set_view(who, cfg, tracks_host, tracks_dev, geom_host, geom_dev, T, guard_cycles, WTK_REPLAY_OPTIMAL, E, track_dev, n_super, share_dev, pos_dev, move_dev, a.s,
                 min_log))
        return 1;
    for (int t = 0; geom_host && t < T; ++t)
        if (!std::isfinite(geom_host[t].time_factor) || !std::isfinite(geom_host[t].dist_factor) || !std::isfinite(geom_host[t].speed_factor))
            return fail(w + ": track " + std::to_string(t) + ": the unit factors must be finite");
    if (!scratch_dev) return fail(w + ": null argument");
    if (analysis_spec(w, acfg, columns_host, n_cols, percentiles_host, Q, max_lds_rows, precise_rows_dev != nullptr, "precise_rows_dev", a.cols, a.q)) return 1;
    long long rows = 0, logs = 0, max_rows = 0, max_logs = 0;
    for (int t = 0; t < T; ++t) {
        rows += tracks_host[t].R, logs += tracks_host[t].n_log;
        max_rows = std::max<long long>(max_rows, tracks_host[t].R), max_logs = std::max<long long>(max_logs, tracks_host[t].n_log);
    }
    if (rows > INT32_MAX) return fail(w + ": the logged rows of all tracks must stay below 2^31");
    if ((long long)T * E * n_cols * a.s.g.L > INT32_MAX || ((long long)E * logs * n_cols + 255) / 256 > INT32_MAX)
        return fail(w + ": too many blocks for one launch");
    if (scratch_doubles < set_ana_scratch(T, E)) return fail(w + ": scratch smaller than wtk_replay_set_analysis_scratch_doubles(tracks_host, T, L, E, n_cols, Q)");
    a.err = precise_rows_dev, a.rows = rows, a.logs = logs, a.c = *acfg, a.n_cols = n_cols, a.Q = Q;
    a.row0 = reinterpret_cast<long long *>(scratch_dev), a.log0 = a.row0 + (T + 1);
    a.flag_counts = reinterpret_cast<long long *>(scratch_dev + set_ana_off_flags(T));
    a.last_cycle = reinterpret_cast<int *>(scratch_dev + set_ana_off_last(T, E));
    a.t_describe = track_describe_dev, a.cycle_max = cycle_max_dev, a.cycle_mean = cycle_mean_dev, a.t_step_q = track_step_quantiles_dev;
    a.t_step_count = track_step_count_dev, a.t_anomaly_counts = reinterpret_cast<long long *>(track_anomaly_counts_dev), a.anomaly_mask = anomaly_mask_dev;
    a.t_stats = reinterpret_cast<long long *>(track_stats_dev);
    a.describe = describe_dev, a.step_q = step_quantiles_dev, a.step_count = step_count_dev;
    a.anomaly_counts = reinterpret_cast<long long *>(anomaly_counts_dev), a.stats = reinterpret_cast<long long *>(stats_dev);
    hipStream_t st = (hipStream_t)stream;
    const int max_keys = max_lds_rows == 0 ? kAnaMaxKeys : std::min((int)max_lds_rows, kAnaMaxKeys);
    const bool segments = track_describe_dev || track_step_quantiles_dev || track_step_count_dev || describe_dev || step_quantiles_dev || step_count_dev;
    // above 64 KiB of dynamic LDS a kernel needs the attribute (per device, so it is set at every call: a host-side table write)
    if (segments)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&set_analysis_segment_sort_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kAnaLdsBytes));
    hipLaunchKernelGGL(set_analysis_prefix_kernel, dim3(1), dim3(64), 0, st, a);
    if (a.c.trim_cycles) hipLaunchKernelGGL(set_analysis_last_cycle_kernel, dim3((unsigned)((long long)T * E)), dim3(kAnaThreads), 0, st, a);
    for (int pooled = 0; pooled < 2; ++pooled) {
        for (int by_step = 0; by_step < 2; ++by_step) {
            const bool of_pooled = by_step ? (step_quantiles_dev || step_count_dev) : describe_dev != nullptr;
            const bool of_track = by_step ? (track_step_quantiles_dev || track_step_count_dev) : track_describe_dev != nullptr;
            const bool wanted = pooled ? of_pooled : of_track;
            if (!wanted) continue;
            a.pooled = pooled, a.by_step = by_step;
            // the longest segment's rows over the tracks the workgroup walks: an upper bound of its kept values
            const long long seg_rows = pooled ? (by_step ? logs : rows) : (by_step ? max_logs : max_rows);
            const unsigned grid = (unsigned)((long long)(pooled ? 1 : T) * E * n_cols * (by_step ? a.s.g.L : 1));
            if (seg_rows <= max_keys) {
                const size_t lds = (size_t)(kAnaHeaderWords + kAnaThreads + std::max(seg_rows, 1ll)) * 8;
                hipLaunchKernelGGL(set_analysis_segment_sort_kernel, dim3(grid), dim3(kAnaThreads), lds, st, a, (int)std::max(seg_rows, 1ll));
            } else {
                hipLaunchKernelGGL(set_analysis_segment_select_kernel, dim3(grid), dim3(kAnaThreads), 0, st, a);
            }
        }
    }
    a.pooled = 0, a.by_step = 0;
    if ((cycle_max_dev || cycle_mean_dev) && logs > 0)
        hipLaunchKernelGGL(set_analysis_cycle_kernel, dim3((unsigned)(((long long)E * logs * n_cols + 255) / 256)), dim3(256), 0, st, a);
    if (track_anomaly_counts_dev || anomaly_mask_dev || track_stats_dev || anomaly_counts_dev || stats_dev) {
        hipLaunchKernelGGL(set_analysis_flags_kernel, dim3((unsigned)((long long)T * E)), dim3(kAnaThreads), 0, st, a);
        if (anomaly_counts_dev || stats_dev) hipLaunchKernelGGL(set_analysis_pool_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, st, a);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// (no geometry table: cfg's sizes and acfg's factors for every track)
extern "C" int wtk_replay_set_analyze(const wtk_replay_config *cfg, const wtk_replay_analysis_config *acfg, const wtk_replay_set_track *tracks_host,
                                      const wtk_replay_set_track *tracks_dev, int32_t T, int32_t guard_cycles, int32_t E, const double *track_dev,
                                      int32_t n_super, const double *share_dev, const int32_t *pos_dev, const int32_t *move_dev, const double *precise_rows_dev,
                                      const int32_t *columns_host, int32_t n_cols, const double *percentiles_host, int32_t Q, int32_t max_lds_rows,
                                      double *track_describe_dev, double *cycle_max_dev, double *cycle_mean_dev, double *track_step_quantiles_dev,
                                      int32_t *track_step_count_dev, int64_t *track_anomaly_counts_dev, uint8_t *anomaly_mask_dev, int64_t *track_stats_dev,
                                      double *describe_dev, double *step_quantiles_dev, int32_t *step_count_dev, int64_t *anomaly_counts_dev, int64_t *stats_dev,
                                      double *scratch_dev, int64_t scratch_doubles, void *stream) {
    return wtk_replay_set_analyze_geom(cfg, acfg, tracks_host, tracks_dev, nullptr, nullptr, T, guard_cycles, E, track_dev, n_super, share_dev, pos_dev, move_dev,
                                       precise_rows_dev, columns_host, n_cols, percentiles_host, Q, max_lds_rows, track_describe_dev, cycle_max_dev, cycle_mean_dev,
                                       track_step_quantiles_dev, track_step_count_dev, track_anomaly_counts_dev, anomaly_mask_dev, track_stats_dev, describe_dev,
                                       step_quantiles_dev, step_count_dev, anomaly_counts_dev, stats_dev, scratch_dev, scratch_doubles, stream);
}
