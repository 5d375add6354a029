// What the analysis of one replayed log (replay_analysis.hip) and of a set of logs (replay_set_analysis.hip, section 28) share: the
// ONE statement of a logged row's columns after DataAnalyzer.initialize (AnaRow, ana_row), of clean's mask (ana_keep) and of change_unit (ana_value), the
// fixed-order block sum, the order-preserving keys with numpy's `linear` percentile rule, the bitonic network and the radix select, and the host checks
// of an analysis spec.  A (track, experiment) pair of a set is the single-track experiment on the track's ReplayView, so it has the single-track bits.
// Everything relies on -ffp-contract=off and on HIP's float64 sqrt and division being the correctly rounded ones.
#pragma once
#include "wtk_internal.h"
#include "replay_device.h"

#include <cmath>
#include <string>

namespace wtk {

constexpr int kAnaThreads = 512;
constexpr int kAnaLdsBytes = 160 * 1024; // the CU's LDS: one workgroup per CU takes all of it at the default limit
constexpr int kAnaHeaderWords = 8;       // 64-bit words in front of the tree's buffer: word 0 holds the key counter
constexpr int kAnaMaxKeys = (kAnaLdsBytes - (kAnaHeaderWords + kAnaThreads) * 8) / 8; // 19960
constexpr int kMaxCols = WTK_ANALYSIS_MAX_COLUMNS;
constexpr int kMaxQ = WTK_ANALYSIS_MAX_PERCENTILES;
constexpr int kMaxRanks = 2 * kMaxQ + 2;

struct AnaArgs {
    ReplayView v;
    const double *pair;     // [R][E] precise error of every pair, NaN = no value (nullable)
    wtk_replay_analysis_config c;
    int n_cols, Q;
    int cols[kMaxCols];
    double q[kMaxQ];
    int by_step;            // the segment launch: 0 = one segment per (experiment, column), 1 = one per cycle step
    int *last_cycle;        // [E] scratch: the largest cycle surviving imaging_only and bounds, -1 where none does
    double *describe;       // [E][n_cols][5 + Q]
    double *cycle_max, *cycle_mean; // [E][n_log][n_cols]
    double *step_q;         // [E][L][n_cols][Q]
    int *step_count;        // [E][L][n_cols]
    long long *anomaly_counts; // [E][7]
    uint8_t *anomaly_mask;  // [E][R]
    long long *stats;       // [E][4]
};

// one logged row's columns after DataAnalyzer.initialize: float64, the reference's order of operations, every one rounded as DataFrame.round(5) rounds
struct AnaRow {
    double plt_x, plt_y, cam_x, cam_y, cam_w, cam_h, mic_x, mic_y, mic_w, mic_h, wx, wy, ww, wh;
    double wcx, wcy, mcx, mcy, sx, sy, sp, dx, dy, dev, err, precise;
    int c, step;
    bool pre; // survives clean's imaging_only and bounds
};

__device__ __forceinline__ double round5(double v) { return isfinite(v) ? rint(v * 1e5) / 1e5 : v; }

__device__ __forceinline__ AnaRow ana_row(const AnaArgs &a, int e, long long r) {
    AnaRow w;
    const ReplayRow row = replay_row(a.v, e, r);
    const RowBoxes &b = row.b;
    w.c = row.at.c, w.step = row.at.step;
    const double wcx = b.wx + b.ww / 2, wcy = b.wy + b.wh / 2, mcx = b.mic_x + b.mic_w / 2, mcy = b.mic_y + b.mic_h / 2; // _calc_centers
    double sx = __builtin_nan(""), sy = __builtin_nan("");
    if (r >= a.c.period) { // _calc_speed: Series.diff(period) over the whole uncleaned log, divided by time.diff(period) = period
        const RowBoxes p = replay_row(a.v, e, r - a.c.period).b;
        const double n = (double)a.c.period;
        sx = (wcx - (p.wx + p.ww / 2)) / n, sy = (wcy - (p.wy + p.wh / 2)) / n;
    }
    const double dx = wcx - mcx, dy = wcy - mcy; // _calc_worm_deviation
    w.plt_x = round5((double)row.px), w.plt_y = round5((double)row.py);
    w.cam_x = round5(b.cam_x), w.cam_y = round5(b.cam_y), w.cam_w = round5((double)a.v.g.cam_w), w.cam_h = round5((double)a.v.g.cam_h);
    w.mic_x = round5(b.mic_x), w.mic_y = round5(b.mic_y), w.mic_w = round5(b.mic_w), w.mic_h = round5(b.mic_h);
    w.wx = round5(b.wx), w.wy = round5(b.wy), w.ww = round5(b.ww), w.wh = round5(b.wh);
    w.wcx = round5(wcx), w.wcy = round5(wcy), w.mcx = round5(mcx), w.mcy = round5(mcy);
    w.sx = round5(sx), w.sy = round5(sy), w.sp = round5(sqrt(sx * sx + sy * sy));
    w.dx = round5(dx), w.dy = round5(dy), w.dev = round5(sqrt(dx * dx + dy * dy));
    w.err = round5(row_bbox_error(b));
    w.precise = a.pair ? a.pair[r * a.v.E + e] : __builtin_nan(""); // assigned after the rounding (calc_precise_error): unrounded
    // clean, on the rounded values.  The reference's `mask_wrm = has_pred; mask_wrm &= ...` updates has_pred in place, so its `~has_pred` is the negation
    // of the finished worm mask: it keeps (has_pred and the worm box inside) or the microscope box inside.
    bool pre = !a.c.imaging_only || w.step < a.v.g.I;
    if (pre && a.c.use_bounds) {
        const double *bd = a.c.bounds;
        const bool has_pred = isfinite(w.wx) && isfinite(w.wy) && isfinite(w.ww) && isfinite(w.wh);
        const bool wrm_in = w.wx >= bd[0] && w.wx + w.ww <= bd[2] && w.wy >= bd[1] && w.wy + w.wh <= bd[3];
        const bool mic_in = w.mic_x >= bd[0] && w.mic_x + w.mic_w <= bd[2] && w.mic_y >= bd[1] && w.mic_y + w.mic_h <= bd[3];
        pre = (has_pred && wrm_in) || mic_in;
    }
    w.pre = pre;
    return w;
}

__device__ __forceinline__ bool ana_keep(const AnaArgs &a, const AnaRow &w, int last) { return w.pre && (!a.c.trim_cycles || (w.c != 0 && w.c != last)); }

// the column's value of a row in the requested unit (change_unit: one multiplication of the rounded value; the factors are 1 for unit "frame")
__device__ __forceinline__ double ana_value(const AnaArgs &a, const AnaRow &w, long long r, int col) {
    const double tf = a.c.time_factor, ds = a.c.dist_factor, sf = a.c.speed_factor;
    switch (col) {
    case WTK_ANALYSIS_COL_FRAME: return (double)r;
    case WTK_ANALYSIS_COL_CYCLE: return (double)w.c;
    case WTK_ANALYSIS_COL_PLT_X: return w.plt_x * ds;
    case WTK_ANALYSIS_COL_PLT_Y: return w.plt_y * ds;
    case WTK_ANALYSIS_COL_CAM_X: return w.cam_x * ds;
    case WTK_ANALYSIS_COL_CAM_Y: return w.cam_y * ds;
    case WTK_ANALYSIS_COL_CAM_W: return w.cam_w * ds;
    case WTK_ANALYSIS_COL_CAM_H: return w.cam_h * ds;
    case WTK_ANALYSIS_COL_MIC_X: return w.mic_x * ds;
    case WTK_ANALYSIS_COL_MIC_Y: return w.mic_y * ds;
    case WTK_ANALYSIS_COL_MIC_W: return w.mic_w * ds;
    case WTK_ANALYSIS_COL_MIC_H: return w.mic_h * ds;
    case WTK_ANALYSIS_COL_WRM_X: return w.wx * ds;
    case WTK_ANALYSIS_COL_WRM_Y: return w.wy * ds;
    case WTK_ANALYSIS_COL_WRM_W: return w.ww * ds;
    case WTK_ANALYSIS_COL_WRM_H: return w.wh * ds;
    case WTK_ANALYSIS_COL_TIME: return (double)r * tf;
    case WTK_ANALYSIS_COL_CYCLE_STEP: return (double)w.step;
    case WTK_ANALYSIS_COL_WRM_CENTER_X: return w.wcx * ds;
    case WTK_ANALYSIS_COL_WRM_CENTER_Y: return w.wcy * ds;
    case WTK_ANALYSIS_COL_MIC_CENTER_X: return w.mcx * ds;
    case WTK_ANALYSIS_COL_MIC_CENTER_Y: return w.mcy * ds;
    case WTK_ANALYSIS_COL_WRM_SPEED_X: return w.sx * sf;
    case WTK_ANALYSIS_COL_WRM_SPEED_Y: return w.sy * sf;
    case WTK_ANALYSIS_COL_WRM_SPEED: return w.sp * sf;
    case WTK_ANALYSIS_COL_WORM_DEVIATION_X: return w.dx * ds;
    case WTK_ANALYSIS_COL_WORM_DEVIATION_Y: return w.dy * ds;
    case WTK_ANALYSIS_COL_WORM_DEVIATION: return w.dev * ds;
    case WTK_ANALYSIS_COL_BBOX_ERROR: return w.err;
    default: return w.precise; // WTK_ANALYSIS_COL_PRECISE_ERROR (the entry point refuses every other id)
    }
}

// the block's sum in a fixed order: a binary tree over the threads' values; every thread gets it
__device__ __forceinline__ double block_sum(double *red, double v) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int half = kAnaThreads / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) red[threadIdx.x] += red[threadIdx.x + half];
        __syncthreads();
    }
    const double sum = red[0];
    __syncthreads();
    return sum;
}

// order-preserving 64-bit keys of float64 values (-0.0 sorts before 0.0; no NaN is ever a key)
__device__ __forceinline__ unsigned long long to_key(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double from_key(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// the ranks a segment of n values needs: [0] min, [1] max, [2 + 2 i], [3 + 2 i] the neighbours of percentile i; numpy's `linear` rule
__device__ __forceinline__ void percentile_rank(double q, long long n, long long &lo, long long &hi, double &t) {
    const double pos = q * (double)(n - 1);
    const double fl = floor(pos);
    lo = (long long)fl, t = pos - fl;
    hi = lo + 1 < n ? lo + 1 : n - 1;
}
__device__ __forceinline__ double lerp_linear(double x, double y, double t) { return t < 0.5 ? x + (y - x) * t : y - (y - x) * (1 - t); }

// The bodies of the two ways to the order statistics.  Their loops stay with the kernels that run them (the values of a segment come from one track or
// from several), and so each kernel's barriers stay in its own text.
//
// Bitonic network over keys[0 .. m) in LDS, every comparator min-to-low-index: per merge size k a flip pass (partner i ^ (k - 1)) and disperse passes
// (partner i ^ j).  With the indices >= m imagined to hold +infinity no comparator ever moves one of them, so leaving them out sorts any m.
__device__ __forceinline__ void bitonic_compare(unsigned long long *keys, int i, int l, int m) {
    if (l > i && l < m) {
        const unsigned long long x = keys[i], y = keys[l];
        if (x > y) keys[i] = y, keys[l] = x;
    }
}

// Most-significant-digit radix select, 8 passes of 8 bits, over all ranks (min, max, both neighbours of every percentile) of n > 0 values at once, a
// 256-bin histogram per rank in LDS (integer atomics: the counts do not depend on the order of arrival).  Per pass, between barriers: the kernel clears
// the histograms, counts the digit of every kept value for every rank whose digits so far the value shares, and radix_digit takes each rank's digit;
// after the last pass prefix[i] is the key of rank i.  (The clearing and the counting are written out in the kernels: called from here, the compiler
// allocated the single-track select kernel's registers differently, and that kernel is held to its earlier instructions.)
// thread i < n_ranks: the rank it looks for
__device__ __forceinline__ void radix_start(unsigned long long *prefix, long long *remain, const double *q, long long n) {
    long long rank = threadIdx.x == 0 ? 0 : n - 1;
    if (threadIdx.x >= 2) {
        long long lo, hi;
        double t;
        percentile_rank(q[(threadIdx.x - 2) >> 1], n, lo, hi, t);
        rank = (threadIdx.x & 1) ? hi : lo;
    }
    remain[threadIdx.x] = rank, prefix[threadIdx.x] = 0ull;
}
// thread i < n_ranks: the pass's digit of its rank
__device__ __forceinline__ void radix_digit(unsigned (*hist)[256], unsigned long long *prefix, long long *remain, int shift) {
    long long rem = remain[threadIdx.x];
    unsigned d = 0;
    for (; d < 255u && rem >= (long long)hist[threadIdx.x][d]; ++d) rem -= (long long)hist[threadIdx.x][d];
    remain[threadIdx.x] = rem, prefix[threadIdx.x] |= (unsigned long long)d << shift;
}

// The refusals of an analysis spec every entry point shares; fills cols / q.  `precise_arg`: the name of the caller's precise-error argument.
inline int analysis_spec(const std::string &w, const wtk_replay_analysis_config *acfg, const int32_t *columns_host, int32_t n_cols, const double *percentiles_host,
                         int32_t Q, int32_t max_lds_rows, bool has_precise, const char *precise_arg, int *cols, double *q) {
    if (!acfg) return fail(w + ": null argument");
    if (!columns_host || (Q > 0 && !percentiles_host)) return fail(w + ": null argument");
    if (n_cols < 1 || n_cols > kMaxCols) return fail(w + ": 1.." + std::to_string(kMaxCols) + " columns");
    if (Q < 0 || Q > kMaxQ) return fail(w + ": 0.." + std::to_string(kMaxQ) + " percentiles");
    if (acfg->period < 1) return fail(w + ": period must be at least 1");
    if (max_lds_rows < 0) return fail(w + ": negative max_lds_rows (0 = the default)");
    for (int j = 0; j < n_cols; ++j) {
        if (columns_host[j] < 0 || columns_host[j] >= WTK_ANALYSIS_N_COLUMNS) return fail(w + ": unknown column");
        if (columns_host[j] == WTK_ANALYSIS_COL_PRECISE_ERROR && !has_precise) return fail(w + ": the precise_error column needs " + precise_arg);
        cols[j] = columns_host[j];
    }
    for (int i = 0; i < Q; ++i) {
        if (!(percentiles_host[i] >= 0.0 && percentiles_host[i] <= 1.0)) return fail(w + ": percentile outside [0, 1]");
        q[i] = percentiles_host[i];
    }
    return 0;
}

} // namespace wtk
