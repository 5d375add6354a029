// What the closed loop's translation units share (replay.hip, replay_set.hip, replay_precise.hip, replay_yolo.hip, replay_analysis.hip): the geometry and the view of
// a scanned population with the ONE host function that fills it, the ONE statement of the motor and of the scan, "row r of experiment e" (cycle, step, platform position,
// boxes), the bbox error of a log row, the fixed chunking of the per-experiment sums with its tree reduction, the summaries' slots, and the declarations of
// the host launchers that cross translation units (defined in replay.hip).
// Everything relies on -ffp-contract=off (the library's build flag): share * move + carry is a rounded product and a rounded sum, as in Python.
#pragma once
#include "wtk_internal.h"

#include <cmath>
#include <functional>
#include <string>

namespace wtk {

constexpr int kRowThreads = 256;
constexpr int kRowChunk = 4096; // logged rows per block of a reducing kernel: the FIXED chunking of the reductions
constexpr double kMoveMax = 1073741824.0; // 2^30: moves are kept as int32

// chunks of R logged rows: the blocks per experiment of a reducing kernel and the partials the finish launch adds
__host__ __device__ inline long long chunk_count(long long R) { return (R + kRowChunk - 1) / kRowChunk; }

// slots of wtk_replay_rows' summary (include/wtk_hip.h documents them as [0]..[5])
enum RowsSlot { kRowsErr = 0, kRowsCount, kRowsTrimmedErr, kRowsTrimmedCount, kRowsNonPerfect, kRowsMse, kSummary };
// slots of wtk_replay_precise's summary: rows without a value (NaN) enter no sum and are counted apart
enum PreciseSlot { kPreciseErr = 0, kPreciseCount, kPreciseTrimmedErr, kPreciseTrimmedCount, kPreciseNonPerfect, kPreciseNan, kPreciseSummary };
static_assert(kSummary == WTK_REPLAY_SUMMARY_DOUBLES && kPreciseSummary == WTK_REPLAY_PRECISE_SUMMARY_DOUBLES, "summary widths of the C ABI");

struct Geometry {
    int L, I, M, P;
    int cam_w, cam_h, mic_w, mic_h;
    int x_max, y_max; // frame_w - 1, frame_h - 1: the clamp of the platform position
};

// A scanned population as the kernels behind the scan read it: E experiments over C cycles, of which n_log are logged as R = n_log * L rows.
struct ReplayView {
    Geometry g;
    int E, C, n_log;
    long long R;         // logged rows per experiment
    const double *track; // [n_track][4] xywh: row r is logged frame r
    const double *share; // [M]
    const int *pos, *move; // [C][E][2] position at cycle start and the cycle's move
};

// the controller's move on one axis from the camera corner; a non-finite result is no move, a huge one saturates at +-2^30
__device__ __forceinline__ double finish_move(double v) {
    if (!isfinite(v)) return 0.0;
    return fmin(fmax(rint(v), -kMoveMax), kMoveMax);
}

// one step of SineMotorController.step + ViewController.move_position on one axis
__device__ __forceinline__ void motor_axis(double share, double mv, double &carry, int &pos, int pos_max) {
    const double want = share * mv + carry;
    const double took = rint(want); // round half to even: Python's round on a float
    carry = want - took;
    pos = (int)fmin(fmax((double)pos + took, 0.0), (double)pos_max);
}

// `steps` motor steps of the move (mx, my) from (px, py), the carry starting at zero: what a cycle's moving phase does to the platform (steps = M) and what
// has happened to it before a frame of that phase (steps < M).  The ONE statement of the motor: the scan, the rows and the YOLO loop's kernels all call it.
__device__ __forceinline__ void motor_steps(const Geometry &g, const double *share, int steps, double mx, double my, int &px, int &py) {
    double cx = 0.0, cy = 0.0;
    for (int k = 0; k < steps; ++k) {
        const double sh = share[k];
        motor_axis(sh, mx, cx, px, g.x_max);
        motor_axis(sh, my, cy, py, g.y_max);
    }
}

// the platform position at the camera picture of step `step` of a cycle, from the cycle's start position and move ([C][E][2] entry ce)
__device__ __forceinline__ void frame_position(const Geometry &g, const double *share, const int *pos, const int *move, long long ce, int step, int &px, int &py) {
    px = pos[2 * ce], py = pos[2 * ce + 1];
    const int done = step <= g.I ? 0 : (step - g.I > g.M ? g.M : step - g.I); // motor steps taken before this frame's camera picture
    if (done > 0) motor_steps(g, share, done, (double)move[2 * ce], (double)move[2 * ce + 1], px, py);
}

// The boxes of a log row from the platform position at its camera picture: camera and microscope corners, and the logged worm box, which is the track's
// row made camera-relative (CsvController.predict) and absolute again (LoggingController); a non-finite row is logged as zeros.  (x - cam) + cam is not
// always x: the rows kernel and the precise kernel both take the box from here.
struct RowBoxes {
    double cam_x, cam_y, mic_x, mic_y, mic_w, mic_h;
    double wx, wy, ww, wh;
};

__device__ __forceinline__ RowBoxes row_boxes(const Geometry &g, const double *track_row, int px, int py) {
    RowBoxes b;
    b.cam_x = (double)(px - g.cam_w / 2), b.cam_y = (double)(py - g.cam_h / 2);
    b.mic_x = (double)(px - g.mic_w / 2), b.mic_y = (double)(py - g.mic_h / 2);
    b.mic_w = (double)g.mic_w, b.mic_h = (double)g.mic_h;
    b.wx = (track_row[0] - b.cam_x) + b.cam_x, b.wy = (track_row[1] - b.cam_y) + b.cam_y, b.ww = track_row[2], b.wh = track_row[3];
    if (!(isfinite(b.wx) && isfinite(b.wy) && isfinite(b.ww) && isfinite(b.wh))) b.wx = b.wy = b.ww = b.wh = 0.0;
    return b;
}

// where logged row r lies in the loop: the same for every experiment (a kernel that answers many experiments of one row divides once)
struct RowCycle {
    int c, step; // cycle and step in it
};

__device__ __forceinline__ RowCycle row_cycle(const Geometry &g, long long r) {
    RowCycle at;
    at.c = (int)(r / g.L), at.step = (int)(r - (long long)at.c * g.L);
    return at;
}

// the rows DataAnalyzer.clean(trim_cycles=True, imaging_only=True) keeps: the imaging phase of every logged cycle but the first and the last
__device__ __forceinline__ bool row_trimmed(const ReplayView &v, RowCycle at) { return at.step < v.g.I && at.c != 0 && at.c != v.n_log - 1; }

// Row r of experiment e: the platform position at its camera picture and its boxes.
struct ReplayRow {
    RowCycle at;
    int px, py;
    RowBoxes b;
};

__device__ __forceinline__ ReplayRow replay_row(const ReplayView &v, int e, long long r, RowCycle at) {
    ReplayRow w;
    w.at = at;
    frame_position(v.g, v.share, v.pos, v.move, (long long)at.c * v.E + e, at.step, w.px, w.py);
    w.b = row_boxes(v.g, v.track + 4 * r, w.px, w.py);
    return w;
}

__device__ __forceinline__ ReplayRow replay_row(const ReplayView &v, int e, long long r) { return replay_row(v, e, r, row_cycle(v.g, r)); }

// ErrorCalculator.calculate_bbox_error of a row: the share of the logged worm box outside the microscope box, 0 where the box has no area
__device__ __forceinline__ double row_bbox_error(const RowBoxes &b) {
    const double il = fmax(b.wx, b.mic_x), it = fmax(b.wy, b.mic_y);
    const double ir = fmin(b.wx + b.ww, b.mic_x + b.mic_w), ib = fmin(b.wy + b.wh, b.mic_y + b.mic_h);
    const double iw = fmax(0.0, ir - il), ih = fmax(0.0, ib - it);
    const double inter = iw * ih, total = b.ww * b.wh;
    return total == 0.0 ? 0.0 : 1.0 - inter / total;
}

// a row counts as non-perfect above this error (print_stats' "Non Perfect Predictions")
__device__ __forceinline__ bool non_perfect(double err) { return err > 1e-7; }

// The per-experiment sums' FIXED order inside a chunk: every thread of the block has added the chunk's rows t, t + 256, ... in order into acc; here a
// binary tree over the 256 threads in LDS, and the chunk's N partials stored at `partial` (the finish launch adds the chunks in index order).  The
// chunking depends on the row count only: an experiment gives the same bits alone and inside any population.  No floating-point atomics.
// (The lane-serial loop stays with its kernels, the precise one as replay_precise_device.h's precise_chunk_rows on the caller's acc array: handed over
// as a callable, the precise reduction's sums went to scratch memory.)
template <int N> __device__ __forceinline__ void chunk_reduce(double (&red)[N][kRowThreads], const double (&acc)[N], double *partial) {
    for (int q = 0; q < N; ++q) red[q][threadIdx.x] = acc[q];
    __syncthreads();
    for (int half = kRowThreads / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half)
            for (int q = 0; q < N; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x < N) partial[threadIdx.x] = red[threadIdx.x][0];
}

// The view of an entry point's scanned population: the refusals every entry point shares (`kind` matters to the scan alone: every reader of a scanned
// population passes WTK_REPLAY_OPTIMAL), the arrays every reader needs, the geometry and the counts derived from it.  The YOLO loop's entry points, whose
// track is their own output, take the geometry and the counts alone (arrays_required = false) and refuse their own nulls.
inline int replay_view(const char *who, const wtk_replay_config *cfg, int32_t kind, int32_t E, int32_t n_cycles, const double *track_dev, int32_t n_track,
                       const double *share_dev, const int32_t *pos_dev, const int32_t *move_dev, ReplayView &v, bool arrays_required = true) {
    const std::string w(who);
    Geometry &g = v.g;
    if (!cfg) return fail(w + ": null argument");
    if (kind < WTK_REPLAY_CSV || kind > WTK_REPLAY_MLP) return fail(w + ": unknown kind");
    if (E < 1) return fail(w + ": at least one experiment (E >= 1)");
    if (cfg->moving_frame_num < 1) return fail(w + ": moving_frame_num must be at least 1");
    if (cfg->imaging_frame_num < 1) return fail(w + ": imaging_frame_num must be at least 1");
    if (cfg->pred_frame_num > cfg->imaging_frame_num) return fail(w + ": pred_frame_num lies beyond imaging_frame_num");
    if (cfg->pred_frame_num < (kind == WTK_REPLAY_CSV ? 1 : 0)) return fail(w + ": pred_frame_num must be at least 1 for the CSV kind (the controller has not seen the decision frame yet)");
    if (cfg->num_frames < 1 || n_track < 0) return fail(w + ": negative size");
    if (cfg->cam_w < cfg->mic_w || cfg->cam_h < cfg->mic_h) return fail(w + ": the camera is smaller than the microscope");
    if (cfg->mic_w < 0 || cfg->mic_h < 0) return fail(w + ": negative microscope size");
    if (cfg->frame_w < 1 || cfg->frame_h < 1) return fail(w + ": empty frame");
    const long long L = (long long)cfg->imaging_frame_num + cfg->moving_frame_num;
    if (L > INT32_MAX) return fail(w + ": cycle too long");
    const int n_log = (int)((cfg->num_frames - 1) / L); // the last cycle is never logged (its end never arrives)
    if ((long long)n_log * L > n_track) return fail(w + ": the track is shorter than the logged rows");
    if (n_cycles < 1 || n_cycles < n_log) return fail(w + ": n_cycles must cover every logged cycle (and be at least 1)");
    if ((long long)(n_cycles - 1) * L + cfg->imaging_frame_num > (long long)cfg->num_frames - 1)
        return fail(w + ": the decision frame of cycle n_cycles - 1 lies beyond the experiment's frames");
    g.L = (int)L, g.I = cfg->imaging_frame_num, g.M = cfg->moving_frame_num, g.P = cfg->pred_frame_num;
    g.cam_w = cfg->cam_w, g.cam_h = cfg->cam_h, g.mic_w = cfg->mic_w, g.mic_h = cfg->mic_h;
    g.x_max = cfg->frame_w - 1, g.y_max = cfg->frame_h - 1;
    if (arrays_required && (!track_dev || !share_dev || !pos_dev || !move_dev)) return fail(w + ": null argument");
    v.E = E, v.C = n_cycles, v.n_log = n_log, v.R = (long long)n_log * L;
    v.track = track_dev, v.share = share_dev, v.pos = pos_dev, v.move = move_dev;
    return 0;
}

// ---- host launchers that cross translation units, defined in replay.hip
struct ScanArgs {
    Geometry g;
    int kind, E, C;
    int init_x, init_y;
    const double *track; // [n_track][4] xywh
    int n_track;
    const double *a;  // [C][E][2] (CSV: unused)
    const double *b;  // [C][E][2] (MLP only)
    const int *valid; // [C][E] (CSV: unused)
    const double *share; // [M]
    int *pos;  // [C][E][2]
    int *move; // [C][E][2]
    const int *stop; // nullable: *stop != 0 -> the launch touches nothing (the objective entry points only)
};

// The scan of ONE experiment over the C cycles of `a`, from the clamped init position: the move of each cycle from the kind's expression (float64, the
// reference's operation order), then the motor's M steps.  The ONE statement of the scan: replay_scan_kernel runs it per experiment, the set's scan per
// (track, experiment) on that track's slice of the arrays.
__device__ __forceinline__ void scan_experiment(const ScanArgs &a, int e) {
    const Geometry g = a.g;
    int px = a.init_x < 0 ? 0 : (a.init_x > g.x_max ? g.x_max : a.init_x), py = a.init_y < 0 ? 0 : (a.init_y > g.y_max ? g.y_max : a.init_y);
    const double half_w = (double)g.cam_w / 2, half_h = (double)g.cam_h / 2;
    for (int c = 0; c < a.C; ++c) {
        const long long ce = (long long)c * a.E + e;
        a.pos[2 * ce] = px, a.pos[2 * ce + 1] = py;
        const double cam_x = (double)(px - g.cam_w / 2), cam_y = (double)(py - g.cam_h / 2);
        double mx = 0.0, my = 0.0;
        if (a.kind == WTK_REPLAY_CSV) {
            const long long f = (long long)c * g.L + g.I - g.P; // the frame the controller saw P frames before the decision
            if (f >= 0 && f < a.n_track) {
                const double x = a.track[4 * f], y = a.track[4 * f + 1], w = a.track[4 * f + 2], h = a.track[4 * f + 3];
                if (isfinite(x) && isfinite(y) && isfinite(w) && isfinite(h)) {
                    mx = finish_move(((x - cam_x) + w / 2) - half_w);
                    my = finish_move(((y - cam_y) + h / 2) - half_h);
                }
            }
        } else if (a.valid[ce]) {
            const double ax = a.a[2 * ce], ay = a.a[2 * ce + 1];
            if (a.kind == WTK_REPLAY_OPTIMAL) {
                mx = finish_move(ax - (cam_x + half_w));
                my = finish_move(ay - (cam_y + half_h));
            } else if (a.kind == WTK_REPLAY_POLYFIT) {
                mx = finish_move((ax - cam_x) - half_w);
                my = finish_move((ay - cam_y) - half_h);
            } else {
                mx = finish_move(ax + (a.b[2 * ce] - (cam_x + half_w)));
                my = finish_move(ay + (a.b[2 * ce + 1] - (cam_y + half_h)));
            }
        }
        a.move[2 * ce] = (int)mx, a.move[2 * ce + 1] = (int)my;
        motor_steps(g, a.share, g.M, mx, my, px, py);
    }
}

// What a reducing kernel adds of one logged row into its kSummary lane sums, and the row's two errors: the ONE statement of the summary's slots.
__device__ __forceinline__ void row_accumulate(const ReplayView &v, const ReplayRow &w, double (&acc)[kSummary], double &err, double &mse) {
    const RowBoxes &b = w.b;
    err = row_bbox_error(b); // ErrorCalculator.calculate_bbox_error
    // ErrorCalculator.calculate_mse_error: mean over the two axes of the squared centre distance
    const double dx = (b.wx + b.ww / 2) - (b.mic_x + b.mic_w / 2), dy = (b.wy + b.wh / 2) - (b.mic_y + b.mic_h / 2);
    mse = (dx * dx + dy * dy) / 2;
    acc[kRowsErr] += err, acc[kRowsCount] += 1.0;
    if (row_trimmed(v, w.at)) acc[kRowsTrimmedErr] += err, acc[kRowsTrimmedCount] += 1.0;
    if (non_perfect(err)) acc[kRowsNonPerfect] += 1.0;
    acc[kRowsMse] += mse;
}

// checks and argument struct of the scan, apart from its launch: the objective entry points refuse before anything is enqueued
int prepare_scan(const char *who, const wtk_replay_config *cfg, int32_t kind, int32_t E, int32_t n_cycles, const double *track_dev, int32_t n_track,
                 const double *a_dev, const double *b_dev, const int32_t *valid_dev, const double *share_dev, int32_t *pos_dev, int32_t *move_dev, ScanArgs &s);
void launch_scan(const ScanArgs &s, hipStream_t st);
// the chunk partials [E][S][n] of every experiment added in index order into summary [E][n] (the rows reduction and the precise reduction)
void launch_finish(const double *partial, double *summary, int E, int S, int n, const int *stop, hipStream_t st);

// an objective: the division of two summary slots its id stands for
struct ObjectiveRule {
    int id, num, den;    // objective = summary[num] / summary[den]
    bool needs_3_cycles; // the trimmed rows: the first and the last logged cycle are dropped
};

// the objectives over wtk_replay_rows' summary (WTK_REPLAY_OBJ_*): one track's (replay.hip) and a set's pooled slots (replay_set.hip)
inline constexpr ObjectiveRule kRowsObjectives[] = {
    {WTK_REPLAY_OBJ_TRIMMED_BBOX, kRowsTrimmedErr, kRowsTrimmedCount, true},
    {WTK_REPLAY_OBJ_MEAN_BBOX, kRowsErr, kRowsCount, false},
    {WTK_REPLAY_OBJ_MEAN_MSE, kRowsMse, kRowsCount, false},
    {WTK_REPLAY_OBJ_NON_PERFECT, kRowsNonPerfect, kRowsCount, false},
};

// The tail of an objective entry point.  Refuses (null objective_dev, an id outside `rules`, a trimmed objective with fewer than 3 logged cycles) before
// anything is enqueued; otherwise calls `produce`, which enqueues the launches that leave the [E][width] summary at summary_dev (non-zero: it failed),
// and enqueues the division behind them.  Every one of those launches reads the same nullable stop flag.
int enqueue_objective(const char *who, const ObjectiveRule *rules, int n_rules, int32_t objective, const double *summary_dev, int width, int32_t E, int n_log,
                      double *objective_dev, const int32_t *stop_dev, hipStream_t st, const std::function<int()> &produce);

} // namespace wtk
