// Closed-loop replay of track-driven experiments on the device: what the reference's Simulator (wtracker/sim/simulator.py:140-194) + SineMotorController
// (motor_controllers.py:58-88) + LoggingController (logging_controller.py:145-185) do frame by frame for ONE experiment, for a whole population at once,
// with the bounding-box and MSE tracking error of every logged row (eval/error_calculator.py:164-212).
//
// During the imaging phase the platform stands still, so a controller's move is round(f(target_c, platform position)) with a per-cycle target that does
// not depend on the platform: the loop is a sequential scan over cycles (a few flops each) followed by an embarrassingly parallel expansion to frames.
//   scan    one lane per experiment, sequential over cycles: move of the cycle from the kind's expression (float64, the reference's operation order),
//           then the motor's M steps (share * move + carry, rounded half to even, the residual carried, the position clamped to the frame).  Per-cycle
//           inputs are [C][E] (cycle-major), so a wave's loads coalesce.  Writes the position at cycle start and the move, [C][E] int32 pairs.
//   rows    one thread per (experiment, logged frame): the frame's platform position from its cycle's start position and move (at most M motor steps, the
//           scan's arithmetic), camera / microscope / logged worm box, bbox and MSE error of the row; per-experiment sums in a FIXED order: lane-serial
//           over the chunk, a binary tree in LDS, and a finish launch that adds the chunk partials in index order (the scheme of wtk_polyfit_weight_mae).
//           The chunking depends on the row count only: an experiment gives the same bits alone and inside any population.  No floating-point atomics.
//   targets one call for the per-cycle Polyfit targets of a whole POPULATION of weight vectors (the weight search's position buffer, on the device), in the
//           layout the scan reads.  The <= 16 x 8 SVD of a fit depends on the weights and on WHICH samples of the cycle are finite only, so the cycles are
//           grouped by that set (a <= 16-bit mask; the caller derives the classes from the track once): pass A solves one SVD per (class, particle) and
//           keeps the rotated matrix, V, s^2, scl and the compacted weights particle-minor in scratch; pass B, one thread per (cycle, particle), reads its
//           class's record and the cycle's centres (LDS: one cycle per block) and solves and evaluates.  Both passes call the functions
//           track_polyfit_kernel calls (polyfit_solve.h: polyfit_factor, polyfit_eval_axes), so the targets have that kernel's bits.
//   objective  scan + rows (no row, per-row or slot output) + one division per experiment: the swarm's objective without a host round trip.
//   yolo    the YOLO controller's loop, whose targets depend on the camera view: between two single-frame detector calls ONE thread
//           turns the detector's float32 row into the move (numpy's float32 arithmetic of HipYoloController.provide_movement_vector) and the next cycle's
//           position, where wtk_yolo_predict_views reads it; after the loop one thread per logged frame gives the frame's platform position (the
//           detector's pos_xy for the log pass) and one thread per logged frame turns view-pixel detections into the absolute float64 track the rows
//           kernel reads (TrackLogger's per-cycle float32 / float64 rule).  The motor is motor_steps() / frame_position(), shared with scan and rows.
//   A nullable stop flag (the swarm's ctrl word) turns the targets, the objective and, through them only, the scan and the rows reduction into no-ops.
// Everything relies on -ffp-contract=off (the library's build flag): share * move + carry is a rounded product and a rounded sum, as in Python.
#include "wtk_internal.h"
#include "polyfit_solve.h"

#include <cmath>

using namespace wtk;

namespace {

constexpr int kScanThreads = 64;
constexpr int kRowThreads = 256;
constexpr int kRowChunk = 4096; // logged rows per block of the rows kernel: the FIXED chunking of the reductions
constexpr int kSummary = WTK_REPLAY_SUMMARY_DOUBLES;
constexpr int kRowDoubles = WTK_REPLAY_ROW_DOUBLES;
constexpr double kMoveMax = 1073741824.0; // 2^30: moves are kept as int32

struct Geometry {
    int L, I, M, P;
    int cam_w, cam_h, mic_w, mic_h;
    int x_max, y_max; // frame_w - 1, frame_h - 1: the clamp of the platform position
};

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
    const int *stop; // nullable: *stop != 0 -> the launch touches nothing (wtk_replay_objective only)
};

struct RowsArgs {
    Geometry g;
    int E, C, S, n_slots;
    long long R; // logged rows per experiment
    int n_log;   // logged cycles
    const double *track;
    const double *share;
    const int *pos, *move; // [C][E][2]
    const int *row_slot;   // [E] slot of the experiment in `rows`, or -1 (nullable)
    double *rows;          // [slots][R][kRowDoubles] (nullable)
    double *bbox_err, *mse_err; // [E][R] (nullable)
    double *partial;       // [E][S][kSummary]
    double *summary;       // [E][kSummary]
    const int *stop;       // nullable, as ScanArgs::stop
};

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

struct ObjectiveArgs {
    const double *summary; // [E][kSummary]
    double *objective;     // [E]
    int E, num, den;       // objective = summary[num] / summary[den]
    const int *stop;
};

struct YoloStepArgs {
    Geometry g;
    int c, C;
    const float *xywh;   // [4] the single-frame call's row, view pixels; NaN x 4 = no detection
    const double *share; // [M]
    int *pos;            // [C][1][2]: reads pos[c], writes pos[c + 1] (where c + 1 < C)
    int *move;           // [C][1][2]: writes move[c]
};

struct YoloFramesArgs {
    Geometry g;
    long long R; // logged rows
    const double *share;
    const int *pos, *move; // [C][1][2]
    int *frame_pos;        // [R][2] platform position at every logged frame's camera picture (the positions kernel writes it)
    const int *frame_pos_in; // the same array as the track kernel reads it
    const float *xywh;     // [R][4] detections in view pixels
    double *track;         // [R][4] absolute xywh
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

// the controller's move on one axis from the camera corner; a non-finite result is no move, a huge one saturates at +-2^30
__device__ __forceinline__ double finish_move(double v) {
    if (!isfinite(v)) return 0.0;
    return fmin(fmax(rint(v), -kMoveMax), kMoveMax);
}

__global__ __launch_bounds__(kScanThreads) void replay_scan_kernel(const ScanArgs a) {
    if (a.stop && *a.stop) return;
    const int e = blockIdx.x * kScanThreads + threadIdx.x;
    if (e >= a.E) return;
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

__global__ __launch_bounds__(kRowThreads) void replay_rows_kernel(const RowsArgs a) {
    __shared__ double red[kSummary][kRowThreads];
    if (a.stop && *a.stop) return; // block-uniform
    const Geometry g = a.g;
    const int e = blockIdx.x / a.S, s = blockIdx.x - e * a.S;
    int slot = a.row_slot ? a.row_slot[e] : -1;
    if (slot >= a.n_slots) slot = -1; // never write past `rows`
    double acc[kSummary];
    for (int q = 0; q < kSummary; ++q) acc[q] = 0.0;
    const long long r0 = (long long)s * kRowChunk;
    for (int i = 0; i < kRowChunk / kRowThreads; ++i) {
        const long long r = r0 + (long long)i * kRowThreads + threadIdx.x;
        if (r >= a.R) continue;
        const int c = (int)(r / g.L), step = (int)(r - (long long)c * g.L);
        const long long ce = (long long)c * a.E + e;
        int px, py;
        frame_position(g, a.share, a.pos, a.move, ce, step, px, py);
        const double cam_x = (double)(px - g.cam_w / 2), cam_y = (double)(py - g.cam_h / 2);
        const double mic_x = (double)(px - g.mic_w / 2), mic_y = (double)(py - g.mic_h / 2);
        const double mic_w = (double)g.mic_w, mic_h = (double)g.mic_h;
        // the logged worm box: camera-relative (CsvController.predict) and back (LoggingController), a non-finite row as zeros
        double wx = (a.track[4 * r] - cam_x) + cam_x, wy = (a.track[4 * r + 1] - cam_y) + cam_y, ww = a.track[4 * r + 2], wh = a.track[4 * r + 3];
        if (!(isfinite(wx) && isfinite(wy) && isfinite(ww) && isfinite(wh))) wx = wy = ww = wh = 0.0;
        // ErrorCalculator.calculate_bbox_error
        const double il = fmax(wx, mic_x), it = fmax(wy, mic_y);
        const double ir = fmin(wx + ww, mic_x + mic_w), ib = fmin(wy + wh, mic_y + mic_h);
        const double iw = fmax(0.0, ir - il), ih = fmax(0.0, ib - it);
        const double inter = iw * ih, total = ww * wh;
        const double err = total == 0.0 ? 0.0 : 1.0 - inter / total;
        // ErrorCalculator.calculate_mse_error: mean over the two axes of the squared centre distance
        const double dx = (wx + ww / 2) - (mic_x + mic_w / 2), dy = (wy + wh / 2) - (mic_y + mic_h / 2);
        const double mse = (dx * dx + dy * dy) / 2;
        const bool imaging = step < g.I;
        if (a.bbox_err) a.bbox_err[(long long)e * a.R + r] = err;
        if (a.mse_err) a.mse_err[(long long)e * a.R + r] = mse;
        if (slot >= 0 && a.rows) {
            double *o = a.rows + ((long long)slot * a.R + r) * kRowDoubles;
            o[0] = (double)px, o[1] = (double)py;
            o[2] = cam_x, o[3] = cam_y, o[4] = (double)g.cam_w, o[5] = (double)g.cam_h;
            o[6] = mic_x, o[7] = mic_y, o[8] = mic_w, o[9] = mic_h;
            o[10] = wx, o[11] = wy, o[12] = ww, o[13] = wh;
            o[14] = (double)c, o[15] = imaging ? 0.0 : 1.0;
        }
        const bool trimmed = imaging && c != 0 && c != a.n_log - 1; // DataAnalyzer.clean(trim_cycles=True, imaging_only=True)
        acc[0] += err, acc[1] += 1.0;
        if (trimmed) acc[2] += err, acc[3] += 1.0;
        if (err > 1e-7) acc[4] += 1.0;
        acc[5] += mse;
    }
    for (int q = 0; q < kSummary; ++q) red[q][threadIdx.x] = acc[q];
    __syncthreads();
    for (int half = kRowThreads / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half)
            for (int q = 0; q < kSummary; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x < kSummary) a.partial[((long long)e * a.S + s) * kSummary + threadIdx.x] = red[threadIdx.x][0];
}

__global__ __launch_bounds__(64) void replay_finish_kernel(const RowsArgs a) {
    if (a.stop && *a.stop) return;
    const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
    if (i >= (long long)a.E * kSummary) return;
    const long long e = i / kSummary;
    const int q = (int)(i - e * kSummary);
    double sum = 0.0;
    for (int s = 0; s < a.S; ++s) sum += a.partial[(e * a.S + s) * kSummary + q];
    a.summary[i] = sum;
}

__global__ __launch_bounds__(64) void replay_objective_kernel(const ObjectiveArgs a) {
    if (a.stop && *a.stop) return;
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= a.E) return;
    // the float64 division Summary's properties perform on the host (counts are exact doubles); 0 / 0 = NaN, which the swarm never lets win
    a.objective[e] = a.summary[(long long)e * kSummary + a.num] / a.summary[(long long)e * kSummary + a.den];
}

// The YOLO controller between two single-frame detector calls: HipYoloController.provide_movement_vector on the row where the detector left it, then the
// cycle's motor steps.  The row is float32 and numpy keeps it so: mid = x + w / 2 and mid - cam_size / 2 are float32 operations (the Python float is weak),
// round() is half to even on that float32 value.  One thread: a cycle is a few dozen flops.
__global__ __launch_bounds__(64) void replay_yolo_step_kernel(const YoloStepArgs a) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const Geometry g = a.g;
    int px = a.pos[2 * a.c], py = a.pos[2 * a.c + 1];
    const float x = a.xywh[0], y = a.xywh[1], w = a.xywh[2], h = a.xywh[3];
    double mx = 0.0, my = 0.0;
    if (isfinite(x) && isfinite(y) && isfinite(w) && isfinite(h)) {
        const float mid_x = x + w / 2.f, mid_y = y + h / 2.f;
        const float half_w = (float)((double)g.cam_w / 2), half_h = (float)((double)g.cam_h / 2);
        mx = finish_move((double)(mid_x - half_w)); // rint of a float32 value is the same number in float64
        my = finish_move((double)(mid_y - half_h));
    }
    a.move[2 * a.c] = (int)mx, a.move[2 * a.c + 1] = (int)my;
    motor_steps(g, a.share, g.M, mx, my, px, py);
    if (a.c + 1 < a.C) a.pos[2 * (a.c + 1)] = px, a.pos[2 * (a.c + 1) + 1] = py;
}

// one thread per logged frame: the position wtk_yolo_predict_views cuts the frame's camera view at (the rows kernel's position of that row)
__global__ __launch_bounds__(kRowThreads) void replay_yolo_positions_kernel(const YoloFramesArgs a) {
    const long long r = (long long)blockIdx.x * kRowThreads + threadIdx.x;
    if (r >= a.R) return;
    const Geometry g = a.g;
    const int c = (int)(r / g.L), step = (int)(r - (long long)c * g.L);
    int px, py;
    frame_position(g, a.share, a.pos, a.move, c, step, px, py);
    a.frame_pos[2 * r] = px, a.frame_pos[2 * r + 1] = py;
}

__device__ __forceinline__ bool finite_row(const float *v) { return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]) && isfinite(v[3]); }

// one thread per logged frame: TrackLogger._write_rows' `boxes[:, 0] += cams[:, 0]` with the dtype the cycle's batch has there.  A cycle without a miss
// is a float32 array (the sum is rounded to float32, then widened); one NaN row makes the whole cycle float64.  Misses stay NaN.
__global__ __launch_bounds__(kRowThreads) void replay_yolo_track_kernel(const YoloFramesArgs a) {
    const long long r = (long long)blockIdx.x * kRowThreads + threadIdx.x;
    if (r >= a.R) return;
    const Geometry g = a.g;
    const long long first = r / g.L * g.L;
    bool any_miss = false;
    for (int i = 0; i < g.L; ++i) any_miss |= !finite_row(a.xywh + 4 * (first + i));
    const float *v = a.xywh + 4 * r;
    double *o = a.track + 4 * r;
    if (!finite_row(v)) {
        const double nanv = __builtin_nan("");
        o[0] = o[1] = o[2] = o[3] = nanv;
        return;
    }
    const int cam_x = a.frame_pos_in[2 * r] - g.cam_w / 2, cam_y = a.frame_pos_in[2 * r + 1] - g.cam_h / 2;
    if (any_miss) {
        o[0] = (double)v[0] + (double)cam_x, o[1] = (double)v[1] + (double)cam_y;
    } else {
        o[0] = (double)(v[0] + (float)cam_x), o[1] = (double)(v[1] + (float)cam_y);
    }
    o[2] = (double)v[2], o[3] = (double)v[3];
}

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

// the refusals both entry points share; fills the geometry and the counts derived from it
int check_config(const char *who, const wtk_replay_config *cfg, int32_t kind, int32_t E, int32_t n_cycles, int32_t n_track, Geometry &g, int &n_log) {
    const std::string w(who);
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
    n_log = (int)((cfg->num_frames - 1) / L); // the last cycle is never logged (its end never arrives)
    if ((long long)n_log * L > n_track) return fail(w + ": the track is shorter than the logged rows");
    if (n_cycles < 1 || n_cycles < n_log) return fail(w + ": n_cycles must cover every logged cycle (and be at least 1)");
    if ((long long)(n_cycles - 1) * L + cfg->imaging_frame_num > (long long)cfg->num_frames - 1)
        return fail(w + ": the decision frame of cycle n_cycles - 1 lies beyond the experiment's frames");
    g.L = (int)L, g.I = cfg->imaging_frame_num, g.M = cfg->moving_frame_num, g.P = cfg->pred_frame_num;
    g.cam_w = cfg->cam_w, g.cam_h = cfg->cam_h, g.mic_w = cfg->mic_w, g.mic_h = cfg->mic_h;
    g.x_max = cfg->frame_w - 1, g.y_max = cfg->frame_h - 1;
    return 0;
}

// checks and argument structs of the two steps, apart from their launches: wtk_replay_objective refuses before anything is enqueued
int prepare_scan(const char *who, const wtk_replay_config *cfg, int32_t kind, int32_t E, int32_t n_cycles, const double *track_dev, int32_t n_track,
                 const double *a_dev, const double *b_dev, const int32_t *valid_dev, const double *share_dev, int32_t *pos_dev, int32_t *move_dev, ScanArgs &s) {
    const std::string w(who);
    int n_log = 0;
    if (check_config(who, cfg, kind, E, n_cycles, n_track, s.g, n_log)) return 1;
    if (!track_dev || !share_dev || !pos_dev || !move_dev) return fail(w + ": null argument");
    if (kind != WTK_REPLAY_CSV && (!a_dev || !valid_dev)) return fail(w + ": null targets");
    if (kind == WTK_REPLAY_MLP && !b_dev) return fail(w + ": null origins (b_dev) for the MLP kind");
    s.kind = kind, s.E = E, s.C = n_cycles, s.init_x = cfg->init_x, s.init_y = cfg->init_y;
    s.track = track_dev, s.n_track = n_track, s.a = a_dev, s.b = b_dev, s.valid = valid_dev, s.share = share_dev, s.pos = pos_dev, s.move = move_dev;
    return 0;
}

void launch_scan(const ScanArgs &s, hipStream_t st) {
    hipLaunchKernelGGL(replay_scan_kernel, dim3((unsigned)((s.E + kScanThreads - 1) / kScanThreads)), dim3(kScanThreads), 0, st, s);
}

int prepare_rows(const char *who, const wtk_replay_config *cfg, int32_t E, int32_t n_cycles, const double *track_dev, int32_t n_track, const double *share_dev,
                 const int32_t *pos_dev, const int32_t *move_dev, const int32_t *row_slot_dev, int32_t n_slots, double *rows_dev, double *bbox_err_dev,
                 double *mse_err_dev, double *summary_dev, double *scratch_dev, int64_t scratch_doubles, RowsArgs &r) {
    const std::string w(who);
    int n_log = 0;
    if (check_config(who, cfg, WTK_REPLAY_OPTIMAL, E, n_cycles, n_track, r.g, n_log)) return 1;
    if (!track_dev || !share_dev || !pos_dev || !move_dev || !summary_dev || !scratch_dev) return fail(w + ": null argument");
    if ((row_slot_dev == nullptr) != (rows_dev == nullptr) || n_slots < 0 || (rows_dev && n_slots < 1))
        return fail(w + ": row_slot_dev, rows_dev and n_slots >= 1 go together");
    r.R = (long long)n_log * r.g.L;
    const long long S = (r.R + kRowChunk - 1) / kRowChunk;
    if (S * E > INT32_MAX) return fail(w + ": too many (experiment, chunk) blocks for one launch");
    if (scratch_doubles < wtk_replay_scratch_doubles(E, r.R)) return fail(w + ": scratch smaller than wtk_replay_scratch_doubles(E, R)");
    r.E = E, r.C = n_cycles, r.S = (int)S, r.n_log = n_log, r.n_slots = rows_dev ? n_slots : 0;
    r.track = track_dev, r.share = share_dev, r.pos = pos_dev, r.move = move_dev, r.row_slot = row_slot_dev, r.rows = rows_dev;
    r.bbox_err = bbox_err_dev, r.mse_err = mse_err_dev, r.partial = scratch_dev, r.summary = summary_dev;
    return 0;
}

void launch_rows(const RowsArgs &r, hipStream_t st) {
    if (r.S > 0) hipLaunchKernelGGL(replay_rows_kernel, dim3((unsigned)((long long)r.S * r.E)), dim3(kRowThreads), 0, st, r);
    hipLaunchKernelGGL(replay_finish_kernel, dim3((unsigned)(((long long)r.E * kSummary + 63) / 64)), dim3(64), 0, st, r);
}

} // namespace

extern "C" int wtk_replay_scan(const wtk_replay_config *cfg, int32_t kind, int32_t E, int32_t n_cycles, const double *track_dev, int32_t n_track,
                               const double *a_dev, const double *b_dev, const int32_t *valid_dev, const double *share_dev, int32_t *pos_dev,
                               int32_t *move_dev, void *stream) {
    ScanArgs s = {};
    if (prepare_scan("wtk_replay_scan", cfg, kind, E, n_cycles, track_dev, n_track, a_dev, b_dev, valid_dev, share_dev, pos_dev, move_dev, s)) return 1;
    launch_scan(s, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int64_t wtk_replay_scratch_doubles(int32_t E, int64_t R) {
    if (E < 0 || R < 0) return -1;
    return (int64_t)E * ((R + kRowChunk - 1) / kRowChunk) * kSummary;
}

extern "C" int wtk_replay_rows(const wtk_replay_config *cfg, int32_t E, int32_t n_cycles, const double *track_dev, int32_t n_track,
                               const double *share_dev, const int32_t *pos_dev, const int32_t *move_dev, const int32_t *row_slot_dev, int32_t n_slots, double *rows_dev,
                               double *bbox_err_dev, double *mse_err_dev, double *summary_dev, double *scratch_dev, int64_t scratch_doubles,
                               void *stream) {
    RowsArgs r = {};
    if (prepare_rows("wtk_replay_rows", cfg, E, n_cycles, track_dev, n_track, share_dev, pos_dev, move_dev, row_slot_dev, n_slots, rows_dev, bbox_err_dev,
                     mse_err_dev, summary_dev, scratch_dev, scratch_doubles, r))
        return 1;
    launch_rows(r, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int wtk_replay_objective(const wtk_replay_config *cfg, int32_t kind, int32_t E, int32_t n_cycles, const double *track_dev, int32_t n_track,
                                    const double *a_dev, const double *b_dev, const int32_t *valid_dev, const double *share_dev, int32_t *pos_dev,
                                    int32_t *move_dev, double *summary_dev, double *scratch_dev, int64_t scratch_doubles, int32_t objective,
                                    double *objective_dev, const int32_t *stop_dev, void *stream) {
    ScanArgs s = {};
    RowsArgs r = {};
    if (prepare_scan("wtk_replay_objective", cfg, kind, E, n_cycles, track_dev, n_track, a_dev, b_dev, valid_dev, share_dev, pos_dev, move_dev, s)) return 1;
    if (prepare_rows("wtk_replay_objective", cfg, E, n_cycles, track_dev, n_track, share_dev, pos_dev, move_dev, nullptr, 0, nullptr, nullptr, nullptr,
                     summary_dev, scratch_dev, scratch_doubles, r))
        return 1;
    if (!objective_dev) return fail("wtk_replay_objective: null argument");
    ObjectiveArgs o = {};
    switch (objective) {
    case WTK_REPLAY_OBJ_TRIMMED_BBOX: o.num = 2, o.den = 3; break;
    case WTK_REPLAY_OBJ_MEAN_BBOX: o.num = 0, o.den = 1; break;
    case WTK_REPLAY_OBJ_MEAN_MSE: o.num = 5, o.den = 1; break;
    case WTK_REPLAY_OBJ_NON_PERFECT: o.num = 4, o.den = 1; break;
    default: return fail("wtk_replay_objective: unknown objective");
    }
    if (objective == WTK_REPLAY_OBJ_TRIMMED_BBOX && r.n_log < 3)
        return fail("wtk_replay_objective: the trimmed objective needs at least 3 logged cycles (the first and the last are dropped)");
    s.stop = r.stop = o.stop = stop_dev;
    o.summary = summary_dev, o.objective = objective_dev, o.E = E;
    hipStream_t st = (hipStream_t)stream;
    launch_scan(s, st);
    launch_rows(r, st);
    hipLaunchKernelGGL(replay_objective_kernel, dim3((unsigned)((E + 63) / 64)), dim3(64), 0, st, o);
    HIP_TRY(hipGetLastError());
    return 0;
}

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

// ---- the YOLO controller's loop: E = 1, every per-cycle array is [n_cycles][1][2]
namespace {

int check_yolo(const char *who, const wtk_replay_config *cfg, int32_t n_cycles, Geometry &g, long long &R) {
    int n_log = 0;
    // (the track these calls stand for is the detector's own output: it always has the R logged rows; pred_frame_num = 0 is the controller's oldest frame)
    if (check_config(who, cfg, WTK_REPLAY_OPTIMAL, 1, n_cycles, INT32_MAX, g, n_log)) return 1;
    if (g.cam_w > 8192 || g.cam_h > 8192 || cfg->frame_w > 8192 || cfg->frame_h > 8192)
        return fail(std::string(who) + ": camera and frame sizes up to 8192 (the float32 sums of the log are exact in the rows' float64 round trip below 2^13)");
    R = (long long)n_log * g.L;
    return 0;
}

} // namespace

extern "C" int wtk_replay_yolo_step(const wtk_replay_config *cfg, int32_t n_cycles, int32_t c, const float *xywh_dev, const double *share_dev,
                                    int32_t *pos_dev, int32_t *move_dev, void *stream) {
    YoloStepArgs a = {};
    long long R = 0;
    if (check_yolo("wtk_replay_yolo_step", cfg, n_cycles, a.g, R)) return 1;
    if (!xywh_dev || !share_dev || !pos_dev || !move_dev) return fail("wtk_replay_yolo_step: null argument");
    if (c < 0 || c >= n_cycles) return fail("wtk_replay_yolo_step: cycle outside [0, n_cycles)");
    a.c = c, a.C = n_cycles, a.xywh = xywh_dev, a.share = share_dev, a.pos = pos_dev, a.move = move_dev;
    hipLaunchKernelGGL(replay_yolo_step_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int wtk_replay_yolo_positions(const wtk_replay_config *cfg, int32_t n_cycles, const double *share_dev, const int32_t *pos_dev,
                                         const int32_t *move_dev, int32_t *frame_pos_dev, void *stream) {
    YoloFramesArgs a = {};
    if (check_yolo("wtk_replay_yolo_positions", cfg, n_cycles, a.g, a.R)) return 1;
    if (!share_dev || !pos_dev || !move_dev || !frame_pos_dev) return fail("wtk_replay_yolo_positions: null argument");
    a.share = share_dev, a.pos = pos_dev, a.move = move_dev, a.frame_pos = frame_pos_dev;
    if (a.R > 0) hipLaunchKernelGGL(replay_yolo_positions_kernel, dim3((unsigned)((a.R + kRowThreads - 1) / kRowThreads)), dim3(kRowThreads), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int wtk_replay_yolo_track(const wtk_replay_config *cfg, int32_t n_cycles, const float *xywh_dev, const int32_t *frame_pos_dev, double *track_dev,
                                     void *stream) {
    YoloFramesArgs a = {};
    if (check_yolo("wtk_replay_yolo_track", cfg, n_cycles, a.g, a.R)) return 1;
    if (!xywh_dev || !frame_pos_dev || !track_dev) return fail("wtk_replay_yolo_track: null argument");
    a.xywh = xywh_dev, a.frame_pos_in = frame_pos_dev, a.track = track_dev;
    if (a.R > 0) hipLaunchKernelGGL(replay_yolo_track_kernel, dim3((unsigned)((a.R + kRowThreads - 1) / kRowThreads)), dim3(kRowThreads), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}
