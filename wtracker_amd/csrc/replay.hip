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
//   precise the reference's analysis metric (ErrorCalculator.calculate_precise: the share of the worm's segmented pixels outside the microscope view) of
//           every (experiment, logged frame) pair, DESIGN.md section 19.  The segmented mask of frame r depends on the frame, the background and the
//           track's row r only, so ONE workgroup per frame builds it once, as an exclusive summed-area table in LDS, and answers every experiment with
//           two rectangle sums: O(F area + E F) pixel work, not O(E F area).  See replay_precise_kernel.
//   A nullable stop flag (the swarm's ctrl word) turns the targets, the objective and, through them only, the scan and the rows reduction into no-ops.
// Everything relies on -ffp-contract=off (the library's build flag): share * move + carry is a rounded product and a rounded sum, as in Python.
#include "wtk_internal.h"
#include "eval_device.h"
#include "polyfit_solve.h"
#include "replay_device.h"

#include <algorithm>
#include <cmath>

using namespace wtk;

namespace {

constexpr int kScanThreads = 64;
constexpr int kRowThreads = 256;
constexpr int kRowChunk = 4096; // logged rows per block of the rows kernel: the FIXED chunking of the reductions
constexpr int kSummary = WTK_REPLAY_SUMMARY_DOUBLES;
constexpr int kRowDoubles = WTK_REPLAY_ROW_DOUBLES;
constexpr double kMoveMax = 1073741824.0; // 2^30: moves are kept as int32
constexpr int kPreciseThreads = 256;
constexpr int kPreciseSummary = WTK_REPLAY_PRECISE_SUMMARY_DOUBLES;
constexpr int kPreciseLdsBytes = 160 * 1024;            // the CU's LDS: one workgroup per CU takes all of it at the default limit
constexpr int kPreciseMaxCells = kPreciseLdsBytes / 4;  // uint32 cells of the largest table


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

struct FinishArgs {
    const double *partial; // [E][S][n]
    double *summary;       // [E][n]
    int E, S, n;
    const int *stop;
};

struct ObjectiveArgs {
    const double *summary; // [E][n]
    double *objective;     // [E]
    int E, n, num, den;    // objective = summary[num] / summary[den]
    const int *stop;
};

struct PreciseArgs {
    Geometry g;
    int E, C, S, n_log;
    long long R;
    const double *track;
    const double *share;
    const int *pos, *move; // [C][E][2]
    const uint8_t *frames; // [n_frames][H][W] gray, row r is frame r
    const uint8_t *bg;     // [H][W]
    int H, W, thr;         // a pixel is foreground where |frame - bg| > thr
    int max_cells;         // a frame whose table needs more uint32 cells walks its crops instead
    double *pair;          // [R][E] the error of every pair, NaN = no value
    int *walk;             // [R] != 0: the frame has pairs the table did not answer (replay_precise_walk_kernel)
    double *err;           // [E][R] (nullable)
    int *counts;           // [E][R][2] (total, inside) (nullable)
    double *partial;       // [E][S][kPreciseSummary]
    double *summary;       // [E][kPreciseSummary]
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
        const RowBoxes b = row_boxes(g, a.track + 4 * r, px, py);
        const double cam_x = b.cam_x, cam_y = b.cam_y, mic_x = b.mic_x, mic_y = b.mic_y, mic_w = b.mic_w, mic_h = b.mic_h;
        const double wx = b.wx, wy = b.wy, ww = b.ww, wh = b.wh;
        const double err = row_bbox_error(b); // ErrorCalculator.calculate_bbox_error
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

// the chunk partials of every experiment added in index order (the rows reduction and the precise reduction)
__global__ __launch_bounds__(64) void replay_finish_kernel(const FinishArgs a) {
    if (a.stop && *a.stop) return;
    const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
    if (i >= (long long)a.E * a.n) return;
    const long long e = i / a.n;
    const int q = (int)(i - e * a.n);
    double sum = 0.0;
    for (int s = 0; s < a.S; ++s) sum += a.partial[(e * a.S + s) * a.n + q];
    a.summary[i] = sum;
}

__global__ __launch_bounds__(64) void replay_objective_kernel(const ObjectiveArgs a) {
    if (a.stop && *a.stop) return;
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= a.E) return;
    // the float64 division Summary's properties perform on the host (counts are exact doubles); 0 / 0 = NaN, which the swarm never lets win
    a.objective[e] = a.summary[(long long)e * a.n + a.num] / a.summary[(long long)e * a.n + a.den];
}

// sum of the exclusive summed-area table over [l, r) x [t, b) in table coordinates; uint32 arithmetic wraps and the result is exact
__device__ __forceinline__ int sat_rect(const unsigned *sat, int pitch, int l, int t, int r, int b) {
    return (int)(sat[b * pitch + r] - sat[t * pitch + r] - sat[b * pitch + l] + sat[t * pitch + l]);
}

// The precise error of every experiment at ONE logged frame r = blockIdx.x (row r is frame r).
//
// Phase 1, once per frame.  The track's row r is discretised as BoxUtils.discretize does, grown by one pixel on every side (the logged box of an
// experiment is the row after (x - cam) + cam, which moves an edge by at most one pixel: DESIGN.md section 19) and clipped to the frame: the padded
// region, pw x ph pixels.  |frame - bg| > thr over it becomes an exclusive summed-area table of (ph + 1) x (pw + 1) uint32 in dynamic LDS:
//   fill    a wave per region row, lane = column: byte loads of 64 consecutive pixels of the frame and of the background (row-contiguous; no alignment
//           of the base or of W is assumed, and the region is a few dozen KB at most, read once), ds_write_b32 of consecutive words.
//   rows    a thread per table row, serial along x.  Lane l of a 32-lane group reads word l * pitch + x: ds_read_b32 / ds_write_b32 bank on 32 words,
//           so the 32 rows hit 32 different banks exactly when the pitch is ODD.  pitch = (pw + 1) | 1.
//   columns a thread per table column, serial along y: lanes read consecutive words, conflict-free for any pitch.
// A row pass of h threads x w steps leaves most of the block idle; it is O(w + h) LDS round trips per frame and runs once for all E experiments.
//
// Phase 2.  Threads stride over the experiments: platform position of (e, r) (frame_position), the row's boxes (row_boxes), both discretised, then
// total = the table over the logged worm box and inside = the table over worm x microscope.  An EMPTY intersection is decided first: its corner may lie
// outside the worm box and the table.  err = 1 - inside / total in float64, 0 where total = 0, NaN for an illegal worm box: precise_error_kernel's rules
// (eval_device.h) and its counts.
//
// Exact fallback.  A pair whose logged box is not inside the padded region (never seen; an illegal track row with a legal logged box would be one) and
// every pair of a frame whose table does not fit `max_cells` is left to replay_precise_walk_kernel, which this kernel tells through walk[r] whether
// frame r has such a pair.  That kernel asks for no LDS, so its waves fill the CUs; here a block that holds 160 KiB would walk with 4 waves per CU
// (measured: 4 x slower than the per-row kernel).  It walks the crop with crop_walk, precise_error_kernel's loop: the lanes that need it are collected
// with a ballot and the whole wave walks them one after the other.  Both ways count the same pixels, so the limit never changes a bit.
//
// Occupancy: at the default limit a workgroup asks for all 160 KiB of LDS, so one workgroup (4 waves) runs per CU, 256 frames at a time on the device; a
// handful of frames leaves most CUs idle, and nothing hides the latency of phase 1's dependent LDS passes.
struct PreciseRegion {
    int pl, pt, pr, pb; // the padded region of the frame, empty where the track's row is illegal
    int pitch;          // of its table, in words
    bool table;         // the table fits max_cells: replay_precise_kernel builds it
};

__device__ __forceinline__ PreciseRegion precise_region(const PreciseArgs &a, long long r) {
    PreciseRegion g;
    const bool track_legal = discretize(a.track + 4 * r, a.H, a.W, g.pl, g.pt, g.pr, g.pb);
    if (track_legal) g.pl = max(g.pl - 1, 0), g.pt = max(g.pt - 1, 0), g.pr = min(g.pr + 1, a.W), g.pb = min(g.pb + 1, a.H);
    g.pitch = (g.pr - g.pl + 1) | 1;
    g.table = track_legal && (long long)(g.pb - g.pt + 1) * g.pitch <= a.max_cells;
    return g;
}

// Phase 2 over the experiments of frame r.  kWalk = false: the pairs the table answers and the pairs without a value; returns whether a pair of this
// thread is left to the walk.  kWalk = true: exactly those pairs, by the walk (`sat` is not read).  Every thread of the block must call it.
template <bool kWalk> __device__ __forceinline__ bool precise_pairs(const PreciseArgs &a, long long r, const PreciseRegion &reg, const unsigned *sat) {
    const Geometry g = a.g;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint8_t *fr = a.frames + r * a.H * a.W;
    const int c = (int)(r / g.L), step = (int)(r - (long long)c * g.L);
    bool left = false;
    for (int e0 = wave * 64; e0 < a.E; e0 += kPreciseThreads) { // wave-uniform trip count: the ballot below sees the whole wave
        const int e = e0 + lane;
        int wl = 0, wt = 0, wr = 0, wb = 0, il = 0, it = 0, ir = 0, ib = 0, total = 0, inside = 0;
        bool legal = false, walk = false;
        if (e < a.E) {
            int px, py, ml, mt, mr, mb;
            frame_position(g, a.share, a.pos, a.move, (long long)c * a.E + e, step, px, py);
            const RowBoxes b = row_boxes(g, a.track + 4 * r, px, py);
            const double worm[4] = {b.wx, b.wy, b.ww, b.wh}, mic[4] = {b.mic_x, b.mic_y, b.mic_w, b.mic_h};
            legal = discretize(worm, a.H, a.W, wl, wt, wr, wb);
            if (legal) {
                discretize(mic, a.H, a.W, ml, mt, mr, mb); // an illegal microscope box is (0, 0, 0, 0): an empty intersection
                intersect(wl, wt, wr, wb, ml, mt, mr, mb, il, it, ir, ib);
                walk = !(reg.table && wl >= reg.pl && wt >= reg.pt && wr <= reg.pr && wb <= reg.pb);
                if (!kWalk && !walk) {
                    total = sat_rect(sat, reg.pitch, wl - reg.pl, wt - reg.pt, wr - reg.pl, wb - reg.pt);
                    inside = (ir > il && ib > it) ? sat_rect(sat, reg.pitch, il - reg.pl, it - reg.pt, ir - reg.pl, ib - reg.pt) : 0; // non-empty: inside the worm box
                }
            }
        }
        left |= walk;
        if (kWalk) {
            for (unsigned long long todo = __ballot(walk); todo; todo &= todo - 1) {
                const int j = __ffsll((long long)todo) - 1;
                int t, in;
                crop_walk(fr, a.bg, a.W, a.thr, lane, __shfl(wl, j), __shfl(wt, j), __shfl(wr, j), __shfl(wb, j), __shfl(il, j), __shfl(it, j),
                          __shfl(ir, j), __shfl(ib, j), t, in);
                if (lane == j) total = t, inside = in;
            }
        }
        if (e < a.E && walk == kWalk) {
            const double err = legal ? precise_error_of(total, inside) : __builtin_nan("");
            a.pair[r * a.E + e] = err;
            if (a.err) a.err[(long long)e * a.R + r] = err;
            if (a.counts) a.counts[2 * ((long long)e * a.R + r)] = total, a.counts[2 * ((long long)e * a.R + r) + 1] = inside;
        }
    }
    return left;
}

__global__ __launch_bounds__(kPreciseThreads) void replay_precise_kernel(const PreciseArgs a) {
    extern __shared__ unsigned sat[];
    if (a.stop && *a.stop) return; // block-uniform
    const long long r = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint8_t *fr = a.frames + r * a.H * a.W;
    const PreciseRegion reg = precise_region(a, r);
    const int pl = reg.pl, pt = reg.pt, pw = reg.pr - reg.pl, ph = reg.pb - reg.pt, pitch = reg.pitch;
    if (reg.table) { // block-uniform
        for (int x = threadIdx.x; x <= pw; x += kPreciseThreads) sat[x] = 0u;
        for (int y = 1 + threadIdx.x; y <= ph; y += kPreciseThreads) sat[y * pitch] = 0u;
        for (int y = wave; y < ph; y += kPreciseThreads / 64) {
            const long long o = (long long)(pt + y) * a.W + pl;
            for (int x = lane; x < pw; x += 64) sat[(y + 1) * pitch + x + 1] = abs((int)fr[o + x] - (int)a.bg[o + x]) > a.thr ? 1u : 0u;
        }
        __syncthreads();
        for (int y = 1 + threadIdx.x; y <= ph; y += kPreciseThreads) {
            unsigned run = 0u;
            for (int x = 1; x <= pw; ++x) run += sat[y * pitch + x], sat[y * pitch + x] = run;
        }
        __syncthreads();
        for (int x = 1 + threadIdx.x; x <= pw; x += kPreciseThreads) {
            unsigned run = 0u;
            for (int y = 1; y <= ph; ++y) run += sat[y * pitch + x], sat[y * pitch + x] = run;
        }
        __syncthreads();
    }
    // any pair left to the walk?  The table's first word becomes the flag once every lookup is done: the kernel has no static LDS (__syncthreads_or
    // would add some, and 160 KiB of dynamic LDS leave room for none)
    const bool left = precise_pairs<false>(a, r, reg, sat);
    __syncthreads();
    if (threadIdx.x == 0) sat[0] = 0u;
    __syncthreads();
    if (left) sat[0] = 1u; // every writer writes the same value
    __syncthreads();
    if (threadIdx.x == 0) a.walk[r] = (int)sat[0];
}

// The pairs replay_precise_kernel left, by the direct walk over the crop: a block per frame, which returns at once where the frame has none.
__global__ __launch_bounds__(kPreciseThreads) void replay_precise_walk_kernel(const PreciseArgs a) {
    if (a.stop && *a.stop) return; // block-uniform
    const long long r = blockIdx.x;
    if (!a.walk[r]) return; // block-uniform
    precise_pairs<true>(a, r, precise_region(a, r), nullptr);
}

// Per-experiment sums of the pairs' errors in the rows kernel's FIXED order: a block per (chunk of 4096 rows, experiment), thread t adds rows t, t + 256,
// ... of the chunk in order, a binary tree in LDS, the finish launch adds the chunk partials in index order.  NaN rows have no value and enter no sum
// (pandas' mean over the column).  Consecutive blocks are consecutive experiments of one chunk: their strided reads of `pair` [R][E] share cache lines.
__global__ __launch_bounds__(kRowThreads) void replay_precise_reduce_kernel(const PreciseArgs a) {
    __shared__ double red[kPreciseSummary][kRowThreads];
    if (a.stop && *a.stop) return; // block-uniform
    const Geometry g = a.g;
    const int s = blockIdx.x / a.E, e = blockIdx.x - s * a.E;
    double acc[kPreciseSummary];
    for (int q = 0; q < kPreciseSummary; ++q) acc[q] = 0.0;
    const long long r0 = (long long)s * kRowChunk;
    for (int i = 0; i < kRowChunk / kRowThreads; ++i) {
        const long long r = r0 + (long long)i * kRowThreads + threadIdx.x;
        if (r >= a.R) continue;
        const double err = a.pair[r * a.E + e];
        if (isnan(err)) {
            acc[5] += 1.0;
            continue;
        }
        const int c = (int)(r / g.L), step = (int)(r - (long long)c * g.L);
        acc[0] += err, acc[1] += 1.0;
        if (step < g.I && c != 0 && c != a.n_log - 1) acc[2] += err, acc[3] += 1.0; // DataAnalyzer.clean(trim_cycles=True, imaging_only=True)
        if (err > 1e-7) acc[4] += 1.0;
    }
    for (int q = 0; q < kPreciseSummary; ++q) red[q][threadIdx.x] = acc[q];
    __syncthreads();
    for (int half = kRowThreads / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half)
            for (int q = 0; q < kPreciseSummary; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x < kPreciseSummary) a.partial[((long long)e * a.S + s) * kPreciseSummary + threadIdx.x] = red[threadIdx.x][0];
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


// checks and argument structs of the two steps, apart from their launches: wtk_replay_objective refuses before anything is enqueued
int prepare_scan(const char *who, const wtk_replay_config *cfg, int32_t kind, int32_t E, int32_t n_cycles, const double *track_dev, int32_t n_track,
                 const double *a_dev, const double *b_dev, const int32_t *valid_dev, const double *share_dev, int32_t *pos_dev, int32_t *move_dev, ScanArgs &s) {
    const std::string w(who);
    int n_log = 0;
    if (replay_check_config(who, cfg, kind, E, n_cycles, n_track, s.g, n_log)) return 1;
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
    if (replay_check_config(who, cfg, WTK_REPLAY_OPTIMAL, E, n_cycles, n_track, r.g, n_log)) return 1;
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

void launch_finish(const FinishArgs &f, hipStream_t st) {
    hipLaunchKernelGGL(replay_finish_kernel, dim3((unsigned)(((long long)f.E * f.n + 63) / 64)), dim3(64), 0, st, f);
}

void launch_rows(const RowsArgs &r, hipStream_t st) {
    if (r.S > 0) hipLaunchKernelGGL(replay_rows_kernel, dim3((unsigned)((long long)r.S * r.E)), dim3(kRowThreads), 0, st, r);
    launch_finish(FinishArgs{r.partial, r.summary, r.E, r.S, kSummary, r.stop}, st);
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
    o.summary = summary_dev, o.objective = objective_dev, o.E = E, o.n = kSummary;
    hipStream_t st = (hipStream_t)stream;
    launch_scan(s, st);
    launch_rows(r, st);
    hipLaunchKernelGGL(replay_objective_kernel, dim3((unsigned)((E + 63) / 64)), dim3(64), 0, st, o);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- the precise error of a replayed population
namespace {

int prepare_precise(const char *who, const wtk_replay_config *cfg, int32_t E, int32_t n_cycles, const double *track_dev, int32_t n_track, const double *share_dev,
                    const int32_t *pos_dev, const int32_t *move_dev, const uint8_t *frames_dev, int32_t n_frames, int32_t H, int32_t W, const uint8_t *bg_dev,
                    double diff_thresh, int32_t max_crop_px, double *err_dev, int32_t *counts_dev, double *summary_dev, double *scratch_dev,
                    int64_t scratch_doubles, PreciseArgs &p) {
    const std::string w(who);
    int n_log = 0;
    if (replay_check_config(who, cfg, WTK_REPLAY_OPTIMAL, E, n_cycles, n_track, p.g, n_log)) return 1;
    if (!track_dev || !share_dev || !pos_dev || !move_dev || !frames_dev || !bg_dev || !summary_dev || !scratch_dev) return fail(w + ": null argument");
    if (H != cfg->frame_h || W != cfg->frame_w) return fail(w + ": the frames' (H, W) differ from the config's frame");
    if ((long long)H * W > (1ll << 30)) return fail(w + ": frames must be H x W gray with H * W <= 2^30");
    if (max_crop_px < 0) return fail(w + ": negative max_crop_px (0 = the default)");
    p.R = (long long)n_log * p.g.L;
    if (n_frames < p.R) return fail(w + ": fewer frames than logged rows (row r is frame r)");
    const long long S = (p.R + kRowChunk - 1) / kRowChunk;
    if (p.R > INT32_MAX || S * E > INT32_MAX) return fail(w + ": too many blocks for one launch");
    if (scratch_doubles < wtk_replay_precise_scratch_doubles(E, p.R)) return fail(w + ": scratch smaller than wtk_replay_precise_scratch_doubles(E, R)");
    p.E = E, p.C = n_cycles, p.S = (int)S, p.n_log = n_log;
    p.track = track_dev, p.share = share_dev, p.pos = pos_dev, p.move = move_dev, p.frames = frames_dev, p.bg = bg_dev;
    p.H = H, p.W = W, p.thr = threshold_int(diff_thresh);
    p.max_cells = max_crop_px == 0 ? kPreciseMaxCells : std::min((int)max_crop_px, kPreciseMaxCells);
    p.pair = scratch_dev, p.partial = scratch_dev + p.R * E, p.walk = reinterpret_cast<int *>(p.partial + (long long)E * S * kPreciseSummary), p.err = err_dev, p.counts = counts_dev, p.summary = summary_dev;
    return 0;
}

int launch_precise(const PreciseArgs &p, hipStream_t st) {
    if (p.R > 0) {
        // above 64 KiB of dynamic LDS a kernel needs the attribute (per device, so it is set at every call: a host-side table write)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&replay_precise_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kPreciseLdsBytes));
        hipLaunchKernelGGL(replay_precise_kernel, dim3((unsigned)p.R), dim3(kPreciseThreads), (size_t)p.max_cells * sizeof(unsigned), st, p);
        hipLaunchKernelGGL(replay_precise_walk_kernel, dim3((unsigned)p.R), dim3(kPreciseThreads), 0, st, p);
        hipLaunchKernelGGL(replay_precise_reduce_kernel, dim3((unsigned)((long long)p.S * p.E)), dim3(kRowThreads), 0, st, p);
    }
    launch_finish(FinishArgs{p.partial, p.summary, p.E, p.S, kPreciseSummary, p.stop}, st);
    return 0;
}

} // namespace

extern "C" int64_t wtk_replay_precise_scratch_doubles(int32_t E, int64_t R) {
    if (E < 0 || R < 0) return -1;
    return (int64_t)E * R + (int64_t)E * ((R + kRowChunk - 1) / kRowChunk) * kPreciseSummary + (R + 1) / 2; // pairs, chunk partials, [R] int32 walk flags
}

extern "C" int wtk_replay_precise(const wtk_replay_config *cfg, int32_t E, int32_t n_cycles, const double *track_dev, int32_t n_track,
                                  const double *share_dev, const int32_t *pos_dev, const int32_t *move_dev, const uint8_t *frames_dev, int32_t n_frames,
                                  int32_t H, int32_t W, const uint8_t *bg_dev, double diff_thresh, int32_t max_crop_px, double *err_dev,
                                  int32_t *counts_dev, double *summary_dev, double *scratch_dev, int64_t scratch_doubles, const int32_t *stop_dev,
                                  void *stream) {
    PreciseArgs p = {};
    if (prepare_precise("wtk_replay_precise", cfg, E, n_cycles, track_dev, n_track, share_dev, pos_dev, move_dev, frames_dev, n_frames, H, W, bg_dev,
                        diff_thresh, max_crop_px, err_dev, counts_dev, summary_dev, scratch_dev, scratch_doubles, p))
        return 1;
    p.stop = stop_dev;
    if (launch_precise(p, (hipStream_t)stream)) return 1;
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int wtk_replay_precise_objective(const wtk_replay_config *cfg, int32_t kind, int32_t E, int32_t n_cycles, const double *track_dev,
                                            int32_t n_track, const double *a_dev, const double *b_dev, const int32_t *valid_dev, const double *share_dev,
                                            int32_t *pos_dev, int32_t *move_dev, const uint8_t *frames_dev, int32_t n_frames, int32_t H, int32_t W,
                                            const uint8_t *bg_dev, double diff_thresh, int32_t max_crop_px, double *summary_dev, double *scratch_dev,
                                            int64_t scratch_doubles, int32_t objective, double *objective_dev, const int32_t *stop_dev, void *stream) {
    const char *who = "wtk_replay_precise_objective";
    ScanArgs s = {};
    PreciseArgs p = {};
    if (prepare_scan(who, cfg, kind, E, n_cycles, track_dev, n_track, a_dev, b_dev, valid_dev, share_dev, pos_dev, move_dev, s)) return 1;
    if (prepare_precise(who, cfg, E, n_cycles, track_dev, n_track, share_dev, pos_dev, move_dev, frames_dev, n_frames, H, W, bg_dev, diff_thresh, max_crop_px,
                        nullptr, nullptr, summary_dev, scratch_dev, scratch_doubles, p))
        return 1;
    if (!objective_dev) return fail(std::string(who) + ": null argument");
    ObjectiveArgs o = {};
    switch (objective) {
    case WTK_REPLAY_POBJ_TRIMMED_PRECISE: o.num = 2, o.den = 3; break;
    case WTK_REPLAY_POBJ_MEAN_PRECISE: o.num = 0, o.den = 1; break;
    case WTK_REPLAY_POBJ_NON_PERFECT: o.num = 4, o.den = 1; break;
    default: return fail(std::string(who) + ": unknown objective");
    }
    if (objective == WTK_REPLAY_POBJ_TRIMMED_PRECISE && p.n_log < 3)
        return fail(std::string(who) + ": the trimmed objective needs at least 3 logged cycles (the first and the last are dropped)");
    s.stop = p.stop = o.stop = stop_dev;
    o.summary = summary_dev, o.objective = objective_dev, o.E = E, o.n = kPreciseSummary;
    hipStream_t st = (hipStream_t)stream;
    launch_scan(s, st);
    if (launch_precise(p, st)) return 1;
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
    if (replay_check_config(who, cfg, WTK_REPLAY_OPTIMAL, 1, n_cycles, INT32_MAX, g, n_log)) return 1;
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
