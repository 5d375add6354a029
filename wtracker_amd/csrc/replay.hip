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
//   objective  scan + rows (no row, per-row or slot output) + one division per experiment: the swarm's objective without a host round trip.
// A nullable stop flag (the swarm's ctrl word) turns the targets, the objective and, through them only, the scan and the rows reduction into no-ops.
// Everything relies on -ffp-contract=off (the library's build flag): share * move + carry is a rounded product and a rounded sum, as in Python.
//
// The rest of the closed loop, each over replay_device.h (the population's view, the motor, the row, the chunk reduction):
//   replay_set.hip       the same scan and rows reduction of a population on a SET of tracks in one call, with a pooled objective
//   replay_targets.hip   the per-cycle Polyfit targets of a whole population of weight vectors, in the layout the scan reads
//   replay_yolo.hip      the YOLO controller's loop, whose targets depend on the camera view: the control kernels between the detector's calls
//   replay_precise.hip   the precise error (segmented pixels outside the microscope view) of every (experiment, logged frame) pair, and its objective
//   replay_analysis.hip  DataAnalyzer's statistics of a replayed population
#include "wtk_internal.h"
#include "replay_device.h"

#include <algorithm>

using namespace wtk;

namespace {

constexpr int kScanThreads = 64;
constexpr int kRowDoubles = WTK_REPLAY_ROW_DOUBLES;

struct RowsArgs {
    ReplayView v;
    int S, n_slots;
    const int *row_slot;   // [E] slot of the experiment in `rows`, or -1 (nullable)
    double *rows;          // [slots][R][kRowDoubles] (nullable)
    double *bbox_err, *mse_err; // [E][R] (nullable)
    double *partial;       // [E][S][kSummary]
    double *summary;       // [E][kSummary]
    const int *stop;       // nullable, as ScanArgs::stop
};

struct ObjectiveArgs {
    const double *summary; // [E][n]
    double *objective;     // [E]
    int E, n, num, den;    // objective = summary[num] / summary[den]
    const int *stop;
};

__global__ __launch_bounds__(kScanThreads) void replay_scan_kernel(const ScanArgs a) {
    if (a.stop && *a.stop) return;
    const int e = blockIdx.x * kScanThreads + threadIdx.x;
    if (e >= a.E) return;
    scan_experiment(a, e);
}

__global__ __launch_bounds__(kRowThreads) void replay_rows_kernel(const RowsArgs a) {
    __shared__ double red[kSummary][kRowThreads];
    if (a.stop && *a.stop) return; // block-uniform
    const ReplayView &v = a.v;
    const int e = blockIdx.x / a.S, s = blockIdx.x - e * a.S;
    int slot = a.row_slot ? a.row_slot[e] : -1;
    if (slot >= a.n_slots) slot = -1; // never write past `rows`
    double acc[kSummary];
    for (int q = 0; q < kSummary; ++q) acc[q] = 0.0;
    const long long r0 = (long long)s * kRowChunk;
    for (int i = 0; i < kRowChunk / kRowThreads; ++i) {
        const long long r = r0 + (long long)i * kRowThreads + threadIdx.x;
        if (r >= v.R) continue;
        const ReplayRow w = replay_row(v, e, r);
        const RowBoxes &b = w.b;
        double err, mse;
        row_accumulate(v, w, acc, err, mse);
        if (a.bbox_err) a.bbox_err[(long long)e * v.R + r] = err;
        if (a.mse_err) a.mse_err[(long long)e * v.R + r] = mse;
        if (slot >= 0 && a.rows) {
            double *o = a.rows + ((long long)slot * v.R + r) * kRowDoubles;
            o[0] = (double)w.px, o[1] = (double)w.py;
            o[2] = b.cam_x, o[3] = b.cam_y, o[4] = (double)v.g.cam_w, o[5] = (double)v.g.cam_h;
            o[6] = b.mic_x, o[7] = b.mic_y, o[8] = b.mic_w, o[9] = b.mic_h;
            o[10] = b.wx, o[11] = b.wy, o[12] = b.ww, o[13] = b.wh;
            o[14] = (double)w.at.c, o[15] = w.at.step < v.g.I ? 0.0 : 1.0; // imaging / moving
        }
    }
    chunk_reduce(red, acc, a.partial + ((long long)e * a.S + s) * kSummary);
}

// the chunk partials of every experiment added in index order (the rows reduction and the precise reduction)
__global__ __launch_bounds__(64) void replay_finish_kernel(const double *partial, double *summary, int E, int S, int n, const int *stop) {
    if (stop && *stop) return;
    const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
    if (i >= (long long)E * n) return;
    const long long e = i / n;
    const int q = (int)(i - e * n);
    double sum = 0.0;
    for (int s = 0; s < S; ++s) sum += partial[(e * S + s) * n + q];
    summary[i] = sum;
}

__global__ __launch_bounds__(64) void replay_objective_kernel(const ObjectiveArgs a) {
    if (a.stop && *a.stop) return;
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= a.E) return;
    // the float64 division Summary's properties perform on the host (counts are exact doubles); 0 / 0 = NaN, which the swarm never lets win
    a.objective[e] = a.summary[(long long)e * a.n + a.num] / a.summary[(long long)e * a.n + a.den];
}

// checks and argument struct of the rows step, apart from its launch: wtk_replay_objective refuses before anything is enqueued
int prepare_rows(const char *who, const wtk_replay_config *cfg, int32_t E, int32_t n_cycles, const double *track_dev, int32_t n_track, const double *share_dev,
                 const int32_t *pos_dev, const int32_t *move_dev, const int32_t *row_slot_dev, int32_t n_slots, double *rows_dev, double *bbox_err_dev,
                 double *mse_err_dev, double *summary_dev, double *scratch_dev, int64_t scratch_doubles, RowsArgs &r) {
    const std::string w(who);
    if (replay_view(who, cfg, WTK_REPLAY_OPTIMAL, E, n_cycles, track_dev, n_track, share_dev, pos_dev, move_dev, r.v)) return 1;
    if (!summary_dev || !scratch_dev) return fail(w + ": null argument");
    if ((row_slot_dev == nullptr) != (rows_dev == nullptr) || n_slots < 0 || (rows_dev && n_slots < 1))
        return fail(w + ": row_slot_dev, rows_dev and n_slots >= 1 go together");
    const long long S = chunk_count(r.v.R);
    if (S * E > INT32_MAX) return fail(w + ": too many (experiment, chunk) blocks for one launch");
    if (scratch_doubles < wtk_replay_scratch_doubles(E, r.v.R)) return fail(w + ": scratch smaller than wtk_replay_scratch_doubles(E, R)");
    r.S = (int)S, r.n_slots = rows_dev ? n_slots : 0;
    r.row_slot = row_slot_dev, r.rows = rows_dev;
    r.bbox_err = bbox_err_dev, r.mse_err = mse_err_dev, r.partial = scratch_dev, r.summary = summary_dev;
    return 0;
}

void launch_rows(const RowsArgs &r, hipStream_t st) {
    if (r.S > 0) hipLaunchKernelGGL(replay_rows_kernel, dim3((unsigned)((long long)r.S * r.v.E)), dim3(kRowThreads), 0, st, r);
    launch_finish(r.partial, r.summary, r.v.E, r.S, kSummary, r.stop, st);
}

} // namespace

namespace wtk {

int prepare_scan(const char *who, const wtk_replay_config *cfg, int32_t kind, int32_t E, int32_t n_cycles, const double *track_dev, int32_t n_track,
                 const double *a_dev, const double *b_dev, const int32_t *valid_dev, const double *share_dev, int32_t *pos_dev, int32_t *move_dev, ScanArgs &s) {
    const std::string w(who);
    ReplayView v = {};
    if (replay_view(who, cfg, kind, E, n_cycles, track_dev, n_track, share_dev, pos_dev, move_dev, v)) return 1;
    if (kind != WTK_REPLAY_CSV && (!a_dev || !valid_dev)) return fail(w + ": null targets");
    if (kind == WTK_REPLAY_MLP && !b_dev) return fail(w + ": null origins (b_dev) for the MLP kind");
    s.g = v.g, s.kind = kind, s.E = E, s.C = n_cycles, s.init_x = cfg->init_x, s.init_y = cfg->init_y;
    s.track = track_dev, s.n_track = n_track, s.a = a_dev, s.b = b_dev, s.valid = valid_dev, s.share = share_dev, s.pos = pos_dev, s.move = move_dev;
    return 0;
}

void launch_scan(const ScanArgs &s, hipStream_t st) {
    hipLaunchKernelGGL(replay_scan_kernel, dim3((unsigned)((s.E + kScanThreads - 1) / kScanThreads)), dim3(kScanThreads), 0, st, s);
}

void launch_finish(const double *partial, double *summary, int E, int S, int n, const int *stop, hipStream_t st) {
    hipLaunchKernelGGL(replay_finish_kernel, dim3((unsigned)(((long long)E * n + 63) / 64)), dim3(64), 0, st, partial, summary, E, S, n, stop);
}

int enqueue_objective(const char *who, const ObjectiveRule *rules, int n_rules, int32_t objective, const double *summary_dev, int width, int32_t E, int n_log,
                      double *objective_dev, const int32_t *stop_dev, hipStream_t st, const std::function<int()> &produce) {
    const std::string w(who);
    if (!objective_dev) return fail(w + ": null argument");
    const ObjectiveRule *rule = std::find_if(rules, rules + n_rules, [&](const ObjectiveRule &r) { return r.id == objective; });
    if (rule == rules + n_rules) return fail(w + ": unknown objective");
    if (rule->needs_3_cycles && n_log < 3) return fail(w + ": the trimmed objective needs at least 3 logged cycles (the first and the last are dropped)");
    if (produce()) return 1;
    hipLaunchKernelGGL(replay_objective_kernel, dim3((unsigned)((E + 63) / 64)), dim3(64), 0, st, ObjectiveArgs{summary_dev, objective_dev, E, width, rule->num, rule->den, stop_dev});
    HIP_TRY(hipGetLastError());
    return 0;
}

} // namespace wtk

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
    return (int64_t)E * chunk_count(R) * kSummary;
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
    const char *who = "wtk_replay_objective";
    ScanArgs s = {};
    RowsArgs r = {};
    if (prepare_scan(who, cfg, kind, E, n_cycles, track_dev, n_track, a_dev, b_dev, valid_dev, share_dev, pos_dev, move_dev, s)) return 1;
    if (prepare_rows(who, cfg, E, n_cycles, track_dev, n_track, share_dev, pos_dev, move_dev, nullptr, 0, nullptr, nullptr, nullptr, summary_dev, scratch_dev,
                     scratch_doubles, r))
        return 1;
    s.stop = r.stop = stop_dev;
    hipStream_t st = (hipStream_t)stream;
    return enqueue_objective(who, kRowsObjectives, (int)std::size(kRowsObjectives), objective, summary_dev, kSummary, E, r.v.n_log, objective_dev, stop_dev, st, [&] {
        launch_scan(s, st);
        launch_rows(r, st);
        return 0;
    });
}
