// The precise error of a replayed population: the reference's analysis metric (ErrorCalculator.calculate_precise: the share of the
// worm's segmented pixels outside the microscope view) of every (experiment, logged frame) pair of a population replay.hip has scanned.  The segmented
// mask of frame r depends on the frame, the background and the track's row r only, so ONE workgroup per frame builds it once, as an exclusive
// summed-area table in LDS, and answers every experiment with two rectangle sums: O(F area + E F) pixel work, not O(E F area).  The per-frame statements
// are replay_precise_device.h's (precise_frame and its comment), which the kernels of a set of tracks (replay_set.hip) call as well.
// The per-experiment sums are taken in the rows kernel's FIXED order (replay_device.h: chunk_reduce, then replay.hip's finish launch), and the objective
// is replay.hip's division of two of their slots.  A nullable stop flag turns every launch into a no-op.
#include "wtk_internal.h"
#include "replay_precise_device.h"

#include <algorithm>

using namespace wtk;

namespace {

// the scratch of wtk_replay_precise, in doubles from its start: the pairs' errors [R][E] first (the Python layer reads them there), the chunk partials
// [E][S][kPreciseSummary], the [R] int32 walk flags
inline long long precise_off_partial(long long E, long long R) { return E * R; }
inline long long precise_off_walk(long long E, long long R) { return precise_off_partial(E, R) + E * chunk_count(R) * kPreciseSummary; }
inline long long precise_scratch(long long E, long long R) { return precise_off_walk(E, R) + (R + 1) / 2; }

// The precise error of every experiment at ONE logged frame r = blockIdx.x (row r is frame r): replay_precise_device.h's precise_frame.
__global__ __launch_bounds__(kPreciseThreads) void replay_precise_kernel(const PreciseArgs a) {
    extern __shared__ unsigned sat[];
    if (a.stop && *a.stop) return; // block-uniform
    precise_frame(a, blockIdx.x, sat);
}

// The pairs replay_precise_kernel left, by the direct walk over the crop: a block per frame, which returns at once where the frame has none.
__global__ __launch_bounds__(kPreciseThreads) void replay_precise_walk_kernel(const PreciseArgs a) {
    if (a.stop && *a.stop) return; // block-uniform
    precise_walk_frame(a, blockIdx.x);
}

// Per-experiment sums of the pairs' errors in the rows kernel's FIXED order: a block per (chunk of 4096 rows, experiment), thread t adds rows t, t + 256,
// ... of the chunk in order, a binary tree in LDS, the finish launch adds the chunk partials in index order.  NaN rows have no value and enter no sum
// (pandas' mean over the column).  Consecutive blocks are consecutive experiments of one chunk: their strided reads of `pair` [R][E] share cache lines.
__global__ __launch_bounds__(kRowThreads) void replay_precise_reduce_kernel(const PreciseArgs a) {
    __shared__ double red[kPreciseSummary][kRowThreads];
    if (a.stop && *a.stop) return; // block-uniform
    const ReplayView &v = a.v;
    const int s = blockIdx.x / v.E, e = blockIdx.x - s * v.E;
    double acc[kPreciseSummary];
    for (int q = 0; q < kPreciseSummary; ++q) acc[q] = 0.0;
    precise_chunk_rows(v, a.pair, e, (long long)s * kRowChunk, acc);
    chunk_reduce(red, acc, a.partial + ((long long)e * a.S + s) * kPreciseSummary);
}

int prepare_precise(const char *who, const wtk_replay_config *cfg, int32_t E, int32_t n_cycles, const double *track_dev, int32_t n_track, const double *share_dev,
                    const int32_t *pos_dev, const int32_t *move_dev, const uint8_t *frames_dev, int32_t n_frames, int32_t H, int32_t W, const uint8_t *bg_dev,
                    double diff_thresh, int32_t max_crop_px, double *err_dev, int32_t *counts_dev, double *summary_dev, double *scratch_dev,
                    int64_t scratch_doubles, PreciseArgs &p) {
    const std::string w(who);
    if (replay_view(who, cfg, WTK_REPLAY_OPTIMAL, E, n_cycles, track_dev, n_track, share_dev, pos_dev, move_dev, p.v)) return 1;
    if (!frames_dev || !bg_dev || !summary_dev || !scratch_dev) return fail(w + ": null argument");
    if (H != cfg->frame_h || W != cfg->frame_w) return fail(w + ": the frames' (H, W) differ from the config's frame");
    if ((long long)H * W > (1ll << 30)) return fail(w + ": frames must be H x W gray with H * W <= 2^30");
    if (max_crop_px < 0) return fail(w + ": negative max_crop_px (0 = the default)");
    const long long R = p.v.R;
    if (n_frames < R) return fail(w + ": fewer frames than logged rows (row r is frame r)");
    const long long S = chunk_count(R);
    if (R > INT32_MAX || S * E > INT32_MAX) return fail(w + ": too many blocks for one launch");
    if (scratch_doubles < precise_scratch(E, R)) return fail(w + ": scratch smaller than wtk_replay_precise_scratch_doubles(E, R)");
    p.S = (int)S, p.frames = frames_dev, p.bg = bg_dev;
    p.H = H, p.W = W, p.thr = threshold_int(diff_thresh);
    p.max_cells = precise_max_cells(max_crop_px);
    p.pair = scratch_dev, p.partial = scratch_dev + precise_off_partial(E, R), p.walk = reinterpret_cast<int *>(scratch_dev + precise_off_walk(E, R));
    p.err = err_dev, p.counts = counts_dev, p.summary = summary_dev, p.out_rows = R;
    return 0;
}

int launch_precise(const PreciseArgs &p, hipStream_t st) {
    if (p.v.R > 0) {
        // above 64 KiB of dynamic LDS a kernel needs the attribute (per device, so it is set at every call: a host-side table write)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&replay_precise_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kPreciseLdsBytes));
        hipLaunchKernelGGL(replay_precise_kernel, dim3((unsigned)p.v.R), dim3(kPreciseThreads), (size_t)p.max_cells * sizeof(unsigned), st, p);
        hipLaunchKernelGGL(replay_precise_walk_kernel, dim3((unsigned)p.v.R), dim3(kPreciseThreads), 0, st, p);
        hipLaunchKernelGGL(replay_precise_reduce_kernel, dim3((unsigned)((long long)p.S * p.v.E)), dim3(kRowThreads), 0, st, p);
    }
    launch_finish(p.partial, p.summary, p.v.E, p.S, kPreciseSummary, p.stop, st);
    return 0;
}

} // namespace

extern "C" int64_t wtk_replay_precise_scratch_doubles(int32_t E, int64_t R) {
    if (E < 0 || R < 0) return -1;
    return precise_scratch(E, R);
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
    s.stop = p.stop = stop_dev;
    hipStream_t st = (hipStream_t)stream;
    return enqueue_objective(who, kPreciseObjectives, (int)std::size(kPreciseObjectives), objective, summary_dev, kPreciseSummary, E, p.v.n_log, objective_dev,
                             stop_dev, st, [&] {
                                 launch_scan(s, st);
                                 return launch_precise(p, st);
                             });
}
