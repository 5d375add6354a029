// A population replayed on a SET of T tracks of different lengths in one call, with an objective pooled over the tracks.
//
// The tracks lie in one guarded "super-track" (include/wtk_hip.h states the layout): track t starts at cycle cyc_off of it, and every per-cycle array
// ([n_super / L][E]...) holds the track's cycles as one contiguous slice.  So a (track, experiment) pair is replay.hip's experiment on a VIEW: the
// super-track and the scan's arrays from the track's offset on, the track's own clamp, counts and init position.  Both kernels build that view and run
// replay_device.h's statements on it (scan_experiment; replay_row, row_accumulate, chunk_reduce), which is why a pair has wtk_replay_scan's and
// wtk_replay_rows' bits for any E, any T and any place in the set.
//   scan    one lane per (track, experiment), a block's lanes on one track, sequential over the track's cycles
//   rows    one block per (experiment, global chunk): the chunks of all tracks are numbered through (chunk0 = prefix sum of chunk_count(R_t)); the block
//           finds its track by a search in that table and reduces the chunk's rows as replay_rows_kernel does
//   finish  per (experiment, slot): each track's chunk partials in index order -> track_summary[t][e]; those in track order from 0.0 -> summary[e]; the
//           one float64 division of the pooled slots (and, where asked for, of each track's)
// Three launches whatever T is.  No floating-point atomics.  Every launch reads the nullable stop flag and touches nothing once it is up.
//
// Recordings at different scales: the *_geom entry points take a per-track geometry table (camera and microscope sizes; the
// analysis also reads its unit factors), which replay_set_device.h's track_geometry puts into the track's view in the place of cfg's sizes.  The
// kernels, the launches and the order of every sum are the same; the entry points without the suffix pass no table.
//
// The PRECISE error of the set, each track with its own frames, background, frame shape and threshold (the frames table):
//   table   one block per GLOBAL logged row (row0 = prefix sum of R): the block finds its track by a search in the frames table, fills a PreciseArgs
//           for that track alone and runs replay_precise_device.h's precise_frame on the track's row, as replay_precise_kernel does
//   walk    the same lookup, precise_walk_frame
//   reduce  one block per (experiment, global chunk), replay_precise_reduce_kernel's lane order and tree on the rows of the chunk's track
//   finish  the finish launch above on the precise partials (both summaries are 6 wide) with the precise objective's slots
// After the scan that is five launches whatever T is, and the frames of all tracks fill the device together.
#include "wtk_internal.h"
#include "replay_precise_device.h"
#include "replay_set_device.h"

#include <algorithm>

using namespace wtk;

namespace {

constexpr int kScanThreads = 64;
constexpr int kFinishExperiments = 8; // per block of the finish launch: 8 experiments x 8 lanes, of which kSummary add

__global__ __launch_bounds__(kScanThreads) void replay_set_scan_kernel(const SetArgs a) {
    if (a.stop && *a.stop) return;
    const int t = blockIdx.y, e = blockIdx.x * kScanThreads + threadIdx.x; // the track is block-uniform: its view stays in scalar registers, as replay_scan_kernel's
    if (e >= a.E) return;
    const wtk_replay_set_track tr = a.tracks[t];
    const long long c0 = (long long)tr.cyc_off * a.E; // the track's slice of the cycle-major arrays
    ScanArgs s;
    s.g = track_geometry(a, t, tr), s.kind = a.kind, s.E = a.E, s.C = tr.n_cycles, s.init_x = tr.init_x, s.init_y = tr.init_y;
    s.track = a.track + 4 * (long long)tr.cyc_off * a.g.L, s.n_track = tr.n_track;
    s.a = a.a ? a.a + 2 * c0 : nullptr, s.b = a.b ? a.b + 2 * c0 : nullptr, s.valid = a.valid ? a.valid + c0 : nullptr;
    s.share = a.share, s.pos = a.pos + 2 * c0, s.move = a.move + 2 * c0, s.stop = nullptr;
    scan_experiment(s, e);
}

__global__ __launch_bounds__(kRowThreads) void replay_set_rows_kernel(const SetArgs a) {
    __shared__ double red[kSummary][kRowThreads];
    if (a.stop && *a.stop) return; // block-uniform
    const int e = blockIdx.x / a.S, gs = blockIdx.x - e * a.S;
    int lo = 0, hi = a.T - 1; // the last track whose first chunk is <= gs (a track without rows has no chunk and is never found)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.tracks[mid].chunk0 <= gs) lo = mid;
        else hi = mid - 1;
    }
    const wtk_replay_set_track tr = a.tracks[lo];
    const ReplayView v = track_view(a, lo, tr);
    double acc[kSummary];
    for (int q = 0; q < kSummary; ++q) acc[q] = 0.0;
    const long long r0 = (long long)(gs - tr.chunk0) * kRowChunk;
    for (int i = 0; i < kRowChunk / kRowThreads; ++i) {
        const long long r = r0 + (long long)i * kRowThreads + threadIdx.x;
        if (r >= v.R) continue;
        double err, mse;
        row_accumulate(v, replay_row(v, e, r), acc, err, mse);
    }
    chunk_reduce(red, acc, a.partial + ((long long)e * a.S + gs) * kSummary);
}

__global__ __launch_bounds__(kFinishExperiments * 8) void replay_set_finish_kernel(const SetArgs a) {
    __shared__ double of_track[kFinishExperiments][8];
    if (a.stop && *a.stop) return; // block-uniform
    const int el = threadIdx.x >> 3, q = threadIdx.x & 7;
    const int e = blockIdx.x * kFinishExperiments + el;
    const bool adds = e < a.E && q < kSummary;
    double pooled = 0.0;
    for (int t = 0; t < a.T; ++t) { // (T is block-uniform: so are the barriers)
        double sum = 0.0;
        if (adds) {
            const int s0 = a.tracks[t].chunk0, s1 = t + 1 < a.T ? a.tracks[t + 1].chunk0 : a.S;
            for (int s = s0; s < s1; ++s) sum += a.partial[((long long)e * a.S + s) * kSummary + q];
            a.track_summary[((long long)t * a.E + e) * kSummary + q] = sum;
            pooled += sum;
        }
        if (a.track_objective) {
            of_track[el][q] = sum;
            __syncthreads();
            if (q == 0 && e < a.E) a.track_objective[(long long)t * a.E + e] = of_track[el][a.num] / of_track[el][a.den];
            __syncthreads();
        }
    }
    if (adds) a.summary[(long long)e * kSummary + q] = pooled;
    if (a.objective) {
        of_track[el][q] = pooled;
        __syncthreads();
        // the float64 division Summary's properties perform on the host (counts are exact doubles); 0 / 0 = NaN, which the swarm never lets win
        if (q == 0 && e < a.E) a.objective[e] = of_track[el][a.num] / of_track[el][a.den];
    }
}

// ---- the precise error of the set
struct SetPreciseArgs {
    SetArgs s;                           // the view of the scanned set; partial, the summaries and the objective are the PRECISE ones
    const wtk_replay_set_frames *frames; // [T] on the device
    long long rows;                      // logged rows of all tracks
    int max_cells;
    double *pair; // [rows][E]: track t's [R_t][E] block starts at row0_t E
    int *walk;    // [rows]
    double *err;  // [E][rows] (nullable)
    int *counts;  // [E][rows][2] (nullable)
};

// the last track whose first global row is <= rho (a track without rows shares its row0 with the next one and is never found); block-uniform, so the
// search and the view built from it stay in scalar registers, as replay_set_rows_kernel's search on chunk0
__device__ __forceinline__ int track_of_row(const SetPreciseArgs &a, long long rho) {
    int lo = 0, hi = a.s.T - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.frames[mid].row0 <= rho) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// track t of the set as replay_precise_kernel's arguments: the track's view, frames and threshold; the output bases at the track's first global row
__device__ __forceinline__ PreciseArgs track_precise(const SetPreciseArgs &a, int t) {
    const wtk_replay_set_frames fr = a.frames[t];
    PreciseArgs p;
    p.v = track_view(a.s, t, a.s.tracks[t]);
    p.frames = fr.frames, p.bg = fr.bg, p.H = fr.H, p.W = fr.W, p.thr = threshold_int(fr.diff_thresh);
    p.max_cells = a.max_cells, p.S = 0, p.out_rows = a.rows;
    p.pair = a.pair + fr.row0 * a.s.E, p.walk = a.walk + fr.row0;
    p.err = a.err ? a.err + fr.row0 : nullptr, p.counts = a.counts ? a.counts + 2 * fr.row0 : nullptr;
    p.partial = nullptr, p.summary = nullptr, p.stop = nullptr;
    return p;
}

__global__ __launch_bounds__(kPreciseThreads) void replay_set_precise_kernel(const SetPreciseArgs a) {
    extern __shared__ unsigned sat[];
    if (a.s.stop && *a.s.stop) return; // block-uniform
    const long long rho = blockIdx.x;
    const int t = track_of_row(a, rho);
    precise_frame(track_precise(a, t), rho - a.frames[t].row0, sat);
}

__global__ __launch_bounds__(kPreciseThreads) void replay_set_precise_walk_kernel(const SetPreciseArgs a) {
    if (a.s.stop && *a.s.stop) return; // block-uniform
    const long long rho = blockIdx.x;
    if (!a.walk[rho]) return; // block-uniform
    const int t = track_of_row(a, rho);
    precise_walk_frame(track_precise(a, t), rho - a.frames[t].row0);
}

// Consecutive blocks are consecutive experiments of one chunk, as replay_precise_reduce_kernel's.
__global__ __launch_bounds__(kRowThreads) void replay_set_precise_reduce_kernel(const SetPreciseArgs a) {
    __shared__ double red[kPreciseSummary][kRowThreads];
    if (a.s.stop && *a.s.stop) return; // block-uniform
    const int gs = blockIdx.x / a.s.E, e = blockIdx.x - gs * a.s.E;
    int lo = 0, hi = a.s.T - 1; // the last track whose first chunk is <= gs, as replay_set_rows_kernel
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.s.tracks[mid].chunk0 <= gs) lo = mid;
        else hi = mid - 1;
    }
    const wtk_replay_set_track tr = a.s.tracks[lo];
    const ReplayView v = track_view(a.s, lo, tr); // the track's own n_log: its first and last logged cycle are trimmed
    double acc[kPreciseSummary];
    for (int q = 0; q < kPreciseSummary; ++q) acc[q] = 0.0;
    precise_chunk_rows(v, a.pair + a.frames[lo].row0 * a.s.E, e, (long long)(gs - tr.chunk0) * kRowChunk, acc);
    chunk_reduce(red, acc, a.s.partial + ((long long)e * a.s.S + gs) * kPreciseSummary);
}
static_assert((int)kPreciseSummary == (int)kSummary, "replay_set_finish_kernel adds the precise partials too");

int set_targets(const char *who, int32_t kind, const double *a_dev, const double *b_dev, const int32_t *valid_dev, SetArgs &a) {
    const std::string w(who);
    if (kind != WTK_REPLAY_CSV && (!a_dev || !valid_dev)) return fail(w + ": null targets");
    if (kind == WTK_REPLAY_MLP && !b_dev) return fail(w + ": null origins (b_dev) for the MLP kind");
    a.a = a_dev, a.b = b_dev, a.valid = valid_dev;
    return 0;
}

int set_sums(const char *who, const wtk_replay_set_track *host, int32_t T, double *track_summary_dev, double *summary_dev, double *scratch_dev, int64_t scratch_doubles,
             SetArgs &a) {
    const std::string w(who);
    if (!track_summary_dev || !summary_dev || !scratch_dev) return fail(w + ": null argument");
    if (scratch_doubles < wtk_replay_set_scratch_doubles(host, T, a.g.L, a.E)) return fail(w + ": scratch smaller than wtk_replay_set_scratch_doubles(tracks_host, T, L, E)");
    a.track_summary = track_summary_dev, a.summary = summary_dev, a.partial = scratch_dev;
    return 0;
}

void launch_set_scan(const SetArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(replay_set_scan_kernel, dim3((unsigned)((a.E + kScanThreads - 1) / kScanThreads), (unsigned)a.T), dim3(kScanThreads), 0, st, a);
}

void launch_set_finish(const SetArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(replay_set_finish_kernel, dim3((unsigned)((a.E + kFinishExperiments - 1) / kFinishExperiments)), dim3(kFinishExperiments * 8), 0, st, a);
}

void launch_set_rows(const SetArgs &a, hipStream_t st) {
    if (a.S > 0) hipLaunchKernelGGL(replay_set_rows_kernel, dim3((unsigned)((long long)a.S * a.E)), dim3(kRowThreads), 0, st, a);
    launch_set_finish(a, st);
}

// the scratch of wtk_replay_set_precise in doubles from its start: the pairs' errors [rows][E], the chunk partials [E][S][6], the [rows] int32 walk flags
inline long long set_precise_off_partial(long long E, long long rows) { return E * rows; }
inline long long set_precise_off_walk(long long E, long long rows, long long S) { return set_precise_off_partial(E, rows) + E * S * kPreciseSummary; }
inline long long set_precise_scratch(long long E, long long rows, long long S) { return set_precise_off_walk(E, rows, S) + (rows + 1) / 2; }

// The checks of the frames table against the track table set_view has accepted (each reported with the track's index), and the precise outputs.
int set_frames(const char *who, const wtk_replay_set_track *host, const wtk_replay_set_frames *frames_host, const wtk_replay_set_frames *frames_dev, int32_t T,
               int32_t max_crop_px, double *err_dev, int32_t *counts_dev, double *track_summary_dev, double *summary_dev, double *scratch_dev,
               int64_t scratch_doubles, SetPreciseArgs &p) {
    const std::string w(who);
    if (!frames_host || !frames_dev || !track_summary_dev || !summary_dev || !scratch_dev) return fail(w + ": null argument");
    long long rows = 0;
    for (int t = 0; t < T; ++t) {
        const wtk_replay_set_frames &fr = frames_host[t];
        const std::string wt = w + ": track " + std::to_string(t);
        if (!fr.frames || !fr.bg) return fail(wt + ": null frames or background");
        if (fr.H != host[t].y_max + 1 || fr.W != host[t].x_max + 1) return fail(wt + ": the frames' (H, W) differ from the track's frame (y_max + 1, x_max + 1)");
        if ((long long)fr.H * fr.W > (1ll << 30)) return fail(wt + ": frames must be H x W gray with H * W <= 2^30");
        if (fr.n_frames < host[t].R) return fail(wt + ": fewer frames than logged rows (row r is frame r)");
        if (!std::isfinite(fr.diff_thresh)) return fail(wt + ": diff_thresh must be finite");
        if (fr.row0 != rows) return fail(wt + ": row0 must be the sum of R over the tracks before it");
        rows += host[t].R;
    }
    if (max_crop_px < 0) return fail(w + ": negative max_crop_px (0 = the default)");
    const long long E = p.s.E, S = p.s.S;
    if (rows > INT32_MAX || S * E > INT32_MAX) return fail(w + ": too many blocks for one launch");
    if (scratch_doubles < set_precise_scratch(E, rows, S))
        return fail(w + ": scratch smaller than wtk_replay_set_precise_scratch_doubles(tracks_host, T, L, E)");
    p.frames = frames_dev, p.rows = rows, p.max_cells = precise_max_cells(max_crop_px);
    p.pair = scratch_dev, p.s.partial = scratch_dev + set_precise_off_partial(E, rows);
    p.walk = reinterpret_cast<int *>(scratch_dev + set_precise_off_walk(E, rows, S));
    p.err = err_dev, p.counts = counts_dev, p.s.track_summary = track_summary_dev, p.s.summary = summary_dev;
    return 0;
}

int launch_set_precise(const SetPreciseArgs &p, hipStream_t st) {
    if (p.rows > 0) {
        // above 64 KiB of dynamic LDS a kernel needs the attribute (per device, so it is set at every call: a host-side table write)
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&replay_set_precise_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kPreciseLdsBytes));
        hipLaunchKernelGGL(replay_set_precise_kernel, dim3((unsigned)p.rows), dim3(kPreciseThreads), (size_t)p.max_cells * sizeof(unsigned), st, p);
        hipLaunchKernelGGL(replay_set_precise_walk_kernel, dim3((unsigned)p.rows), dim3(kPreciseThreads), 0, st, p);
        hipLaunchKernelGGL(replay_set_precise_reduce_kernel, dim3((unsigned)((long long)p.s.S * p.s.E)), dim3(kRowThreads), 0, st, p);
    }
    launch_set_finish(p.s, st);
    return 0;
}

} // namespace

// (declared in replay_set_device.h: replay_set_analysis.hip checks its table with it too)
int wtk::set_view(const char *who, const wtk_replay_config *cfg, const wtk_replay_set_track *host, const wtk_replay_set_track *dev,
                  const wtk_replay_set_geometry *geom_host, const wtk_replay_set_geometry *geom_dev, int32_t T, int32_t guard_cycles, int32_t kind, int32_t E,
                  const double *track_dev, int32_t n_super, const double *share_dev, const int32_t *pos_dev, const int32_t *move_dev, SetArgs &a,
                  int &min_log) {
    const std::string w(who);
    if (!cfg || !host || !dev) return fail(w + ": null argument");
    if (T < 1) return fail(w + ": at least one track (T >= 1)");
    if (guard_cycles < 0) return fail(w + ": negative guard_cycles");
    if ((geom_host == nullptr) != (geom_dev == nullptr)) return fail(w + ": the geometry table needs its host and its device copy (or neither)");
    long long chunks = 0, end_before = 0; // end_before: the first cycle behind the slot and guard of the track before
    min_log = INT32_MAX;
    for (int t = 0; t < T; ++t) {
        const wtk_replay_set_track &tr = host[t];
        const std::string wt = w + ": track " + std::to_string(t);
        wtk_replay_config c = *cfg;
        c.num_frames = tr.num_frames, c.frame_w = tr.x_max < INT32_MAX ? tr.x_max + 1 : 0, c.frame_h = tr.y_max < INT32_MAX ? tr.y_max + 1 : 0;
        c.init_x = tr.init_x, c.init_y = tr.init_y;
        if (geom_host) c.cam_w = geom_host[t].cam_w, c.cam_h = geom_host[t].cam_h, c.mic_w = geom_host[t].mic_w, c.mic_h = geom_host[t].mic_h;
        ReplayView v = {};
        if (replay_view(wt.c_str(), &c, kind, E, tr.n_cycles, track_dev, tr.n_track, share_dev, pos_dev, move_dev, v)) return 1;
        if (tr.n_log != v.n_log || tr.R != v.R) return fail(wt + ": n_log and R must be (num_frames - 1) / L and n_log L");
        if (tr.init_x < 0 || tr.init_x > tr.x_max || tr.init_y < 0 || tr.init_y > tr.y_max) return fail(wt + ": the init position must be clamped to the frame");
        if (tr.chunk0 != chunks) return fail(wt + ": chunk0 must be the sum of the chunk counts of the tracks before it");
        if (tr.cyc_off < end_before) return fail(wt + ": its slot overlaps the slot or the guard of the track before it (or cyc_off is negative)");
        const long long L = v.g.L, slot = std::max<long long>(tr.n_cycles, (tr.n_track + L - 1) / L);
        end_before = tr.cyc_off + slot + guard_cycles;
        if (n_super < 0 || n_super % L != 0 || end_before * L > n_super) return fail(wt + ": its slot and guard end beyond the super-track (n_super must be a multiple of L)");
        chunks += chunk_count(v.R);
        min_log = std::min(min_log, v.n_log);
        a.g = v.g;
    }
    if (chunks * E > INT32_MAX) return fail(w + ": too many (experiment, chunk) blocks for one launch");
    if (T > 65535) return fail(w + ": at most 65535 tracks (the scan's grid)");
    a.tracks = dev, a.geom = geom_dev, a.T = T, a.E = E, a.kind = kind, a.S = (int)chunks, a.track = track_dev, a.share = share_dev;
    a.pos = const_cast<int *>(pos_dev), a.move = const_cast<int *>(move_dev);
    return 0;
}

extern "C" int wtk_replay_set_scan_geom(const wtk_replay_config *cfg, const wtk_replay_set_track *tracks_host, const wtk_replay_set_track *tracks_dev,
                                        const wtk_replay_set_geometry *geom_host, const wtk_replay_set_geometry *geom_dev, int32_t T, int32_t guard_cycles,
                                        int32_t kind, int32_t E, const double *track_dev, int32_t n_super, const double *a_dev, const double *b_dev,
                                        const int32_t *valid_dev, const double *share_dev, int32_t *pos_dev, int32_t *move_dev, const int32_t *stop_dev,
                                        void *stream) {
    const char *who = geom_host || geom_dev ? "wtk_replay_set_scan_geom" : "wtk_replay_set_scan";
    SetArgs a = {};
    int min_log = 0;
    if (set_view(who, cfg, tracks_host, tracks_dev, geom_host, geom_dev, T, guard_cycles, kind, E, track_dev, n_super, share_dev, pos_dev, move_dev, a,
                 min_log))
        return 1;
    if (set_targets(who, kind, a_dev, b_dev, valid_dev, a)) return 1;
    a.stop = stop_dev;
    launch_set_scan(a, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int64_t wtk_replay_set_scratch_doubles(const wtk_replay_set_track *tracks_host, int32_t T, int32_t cycle_frame_num, int32_t E) {
    if (!tracks_host || T < 1 || cycle_frame_num < 1 || E < 0) return -1;
    int64_t chunks = 0;
    for (int t = 0; t < T; ++t) {
        if (tracks_host[t].n_log < 0) return -1;
        chunks += chunk_count((long long)tracks_host[t].n_log * cycle_frame_num);
    }
    return (int64_t)E * chunks * kSummary;
}

extern "C" int wtk_replay_set_rows_geom(const wtk_replay_config *cfg, const wtk_replay_set_track *tracks_host, const wtk_replay_set_track *tracks_dev,
                                        const wtk_replay_set_geometry *geom_host, const wtk_replay_set_geometry *geom_dev, int32_t T, int32_t guard_cycles,
                                        int32_t E, const double *track_dev, int32_t n_super, const double *share_dev, const int32_t *pos_dev,
                                        const int32_t *move_dev, double *track_summary_dev, double *summary_dev, double *scratch_dev,
                                        int64_t scratch_doubles, const int32_t *stop_dev, void *stream) {
    const char *who = geom_host || geom_dev ? "wtk_replay_set_rows_geom" : "wtk_replay_set_rows";
    SetArgs a = {};
    int min_log = 0;
    if (set_view(who, cfg, tracks_host, tracks_dev, geom_host, geom_dev, T, guard_cycles, WTK_REPLAY_OPTIMAL, E, track_dev, n_super, share_dev, pos_dev, move_dev, a,
                 min_log))
        return 1;
    if (set_sums(who, tracks_host, T, track_summary_dev, summary_dev, scratch_dev, scratch_doubles, a)) return 1;
    a.stop = stop_dev;
    launch_set_rows(a, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int wtk_replay_set_objective_geom(const wtk_replay_config *cfg, const wtk_replay_set_track *tracks_host, const wtk_replay_set_track *tracks_dev,
                                             const wtk_replay_set_geometry *geom_host, const wtk_replay_set_geometry *geom_dev, int32_t T,
                                             int32_t guard_cycles, int32_t kind, int32_t E, const double *track_dev, int32_t n_super, const double *a_dev,
                                             const double *b_dev, const int32_t *valid_dev, const double *share_dev, int32_t *pos_dev, int32_t *move_dev,
                                             double *track_summary_dev, double *summary_dev, double *scratch_dev, int64_t scratch_doubles,
                                             int32_t objective, double *objective_dev, double *track_objective_dev, const int32_t *stop_dev,
                                             void *stream) {
    const char *who = geom_host || geom_dev ? "wtk_replay_set_objective_geom" : "wtk_replay_set_objective";
    const std::string w(who);
    SetArgs a = {};
    int min_log = 0;
    if (set_view(who, cfg, tracks_host, tracks_dev, geom_host, geom_dev, T, guard_cycles, kind, E, track_dev, n_super, share_dev, pos_dev, move_dev, a,
                 min_log))
        return 1;
    if (set_targets(who, kind, a_dev, b_dev, valid_dev, a)) return 1;
    if (set_sums(who, tracks_host, T, track_summary_dev, summary_dev, scratch_dev, scratch_doubles, a)) return 1;
    if (!objective_dev) return fail(w + ": null argument");
    const ObjectiveRule *rule = std::find_if(std::begin(kRowsObjectives), std::end(kRowsObjectives), [&](const ObjectiveRule &r) { return r.id == objective; });
    if (rule == std::end(kRowsObjectives)) return fail(w + ": unknown objective");
    if (rule->needs_3_cycles && min_log < 3)
        return fail(w + ": the trimmed objective needs at least 3 logged cycles of every track (the first and the last of each are dropped)");
    a.objective = objective_dev, a.track_objective = track_objective_dev, a.num = rule->num, a.den = rule->den, a.stop = stop_dev;
    hipStream_t st = (hipStream_t)stream;
    launch_set_scan(a, st);
    launch_set_rows(a, st);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int64_t wtk_replay_set_precise_scratch_doubles(const wtk_replay_set_track *tracks_host, int32_t T, int32_t cycle_frame_num, int32_t E) {
    if (!tracks_host || T < 1 || cycle_frame_num < 1 || E < 0) return -1;
    int64_t chunks = 0, rows = 0;
    for (int t = 0; t < T; ++t) {
        if (tracks_host[t].n_log < 0) return -1;
        const long long R = (long long)tracks_host[t].n_log * cycle_frame_num;
        chunks += chunk_count(R), rows += R;
    }
    return set_precise_scratch(E, rows, chunks);
}

extern "C" int wtk_replay_set_precise_geom(const wtk_replay_config *cfg, const wtk_replay_set_track *tracks_host, const wtk_replay_set_track *tracks_dev,
                                           const wtk_replay_set_geometry *geom_host, const wtk_replay_set_geometry *geom_dev,
                                           const wtk_replay_set_frames *frames_host, const wtk_replay_set_frames *frames_dev, int32_t T,
                                           int32_t guard_cycles, int32_t E, const double *track_dev, int32_t n_super, const double *share_dev,
                                           const int32_t *pos_dev, const int32_t *move_dev, int32_t max_crop_px, double *err_dev, int32_t *counts_dev,
                                           double *track_summary_dev, double *summary_dev, double *scratch_dev, int64_t scratch_doubles,
                                           const int32_t *stop_dev, void *stream) {
    const char *who = geom_host || geom_dev ? "wtk_replay_set_precise_geom" : "wtk_replay_set_precise";
    SetPreciseArgs p = {};
    int min_log = 0;
    if (set_view(who, cfg, tracks_host, tracks_dev, geom_host, geom_dev, T, guard_cycles, WTK_REPLAY_OPTIMAL, E, track_dev, n_super, share_dev, pos_dev, move_dev, p.s,
                 min_log))
        return 1;
    if (set_frames(who, tracks_host, frames_host, frames_dev, T, max_crop_px, err_dev, counts_dev, track_summary_dev, summary_dev, scratch_dev, scratch_doubles, p))
        return 1;
    p.s.stop = stop_dev;
    if (launch_set_precise(p, (hipStream_t)stream)) return 1;
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int wtk_replay_set_precise_objective_geom(const wtk_replay_config *cfg, const wtk_replay_set_track *tracks_host,
                                                     const wtk_replay_set_track *tracks_dev, const wtk_replay_set_geometry *geom_host,
                                                     const wtk_replay_set_geometry *geom_dev, const wtk_replay_set_frames *frames_host,
                                                     const wtk_replay_set_frames *frames_dev, int32_t T, int32_t guard_cycles, int32_t kind, int32_t E,
                                                     const double *track_dev, int32_t n_super, const double *a_dev, const double *b_dev,
                                                     const int32_t *valid_dev, const double *share_dev, int32_t *pos_dev, int32_t *move_dev,
                                                     int32_t max_crop_px, double *track_summary_dev, double *summary_dev, double *scratch_dev,
                                                     int64_t scratch_doubles, int32_t objective, double *objective_dev, double *track_objective_dev,
                                                     const int32_t *stop_dev, void *stream) {
    const char *who = geom_host || geom_dev ? "wtk_replay_set_precise_objective_geom" : "wtk_replay_set_precise_objective";
    const std::string w(who);
    SetPreciseArgs p = {};
    int min_log = 0;
    if (set_view(who, cfg, tracks_host, tracks_dev, geom_host, geom_dev, T, guard_cycles, kind, E, track_dev, n_super, share_dev, pos_dev, move_dev, p.s,
                 min_log))
        return 1;
    if (set_targets(who, kind, a_dev, b_dev, valid_dev, p.s)) return 1;
    if (set_frames(who, tracks_host, frames_host, frames_dev, T, max_crop_px, nullptr, nullptr, track_summary_dev, summary_dev, scratch_dev, scratch_doubles, p))
        return 1;
    if (!objective_dev) return fail(w + ": null argument");
    const ObjectiveRule *rule = std::find_if(std::begin(kPreciseObjectives), std::end(kPreciseObjectives), [&](const ObjectiveRule &r) { return r.id == objective; });
    if (rule == std::end(kPreciseObjectives)) return fail(w + ": unknown objective");
    if (rule->needs_3_cycles && min_log < 3)
        return fail(w + ": the trimmed objective needs at least 3 logged cycles of every track (the first and the last of each are dropped)");
    p.s.objective = objective_dev, p.s.track_objective = track_objective_dev, p.s.num = rule->num, p.s.den = rule->den, p.s.stop = stop_dev;
    hipStream_t st = (hipStream_t)stream;
    launch_set_scan(p.s, st);
    if (launch_set_precise(p, st)) return 1;
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- the entry points without a geometry table: cfg's camera and microscope for every track
extern "C" int wtk_replay_set_scan(const wtk_replay_config *cfg, const wtk_replay_set_track *tracks_host, const wtk_replay_set_track *tracks_dev, int32_t T,
                                   int32_t guard_cycles, int32_t kind, int32_t E, const double *track_dev, int32_t n_super, const double *a_dev,
                                   const double *b_dev, const int32_t *valid_dev, const double *share_dev, int32_t *pos_dev, int32_t *move_dev,
                                   const int32_t *stop_dev, void *stream) {
    return wtk_replay_set_scan_geom(cfg, tracks_host, tracks_dev, nullptr, nullptr, T, guard_cycles, kind, E, track_dev, n_super, a_dev, b_dev, valid_dev, share_dev,
                                    pos_dev, move_dev, stop_dev, stream);
}

extern "C" int wtk_replay_set_rows(const wtk_replay_config *cfg, const wtk_replay_set_track *tracks_host, const wtk_replay_set_track *tracks_dev, int32_t T,
                                   int32_t guard_cycles, int32_t E, const double *track_dev, int32_t n_super, const double *share_dev,
                                   const int32_t *pos_dev, const int32_t *move_dev, double *track_summary_dev, double *summary_dev, double *scratch_dev,
                                   int64_t scratch_doubles, const int32_t *stop_dev, void *stream) {
    return wtk_replay_set_rows_geom(cfg, tracks_host, tracks_dev, nullptr, nullptr, T, guard_cycles, E, track_dev, n_super, share_dev, pos_dev, move_dev,
                                    track_summary_dev, summary_dev, scratch_dev, scratch_doubles, stop_dev, stream);
}

extern "C" int wtk_replay_set_objective(const wtk_replay_config *cfg, const wtk_replay_set_track *tracks_host, const wtk_replay_set_track *tracks_dev,
                                        int32_t T, int32_t guard_cycles, int32_t kind, int32_t E, const double *track_dev, int32_t n_super,
                                        const double *a_dev, const double *b_dev, const int32_t *valid_dev, const double *share_dev, int32_t *pos_dev,
                                        int32_t *move_dev, double *track_summary_dev, double *summary_dev, double *scratch_dev, int64_t scratch_doubles,
                                        int32_t objective, double *objective_dev, double *track_objective_dev, const int32_t *stop_dev, void *stream) {
    return wtk_replay_set_objective_geom(cfg, tracks_host, tracks_dev, nullptr, nullptr, T, guard_cycles, kind, E, track_dev, n_super, a_dev, b_dev, valid_dev,
                                         share_dev, pos_dev, move_dev, track_summary_dev, summary_dev, scratch_dev, scratch_doubles, objective, objective_dev,
                                         track_objective_dev, stop_dev, stream);
}

extern "C" int wtk_replay_set_precise(const wtk_replay_config *cfg, const wtk_replay_set_track *tracks_host, const wtk_replay_set_track *tracks_dev,
                                      const wtk_replay_set_frames *frames_host, const wtk_replay_set_frames *frames_dev, int32_t T, int32_t guard_cycles,
                                      int32_t E, const double *track_dev, int32_t n_super, const double *share_dev, const int32_t *pos_dev,
                                      const int32_t *move_dev, int32_t max_crop_px, double *err_dev, int32_t *counts_dev, double *track_summary_dev,
                                      double *summary_dev, double *scratch_dev, int64_t scratch_doubles, const int32_t *stop_dev, void *stream) {
    return wtk_replay_set_precise_geom(cfg, tracks_host, tracks_dev, nullptr, nullptr, frames_host, frames_dev, T, guard_cycles, E, track_dev, n_super, share_dev,
                                       pos_dev, move_dev, max_crop_px, err_dev, counts_dev, track_summary_dev, summary_dev, scratch_dev, scratch_doubles, stop_dev,
                                       stream);
}

extern "C" int wtk_replay_set_precise_objective(const wtk_replay_config *cfg, const wtk_replay_set_track *tracks_host, const wtk_replay_set_track *tracks_dev,
                                                const wtk_replay_set_frames *frames_host, const wtk_replay_set_frames *frames_dev, int32_t T,
                                                int32_t guard_cycles, int32_t kind, int32_t E, const double *track_dev, int32_t n_super, const double *a_dev,
                                                const double *b_dev, const int32_t *valid_dev, const double *share_dev, int32_t *pos_dev, int32_t *move_dev,
                                                int32_t max_crop_px, double *track_summary_dev, double *summary_dev, double *scratch_dev,
                                                int64_t scratch_doubles, int32_t objective, double *objective_dev, double *track_objective_dev,
                                                const int32_t *stop_dev, void *stream) {
    return wtk_replay_set_precise_objective_geom(cfg, tracks_host, tracks_dev, nullptr, nullptr, frames_host, frames_dev, T, guard_cycles, kind, E, track_dev,
                                                 n_super, a_dev, b_dev, valid_dev, share_dev, pos_dev, move_dev, max_crop_px, track_summary_dev, summary_dev,
                                                 scratch_dev, scratch_doubles, objective, objective_dev, track_objective_dev, stop_dev, stream);
}
