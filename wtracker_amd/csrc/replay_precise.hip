// The precise error of a replayed population: the reference's analysis metric (ErrorCalculator.calculate_precise: the share of the
// worm's segmented pixels outside the microscope view) of every (experiment, logged frame) pair of a population replay.hip has scanned.  The segmented
// mask of frame r depends on the frame, the background and the track's row r only, so ONE workgroup per frame builds it once, as an exclusive
// summed-area table in LDS, and answers every experiment with two rectangle sums: O(F area + E F) pixel work, not O(E F area).  See replay_precise_kernel.
// The per-experiment sums are taken in the rows kernel's FIXED order (replay_device.h: chunk_reduce, then replay.hip's finish launch), and the objective
// is replay.hip's division of two of their slots.  A nullable stop flag turns every launch into a no-op.
#include "wtk_internal.h"
#include "eval_device.h"
#include "replay_device.h"

#include <algorithm>

using namespace wtk;

namespace {

constexpr int kPreciseThreads = 256;
constexpr int kPreciseLdsBytes = 160 * 1024;            // the CU's LDS: one workgroup per CU takes all of it at the default limit
constexpr int kPreciseMaxCells = kPreciseLdsBytes / 4;  // uint32 cells of the largest table

struct PreciseArgs {
    ReplayView v;
    const uint8_t *frames; // [n_frames][H][W] gray, row r is frame r
    const uint8_t *bg;     // [H][W]
    int H, W, thr;         // a pixel is foreground where |frame - bg| > thr
    int max_cells;         // a frame whose table needs more uint32 cells walks its crops instead
    int S;                 // chunks of the R rows: the reduce kernel's blocks per experiment
    double *pair;          // [R][E] the error of every pair, NaN = no value
    int *walk;             // [R] != 0: the frame has pairs the table did not answer (replay_precise_walk_kernel)
    double *err;           // [E][R] (nullable)
    int *counts;           // [E][R][2] (total, inside) (nullable)
    double *partial;       // [E][S][kPreciseSummary]
    double *summary;       // [E][kPreciseSummary]
    const int *stop;
};

// the scratch of wtk_replay_precise, in doubles from its start: the pairs' errors [R][E] first (the Python layer reads them there), the chunk partials
// [E][S][kPreciseSummary], the [R] int32 walk flags
inline long long precise_off_partial(long long E, long long R) { return E * R; }
inline long long precise_off_walk(long long E, long long R) { return precise_off_partial(E, R) + E * chunk_count(R) * kPreciseSummary; }
inline long long precise_scratch(long long E, long long R) { return precise_off_walk(E, R) + (R + 1) / 2; }

constexpr ObjectiveRule kPreciseObjectives[] = {
    {WTK_REPLAY_POBJ_TRIMMED_PRECISE, kPreciseTrimmedErr, kPreciseTrimmedCount, true},
    {WTK_REPLAY_POBJ_MEAN_PRECISE, kPreciseErr, kPreciseCount, false},
    {WTK_REPLAY_POBJ_NON_PERFECT, kPreciseNonPerfect, kPreciseCount, false},
};

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
// Phase 2.  Threads stride over the experiments: platform position of (e, r) and the row's boxes (replay_row), both discretised, then
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
    const bool track_legal = discretize(a.v.track + 4 * r, a.H, a.W, g.pl, g.pt, g.pr, g.pb);
    if (track_legal) g.pl = max(g.pl - 1, 0), g.pt = max(g.pt - 1, 0), g.pr = min(g.pr + 1, a.W), g.pb = min(g.pb + 1, a.H);
    g.pitch = (g.pr - g.pl + 1) | 1;
    g.table = track_legal && (long long)(g.pb - g.pt + 1) * g.pitch <= a.max_cells;
    return g;
}

// Phase 2 over the experiments of frame r.  kWalk = false: the pairs the table answers and the pairs without a value; returns whether a pair of this
// thread is left to the walk.  kWalk = true: exactly those pairs, by the walk (`sat` is not read).  Every thread of the block must call it.
template <bool kWalk> __device__ __forceinline__ bool precise_pairs(const PreciseArgs &a, long long r, const PreciseRegion &reg, const unsigned *sat) {
    const ReplayView &v = a.v;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint8_t *fr = a.frames + r * a.H * a.W;
    const RowCycle at = row_cycle(v.g, r);
    bool left = false;
    for (int e0 = wave * 64; e0 < v.E; e0 += kPreciseThreads) { // wave-uniform trip count: the ballot below sees the whole wave
        const int e = e0 + lane;
        int wl = 0, wt = 0, wr = 0, wb = 0, il = 0, it = 0, ir = 0, ib = 0, total = 0, inside = 0;
        bool legal = false, walk = false;
        if (e < v.E) {
            int ml, mt, mr, mb;
            const RowBoxes b = replay_row(v, e, r, at).b;
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
        if (e < v.E && walk == kWalk) {
            const double err = legal ? precise_error_of(total, inside) : __builtin_nan("");
            a.pair[r * v.E + e] = err;
            if (a.err) a.err[(long long)e * v.R + r] = err;
            if (a.counts) a.counts[2 * ((long long)e * v.R + r)] = total, a.counts[2 * ((long long)e * v.R + r) + 1] = inside;
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
    const ReplayView &v = a.v;
    const int s = blockIdx.x / v.E, e = blockIdx.x - s * v.E;
    double acc[kPreciseSummary];
    for (int q = 0; q < kPreciseSummary; ++q) acc[q] = 0.0;
    const long long r0 = (long long)s * kRowChunk;
    for (int i = 0; i < kRowChunk / kRowThreads; ++i) {
        const long long r = r0 + (long long)i * kRowThreads + threadIdx.x;
        if (r >= v.R) continue;
        const double err = a.pair[r * v.E + e];
        if (isnan(err)) {
            acc[kPreciseNan] += 1.0;
            continue;
        }
        acc[kPreciseErr] += err, acc[kPreciseCount] += 1.0;
        if (row_trimmed(v, row_cycle(v.g, r))) acc[kPreciseTrimmedErr] += err, acc[kPreciseTrimmedCount] += 1.0;
        if (non_perfect(err)) acc[kPreciseNonPerfect] += 1.0;
    }
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
    p.max_cells = max_crop_px == 0 ? kPreciseMaxCells : std::min((int)max_crop_px, kPreciseMaxCells);
    p.pair = scratch_dev, p.partial = scratch_dev + precise_off_partial(E, R), p.walk = reinterpret_cast<int *>(scratch_dev + precise_off_walk(E, R));
    p.err = err_dev, p.counts = counts_dev, p.summary = summary_dev;
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
