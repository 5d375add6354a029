// The precise error's per-frame statements (DESIGN.md sections 19 and 27), shared by replay_precise.hip (one track) and replay_set.hip (a set of tracks):
// the padded region of a frame, its summed-area table in LDS, the experiments' rectangle sums and their exact fallback, the whole body of a table block
// and of a walk block, and the lane-serial row loop of the reduction.  A kernel fills a PreciseArgs for ONE track (the set's kernels per block, from
// their tables, with the output bases moved to the track's first row) and calls these, which is why a (track, experiment) pair has the same bits alone
// and in any set.  Also the host side both files share: the objectives over the summary's slots.
#pragma once
#include "eval_device.h"
#include "replay_device.h"

namespace wtk {

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
    long long out_rows;    // rows of an experiment in err / counts: R, or the rows of all tracks of a set (the bases then point at this track's first row)
    double *pair;          // [R][E] the error of every pair, NaN = no value
    int *walk;             // [R] != 0: the frame has pairs the table did not answer (the walk kernel)
    double *err;           // [E][out_rows] (nullable)
    int *counts;           // [E][out_rows][2] (total, inside) (nullable)
    double *partial;       // [E][S][kPreciseSummary]
    double *summary;       // [E][kPreciseSummary]
    const int *stop;
};

inline constexpr ObjectiveRule kPreciseObjectives[] = {
    {WTK_REPLAY_POBJ_TRIMMED_PRECISE, kPreciseTrimmedErr, kPreciseTrimmedCount, true},
    {WTK_REPLAY_POBJ_MEAN_PRECISE, kPreciseErr, kPreciseCount, false},
    {WTK_REPLAY_POBJ_NON_PERFECT, kPreciseNonPerfect, kPreciseCount, false},
};

// the table limit of a call: max_crop_px = 0 and everything above the LDS mean the default
inline int precise_max_cells(int32_t max_crop_px) { return max_crop_px == 0 ? kPreciseMaxCells : (max_crop_px < kPreciseMaxCells ? (int)max_crop_px : kPreciseMaxCells); }

// sum of the exclusive summed-area table over [l, r) x [t, b) in table coordinates; uint32 arithmetic wraps and the result is exact
__device__ __forceinline__ int sat_rect(const unsigned *sat, int pitch, int l, int t, int r, int b) {
    return (int)(sat[b * pitch + r] - sat[t * pitch + r] - sat[b * pitch + l] + sat[t * pitch + l]);
}

// The precise error of every experiment at ONE logged frame r (row r is frame r): precise_frame is the body of a table block.
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
// every pair of a frame whose table does not fit `max_cells` is left to the walk kernel (precise_walk_frame), which the table block tells through walk[r]
// whether frame r has such a pair.  That kernel asks for no LDS, so its waves fill the CUs; here a block that holds 160 KiB would walk with 4 waves per CU
// (measured: 4 x slower than the per-row kernel).  It walks the crop with crop_walk, precise_error_kernel's loop: the lanes that need it are collected
// with a ballot and the whole wave walks them one after the other.  Both ways count the same pixels, so the limit never changes a bit.
//
// Occupancy: at the default limit a workgroup asks for all 160 KiB of LDS, so one workgroup (4 waves) runs per CU, 256 frames at a time on the device; a
// handful of frames leaves most CUs idle, and nothing hides the latency of phase 1's dependent LDS passes.  The frames of a set's
// tracks are blocks of ONE launch.
struct PreciseRegion {
    int pl, pt, pr, pb; // the padded region of the frame, empty where the track's row is illegal
    int pitch;          // of its table, in words
    bool table;         // the table fits max_cells: the table block builds it
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
            if (a.err) a.err[(long long)e * a.out_rows + r] = err;
            if (a.counts) a.counts[2 * ((long long)e * a.out_rows + r)] = total, a.counts[2 * ((long long)e * a.out_rows + r) + 1] = inside;
        }
    }
    return left;
}

// The body of a table block for frame r of the track `a` describes: phase 1 into `sat` (the block's dynamic LDS, a.max_cells words), phase 2, walk[r].
// Every thread of the block must call it; r and a are block-uniform.
__device__ __forceinline__ void precise_frame(const PreciseArgs &a, long long r, unsigned *sat) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint8_t *fr = a.frames + r * a.H * a.W;
    const PreciseRegion reg = precise_region(a, r);
    const int pl = reg.pl, pt = reg.pt, pw = reg.pr - reg.pl, ph = reg.pb - reg.pt, pitch = reg.pitch;
    if (reg.table) { // block-uniform
        // The fill reads through pointers TYPED as global.  A set's kernel reads them from its frames table, and such a pointer is generic to the
        // compiler: the loads became flat loads and the loop was not unrolled (10 % of the set's time at one track).  A kernel argument is known
        // to be global anyway: replay_precise_kernel's code does not change.
        const __attribute__((address_space(1))) uint8_t *gfr = (const __attribute__((address_space(1))) uint8_t *)fr;
        const __attribute__((address_space(1))) uint8_t *gbg = (const __attribute__((address_space(1))) uint8_t *)a.bg;
        for (int x = threadIdx.x; x <= pw; x += kPreciseThreads) sat[x] = 0u;
        for (int y = 1 + threadIdx.x; y <= ph; y += kPreciseThreads) sat[y * pitch] = 0u;
        for (int y = wave; y < ph; y += kPreciseThreads / 64) {
            const long long o = (long long)(pt + y) * a.W + pl;
            for (int x = lane; x < pw; x += 64) sat[(y + 1) * pitch + x + 1] = abs((int)gfr[o + x] - (int)gbg[o + x]) > a.thr ? 1u : 0u;
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

// The body of a walk block for frame r: the pairs the table block left, by the direct walk over the crop; returns at once where the frame has none.
__device__ __forceinline__ void precise_walk_frame(const PreciseArgs &a, long long r) {
    if (!a.walk[r]) return; // block-uniform
    precise_pairs<true>(a, r, precise_region(a, r), nullptr);
}

// What thread t of a reducing block adds of the chunk that starts at row r0 of the view: rows r0 + t, r0 + t + 256, ... of experiment e in order, from
// pair [R][E].  NaN rows have no value and enter no sum (pandas' mean over the column).  chunk_reduce follows.
__device__ __forceinline__ void precise_chunk_rows(const ReplayView &v, const double *pair, int e, long long r0, double (&acc)[kPreciseSummary]) {
    for (int i = 0; i < kRowChunk / kRowThreads; ++i) {
        const long long r = r0 + (long long)i * kRowThreads + threadIdx.x;
        if (r >= v.R) continue;
        const double err = pair[r * v.E + e];
        if (isnan(err)) {
            acc[kPreciseNan] += 1.0;
            continue;
        }
        acc[kPreciseErr] += err, acc[kPreciseCount] += 1.0;
        if (row_trimmed(v, row_cycle(v.g, r))) acc[kPreciseTrimmedErr] += err, acc[kPreciseTrimmedCount] += 1.0;
        if (non_perfect(err)) acc[kPreciseNonPerfect] += 1.0;
    }
}

} // namespace wtk
