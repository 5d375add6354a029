// Background-subtraction worm boxes on the device: BoxCalculator._calc_bounding_box (wtracker/dataset/box_calculator.py:75-101) for gray frames, in
// exact integer arithmetic.
//
// Mask stage (boxes_mask_kernel): one block per band of kBandRows image rows and kOutWords 32-pixel words of one selected frame.  A wave owns one row at a
// time and a lane one word of it: the lane reads its 32 frame bytes and 32 background bytes as dwords (funnel-shifted where the row does not start on a
// dword; bytes one at a time where the dword window would leave the buffer), thresholds them into one word, and the wave ANDs the word with its two
// horizontal neighbours' bits (5-wide erosion, carries by lane shuffle).  The band with 2 + 7 halo rows on each side then sits in LDS as bit rows: the
// vertical 5-row AND, the 15-wide OR (shuffles again) and the vertical 15-row OR follow on words.  Out-of-image pixels never erode (they are ones under the
// AND) and never dilate (zeros under the OR).  Only the final bit mask is written: H x ceil(W / 32) words per frame.  Lanes 0 and 63 of a row are halo words:
// their outer bits are wrong, and nothing reads those (a word's result needs 9 bits of each neighbour).
// Contour stage (boxes_trace_kernel): a wave walks a strip of mask rows, a lane one word column, and finds the candidates -- set pixels whose W, NW, N and NE
// neighbours are clear -- with bit operations on the row and the row above it (kept in registers).  The lane traces the outer border from each of its
// candidates (Moore neighbourhood, clockwise from the backtrack pixel, closed when the start pixel is about to be left by its first move again),
// summing the shoelace terms as integers, and gives up as soon as it meets a pixel that precedes the start in raster order: such a start is a local top of a
// component, not its first pixel.  The kept traces are one per 8-connected component; each does one 64-bit atomicMax of (A2, start index) on the frame's
// key, so the winner does not depend on the order the atomics land in.  boxes_finish_kernel retraces the winner for its extent, one thread per frame.
// Every trace is bounded by 8 H W steps (a trace visits a (pixel, backtrack direction) pair once): past it the frame is reported as a fault.
#include "wtk_internal.h"

#include <algorithm>
#include <climits>

using namespace wtk;

namespace {

constexpr int kMaskThreads = 256;
constexpr int kBandRows = 64;                    // output rows of a block
constexpr int kErodeR = 2, kDilateR = 7;         // 5 x 5 erosion, 15 x 15 dilation
constexpr int kHalo = kErodeR + kDilateR;
constexpr int kOutWords = 62;                    // output words of a block: a wave's 64 lanes less one halo word on each side
constexpr int kRowsA = kBandRows + 2 * kHalo;    // thresholded, horizontally eroded rows
constexpr int kRowsB = kBandRows + 2 * kDilateR; // eroded, horizontally dilated rows
constexpr int kTraceThreads = 256;
constexpr int kStripRows = 32;                   // mask rows a wave walks for candidates
constexpr int kRootBits = 30;                    // H W <= 2^30
constexpr unsigned long long kKeyFault = ~0ull;

typedef unsigned long long u64;
typedef unsigned u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

struct BoxArgs {
    const uint8_t *frames; // [n_frames][H][W]
    int n_frames, H, W;
    const uint8_t *bg;     // [H][W]
    const int *frame_idx;  // [n_sel] or null
    int n_sel, thr;
    int wpr;               // words per mask row
    int bands, ctiles;     // mask stage: bands of rows and tiles of words per frame
    int strips, wtiles;    // contour stage: strips of rows and tiles of 64 words per frame
    u64 *keys;             // [n_sel] 0: no foreground; kKeyFault; else ((A2 << 30) | start index) + 1 of the best component so far
    unsigned *mask;        // [n_sel][H][wpr]
    int *boxes;            // [n_sel][4], nullable
    long long *area2;      // [n_sel], nullable
    uint8_t *mask_out;     // [n_sel][H][W], nullable
    int *faults;
};

__device__ __forceinline__ long long selected_frame(const BoxArgs &a, int s) {
    const long long f = a.frame_idx ? a.frame_idx[s] : s;
    return (f < 0 || f >= a.n_frames) ? -1 : f;
}

// 32 bytes at p as 8 dwords (byte j of the run in bits 8 (j % 4) of v[j / 4]); only the first nvalid bytes matter.  [lo, hi) is the buffer p lies in: the
// dword path reads the 36 bytes from p rounded down to a dword, and is taken only where they are all inside it.
__device__ __forceinline__ void load32(const uint8_t *p, const uint8_t *lo, const uint8_t *hi, int nvalid, unsigned (&v)[8]) {
    const unsigned m = (unsigned)((uintptr_t)p & 3u);
    const uint8_t *q = p - m;
    if (q >= lo && q + 36 <= hi) {
        const u32x4_a4 d0 = *reinterpret_cast<const u32x4_a4 *>(q), d1 = *reinterpret_cast<const u32x4_a4 *>(q + 16);
        const unsigned d[9] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w, *reinterpret_cast<const unsigned *>(q + 32)};
        const unsigned sh = 8u * m;
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = (unsigned)((((u64)d[i + 1] << 32) | d[i]) >> sh);
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            unsigned w = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (4 * i + j < nvalid) w |= (unsigned)p[4 * i + j] << (8 * j);
            v[i] = w;
        }
    }
}

// bit j = |f_j - b_j| > thr
__device__ __forceinline__ unsigned thresh32(const unsigned (&f)[8], const unsigned (&b)[8], unsigned thr) {
    unsigned w = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned mk = 0xffu << (8 * j);
            const unsigned d = __builtin_amdgcn_sad_u8(f[i] & mk, b[i] & mk, 0u); // the other three bytes are zero on both sides
            w |= (d > thr ? 1u : 0u) << (4 * i + j);
        }
    return w;
}

// a row word with its neighbours' words: the AND (kAnd) or OR of the pixels within kR of each pixel.  `fill`: the neighbour a wave's end lane lacks.
template <bool kAnd, int kR> __device__ __forceinline__ unsigned horizontal(unsigned t, int lane, unsigned fill) {
    unsigned l = __shfl_up(t, 1), r = __shfl_down(t, 1);
    if (lane == 0) l = fill;
    if (lane == 63) r = fill;
    u64 x = ((u64)t << 32) | l; // pixel i - k of the row: bit 32 + i of x << k
    u64 z = ((u64)r << 32) | t; // pixel i + k: bit i of z >> k
    if (kAnd) {
#pragma unroll
        for (int k = 1; k <= kR; ++k) x &= x << 1, z &= z >> 1; // after k steps: AND of k + 1 neighbours
        return (unsigned)(x >> 32) & (unsigned)z;
    }
    static_assert(kAnd || kR == 7, "the OR doubles its reach: 1, 3, 7");
    x |= x << 1, x |= x << 2, x |= x << 4;
    z |= z >> 1, z |= z >> 2, z |= z >> 4;
    return (unsigned)(x >> 32) | (unsigned)z;
}

__global__ __launch_bounds__(kMaskThreads) void boxes_mask_kernel(const BoxArgs a) {
    __shared__ unsigned rows_a[kRowsA][64];
    __shared__ unsigned rows_b[kRowsB][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long blk = blockIdx.x;
    const int ct = (int)(blk % a.ctiles);
    blk /= a.ctiles;
    const int band = (int)(blk % a.bands), s = (int)(blk / a.bands);
    const long long f = selected_frame(a, s);
    if (f < 0) return; // the whole block
    const long long c = (long long)ct * kOutWords - 1 + lane; // the lane's word of the row
    const int r0 = band * kBandRows;
    int nvalid = 0;
    if (c >= 0 && c < a.wpr) nvalid = (int)min(32ll, (long long)a.W - 32 * c);
    const unsigned valid = nvalid == 32 ? ~0u : (1u << nvalid) - 1u;
    const long long hw = (long long)a.H * a.W;
    const uint8_t *fr = a.frames + f * hw, *fr_hi = a.frames + (long long)a.n_frames * hw, *bg_hi = a.bg + hw;

    for (int r = wave; r < kRowsA; r += kMaskThreads / 64) {
        const int y = r0 - kHalo + r;
        unsigned t = ~0u; // out of the image: never erodes
        if (y >= 0 && y < a.H && nvalid > 0) {
            const long long off = (long long)y * a.W + 32 * c;
            unsigned fv[8], bv[8];
            load32(fr + off, a.frames, fr_hi, nvalid, fv);
            load32(a.bg + off, a.bg, bg_hi, nvalid, bv);
            t = thresh32(fv, bv, (unsigned)a.thr) | ~valid;
        }
        rows_a[r][lane] = horizontal<true, kErodeR>(t, lane, ~0u);
    }
    __syncthreads();
    for (int r = wave; r < kRowsB; r += kMaskThreads / 64) { // image row r0 - kDilateR + r: rows_a[r .. r + 4] are its 5 rows
        const int y = r0 - kDilateR + r;
        unsigned e = rows_a[r][lane];
#pragma unroll
        for (int k = 1; k <= 2 * kErodeR; ++k) e &= rows_a[r + k][lane];
        e = (y >= 0 && y < a.H) ? e & valid : 0u; // out of the image: never dilates
        rows_b[r][lane] = horizontal<false, kDilateR>(e, lane, 0u);
    }
    __syncthreads();
    for (int r = wave; r < kBandRows; r += kMaskThreads / 64) { // image row r0 + r: rows_b[r .. r + 14]
        const int y = r0 + r;
        if (y >= a.H) break;
        unsigned d = rows_b[r][lane];
#pragma unroll
        for (int k = 1; k <= 2 * kDilateR; ++k) d |= rows_b[r + k][lane];
        if (lane >= 1 && lane <= kOutWords && nvalid > 0) a.mask[((long long)s * a.H + y) * a.wpr + c] = d & valid;
    }
}

// the eight neighbours clockwise on the screen (y down) from east: E SE S SW W NW N NE, as dx + 1 and dy + 1 in two bits each
constexpr unsigned kDx = 2u | 2u << 2 | 1u << 4 | 0u << 6 | 0u << 8 | 0u << 10 | 1u << 12 | 2u << 14;
constexpr unsigned kDy = 1u | 2u << 2 | 2u << 4 | 2u << 6 | 1u << 8 | 0u << 10 | 0u << 12 | 0u << 14;

__device__ __forceinline__ bool mask_px(const unsigned *m, int wpr, int W, int H, int x, int y) {
    if ((unsigned)x >= (unsigned)W || (unsigned)y >= (unsigned)H) return false;
    return (m[(long long)y * wpr + (x >> 5)] >> (x & 31)) & 1u;
}

enum TraceResult { TRACE_KEPT = 0, TRACE_NOT_FIRST = 1, TRACE_BOUND = 2 };

// Border trace from (sx, sy), a set pixel whose W neighbour is clear.  kExtent: ext = (min x, min y, max x, max y) of the border, and the raster-order
// test is left out (the start is known to be a component's first pixel).
template <bool kExtent>
__device__ TraceResult trace_border(const unsigned *m, int wpr, int W, int H, int sx, int sy, long long max_steps, long long &a2, int *ext) {
    int x = sx, y = sy, b = 4, d0 = -1; // b: direction of the backtrack pixel (clear) seen from (x, y)
    long long sum = 0;
    const long long start = (long long)sy * W + sx;
    if (kExtent) ext[0] = ext[2] = sx, ext[1] = ext[3] = sy;
    for (long long step = 0; step <= max_steps; ++step) {
        int d = -1, nx = 0, ny = 0;
        for (int k = 1; k <= 8; ++k) {
            const int dd = (b + k) & 7;
            nx = x + (int)((kDx >> (2 * dd)) & 3u) - 1, ny = y + (int)((kDy >> (2 * dd)) & 3u) - 1;
            if (mask_px(m, wpr, W, H, nx, ny)) {
                d = dd;
                break;
            }
        }
        if (d < 0) { // a single pixel
            a2 = 0;
            return TRACE_KEPT;
        }
        if (x == sx && y == sy) {
            if (d0 < 0)
                d0 = d;
            else if (d == d0) { // about to repeat the first move: the border is closed
                a2 = sum < 0 ? -sum : sum;
                return TRACE_KEPT;
            }
        }
        sum += (long long)x * ny - (long long)nx * y;
        x = nx, y = ny;
        b = (d - 2 - (d & 1)) & 7; // the clear pixel examined just before (nx, ny), seen from (nx, ny)
        if (!kExtent && (long long)y * W + x < start) return TRACE_NOT_FIRST;
        if (kExtent) ext[0] = min(ext[0], x), ext[1] = min(ext[1], y), ext[2] = max(ext[2], x), ext[3] = max(ext[3], y);
    }
    return TRACE_BOUND;
}

__device__ __forceinline__ unsigned mask_word(const unsigned *m, int wpr, int y, long long c) { return (c >= 0 && c < wpr) ? m[(long long)y * wpr + c] : 0u; }

// (l, w, r) of the lane's word column c in row y: neighbours by shuffle, loaded at a wave's end lanes
__device__ __forceinline__ void row_words(const unsigned *m, int wpr, int y, long long c, int lane, unsigned &l, unsigned &w, unsigned &r) {
    w = mask_word(m, wpr, y, c);
    l = __shfl_up(w, 1), r = __shfl_down(w, 1);
    if (lane == 0) l = mask_word(m, wpr, y, c - 1);
    if (lane == 63) r = mask_word(m, wpr, y, c + 1);
}

__global__ __launch_bounds__(kTraceThreads) void boxes_trace_kernel(const BoxArgs a) {
    const int lane = threadIdx.x & 63;
    long long unit = (long long)blockIdx.x * (kTraceThreads / 64) + (threadIdx.x >> 6); // (frame, strip, tile of 64 words)
    const int wt = (int)(unit % a.wtiles);
    unit /= a.wtiles;
    const int strip = (int)(unit % a.strips);
    const long long s = unit / a.strips;
    if (s >= a.n_sel || selected_frame(a, (int)s) < 0) return; // the whole wave
    const unsigned *m = a.mask + s * a.H * a.wpr;
    const long long c = (long long)wt * 64 + lane;
    const int y0 = strip * kStripRows, y1 = min(a.H, y0 + kStripRows);
    const long long max_steps = 8ll * a.H * a.W;
    unsigned nl = 0, nw = 0, nr = 0, l, w, r;
    if (y0 > 0) row_words(m, a.wpr, y0 - 1, c, lane, nl, nw, nr);
    u64 best = 0;
    for (int y = y0; y < y1; ++y) {
        row_words(m, a.wpr, y, c, lane, l, w, r);
        unsigned cand = w & ~((w << 1) | (l >> 31)) & ~nw & ~((nw << 1) | (nl >> 31)) & ~((nw >> 1) | (nr << 31));
        while (cand) {
            const int bit = __builtin_ctz(cand);
            cand &= cand - 1;
            const int x = (int)(32 * c) + bit;
            long long a2 = 0;
            const TraceResult t = trace_border<false>(m, a.wpr, a.W, a.H, x, y, max_steps, a2, nullptr);
            if (t == TRACE_KEPT) best = max(best, (((u64)a2 << kRootBits) | (u64)((long long)y * a.W + x)) + 1);
            if (t == TRACE_BOUND) best = kKeyFault;
        }
        nl = l, nw = w, nr = r;
    }
    if (best) atomicMax(&a.keys[s], best);
}

__global__ __launch_bounds__(256) void boxes_finish_kernel(const BoxArgs a) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= a.n_sel) return;
    int box[4] = {0, 0, 0, 0};
    long long a2 = 0;
    bool fault = selected_frame(a, s) < 0;
    const u64 key = fault ? 0 : a.keys[s];
    if (key == kKeyFault) fault = true;
    if (!fault && key && a.boxes) {
        const long long root = (long long)((key - 1) & ((1ull << kRootBits) - 1));
        int ext[4];
        const TraceResult t = trace_border<true>(a.mask + (long long)s * a.H * a.wpr, a.wpr, a.W, a.H, (int)(root % a.W), (int)(root / a.W), 8ll * a.H * a.W, a2, ext);
        if (t != TRACE_KEPT || a2 != (long long)((key - 1) >> kRootBits))
            fault = true;
        else
            box[0] = ext[0], box[1] = ext[1], box[2] = ext[2] - ext[0] + 1, box[3] = ext[3] - ext[1] + 1;
    }
    if (fault) {
        atomicAdd(a.faults, 1);
        box[0] = box[1] = box[2] = box[3] = -1, a2 = -1;
    }
    if (a.boxes)
#pragma unroll
        for (int k = 0; k < 4; ++k) a.boxes[4 * (long long)s + k] = box[k];
    if (a.area2) a.area2[s] = a2;
}

// mask_out[s][y][x] = 255 where the bit is set (0 for a frame that was not computed), one byte per thread and step
__global__ __launch_bounds__(256) void boxes_expand_kernel(const BoxArgs a) {
    const long long hw = (long long)a.H * a.W, total = hw * a.n_sel;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long s = i / hw, p = i - s * hw;
        const int y = (int)(p / a.W), x = (int)(p - (long long)y * a.W);
        const bool faulted = selected_frame(a, (int)s) < 0 || (a.boxes && a.keys[s] == kKeyFault);
        a.mask_out[i] = (!faulted && mask_px(a.mask + s * a.H * a.wpr, a.wpr, a.W, a.H, x, y)) ? 255 : 0;
    }
}

long long words_per_row(long long W) { return (W + 31) / 32; }
long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }
bool boxes_shape_ok(int32_t H, int32_t W, int32_t n_sel) { return H > 0 && W > 0 && n_sel > 0 && (long long)H * W <= (1ll << kRootBits); }

} // namespace

extern "C" int64_t wtk_boxes_scratch_bytes(int32_t H, int32_t W, int32_t n_sel) {
    if (!boxes_shape_ok(H, W, n_sel)) return -1;
    return (int64_t)n_sel * (8 + 4 * (int64_t)H * words_per_row(W));
}

extern "C" int wtk_boxes(const uint8_t *frames_dev, int32_t n_frames, int32_t H, int32_t W, const uint8_t *bg_dev, const int32_t *frame_idx_dev, int32_t n_sel,
                         int32_t diff_thresh, int32_t *boxes_dev, int64_t *area2_dev, uint8_t *mask_dev, int32_t *fault_count_dev, void *scratch,
                         int64_t scratch_bytes, void *stream) {
    if (!frames_dev || !bg_dev || !fault_count_dev || !scratch) return fail("wtk_boxes: null argument");
    if (!boxes_dev && area2_dev) return fail("wtk_boxes: null argument (area2_dev needs boxes_dev)");
    if (n_frames <= 0 || n_sel <= 0) return fail("wtk_boxes: n_frames and n_sel must be positive");
    if (!boxes_shape_ok(H, W, n_sel)) return fail("wtk_boxes: frames must be H x W gray with 0 < H * W <= 2^30");
    if (diff_thresh < 1 || diff_thresh > 255) return fail("wtk_boxes: diff_thresh must be in 1 .. 255");
    if (!frame_idx_dev && n_sel > n_frames) return fail("wtk_boxes: without frame ids n_sel must not exceed n_frames");
    if (scratch_bytes < wtk_boxes_scratch_bytes(H, W, n_sel)) return fail("wtk_boxes: scratch too small (wtk_boxes_scratch_bytes)");
    if ((uintptr_t)scratch % 8) return fail("wtk_boxes: scratch must be 8-byte aligned");
    BoxArgs a;
    a.frames = frames_dev, a.n_frames = n_frames, a.H = H, a.W = W, a.bg = bg_dev, a.frame_idx = frame_idx_dev, a.n_sel = n_sel, a.thr = diff_thresh;
    a.wpr = (int)words_per_row(W);
    a.bands = (int)ceil_div(H, kBandRows), a.ctiles = (int)ceil_div(a.wpr, kOutWords);
    a.strips = (int)ceil_div(H, kStripRows), a.wtiles = (int)ceil_div(a.wpr, 64);
    a.keys = reinterpret_cast<u64 *>(scratch), a.mask = reinterpret_cast<unsigned *>(a.keys + n_sel);
    a.boxes = boxes_dev, a.area2 = reinterpret_cast<long long *>(area2_dev), a.mask_out = mask_dev, a.faults = fault_count_dev;
    const long long mask_blocks = (long long)n_sel * a.bands * a.ctiles;
    const long long trace_blocks = ceil_div((long long)n_sel * a.strips * a.wtiles, kTraceThreads / 64);
    if (mask_blocks > INT_MAX || trace_blocks > INT_MAX) return fail("wtk_boxes: more than 2^31 - 1 blocks, split the selection");
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(a.keys, 0, 8 * (size_t)n_sel, s));
    hipLaunchKernelGGL(boxes_mask_kernel, dim3((unsigned)mask_blocks), dim3(kMaskThreads), 0, s, a);
    if (boxes_dev) hipLaunchKernelGGL(boxes_trace_kernel, dim3((unsigned)trace_blocks), dim3(kTraceThreads), 0, s, a);
    hipLaunchKernelGGL(boxes_finish_kernel, dim3((unsigned)ceil_div(n_sel, 256)), dim3(256), 0, s, a);
    if (mask_dev) {
        const long long blocks = std::min<long long>(ceil_div((long long)n_sel * H * W, 256), 1 << 18);
        hipLaunchKernelGGL(boxes_expand_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}
