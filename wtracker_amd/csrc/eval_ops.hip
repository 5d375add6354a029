// Experiment evaluation on the device: the background of an experiment (BGExtractor.calc_background, wtracker/dataset/bg_extractor.py:18-75)
// and the precise tracking error of a log (ErrorCalculator.calculate_precise, wtracker/eval/error_calculator.py:64-160), both bit-exact to the
// reference's numpy arithmetic.
//
// Background: per-byte median or mean over n probe frames, streamed along the pixel axis.  Lane l of a block owns 4 consecutive bytes of every
// probe, so a wave reads 256 contiguous bytes of one probe per load and 16 loads (16 probes) are in flight per lane.
//   median  two-pass radix select by nibble.  Pass A counts the high nibbles of the lane's 4 bytes into 4 x 16 uint16 bins in LDS (two bins per
//           32-bit word, one ds_add per byte; the words are lane-private and lane-minor, bank = lane % 32 whatever the data), which gives the high
//           nibble and the residual rank of the two middle ranks (n-1)/2 and n/2.  Pass B re-reads the probes and counts the low nibbles of the
//           bytes in the first middle rank's bucket; the second middle rank, when it falls in a later bucket, is that bucket's smallest byte (a
//           running minimum).  np.median(...).astype(uint8) is floor((a + b) / 2) of the two middle values (numpy averages them in float64, the
//           cast truncates).  2 n bytes read per output byte; uint16 bins keep n <= 65535 exact.
//   mean    uint32 sums in registers, floor(sum / n) = the reference's float64 sum / n with a truncating cast; n <= 2^24 keeps 255 n < 2^32.
// Precise error: one wave per log row (grid-stride).  The worm and microscope boxes are discretised as BoxUtils.discretize does
// (bbox_utils.py:118-167: x + w in the array's own dtype, floor / ceil, the int32 cast, clip to the frame, zero-area boxes illegal), the wave walks the
// worm crop of the row's full frame and counts |frame - background| > thr (total) and the same pixels inside the worm / microscope intersection
// (inside) with ballots; err = 1 - inside / total in float64, 0 where total = 0, NaN for an illegal worm box or a frame number outside [0, F).
// The row's rules (discretize, intersect, crop_walk, precise_error_of) live in eval_device.h, shared with replay_precise_kernel (replay_precise.hip).
#include "wtk_internal.h"
#include "eval_device.h"

#include <algorithm>
#include <climits>
#include <cmath>

using namespace wtk;

namespace {

constexpr int kBgThreads = 256;
constexpr int kBgBytes = 4;  // bytes per lane
constexpr int kBgUnroll = 16; // probe loads in flight per lane
constexpr int kBgMedianMaxProbes = 65535;
constexpr int kBgMeanMaxProbes = 1 << 24;
constexpr int kPeThreads = 256; // four rows per block

struct BackgroundArgs {
    const uint8_t *frames; // [n_frames][frame_bytes]
    long long frame_bytes;
    int n_frames;
    const int *probe_idx; // [n_probes] frame ids, or null: frames 0 .. n_probes - 1
    int n_probes;
    uint8_t *bg; // [frame_bytes]
};

struct PreciseErrorArgs {
    const uint8_t *frames; // [n_frames][H][W] gray
    int n_frames, H, W;
    const uint8_t *bg;          // [H][W]
    const void *worm, *mic;     // [n_rows][4] xywh, float or double
    const int *frame_nums;      // [n_rows]
    int n_rows;
    int thr;                    // a pixel is foreground where |frame - bg| > thr (the integer form of the float threshold)
    double *err;                // [n_rows]
    int *counts;                // [n_rows][2] (total, inside), nullable
    int *n_bad_frame;           // += rows with a legal worm box and a frame number outside [0, n_frames), nullable
};

__device__ __forceinline__ const uint8_t *probe_frame(const BackgroundArgs &a, int p) {
    long long f = a.probe_idx ? a.probe_idx[p] : p;
    f = f < 0 ? 0 : (f >= a.n_frames ? a.n_frames - 1 : f); // memory safety only: the entry point requires ids in [0, n_frames)
    return a.frames + f * a.frame_bytes;
}

// the lane's 4 bytes of one probe (byte j in bits 8j .. 8j+7); kVec: 4-byte aligned, whole chunk in range
template <bool kVec> __device__ __forceinline__ unsigned load4(const uint8_t *frame, long long off, long long n) {
    if (kVec) return *reinterpret_cast<const unsigned *>(frame + off);
    unsigned v = 0;
#pragma unroll
    for (int j = 0; j < kBgBytes; ++j)
        if (off + j < n) v |= (unsigned)frame[off + j] << (8 * j);
    return v;
}

template <bool kVec> __device__ __forceinline__ void store4(uint8_t *bg, long long off, long long n, unsigned v) {
    if (kVec) {
        *reinterpret_cast<unsigned *>(bg + off) = v;
        return;
    }
#pragma unroll
    for (int j = 0; j < kBgBytes; ++j)
        if (off + j < n) bg[off + j] = (uint8_t)(v >> (8 * j));
}

// one probe's 4 bytes into the lane's histograms: bin of byte e = its high nibble (kHigh) or, for bytes whose high nibble is hsel[e], its low nibble
template <bool kHigh> __device__ __forceinline__ void count4(unsigned (*bins)[8][64], int lane, unsigned w, const int *hsel, int *mn) {
#pragma unroll
    for (int e = 0; e < kBgBytes; ++e) {
        const unsigned v = (w >> (8 * e)) & 255u;
        const unsigned key = kHigh ? v >> 4 : v & 15u;
        const unsigned inc = (kHigh || (int)(v >> 4) == hsel[2 * e]) ? 1u << (16 * (key & 1u)) : 0u;
        atomicAdd(&bins[e][key >> 1][lane], inc); // lane-private word: ds_add is the one-instruction read-modify-write of LDS (5 % faster than ds_read + ds_write)
        if (!kHigh && (int)(v >> 4) == hsel[2 * e + 1]) mn[e] = min(mn[e], (int)key);
    }
}

template <bool kHigh, bool kVec>
__device__ __forceinline__ void count_pass(const BackgroundArgs &a, unsigned (*bins)[8][64], int lane, long long off, const int *hsel, int *mn) {
    int p = 0;
    for (; p + kBgUnroll <= a.n_probes; p += kBgUnroll) {
        unsigned w[kBgUnroll];
#pragma unroll
        for (int u = 0; u < kBgUnroll; ++u) w[u] = load4<kVec>(probe_frame(a, p + u), off, a.frame_bytes);
#pragma unroll
        for (int u = 0; u < kBgUnroll; ++u) count4<kHigh>(bins, lane, w[u], hsel, mn);
    }
    for (; p < a.n_probes; ++p) count4<kHigh>(bins, lane, load4<kVec>(probe_frame(a, p), off, a.frame_bytes), hsel, mn);
}

// bin and residual rank of rank k in the 16 uint16 bins of element e
__device__ __forceinline__ void select_bin(unsigned (*bins)[8][64], int e, int lane, int k, int &bin, int &rest) {
    int c = 0;
    bin = 15, rest = 0;
    bool found = false;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const unsigned w = bins[e][q][lane];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int cnt = (int)((w >> (16 * s)) & 0xffffu);
            if (!found && c + cnt > k) found = true, bin = 2 * q + s, rest = k - c;
            c += cnt;
        }
    }
}

__device__ __forceinline__ void clear_bins(unsigned (*bins)[8][64], int lane) {
#pragma unroll
    for (int e = 0; e < kBgBytes; ++e)
#pragma unroll
        for (int q = 0; q < 8; ++q) bins[e][q][lane] = 0u;
}

template <bool kVec> __global__ __launch_bounds__(kBgThreads) void background_median_kernel(const BackgroundArgs a) {
    __shared__ unsigned bins_all[kBgThreads / 64][kBgBytes][8][64]; // [wave][byte][bin pair][lane]: 32 KiB
    const int lane = threadIdx.x & 63;
    unsigned (*bins)[8][64] = bins_all[threadIdx.x >> 6];
    const long long off = ((long long)blockIdx.x * kBgThreads + threadIdx.x) * kBgBytes;
    if (off >= a.frame_bytes) return; // no barrier below: every word is private to its lane
    const int k0 = (a.n_probes - 1) / 2, k1 = a.n_probes / 2;
    int hsel[2 * kBgBytes] = {}, r0[kBgBytes], r1[kBgBytes], mn[kBgBytes] = {};
    clear_bins(bins, lane);
    count_pass<true, kVec>(a, bins, lane, off, hsel, mn);
#pragma unroll
    for (int e = 0; e < kBgBytes; ++e) {
        select_bin(bins, e, lane, k0, hsel[2 * e], r0[e]);
        select_bin(bins, e, lane, k1, hsel[2 * e + 1], r1[e]);
        mn[e] = 15;
    }
    clear_bins(bins, lane);
    count_pass<false, kVec>(a, bins, lane, off, hsel, mn);
    unsigned out = 0;
#pragma unroll
    for (int e = 0; e < kBgBytes; ++e) {
        const int h0 = hsel[2 * e], h1 = hsel[2 * e + 1];
        int l0, l1, unused;
        select_bin(bins, e, lane, r0[e], l0, unused);
        if (h1 == h0)
            select_bin(bins, e, lane, r1[e], l1, unused);
        else
            l1 = mn[e]; // rank n/2 opens the next non-empty bucket: its smallest byte
        out |= (unsigned)((((h0 << 4) | l0) + ((h1 << 4) | l1)) >> 1) << (8 * e);
    }
    store4<kVec>(a.bg, off, a.frame_bytes, out);
}

template <bool kVec> __global__ __launch_bounds__(kBgThreads) void background_mean_kernel(const BackgroundArgs a) {
    const long long off = ((long long)blockIdx.x * kBgThreads + threadIdx.x) * kBgBytes;
    if (off >= a.frame_bytes) return;
    unsigned s[kBgBytes] = {0u, 0u, 0u, 0u};
    int p = 0;
    for (; p + kBgUnroll <= a.n_probes; p += kBgUnroll) {
        unsigned w[kBgUnroll];
#pragma unroll
        for (int u = 0; u < kBgUnroll; ++u) w[u] = load4<kVec>(probe_frame(a, p + u), off, a.frame_bytes);
#pragma unroll
        for (int u = 0; u < kBgUnroll; ++u)
#pragma unroll
            for (int e = 0; e < kBgBytes; ++e) s[e] += (w[u] >> (8 * e)) & 255u;
    }
    for (; p < a.n_probes; ++p) {
        const unsigned w = load4<kVec>(probe_frame(a, p), off, a.frame_bytes);
#pragma unroll
        for (int e = 0; e < kBgBytes; ++e) s[e] += (w >> (8 * e)) & 255u;
    }
    unsigned out = 0;
#pragma unroll
    for (int e = 0; e < kBgBytes; ++e) out |= (s[e] / (unsigned)a.n_probes) << (8 * e);
    store4<kVec>(a.bg, off, a.frame_bytes, out);
}

template <typename T> __global__ __launch_bounds__(kPeThreads) void precise_error_kernel(const PreciseErrorArgs a) {
    const int lane = threadIdx.x & 63;
    const T *worm = reinterpret_cast<const T *>(a.worm);
    const T *mic = reinterpret_cast<const T *>(a.mic);
    for (long long r = (long long)blockIdx.x * (kPeThreads / 64) + (threadIdx.x >> 6); r < a.n_rows; r += (long long)gridDim.x * (kPeThreads / 64)) {
        int wl, wt, wr, wb, ml, mt, mr, mb;
        const bool legal = discretize(worm + 4 * r, a.H, a.W, wl, wt, wr, wb);
        const int f = a.frame_nums[r];
        if (!legal || f < 0 || f >= a.n_frames) {
            if (lane == 0) {
                a.err[r] = nan("");
                if (a.counts) a.counts[2 * r] = a.counts[2 * r + 1] = 0;
                if (legal && a.n_bad_frame) atomicAdd(a.n_bad_frame, 1);
            }
            continue;
        }
        discretize(mic + 4 * r, a.H, a.W, ml, mt, mr, mb); // an illegal microscope box is (0, 0, 0, 0): an empty intersection
        int il, it, ir, ib, total, inside;
        intersect(wl, wt, wr, wb, ml, mt, mr, mb, il, it, ir, ib);
        crop_walk(a.frames + (long long)f * a.H * a.W, a.bg, a.W, a.thr, lane, wl, wt, wr, wb, il, it, ir, ib, total, inside);
        if (lane == 0) {
            a.err[r] = precise_error_of(total, inside);
            if (a.counts) a.counts[2 * r] = total, a.counts[2 * r + 1] = inside;
        }
    }
}

} // namespace

extern "C" int wtk_background(const uint8_t *frames_dev, int32_t n_frames, int64_t frame_bytes, const int32_t *probe_idx_dev, int32_t n_probes,
                              int32_t method, uint8_t *bg_dev, void *stream) {
    if (!frames_dev || !bg_dev) return fail("wtk_background: null argument");
    if (n_frames <= 0 || frame_bytes <= 0 || n_probes <= 0) return fail("wtk_background: n_frames, frame_bytes and n_probes must be positive");
    if (method != WTK_BG_MEDIAN && method != WTK_BG_MEAN) return fail("wtk_background: method must be WTK_BG_MEDIAN or WTK_BG_MEAN");
    if (method == WTK_BG_MEDIAN && n_probes > kBgMedianMaxProbes) return fail("wtk_background: the median takes at most 65535 probes (uint16 counts)");
    if (method == WTK_BG_MEAN && n_probes > kBgMeanMaxProbes) return fail("wtk_background: the mean takes at most 2^24 probes (uint32 sums)");
    if (!probe_idx_dev && n_probes > n_frames) return fail("wtk_background: without probe ids n_probes must not exceed n_frames");
    const long long blocks = (frame_bytes + (long long)kBgThreads * kBgBytes - 1) / ((long long)kBgThreads * kBgBytes);
    if (blocks > INT_MAX) return fail("wtk_background: frame too large");
    BackgroundArgs a;
    a.frames = frames_dev, a.frame_bytes = frame_bytes, a.n_frames = n_frames, a.probe_idx = probe_idx_dev, a.n_probes = n_probes, a.bg = bg_dev;
    const bool vec = frame_bytes % kBgBytes == 0 && (uintptr_t)frames_dev % kBgBytes == 0 && (uintptr_t)bg_dev % kBgBytes == 0;
    const dim3 grid((unsigned)blocks), block(kBgThreads);
    hipStream_t s = (hipStream_t)stream;
    if (method == WTK_BG_MEDIAN) {
        if (vec)
            hipLaunchKernelGGL(background_median_kernel<true>, grid, block, 0, s, a);
        else
            hipLaunchKernelGGL(background_median_kernel<false>, grid, block, 0, s, a);
    } else {
        if (vec)
            hipLaunchKernelGGL(background_mean_kernel<true>, grid, block, 0, s, a);
        else
            hipLaunchKernelGGL(background_mean_kernel<false>, grid, block, 0, s, a);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int wtk_precise_error(const uint8_t *frames_dev, int32_t n_frames, int32_t H, int32_t W, const uint8_t *bg_dev, const void *worm_xywh_dev,
                                 const void *mic_xywh_dev, int32_t boxes_are_f64, const int32_t *frame_nums_dev, int32_t n_rows, double diff_thresh,
                                 double *err_dev, int32_t *counts_dev, int32_t *n_bad_frame_dev, void *stream) {
    if (!frames_dev || !bg_dev || !worm_xywh_dev || !mic_xywh_dev || !frame_nums_dev || !err_dev) return fail("wtk_precise_error: null argument");
    if (n_frames < 0 || n_rows < 0) return fail("wtk_precise_error: negative size");
    if (H <= 0 || W <= 0 || (long long)H * W > (1ll << 30)) return fail("wtk_precise_error: frames must be H x W gray with 0 < H * W <= 2^30");
    if (n_rows == 0) return 0;
    PreciseErrorArgs a;
    a.frames = frames_dev, a.n_frames = n_frames, a.H = H, a.W = W, a.bg = bg_dev, a.worm = worm_xywh_dev, a.mic = mic_xywh_dev;
    a.frame_nums = frame_nums_dev, a.n_rows = n_rows, a.thr = threshold_int(diff_thresh), a.err = err_dev, a.counts = counts_dev;
    a.n_bad_frame = n_bad_frame_dev;
    const long long rows_per_block = kPeThreads / 64;
    const dim3 grid((unsigned)std::min<long long>((n_rows + rows_per_block - 1) / rows_per_block, 16384)), block(kPeThreads);
    if (boxes_are_f64)
        hipLaunchKernelGGL(precise_error_kernel<double>, grid, block, 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(precise_error_kernel<float>, grid, block, 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}
