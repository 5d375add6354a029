// The rules of the precise tracking error (ErrorCalculator.calculate_precise, wtracker/eval/error_calculator.py:64-160) that more than one kernel
// needs, stated once: numpy's float -> int32 cast, BoxUtils.discretize (bbox_utils.py:118-167), the integer form of the foreground threshold, the
// worm / microscope intersection and the wave's walk over a worm crop.  precise_error_kernel (eval_ops.hip) and replay_precise_kernel (replay_precise.hip)
// call these functions, so a log row and a replayed (experiment, frame) pair with the same boxes get the same counts.
#pragma once
#include <climits>
#include <cmath>
#include <cstdint>

#include <hip/hip_runtime.h>

namespace wtk {

// numpy's float -> int32 cast on x86-64 (cvttsd2si): out of range and NaN give INT_MIN
__device__ __forceinline__ int to_i32(double v) { return (v >= -2147483648.0 && v < 2147483648.0) ? (int)v : INT_MIN; }
__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// BoxUtils.discretize of one xywh row to xyxy; false (and a zero box) when the row is illegal
template <typename T> __device__ __forceinline__ bool discretize(const T *box, int H, int W, int &x1, int &y1, int &x2, int &y2) {
    T x = box[0], y = box[1], w = box[2], h = box[3];
    if (!(isfinite(x) && isfinite(y) && isfinite(w) && isfinite(h))) x = y = w = h = (T)0;
    const T xr = x + w, yb = y + h; // BoxConverter.to_xyxy in the array's dtype
    x1 = clampi(to_i32(floor((double)x)), W), y1 = clampi(to_i32(floor((double)y)), H);
    x2 = clampi(to_i32(ceil((double)xr)), W), y2 = clampi(to_i32(ceil((double)yb)), H);
    if (x2 - x1 > 0 && y2 - y1 > 0) return true;
    x1 = y1 = x2 = y2 = 0;
    return false;
}

// the worm / microscope intersection in xyxy, as the reference forms it: a corner and a non-negative size.  An empty one has ir == il or ib == it,
// and then (il, it) may lie OUTSIDE the worm box: nothing may be indexed with it before the emptiness is decided.
__device__ __forceinline__ void intersect(int wl, int wt, int wr, int wb, int ml, int mt, int mr, int mb, int &il, int &it, int &ir, int &ib) {
    il = max(wl, ml), it = max(wt, mt);
    ir = il + max(0, min(wr, mr) - il), ib = it + max(0, min(wb, mb) - it);
}

// One wave walks the worm crop [wl, wr) x [wt, wb) of a full frame (row pitch W): total = pixels with |frame - bg| > thr, inside = those of them
// inside [il, ir) x [it, ib).  Every lane of the wave must call it with the same arguments; every lane gets both counts.
__device__ __forceinline__ void crop_walk(const uint8_t *fr, const uint8_t *bg, int W, int thr, int lane, int wl, int wt, int wr, int wb, int il, int it,
                                          int ir, int ib, int &total, int &inside) {
    const int cw = wr - wl, npx = cw * (wb - wt);
    total = 0, inside = 0;
    for (int i0 = 0; i0 < npx; i0 += 64) { // wave-uniform trip count
        const int i = i0 + lane;
        bool fg = false, in = false;
        if (i < npx) {
            const int yy = i / cw, X = wl + (i - yy * cw), Y = wt + yy;
            const long long o = (long long)Y * W + X;
            fg = abs((int)fr[o] - (int)bg[o]) > thr;
            in = fg && X >= il && X < ir && Y >= it && Y < ib;
        }
        total += __popcll(__ballot(fg));
        inside += __popcll(__ballot(in));
    }
}

// err of a row from its counts: float64, 0 where nothing is foreground
__device__ __forceinline__ double precise_error_of(int total, int inside) { return total == 0 ? 0.0 : 1.0 - (double)inside / (double)total; }

// |frame - bg| > t for integer |frame - bg| in [0, 255]: > floor(t) for finite t.  The entry points of one track call it on the host; a set's kernels
// call it per block on the threshold of the block's track (the frames table holds the double).
__host__ __device__ inline int threshold_int(double t) {
    if (t != t || t >= 255.0) return 255; // (NaN) nothing is foreground
    if (t < 0.0) return -1;               // everything is
    return (int)floor(t);
}

} // namespace wtk
