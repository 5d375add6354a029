// Batched per-cycle predictors over a device-resident bbox track: the arithmetic of the reference's
// OptimalController (median head position of the next imaging phase), PolyfitController (weighted least-squares polynomial
// through sampled head centres, extrapolated) and NumpyDataset.create_from_config (ResMLP training pairs), for ALL cycles /
// rows of a track in one launch each.  These are a few dozen flops per cycle: latency-bound gathers, one thread per sample,
// fp64 like the reference's numpy code.  No MFMA, no LDS tiling — there is nothing to tile.
#include "wtk_kernels.h"
#include "polyfit_solve.h"

#include <cmath>

namespace wtk {
namespace {

template <typename T> __device__ __forceinline__ bool load_center(const T *track, int n_frames, int f, double &cx, double &cy) {
    if (f < 0 || f >= n_frames) return false;
    const double x = (double)track[4 * (long long)f + 0], y = (double)track[4 * (long long)f + 1];
    const double w = (double)track[4 * (long long)f + 2], h = (double)track[4 * (long long)f + 3];
    cx = x + w / 2; // BoxUtils.center / optimal_controller.py:12-14
    cy = y + h / 2;
    return isfinite(cx) && isfinite(cy);
}

__device__ __forceinline__ double median_sorted_insert(double *v, int n) {
    for (int i = 1; i < n; ++i) { // insertion sort: n <= kTrackMaxWindow
        const double key = v[i];
        int j = i - 1;
        while (j >= 0 && v[j] > key) {
            v[j + 1] = v[j];
            --j;
        }
        v[j + 1] = key;
    }
    return (n & 1) ? v[n / 2] : (v[n / 2 - 1] + v[n / 2]) / 2.0; // numpy.median: mean of the two middle values
}

// OptimalController.provide_movement_vector (optimal_controller.py:16-32) up to the camera offset: median centre of the
// finite rows among frames [(cycle+1)*cyc, +imaging)
template <typename T> __global__ __launch_bounds__(64) void track_median_kernel(const TrackMedianArgs a) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n_samples) return;
    const T *track = reinterpret_cast<const T *>(a.track);
    const long long lo = (long long)(a.cycles[i] + 1) * a.cycle_frame_num;
    double xs[kTrackMaxWindow], ys[kTrackMaxWindow];
    int n = 0;
    for (int k = 0; k < a.imaging_frame_num; ++k) {
        const long long f = lo + k;
        double cx, cy;
        if (f < a.n_frames && load_center(track, a.n_frames, (int)f, cx, cy)) xs[n] = cx, ys[n] = cy, ++n;
    }
    if (n == 0) {
        a.pred[2 * i] = a.pred[2 * i + 1] = 0.0;
        a.valid[i] = 0;
        return;
    }
    a.pred[2 * i] = median_sorted_insert(xs, n);
    a.pred[2 * i + 1] = median_sorted_insert(ys, n);
    a.valid[i] = 1;
}

// PolyfitController.provide_movement_vector (polyfit_controller.py:54-84) up to the camera offsets (the fit commutes with the
// translation by the camera corner): numpy's weighted polyfit through the finite samples of the cycle (len(t) = their count), then
// polyval at `t_eval`.  The fit itself is polyfit_solve.h's.
template <typename T> __global__ __launch_bounds__(64) void track_polyfit_kernel(const TrackPolyfitArgs a) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n_samples) return;
    const T *track = reinterpret_cast<const T *>(a.track);
    const int K = a.degree + 1;
    const long long base = (long long)a.cycles[i] * a.cycle_frame_num;
    double tt[kTrackMaxTimes], ww[kTrackMaxTimes], px[kTrackMaxTimes], py[kTrackMaxTimes];
    int n = 0;
    for (int j = 0; j < a.n_times; ++j) {
        const long long f = base + a.times[j];
        double cx, cy;
        if (f >= 0 && f < a.n_frames && load_center(track, a.n_frames, (int)f, cx, cy)) tt[n] = (double)a.times[j], ww[n] = a.weights[j], px[n] = cx, py[n] = cy, ++n;
    }
    PolyfitFactor fit;
    if (n == 0 || !polyfit_factor(fit, tt, ww, n, K)) { // no sample, or no converged SVD (never seen): "no prediction" rather than a silently wrong fit
        a.pred[2 * i] = a.pred[2 * i + 1] = 0.0;
        a.valid[i] = 0;
        return;
    }
    double x, y;
    polyfit_eval_axes(PolyfitLocal{fit, ww}, px, py, n, K, a.t_eval, x, y);
    a.pred[2 * i] = x;
    a.pred[2 * i + 1] = y;
    a.valid[i] = 1;
}

// NumpyDataset.create_from_config (neural/dataset.py:42-96): row r holds the boxes at r + input_frames and the box centres at
// r + pred_frames; float64 -> float32 FIRST, then relative to the (float32) corner of the first input box; rows with any NaN
// are flagged in `keep` (the caller compacts).  One thread per candidate row.
template <typename T> __global__ __launch_bounds__(64) void track_pairs_kernel(const TrackPairsArgs a) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= a.n_rows) return;
    const T *track = reinterpret_cast<const T *>(a.track);
    const long long r = (long long)a.row0 + i;
    float *X = a.X + (long long)i * 4 * a.n_in;
    float *Y = a.Y + (long long)i * 2 * a.n_out;
    bool ok = true;
    for (int j = 0; j < a.n_in; ++j) {
        const long long f = r + a.in_frames[j];
        for (int c = 0; c < 4; ++c) {
            const double v = (f >= 0 && f < a.n_frames) ? (double)track[4 * f + c] : nan("");
            ok = ok && !isnan(v);
            X[4 * j + c] = (float)v;
        }
    }
    for (int j = 0; j < a.n_out; ++j) {
        const long long f = r + a.out_frames[j];
        double cx = nan(""), cy = nan("");
        if (f >= 0 && f < a.n_frames) {
            cx = (double)track[4 * f + 0] + (double)track[4 * f + 2] / 2;
            cy = (double)track[4 * f + 1] + (double)track[4 * f + 3] / 2;
        }
        ok = ok && !isnan(cx) && !isnan(cy);
        Y[2 * j] = (float)cx;
        Y[2 * j + 1] = (float)cy;
    }
    const float x0 = X[0], y0 = X[1];
    for (int j = 0; j < a.n_out; ++j) Y[2 * j] -= x0, Y[2 * j + 1] -= y0;
    for (int j = 0; j < a.n_in; ++j) X[4 * j] -= x0, X[4 * j + 1] -= y0;
    a.keep[i] = ok ? 1 : 0;
}

// rank of every margin among the batch's (ties broken by row): the K smallest go to slots[rank]; for the ORDER a NaN counts as +inf
// (it ties with a real +inf, lower row first).  The weak rows are counted on the RAW margin (margin < thr: a NaN row is never weak,
// whatever thr — +inf included — exactly as recheck_merge_kernel and recheck_enqueue_plan_kernel decide it) by all 256 threads (wave
// shuffles + one LDS add per wave); what the ceiling K cuts off is ADDED to *n_overflow, so that a caller with K < B can see that rows
// kept their fast result without a second look.
__global__ __launch_bounds__(256) void recheck_select_kernel(const RecheckArgs a) {
    __shared__ float m[1024];
    __shared__ int weak;
    if (threadIdx.x == 0) weak = 0;
    for (int i = threadIdx.x; i < a.B; i += 256) {
        const float v = a.margins[i];
        m[i] = v == v ? v : INFINITY;
    }
    __syncthreads();
    int mine = 0;
    for (int i = threadIdx.x; i < a.B; i += 256) {
        const float mi = m[i];
        int rank = 0;
        for (int j = 0; j < a.B; ++j) rank += (m[j] < mi || (m[j] == mi && j < i)) ? 1 : 0;
        if (rank < a.K) a.slots[rank] = i;
        mine += a.margins[i] < a.thr ? 1 : 0;
    }
    if (a.n_weak || a.n_overflow) {
        for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off, 64);
        if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&weak, mine);
        __syncthreads();
        if (threadIdx.x == 0) {
            const int n = weak;
            if (a.n_weak) *a.n_weak = n < a.K ? n : a.K;
            if (a.n_overflow && n > a.K) *a.n_overflow += n - a.K;  // one block per launch, launches of a stream are ordered: a plain add
        }
    }
}

__global__ __launch_bounds__(64) void recheck_merge_kernel(const RecheckArgs a) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= a.K) return;
    const int row = a.slots[k];
    if ((unsigned)row >= (unsigned)a.B || !(a.margins[row] < a.thr)) return;
    reinterpret_cast<float4 *>(a.dst_xywh)[row] = reinterpret_cast<const float4 *>(a.src_xywh)[k];
    if (a.dst_conf && a.src_conf) a.dst_conf[row] = a.src_conf[k];
    if (a.dst_anchor && a.src_anchor) a.dst_anchor[row] = a.src_anchor[k];
    if (a.n_replaced) atomicAdd(a.n_replaced, 1);
}

// ---- deferred second look: queue of weak rows over several fast passes
// one block: queue position of every weak row of the batch (row order), the addresses its re-detected row will be written to, the new length
__global__ __launch_bounds__(256) void recheck_enqueue_plan_kernel(const RecheckQueueArgs a) {
    __shared__ int weak[1024];
    __shared__ int total;
    const int len0 = *a.q_len;
    for (int i = threadIdx.x; i < a.B; i += 256) {
        const float v = a.margins[i];
        weak[i] = (v == v && v < a.thr) ? 1 : 0; // NaN margin = no decision to revisit
    }
    __syncthreads();
    for (int i = threadIdx.x; i < a.B; i += 256) {
        int before = 0;
        for (int j = 0; j < i; ++j) before += weak[j];
        int p = -1;
        if (weak[i] && len0 + before < a.q_cap) {
            p = len0 + before;
            a.q_xywh[p] = a.dst_xywh + 4 * (long long)i;
            a.q_conf[p] = a.dst_conf ? a.dst_conf + i : nullptr;
            a.q_anchor[p] = a.dst_anchor ? a.dst_anchor + i : nullptr;
        }
        a.pos[i] = p;
        if (i == a.B - 1) total = before + weak[i];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int fit = min(total, a.q_cap - len0);
        *a.q_len = len0 + fit;
        if (a.n_overflow && total > fit) *a.n_overflow += total - fit;
    }
}

// blockIdx.y = batch row; its frame goes to its queue slot, 16 bytes per thread and step (rows that are not queued exit at once)
__global__ __launch_bounds__(256) void recheck_enqueue_copy_kernel(const RecheckQueueArgs a) {
    const int b = blockIdx.y;
    const int p = a.pos[b];
    if (p < 0) return;
    const uint4 *src = reinterpret_cast<const uint4 *>(a.frames + (long long)b * a.frame_bytes);
    uint4 *dst = reinterpret_cast<uint4 *>(a.q_frames + (long long)p * a.frame_bytes);
    const long long n16 = a.frame_bytes / 16;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n16; i += (long long)gridDim.x * 256) dst[i] = src[i];
}

__global__ __launch_bounds__(64) void recheck_scatter_kernel(const RecheckQueueArgs a) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= *a.q_len || k >= a.q_cap) return;
    *reinterpret_cast<float4 *>(a.q_xywh[k]) = reinterpret_cast<const float4 *>(a.src_xywh)[k];
    if (a.q_conf[k] && a.src_conf) *a.q_conf[k] = a.src_conf[k];
    if (a.q_anchor[k] && a.src_anchor) *a.q_anchor[k] = a.src_anchor[k];
    if (a.n_replaced) atomicAdd(a.n_replaced, 1);
}

// the weak rows' (frame, view centre) for the second look of the views entry point: row i of the second look = batch row slots[i]
__global__ __launch_bounds__(64) void recheck_gather_views_kernel(const int *slots, int K, const int *frame_index, const int *pos_xy, int *idx_out, int *pos_out) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= K) return;
    const int b = slots[i];
    idx_out[i] = frame_index ? frame_index[b] : b;
    pos_out[2 * i] = pos_xy[2 * b], pos_out[2 * i + 1] = pos_xy[2 * b + 1];
}

} // namespace

hipError_t launch_recheck_gather_views(const int *slots, int K, const int *frame_index, const int *pos_xy, int *idx_out, int *pos_out, hipStream_t stream) {
    if (K <= 0 || !slots || !pos_xy || !idx_out || !pos_out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(recheck_gather_views_kernel, dim3((unsigned)((K + 63) / 64)), dim3(64), 0, stream, slots, K, frame_index, pos_xy, idx_out, pos_out);
    return hipGetLastError();
}

hipError_t launch_recheck_enqueue(const RecheckQueueArgs &a, hipStream_t stream) {
    if (a.B <= 0 || a.B > 1024 || a.q_cap <= 0 || a.frame_bytes <= 0 || a.frame_bytes % 16) return hipErrorInvalidValue;
    hipLaunchKernelGGL(recheck_enqueue_plan_kernel, dim3(1), dim3(256), 0, stream, a);
    const long long n16 = a.frame_bytes / 16;
    const unsigned bx = (unsigned)((n16 + 256 * 8 - 1) / (256 * 8) > 64 ? 64 : (n16 + 256 * 8 - 1) / (256 * 8)); // <= 64 blocks per frame, >= 8 steps each
    hipLaunchKernelGGL(recheck_enqueue_copy_kernel, dim3(bx ? bx : 1, (unsigned)a.B), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_recheck_scatter(const RecheckQueueArgs &a, hipStream_t stream) {
    if (a.q_cap <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(recheck_scatter_kernel, dim3((unsigned)((a.q_cap + 63) / 64)), dim3(64), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return hipMemsetAsync(a.q_len, 0, sizeof(int), stream); // the queue is empty again (stream order: after the scatter)
}

hipError_t launch_recheck_select(const RecheckArgs &a, hipStream_t stream) {
    if (a.B <= 0 || a.B > 1024 || a.K <= 0 || a.K > a.B) return hipErrorInvalidValue;
    hipLaunchKernelGGL(recheck_select_kernel, dim3(1), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_recheck_merge(const RecheckArgs &a, hipStream_t stream) {
    if (a.B <= 0 || a.K <= 0 || a.K > a.B) return hipErrorInvalidValue;
    hipLaunchKernelGGL(recheck_merge_kernel, dim3((unsigned)((a.K + 63) / 64)), dim3(64), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_track_median(const TrackMedianArgs &a, int track_f64, hipStream_t stream) {
    if (a.n_samples <= 0 || a.imaging_frame_num <= 0 || a.imaging_frame_num > kTrackMaxWindow || a.cycle_frame_num <= 0) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((a.n_samples + 63) / 64));
    if (track_f64)
        hipLaunchKernelGGL(track_median_kernel<double>, grid, dim3(64), 0, stream, a);
    else
        hipLaunchKernelGGL(track_median_kernel<float>, grid, dim3(64), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_track_polyfit(const TrackPolyfitArgs &a, int track_f64, hipStream_t stream) {
    if (a.n_samples <= 0 || a.n_times <= 0 || a.n_times > kTrackMaxTimes || a.degree < 0 || a.degree + 1 > kTrackMaxCoef || a.cycle_frame_num <= 0)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)((a.n_samples + 63) / 64));
    if (track_f64)
        hipLaunchKernelGGL(track_polyfit_kernel<double>, grid, dim3(64), 0, stream, a);
    else
        hipLaunchKernelGGL(track_polyfit_kernel<float>, grid, dim3(64), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_track_pairs(const TrackPairsArgs &a, int track_f64, hipStream_t stream) {
    if (a.n_rows <= 0 || a.n_in <= 0 || a.n_in > kTrackMaxTimes || a.n_out <= 0 || a.n_out > kTrackMaxTimes) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((a.n_rows + 63) / 64));
    if (track_f64)
        hipLaunchKernelGGL(track_pairs_kernel<double>, grid, dim3(64), 0, stream, a);
    else
        hipLaunchKernelGGL(track_pairs_kernel<float>, grid, dim3(64), 0, stream, a);
    return hipGetLastError();
}

} // namespace wtk
