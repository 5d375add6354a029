// The YOLO controller's closed loop from device-resident state: the one experiment kind whose targets depend on the camera view, so
// replay.hip's scan cannot run ahead of the detector.  Between two single-frame detector calls ONE thread turns the detector's float32 row into the move
// (numpy's float32 arithmetic of HipYoloController.provide_movement_vector) and the next cycle's position, where wtk_yolo_predict_views reads it; after the
// loop one thread per logged frame gives the frame's platform position (the detector's pos_xy for the log pass) and one thread per logged frame turns
// view-pixel detections into the absolute float64 track the rows kernel reads (TrackLogger's per-cycle float32 / float64 rule).  The motor is
// motor_steps() / frame_position() of replay_device.h, shared with scan and rows.  E = 1: every per-cycle array is [n_cycles][1][2].
#include "wtk_internal.h"
#include "replay_device.h"

using namespace wtk;

namespace {

struct YoloStepArgs {
    Geometry g;
    int c, C;
    const float *xywh;   // [4] the single-frame call's row, view pixels; NaN x 4 = no detection
    const double *share; // [M]
    int *pos;            // [C][1][2]: reads pos[c], writes pos[c + 1] (where c + 1 < C)
    int *move;           // [C][1][2]: writes move[c]
};

struct YoloPositionsArgs {
    ReplayView v;   // share, pos and move [C][1][2]; no track yet
    int *frame_pos; // [R][2] platform position at every logged frame's camera picture
};

struct YoloTrackArgs {
    Geometry g;
    long long R; // logged rows
    const float *xywh;    // [R][4] detections in view pixels
    const int *frame_pos; // [R][2] as the positions kernel wrote it
    double *track;        // [R][4] absolute xywh
};

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
__global__ __launch_bounds__(kRowThreads) void replay_yolo_positions_kernel(const YoloPositionsArgs a) {
    const long long r = (long long)blockIdx.x * kRowThreads + threadIdx.x;
    const ReplayView &v = a.v;
    if (r >= v.R) return;
    const RowCycle at = row_cycle(v.g, r);
    int px, py;
    frame_position(v.g, v.share, v.pos, v.move, at.c, at.step, px, py);
    a.frame_pos[2 * r] = px, a.frame_pos[2 * r + 1] = py;
}

__device__ __forceinline__ bool finite_row(const float *v) { return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]) && isfinite(v[3]); }

// one thread per logged frame: TrackLogger._write_rows' `boxes[:, 0] += cams[:, 0]` with the dtype the cycle's batch has there.  A cycle without a miss
// is a float32 array (the sum is rounded to float32, then widened); one NaN row makes the whole cycle float64.  Misses stay NaN.
__global__ __launch_bounds__(kRowThreads) void replay_yolo_track_kernel(const YoloTrackArgs a) {
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
    const int cam_x = a.frame_pos[2 * r] - g.cam_w / 2, cam_y = a.frame_pos[2 * r + 1] - g.cam_h / 2;
    if (any_miss) {
        o[0] = (double)v[0] + (double)cam_x, o[1] = (double)v[1] + (double)cam_y;
    } else {
        o[0] = (double)(v[0] + (float)cam_x), o[1] = (double)(v[1] + (float)cam_y);
    }
    o[2] = (double)v[2], o[3] = (double)v[3];
}

// the loop's population: one experiment whose track does not exist yet (every entry point refuses the nulls of what it reads)
int check_yolo(const char *who, const wtk_replay_config *cfg, int32_t n_cycles, const double *share_dev, const int32_t *pos_dev, const int32_t *move_dev, ReplayView &v) {
    // (the track these calls stand for is the detector's own output: it always has the R logged rows; pred_frame_num = 0 is the controller's oldest frame)
    if (replay_view(who, cfg, WTK_REPLAY_OPTIMAL, 1, n_cycles, nullptr, INT32_MAX, share_dev, pos_dev, move_dev, v, false)) return 1;
    if (v.g.cam_w > 8192 || v.g.cam_h > 8192 || cfg->frame_w > 8192 || cfg->frame_h > 8192)
        return fail(std::string(who) + ": camera and frame sizes up to 8192 (the float32 sums of the log are exact in the rows' float64 round trip below 2^13)");
    return 0;
}

unsigned row_blocks(long long R) { return (unsigned)((R + kRowThreads - 1) / kRowThreads); }

} // namespace

extern "C" int wtk_replay_yolo_step(const wtk_replay_config *cfg, int32_t n_cycles, int32_t c, const float *xywh_dev, const double *share_dev,
                                    int32_t *pos_dev, int32_t *move_dev, void *stream) {
    ReplayView v = {};
    if (check_yolo("wtk_replay_yolo_step", cfg, n_cycles, share_dev, pos_dev, move_dev, v)) return 1;
    if (!xywh_dev || !share_dev || !pos_dev || !move_dev) return fail("wtk_replay_yolo_step: null argument");
    if (c < 0 || c >= n_cycles) return fail("wtk_replay_yolo_step: cycle outside [0, n_cycles)");
    const YoloStepArgs a = {v.g, c, n_cycles, xywh_dev, share_dev, pos_dev, move_dev};
    hipLaunchKernelGGL(replay_yolo_step_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int wtk_replay_yolo_positions(const wtk_replay_config *cfg, int32_t n_cycles, const double *share_dev, const int32_t *pos_dev,
                                         const int32_t *move_dev, int32_t *frame_pos_dev, void *stream) {
    ReplayView v = {};
    if (check_yolo("wtk_replay_yolo_positions", cfg, n_cycles, share_dev, pos_dev, move_dev, v)) return 1;
    if (!share_dev || !pos_dev || !move_dev || !frame_pos_dev) return fail("wtk_replay_yolo_positions: null argument");
    const YoloPositionsArgs a = {v, frame_pos_dev};
    if (v.R > 0) hipLaunchKernelGGL(replay_yolo_positions_kernel, dim3(row_blocks(v.R)), dim3(kRowThreads), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int wtk_replay_yolo_track(const wtk_replay_config *cfg, int32_t n_cycles, const float *xywh_dev, const int32_t *frame_pos_dev, double *track_dev,
                                     void *stream) {
    ReplayView v = {};
    if (check_yolo("wtk_replay_yolo_track", cfg, n_cycles, nullptr, nullptr, nullptr, v)) return 1;
    if (!xywh_dev || !frame_pos_dev || !track_dev) return fail("wtk_replay_yolo_track: null argument");
    const YoloTrackArgs a = {v.g, v.R, xywh_dev, frame_pos_dev, track_dev};
    if (a.R > 0) hipLaunchKernelGGL(replay_yolo_track_kernel, dim3(row_blocks(a.R)), dim3(kRowThreads), 0, (hipStream_t)stream, a);
    HIP_TRY(hipGetLastError());
    return 0;
}
