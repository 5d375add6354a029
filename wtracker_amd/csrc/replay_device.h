// The closed loop's device functions that more than one translation unit calls (replay.hip, replay_analysis.hip): the geometry, the ONE statement of the
// motor, the platform position of a logged frame, the boxes and the bbox error of a log row, and the host-side refusals of an experiment's geometry.
// Everything relies on -ffp-contract=off (the library's build flag): share * move + carry is a rounded product and a rounded sum, as in Python.
#pragma once
#include "wtk_internal.h"

#include <cmath>
#include <string>

namespace wtk {

struct Geometry {
    int L, I, M, P;
    int cam_w, cam_h, mic_w, mic_h;
    int x_max, y_max; // frame_w - 1, frame_h - 1: the clamp of the platform position
};

// one step of SineMotorController.step + ViewController.move_position on one axis
__device__ __forceinline__ void motor_axis(double share, double mv, double &carry, int &pos, int pos_max) {
    const double want = share * mv + carry;
    const double took = rint(want); // round half to even: Python's round on a float
    carry = want - took;
    pos = (int)fmin(fmax((double)pos + took, 0.0), (double)pos_max);
}

// `steps` motor steps of the move (mx, my) from (px, py), the carry starting at zero: what a cycle's moving phase does to the platform (steps = M) and what
// has happened to it before a frame of that phase (steps < M).  The ONE statement of the motor: the scan, the rows and the YOLO loop's kernels all call it.
__device__ __forceinline__ void motor_steps(const Geometry &g, const double *share, int steps, double mx, double my, int &px, int &py) {
    double cx = 0.0, cy = 0.0;
    for (int k = 0; k < steps; ++k) {
        const double sh = share[k];
        motor_axis(sh, mx, cx, px, g.x_max);
        motor_axis(sh, my, cy, py, g.y_max);
    }
}

// the platform position at the camera picture of step `step` of a cycle, from the cycle's start position and move ([C][E][2] entry ce)
__device__ __forceinline__ void frame_position(const Geometry &g, const double *share, const int *pos, const int *move, long long ce, int step, int &px, int &py) {
    px = pos[2 * ce], py = pos[2 * ce + 1];
    const int done = step <= g.I ? 0 : (step - g.I > g.M ? g.M : step - g.I); // motor steps taken before this frame's camera picture
    if (done > 0) motor_steps(g, share, done, (double)move[2 * ce], (double)move[2 * ce + 1], px, py);
}

// The boxes of a log row from the platform position at its camera picture: camera and microscope corners, and the logged worm box, which is the track's
// row made camera-relative (CsvController.predict) and absolute again (LoggingController); a non-finite row is logged as zeros.  (x - cam) + cam is not
// always x: the rows kernel and the precise kernel both take the box from here.
struct RowBoxes {
    double cam_x, cam_y, mic_x, mic_y, mic_w, mic_h;
    double wx, wy, ww, wh;
};

__device__ __forceinline__ RowBoxes row_boxes(const Geometry &g, const double *track_row, int px, int py) {
    RowBoxes b;
    b.cam_x = (double)(px - g.cam_w / 2), b.cam_y = (double)(py - g.cam_h / 2);
    b.mic_x = (double)(px - g.mic_w / 2), b.mic_y = (double)(py - g.mic_h / 2);
    b.mic_w = (double)g.mic_w, b.mic_h = (double)g.mic_h;
    b.wx = (track_row[0] - b.cam_x) + b.cam_x, b.wy = (track_row[1] - b.cam_y) + b.cam_y, b.ww = track_row[2], b.wh = track_row[3];
    if (!(isfinite(b.wx) && isfinite(b.wy) && isfinite(b.ww) && isfinite(b.wh))) b.wx = b.wy = b.ww = b.wh = 0.0;
    return b;
}

// ErrorCalculator.calculate_bbox_error of a row: the share of the logged worm box outside the microscope box, 0 where the box has no area
__device__ __forceinline__ double row_bbox_error(const RowBoxes &b) {
    const double il = fmax(b.wx, b.mic_x), it = fmax(b.wy, b.mic_y);
    const double ir = fmin(b.wx + b.ww, b.mic_x + b.mic_w), ib = fmin(b.wy + b.wh, b.mic_y + b.mic_h);
    const double iw = fmax(0.0, ir - il), ih = fmax(0.0, ib - it);
    const double inter = iw * ih, total = b.ww * b.wh;
    return total == 0.0 ? 0.0 : 1.0 - inter / total;
}

// the refusals both entry points share; fills the geometry and the counts derived from it
inline int replay_check_config(const char *who, const wtk_replay_config *cfg, int32_t kind, int32_t E, int32_t n_cycles, int32_t n_track, Geometry &g, int &n_log) {
    const std::string w(who);
    if (!cfg) return fail(w + ": null argument");
    if (kind < WTK_REPLAY_CSV || kind > WTK_REPLAY_MLP) return fail(w + ": unknown kind");
    if (E < 1) return fail(w + ": at least one experiment (E >= 1)");
    if (cfg->moving_frame_num < 1) return fail(w + ": moving_frame_num must be at least 1");
    if (cfg->imaging_frame_num < 1) return fail(w + ": imaging_frame_num must be at least 1");
    if (cfg->pred_frame_num > cfg->imaging_frame_num) return fail(w + ": pred_frame_num lies beyond imaging_frame_num");
    if (cfg->pred_frame_num < (kind == WTK_REPLAY_CSV ? 1 : 0)) return fail(w + ": pred_frame_num must be at least 1 for the CSV kind (the controller has not seen the decision frame yet)");
    if (cfg->num_frames < 1 || n_track < 0) return fail(w + ": negative size");
    if (cfg->cam_w < cfg->mic_w || cfg->cam_h < cfg->mic_h) return fail(w + ": the camera is smaller than the microscope");
    if (cfg->mic_w < 0 || cfg->mic_h < 0) return fail(w + ": negative microscope size");
    if (cfg->frame_w < 1 || cfg->frame_h < 1) return fail(w + ": empty frame");
    const long long L = (long long)cfg->imaging_frame_num + cfg->moving_frame_num;
    if (L > INT32_MAX) return fail(w + ": cycle too long");
    n_log = (int)((cfg->num_frames - 1) / L); // the last cycle is never logged (its end never arrives)
    if ((long long)n_log * L > n_track) return fail(w + ": the track is shorter than the logged rows");
    if (n_cycles < 1 || n_cycles < n_log) return fail(w + ": n_cycles must cover every logged cycle (and be at least 1)");
    if ((long long)(n_cycles - 1) * L + cfg->imaging_frame_num > (long long)cfg->num_frames - 1)
        return fail(w + ": the decision frame of cycle n_cycles - 1 lies beyond the experiment's frames");
    g.L = (int)L, g.I = cfg->imaging_frame_num, g.M = cfg->moving_frame_num, g.P = cfg->pred_frame_num;
    g.cam_w = cfg->cam_w, g.cam_h = cfg->cam_h, g.mic_w = cfg->mic_w, g.mic_h = cfg->mic_h;
    g.x_max = cfg->frame_w - 1, g.y_max = cfg->frame_h - 1;
    return 0;
}

} // namespace wtk
