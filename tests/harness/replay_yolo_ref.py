"""TEST INFRASTRUCTURE: numpy restatement of the YOLO controller's device loop (wtracker_amd/csrc/replay_yolo.hip: replay_yolo_step_kernel,
replay_yolo_positions_kernel, replay_yolo_track_kernel; wtracker_amd.replay.YoloReplay), driven by any `predict_views`-like callable.

  move_rule(row, cam)      HipYoloController.provide_movement_vector on a float32 row, every operation in the dtype numpy 2 gives it
  step(...)                the move + the cycle's motor steps (replay_ref's motor)
  frame_positions(...)     the platform position at every logged frame's camera picture
  track(...)               view-pixel detections -> the absolute float64 track, TrackLogger._write_rows' per-cycle dtype rule
  run(g, predict_views)    the whole experiment: phase 1 (one single-frame call per cycle), phase 2 (the log's detections in batches), rows

`predict_views(frame_numbers, positions) -> [n, 4]` xywh in view pixels with NaN rows for misses (any float dtype; the values are float32 numbers).

It is pinned, not trusted: tests/test_replay_yolo_ref.py holds it to the host loop (harness Simulator + TrackLogger + the oracle's YOLO controller), move for
move and row for row, at a threshold that keeps every detection and at one that makes some cycles miss."""
from __future__ import annotations

import numpy as np

from harness import replay_ref as rr

# The closed-loop fixture of tests/test_gpu_latency.py (synthetic "s" weights seed 0, synthetic_frames(40, 256, seed=8), imgsz 128), started at
# FIXTURE_INIT instead of (128, 128): from the centre the host run makes ONE non-zero move, from here three (on both axes).  The two thresholds are chosen
# from the confidences its host run logs (0.2058 .. 0.5395 at conf 0.1; tests/test_replay_yolo_ref.py asserts what each value is for):
#   FIXTURE_CONFS[0]  below every logged confidence: every detection is kept, moves (0, 1), (-3, 0), (0, 0), (-2, 0)
#   FIXTURE_CONFS[1]  between 0.2320 (cycle 0's decision view) and 0.2815 (the next one up): the first decision misses, so the move is (0, 0), the
#                     run takes another path, cycle 0 is logged with a NaN row (float64 sums) and cycles 1 .. 3 without one (float32 sums)
FIXTURE_INIT = (176, 116)
FIXTURE_CONFS = (0.1, 0.265)


def decision_offset(I: int, P: int) -> int:
    """Frame of the cycle whose view the controller decides on: its deque holds the cycle's frames 0 .. I at the decision and it reads entry [-P]."""
    return list(range(I + 1))[-P]


def move_rule(row, cam) -> tuple:
    """(0, 0) unless the row is finite; else per axis round_half_even(float32(float32(x + w / 2) - cam / 2))."""
    row = np.asarray(row, dtype=np.float32)
    if not np.isfinite(row).all():
        return 0, 0
    mid = row[:2] + row[2:] / np.float32(2)                      # float32
    d = mid - (np.asarray(cam, dtype=np.float64) / 2).astype(np.float32)  # the Python float is weak: the difference stays float32
    assert d.dtype == np.float32
    mv = rr._finish(d.astype(np.float64))
    return int(mv[0]), int(mv[1])


def step(g: rr.Geometry, share: np.ndarray, row, pos) -> tuple:
    """-> (move (2,), position at the next cycle's start (2,))."""
    mv = np.array(move_rule(row, g.cam), dtype=np.float64)
    p = np.array(pos, dtype=np.float64)
    pmax = np.array([g.frame_wh[0] - 1, g.frame_wh[1] - 1], dtype=np.float64)
    carry = np.zeros(2)
    for k in range(g.M):
        carry, p = rr._motor(share[k], mv, carry, p, pmax)
    return mv.astype(np.int32), p.astype(np.int32)


def frame_positions(g: rr.Geometry, pos: np.ndarray, move: np.ndarray) -> np.ndarray:
    """pos, move [C, 1, 2] -> int32 [R, 2]."""
    share = rr.share_table(g.M)
    R = g.n_log * g.L
    out = np.empty((R, 2), dtype=np.int32)
    pmax = np.array([g.frame_wh[0] - 1, g.frame_wh[1] - 1], dtype=np.float64)
    for r in range(R):
        c, s = divmod(r, g.L)
        p, mv, carry = pos[c, 0].astype(np.float64), move[c, 0].astype(np.float64), np.zeros(2)
        for k in range(min(max(s - g.I, 0), g.M)):
            carry, p = rr._motor(share[k], mv, carry, p, pmax)
        out[r] = p
    return out


def track(g: rr.Geometry, det: np.ndarray, frame_pos: np.ndarray) -> np.ndarray:
    """det float32 [R, 4] (NaN rows = misses), frame_pos int32 [R, 2] -> float64 [R, 4] absolute boxes."""
    det = np.asarray(det, dtype=np.float32)
    out = np.full(det.shape, np.nan, dtype=np.float64)
    corner = (frame_pos.astype(np.int64) - np.array([g.cam[0] // 2, g.cam[1] // 2])).astype(np.int64)
    for c in range(g.n_log):
        sl = slice(c * g.L, (c + 1) * g.L)
        ok = np.isfinite(det[sl]).all(axis=1)
        boxes = det[sl].astype(np.float32 if ok.all() else np.float64)  # one NaN row: numpy stacks the cycle as float64
        boxes[:, :2] = boxes[:, :2] + corner[sl].astype(boxes.dtype)    # a sum in the array's own dtype
        boxes[~ok] = np.nan
        out[sl] = boxes
    return out


def run(g: rr.Geometry, predict_views, log_batch=None) -> dict:
    """The whole experiment.  -> moves, positions [C, 1, 2] int32, frame_pos [R, 2], detections float32 [R, 4], track float64 [R, 4] and replay_ref.rows'
    dictionary (rows, bbox_error, mse_error, summary)."""
    C, L, R = g.n_cycles, g.L, g.n_log * g.L
    share = rr.share_table(g.M)
    pos, move = np.zeros((C, 1, 2), dtype=np.int32), np.zeros((C, 1, 2), dtype=np.int32)
    pos[0, 0] = (min(max(g.init[0], 0), g.frame_wh[0] - 1), min(max(g.init[1], 0), g.frame_wh[1] - 1))
    off = decision_offset(g.I, g.P)
    for c in range(C):
        row = np.asarray(predict_views([c * L + off], [tuple(int(v) for v in pos[c, 0])]))[0]
        move[c, 0], nxt = step(g, share, row, pos[c, 0])
        if c + 1 < C:
            pos[c + 1, 0] = nxt
    fpos = frame_positions(g, pos, move)
    det = np.empty((R, 4), dtype=np.float32)
    n = L if log_batch is None else int(log_batch)
    for r0 in range(0, R, n):
        r1 = min(r0 + n, R)
        det[r0:r1] = np.asarray(predict_views(list(range(r0, r1)), [tuple(int(v) for v in p) for p in fpos[r0:r1]]))
    trk = track(g, det, fpos)
    res = rr.rows(g, trk, pos, move)
    res.update(moves=move, positions=pos, frame_pos=fpos, detections=det, track=trk)
    return res
