"""TEST INFRASTRUCTURE: float64 numpy restatement of the two replay kernels (wtracker_amd/csrc/replay.hip) and of the per-cycle targets they are fed.

  scan(...)   replay_scan_kernel: per experiment, sequentially over cycles, the move from the kind's expression and the motor's M steps
  rows(...)   replay_rows_kernel + the finish launch: log rows, per-row bbox / MSE error, per-experiment summaries in the kernel's reduction order
  targets_*   what wtracker_amd.replay's builders compute on the device (medians, numpy polyfit, the oracle ResMLP)

It is pinned, not trusted: tests/test_replay_ref.py holds it to every row and move the real reference wrote (tests/golden/sim_*_bboxes.csv, sim_moves.json,
polyfit_cases.json, polyfit_highdeg.json, replay_hard.npz).  The GPU tests then hold the kernels to it and to those fixtures."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

CSV, OPTIMAL, POLYFIT, MLP = 0, 1, 2, 3
ROW_CHUNK, ROW_THREADS = 4096, 256  # kRowChunk, kRowThreads
ROW_COLUMNS = ["plt_x", "plt_y", "cam_x", "cam_y", "cam_w", "cam_h", "mic_x", "mic_y", "mic_w", "mic_h", "wrm_x", "wrm_y", "wrm_w", "wrm_h", "cycle", "phase"]


@dataclass
class Geometry:
    num_frames: int
    I: int
    M: int
    P: int
    cam: tuple   # (w, h)
    mic: tuple
    frame_wh: tuple  # (W, H): the position is clamped to [0, W - 1] x [0, H - 1]
    init: tuple

    @property
    def L(self) -> int:
        return self.I + self.M

    @property
    def n_log(self) -> int:
        return (self.num_frames - 1) // self.L

    @property
    def n_cycles(self) -> int:
        return (self.num_frames - 1 - self.I) // self.L + 1

    @classmethod
    def of(cls, timing_config, experiment_config, frame_shape=None) -> "Geometry":
        tc, ec = timing_config, experiment_config
        cam = tuple(int(v) for v in tc.camera_size_px)
        if frame_shape is None:  # DummyReader's resolution: orig_resolution + camera_size // 2 * 2, element by element
            frame_shape = tuple(a + b for a, b in zip(ec.orig_resolution, (cam[0] // 2 * 2, cam[1] // 2 * 2)))
        return cls(int(ec.num_frames), int(tc.imaging_frame_num), int(tc.moving_frame_num), int(tc.pred_frame_num), cam,
                   tuple(int(v) for v in tc.micro_size_px), (int(frame_shape[1]), int(frame_shape[0])), tuple(int(v) for v in ec.init_position))


def share_table(M: int) -> np.ndarray:
    """SineMotorController's profile, with numpy's cos as the reference computes it."""
    return np.array([(np.cos((k * np.pi) / M) - np.cos(((k + 1) * np.pi) / M)) / 2 for k in range(M)], dtype=np.float64)


def _motor(share, mv, carry, pos, pos_max):
    want = share * mv + carry
    took = np.rint(want)
    return want - took, np.clip(pos + took, 0, pos_max)


def _finish(v):
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(v), np.clip(np.rint(v), -2.0 ** 30, 2.0 ** 30), 0.0)


def scan(kind: int, g: Geometry, track: np.ndarray, a=None, b=None, valid=None, E: int = 1, n_cycles=None):
    """-> (pos [C, E, 2] int32 at cycle start, move [C, E, 2] int32).  a, b [C, E, 2] float64, valid [C, E]."""
    C = g.n_cycles if n_cycles is None else n_cycles
    share = share_table(g.M)
    pos = np.empty((C, E, 2), dtype=np.int32)
    move = np.empty((C, E, 2), dtype=np.int32)
    p = np.empty((E, 2), dtype=np.float64)
    p[:, 0] = min(max(g.init[0], 0), g.frame_wh[0] - 1)
    p[:, 1] = min(max(g.init[1], 0), g.frame_wh[1] - 1)
    cam_size = np.array(g.cam, dtype=np.float64)
    half = cam_size / 2
    pmax = np.array([g.frame_wh[0] - 1, g.frame_wh[1] - 1], dtype=np.float64)
    for c in range(C):
        pos[c] = p
        cam = p - np.array([g.cam[0] // 2, g.cam[1] // 2])
        mv = np.zeros((E, 2))
        if kind == CSV:
            f = c * g.L + g.I - g.P
            if 0 <= f < len(track) and np.isfinite(track[f]).all():
                xy, wh = track[f, :2], track[f, 2:]
                mv = _finish(((xy - cam) + wh / 2) - half)
        else:
            if kind == OPTIMAL:
                v = a[c] - (cam + half)
            elif kind == POLYFIT:
                v = (a[c] - cam) - half
            else:
                v = a[c] + (b[c] - (cam + half))
            mv = np.where(np.asarray(valid[c], dtype=bool)[:, None], _finish(v), 0.0)
        move[c] = mv
        carry = np.zeros((E, 2))
        for k in range(g.M):
            carry, p = _motor(share[k], mv, carry, p, pmax)
    return pos, move


def _tree_sum(values: np.ndarray) -> float:
    """The kernel's order: chunks of 4096 rows; in a chunk thread t adds rows t, t + 256, ... in order, then a binary tree over the 256 threads; the
    chunk partials are added in index order."""
    total = 0.0
    for s in range(0, len(values), ROW_CHUNK):
        chunk = np.zeros(ROW_CHUNK)
        chunk[: len(values[s : s + ROW_CHUNK])] = values[s : s + ROW_CHUNK]
        lanes = np.zeros(ROW_THREADS)
        for i in range(ROW_CHUNK // ROW_THREADS):
            lanes = lanes + chunk[i * ROW_THREADS : (i + 1) * ROW_THREADS]
        half = ROW_THREADS // 2
        while half > 0:
            lanes[:half] = lanes[:half] + lanes[half : 2 * half]
            half //= 2
        total = total + lanes[0]
    return float(total)


def rows(g: Geometry, track: np.ndarray, pos: np.ndarray, move: np.ndarray, e: int = 0, summaries: bool = True) -> dict:
    """Experiment e's log: `rows` [R, 16] (ROW_COLUMNS), `bbox_error` [R], `mse_error` [R] and `summary` [6]."""
    L, R = g.L, g.n_log * g.L
    share = share_table(g.M)
    out = np.zeros((R, len(ROW_COLUMNS)), dtype=np.float64)
    pmax = np.array([g.frame_wh[0] - 1, g.frame_wh[1] - 1], dtype=np.float64)
    for r in range(R):
        c, step = divmod(r, L)
        p = pos[c, e].astype(np.float64)
        mv = move[c, e].astype(np.float64)
        carry = np.zeros(2)
        for k in range(min(max(step - g.I, 0), g.M)):
            carry, p = _motor(share[k], mv, carry, p, pmax)
        cam = p - np.array([g.cam[0] // 2, g.cam[1] // 2])
        mic = p - np.array([g.mic[0] // 2, g.mic[1] // 2])
        w = np.array([(track[r, 0] - cam[0]) + cam[0], (track[r, 1] - cam[1]) + cam[1], track[r, 2], track[r, 3]])
        if not np.isfinite(w).all():
            w[:] = 0.0
        out[r] = [p[0], p[1], cam[0], cam[1], g.cam[0], g.cam[1], mic[0], mic[1], g.mic[0], g.mic[1], w[0], w[1], w[2], w[3], c, 0.0 if step < g.I else 1.0]
    wx, wy, ww, wh = out[:, 10], out[:, 11], out[:, 12], out[:, 13]
    mx, my, mw, mh = out[:, 6], out[:, 7], out[:, 8], out[:, 9]
    iw = np.maximum(0.0, np.minimum(wx + ww, mx + mw) - np.maximum(wx, mx))
    ih = np.maximum(0.0, np.minimum(wy + wh, my + mh) - np.maximum(wy, my))
    total = ww * wh
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.where(total == 0, 0.0, 1.0 - (iw * ih) / total)
    dx, dy = (wx + ww / 2) - (mx + mw / 2), (wy + wh / 2) - (my + mh / 2)
    mse = (dx * dx + dy * dy) / 2
    res = dict(rows=out, bbox_error=err, mse_error=mse)
    if summaries:
        trimmed = (out[:, 15] == 0) & (out[:, 14] != 0) & (out[:, 14] != g.n_log - 1)
        res["summary"] = np.array([_tree_sum(err), float(R), _tree_sum(np.where(trimmed, err, 0.0)), float(trimmed.sum()), float((err > 1e-7).sum()),
                                   _tree_sum(mse)])
    return res


def long_track(F: int, period: int) -> np.ndarray:
    """A seeded head track [F, 4] with exact duplicates, NaN rows, and rows whose centre differs from the one `period` frames before by -1e-6, 0 and +1e-6
    (speeds that round to -0.0 and +0.0)."""
    rng = np.random.default_rng(77)
    pos = np.array([700.0, 600.0])
    heading = 0.3
    out = np.empty((F, 4))
    for i in range(F):
        heading += rng.normal(0.0, 0.15)
        pos = 300 + (pos + max(0.2, rng.normal(2.5, 1.0)) * np.array([math.cos(heading), math.sin(heading)]) - 300) % 800  # folded back: a few large jumps
        w, h = np.round(13.8 + rng.normal(0, 0.6), 1), np.round(14.6 + rng.normal(0, 0.6), 1)  # one decimal: widths and heights repeat
        out[i] = (pos[0] - w / 2, pos[1] - h / 2, w, h)
    for r0 in range(50, F - 40, 397):
        out[r0 + 1:r0 + 2 * period + 1] = out[r0]  # exact duplicates: zero speed, equal values in every column
        out[r0 + 20 + period] = out[r0 + 20] + (-1e-6, 1e-6, 0, 0)
    out[[11, 300, 301, 4100, F - 5]] = np.nan
    return out


# ------------------------------------------------------------------------------------------------- per-cycle targets (host)
def _table(track):
    return np.vstack([track, np.full((1, 4), np.nan)])


def _centers(boxes):
    return np.stack([boxes[:, 0] + boxes[:, 2] / 2, boxes[:, 1] + boxes[:, 3] / 2], axis=1)


def targets_optimal(g: Geometry, track: np.ndarray, n_cycles=None):
    """OptimalController: the median head centre of the NEXT cycle's imaging phase."""
    C = g.n_cycles if n_cycles is None else n_cycles
    cen = _centers(track)
    a, v = np.zeros((C, 2)), np.zeros(C, dtype=np.int32)
    for c in range(C):
        w = cen[(c + 1) * g.L : (c + 1) * g.L + g.I]
        w = w[np.isfinite(w).all(axis=1)]
        if len(w):
            a[c], v[c] = np.median(w, axis=0), 1
    return a, v


def targets_polyfit(g: Geometry, track: np.ndarray, degree: int, sample_times, weights=None, n_cycles=None):
    """PolyfitController on absolute centres (the fit commutes with the camera translation, as HipPolyfitController states)."""
    import warnings

    from numpy.polynomial import polynomial as poly

    C = g.n_cycles if n_cycles is None else n_cycles
    st = np.array(sorted(sample_times), dtype=int)  # the reference sorts the times, not the weights
    wt = np.ones(len(st)) if weights is None else np.asarray(weights, dtype=float)
    tab, N = _table(track), len(track)
    a, v = np.zeros((C, 2)), np.zeros(C, dtype=np.int32)
    for c in range(C):
        fr = c * g.L + st
        cen = _centers(tab[np.where((fr >= 0) & (fr < N), fr, N)])
        ok = np.isfinite(cen).all(axis=1)
        if ok.sum():
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                co = poly.polyfit(st[ok], cen[ok], deg=degree, w=wt[ok])
            a[c], v[c] = poly.polyval(g.L + g.I // 2, co), 1
    return a, v


def targets_mlp(g: Geometry, track: np.ndarray, state: dict, max_dist_per_pred: float, n_cycles=None):
    """MLPController up to the camera: (clipped float32 model output as float64, corner of the first input box, valid); `state`: oracle.resmlp_oracle.load_state."""
    from oracle import resmlp_oracle

    C = g.n_cycles if n_cycles is None else n_cycles
    tab, N = _table(track), len(track)
    a, b, v = np.zeros((C, 2)), np.zeros((C, 2)), np.zeros(C, dtype=np.int32)
    for c in range(C):
        fr = np.asarray(state["input_frames"], dtype=int) + (c * g.L + g.I - g.P)
        boxes = tab[np.where((fr >= 0) & (fr < N), fr, N)].reshape(1, -1).copy()
        if not np.isfinite(boxes).all():
            continue
        x0, y0 = boxes[0, 0], boxes[0, 1]
        boxes[:, 0::4] -= x0
        boxes[:, 1::4] -= y0
        pred = np.clip(resmlp_oracle.forward(state, boxes.astype(np.float32)).flatten(), -max_dist_per_pred, max_dist_per_pred)
        a[c], b[c], v[c] = (pred[0].item(), pred[1].item()), (x0, y0), 1
    return a, b, v


def max_dist_per_pred(timing_config, pred_frames, max_speed: float) -> float:
    return max_speed * (timing_config.px_per_mm / timing_config.frames_per_sec) * pred_frames[0]


def log_rows(res: dict) -> list:
    """rows() as the dictionaries TrackLogger keeps (sim.LOG_COLUMNS)."""
    out = []
    for r, v in enumerate(res["rows"]):
        d = dict(frame=r, cycle=int(v[14]), phase="imaging" if v[15] == 0 else "moving")
        for k, name in enumerate(ROW_COLUMNS[:10]):
            d[name] = int(v[k])
        for k, name in enumerate(ROW_COLUMNS[10:14]):
            d[name] = float(v[10 + k])
        out.append(d)
    return out
