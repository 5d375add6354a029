"""TEST INFRASTRUCTURE: numpy restatement of replay_precise_kernel and its reduction (wtracker_amd/csrc/replay_precise.hip), and the
scenarios its tests share.

  precise(...)     per (experiment, frame): the padded table of the frame, two rectangle sums, the empty-intersection guard, the fallback rule
  summaries(...)   the six slots of WTK_REPLAY_PRECISE_SUMMARY_DOUBLES in the kernel's reduction order (replay_ref._tree_sum)
  composition(...) the route that existed before: replay_ref.rows -> eval_ref.precise on the rows' wrm / mic columns, one experiment at a time

It is pinned, not trusted: tests/test_replay_precise_ref.py holds precise() equal to composition(), counts and error bits, and to what the real
reference's ErrorCalculator.calculate_precise returned on replayed logs (tests/golden/replay_precise.npz)."""
from __future__ import annotations

import numpy as np

from . import eval_ref as ev
from . import replay_ref as rr

MAX_CELLS = 160 * 1024 // 4  # uint32 cells of the largest table (kPreciseMaxCells)


def threshold_int(t: float) -> int:
    """|frame - bg| > t on integers 0 .. 255 (eval_device.h threshold_int)."""
    if np.isnan(t) or t >= 255.0:
        return 255
    if t < 0.0:
        return -1
    return int(np.floor(t))


def frame_positions(g: rr.Geometry, pos: np.ndarray, move: np.ndarray) -> np.ndarray:
    """The platform position at every logged frame's camera picture: float64 [R, E, 2] (frame_position of replay_device.h)."""
    L, R, E = g.L, g.n_log * g.L, pos.shape[1]
    share = rr.share_table(g.M)
    pmax = np.array([g.frame_wh[0] - 1, g.frame_wh[1] - 1], dtype=np.float64)
    out = np.empty((R, E, 2), dtype=np.float64)
    for r in range(R):
        c, step = divmod(r, L)
        p, mv, carry = pos[c].astype(np.float64), move[c].astype(np.float64), np.zeros((E, 2))
        for k in range(min(max(step - g.I, 0), g.M)):
            carry, p = rr._motor(share[k], mv, carry, p, pmax)
        out[r] = p
    return out


def logged_boxes(g: rr.Geometry, track_row: np.ndarray, p: np.ndarray):
    """(worm [E, 4], mic [E, 4]) float64 of one frame from the platform positions p [E, 2] (row_boxes of replay_device.h)."""
    cam = p - np.array([g.cam[0] // 2, g.cam[1] // 2], dtype=np.float64)
    mic_xy = p - np.array([g.mic[0] // 2, g.mic[1] // 2], dtype=np.float64)
    E = len(p)
    with np.errstate(invalid="ignore"):
        worm = np.stack([(track_row[0] - cam[:, 0]) + cam[:, 0], (track_row[1] - cam[:, 1]) + cam[:, 1], np.full(E, track_row[2]), np.full(E, track_row[3])], axis=1)
    worm[~np.isfinite(worm).all(axis=1)] = 0.0
    mic = np.concatenate([mic_xy, np.tile(np.array(g.mic, dtype=np.float64), (E, 1))], axis=1)
    return worm, mic


def _rect(S: np.ndarray, l: int, t: int, r: int, b: int) -> int:
    with np.errstate(over="ignore"):
        return int(np.uint32(S[b, r] - S[t, r] - S[b, l] + S[t, l]))


def precise(g: rr.Geometry, track: np.ndarray, pos: np.ndarray, move: np.ndarray, frames: np.ndarray, bg: np.ndarray, diff_thresh: float,
            max_cells: int = MAX_CELLS):
    """-> (err float64 [E, R], counts int32 [E, R, 2], stats): the kernel's formulation.  stats counts the pairs answered by the table, the pairs of
    frames without a table and the pairs that left the padded region."""
    (W, H), E, R = g.frame_wh, pos.shape[1], g.n_log * g.L
    thr = threshold_int(diff_thresh)
    bgi = np.asarray(bg).astype(np.int32)  # the reference's astype(np.int32): a floating background is truncated
    err = np.full((E, R), np.nan)
    counts = np.zeros((E, R, 2), dtype=np.int32)
    stats = dict(table=0, frame_walk=0, pair_walk=0)
    P = frame_positions(g, pos, move)
    for r in range(R):
        mask = np.abs(frames[r].astype(np.int32) - bgi) > thr
        x1, y1, x2, y2, legal = ev.discretize(track[r:r + 1], (H, W))
        pl = pt = pr = pb = 0
        if legal[0]:
            pl, pt, pr, pb = max(int(x1[0]) - 1, 0), max(int(y1[0]) - 1, 0), min(int(x2[0]) + 1, W), min(int(y2[0]) + 1, H)
        pw, ph = pr - pl, pb - pt
        table = bool(legal[0]) and (ph + 1) * ((pw + 1) | 1) <= max_cells
        if table:
            S = np.zeros((ph + 1, pw + 1), dtype=np.uint32)
            S[1:, 1:] = mask[pt:pb, pl:pr].astype(np.uint32).cumsum(axis=0, dtype=np.uint32).cumsum(axis=1, dtype=np.uint32)
        worm, mic = logged_boxes(g, track[r], P[r])
        wl, wt, wr, wb, wlegal = ev.discretize(worm, (H, W))
        ml, mt, mr, mb, _ = ev.discretize(mic, (H, W))
        for e in np.flatnonzero(wlegal):
            il, it = max(wl[e], ml[e]), max(wt[e], mt[e])
            ir, ib = il + max(0, min(wr[e], mr[e]) - il), it + max(0, min(wb[e], mb[e]) - it)
            if table and wl[e] >= pl and wt[e] >= pt and wr[e] <= pr and wb[e] <= pb:
                total = _rect(S, wl[e] - pl, wt[e] - pt, wr[e] - pl, wb[e] - pt)
                inside = _rect(S, il - pl, it - pt, ir - pl, ib - pt) if ir > il and ib > it else 0  # decided before any lookup
                stats["table"] += 1
            else:
                total = int(mask[wt[e]:wb[e], wl[e]:wr[e]].sum())
                inside = int(mask[it:ib, il:ir].sum())
                stats["pair_walk" if table else "frame_walk"] += 1
            counts[e, r] = total, inside
            err[e, r] = 0.0 if total == 0 else 1.0 - np.int64(inside) / np.int64(total)
    return err, counts, stats


def summaries(g: rr.Geometry, err: np.ndarray) -> np.ndarray:
    """[E, 6]: the slots of WTK_REPLAY_PRECISE_SUMMARY_DOUBLES; NaN rows enter no sum."""
    R = err.shape[1]
    cyc, step = np.divmod(np.arange(R), g.L)
    trimmed = (step < g.I) & (cyc != 0) & (cyc != g.n_log - 1)
    out = np.empty((err.shape[0], 6))
    for e, v in enumerate(err):
        has = ~np.isnan(v)
        with np.errstate(invalid="ignore"):
            out[e] = [rr._tree_sum(np.where(has, v, 0.0)), has.sum(), rr._tree_sum(np.where(has & trimmed, v, 0.0)), (has & trimmed).sum(), (v > 1e-7).sum(),
                      (~has).sum()]
    return out


def composition(g: rr.Geometry, track: np.ndarray, pos: np.ndarray, move: np.ndarray, frames: np.ndarray, bg: np.ndarray, diff_thresh: float, experiments=None):
    """The route of the parent commit: experiment by experiment the log rows, then the per-row precise error on their wrm / mic columns.
    -> {e: (err [R], counts [R, 2], rows [R, 16])}"""
    R = g.n_log * g.L
    out = {}
    for e in range(pos.shape[1]) if experiments is None else experiments:
        rows = rr.rows(g, track, pos, move, e, summaries=False)["rows"]
        err, counts = ev.precise(frames, bg, rows[:, 10:14], rows[:, 6:10], np.arange(R), diff_thresh)
        out[e] = (err, counts.astype(np.int32), rows)
    return out


# ------------------------------------------------------------------------------------------------- scenarios
def _jitter_targets(g: rr.Geometry, track: np.ndarray, E: int, rng, step: float):
    """OPTIMAL-kind targets [C, E, 2] whose jitter grows with e; every tenth cycle (at random) is invalid."""
    a0, v0 = rr.targets_optimal(g, track)
    C = g.n_cycles
    a = a0[:, None, :] + rng.standard_normal((C, E, 2)) * (np.arange(E)[None, :, None] * step)
    valid = (v0[:, None] * (rng.random((C, E)) >= 0.1)).astype(np.int32)
    return np.ascontiguousarray(a), np.ascontiguousarray(valid)


def _blocky_background(rng, H: int, W: int) -> np.ndarray:
    levels = np.array([90, 120, 150], dtype=np.uint8)
    blocks = rng.integers(0, 3, ((H + 15) // 16, (W + 15) // 16))
    return levels[np.kron(blocks, np.ones((16, 16), dtype=np.int64))[:H, :W]]


def _paint(rng, bg: np.ndarray, track: np.ndarray, n_frames: int, speckles: int = 40) -> np.ndarray:
    """Frames: the background, a dark ellipse in each finite track box and `speckles` bright pixels."""
    H, W = bg.shape
    yy, xx = np.mgrid[0:H, 0:W]
    frames = np.repeat(bg[None], n_frames, axis=0).copy()
    for f in range(n_frames):
        if f < len(track) and np.isfinite(track[f]).all() and track[f, 2] > 0 and track[f, 3] > 0:
            x, y, w, h = track[f]
            shrink = rng.uniform(0.25, 0.5)
            inside = ((xx - (x + w / 2)) / (w * shrink)) ** 2 + ((yy - (y + h / 2)) / (h * shrink)) ** 2 < 1
            frames[f][inside] = 30
        frames[f][rng.integers(0, H, speckles), rng.integers(0, W, speckles)] = 250
    return frames


def scenario_main(seed: int = 5, E: int = 70) -> dict:
    """96 x 131 frames, camera (40, 32), microscope (14, 10), I = 4, M = 2, P = 1, 121 frames (R = 120), init (30, 30): a drifting fractional track of
    14-26 x 9-19 px boxes with NaN rows, a zero-area row, a 1 x 1 crop, a box clipped at the left edge and one at the bottom-right corner; a three-level
    blocky background, a dark ellipse in each box, 40 bright speckles per frame, one frame equal to the background; E jittered OPTIMAL targets."""
    rng = np.random.default_rng(seed)
    H, W, F = 96, 131, 121
    g = rr.Geometry(F, 4, 2, 1, (40, 32), (14, 10), (W, H), (30, 30))
    t = np.arange(F)
    track = np.stack([22 + 0.61 * t + 3 * np.sin(t / 5.0) + rng.uniform(0, 1, F), 24 + 0.33 * t + 2 * np.cos(t / 7.0) + rng.uniform(0, 1, F),
                      rng.uniform(14, 26, F), rng.uniform(9, 19, F)], axis=1)
    track[[7, 8, 40, 77]] = np.nan
    track[13, 0] = np.nan
    track[21] = [50.0, 31.0, 0.0, 12.0]          # no area
    track[33] = [70.3, 40.7, 0.4, 0.2]           # a 1 x 1 crop
    track[45] = [-6.4, 50.2, 19.3, 13.7]         # clipped at the left edge
    track[101] = [118.6, 84.3, 21.9, 17.2]       # clipped at the bottom-right corner
    bg = _blocky_background(rng, H, W)
    frames = _paint(rng, bg, track, F)
    frames[58] = bg
    a, valid = _jitter_targets(g, track, E, rng, 0.12)
    return dict(g=g, track=track, frames=frames, bg=bg, a=a, valid=valid, E=E, frame_shape=(H, W))


ULP_GROW = (float.fromhex("0x1.8000000000003p+2"), float.fromhex("0x1.1ffffffffffffp+3"))  # with cam = -9 the logged box ends one pixel later
ULP_SHRINK = float.fromhex("0x1.7ffffffffffffp+1")                                          # with cam = -4 the logged box starts one pixel later


def scenario_ulp(seed: int = 9) -> dict:
    """48 x 64 noise frames near the frame's corner (init (11, 8): cam = (-9, -8)), three experiments: e = 0 stays (cam_x = -9), e = 1 moves to x = 16
    in cycle 0 (cam_x = -4 from cycle 1 on), e = 2 moves to (20, 16) (cam = 0: the logged box is the track's).  The rows are the two examples of
    DESIGN.md section 19 on x, and on y with cam_y = -8 the same values shifted by one."""
    rng = np.random.default_rng(seed)
    H, W, F = 48, 64, 25
    g = rr.Geometry(F, 4, 2, 1, (40, 32), (14, 10), (W, H), (11, 8))
    track = np.empty((F, 4))
    for r in range(F):
        if r % 2 == 0:
            track[r] = [ULP_GROW[0], 5.25 + 0.5 * (r % 5), ULP_GROW[1], 7.5]
        else:
            track[r] = [ULP_SHRINK, 4.75 + 0.5 * (r % 3), 9.25, 6.5]
    track[10] = [5.5, float.fromhex("0x1.4000000000003p+2"), 8.0, float.fromhex("0x1.1ffffffffffffp+3")]  # the grow example on y (y = 5 + 3 ulp, cam_y = -8)
    bg = np.full((H, W), 100, dtype=np.uint8)
    frames = rng.integers(0, 256, (F, H, W), dtype=np.uint8)
    C, E = g.n_cycles, 3
    a = np.empty((C, E, 2))
    a[:, 0], a[:, 1], a[:, 2] = (11.0, 8.0), (16.0, 8.0), (20.0, 16.0)
    return dict(g=g, track=track, frames=frames, bg=bg, a=a, valid=np.ones((C, E), dtype=np.int32), E=E, frame_shape=(H, W))


def scenario_long(seed: int = 3) -> dict:
    """4105 frames of 24 x 32 (R = 4104: the reduction crosses a chunk), camera (12, 10), microscope (6, 4), three experiments."""
    rng = np.random.default_rng(seed)
    H, W, F = 24, 32, 4105
    g = rr.Geometry(F, 4, 2, 1, (12, 10), (6, 4), (W, H), (10, 9))
    t = np.arange(F)
    track = np.stack([10 + 8 * np.sin(t / 90.0) + rng.uniform(0, 1, F), 8 + 5 * np.cos(t / 70.0) + rng.uniform(0, 1, F), rng.uniform(5, 10, F),
                      rng.uniform(4, 8, F)], axis=1)
    track[rng.random(F) < 0.03] = np.nan
    bg = _blocky_background(rng, H, W)
    frames = _paint(rng, bg, track, F, speckles=6)
    a, valid = _jitter_targets(g, track, 3, rng, 1.5)
    return dict(g=g, track=track, frames=frames, bg=bg, a=a, valid=valid, E=3, frame_shape=(H, W))


def scenario_big_box(seed: int = 4) -> dict:
    """256 x 256 frames with a 210 x 210 box: its 213 x 213 table is beyond 160 KiB, so every pair walks its crop at the default limit too."""
    rng = np.random.default_rng(seed)
    H, W, F = 256, 256, 7
    g = rr.Geometry(F, 4, 2, 1, (40, 32), (14, 10), (W, H), (128, 128))
    track = np.tile(np.array([20.5, 22.25, 209.5, 209.25]), (F, 1)) + rng.uniform(0, 0.2, (F, 4))
    bg = _blocky_background(rng, H, W)
    frames = np.where(rng.random((F, H, W)) < 0.2, 250, bg[None]).astype(np.uint8)
    a, valid = _jitter_targets(g, track, 5, rng, 20.0)
    return dict(g=g, track=track, frames=frames, bg=bg, a=a, valid=valid, E=5, frame_shape=(H, W))


def scan_of(sc: dict, experiments=None):
    """(pos, move) [C, E', 2] of the scenario's OPTIMAL targets, for all or the named experiments."""
    a, valid = sc["a"], sc["valid"]
    if experiments is not None:
        a, valid = a[:, list(experiments)], valid[:, list(experiments)]
    return rr.scan(rr.OPTIMAL, sc["g"], sc["track"], a, None, valid, E=a.shape[1])
