"""TEST INFRASTRUCTURE: numpy restatement of the precise error of a population on a SET of tracks (the replay_set_precise kernels of
wtracker_amd/csrc/replay_set.hip), and the one scene its tests share.  Built on harness.replay_precise_ref (the per-track
yardstick: precise / summaries on one track alone) and harness.replay_set_ref (the super-track), which it imports and never edits.

  scene(E, which)        four tracks of different frame shapes with their frames, backgrounds and jittered OPTIMAL targets in the super-track's slices
  set_precise(...)       the set form: a global logged row -> its track by a search on row0 -> that track's view, frames, (H, W) and threshold -> the
                         row's pairs; every experiment of a row at once, from the integral image of the row's mask (the counts of a rectangle do not
                         depend on how they are taken: table and walk are the per-track harness's and the device's business)
  set_summaries(...)     the reduction: a block per (experiment, global chunk), chunks numbered through chunk0, the chunk's track found by a search,
                         the track's own trimmed rows; the finish: per-track sums of the chunk partials in index order, pooled in track order from 0.0
  objective(...)         one division of the pooled slots, or of each track's

`defect` plants one of the mistakes the layout invites (tests/test_replay_set_precise_ref.py shows that each is caught):
  "frames_track0"   every row reads track 0's frames and background
  "hw_track0"       every box is discretised against track 0's (H, W)
  "global_row"      the global row is used as the track's row
  "trim_set"        only the set's first and last logged cycle are trimmed, not every track's
  "mean_of_means"   the pooled objective is the mean of the tracks' means"""
from __future__ import annotations

import functools

import numpy as np

from harness import eval_ref as ev
from harness import replay_precise_ref as pr
from harness import replay_ref as rr
from harness import replay_set_ref as rs_ref

DEFECTS = ("frames_track0", "hw_track0", "global_row", "trim_set", "mean_of_means")
ROW_CHUNK = 4096
REACH = 64  # ReplaySet's default reach for this timing: max(64, L + I)
OBJECTIVE_SLOTS = {"trimmed_precise_error": (2, 3), "precise_error": (0, 1), "precise_non_perfect": (4, 1)}
THRESHOLDS = [20, 35, 20, 5]


# ------------------------------------------------------------------------------------------------- the scene
def _track_main(E: int) -> dict:
    return pr.scenario_main(E=E)


def _track_ulp(E: int) -> dict:
    """scenario_ulp with E experiments: its three constant targets first (the grow and shrink rows need them), jittered ones behind."""
    sc = pr.scenario_ulp()
    a, valid = pr._jitter_targets(sc["g"], sc["track"], E, np.random.default_rng(19), 0.2)
    n = min(3, E)
    a[:, :n], valid[:, :n] = sc["a"][:, :n], sc["valid"][:, :n]
    return dict(sc, a=a, valid=valid, E=E)


def _track_big_box(E: int) -> dict:
    """scenario_big_box's recipe with 19 frames: n_log = 3 (the least the trimmed objective admits), R = 18, a 213 x 213 table."""
    rng = np.random.default_rng(4)
    H, W, F = 256, 256, 19
    g = rr.Geometry(F, 4, 2, 1, (40, 32), (14, 10), (W, H), (128, 128))
    track = np.tile(np.array([20.5, 22.25, 209.5, 209.25]), (F, 1)) + rng.uniform(0, 0.2, (F, 4))
    bg = pr._blocky_background(rng, H, W)
    frames = np.where(rng.random((F, H, W)) < 0.2, 250, bg[None]).astype(np.uint8)
    a, valid = pr._jitter_targets(g, track, E, rng, 2.0)
    return dict(g=g, track=track, frames=frames, bg=bg, a=a, valid=valid, E=E, frame_shape=(H, W))


def _track_long(E: int) -> dict:
    """scenario_long's recipe on 48 x 64 frames with the scene's camera: 4105 frames, R = 4104 (two reduction chunks inside one track), 3 % NaN rows."""
    rng = np.random.default_rng(3)
    H, W, F = 48, 64, 4105
    g = rr.Geometry(F, 4, 2, 1, (40, 32), (14, 10), (W, H), (30, 22))
    t = np.arange(F)
    track = np.stack([26 + 16 * np.sin(t / 90.0) + rng.uniform(0, 1, F), 20 + 10 * np.cos(t / 70.0) + rng.uniform(0, 1, F), rng.uniform(5, 10, F),
                      rng.uniform(4, 8, F)], axis=1)
    track[rng.random(F) < 0.03] = np.nan
    bg = pr._blocky_background(rng, H, W)
    frames = pr._paint(rng, bg, track, F, speckles=6)
    a, valid = pr._jitter_targets(g, track, E, rng, 0.05)
    return dict(g=g, track=track, frames=frames, bg=bg, a=a, valid=valid, E=E, frame_shape=(H, W))


_MAKERS = (_track_main, _track_ulp, _track_big_box, _track_long)


@functools.lru_cache(maxsize=None)
def _track(i: int, E: int) -> dict:
    """Track i of the four with E experiments: built once and shared by every scene that holds it (nobody modifies it)."""
    return _MAKERS[i](E)


def scene(E: int = 70, which=(0, 1, 2, 3), thresholds=None) -> dict:
    """The tracks `which` of the four (in that order) as one set: per-track scenario dicts, the super-track, the targets [n_super_cycles, E, ...] with
    every track's targets in its slice (cycles of no track are invalid), the tables row0 / chunk0."""
    tracks = [_track(i, E) for i in which]
    geoms = [sc["g"] for sc in tracks]
    assert all((g.I, g.M, g.P, g.cam, g.mic) == (4, 2, 1, (40, 32), (14, 10)) for g in geoms)
    st = rs_ref.super_track([sc["track"] for sc in tracks], geoms, REACH)
    a = np.zeros((st.n_cycles, E, 2))
    valid = np.zeros((st.n_cycles, E), dtype=np.int32)
    for sc, off in zip(tracks, st.cyc_off):
        a[off:off + sc["g"].n_cycles], valid[off:off + sc["g"].n_cycles] = sc["a"], sc["valid"]
    R = [g.n_log * g.L for g in geoms]
    thr = [20] * len(tracks) if thresholds is None else list(thresholds)
    return dict(tracks=tracks, geoms=geoms, st=st, a=a, valid=valid, E=E, R=R, thr=thr, row0=np.concatenate([[0], np.cumsum(R)]).astype(np.int64),
                chunk0=np.concatenate([[0], np.cumsum([-(-r // ROW_CHUNK) for r in R])]).astype(np.int64))


def scan_of(sn: dict, experiments=None):
    """(pos, move) [n_super_cycles, E', 2] of the scene's targets, for all or the named experiments (replay_set_ref.set_scan)."""
    a, valid = sn["a"], sn["valid"]
    if experiments is not None:
        a, valid = a[:, list(experiments)], valid[:, list(experiments)]
    return rs_ref.set_scan(rr.OPTIMAL, sn["st"], [sc["track"] for sc in sn["tracks"]], sn["geoms"], a, None, valid, E=a.shape[1])


def track_alone(sn: dict, t: int, pos, move):
    """The per-track yardstick: replay_precise_ref.precise / summaries on track t alone, from the track's slice of the set's scan.
    -> dict(err [E, R_t], counts [E, R_t, 2], stats, summary [E, 6])"""
    sc, g, off = sn["tracks"][t], sn["geoms"][t], sn["st"].cyc_off[t]
    err, counts, stats = pr.precise(g, sc["track"], pos[off:off + g.n_cycles], move[off:off + g.n_cycles], sc["frames"], sc["bg"], sn["thr"][t])
    return dict(err=err, counts=counts, stats=stats, summary=pr.summaries(g, err))


# ------------------------------------------------------------------------------------------------- the set form
def _row_pairs(g: rr.Geometry, track_row, P_r, frame, bg, thr: int, HW):
    """Every experiment of one logged frame: (err [E], counts [E, 2]) from the integral image of the frame's mask."""
    H, W = HW
    mask = np.abs(frame.astype(np.int32) - np.asarray(bg).astype(np.int32)) > thr
    S = np.zeros((mask.shape[0] + 1, mask.shape[1] + 1), dtype=np.int64)
    S[1:, 1:] = mask.cumsum(axis=0).cumsum(axis=1)
    worm, mic = pr.logged_boxes(g, track_row, P_r)
    wl, wt, wr, wb, legal = ev.discretize(worm, (H, W))
    ml, mt, mr, mb, _ = ev.discretize(mic, (H, W))
    il, it = np.maximum(wl, ml), np.maximum(wt, mt)
    ir, ib = il + np.maximum(0, np.minimum(wr, mr) - il), it + np.maximum(0, np.minimum(wb, mb) - it)
    cx, cy = (lambda v: np.minimum(v, mask.shape[1])), (lambda v: np.minimum(v, mask.shape[0]))  # (only a planted defect indexes beyond the mask)

    def rect(l, t, r, b):
        l, t, r, b = cx(l), cy(t), cx(r), cy(b)
        return S[b, r] - S[t, r] - S[b, l] + S[t, l]

    total, inside = rect(wl, wt, wr, wb), rect(il, it, ir, ib)
    total, inside = np.where(legal, total, 0), np.where(legal, inside, 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.where(legal, np.where(total == 0, 0.0, 1.0 - inside / np.where(total == 0, 1, total)), np.nan)
    return err, np.stack([total, inside], axis=1).astype(np.int32)


def set_precise(sn: dict, pos, move, defect=None):
    """-> (err [E, sum R], counts [E, sum R, 2]): one step per GLOBAL logged row, as one workgroup of replay_set_precise_kernel."""
    E, row0, T = pos.shape[1], sn["row0"], len(sn["tracks"])
    rows = int(row0[-1])
    err, counts = np.full((E, rows), np.nan), np.zeros((E, rows, 2), dtype=np.int32)
    views = []
    for t in range(T):  # the track's view: its slice of the scan, its own clamp and counts
        g, off = sn["geoms"][t], sn["st"].cyc_off[t]
        views.append(pr.frame_positions(g, pos[off:off + g.n_cycles], move[off:off + g.n_cycles]))
    for rho in range(rows):
        t = int(np.searchsorted(row0, rho, side="right")) - 1  # the last track whose row0 <= rho
        sc, g = sn["tracks"][t], sn["geoms"][t]
        r = rho - int(row0[t])
        src = sn["tracks"][0] if defect == "frames_track0" else sc
        frame, bg = src["frames"][r % len(src["frames"])], src["bg"]
        if defect == "frames_track0":  # (cut or pad to the track's own shape: the defect is the content, not a crash)
            H, W = sc["frame_shape"]
            pad = lambda x: np.pad(x, ((0, max(0, H - x.shape[0])), (0, max(0, W - x.shape[1]))))[:H, :W]  # noqa: E731
            frame, bg = pad(frame), pad(bg)
        HW = sn["tracks"][0]["frame_shape"] if defect == "hw_track0" else sc["frame_shape"]
        tr = rho % len(sc["track"]) if defect == "global_row" else r
        err[:, rho], counts[:, rho] = _row_pairs(g, sc["track"][tr], views[t][r], frame, bg, pr.threshold_int(sn["thr"][t]), HW)
    return err, counts


def set_summaries(sn: dict, err, defect=None):
    """-> (track_summary [T, E, 6], summary [E, 6]) of err [E, sum R]: the reduce launch and the finish launch."""
    T, E, row0, chunk0 = len(sn["tracks"]), err.shape[0], sn["row0"], sn["chunk0"]
    S = int(chunk0[-1])
    partial = np.zeros((E, S, 6))
    logged = [t for t in range(T) if sn["geoms"][t].n_log > 0]
    for gs in range(S):
        t = int(np.searchsorted(chunk0[:-1], gs, side="right")) - 1  # the last track whose chunk0 <= gs
        while sn["R"][t] == 0:
            t -= 1
        g = sn["geoms"][t]
        r = np.arange((gs - int(chunk0[t])) * ROW_CHUNK, min((gs - int(chunk0[t]) + 1) * ROW_CHUNK, sn["R"][t]))
        cyc, step = np.divmod(r, g.L)
        if defect == "trim_set":
            trimmed = (step < g.I) & ~((t == logged[0]) & (cyc == 0)) & ~((t == logged[-1]) & (cyc == g.n_log - 1))
        else:
            trimmed = (step < g.I) & (cyc != 0) & (cyc != g.n_log - 1)  # the track's own n_log
        for e in range(E):
            v = err[e, int(row0[t]) + r]
            has = ~np.isnan(v)
            with np.errstate(invalid="ignore"):
                partial[e, gs] = [rr._tree_sum(np.where(has, v, 0.0)), has.sum(), rr._tree_sum(np.where(has & trimmed, v, 0.0)), (has & trimmed).sum(),
                                  (v > 1e-7).sum(), (~has).sum()]
    ts = np.zeros((T, E, 6))
    pooled = np.zeros((E, 6))
    for t in range(T):
        for s in range(int(chunk0[t]), int(chunk0[t + 1])):
            ts[t] = ts[t] + partial[:, s]
        pooled = pooled + ts[t]
    return ts, pooled


def objective(ts, pooled, kind: str, per_track: bool = False, defect=None):
    num, den = OBJECTIVE_SLOTS[kind]
    with np.errstate(invalid="ignore", divide="ignore"):
        if per_track:
            return ts[:, :, num] / ts[:, :, den]
        if defect == "mean_of_means":
            return (ts[:, :, num] / ts[:, :, den]).mean(axis=0)
        return pooled[:, num] / pooled[:, den]
