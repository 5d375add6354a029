"""TEST INFRASTRUCTURE: numpy statement of the class grouping behind wtk_replay_polyfit_targets (wtracker_amd/csrc/replay_targets.hip).

The least-squares problem of a cycle's fit is `A c = diag(w) y` with `A = diag(w) V(t) / scl` over the samples of the cycle that exist (inside the track,
finite centre): `A` depends on the weights and on WHICH samples exist, never on the centres.  So the cycles of a track fall into classes by that set,
a bit mask over the sorted sample times, and one decomposition per class serves all its cycles.

  class_table(...)             cycle -> class and class -> mask, stated with plain loops (the product derives it vectorised: wtracker_amd.replay.polyfit_classes)
  targets_polyfit_grouped(...) numpy's polyfit called ONCE per class with the centres of all its cycles as right-hand sides, then polyval
  condition(...)               the effective condition number of a class's scaled matrix (numpy's rcond cut applied): the scale of the rounding difference
                               between one solve with many right-hand sides and one solve per cycle

tests/test_replay_opt_ref.py holds the grouped targets to replay_ref.targets_polyfit (one numpy fit per cycle, itself pinned to the real reference)."""
from __future__ import annotations

import warnings

import numpy as np
from numpy.polynomial import polynomial as poly

from . import replay_ref as rr


def class_table(track: np.ndarray, L: int, n_cycles: int, sample_times) -> tuple:
    """-> (cycle_class [n_cycles], class_mask [K]); bit j of a mask: frame c L + sorted(sample_times)[j] is inside the track and its centre is finite.
    Classes are numbered by ascending mask."""
    st = sorted(int(t) for t in sample_times)
    masks = []
    for c in range(n_cycles):
        m = 0
        for j, t in enumerate(st):
            f = c * L + t
            if 0 <= f < len(track):
                x, y, w, h = (float(v) for v in track[f])
                if np.isfinite(x + w / 2) and np.isfinite(y + h / 2):
                    m |= 1 << j
        masks.append(m)
    class_mask = sorted(set(masks))
    index = {m: k for k, m in enumerate(class_mask)}
    return np.array([index[m] for m in masks], dtype=np.int32), np.array(class_mask, dtype=np.int32)


def _kept(mask: int, n: int) -> np.ndarray:
    return np.array([(mask >> j) & 1 for j in range(n)], dtype=bool)


def targets_polyfit_grouped(g: rr.Geometry, track: np.ndarray, degree: int, sample_times, weights=None, n_cycles=None):
    """replay_ref.targets_polyfit with one numpy fit per CLASS: -> (a [C, 2], valid [C])."""
    C = g.n_cycles if n_cycles is None else n_cycles
    st = np.array(sorted(sample_times), dtype=int)
    wt = np.ones(len(st)) if weights is None else np.asarray(weights, dtype=float)
    cycle_class, class_mask = class_table(track, g.L, C, st)
    a, v = np.zeros((C, 2)), np.zeros(C, dtype=np.int32)
    for k, mask in enumerate(class_mask):
        ok = _kept(int(mask), len(st))
        cycles = np.nonzero(cycle_class == k)[0]
        if not ok.any():
            continue  # no sample: valid = 0, target 0
        frames = cycles[:, None] * g.L + st[ok][None, :]  # [cycles, n]: all inside the track by the mask
        cen = rr._centers(track[frames.reshape(-1)]).reshape(len(cycles), int(ok.sum()), 2)
        rhs = cen.transpose(1, 0, 2).reshape(int(ok.sum()), -1)  # [n, 2 cycles]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            co = poly.polyfit(st[ok], rhs, deg=degree, w=wt[ok])
        a[cycles], v[cycles] = poly.polyval(g.L + g.I // 2, co).reshape(len(cycles), 2), 1
    return a, v


def condition(mask: int, degree: int, sample_times, weights=None) -> float:
    """s_max / (smallest singular value numpy keeps) of diag(w) V(t) / scl over the samples of `mask`; 1 for an empty class."""
    st = np.array(sorted(sample_times), dtype=float)
    wt = np.ones(len(st)) if weights is None else np.asarray(weights, dtype=float)
    ok = _kept(int(mask), len(st))
    if not ok.any():
        return 1.0
    A = poly.polyvander(st[ok], degree) * wt[ok][:, None]
    scl = np.sqrt((A * A).sum(axis=0))
    scl[scl == 0] = 1
    s = np.linalg.svd(A / scl, compute_uv=False)
    kept = s[s > ok.sum() * np.finfo(float).eps * s.max()]
    return float(s.max() / kept.min()) if len(kept) else 1.0


def log_bbox_error(rows: list) -> np.ndarray:
    """ErrorCalculator.calculate_bbox_error of every row of a TrackLogger log (dictionaries with sim.LOG_COLUMNS), in the reference's operation order
    (replay_ref.rows states the same expression; tests/test_replay_ref.py pins it to the reference bit for bit)."""
    wx, wy, ww, wh = (np.array([float(r[k]) for r in rows]) for k in ("wrm_x", "wrm_y", "wrm_w", "wrm_h"))
    mx, my, mw, mh = (np.array([float(r[k]) for r in rows]) for k in ("mic_x", "mic_y", "mic_w", "mic_h"))
    iw = np.maximum(0.0, np.minimum(wx + ww, mx + mw) - np.maximum(wx, mx))
    ih = np.maximum(0.0, np.minimum(wy + wh, my + mh) - np.maximum(wy, my))
    total = ww * wh
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(total == 0, 0.0, 1.0 - (iw * ih) / total)


def kept_rows(rows: list) -> np.ndarray:
    """DataAnalyzer.clean(trim_cycles=True, imaging_only=True): imaging rows, without cycle 0 and the last logged cycle."""
    cycle = np.array([int(r["cycle"]) for r in rows])
    imaging = np.array([r["phase"] == "imaging" for r in rows])
    last = cycle[imaging].max()
    return imaging & (cycle != 0) & (cycle != last)
