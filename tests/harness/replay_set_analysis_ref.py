"""TEST INFRASTRUCTURE: float64 numpy restatement of the analysis of a population replayed on a SET of tracks (wtracker_amd/csrc/replay_set_analysis.hip,
DESIGN.md section 28), on top of harness.analysis_ref (one log) and harness.replay_set_ref / replay_ref (the logs themselves): what the reference's
Plotter computes from several logs at once (wtracker/eval/plotter.py:37-40).  Every log goes through analysis_ref.analyze on its own (its own frame
numbers, its own speed, its own last surviving cycle); the pooled statistics are taken over the concatenation of the cleaned logs in track order.

  the_scene(golden_dir)            the three tracks every test of the set analysis uses, their geometries and the CPU-replayed logs of csv, optimal, polyfit
  kernel_sum(values, use)          one track's sum in the per-track kernel's order: lane i adds the used rows i, i + 512, ... in order, then a binary tree
  pooled_describe(parts, q)        count, mean, std, min, percentiles, max of the union of the parts' used values: order statistics exact, the moments in
                                   the order the C header defines (sum_t chained over the tracks that keep a value, ss_t about the pooled mean)
  analyze_set(logs, L, spec)       dict(track=[analysis_ref.analyze(...)], pooled=dict(describe, step_quantiles, step_count, cycle_max, cycle_mean,
                                   anomaly_counts, anomaly_mask, stats, n_rows, values))

It is pinned, not trusted: tests/test_replay_set_analysis_ref.py holds it to tests/golden/analysis_set.npz, which the real DataAnalyzer, the real Plotter's
concatenation and pandas wrote.  `defect` plants one of the mistakes the set form invites (that test shows each is caught):
  "speed_across"         wrm_speed differenced across a track boundary (the first `period` rows of track t > 0 look back into track t - 1)
  "trim_set"             every log trimmed by the set's last surviving cycle instead of its own
  "mean_of_percentiles"  a pooled percentile taken as the mean of the per-track percentiles
  "std_per_track"        the pooled sum of squares taken about each track's own mean"""
from __future__ import annotations

import dataclasses
import json
import math
import os

import numpy as np

from harness import analysis_ref as ar
from harness import replay_ref as rr

DEFECTS = ("speed_across", "trim_set", "mean_of_percentiles", "std_per_track")
THREADS = 512  # kAnaThreads
TIMES, DEGREE = [-8, -6, -4, -2, 0, 1], 1  # the fixture's Polyfit experiment
KINDS = ("csv", "optimal", "polyfit")


def the_scene(golden_dir: str) -> dict:
    """Three deterministic tracks that share the L = 5 timing of replay_hard.npz's `_100` runs: the pinned hard track, its first 137 rows translated
    into a 400 x 300 frame, and replay_ref.long_track with 4125 logged rows.  -> dict(tracks, geoms, timing = (imaging, pred, moving) ms, meta,
    logs[kind][t] = rows16 [R_t, 16] of experiment `kind` replayed on track t by replay_ref (pinned to the reference's logs row for row))."""
    z = np.load(os.path.join(golden_dir, "replay_hard.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    geo = meta["geometry"]["100"]
    cam, mic = tuple(geo["camera_size_px"]), tuple(geo["micro_size_px"])
    I, M, P, L = geo["I"], geo["M"], geo["P"], geo["L"]
    res = tuple(meta["orig_resolution"])
    full = (res[1] + cam[1] // 2 * 2, res[0] + cam[0] // 2 * 2)  # (W, H) of the default frame: orig_resolution + camera_size // 2 * 2 is read as (H, W)
    tracks = [z["track"].copy(), z["track"][:137] + np.array([150.0, 250.0, 0.0, 0.0]), rr.long_track(4130, 5)]
    g0 = rr.Geometry(meta["num_frames"], I, M, P, cam, mic, full, tuple(meta["init_position"]))
    geoms = [g0, dataclasses.replace(g0, num_frames=137, frame_wh=(400, 300), init=(500, 120)),
             dataclasses.replace(g0, num_frames=4130, frame_wh=(1400, 1400), init=(700, 600))]
    assert L == 5 and [g.n_log * L for g in geoms] == [395, 135, 4125]
    logs = {k: [] for k in KINDS}
    for tr, g in zip(tracks, geoms):
        for kind in KINDS:
            if kind == "csv":
                pos, move = rr.scan(rr.CSV, g, tr)
            else:
                a, v = rr.targets_optimal(g, tr) if kind == "optimal" else rr.targets_polyfit(g, tr, DEGREE, TIMES)
                pos, move = rr.scan(rr.OPTIMAL if kind == "optimal" else rr.POLYFIT, g, tr, a[:, None], None, v[:, None])
            logs[kind].append(rr.rows(g, tr, pos, move, 0, summaries=False)["rows"])
    return dict(tracks=tracks, geoms=geoms, meta=meta, L=L, logs=logs)


def kernel_sum(values: np.ndarray, use: np.ndarray) -> float:
    """The sum of values[use] in the segment kernels' order: thread i of 512 adds the used rows i, i + 512, ... in order from 0.0, then a binary tree
    over the threads.  `values` holds the segment's rows in order, used or not."""
    n = -(-len(values) // THREADS) * THREADS
    v, u = np.zeros(n), np.zeros(n, dtype=bool)
    v[:len(values)], u[:len(values)] = values, use
    lanes = np.zeros(THREADS)
    for row, used in zip(v.reshape(-1, THREADS), u.reshape(-1, THREADS)):  # all lanes at once, each lane's rows in order
        with np.errstate(invalid="ignore"):
            lanes = lanes + np.where(used, row, 0.0)  # (a lane starts at +0.0 and never becomes -0.0: adding +0.0 for a skipped row changes no bit)
    half = THREADS // 2
    while half > 0:
        lanes[:half] = lanes[:half] + lanes[half:2 * half]
        half //= 2
    return float(lanes[0])


def pooled_describe(parts, percentiles, defect=None) -> np.ndarray:
    """[5 + Q] over the union of the parts' used values; `parts`: per track, in track order, (values of the segment's rows in order, use = kept and not NaN)."""
    Q = len(percentiles)
    out = np.full(5 + Q, np.nan)
    S, N = 0.0, 0
    for v, use in parts:
        n_t = int(use.sum())
        if n_t:  # a track without a kept value is no link of the chain
            s_t = kernel_sum(v, use)
            S, N = (s_t if N == 0 else S + s_t), N + n_t
    out[0] = N
    if N == 0:
        return out
    mean = S / N
    out[1] = mean
    if N > 1:
        SS, first = 0.0, True
        for v, use in parts:
            if not use.any():
                continue
            about = kernel_sum(v, use) / int(use.sum()) if defect == "std_per_track" else mean
            with np.errstate(invalid="ignore"):
                ss_t = kernel_sum((v - about) * (v - about), use)
            SS, first = (ss_t if first else SS + ss_t), False
        out[2] = math.sqrt(SS / (N - 1))
    allv = np.sort(np.concatenate([v[use] for v, use in parts]))
    out[3], out[4 + Q] = allv[0], allv[-1]
    if defect == "mean_of_percentiles":
        each = [[ar.quantile(np.sort(v[use]), q) for q in percentiles] for v, use in parts if use.any()]
        out[4:4 + Q] = np.mean(np.array(each), axis=0)
    else:
        out[4:4 + Q] = [ar.quantile(allv, q) for q in percentiles]
    return out


def _log_tables(logs, L: int, spec: ar.Spec, precise=None, defect=None):
    """Per log: (analysis_ref.analyze's dict, the unit-changed table, the keep mask); the defects of the per-log stage change the last two."""
    per = [ar.analyze(rows, L, spec, None if precise is None else precise[t]) for t, rows in enumerate(logs)]
    tabs, keeps = [p["table"].copy() for p in per], [p["keep"].copy() for p in per]
    if defect == "speed_across":
        for t in range(1, len(logs)):
            n = min(spec.period, len(logs[t - 1]))
            joined = ar.table(np.concatenate([logs[t - 1][len(logs[t - 1]) - n:], logs[t]]), L, spec.period)[n:]
            for name in ar.SPEED_COLUMNS:
                tabs[t][:, ar.COL[name]] = joined[:, ar.COL[name]]
    if defect == "trim_set" and spec.trim_cycles:
        pres = [ar.pre_mask(tab, rows[:, 15], spec) for tab, rows in zip(tabs, logs)]
        lasts = [tab[pre, ar.COL["cycle"]].max() for tab, pre in zip(tabs, pres) if pre.any()]
        for t, (tab, pre) in enumerate(zip(tabs, pres)):
            cyc = tab[:, ar.COL["cycle"]]
            keeps[t] = pre & (cyc != 0) & (cyc != max(lasts)) if lasts else pre
    return per, [ar.to_unit(tab, spec.factors) for tab in tabs], keeps


def analyze_set(logs, L: int, spec: ar.Spec, precise=None, defect=None) -> dict:
    """`logs`: per track the rows16 [R_t, 16] of ONE experiment; `precise`: per track the unrounded precise errors [R_t] or None."""
    per, tabs, keeps = _log_tables(logs, L, spec, precise, defect)
    cols = [ar.COL[c] if isinstance(c, str) else int(c) for c in spec.columns]
    Q = len(spec.percentiles)

    def parts(c, step=None):
        out = []
        for tab, keep in zip(tabs, keeps):
            sel = slice(None) if step is None else slice(step, None, L)
            v = tab[sel, c]
            out.append((v, keep[sel] & ~np.isnan(v)))
        return out

    pooled = dict(n_rows=int(sum(len(r) for r in logs)))
    pooled["describe"] = np.stack([pooled_describe(parts(c), spec.percentiles, defect) for c in cols])
    sq, sc = np.full((L, len(cols), Q), np.nan), np.zeros((L, len(cols)), dtype=np.int64)
    for s in range(L):
        for j, c in enumerate(cols):
            d = pooled_describe(parts(c, s), spec.percentiles, defect)
            sq[s, j], sc[s, j] = d[4:4 + Q], int(d[0])
    pooled["step_quantiles"], pooled["step_count"] = sq, sc
    pooled["cycle_max"], pooled["cycle_mean"] = (np.concatenate([p[k] for p in per]) for k in ("cycle_max", "cycle_mean"))
    pooled["anomaly_mask"] = np.concatenate([p["anomaly_mask"] for p in per])
    pooled["anomaly_counts"], pooled["stats"] = (np.sum([p[k] for p in per], axis=0) for k in ("anomaly_counts", "stats"))
    pooled["values"] = [np.concatenate([tab[keep, c] for tab, keep in zip(tabs, keeps)]) for c in cols]  # the concatenation's kept values per column
    return dict(track=per, pooled=pooled, keep=keeps)
