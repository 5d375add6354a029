"""TEST INFRASTRUCTURE: float64 numpy restatement of a ReplaySet whose tracks each have their OWN TimingConfig: camera size,
microscope size, MLP clip bound and unit factors per track, one cycle structure for all.  Built on harness.replay_set_ref (the guarded super-track,
the set's scan and rows reduction on each track's slice, the pooling), harness.replay_ref (the targets) and harness.replay_set_analysis_ref (the pooled
statistics' defined order); what is new here is only WHICH geometry, bound and factors a track is given.

  load(golden_dir)                 the fixture tests/golden/replay_set_scales.npz: tracks, per-track replay_ref.Geometry, clip bounds, sec factors
  targets(fx, kind, st, bounds)    the per-cycle targets over the super-track; the MLP's clipped with the bound of the cycle's track
  replay(fx, kind, defect)         scan + rows of every track: dict(st, pos, move, logs[t] = replay_ref.rows' dict, track_summary, summary)
  analyze(logs, L, specs)          replay_set_analysis_ref.analyze_set with one analysis_ref.Spec (its factors) per track

It is pinned, not trusted: tests/test_replay_set_scales_ref.py holds it to the fixture the real reference wrote.  `defect` plants the mistake the
feature removes: "config_track0" gives every track the camera, microscope, frame, clip bound and factors of track 0's TimingConfig."""
from __future__ import annotations

import dataclasses
import json
import os

import numpy as np

from harness import analysis_ref as ar
from harness import replay_ref as rr
from harness import replay_set_analysis_ref as sr
from harness import replay_set_ref as rset

DEFECTS = ("config_track0",)
REACH = 64  # wtracker_amd.replay.DEFAULT_REACH: beyond the fixture's sample times and the model's input frames
KIND_ID = {"csv": rr.CSV, "polyfit": rr.POLYFIT, "mlp": rr.MLP}


def load(golden_dir: str) -> dict:
    from oracle import resmlp_oracle

    z = np.load(os.path.join(golden_dir, "replay_set_scales.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    res, geoms, bounds, factors = tuple(meta["orig_resolution"]), [], [], []
    for rec, geo in zip(meta["recordings"], meta["geometry"]):
        cam, mic = tuple(geo["camera_size_px"]), tuple(geo["micro_size_px"])
        frame_wh = (res[1] + cam[1] // 2 * 2, res[0] + cam[0] // 2 * 2)  # the default frame: orig_resolution + camera_size // 2 * 2, read as (H, W)
        geoms.append(rr.Geometry(rec["num_frames"], geo["I"], geo["M"], geo["P"], cam, mic, frame_wh, tuple(rec["init_position"])))
        bounds.append(float(geo["max_dist_per_pred"]))
        factors.append(ar.sec_factors(geo["mm_per_px"], geo["ms_per_frame"]))
    T = len(geoms)
    return dict(z=z, meta=meta, T=T, tracks=[z[f"t{t}/track"] for t in range(T)], geoms=geoms, bounds=bounds, factors=factors,
                state=resmlp_oracle.load_state(os.path.join(golden_dir, meta["model"])))


def with_defect(fx: dict, defect=None) -> tuple:
    """(geoms, bounds, factors) of the tracks as the replay is to see them."""
    assert defect is None or defect in DEFECTS
    if defect != "config_track0":
        return fx["geoms"], fx["bounds"], fx["factors"]
    g0 = fx["geoms"][0]
    geoms = [dataclasses.replace(g, cam=g0.cam, mic=g0.mic, frame_wh=g0.frame_wh) for g in fx["geoms"]]
    return geoms, [fx["bounds"][0]] * fx["T"], [fx["factors"][0]] * fx["T"]


def cycle_bounds(st: rset.SuperTrack, bounds) -> np.ndarray:
    """float32 [n_super_cycles]: the clip bound of the track a cycle's slot (and the guard behind it) belongs to."""
    ends = st.cyc_off[1:] + [st.n_cycles]
    return np.concatenate([np.full(e - o, b, dtype=np.float32) for o, e, b in zip(st.cyc_off, ends, bounds)])


def clip_f32(pred, bound) -> np.ndarray:
    """MLPController's np.clip of the float32 prediction with the float bound (the bound rounds to float32), as float64."""
    b = np.asarray(bound, dtype=np.float32)
    return np.clip(np.asarray(pred, dtype=np.float32), -b, b).astype(np.float64)


def targets(fx: dict, kind: str, st: rset.SuperTrack, g: rr.Geometry, bounds) -> tuple:
    """(a, b, valid, raw) over the super-track, [n_super_cycles, 1, ...] or Nones (csv), as the set's builders compute them in one call; `raw`: the
    MLP's predictions before the clip (the fixture's conditions read them), None for the other kinds."""
    C = st.n_cycles
    if kind == "csv":
        return None, None, None, None
    if kind == "polyfit":
        p = fx["meta"]["polyfit"]
        a, v = rr.targets_polyfit(g, st.track, p["degree"], p["sample_times"], p["weights"], n_cycles=C)
        return a[:, None], None, v[:, None], None
    raw, b, v = rr.targets_mlp(g, st.track, fx["state"], np.inf, n_cycles=C)
    a = clip_f32(raw, cycle_bounds(st, bounds)[:, None])
    return a[:, None], b[:, None], v[:, None], raw


def replay(fx: dict, kind: str, defect=None) -> dict:
    geoms, bounds, _ = with_defect(fx, defect)
    tracks = fx["tracks"]
    st = rset.super_track(tracks, geoms, REACH)
    a, b, valid, raw = targets(fx, kind, st, geoms[0], bounds)
    pos, move = rset.set_scan(KIND_ID[kind], st, tracks, geoms, a, b, valid, 1)
    logs = []
    for t, (tr, g) in enumerate(zip(tracks, geoms)):
        sl = slice(st.cyc_off[t], st.cyc_off[t] + g.n_cycles)
        logs.append(rr.rows(g, st.rows_of(t, len(tr)), pos[sl], move[sl], 0))
    ts = np.stack([lg["summary"] for lg in logs])[:, None, :]
    pooled = np.zeros((1, 6))
    for t in range(fx["T"]):
        pooled = pooled + ts[t]
    return dict(st=st, pos=pos, move=move, logs=logs, track_summary=ts, summary=pooled, raw=raw, valid=valid, geoms=geoms, bounds=bounds)


def analyze(logs, L: int, specs) -> dict:
    """replay_set_analysis_ref.analyze_set where log t goes through its own Spec (they differ in `factors` only): every log through
    analysis_ref.analyze and change_unit with its own factors, the pooled statistics over the concatenation of the values so converted."""
    per = [ar.analyze(rows, L, spec) for rows, spec in zip(logs, specs)]
    tabs, keeps = [ar.to_unit(p["table"], spec.factors) for p, spec in zip(per, specs)], [p["keep"] for p in per]
    spec0 = specs[0]
    cols = [ar.COL[c] if isinstance(c, str) else int(c) for c in spec0.columns]
    Q = len(spec0.percentiles)

    def parts(c, step=None):
        out = []
        for tab, keep in zip(tabs, keeps):
            v = tab[slice(None) if step is None else slice(step, None, L), c]
            out.append((v, keep[slice(None) if step is None else slice(step, None, L)] & ~np.isnan(v)))
        return out

    pooled = dict(n_rows=int(sum(len(r) for r in logs)))
    pooled["describe"] = np.stack([sr.pooled_describe(parts(c), spec0.percentiles) for c in cols])
    sq, sc = np.full((L, len(cols), Q), np.nan), np.zeros((L, len(cols)), dtype=np.int64)
    for s in range(L):
        for j, c in enumerate(cols):
            d = sr.pooled_describe(parts(c, s), spec0.percentiles)
            sq[s, j], sc[s, j] = d[4:4 + Q], int(d[0])
    pooled["step_quantiles"], pooled["step_count"] = sq, sc
    pooled["anomaly_counts"], pooled["stats"] = (np.sum([p[k] for p in per], axis=0) for k in ("anomaly_counts", "stats"))
    pooled["values"] = [np.concatenate([tab[keep, c] for tab, keep in zip(tabs, keeps)]) for c in cols]
    return dict(track=per, pooled=pooled, keep=keeps)
