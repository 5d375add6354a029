#!/usr/bin/env python3
"""Generate tests/golden/analysis_set.npz: the REAL reference's analysis of several logs at once.  Every log goes through its own DataAnalyzer
(wtracker/eval/data_analyzer.py: initialize, clean, change_unit), the cleaned frames through the real Plotter's concatenation with a log_num column
(wtracker/eval/plotter.py:37-40), and the concatenation through the pandas calls of plotter.py:164-168, 203-213, 237-245 and through describe.

Runs only where a checkout of the reference is available (make_golden.REF; it never travels with the tests).  Nothing of the reference's source is
copied: the output is numeric data only.  Placeholder modules stand in for tkinter / cv2 / ultralytics / seaborn as in make_analysis_golden.py.

Input: harness.replay_set_analysis_ref.the_scene: three deterministic tracks that share the L = 5 timing of replay_hard.npz's `_100` runs (the pinned hard
track; its first 137 rows translated into a 400 x 300 frame; replay_ref.long_track with 4125 logged rows), each replayed with csv, optimal and a degree-1
Polyfit by the CPU replay harness, which tests/test_replay_ref.py pins to the reference's logs row for row.  Set (experiment) e is log e of every track.

Configurations: a and b of make_analysis_golden.py, and c: initialize(period=3); clean(trim_cycles, bounds) with bounds to the right of every worm and
microscope box of track 1, so that track 1 keeps no row while tracks 0 and 2 keep some.

Stored per `<config>/<experiment>/`: keep [sum R] (the rows clean kept, the logs side by side), describe [29, 5 + Q] of the concatenation, step_quantiles
[L, 29, Q], step_count [L, 29], cycle_max / cycle_mean [sum n_log, len(CYCLE_COLUMNS)] (groupby(["log_num", "cycle"]); log t's cycles follow those of the
logs before it; NaN: no kept non-NaN row), anomaly_counts [7] and stats [4] (removed rows, no-pred rows, distinct (log_num, cycle) pairs, rows with
bbox_error > 1e-7) over all logs, and kept [T] the kept rows of every log.

Usage: python tests/golden/make_analysis_set_golden.py
"""
import json
import math
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_eval_golden  # noqa: E402
import make_golden  # noqa: E402
from make_analysis_golden import BOUNDS_A, PERCENTILES, THRESHOLDS  # noqa: E402
from make_golden import REF  # noqa: E402

CYCLE_COLUMNS = ["wrm_speed", "worm_deviation", "bbox_error"]  # what the Plotter aggregates per cycle (plotter.py:168, 242-244)


def main():
    make_eval_golden._register_placeholders()
    make_golden._register_placeholders()
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import pandas as pd
    from harness import analysis_ref as ar
    from harness import replay_set_analysis_ref as sr
    from wtracker.eval.data_analyzer import DataAnalyzer
    from wtracker.eval.plotter import Plotter
    from wtracker.sim.config import ExperimentConfig, TimingConfig

    columns = [c for c in ar.COLUMNS if c != "precise_error"]  # (all NaN in a log without frames)
    sc = sr.the_scene(HERE)
    meta, L, T = sc["meta"], sc["L"], len(sc["tracks"])
    geo = meta["geometry"]["100"]
    ec = ExperimentConfig(name="hard", num_frames=meta["num_frames"], frames_per_sec=meta["frames_per_sec"], orig_resolution=tuple(meta["orig_resolution"]),
                          px_per_mm=meta["px_per_mm"], init_position=tuple(meta["init_position"]))
    tc = TimingConfig(ec, *geo["timing"], tuple(meta["camera_size_mm"]), tuple(meta["micro_size_mm"]))
    assert tc.cycle_frame_num == L

    def frame_of(rows16):
        """The DataFrame read_csv gives for a log: integer platform / camera / microscope columns, float worm columns."""
        R = len(rows16)
        d = dict(frame=np.arange(R, dtype=np.int64), cycle=rows16[:, 14].astype(np.int64), phase=np.where(rows16[:, 15] == 0, "imaging", "moving"))
        for k, n in enumerate(("plt_x", "plt_y", "cam_x", "cam_y", "cam_w", "cam_h", "mic_x", "mic_y", "mic_w", "mic_h")):
            d[n] = rows16[:, k].astype(np.int64)
        for k, n in enumerate(("wrm_x", "wrm_y", "wrm_w", "wrm_h")):
            d[n] = rows16[:, 10 + k].astype(np.float64)
        return pd.DataFrame(d)

    # the bounds of c: to the right of everything track 1 ever logs
    right = max(float(np.max(rows[:, [6, 10]])) for kind in sr.KINDS for rows in [sc["logs"][kind][1]])
    bounds_c = (float(math.ceil(right)) + 1.0, -10000.0, 10000.0, 10000.0)
    configs = {
        "a": dict(period=3, clean=dict(trim_cycles=True, imaging_only=True, bounds=BOUNDS_A), unit="frame"),
        "b": dict(period=10, clean=None, unit="sec"),
        "c": dict(period=3, clean=dict(trim_cycles=True, imaging_only=False, bounds=bounds_c), unit="frame"),
    }
    n_log = [len(rows) // L for rows in sc["logs"]["csv"]]
    log0, row0 = np.concatenate([[0], np.cumsum(n_log)]), np.concatenate([[0], np.cumsum([n * L for n in n_log])])
    out, Q = {}, len(PERCENTILES)
    for cname, cfg in configs.items():
        for kind in sr.KINDS:
            key = f"{cname}/{kind}/"
            cleaned, keep, counts, stats = [], np.zeros(row0[-1], dtype=bool), np.zeros(7, dtype=np.int64), np.zeros(4, dtype=np.int64)
            for t in range(T):
                an = DataAnalyzer(tc, frame_of(sc["logs"][kind][t]))
                an.initialize(period=cfg["period"])
                if cfg["clean"] is not None:
                    an.clean(**cfg["clean"])
                keep[row0[t] + an.data["frame"].to_numpy()] = True
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    an.change_unit(cfg["unit"])
                anom = an.calc_anomalies(no_preds=True, **THRESHOLDS)
                names = ("speed", "bbox_error", "dist_error", "width", "height", "no_pred")
                counts += np.array([int(anom[n + "_anomaly"].sum()) for n in names] + [len(anom)], dtype=np.int64)
                wrm = an.data[["wrm_x", "wrm_y", "wrm_w", "wrm_h"]]
                stats += np.array([len(an._orig_data.index) - len(an.data.index), int(wrm.isna().any(axis=1).sum()), 0, int((an.data["bbox_error"] > 1e-7).sum())])
                cleaned.append(an.data)
            data = Plotter(cleaned).data  # log_num and the concatenation are the Plotter's own
            assert list(data["log_num"].unique()) == [t for t in range(T) if len(cleaned[t])]
            stats[2] = len(data[["log_num", "cycle"]].drop_duplicates())
            desc = data[columns].describe(list(PERCENTILES))
            assert list(desc.index[:4]) == ["count", "mean", "std", "min"] and desc.index[-1] == "max" and len(desc.index) == 5 + Q, list(desc.index)
            out[key + "describe"] = desc.to_numpy(dtype=np.float64).T.copy()
            cmax, cmean = np.full((log0[-1], len(CYCLE_COLUMNS)), np.nan), np.full((log0[-1], len(CYCLE_COLUMNS)), np.nan)
            gmax = data.groupby(["log_num", "cycle"])[CYCLE_COLUMNS].max().reset_index()  # plotter.py:168
            gmean = data.groupby(["log_num", "cycle"])[CYCLE_COLUMNS].aggregate({c: "mean" for c in CYCLE_COLUMNS}).reset_index()  # plotter.py:242-244
            cmax[log0[gmax["log_num"].to_numpy()] + gmax["cycle"].to_numpy()] = gmax[CYCLE_COLUMNS].to_numpy(np.float64)
            cmean[log0[gmean["log_num"].to_numpy()] + gmean["cycle"].to_numpy()] = gmean[CYCLE_COLUMNS].to_numpy(np.float64)
            out[key + "cycle_max"], out[key + "cycle_mean"] = cmax, cmean
            sq, scnt = np.full((L, len(columns), Q), np.nan), np.zeros((L, len(columns)), dtype=np.int64)
            for s, grp in data.groupby("cycle_step"):  # the distributions plot_cycle_error draws per cycle step
                for j, c in enumerate(columns):
                    scnt[int(s), j] = int(grp[c].count())
                    if scnt[int(s), j]:
                        sq[int(s), j] = grp[c].quantile(list(PERCENTILES)).to_numpy()
            out[key + "step_quantiles"], out[key + "step_count"] = sq, scnt
            out[key + "anomaly_counts"], out[key + "stats"], out[key + "keep"] = counts, stats, keep
            out[key + "kept"] = np.array([int(keep[row0[t]:row0[t + 1]].sum()) for t in range(T)], dtype=np.int64)
            print(key, "kept", out[key + "kept"].tolist(), "anomalies", counts.tolist(), "stats", stats.tolist())
    # what the fixture exists for
    for kind in sr.KINDS:
        k = out[f"c/{kind}/kept"]
        assert k[1] == 0 and k[0] > 0 and k[2] > 0, (kind, k)
        assert (out[f"a/{kind}/kept"] > 0).all() and out[f"b/{kind}/kept"].tolist() == [395, 135, 4125]
    j = columns.index("wrm_speed")
    assert out["b/csv/describe"][j, 0] <= 395 + 135 + 4125 - T * 10, "every log has its own NaN head of `period` speeds"
    out["meta"] = np.frombuffer(json.dumps(dict(
        kinds=list(sr.KINDS), columns=columns, cycle_columns=CYCLE_COLUMNS, percentiles=list(PERCENTILES), thresholds=THRESHOLDS, n_log=n_log,
        configs={k: dict(period=v["period"], clean=v["clean"] and dict(v["clean"], bounds=list(v["clean"]["bounds"])), unit=v["unit"]) for k, v in configs.items()},
        sec_factors=dict(mm_per_px=ec.mm_per_px, ms_per_frame=ec.ms_per_frame))).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "analysis_set.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "analysis.npz"))


if __name__ == "__main__":
    main()
