#!/usr/bin/env python3
"""Generate tests/golden/analysis.npz by running the REAL reference's DataAnalyzer (wtracker/eval/data_analyzer.py) and the pandas calls of its
Plotter (wtracker/eval/plotter.py:164-168, 203-213, 237-245) on the logs already pinned in tests/golden/replay_hard.npz.

Runs only where a checkout of the reference is available (make_golden.REF; it never travels with the tests).  Nothing of the reference's source is
copied: the output is numeric data only.  Placeholder modules stand in for tkinter / cv2 / ultralytics / seaborn as in make_replay_golden.py.

Input: the runs csv_100, optimal_100, polyfit0..3_100 and polyfit1_200 of replay_hard.npz (30 frames/s: L = 5 and 8, R = 395 and 392).  The DataFrame of
a run is rebuilt from plt / cam / mic / wrm / cycle / phase with the camera 360 x 360 and the microscope 29 x 29, the dtypes read_csv gives them.

Configurations (name: what is called on the DataAnalyzer, in this order):
  a    initialize(period=3); clean(trim_cycles, imaging_only, bounds=(40, 40, 1500, 1300))
  b    initialize(period=10); change_unit("sec")
  c0   initialize(period=3); clean(trim_cycles, imaging_only, bounds=(-2, -2, -1, -1)): no row survives
  c1   initialize(period=3); clean(bounds = the rounded worm box of row 200 of csv_100): exactly one row of csv_100 survives
then describe(COLUMNS, percentiles=PERCENTILES), the two groupby aggregates, the per-cycle_step quantiles and counts, calc_anomalies(min_bbox_error=0.5,
min_dist_error=15, min_speed=4.5, min_size=14.5) and the figures of print_stats.

Stored per `<config>/<run>/`: table [R, 29] (a and b only: every numeric column after initialize, uncleaned, frame units, in the order of meta's `columns`), keep [R]
(the rows clean kept), describe [29, 5 + Q] (count, mean, std, min, percentiles, max), cycle_max / cycle_mean [n_log, 29] (NaN: no kept non-NaN row),
step_quantiles [L, 29, Q], step_count [L, 29], anomaly_mask uint8 [R] (bit k: the k-th of speed, bbox_error, dist_error, width, height, no_pred; 0 on rows
that were not kept), anomaly_counts [7] (the six and `any`), stats [4] (removed rows, no-pred rows, distinct cycles, rows with bbox_error > 1e-7).

Usage: python tests/golden/make_analysis_golden.py
"""
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_eval_golden  # noqa: E402
import make_golden  # noqa: E402
from make_golden import REF  # noqa: E402

RUNS = ["csv_100", "optimal_100", "polyfit0_100", "polyfit1_100", "polyfit2_100", "polyfit3_100", "polyfit1_200"]
PERCENTILES = (0.05, 0.25, 0.5, 0.75, 0.95, 0.99)
THRESHOLDS = dict(min_bbox_error=0.5, min_dist_error=15, min_speed=4.5, min_size=14.5)
BOUNDS_A = (40, 40, 1500, 1300)
ONE_ROW = 200  # of csv_100: configuration c1 keeps this row alone


def main():
    make_eval_golden._register_placeholders()
    make_golden._register_placeholders()
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import pandas as pd
    from harness import analysis_ref as ar
    from wtracker.eval.data_analyzer import DataAnalyzer
    from wtracker.sim.config import ExperimentConfig, TimingConfig

    columns = [c for c in ar.COLUMNS if c != "precise_error"]  # (all NaN in a log without frames)
    z = np.load(os.path.join(HERE, "replay_hard.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    ec = ExperimentConfig(name="hard", num_frames=meta["num_frames"], frames_per_sec=meta["frames_per_sec"], orig_resolution=tuple(meta["orig_resolution"]),
                          px_per_mm=meta["px_per_mm"], init_position=tuple(meta["init_position"]))

    def frame_of(run):
        geo = meta["geometry"][run.split("_")[1]]
        R = len(z[run + "/cycle"])
        d = dict(frame=np.arange(R, dtype=np.int64), cycle=z[run + "/cycle"].astype(np.int64),
                 phase=np.where(z[run + "/phase"] == 0, "imaging", "moving"))
        for k, n in enumerate(("plt_x", "plt_y")):
            d[n] = z[run + "/plt"][:, k].astype(np.int64)
        for k, n in enumerate(("cam_x", "cam_y")):
            d[n] = z[run + "/cam"][:, k].astype(np.int64)
        d["cam_w"], d["cam_h"] = np.full(R, geo["camera_size_px"][0], np.int64), np.full(R, geo["camera_size_px"][1], np.int64)
        for k, n in enumerate(("mic_x", "mic_y")):
            d[n] = z[run + "/mic"][:, k].astype(np.int64)
        d["mic_w"], d["mic_h"] = np.full(R, geo["micro_size_px"][0], np.int64), np.full(R, geo["micro_size_px"][1], np.int64)
        for k, n in enumerate(("wrm_x", "wrm_y", "wrm_w", "wrm_h")):
            d[n] = z[run + "/wrm"][:, k].astype(np.float64)
        assert geo["camera_size_px"] == [360, 360] and geo["micro_size_px"] == [29, 29]
        tc = TimingConfig(ec, *geo["timing"], tuple(meta["camera_size_mm"]), tuple(meta["micro_size_mm"]))
        assert tc.cycle_frame_num == geo["L"]
        return pd.DataFrame(d), tc, geo["L"]

    # the bounds of c1: the rounded worm box of one row of csv_100
    w = ar.round5(z["csv_100/wrm"][ONE_ROW])
    bounds_c1 = (float(w[0]), float(w[1]), float(w[0] + w[2]), float(w[1] + w[3]))
    configs = {
        "a": dict(period=3, clean=dict(trim_cycles=True, imaging_only=True, bounds=BOUNDS_A), unit="frame"),
        "b": dict(period=10, clean=None, unit="sec"),
        "c0": dict(period=3, clean=dict(trim_cycles=True, imaging_only=True, bounds=(-2, -2, -1, -1)), unit="frame"),
        "c1": dict(period=3, clean=dict(trim_cycles=False, imaging_only=False, bounds=bounds_c1), unit="frame"),
    }
    out, kept_rows, Q = {}, {}, len(PERCENTILES)
    for cname, cfg in configs.items():
        for run in RUNS:
            df, tc, L = frame_of(run)
            R, n_log = len(df), len(df) // L
            an = DataAnalyzer(tc, df)
            an.initialize(period=cfg["period"])
            table = an.data[columns].to_numpy(dtype=np.float64)
            if cfg["clean"] is not None:
                an.clean(**cfg["clean"])
            keep = np.zeros(R, dtype=bool)
            keep[an.data["frame"].to_numpy()] = True
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                an.change_unit(cfg["unit"])
            data = an.data
            data["log_num"] = 0
            key = f"{cname}/{run}/"
            desc = an.describe(columns, percentiles=list(PERCENTILES))
            assert list(desc.index[:4]) == ["count", "mean", "std", "min"] and desc.index[-1] == "max" and len(desc.index) == 5 + Q, list(desc.index)
            out[key + "describe"] = desc.to_numpy(dtype=np.float64).T.copy()
            cmax, cmean = np.full((n_log, len(columns)), np.nan), np.full((n_log, len(columns)), np.nan)
            if len(data):
                others = [c for c in columns if c != "cycle"]  # (the group key itself aggregates to its own value)
                gmax = data.groupby(["log_num", "cycle"])[others].max().reset_index()  # plotter.py:168, for every column
                gmean = data.groupby(["log_num", "cycle"])[others].aggregate({c: "mean" for c in others}).reset_index()  # plotter.py:242-244
                cmax[gmax["cycle"].to_numpy()], cmean[gmean["cycle"].to_numpy()] = gmax[columns].to_numpy(np.float64), gmean[columns].to_numpy(np.float64)
            out[key + "cycle_max"], out[key + "cycle_mean"] = cmax, cmean
            sq, sc = np.full((L, len(columns), Q), np.nan), np.zeros((L, len(columns)), dtype=np.int64)
            for s, grp in data.groupby("cycle_step"):  # the distributions plot_cycle_error draws per cycle step
                for j, c in enumerate(columns):
                    sc[int(s), j] = int(grp[c].count())
                    if sc[int(s), j]:
                        sq[int(s), j] = grp[c].quantile(list(PERCENTILES)).to_numpy()
            out[key + "step_quantiles"], out[key + "step_count"] = sq, sc
            anom = an.calc_anomalies(no_preds=True, **THRESHOLDS)
            bits = np.zeros(R, dtype=np.uint8)
            for k, n in enumerate(("speed", "bbox_error", "dist_error", "width", "height", "no_pred")):
                bits[anom["frame"].to_numpy()[anom[n + "_anomaly"].to_numpy(dtype=bool)]] |= np.uint8(1 << k)
            out[key + "anomaly_mask"] = bits
            out[key + "anomaly_counts"] = np.array([int(anom[n + "_anomaly"].sum()) for n in ("speed", "bbox_error", "dist_error", "width", "height", "no_pred")]
                                                   + [len(anom)], dtype=np.int64)
            wrm = data[["wrm_x", "wrm_y", "wrm_w", "wrm_h"]]
            out[key + "stats"] = np.array([len(an._orig_data.index) - len(data.index), int(wrm.isna().any(axis=1).sum()), int(data["cycle"].nunique()),
                                           int((data["bbox_error"] > 1e-7).sum())], dtype=np.int64)
            out[key + "keep"] = keep
            if cname in ("a", "b"):  # (c0 and c1 initialise as a does)
                out[key + "table"] = table
            kept_rows[(cname, run)] = int(keep.sum())
            print(key, "kept", int(keep.sum()), "of", R, "anomalies", out[key + "anomaly_counts"].tolist(), "stats", out[key + "stats"].tolist())
    # what the fixture exists for
    assert kept_rows[("a", "csv_100")] == 120 and kept_rows[("a", "polyfit1_200")] == 155, kept_rows
    assert all(kept_rows[("c0", r)] == 0 for r in RUNS) and kept_rows[("c1", "csv_100")] == 1
    assert all(kept_rows[("b", r)] == len(z[r + "/cycle"]) for r in RUNS)
    j = columns.index("bbox_error")
    quart = out["a/csv_100/step_quantiles"][:, j, 1:4]
    assert len({tuple(q) for q in quart[~np.isnan(quart).any(axis=1)]}) > 1, "the bbox-error quartiles do not differ between cycle steps"
    assert (out["a/csv_100/anomaly_counts"][:3] > 0).all(), "a speed, bbox or distance anomaly class is empty"
    tails = {int(np.nanmax(np.where(out[f"a/{r}/keep"], out[f"a/{r}/table"][:, columns.index("cycle")], np.nan))) for r in RUNS if r.endswith("_100")}
    print("last kept cycles at L = 5:", sorted(tails))
    out["meta"] = np.frombuffer(json.dumps(dict(
        runs=RUNS, columns=columns, percentiles=list(PERCENTILES), thresholds=THRESHOLDS,
        configs={k: dict(period=v["period"], clean=v["clean"] and dict(v["clean"], bounds=list(v["clean"]["bounds"])), unit=v["unit"]) for k, v in configs.items()},
        sec_factors={t: dict(mm_per_px=ec.mm_per_px, ms_per_frame=ec.ms_per_frame) for t in ("100", "200")})).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "analysis.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
