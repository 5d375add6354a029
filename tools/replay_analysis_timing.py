#!/usr/bin/env python3
"""Timing of DataAnalyzer's statistics of a replayed population on the device (Replay.run(analysis=...), wtk_replay_analyze) against
the route a user had before it, in one process on one device; prints one JSON line.

  scenario   a seeded random-walk track at (100, 40, 50) ms and 60 frames/s (L = 9), camera 4 mm and microscope 0.32 mm at 90 px/mm; per population size E
             of --experiments: E Polyfit experiments with distinct seeded weights; per row count of --rows (1800: every segment is sorted in LDS; 21600:
             above the 19960 keys the LDS holds, so the whole-experiment segments go through the radix select).  The analysis: period 10, all three clean
             options, unit "sec", --columns columns, six percentiles, four anomaly thresholds.
  device     wtk_replay_analyze on the scan's positions (every output, the scan excluded): milliseconds by device events, median of --reps runs after
             one warm-up.  `run_ms`: Replay.run(targets, rows=[], analysis=spec) by the host clock, the scan, the rows kernel and the copies included.
  host       the route before: Replay.run(targets, rows=range(E)) (16 doubles per row and experiment to the host; `rows_ms`, host clock) and the numpy
             restatement tests/harness/analysis_ref.py per experiment.  That harness is written for checking, not for speed (explicit summation loops):
             it is timed on --host-sample experiments and `host_ms` = rows_ms + E x the mean of those; pandas itself is not on this machine's path.
  The device's describe tables of the sampled experiments are compared with the harness's (order statistics and counts exactly) before anything is timed.
Usage: python tools/replay_analysis_timing.py [--experiments 1 16 256] [--rows 1800 21600] [--reps 5] [--host-sample 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

COLUMNS = ["wrm_speed", "worm_deviation", "bbox_error", "wrm_speed_x", "worm_deviation_x", "wrm_w", "wrm_h", "wrm_center_x", "wrm_center_y", "time"]
PERCENTILES = [0.05, 0.25, 0.5, 0.75, 0.95, 0.99]


def walk_track(n: int, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(seed)
    heading = np.cumsum(rng.normal(0.0, 0.1, n))
    centre = np.array([800.0, 700.0]) + np.cumsum(2.5 * np.stack([np.cos(heading), np.sin(heading)], axis=1), axis=0)
    centre = 300 + (centre - 300) % 900  # folded back into the frame
    wh = 14.0 + rng.normal(0.0, 0.6, (n, 2))
    track = np.concatenate([centre - wh / 2, wh], axis=1)
    track[rng.random(n) < 0.01] = np.nan
    return track


def _event_ms(fn, reps: int) -> float:
    import torch

    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def _clock_ms(fn, reps: int):
    fn()
    out, last = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        last = fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--experiments", type=int, nargs="+", default=[1, 16, 256])
    ap.add_argument("--rows", type=int, nargs="+", default=[1800, 21600])
    ap.add_argument("--columns", type=int, default=len(COLUMNS))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-sample", type=int, default=2)
    args = ap.parse_args()

    import torch
    from harness import analysis_ref as ar

    from wtracker_amd import hip
    from wtracker_amd.controllers import PolyfitConfig
    from wtracker_amd.replay import Analysis, Replay, _enqueue_analysis
    from wtracker_amd.sim import ExperimentConfig, TimingConfig

    if hip.device_count() < 1:
        raise SystemExit("replay_analysis_timing: no HIP device visible (nothing is timed on the CPU)")
    cols = COLUMNS[:args.columns]
    out = dict(columns=cols, percentiles=PERCENTILES, reps=args.reps, host_sample=args.host_sample, cases=[])
    rng = np.random.default_rng(1)
    for R in args.rows:
        F = R + 1
        ec = ExperimentConfig("timing", F, 60, (1600, 1400), 90, (800, 700))
        tc = TimingConfig(ec, 100, 40, 50, (4, 4), (0.32, 0.32))
        rp = Replay(walk_track(F), tc, ec)
        bounds = (320.0, 320.0, 1180.0, 1180.0)
        spec = Analysis(period=10, trim_cycles=True, imaging_only=True, bounds=bounds, unit="sec", columns=cols, percentiles=PERCENTILES, min_bbox_error=0.5,
                        min_dist_error=15 * tc.mm_per_px * 1000, min_speed=300.0, min_size=14.5 * tc.mm_per_px * 1000)
        ref_spec = ar.Spec(period=10, trim_cycles=True, imaging_only=True, bounds=bounds, factors=spec.factors(tc), columns=tuple(cols),
                           percentiles=tuple(PERCENTILES), min_bbox_error=0.5, min_dist_error=spec.min_dist_error, min_speed=300.0, min_width=spec.min_size,
                           min_height=spec.min_size)
        stream = torch.cuda.current_stream(rp._dev).cuda_stream
        for E in args.experiments:
            cfgs = [PolyfitConfig(2, [-9, -6, -3, 0, 2, 4], [float(v) for v in w]) for w in rng.uniform(0.05, 1.0, size=(E, 6))]
            tg = rp.polyfit(cfgs)
            sample = list(range(min(E, args.host_sample)))
            res = rp.run(tg, rows=sample, analysis=spec)
            host_each = []
            for e in sample:  # faster and different is not faster
                t0 = time.perf_counter()
                want = ar.analyze(res.row_array(e), rp.L, ref_spec)
                host_each.append((time.perf_counter() - t0) * 1e3)
                got, ref = res.analysis.describe[e], want["describe"]
                exact = np.r_[0, 3:ref.shape[1]]
                if not (((got[:, exact] == ref[:, exact]) | (np.isnan(got[:, exact]) & np.isnan(ref[:, exact]))).all()
                        and np.array_equal(res.analysis.stats[e], want["stats"]) and np.array_equal(res.analysis.anomaly_counts[e], want["anomaly_counts"])):
                    raise SystemExit(f"replay_analysis_timing: experiment {e} of {E} at {rp.n_rows} rows differs from the harness")
            buf = rp._objective_buffers(E)
            hip.replay_scan(rp._cfg, hip.REPLAY_POLYFIT, E, rp.n_cycles, rp.track, rp.n_track, tg.a, None, tg.valid, rp._share, buf["pos"], buf["move"], stream=stream)
            device = lambda: _enqueue_analysis(rp.geometry, tc, spec, E, rp.track, rp.n_track, rp._share, buf["pos"], buf["move"], None, stream)  # noqa: E731
            case = dict(rows=rp.n_rows, experiments=E, device_ms=_event_ms(device, args.reps))
            case["run_ms"], _ = _clock_ms(lambda: rp.run(tg, rows=[], analysis=spec), args.reps)
            case["rows_ms"], _ = _clock_ms(lambda: rp.run(tg, rows=range(E)), max(1, args.reps // 2))
            case["harness_ms_per_experiment"] = float(np.mean(host_each))
            case["host_ms"] = case["rows_ms"] + E * case["harness_ms_per_experiment"]
            case["host_over_run"] = case["host_ms"] / case["run_ms"]
            case["rows_over_run"] = case["rows_ms"] / case["run_ms"]
            case["kept_rows_first"] = int(res.analysis.describe[0, cols.index("bbox_error") if "bbox_error" in cols else 0, 0])
            out["cases"].append(case)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
