#!/usr/bin/env python3
"""Timing of the analysis of a population replayed on a SET of tracks (ReplaySet.analyze, wtk_replay_set_analyze) against the same
commit's per-track loop, in one process on one device; prints one JSON line.

  scenario   T seeded random-walk tracks (tools/replay_analysis_timing.py's walk, one seed per track) of --rows logged rows each at (100, 40, 50) ms and
             60 frames/s (L = 9); 1800 rows: every segment, per track and pooled up to T = 11, is sorted in LDS; 21600: above the 19960 keys the LDS
             holds, so the whole-log segments go through the radix select.  E Polyfit experiments with distinct seeded weights (one population call).
             The analysis is section 20's timing spec: period 10, all three clean options, unit "sec", ten columns, six percentiles, four thresholds.
  set        rs.analyze(targets, spec): the set's scan and wtk_replay_set_analyze, every per-track and every pooled output.
  loop       for t: rs.replay(t).analyze(targets of t, spec): the scan and wtk_replay_analyze per track.  Its path is the parent commit's.  It yields the
             per-track results only: the pooled order statistics cannot be had from them at all (a median of medians is not the median), so the loop
             is the lower bound of any route to the pooled result that goes through per-track calls.
  Both are timed by device events around the enqueue, alternating set / loop, --reps times after one warm-up each: median and min - max.
  Before anything is timed the pooled describe table of experiment 0 (order statistics and counts exactly, the rest by value) and every per-track array
  are compared: pooled with tests/harness/replay_set_analysis_ref.py on the logs the per-track path writes, per track with the loop's bits.  The
  harness is slow (explicit loops), so that comparison runs at T = --check-tracks only.
Usage: python tools/replay_set_analysis_timing.py [--experiments 1 16 256] [--tracks 1 4 16] [--rows 1800 21600] [--reps 5] [--check-tracks 4]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from replay_analysis_timing import COLUMNS, PERCENTILES, walk_track  # noqa: E402

TIMES, DEGREE = [-9, -6, -3, 0, 2, 4], 2
ARRAYS = ("describe", "cycle_max", "cycle_mean", "step_quantiles", "step_count", "anomaly_counts", "stats")


def _alternating_ms(fns: dict, reps: int) -> dict:
    """name -> (median, min, max) milliseconds by device events, the functions taking turns."""
    import torch

    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out[k].append(a.elapsed_time(b))
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--experiments", type=int, nargs="+", default=[1, 16, 256])
    ap.add_argument("--tracks", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--rows", type=int, nargs="+", default=[1800, 21600])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--check-tracks", type=int, default=4)
    args = ap.parse_args()

    from harness import analysis_ref as ar
    from harness import replay_set_analysis_ref as sr

    from wtracker_amd import hip
    from wtracker_amd.replay import Analysis, ReplaySet, Targets
    from wtracker_amd.sim import ExperimentConfig, TimingConfig

    if hip.device_count() < 1:
        raise SystemExit("replay_set_analysis_timing: no HIP device visible (nothing is timed on the CPU)")
    out = dict(columns=COLUMNS, percentiles=PERCENTILES, reps=args.reps, cases=[])
    rng = np.random.default_rng(1)
    bounds = (320.0, 320.0, 1180.0, 1180.0)
    for R in args.rows:
        F = R + 1
        ec = ExperimentConfig("timing", F, 60, (1600, 1400), 90, (800, 700))
        tc = TimingConfig(ec, 100, 40, 50, (4, 4), (0.32, 0.32))
        spec = Analysis(period=10, trim_cycles=True, imaging_only=True, bounds=bounds, unit="sec", columns=COLUMNS, percentiles=PERCENTILES, min_bbox_error=0.5,
                        min_dist_error=15 * tc.mm_per_px * 1000, min_speed=300.0, min_size=14.5 * tc.mm_per_px * 1000)
        ref_spec = ar.Spec(period=10, trim_cycles=True, imaging_only=True, bounds=bounds, factors=spec.factors(tc), columns=tuple(COLUMNS),
                           percentiles=tuple(PERCENTILES), min_bbox_error=0.5, min_dist_error=spec.min_dist_error, min_speed=300.0, min_width=spec.min_size,
                           min_height=spec.min_size)
        for T in args.tracks:
            rs = ReplaySet([walk_track(F, seed) for seed in range(T)], tc, ec)
            for E in args.experiments:
                tg = rs.polyfit_population(rng.uniform(0.05, 1.0, size=(E, len(TIMES))), DEGREE, TIMES)
                cut = lambda x, t: x[rs.cyc_off[t]:rs.cyc_off[t] + rs.n_cycles[t]].contiguous()  # noqa: E731
                tgs = [Targets(tg.kind, E, cut(tg.a, t), None, cut(tg.valid, t)) for t in range(T)]
                loop = lambda: [rs.replay(t).analyze(tgs[t], spec) for t in range(T)]  # noqa: E731
                if T == args.check_tracks and E == args.experiments[0]:  # faster and different is not faster
                    got, per = rs.analyze(tg, spec), loop()
                    for t in range(T):
                        for n in ARRAYS:
                            if getattr(got.track[t], n).cpu().numpy().tobytes() != getattr(per[t], n).cpu().numpy().tobytes():
                                raise SystemExit(f"replay_set_analysis_timing: track {t} of {T} at {R} rows: {n} differs from the per-track path")
                    want = sr.analyze_set([rs.replay(t).run(tgs[t], rows=[0]).row_array(0) for t in range(T)], rs.L, ref_spec)["pooled"]
                    d, ref = got.pooled.describe[0].cpu().numpy(), want["describe"]
                    exact = np.r_[0, 3:ref.shape[1]]
                    if not (((d[:, exact] == ref[:, exact]) | (np.isnan(d[:, exact]) & np.isnan(ref[:, exact]))).all()
                            and np.allclose(d[:, 1:3], ref[:, 1:3], rtol=1e-12, atol=0, equal_nan=True)
                            and np.array_equal(got.pooled.stats[0].cpu().numpy(), want["stats"])
                            and np.array_equal(got.pooled.anomaly_counts[0].cpu().numpy(), want["anomaly_counts"])):
                        raise SystemExit(f"replay_set_analysis_timing: the pooled result of {T} tracks at {R} rows differs from the harness")
                ms = _alternating_ms(dict(set=lambda: rs.analyze(tg, spec), loop=loop), args.reps)
                out["cases"].append(dict(rows=R, tracks=T, experiments=E, set_ms=ms["set"], loop_ms=ms["loop"], loop_over_set=ms["loop"][0] / ms["set"][0]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
