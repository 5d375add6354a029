#!/usr/bin/env python3
"""Timing of the Polyfit weight search (csrc/polyfit_opt.hip) at the sizes of the reference's polyfit_optimizer.ipynb; prints one JSON line.

  dataset      a seeded 60 000-frame random-walk track with 0.5 % NaN rows, 200 / 40 / 50 ms timing at 60 fps, the notebook's 8 offsets and its speed
               window 0.1 .. 2 px / frame; `series` = M
  eval_many    P = 100 weight vectors, degree --degree: milliseconds per call by device events (median of --reps calls after a warm-up), once for the
               public call (allocates its result and scratch) and once for the bare three-launch chain on preallocated buffers
  search       wall seconds (host clock around a call that ends in a device synchronise) of optimize() with 100 particles and 300 epochs, early stop
               disabled so that all 300 epochs run: random numbers, upload, 300 x 4 launches, one synchronise; median of --search-reps runs after a warm-up
  host         the float64 numpy restatement (tests/harness/polyfit_opt_ref.py) of one eval on the same dataset: seconds per call over --host-evals
               calls, and that figure x 30 000 (labelled as scaled, not run)
Usage: python tools/polyfit_opt_timing.py [--frames 60000] [--degree 1] [--reps 50] [--search-reps 3] [--host-evals 300]
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


def seeded_track(n: int, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(seed)
    heading = np.cumsum(rng.normal(0.0, 0.15, n)) + rng.uniform(0, 2 * np.pi)
    speed = np.maximum(0.0, rng.normal(0.54, 0.28, n))
    c = np.cumsum(np.stack([speed * np.cos(heading), speed * np.sin(heading)], axis=1), axis=0) + (900.0, 700.0)
    wh = rng.normal((13.8, 14.6), 0.6, (n, 2))
    t = np.concatenate([c - wh / 2, wh], axis=1)
    t[rng.choice(n, size=n // 200, replace=False)] = np.nan
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60000)
    ap.add_argument("--degree", type=int, default=1)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--search-reps", type=int, default=3)
    ap.add_argument("--host-evals", type=int, default=300)
    args = ap.parse_args()

    import torch

    from harness import polyfit_opt_ref as ref
    from wtracker_amd import _build, hip
    from wtracker_amd.polyfit_opt import WeightEvaluator
    from wtracker_amd.sim import ExperimentConfig, TimingConfig

    if hip.device_count() < 1:
        raise SystemExit("polyfit_opt_timing: no HIP device visible (nothing is timed on the CPU)")
    tc = TimingConfig(ExperimentConfig("timing", args.frames, 60, (1600, 1400), 90, (900, 700)), 200, 40, 50, (4, 4), (0.32, 0.32))
    L = tc.cycle_frame_num
    offsets = [-3 * L, -3 * L + 6, -2 * L, -2 * L + 6, -L, -L + 6, 0, 3]
    pred = L + tc.imaging_frame_num // 2
    track = seeded_track(args.frames)
    t0 = time.perf_counter()
    ev = WeightEvaluator.from_tracks([track], tc, offsets, pred, min_speed=0.1, max_speed=2.0)
    out = {"frames": args.frames, "series": ev.n_series, "cycles": ev.cycle_stats, "degree": args.degree, "dataset_first_call_s": round(time.perf_counter() - t0, 3)}

    P, N = 100, len(offsets)
    w = torch.from_numpy(np.random.default_rng(1).random((P, N))).cuda()
    mae = torch.empty(P, dtype=torch.float64, device="cuda")
    scratch = torch.empty(hip.polyfit_mae_scratch_doubles(P, ev.n_series), dtype=torch.float64, device="cuda")

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return round(float(np.median(ms)), 4), round(float(np.min(ms)), 4), round(float(np.max(ms)), 4)

    out["eval_many_p100_ms_median_min_max"] = timed(lambda: ev.eval_many(w, args.degree))
    out["eval_chain_p100_ms_median_min_max"] = timed(lambda: ev._enqueue_mae(w, args.degree, mae, scratch))

    runs = []
    for i in range(args.search_reps + 1):
        t = time.perf_counter()
        res = ev.optimize(args.degree, pop_size=100, max_epoch=300, max_early_stop=300, seed=0)
        runs.append(time.perf_counter() - t)
    out["search_300_epochs_wall_s_median"] = round(float(np.median(runs[1:])), 4)
    out["search_300_epochs_wall_s_all"] = [round(r, 4) for r in runs]
    out["search_epochs_run"], out["search_mae"], out["uniform_mae"] = res.epochs, res.mae, ev.eval(np.ones(N), args.degree)

    y_in, y_tg = ev.y_input.cpu().numpy(), ev.y_target.cpu().numpy()
    wh = w.cpu().numpy()
    ref.mae(y_in, y_tg, offsets, wh[0], args.degree, pred)
    t = time.perf_counter()
    for i in range(args.host_evals):
        ref.mae(y_in, y_tg, offsets, wh[i % P], args.degree, pred)
    per = (time.perf_counter() - t) / args.host_evals
    out["host_numpy_eval_s"] = round(per, 6)
    out["host_numpy_30000_evals_s_scaled"] = round(per * 30000, 2)
    out["host_threads"] = torch.get_num_threads()
    out["device"] = torch.cuda.get_device_name(0)
    out["source_sha"] = _build.source_sha()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
