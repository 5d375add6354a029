#!/usr/bin/env python3
"""Timing of ONE EPOCH of the closed-loop weight search (Replay.optimize_polyfit) at the notebook's sizes, against the same epoch
assembled from the calls that existed before it; prints one JSON line.

  new      wtk_replay_polyfit_targets on the device-resident weights [P, N], wtk_replay_objective, wtk_polyfit_swarm_step: what optimize_polyfit enqueues
           per epoch.  Device milliseconds (events around the epoch) and host wall milliseconds of the enqueue alone; nothing is downloaded.
  parent   weights downloaded, one PolyfitConfig per particle, Replay.polyfit(configs) (one wtk_track_polyfit and two strided copies per config), then
           Replay.run (scan, rows, one synchronisation, downloads): the only way to get the population's closed-loop error before.  Device milliseconds
           and host wall milliseconds of the whole round trip.
  svd      decompositions per epoch: classes x P (new) against cycles x P (parent).
Median of --reps runs after one warm-up.  Sizes: P = 100, N = 8 (the notebook's offsets -3L, -3L+6, -2L, -2L+6, -L, -L+6, 0, 3), degree 2, (200, 40, 50) ms
at 60 frames/s, a 9 000-frame track: --track BBOXES_CSV, else the seeded random walk of tools/replay_timing.py (1 % NaN rows) cut to --frames.
Usage: python tools/replay_opt_timing.py [--pop-size 100] [--frames 9000] [--reps 5] [--track bboxes.csv]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _time(fn, reps):
    """-> (median device ms, median host wall ms) of fn() followed by a synchronisation of the current stream."""
    import torch

    fn()
    torch.cuda.synchronize()
    dev_ms, wall_ms = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        t1 = time.perf_counter()
        b.synchronize()
        dev_ms.append(a.elapsed_time(b))
        wall_ms.append((t1 - t0) * 1e3)
    return float(np.median(dev_ms)), float(np.median(wall_ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pop-size", type=int, default=100)
    ap.add_argument("--frames", type=int, default=9000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--track", default=None)
    args = ap.parse_args()

    import torch

    from replay_timing import random_walk
    from wtracker_amd import hip
    from wtracker_amd.controllers import PolyfitConfig, _read_track_csv
    from wtracker_amd.replay import OBJECTIVES, Replay, Targets
    from wtracker_amd.sim import ExperimentConfig, TimingConfig

    if hip.device_count() < 1:
        raise SystemExit("replay_opt_timing: no HIP device visible (nothing is timed on the CPU)")
    track = _read_track_csv(args.track)[: args.frames] if args.track else random_walk(args.frames)
    F, P, degree = len(track), args.pop_size, 2
    ec = ExperimentConfig("timing", F, 60, (1600, 1400), 90, (1300, 1200))
    tc = TimingConfig(ec, 200, 40, 50, (4, 4), (0.32, 0.32))
    rp = Replay(track, tc, ec)
    L = rp.L
    times = sorted([-3 * L, -3 * L + 6, -2 * L, -2 * L + 6, -L, -L + 6, 0, 3])
    N = len(times)
    dev, f64 = rp._dev, torch.float64
    weights = torch.from_numpy(np.random.default_rng(1).uniform(0.05, 1.0, size=(P, N))).to(dev)
    classes = rp.polyfit_class_table(times)
    n_classes = int(classes[1].numel())
    out = dict(pop_size=P, n_times=N, degree=degree, frames=F, track=args.track or "seeded random walk", cycles=rp.n_cycles, rows=rp.n_rows, classes=n_classes,
               reps=args.reps, svd_per_epoch_new=n_classes * P, svd_per_epoch_parent=rp.n_cycles * P)

    # ---- the new path: what optimize_polyfit enqueues per epoch, on buffers allocated once
    tg = Targets("polyfit", P, torch.zeros((rp.n_cycles, P, 2), dtype=f64, device=dev), None, torch.zeros((rp.n_cycles, P), dtype=torch.int32, device=dev))
    fit = torch.empty((hip.replay_polyfit_targets_scratch_doubles(n_classes, P, N, degree),), dtype=f64, device=dev)
    buf, value = rp._objective_buffers(P), torch.empty((P,), dtype=f64, device=dev)
    pos, vel, pbest_pos = weights.clone(), torch.zeros((P, N), dtype=f64, device=dev), weights.clone()
    pbest_val, gbest_pos, gbest_val = torch.full((P,), float("inf"), dtype=f64, device=dev), weights[0].clone(), torch.full((1,), float("inf"), dtype=f64, device=dev)
    ctrl, history = torch.zeros((4,), dtype=torch.int32, device=dev), torch.zeros((1,), dtype=f64, device=dev)
    rand = torch.zeros((2, P, N), dtype=f64, device=dev)  # no motion: every repetition times the same positions
    stream = torch.cuda.current_stream(dev).cuda_stream

    def new_epoch():
        rp._enqueue_population(pos, degree, tuple(times), classes, tg.a, tg.valid, fit, stop_dev=ctrl)
        rp._enqueue_objective(tg, OBJECTIVES["trimmed_bbox_error"], buf, value, stop_dev=ctrl)
        hip.polyfit_swarm_step(value, rand, P, N, 0, 1 << 30, 0.9, 2.05, 2.05, 0.0, 1.0, 0.5, pos, vel, pbest_pos, pbest_val, gbest_pos, gbest_val, ctrl, history,
                               stream=stream)

    out["new_epoch_device_ms"], out["new_epoch_enqueue_wall_ms"] = _time(new_epoch, args.reps)
    torch.cuda.synchronize()
    new_value = value.cpu().numpy()

    # ---- the parent's route: host weights, one launch and two copies per config, run() with its synchronisation and downloads
    holder = {}

    def parent_epoch():
        w = weights.cpu().numpy()
        cfgs = [PolyfitConfig(degree, times, [float(v) for v in row]) for row in w]
        holder["res"] = rp.run(rp.polyfit(cfgs), rows=[])

    out["parent_epoch_device_ms"], out["parent_epoch_wall_ms"] = _time(parent_epoch, args.reps)
    same = np.asarray(holder["res"].summary.trimmed_mean_bbox_error).tobytes() == new_value.tobytes()
    out["objective_bits_equal"] = bool(same)
    out["trimmed_bbox_error_min_max"] = [float(np.nanmin(new_value)), float(np.nanmax(new_value))]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
