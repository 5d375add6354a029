#!/usr/bin/env python3
"""Timing of the closed-loop replay (wtracker_amd/replay.py, csrc/replay.hip) at experiment scale; prints one JSON line.

  replay   --experiments Polyfit configs (distinct seeded weights) x --frames frames of a seeded random-walk track at (100, 40, 50) ms, 60 frames/s:
           milliseconds by device events (median of --reps runs after one warm-up) of the targets (one wtk_track_polyfit per config), of the scan and
           the rows kernels together (Replay.run without its downloads is not separable from the host: the two entry points are timed directly), and
           the wall time of builders + run() including the downloads.
  host     the host frame loop (tests/harness/sim_harness.py: Simulator + TrackLogger + PolyfitController) for ONE experiment on the first
           --host-frames frames of the same track, in seconds, and scaled linearly to --frames (labelled as extrapolated).
Usage: python tools/replay_timing.py [--experiments 256] [--frames 60000] [--reps 5] [--host-frames 6000]
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def random_walk(n: int, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(seed)
    speed = np.maximum(0.0, rng.normal(0.54, 0.28, n))
    heading = rng.uniform(0, 2 * np.pi) + np.cumsum(rng.normal(0.0, 0.15, n))
    pos = np.array([1300.0, 1200.0]) + np.cumsum(speed[:, None] * np.stack([np.cos(heading), np.sin(heading)], axis=1), axis=0)
    pos = np.abs(pos) % 2800.0  # folded back: the walk stays within a few frames' width
    w, h = 13.8 + rng.normal(0, 0.6, n), 14.6 + rng.normal(0, 0.6, n)
    track = np.stack([pos[:, 0] - w / 2, pos[:, 1] - h / 2, w, h], axis=1)
    track[rng.random(n) < 0.01] = np.nan
    return track


def _time_ms(fn, reps):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--experiments", type=int, default=256)
    ap.add_argument("--frames", type=int, default=60000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-frames", type=int, default=6000)
    args = ap.parse_args()

    import torch

    from wtracker_amd import hip
    from wtracker_amd.controllers import PolyfitConfig, PolyfitController
    from wtracker_amd.replay import KINDS, Replay
    from wtracker_amd.sim import ExperimentConfig, TimingConfig, TrackLogger

    if hip.device_count() < 1:
        raise SystemExit("replay_timing: no HIP device visible (nothing is timed on the CPU)")
    E, F = args.experiments, args.frames
    track = random_walk(F)
    ec = ExperimentConfig("timing", F, 60, (1600, 1400), 90, (1300, 1200))
    tc = TimingConfig(ec, 100, 40, 50, (4, 4), (0.32, 0.32))
    rp = Replay(track, tc, ec)
    rng = np.random.default_rng(1)
    cfgs = [PolyfitConfig(2, [-9, -6, -3, 0, 2, 4], [float(v) for v in w]) for w in rng.uniform(0.05, 1.0, size=(E, 6))]
    out = dict(experiments=E, frames=F, cycles=rp.n_cycles, rows=rp.n_rows, reps=args.reps)

    holder = {}
    out["targets_ms"] = _time_ms(lambda: holder.__setitem__("t", rp.polyfit(cfgs)), args.reps)
    tg = holder["t"]
    dev, C, R = rp._dev, rp.n_cycles, rp.n_rows
    pos = torch.empty((C, E, 2), dtype=torch.int32, device=dev)
    move = torch.empty((C, E, 2), dtype=torch.int32, device=dev)
    summary = torch.empty((E, hip.REPLAY_SUMMARY_DOUBLES), dtype=torch.float64, device=dev)
    scratch = torch.empty((hip.replay_scratch_doubles(E, R),), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    scan = lambda: hip.replay_scan(rp._cfg, KINDS["polyfit"], E, C, rp.track, rp.n_track, tg.a, None, tg.valid, rp._share, pos, move, stream=stream)  # noqa: E731
    rows = lambda: hip.replay_rows(rp._cfg, E, C, rp.track, rp.n_track, rp._share, pos, move, None, 0, None, None, None, summary, scratch, scratch.numel(),  # noqa: E731
                                   stream=stream)
    out["scan_ms"] = _time_ms(scan, args.reps)
    out["rows_ms"] = _time_ms(rows, args.reps)
    t0 = time.perf_counter()
    res = rp.run(rp.polyfit(cfgs), rows=[0])
    out["builders_and_run_wall_s"] = time.perf_counter() - t0
    out["mean_bbox_error_min_max"] = [float(res.summary.mean_bbox_error.min()), float(res.summary.mean_bbox_error.max())]

    # the host loop, one experiment
    from harness.sim_harness import Simulator

    Fh = min(args.host_frames, F)
    import tempfile

    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "track.csv")
        with open(path, "w") as f:
            f.write("frame,wrm_x,wrm_y,wrm_w,wrm_h\n")
            for i, r in enumerate(track[:Fh]):
                f.write(f"{i}," + ",".join("" if not np.isfinite(v) else repr(float(v)) for v in r) + "\n")
        ech = ExperimentConfig("timing", Fh, 60, (1600, 1400), 90, (1300, 1200))
        tch = TimingConfig(ech, 100, 40, 50, (4, 4), (0.32, 0.32))
        log = TrackLogger(PolyfitController(tch, cfgs[0], path))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            t0 = time.perf_counter()
            Simulator(tch, ech, log).run()
            out["host_loop_s"] = time.perf_counter() - t0
    out["host_frames"] = Fh
    out["host_loop_s_extrapolated_to_frames"] = out["host_loop_s"] * F / Fh
    print(json.dumps(out))


if __name__ == "__main__":
    main()
