#!/usr/bin/env python3
"""Timing of the PRECISE objective of a population on a SET of tracks (ReplaySet after attach_frames) against the same work done
as one Replay per track and a host loop around them (the only route before, unchanged since); prints one JSON line.

  scenario   per track --frames gray frames of --size x --size (seeded noise over a flat background, resident on the device) and a seeded random-walk
             track of about --box x --box pixel boxes, (100, 40, 50) ms at 60 frames/s, camera 4 mm and microscope 2 mm at 90 px/mm; E of --experiments
             Polyfit weight vectors; T of --tracks tracks.
  objective  one evaluation of "trimmed_precise_error" on buffers allocated once:
               set    wtk_replay_set_precise_objective: 5 launches whatever T is
               loop   per track wtk_replay_precise_objective (5 launches), T times; at T = 1 this is Replay.objective on that track
  epoch      one swarm epoch without the swarm step: the Polyfit targets of the positions, then the objective, in both forms.
Device milliseconds by events around the enqueue and host wall milliseconds with the final synchronisation: median, min and max of --reps runs after a
warm-up, the two forms alternating.  `bits_equal`: the set's per-track objectives are the loop's, checked at the timed sizes before anything is timed.
  --single   times Replay.objective(..., "trimmed_precise_error") on track 0 alone and nothing else: the same script runs on a checkout without ReplaySet's
             precise error, for an A/B of two builds in alternating processes.
Usage: python tools/replay_set_precise_timing.py [--tracks 1 4 16] [--frames 1801] [--size 400] [--box 180] [--experiments 100] [--reps 5] [--single]
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


def _alternate(fns: dict, reps: int) -> dict:
    """name -> dict(wall_ms, device_ms: median, min, max) of each fn() + one synchronisation, the functions alternating, after one warm-up each."""
    import torch

    for fn in fns.values():
        fn()
        torch.cuda.synchronize()
    wall, dev = {k: [] for k in fns}, {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            wall[k].append((time.perf_counter() - t0) * 1e3)
            dev[k].append(a.elapsed_time(b))
    stat = lambda v: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))  # noqa: E731
    return {k: dict(wall_ms=stat(wall[k]), device_ms=stat(dev[k])) for k in fns}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--frames", type=int, default=1801)
    ap.add_argument("--size", type=int, default=400)
    ap.add_argument("--box", type=int, default=180)
    ap.add_argument("--experiments", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--single", action="store_true")
    args = ap.parse_args()

    import torch

    from replay_precise_timing import walk_track
    from wtracker_amd import hip
    from wtracker_amd.replay import PRECISE_OBJECTIVES, Replay
    from wtracker_amd.sim import ExperimentConfig, TimingConfig

    if hip.device_count() < 1:
        raise SystemExit("replay_set_precise_timing: no HIP device visible (nothing is timed on the CPU)")
    F, S, E, thr, degree, f64 = args.frames, args.size, args.experiments, 20, 2, torch.float64
    times = (-9, -6, -3, 0, 2, 4)
    ec = ExperimentConfig("timing", F, 60, (S, S), 90, (S // 2, S // 2))
    tc = TimingConfig(ec, 100, 40, 50, (4, 4), (2, 2))
    n_max = 1 if args.single else max(args.tracks)
    gen = torch.Generator(device="cuda").manual_seed(0)
    bg = torch.full((S, S), 100, dtype=torch.uint8, device="cuda")
    walks, frames, replays = [], [], []
    for t in range(n_max):
        fr = torch.empty((F, S, S), dtype=torch.uint8, device="cuda")
        for f0 in range(0, F, 64):  # (in chunks: the float32 draws of all frames at once would be four times the frames)
            fr[f0:f0 + 64] = (torch.rand((min(64, F - f0), S, S), device="cuda", generator=gen) < 0.15).to(torch.uint8) * 100 + 100
        walks.append(walk_track(F, S, args.box, seed=t)), frames.append(fr)
        replays.append(Replay(walks[t], tc, ec, frame_shape=(S, S)))
        replays[t].attach_frames(fr, bg, thr)
    dev = replays[0]._dev
    weights = torch.from_numpy(np.random.default_rng(1).uniform(0.05, 1.0, size=(E, len(times)))).to(dev)
    kind = PRECISE_OBJECTIVES["trimmed_precise_error"]
    out = dict(frames=F, size=S, box=args.box, experiments=E, rows_per_track=replays[0].n_rows, reps=args.reps, lib=os.path.basename(hip.lib_path()))

    def loop_state(rp):
        tg, fit, classes = rp._population_buffers(E, times, degree, torch.zeros)
        return rp, tg, fit, classes, rp._all_objective_buffers(E, True), torch.empty((E,), dtype=f64, device=dev)

    states = [loop_state(rp) for rp in replays]
    for rp, tg, fit, classes, _, _ in states:
        rp._enqueue_population(weights, degree, times, classes, tg.a, tg.valid, fit)
    torch.cuda.synchronize()

    def loop_objective(T):
        for rp, tg, _, _, buf, value in states[:T]:
            rp._enqueue_objective(tg, kind, buf, value)

    def loop_epoch(T):
        for rp, tg, fit, classes, buf, value in states[:T]:
            rp._enqueue_population(weights, degree, times, classes, tg.a, tg.valid, fit)
            rp._enqueue_objective(tg, kind, buf, value)

    if args.single:
        out["single"] = _alternate({"objective": lambda: loop_objective(1)}, args.reps)["objective"]
        print(json.dumps(out))
        return

    from wtracker_amd.replay import ReplaySet

    out["cases"] = {}
    for T in args.tracks:
        rs = ReplaySet(walks[:T], tc, ec, [(S, S)] * T)
        rs.attach_frames(frames[:T], [bg] * T, thr)
        sp = rs._super
        tg, fit, classes = sp._population_buffers(E, times, degree, torch.zeros)
        buf, value, each = rs._objective_buffers(E, True), torch.empty((E,), dtype=f64, device=dev), torch.empty((T, E), dtype=f64, device=dev)
        sp._enqueue_population(weights, degree, times, classes, tg.a, tg.valid, fit)
        rs._enqueue_objective(tg, kind, buf, value, each)
        loop_objective(T)
        torch.cuda.synchronize()
        if not all(each[t].cpu().numpy().tobytes() == states[t][5].cpu().numpy().tobytes() for t in range(T)):  # faster and different is not faster
            raise SystemExit(f"replay_set_precise_timing: the set's per-track objectives differ from the loop's at T = {T}")

        def set_epoch():
            sp._enqueue_population(weights, degree, times, classes, tg.a, tg.valid, fit)
            rs._enqueue_objective(tg, kind, buf, value)

        r = dict(bits_equal=True, rows=sum(rs.n_rows))
        r["objective"] = _alternate({"set": lambda: rs._enqueue_objective(tg, kind, buf, value), "loop": lambda: loop_objective(T)}, args.reps)
        r["epoch"] = _alternate({"set": set_epoch, "loop": lambda: loop_epoch(T)}, args.reps)
        for k in ("objective", "epoch"):
            r[k]["loop_over_set_device"] = r[k]["loop"]["device_ms"]["median"] / r[k]["set"]["device_ms"]["median"]
            r[k]["loop_over_set_wall"] = r[k]["loop"]["wall_ms"]["median"] / r[k]["set"]["wall_ms"]["median"]
        out["cases"][str(T)] = r
        del rs, buf
    print(json.dumps(out))


if __name__ == "__main__":
    main()
