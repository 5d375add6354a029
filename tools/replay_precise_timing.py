#!/usr/bin/env python3
"""Timing of the precise error of a replayed population (Replay.run(precise=True), wtk_replay_precise) against the route that was
there before it, in one process on one device; prints one JSON line.

  scenario    --frames gray frames of --size x --size (seeded noise over a flat background, resident on the device), a seeded random-walk track of
              about --box x --box pixel boxes, (100, 40, 50) ms at 60 frames/s, camera 4 mm and microscope 2 mm at 90 px/mm; per population size E of
              --experiments: E Polyfit experiments with distinct seeded weights.
  population  wtk_replay_precise on the scan's positions (summaries only): milliseconds by device events, median of --reps runs after one warm-up.
              `objective_ms`: Replay.objective(targets, "trimmed_precise_error"), the scan included.
  per_row     evaluation.precise_error once per experiment over the same rows (the replayed log's wrm / mic columns, already on the device): the E calls
              between one pair of device events, same median.  Each call ends in its frame-number check, which waits for the device.
  The per-row errors of both routes are compared bit for bit at every E before anything is timed; a difference ends the run.
  `bytes_min`: what the population call must move, from the shapes: the padded crop of every frame and of the background once (2 R (w + 2)(h + 2)), and
  per pair the cycle's position and move (16 B, shared by the L frames of a cycle only through the cache) and the error written and read once (16 B).
Usage: python tools/replay_precise_timing.py [--experiments 1 16 256] [--frames 1801] [--size 640] [--box 180] [--reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def walk_track(n: int, size: int, box: int, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(seed)
    centre = size / 2 + np.cumsum(rng.normal(0.0, 0.6, (n, 2)), axis=0)
    centre = size / 2 + (centre - size / 2) % (size / 8)  # folded back: the box stays inside the frame
    wh = box + rng.normal(0.0, 2.0, (n, 2))
    track = np.concatenate([centre - wh / 2, wh], axis=1)
    track[rng.random(n) < 0.01] = np.nan
    return track


def _time_ms(fn, reps: int) -> float:
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
    ap.add_argument("--experiments", type=int, nargs="+", default=[1, 16, 256])
    ap.add_argument("--frames", type=int, default=1801)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--box", type=int, default=180)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()

    import torch

    from wtracker_amd import evaluation, hip
    from wtracker_amd.controllers import PolyfitConfig
    from wtracker_amd.replay import Replay
    from wtracker_amd.sim import ExperimentConfig, TimingConfig

    if hip.device_count() < 1:
        raise SystemExit("replay_precise_timing: no HIP device visible (nothing is timed on the CPU)")
    F, S, thr = args.frames, args.size, 20
    track = walk_track(F, S, args.box)
    ec = ExperimentConfig("timing", F, 60, (S, S), 90, (S // 2, S // 2))
    tc = TimingConfig(ec, 100, 40, 50, (4, 4), (2, 2))
    rp = Replay(track, tc, ec, frame_shape=(S, S))
    gen = torch.Generator(device="cuda").manual_seed(0)
    frames = torch.empty((F, S, S), dtype=torch.uint8, device="cuda")
    for f0 in range(0, F, 64):  # (in chunks: the float32 draws of all frames at once would be four times the frames)
        frames[f0:f0 + 64] = (torch.rand((min(64, F - f0), S, S), device="cuda", generator=gen) < 0.15).to(torch.uint8) * 100 + 100
    bg = torch.full((S, S), 100, dtype=torch.uint8, device="cuda")
    rp.attach_frames(frames, bg, thr)
    dev, C, R = rp._dev, rp.n_cycles, rp.n_rows
    stream = torch.cuda.current_stream(dev).cuda_stream
    frame_nums = torch.arange(R, dtype=torch.int32, device=dev)
    area = float(np.nanmean((track[:R, 2] + 2) * (track[:R, 3] + 2)))
    out = dict(frames=F, size=S, box=args.box, rows=R, cycles=C, reps=args.reps, frames_bytes=int(frames.numel()), cases=[])
    rng = np.random.default_rng(1)
    for E in args.experiments:
        cfgs = [PolyfitConfig(2, [-9, -6, -3, 0, 2, 4], [float(v) for v in w]) for w in rng.uniform(0.05, 1.0, size=(E, 6))]
        tg = rp.polyfit(cfgs)
        res = rp.run(tg, rows=range(E), per_row_errors=True, precise=True)
        worm = torch.from_numpy(np.stack([res.row_array(e)[:, 10:14] for e in range(E)])).to(dev)  # [E, R, 4]
        mic = torch.from_numpy(np.stack([res.row_array(e)[:, 6:10] for e in range(E)])).to(dev)
        for e in range(E):  # faster and different is not faster
            old = evaluation.precise_error(frames, bg, worm[e], mic[e], frame_nums, thr).cpu().numpy()
            if old.view(np.int64).tolist() != res.precise_error[e].view(np.int64).tolist():
                raise SystemExit(f"replay_precise_timing: experiment {e} of {E} differs between the two routes")
        buf, pb = rp._objective_buffers(E), rp._precise_buffers(E)
        hip.replay_scan(rp._cfg, hip.REPLAY_POLYFIT, E, C, rp.track, rp.n_track, tg.a, None, tg.valid, rp._share, buf["pos"], buf["move"], stream=stream)
        population = lambda: hip.replay_precise(rp._cfg, E, C, rp.track, rp.n_track, rp._share, buf["pos"], buf["move"], frames, F, S, S, bg, thr, 0, None, None,  # noqa: E731
                                                pb["summary"], pb["scratch"], pb["scratch"].numel(), stream=stream)
        per_row = lambda: [evaluation.precise_error(frames, bg, worm[e], mic[e], frame_nums, thr) for e in range(E)]  # noqa: E731
        case = dict(experiments=E, population_ms=_time_ms(population, args.reps), per_row_ms=_time_ms(per_row, args.reps),
                    objective_ms=_time_ms(lambda: rp.objective(tg, "trimmed_precise_error"), args.reps))
        case["per_row_over_population"] = case["per_row_ms"] / case["population_ms"]
        case["bytes_min"] = int(2 * R * area + E * R * 32)
        case["mean_precise_error_min_max"] = [float(np.min(res.precise_summary.mean_precise_error)), float(np.max(res.precise_summary.mean_precise_error))]
        out["cases"].append(case)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
