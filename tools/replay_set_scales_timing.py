#!/usr/bin/env python3
"""Timing of ONE EPOCH of the closed-loop search on a ReplaySet whose tracks each have their own TimingConfig, beside the same
epoch on the uniform set (one TimingConfig, the entry points without a geometry table) and on one Replay per track with that track's config and a host
loop around them; prints one JSON line.

  epoch   what tools/replay_set_timing.py times: the targets of the swarm's positions + the pooled objective, P = 100 weight vectors, the notebook's
          sample times, degree 2, (200, 40, 50) ms at 60 frames/s, T tracks of --frames frames (seeded random walks), on buffers allocated once:
            uniform  ReplaySet(tracks, timing_config, ...): wtk_replay_set_objective
            scaled   ReplaySet.from_experiments at 88, 90, 92 px/mm in turn: wtk_replay_set_objective_geom, the same launches
            loop     per track Replay(track_t, timing_config_t, ...): wtk_replay_polyfit_targets + wtk_replay_objective, T times
Device milliseconds by events around the enqueue and host wall milliseconds with the final synchronisation: median, min and max of --reps runs after
a warm-up, the forms alternating.  `bits_equal`: the scaled set's per-track objectives are the loop's.
--uniform-only times the uniform form alone and uses nothing this feature added, so the same file runs on an older tree: --root PATH imports
wtracker_amd from that tree (a checkout of the parent commit with its library built), for the comparison with the commit before.
--scaled-only times the scaled form alone, for the comparison with --uniform-only without the other forms running in between.
Usage: python tools/replay_set_scales_timing.py [--tracks 3 12] [--frames 60000] [--pop-size 100] [--reps 7] [--uniform-only | --scaled-only] [--root PATH]
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, nargs="+", default=[3, 12])
    ap.add_argument("--frames", type=int, default=60000)
    ap.add_argument("--pop-size", type=int, default=100)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--uniform-only", action="store_true")
    ap.add_argument("--scaled-only", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(HERE))
    args = ap.parse_args()
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tools"))

    import torch

    from replay_mlp_timing import _alternate
    from replay_timing import random_walk
    from wtracker_amd import hip
    from wtracker_amd.replay import OBJECTIVES, Replay, ReplaySet
    from wtracker_amd.sim import ExperimentConfig, TimingConfig

    if hip.device_count() < 1:
        raise SystemExit("replay_set_scales_timing: no HIP device visible (nothing is timed on the CPU)")
    F, P, degree, f64 = args.frames, args.pop_size, 2, torch.float64
    n_max = max(args.tracks)
    ecs = [ExperimentConfig("timing", F, 60, (1600, 1400), (88, 90, 92)[t % 3], (1300, 1200)) for t in range(n_max)]
    timing, cam_mm, mic_mm = (200, 40, 50), (4, 4.1), (0.32, 0.33)
    tcs = [TimingConfig(ec, *timing, cam_mm, mic_mm) for ec in ecs]
    walks = [random_walk(F, seed=t) for t in range(n_max)]
    kind = OBJECTIVES["trimmed_bbox_error"]
    L = tcs[0].cycle_frame_num
    times = tuple(sorted([-3 * L, -3 * L + 6, -2 * L, -2 * L + 6, -L, -L + 6, 0, 3]))
    dev = torch.device("cuda", 0)
    weights = torch.from_numpy(np.random.default_rng(1).uniform(0.05, 1.0, size=(P, len(times)))).to(dev)
    out = dict(root=root, pop_size=P, frames=F, reps=args.reps, lib=hip.lib_path(), epoch={})

    def set_epoch_of(rs):
        sp = rs._super
        tg, fit, classes = sp._population_buffers(P, times, degree, torch.zeros)
        buf, value = rs._objective_buffers(P), torch.empty((P,), dtype=f64, device=dev)

        def epoch():
            sp._enqueue_population(weights, degree, times, classes, tg.a, tg.valid, fit)
            rs._enqueue_objective(tg, kind, buf, value)

        return epoch, (tg, buf, value)

    if args.uniform_only and args.scaled_only:
        ap.error("--uniform-only and --scaled-only exclude each other")
    replays = [] if args.uniform_only or args.scaled_only else [Replay(w, tc, ec) for w, tc, ec in zip(walks, tcs, ecs)]
    states = []
    for rp in replays:
        tg, fit, classes = rp._population_buffers(P, times, degree, torch.zeros)
        states.append((rp, tg, fit, classes, rp._objective_buffers(P), torch.empty((P,), dtype=f64, device=dev)))
    for T in args.tracks:
        fns = {}
        if not args.scaled_only:
            uniform = ReplaySet(walks[:T], tcs[0], ecs[0])
            fns["uniform"] = set_epoch_of(uniform)[0]
        if not args.uniform_only:
            scaled = ReplaySet.from_experiments(walks[:T], ecs[:T], *timing, cam_mm, mic_mm)
            fns["scaled"], (tg, buf, value) = set_epoch_of(scaled)
        if not (args.uniform_only or args.scaled_only):

            def loop_epoch():
                for rp, ltg, lfit, lclasses, lbuf, lvalue in states[:T]:
                    rp._enqueue_population(weights, degree, times, lclasses, ltg.a, ltg.valid, lfit)
                    rp._enqueue_objective(ltg, kind, lbuf, lvalue)

            fns["loop"] = loop_epoch
        r = _alternate(fns, args.reps)
        if not (args.uniform_only or args.scaled_only):
            each = torch.empty((T, P), dtype=f64, device=dev)
            scaled._enqueue_objective(tg, kind, buf, value, each)  # (untimed: the per-track objectives, for the comparison)
            torch.cuda.synchronize()
            r["bits_equal"] = all(each[t].cpu().numpy().tobytes() == states[t][5].cpu().numpy().tobytes() for t in range(T))
            r["scaled_over_uniform_device"] = r["scaled"]["device_ms"]["median"] / r["uniform"]["device_ms"]["median"]
            r["loop_over_scaled_device"] = r["loop"]["device_ms"]["median"] / r["scaled"]["device_ms"]["median"]
            r["loop_over_scaled_wall"] = r["loop"]["wall_ms"]["median"] / r["scaled"]["wall_ms"]["median"]
        out["epoch"][str(T)] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
