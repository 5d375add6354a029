#!/usr/bin/env python3
"""Timing of ONE EPOCH of the closed-loop search on a SET of tracks (ReplaySet) against the same work done as one Replay per track
and a host loop around them (the only route before, unchanged since); prints one JSON line.

  epoch   targets of the swarm's positions + objective (what optimize_polyfit enqueues per epoch without the swarm step), P = 100 weight vectors, the
          notebook's sample times (-3L, -3L+6, -2L, -2L+6, -L, -L+6, 0, 3), degree 2, (200, 40, 50) ms at 60 frames/s, on T of --tracks tracks of
          --frames frames each (seeded random walks, 1 % NaN rows), on buffers allocated once:
            set    wtk_replay_polyfit_targets over the super-track + wtk_replay_set_objective: 5 launches whatever T is
            loop   per track wtk_replay_polyfit_targets + wtk_replay_objective (6 launches), T times
  mlp     one mlp_population + objective of E of --experiments models (the notebook's structure) on --mlp-tracks tracks, in both forms.
Device milliseconds by events around the enqueue and host wall milliseconds with the final synchronisation: median, min and max of --reps runs after a
warm-up, the two forms alternating.  `bits_equal`: the set's per-track objectives are the loop's.
Usage: python tools/replay_set_timing.py [--tracks 1 4 16] [--frames 60000] [--pop-size 100] [--experiments 16 256] [--mlp-tracks 4] [--reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--frames", type=int, default=60000)
    ap.add_argument("--pop-size", type=int, default=100)
    ap.add_argument("--experiments", type=int, nargs="*", default=[16, 256])
    ap.add_argument("--mlp-tracks", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()

    import torch

    from replay_mlp_timing import _alternate, random_model
    from replay_timing import random_walk
    from wtracker_amd import hip
    from wtracker_amd.replay import OBJECTIVES, Replay, ReplaySet
    from wtracker_amd.sim import ExperimentConfig, TimingConfig
    from wtracker_amd.training import HipMLPTrainer

    if hip.device_count() < 1:
        raise SystemExit("replay_set_timing: no HIP device visible (nothing is timed on the CPU)")
    F, P, degree, f64 = args.frames, args.pop_size, 2, torch.float64
    ec = ExperimentConfig("timing", F, 60, (1600, 1400), 90, (1300, 1200))
    tc = TimingConfig(ec, 200, 40, 50, (4, 4), (0.32, 0.32))
    n_max = max(args.tracks + [args.mlp_tracks])
    walks = [random_walk(F, seed=t) for t in range(n_max)]
    replays = [Replay(w, tc, ec) for w in walks]  # shared by every T: the loop form's objects
    L = replays[0].L
    times = tuple(sorted([-3 * L, -3 * L + 6, -2 * L, -2 * L + 6, -L, -L + 6, 0, 3]))
    dev = replays[0]._dev
    weights = torch.from_numpy(np.random.default_rng(1).uniform(0.05, 1.0, size=(P, len(times)))).to(dev)
    kind = OBJECTIVES["trimmed_bbox_error"]
    out = dict(pop_size=P, n_times=len(times), degree=degree, frames=F, cycles_per_track=replays[0].n_cycles, rows_per_track=replays[0].n_rows, reps=args.reps,
               epoch={}, mlp={})

    def loop_state(rp):
        tg, fit, classes = rp._population_buffers(P, times, degree, torch.zeros)
        return rp, tg, fit, classes, rp._objective_buffers(P), torch.empty((P,), dtype=f64, device=dev)

    states = [loop_state(rp) for rp in replays]
    for T in args.tracks:
        rs = ReplaySet(walks[:T], tc, ec)
        sp = rs._super
        tg, fit, classes = sp._population_buffers(P, times, degree, torch.zeros)
        buf, value, each = rs._objective_buffers(P), torch.empty((P,), dtype=f64, device=dev), torch.empty((T, P), dtype=f64, device=dev)

        def set_epoch():
            sp._enqueue_population(weights, degree, times, classes, tg.a, tg.valid, fit)
            rs._enqueue_objective(tg, kind, buf, value)

        def loop_epoch():
            for rp, ltg, lfit, lclasses, lbuf, lvalue in states[:T]:
                rp._enqueue_population(weights, degree, times, lclasses, ltg.a, ltg.valid, lfit)
                rp._enqueue_objective(ltg, kind, lbuf, lvalue)

        r = _alternate({"set": set_epoch, "loop": loop_epoch}, args.reps)
        rs._enqueue_objective(tg, kind, buf, value, each)  # (untimed: the per-track objectives, for the comparison)
        torch.cuda.synchronize()
        r["bits_equal"] = all(each[t].cpu().numpy().tobytes() == states[t][5].cpu().numpy().tobytes() for t in range(T))
        r["super_cycles"], r["classes_set"], r["classes_per_track"] = rs.n_super_cycles, int(classes[1].numel()), [int(s[3][1].numel()) for s in states[:T]]
        r["loop_over_set_device"] = r["loop"]["device_ms"]["median"] / r["set"]["device_ms"]["median"]
        r["loop_over_set_wall"] = r["loop"]["wall_ms"]["median"] / r["set"]["wall_ms"]["median"]
        out["epoch"][str(T)] = r

    T = args.mlp_tracks
    for E in args.experiments:
        trainer = HipMLPTrainer([random_model("notebook", 10 + e) for e in range(E)], max_batch=2)
        rs = ReplaySet(walks[:T], tc, ec)
        holder = {}

        def set_mlp():
            holder["set"] = rs.objective(rs.mlp_population(trainer), per_track=True)

        def loop_mlp():
            holder["loop"] = [rp.objective(rp.mlp_population(trainer)) for rp in replays[:T]]

        r = _alternate({"set": set_mlp, "loop": loop_mlp}, args.reps)
        torch.cuda.synchronize()
        r["bits_equal"] = all(holder["set"][t].cpu().numpy().tobytes() == holder["loop"][t].cpu().numpy().tobytes() for t in range(T))
        r["tracks"] = T
        r["loop_over_set_device"] = r["loop"]["device_ms"]["median"] / r["set"]["device_ms"]["median"]
        r["loop_over_set_wall"] = r["loop"]["wall_ms"]["median"] / r["set"]["wall_ms"]["median"]
        out["mlp"][str(E)] = r
        trainer.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
