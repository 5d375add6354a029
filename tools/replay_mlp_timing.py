#!/usr/bin/env python3
"""Timing of the closed-loop selection of a trained ResMLP population (Replay.mlp_population) against the loop that existed before
it; prints one JSON line.

  select   rp.objective(rp.mlp_population(trainer, which="best")) followed by one synchronisation, against the README's former loop
           [rp.run(rp.mlp(trainer.folded(e, best=True))) for e in range(E)] (per model: every model's state copied to the host, a numpy fold, a wtk_mlp
           handle, one launch, one synchronisation).  Wall and device milliseconds, the two alternating, --reps times after one warm-up each: median and
           (min, max).  The loop runs the code of the parent commit unchanged, so it is timed in this process.  Above --loop-max-e models the loop is timed
           on the first --loop-max-e of them and scaled by E / --loop-max-e in `loop_wall_ms_scaled` (every turn copies all E states, so the scaled figure
           is what the measured turns cost; the unscaled run would take minutes).
  kernel   wtk_replay_mlp_targets alone on a folded blob (device ms by events), per (model, cycle) and per 16-sample tile of a wave, next to one
           wtk_mlp_predict_track call of the per-model path on the same track; the waves per workgroup of the blob.
  fit      one epoch of HipMLPTrainer.fit with and without closed_loop (E of --experiments, --fit-cycles cycles), wall ms with the final synchronisation.
Models: "notebook" (28 -> 80, [40, 10, 40, 80] x 4, one predicted frame: 150 KB blob, read from global memory), "100ms" and "200ms" (the structures of the
shipped predictors: 33 KB and 105 KB blobs, in LDS), seeded random parameters.  Track: the seeded random walk of tools/replay_timing.py.
Usage: python tools/replay_mlp_timing.py [--experiments 1 16 256] [--cycles 120 4000] [--models notebook 100ms 200ms] [--reps 5]
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

MODELS = {  # name -> (residual width, block widths, blocks, input frames, predicted frame)
    "notebook": (80, [40, 10, 40, 80], 4, [0, -2, -9, -11, -18, -20, -27], 9),
    "100ms": (40, [10, 4, 10, 40], 4, [0, -2, -9, -11, -18, -20, -27], 9),
    "200ms": (60, [20, 8, 20, 60], 6, [0, -3, -15, -18, -30, -33, -45], 12),
}


def random_model(name: str, seed: int) -> dict:
    """A state dict of the structure with Linear + BatchNorm1d + ReLU layers and small random parameters (outputs of a few pixels)."""
    width, dims, n_blocks, xi, yi = MODELS[name]
    rng = np.random.default_rng(seed)
    sd = {}

    def layer(prefix, k, n):
        sd[prefix + ".0.weight"] = (rng.normal(0, 1, (n, k)) * 0.3 / np.sqrt(k)).astype(np.float32)
        sd[prefix + ".0.bias"] = rng.normal(0, 0.1, n).astype(np.float32)
        sd[prefix + ".1.weight"] = rng.uniform(0.5, 1.5, n).astype(np.float32)
        sd[prefix + ".1.bias"] = rng.normal(0, 0.1, n).astype(np.float32)
        sd[prefix + ".1.running_mean"] = rng.normal(0, 0.2, n).astype(np.float32)
        sd[prefix + ".1.running_var"] = rng.uniform(0.5, 2.0, n).astype(np.float32)
        sd[prefix + ".1.num_batches_tracked"] = np.asarray(0, np.int64)

    layer("model.input.mlp_layer", 4 * len(xi), width)
    for b in range(n_blocks):
        k = width
        for l, n in enumerate(dims):
            layer(f"model.blocks.{b}.sequence.{l}.mlp_layer", k, n)
            k = n
    sd["model.output.weight"] = (rng.normal(0, 1, (2, width)) / np.sqrt(width)).astype(np.float32)
    sd["model.output.bias"] = rng.normal(0, 0.3, 2).astype(np.float32)
    return dict(sd, activations=["relu"] * (1 + n_blocks * len(dims)), input_frames=xi, pred_frames=[yi])


def _alternate(fns: dict, reps: int) -> dict:
    """name -> dict(wall_ms, device_ms: median, spread: (min, max)) of each fn() + one synchronisation, the functions alternating."""
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
    ap.add_argument("--experiments", type=int, nargs="+", default=[1, 16, 256])
    ap.add_argument("--cycles", type=int, nargs="+", default=[120, 4000])
    ap.add_argument("--models", nargs="+", default=["notebook", "100ms", "200ms"], choices=sorted(MODELS))
    ap.add_argument("--select-model", default="notebook", choices=sorted(MODELS))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-max-e", type=int, default=16)
    ap.add_argument("--fit-cycles", type=int, default=120)
    ap.add_argument("--skip", nargs="*", default=[], choices=["select", "kernel", "fit"])
    args = ap.parse_args()

    import torch

    from replay_timing import random_walk
    from wtracker_amd import hip
    from wtracker_amd.replay import Replay
    from wtracker_amd.sim import ExperimentConfig, TimingConfig
    from wtracker_amd.training import HipMLPTrainer

    if hip.device_count() < 1:
        raise SystemExit("replay_mlp_timing: no HIP device visible (nothing is timed on the CPU)")

    def replay(cycles: int, imaging_ms: int = 100):
        ec0 = ExperimentConfig("timing", 1000, 60, (1600, 1400), 90, (1300, 1200))
        L = TimingConfig(ec0, imaging_ms, 40, 50, (4, 4), (0.32, 0.32)).cycle_frame_num
        F = cycles * L + 1
        ec = ExperimentConfig("timing", F, 60, (1600, 1400), 90, (1300, 1200))
        return Replay(random_walk(F), TimingConfig(ec, imaging_ms, 40, 50, (4, 4), (0.32, 0.32)), ec)

    out = dict(reps=args.reps, select=[], kernel=[], fit=[])
    # ---- model selection: the one-call form against the per-model loop
    if "select" not in args.skip:
        for cycles in args.cycles:
            rp = replay(cycles)
            for E in args.experiments:
                t = HipMLPTrainer([random_model(args.select_model, 10 + e) for e in range(E)], max_batch=2)
                n_loop = min(E, args.loop_max_e)
                holder = {}

                def one_call():
                    holder["pop"] = rp.objective(rp.mlp_population(t, which="best"))

                def loop():
                    holder["loop"] = [rp.run(rp.mlp(t.folded(e, best=True), max_speed=0.9)) for e in range(n_loop)]

                r = _alternate(dict(population=one_call, loop=loop), args.reps)
                pop = holder["pop"].cpu().numpy()
                same = all(pop[e] == holder["loop"][e].summary.trimmed_mean_bbox_error[0] for e in range(n_loop))
                out["select"].append(dict(model=args.select_model, experiments=E, cycles=rp.n_cycles, loop_models=n_loop, population=r["population"], loop=r["loop"],
                                          loop_wall_ms_scaled=r["loop"]["wall_ms"]["median"] * E / n_loop,
                                          speedup_wall=r["loop"]["wall_ms"]["median"] * E / n_loop / r["population"]["wall_ms"]["median"], objective_bits_equal=bool(same)))
                t.close()
    # ---- the kernel itself
    if "kernel" not in args.skip:
        for name in args.models:
            rp = replay(max(args.cycles), 200 if name == "200ms" else 100)
            for E in args.experiments:
                t = HipMLPTrainer([random_model(name, 10 + e) for e in range(E)], max_batch=2)
                blob = t.folded_blob("current")
                tg = rp.mlp_population(t)  # (allocates the outputs and the float32 track once)
                layers, n_blocks, per_block = t.blob_structure()
                xi = MODELS[name][3]
                bound = 12.0
                st = torch.cuda.current_stream().cuda_stream

                def kernel():
                    hip.replay_mlp_targets(layers, n_blocks, per_block, blob, E, rp._track_f32, rp.track, rp.n_track, rp._anchors, rp.n_cycles, xi, bound, tg.a, tg.b,
                                           tg.valid, stream=st)

                net = hip.HipMLP(t.folded(0).layers, t.n_blocks, t.layers_per_block)
                pred = torch.zeros((rp.n_cycles, 2), dtype=torch.float32, device="cuda")
                ok = torch.zeros((rp.n_cycles,), dtype=torch.int32, device="cuda")

                def per_model():
                    net.predict_track(rp._track_f32, rp.n_track, rp._anchors, rp.n_cycles, xi, pred, ok, stream=st)

                r = _alternate(dict(population=kernel, per_model=per_model), args.reps)
                ms, one = r["population"]["device_ms"]["median"], r["per_model"]["device_ms"]["median"]
                waves = hip.replay_mlp_targets_waves(int(blob.shape[1]))
                out["kernel"].append(dict(model=name, blob_bytes=int(blob.shape[1]) * 4, waves_per_workgroup=waves, experiments=E, cycles=rp.n_cycles,
                                          population_device_ms=r["population"]["device_ms"], us_per_model_cycle=1e3 * ms / (E * rp.n_cycles),
                                          per_model_call_device_ms=r["per_model"]["device_ms"], per_model_path_ms_for_E=one * E, kernel_speedup=one * E / ms))
                t.close()
    # ---- scoring during fit
    if "fit" not in args.skip:
        rp = replay(args.fit_cycles)
        n, B = 2048, 128
        for E in args.experiments:
            if E == 1:
                continue
            torch.manual_seed(0)
            X, y = torch.randn((n, 28), device="cuda") * 6, torch.randn((n, 2), device="cuda")
            t = HipMLPTrainer([random_model(args.select_model, 10 + e) for e in range(E)], max_batch=B)

            def plain():
                t.fit(X, y, X[:512].contiguous(), y[:512].contiguous(), 1, batch_size=B, shuffle=False)

            def scored():
                t.fit(X, y, X[:512].contiguous(), y[:512].contiguous(), 1, batch_size=B, shuffle=False, closed_loop=rp)

            r = _alternate(dict(plain=plain, closed_loop=scored), args.reps)
            out["fit"].append(dict(model=args.select_model, experiments=E, cycles=rp.n_cycles, rows=n, batch=B, plain=r["plain"]["wall_ms"], closed_loop=r["closed_loop"]["wall_ms"],
                                   added_ms=r["closed_loop"]["wall_ms"]["median"] - r["plain"]["wall_ms"]["median"]))
            t.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
