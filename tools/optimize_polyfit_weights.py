#!/usr/bin/env python3
"""The reference's polyfit_optimizer.ipynb as a script: search the weights of the polynomial-fit controller on the device and write them as a
PolyfitConfig JSON file (keys degree, sample_times, weights: the layout of the reference's PolyfitConfig.save_json / load_json, so its
simulate.ipynb loads the file too; here `load_config(path)` gives the controllers.PolyfitConfig that PolyfitController / HipPolyfitController take).

  python tools/optimize_polyfit_weights.py EXPERIMENT_FOLDER_OR_BBOXES_CSV [more logs ...] --out polyfit_config.json
         [--fps 60] [--imaging-ms 200 --pred-ms 40 --moving-ms 50] [--offsets -45 -39 ...] [--pred-offset 21] [--degrees 1 2 3]
         [--min-speed 0.1 --max-speed 2] [--seed 0] [--pop-size 100 --max-epoch 300 --max-early-stop 100]

A folder stands for its bboxes.csv, and its exp_config.json supplies frames_per_sec when --fps is not given.  Defaults are the notebook's: with L the
cycle length in frames, offsets (-3L, -3L+6, -2L, -2L+6, -L, -L+6, 0, 3), target offset L + imaging_frames // 2, speed window 0.1 .. 2 px / frame.
With several --degrees every degree is searched (the notebook's "assess each degree"), one JSON result line is printed per degree, every degree's
config goes to <out stem>_deg<d>.json and the best one to --out.  Needs a GPU (there is no CPU fallback)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def save_config(cfg, path: str) -> None:
    with open(path, "w") as f:
        json.dump({"degree": int(cfg.degree), "sample_times": [int(t) for t in cfg.sample_times], "weights": [float(w) for w in cfg.weights]}, f, indent=4)


def load_config(path: str):
    from wtracker_amd.controllers import PolyfitConfig

    with open(path) as f:
        return PolyfitConfig(**json.load(f))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("logs", nargs="+", help="experiment folders (holding bboxes.csv) or bboxes.csv files")
    ap.add_argument("--out", required=True)
    ap.add_argument("--fps", type=float, default=None)
    ap.add_argument("--imaging-ms", type=float, default=200.0)
    ap.add_argument("--pred-ms", type=float, default=40.0)
    ap.add_argument("--moving-ms", type=float, default=50.0)
    ap.add_argument("--offsets", type=int, nargs="+", default=None)
    ap.add_argument("--pred-offset", type=int, default=None)
    ap.add_argument("--degrees", type=int, nargs="+", default=[1])
    ap.add_argument("--min-speed", type=float, default=0.1)
    ap.add_argument("--max-speed", type=float, default=2.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--pop-size", type=int, default=100)
    ap.add_argument("--max-epoch", type=int, default=300)
    ap.add_argument("--max-early-stop", type=int, default=100)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)

    from wtracker_amd.polyfit_opt import WeightEvaluator
    from wtracker_amd.sim import ExperimentConfig, TimingConfig

    paths, fps = [], args.fps
    for p in args.logs:
        if os.path.isdir(p):
            cfg = os.path.join(p, "exp_config.json")
            if fps is None and os.path.exists(cfg):
                fps = float(json.load(open(cfg))["frames_per_sec"])
            p = os.path.join(p, "bboxes.csv")
        paths.append(p)
    if fps is None:
        fps = 60.0
    ec = ExperimentConfig("weights", 0, fps, (0, 0), 1.0, (0, 0))
    tc = TimingConfig(ec, args.imaging_ms, args.pred_ms, args.moving_ms, (1, 1), (1, 1))
    L = tc.cycle_frame_num
    offsets = args.offsets if args.offsets is not None else [-3 * L, -3 * L + 6, -2 * L, -2 * L + 6, -L, -L + 6, 0, 3]
    pred = args.pred_offset if args.pred_offset is not None else L + tc.imaging_frame_num // 2
    ev = WeightEvaluator(paths, tc, offsets, pred, min_speed=args.min_speed, max_speed=args.max_speed, device=args.device)
    stem, ext = os.path.splitext(args.out)
    best = None
    for deg in args.degrees:
        res = ev.optimize(deg, pop_size=args.pop_size, max_epoch=args.max_epoch, max_early_stop=args.max_early_stop, seed=args.seed)
        cfg = ev.to_config(deg, res.weights)
        if len(args.degrees) > 1:
            save_config(cfg, f"{stem}_deg{deg}{ext}")
        print(json.dumps({"degree": deg, "mae": res.mae, "mae_uniform_weights": ev.eval([1.0] * len(offsets), deg), "epochs": res.epochs,
                          "series": ev.n_series, "cycles_per_log": ev.cycle_stats, "weights": cfg.weights}))
        if best is None or res.mae < best[0]:
            best = (res.mae, cfg)
    save_config(best[1], args.out)
    print(f"wrote {args.out}: degree {best[1].degree}, MAE {best[0]:.6g} px")


if __name__ == "__main__":
    main()
