#!/usr/bin/env python3
"""The reference's polyfit_optimizer.ipynb as a script: search the weights of the polynomial-fit controller on the device and write them as a
PolyfitConfig JSON file (keys degree, sample_times, weights: the layout of the reference's PolyfitConfig.save_json / load_json, so its
simulate.ipynb loads the file too; here `load_config(path)` gives the controllers.PolyfitConfig that PolyfitController / HipPolyfitController take).

  python tools/optimize_polyfit_weights.py EXPERIMENT_FOLDER_OR_BBOXES_CSV [more logs ...] --out polyfit_config.json
         [--fps 60] [--imaging-ms 200 --pred-ms 40 --moving-ms 50] [--offsets -45 -39 ...] [--pred-offset 21] [--degrees 1 2 3]
         [--min-speed 0.1 --max-speed 2] [--seed 0] [--pop-size 100 --max-epoch 300 --max-early-stop 100]
         [--closed-loop EXP_CONFIG_JSON [one per log ...] [--camera-mm 4 4] [--micro-mm 0.32 0.32] [--precise FRAMES_NPY BACKGROUND_NPY [one pair per log ...]]]
         [--closed-loop-scales EXP_CONFIG_JSON one per log ...]

A folder stands for its bboxes.csv, and its exp_config.json supplies frames_per_sec when --fps is not given.  Defaults are the notebook's: with L the
cycle length in frames, offsets (-3L, -3L+6, -2L, -2L+6, -L, -L+6, 0, 3), target offset L + imaging_frames // 2, speed window 0.1 .. 2 px / frame.
With several --degrees every degree is searched (the notebook's "assess each degree"), one JSON result line is printed per degree, every degree's
config goes to <out stem>_deg<d>.json and the best one to --out.  Needs a GPU (there is no CPU fallback).

--closed-loop EXP_CONFIG_JSON (the reference's exp_config.json: num_frames, frames_per_sec, orig_resolution, px_per_mm, init_position) adds a second
search per degree whose objective is the tracking error of the closed loop itself (Replay.optimize_polyfit: the trimmed mean bbox error of the replayed
experiment), started from the open-loop winner, so its result is never worse than that winner in the loop.  With several logs the experiments are
replayed together and the error is pooled over the rows of all of them (ReplaySet.optimize_polyfit); give one EXP_CONFIG_JSON for all logs or one per log.  The result line then
also holds `closed_loop_error_of_open_loop_weights`, `closed_loop_error` and `closed_loop_weights`, and the closed-loop config of the best degree goes to
<out stem>_closed_loop.json.  The closed-loop error is piecewise constant in the weights (moves are whole pixels).  Without the option nothing changes.
With --precise FRAMES_NPY BACKGROUND_NPY (the experiment's gray frames, uint8 [F, H, W] with F >= the logged rows, and its background [H, W]) the
closed-loop objective is the trimmed mean PRECISE error instead (Replay.attach_frames; the frames are held on the device and give the frame shape).
With several logs give one FRAMES_NPY BACKGROUND_NPY pair per log, in the logs' order: the search runs on the ReplaySet with every log's frames
attached (ReplaySet.attach_frames) and the precise error is pooled over the rows of all logs.

--closed-loop-scales EXP_CONFIG_JSON ... (one per log, in the logs' order; in the place of --closed-loop) is for logs recorded at DIFFERENT px_per_mm: every
log gets the TimingConfig of its own exp_config.json, so --camera-mm and --micro-mm become that log's own camera and microscope in pixels
(ReplaySet.from_experiments), where --closed-loop replays every log with the pixel sizes of the first exp_config.json.  The
frame counts of --imaging-ms / --pred-ms / --moving-ms must come out equal for all logs (recordings at one frame rate)."""
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
    ap.add_argument("--closed-loop", default=None, nargs="+", metavar="EXP_CONFIG_JSON")
    ap.add_argument("--closed-loop-scales", default=None, nargs="+", metavar="EXP_CONFIG_JSON")
    ap.add_argument("--camera-mm", type=float, nargs=2, default=[4.0, 4.0])
    ap.add_argument("--micro-mm", type=float, nargs=2, default=[0.32, 0.32])
    ap.add_argument("--precise", nargs="+", default=None, metavar="FRAMES_NPY BACKGROUND_NPY")
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
    rp = best_closed = None
    objective = "trimmed_bbox_error"
    per_log = args.closed_loop_scales is not None
    if per_log:
        if args.closed_loop is not None:
            ap.error("--closed-loop-scales stands in the place of --closed-loop: give one of them")
        if len(args.closed_loop_scales) != len(paths):
            ap.error(f"--closed-loop-scales takes one exp_config.json per log ({len(paths)})")
        args.closed_loop = args.closed_loop_scales
    if args.precise is not None and args.closed_loop is None:
        ap.error("--precise goes with --closed-loop")
    if args.closed_loop is not None:
        from wtracker_amd.replay import Replay, ReplaySet

        if len(args.closed_loop) not in (1, len(paths)):
            ap.error(f"--closed-loop takes one exp_config.json for all logs or one per log ({len(paths)})")
        if args.precise is not None and len(args.precise) != 2 * len(paths):
            ap.error(f"--precise takes one FRAMES_NPY BACKGROUND_NPY pair per log ({len(paths)} logs: {2 * len(paths)} files)")
        exps = [ExperimentConfig.from_dict(json.load(open(c))) for c in args.closed_loop]
        exp = exps[0]
        loop_tc = TimingConfig(exp, args.imaging_ms, args.pred_ms, args.moving_ms, tuple(args.camera_mm), tuple(args.micro_mm))
        frames = None
        if args.precise is not None:
            import numpy as np
            import torch

            frames = [torch.from_numpy(np.load(p)).to(f"cuda:{args.device}") for p in args.precise[0::2]]
            backgrounds, objective = [np.load(p) for p in args.precise[1::2]], "trimmed_precise_error"
        if len(paths) > 1:
            shapes = None if frames is None else [tuple(fr.shape[1:3]) for fr in frames]
            if per_log:  # every log with the TimingConfig of its own recording
                rp = ReplaySet.from_experiments(paths, exps, args.imaging_ms, args.pred_ms, args.moving_ms, tuple(args.camera_mm), tuple(args.micro_mm),
                                                frame_shapes=shapes, device=args.device)
            else:
                rp = ReplaySet(paths, loop_tc, exp if len(exps) == 1 else exps, shapes, device=args.device)
            if frames is not None:
                rp.attach_frames(frames, backgrounds)
        else:
            rp = Replay(paths[0], loop_tc, exp, frame_shape=None if frames is None else frames[0].shape[1:3], device=args.device)
            if frames is not None:
                rp.attach_frames(frames[0], backgrounds[0])
    for deg in args.degrees:
        res = ev.optimize(deg, pop_size=args.pop_size, max_epoch=args.max_epoch, max_early_stop=args.max_early_stop, seed=args.seed)
        cfg = ev.to_config(deg, res.weights)
        if len(args.degrees) > 1:
            save_config(cfg, f"{stem}_deg{deg}{ext}")
        line = {"degree": deg, "mae": res.mae, "mae_uniform_weights": ev.eval([1.0] * len(offsets), deg), "epochs": res.epochs,
                "series": ev.n_series, "cycles_per_log": ev.cycle_stats, "weights": cfg.weights}
        if rp is not None:
            closed = rp.optimize_polyfit(deg, cfg.sample_times, objective=objective, pop_size=args.pop_size, max_epoch=args.max_epoch, max_early_stop=args.max_early_stop,
                                         seed=args.seed, start=[res.weights])
            of_open = float(rp.objective(rp.polyfit_population([cfg.weights], deg, cfg.sample_times), objective).cpu().numpy()[0])
            line.update(closed_loop_error_of_open_loop_weights=of_open, closed_loop_error=closed.mae, closed_loop_epochs=closed.epochs,
                        closed_loop_weights=[float(w) for w in closed.weights])
            if best_closed is None or closed.mae < best_closed[0]:
                best_closed = (closed.mae, rp.to_config(deg, closed.weights, cfg.sample_times))
        print(json.dumps(line))
        if best is None or res.mae < best[0]:
            best = (res.mae, cfg)
    save_config(best[1], args.out)
    print(f"wrote {args.out}: degree {best[1].degree}, MAE {best[0]:.6g} px")
    if best_closed is not None:
        save_config(best_closed[1], f"{stem}_closed_loop{ext}")
        print(f"wrote {stem}_closed_loop{ext}: degree {best_closed[1].degree}, closed-loop {objective.replace('_', ' ')} {best_closed[0]:.6g}")


if __name__ == "__main__":
    main()
