#!/usr/bin/env python3
"""Timing of the YOLO controller's closed loop from device-resident state (wtracker_amd.replay.YoloReplay) beside the host frame loop
it replaces, in one process on one box; prints one JSON line.

The reference's operating point as bench.py's closed-loop leg sets it up: synthetic 1024 x 1024 gray frames resident in HBM, 360 x 360 camera views
letterboxed to imgsz 384, (200, 40, 50) ms at 60 frames/s = 15-frame cycles, synthetic "s" weights, dtype f16x3, plan "auto".

  yolo_replay_log_batch_<n>   ms per cycle of YoloReplay.run(): wall clock around a run and its one synchronisation, downloads of the result included,
                              after one untimed run; log_batch = the cycle length (the host loop's cycle batch) and --log-batch (a throughput-plan handle)
  host_loop, host_loop_deferred_log   the same experiment under tests/harness' Simulator with TrackLogger / TrackLogger(deferred=True): wall clock of the
                              whole run over the cycles, after one untimed run
Every variant is run --reps times, ALTERNATING (a b c d, a b c d, ...) so that drift of the box hits all of them alike; reported are the runs, their median
and their spread (max - min).  `faster` is only claimed where the gain exceeds the spreads of both sides.
Usage: python tools/replay_yolo_timing.py [--cycles 30] [--reps 3] [--log-batch 256] [--conf 0.1]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cycles", type=int, default=30)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--log-batch", type=int, default=256)
    ap.add_argument("--conf", type=float, default=0.1)
    args = ap.parse_args()

    import torch

    from harness.sim_harness import ArrayReader, Simulator
    from wtracker_amd import frames as fr
    from wtracker_amd import hip
    from wtracker_amd import yolo_spec as ys
    from wtracker_amd.controllers import HipYoloController, YoloConfig
    from wtracker_amd.replay import YoloReplay
    from wtracker_amd.sim import ExperimentConfig, TimingConfig, TrackLogger

    if hip.device_count() < 1:
        raise SystemExit("replay_yolo_timing: no HIP device visible (nothing is timed on the CPU)")
    size, cycles = 1024, args.cycles
    ec = ExperimentConfig("closed_loop", cycles * 15 + 1, 60, (size, size), 90, (size // 2, size // 2))
    tc = TimingConfig(ec, 200, 40, 50, (4, 4), (0.32, 0.32))
    assert (tc.imaging_frame_num, tc.pred_frame_num, tc.moving_frame_num, tc.cycle_frame_num, tc.camera_size_px) == (12, 3, 3, 15, (360, 360))
    frames_np, _ = fr.synthetic_frames(ec.num_frames, size, seed=77)
    dev_frames = torch.from_numpy(frames_np).cuda()
    tmp = tempfile.NamedTemporaryFile(suffix=".wtk", delete=False)
    tmp.close()
    ys.save_weights(tmp.name, ys.synthetic_weights("s", 1, seed=0), "s", 1)
    cfg = YoloConfig(model_path=tmp.name, device="cuda", pred_kwargs={"imgsz": 384, "conf": args.conf}, dtype="f16x3", scale="s", max_batch=16, plan="auto")

    results = {}

    def host(deferred):
        log = TrackLogger(HipYoloController(tc, cfg, device_frames=dev_frames), deferred=deferred)
        t0 = time.perf_counter()
        Simulator(tc, ec, log, reader=ArrayReader(frames_np)).run()
        dt = time.perf_counter() - t0
        results["host_rows"] = log.rows
        return dt * 1e3 / cycles

    def replay(yr, key):
        t0 = time.perf_counter()
        res = yr.run()
        dt = time.perf_counter() - t0
        results[key] = res
        return dt * 1e3 / cycles

    yr_l = YoloReplay(dev_frames, tc, ec, cfg)
    yr_b = YoloReplay(dev_frames, tc, ec, cfg, log_batch=args.log_batch)
    name_l, name_b = f"yolo_replay_log_batch_{yr_l.log_batch}", f"yolo_replay_log_batch_{yr_b.log_batch}"
    variants = [(name_l, lambda: replay(yr_l, "res_l")), (name_b, lambda: replay(yr_b, "res_b")), ("host_loop", lambda: host(False)),
                ("host_loop_deferred_log", lambda: host(True))]
    for _, fn in variants:  # one untimed run each: buffers, the controllers' first calls
        fn()
    runs = {name: [] for name, _ in variants}
    for _ in range(args.reps):
        for name, fn in variants:
            runs[name].append(fn())
    out = dict(what="ms per cycle, wall clock, host included; alternating runs in one process", cycles=cycles, cycle_frames=15, reps=args.reps,
               frames=f"{ec.num_frames} synthetic {size}x{size} uint8 gray frames in HBM, camera view 360x360 -> imgsz 384, conf {args.conf}, f16x3, plan auto",
               device=torch.cuda.get_device_name(0))
    for name, v in runs.items():
        out[name] = dict(ms_per_cycle_runs=[round(x, 4) for x in v], ms_per_cycle_median=round(float(np.median(v)), 4), spread=round(max(v) - min(v), 4))
    # the same experiment: the replay at the cycle batch's size logs the host loop's rows
    mine, rows = results["res_l"].log(0), results["host_rows"]
    out["rows_equal_host_loop"] = len(mine) == len(rows) and all(
        all(float(a[k]) == float(b[k]) for k in ("plt_x", "plt_y", "wrm_x", "wrm_y", "wrm_w", "wrm_h")) for a, b in zip(mine, rows))
    out["moves_equal_across_log_batches"] = bool(np.array_equal(results["res_l"].moves, results["res_b"].moves))
    best_host = min(("host_loop", "host_loop_deferred_log"), key=lambda n: out[n]["ms_per_cycle_median"])
    for name in (name_l, name_b):
        gain = out[best_host]["ms_per_cycle_median"] - out[name]["ms_per_cycle_median"]
        out[name]["gain_over_" + best_host] = round(gain, 4)
        out[name]["faster"] = bool(gain > max(out[name]["spread"], out[best_host]["spread"]))
    yr_b.close()
    os.unlink(tmp.name)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
