#!/usr/bin/env python3
"""Timing of the experiment evaluation kernels (csrc/eval_ops.hip) at the reference's experiment scale; prints one JSON line.

  background   1000 probes of 1500 x 1500 gray (2.25 GB of frames in device memory), median and mean: milliseconds by device events (median of
               --reps runs after one warm-up) and the effective rate counting the bytes the kernel must read: 2 n H W for the median (two
               passes), n H W for the mean.  copy_GBps: a device-to-device copy of the same frames (read + write bytes over time), the rate the
               streaming kernels are held against.
  precise      60 000 log rows of head-sized boxes (about 14 x 15 px) on those frames, diff_thresh 10: milliseconds by device events.
  host         numpy's median / mean (BGExtractor's arithmetic) on a band of --host-rows image rows of the same probes, in seconds, and scaled
               linearly to the whole frame (labelled as extrapolated).
Usage: python tools/eval_timing.py [--probes 1000] [--size 1500] [--rows 60000] [--reps 5] [--host-rows 150]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    ap.add_argument("--probes", type=int, default=1000)
    ap.add_argument("--size", type=int, default=1500)
    ap.add_argument("--rows", type=int, default=60000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-rows", type=int, default=150)
    args = ap.parse_args()

    import torch

    from wtracker_amd import evaluation as ev
    from wtracker_amd import hip

    if hip.device_count() < 1:
        raise SystemExit("eval_timing: no HIP device visible (nothing is timed on the CPU)")
    n, S = args.probes, args.size
    g = torch.Generator(device="cuda").manual_seed(0)
    frames = torch.randint(0, 256, (n, S, S), dtype=torch.uint8, device="cuda", generator=g)
    nbytes = n * S * S
    out = {"probes": n, "frame": [S, S], "frame_bytes_total": nbytes}
    for method, passes in (("median", 2), ("mean", 1)):
        ms = _time_ms(lambda: ev.background(frames, n, "uniform", method), args.reps)
        out[f"bg_{method}_ms"] = round(ms, 3)
        out[f"bg_{method}_GBps"] = round(passes * nbytes / ms / 1e6, 1)
    dst = torch.empty_like(frames)
    ms = _time_ms(lambda: dst.copy_(frames), args.reps)
    out["copy_GBps"] = round(2 * nbytes / ms / 1e6, 1)
    del dst

    rng = np.random.default_rng(1)
    N = args.rows
    worm = np.concatenate([rng.uniform(0, S - 20, (N, 2)), rng.normal((13.8, 14.6), 0.6, (N, 2))], axis=1)
    mic = worm + rng.uniform(-4, 4, (N, 4))
    fn = rng.integers(0, n, N)
    bg = ev.background(frames, n, "uniform", "median")
    wd, md = torch.from_numpy(worm).cuda(), torch.from_numpy(mic).cuda()
    fd = torch.from_numpy(fn.astype(np.int32)).cuda()
    err = torch.empty(N, dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ms = _time_ms(lambda: hip.precise_error(frames, n, S, S, bg, wd, md, fd, N, 10.0, err, None, None, stream), args.reps)
    out["precise_rows"] = N
    out["precise_ms"] = round(ms, 3)

    hr = min(args.host_rows, S)
    band = frames[:, :hr, :].cpu().numpy()
    t = time.perf_counter()
    np.median(band, axis=0).astype(np.uint8)
    t_med = time.perf_counter() - t
    t = time.perf_counter()
    s = np.zeros(band.shape[1:], np.float64)
    for f in band:
        s += f
    (s / n).astype(np.uint8)
    t_mean = time.perf_counter() - t
    out["host_rows_measured"] = hr
    out["host_median_s_extrapolated"] = round(t_med * S / hr, 2)
    out["host_mean_s_extrapolated"] = round(t_mean * S / hr, 2)
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
