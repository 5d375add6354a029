#!/usr/bin/env python3
"""Timing of the background-subtraction worm boxes (csrc/box_ops.hip) at the reference's experiment scale; prints one JSON line.

  frames       --frames frames of --size x --size gray in device memory: a textured background, 0.2 % speckle at 255 and a curled worm 9 pixels thick
               that moves from frame to frame.
  boxes_ms     evaluation.boxes over all frames (mask stage, contour stage, the winner's retrace; the chunking of the Python layer included),
               milliseconds by device events, median of --reps runs after one warm-up; boxes_GBps counts the frame bytes once.
  mask_ms      the mask stage alone over the same chunks (wtk_boxes without boxes_dev): threshold, 5 x 5 erosion, 15 x 15 dilation, bit-packed store.
  bg_mean_ms   the `mean` background over the same frames in the same run: a kernel that reads the same bytes once and does next to nothing with them,
               the rate the mask stage is held against (mask_vs_mean = mask rate / mean rate).
  host         the numpy restatement (tests/harness/box_ref.py) on --host-frames frames, in seconds per frame and scaled linearly to all frames
               (labelled as extrapolated); its boxes must equal the device's.
  source       wtracker_amd._build.source_sha() of the library that was timed.
Usage: python tools/boxes_timing.py [--frames 1000] [--size 1500] [--reps 5] [--host-frames 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


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


def _worm_patch():
    """Boolean [150, 150] patch: discs of radius 4 along a curled line."""
    p = np.zeros((150, 150), bool)
    yy, xx = np.mgrid[-4:5, -4:5]
    disc = yy ** 2 + xx ** 2 <= 16
    s = np.linspace(0, 1, 400)
    cx = 75 + 55 * np.cos(4.5 * np.pi * s) * (1 - 0.7 * s)
    cy = 60 + 45 * np.sin(4.5 * np.pi * s) * (1 - 0.7 * s) + 30 * s
    for x, y in zip(cx.astype(int), cy.astype(int)):
        p[y - 4:y + 5, x - 4:x + 5] |= disc
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--size", type=int, default=1500)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-frames", type=int, default=3)
    args = ap.parse_args()

    import torch

    from harness import box_ref
    from wtracker_amd import _build
    from wtracker_amd import evaluation as ev
    from wtracker_amd import hip

    if hip.device_count() < 1:
        raise SystemExit("boxes_timing: no HIP device visible (nothing is timed on the CPU)")
    n, S = args.frames, args.size
    g = torch.Generator(device="cuda").manual_seed(0)
    bg = torch.randint(90, 140, (S, S), dtype=torch.uint8, device="cuda", generator=g)
    frames = bg.expand(n, S, S).contiguous()
    worm = torch.from_numpy(_worm_patch()).cuda()
    for lo in range(0, n, 50):
        part = frames[lo:lo + 50]
        part[torch.rand(part.shape, device="cuda", generator=g) < 0.002] = 255
    for k in range(n):
        x, y = 100 + (k * 7) % (S - 400), 100 + (k * 3) % (S - 400)
        frames[k, y:y + 150, x:x + 150][worm] = 20
    nbytes = n * S * S
    out = {"frames": n, "frame": [S, S], "frame_bytes_total": nbytes, "diff_thresh": 20}

    ms = _time_ms(lambda: ev.background(frames, n, "uniform", "mean"), args.reps)
    out["bg_mean_ms"], out["bg_mean_GBps"] = round(ms, 3), round(nbytes / ms / 1e6, 1)

    ms = _time_ms(lambda: ev.boxes(frames, bg, 20), args.reps)
    out["boxes_ms"], out["boxes_GBps"] = round(ms, 3), round(nbytes / ms / 1e6, 1)

    chunk = max(1, ev.BOXES_SCRATCH_BYTES // hip.boxes_scratch_bytes(S, S, 1))
    scratch = torch.empty(hip.boxes_scratch_bytes(S, S, min(chunk, n)), dtype=torch.uint8, device="cuda")
    faults = torch.zeros(1, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def mask_stage():
        for lo in range(0, n, chunk):
            k = min(chunk, n - lo)
            hip.boxes(frames[lo:lo + k], k, S, S, bg, None, k, 20, None, None, None, faults, scratch, scratch.numel(), stream)

    ms = _time_ms(mask_stage, args.reps)
    out["mask_ms"], out["mask_GBps"] = round(ms, 3), round(nbytes / ms / 1e6, 1)
    out["mask_vs_mean"] = round(out["mask_GBps"] / out["bg_mean_GBps"], 3)
    out["chunk_frames"] = chunk

    dev_boxes = ev.boxes(frames, bg, 20).cpu().numpy()
    out["faults"] = int(faults.item())
    out["boxes_with_foreground"] = int((dev_boxes[:, 2] > 0).sum())
    h = min(args.host_frames, n)
    host_frames, host_bg = frames[:h].cpu().numpy(), bg.cpu().numpy()
    t = time.perf_counter()
    host_boxes = box_ref.boxes_ref(host_frames, host_bg, 20)[0]
    per_frame = (time.perf_counter() - t) / h
    out["host_frames_measured"] = h
    out["host_s_per_frame"] = round(per_frame, 3)
    out["host_s_extrapolated"] = round(per_frame * n, 1)
    out["host_boxes_equal"] = bool((host_boxes == dev_boxes[:h]).all())
    out["source"] = _build.source_sha()
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
