"""Numpy restatement of the reference's evaluation arithmetic, the yardstick of wtracker_amd.evaluation (tests/test_eval_golden.py pins it to the
real reference's outputs in tests/golden/eval_*.npz):
  * background()   BGExtractor._calc_background_median / _mean   wtracker/dataset/bg_extractor.py:55-75
  * discretize()   BoxUtils.discretize                           wtracker/utils/bbox_utils.py:118-167 (on a copy: the reference zeroes in place)
  * precise()      ErrorCalculator.calculate_precise, per row    wtracker/eval/error_calculator.py:64-160, with the (total, inside) counts
  * reference_layout()  the same function's own return value (legal rows' errors shifted to the front, :104-108 and :133-159)
"""
from __future__ import annotations

import numpy as np


def background(frames: np.ndarray, ids, method: str) -> np.ndarray:
    stack = np.asarray(frames)[np.asarray(ids, dtype=np.int64)]
    if method == "median":
        return np.median(stack, axis=0).astype(np.uint8)
    s = np.zeros(stack.shape[1:], dtype=np.float64)
    for f in stack:
        s += f
    return (s / len(stack)).astype(np.uint8)


def discretize(boxes: np.ndarray, bounds):
    """(x1, y1, x2, y2) int32 and the legal mask; illegal rows are all zero.  Arithmetic in the array's own dtype, as the reference."""
    b = np.array(boxes, copy=True)
    legal = np.isfinite(b).all(axis=1)
    b[~legal] = 0
    x1, y1 = np.floor(b[:, 0]).astype(np.int32), np.floor(b[:, 1]).astype(np.int32)
    x2, y2 = np.ceil(b[:, 0] + b[:, 2]).astype(np.int32), np.ceil(b[:, 1] + b[:, 3]).astype(np.int32)
    H, W = bounds
    x1, x2 = np.clip(x1, 0, W), np.clip(x2, 0, W)
    y1, y2 = np.clip(y1, 0, H), np.clip(y2, 0, H)
    legal = (x2 - x1 > 0) & (y2 - y1 > 0)
    for v in (x1, y1, x2, y2):
        v[~legal] = 0
    return x1, y1, x2, y2, legal


def precise(frames: np.ndarray, bg: np.ndarray, worm: np.ndarray, mic: np.ndarray, frame_nums, diff_thresh: float):
    """Per-row errors (NaN where the worm box is illegal) and int64 [N, 2] (total, inside) foreground counts."""
    H, W = bg.shape[:2]
    wl, wt, wr, wb, legal = discretize(worm, (H, W))
    ml, mt, mr, mb, _ = discretize(mic, (H, W))
    il, it = np.maximum(wl, ml), np.maximum(wt, mt)
    iw, ih = np.maximum(0, np.minimum(wr, mr) - il), np.maximum(0, np.minimum(wb, mb) - it)
    n = len(frame_nums)
    err = np.full(n, np.nan)
    counts = np.zeros((n, 2), dtype=np.int64)
    for i in np.flatnonzero(legal):
        view = frames[int(frame_nums[i])][wt[i]:wb[i], wl[i]:wr[i]]
        diff = np.abs(view.astype(np.int32) - bg[wt[i]:wb[i], wl[i]:wr[i]].astype(np.int32)).astype(np.uint8)
        mask = diff > diff_thresh
        total = int(mask.sum())
        y0, x0 = it[i] - wt[i], il[i] - wl[i]
        inside = int(mask[y0:y0 + ih[i], x0:x0 + iw[i]].sum())
        counts[i] = total, inside
        err[i] = 0.0 if total == 0 else 1.0 - np.int64(inside) / np.int64(total)
    return err, counts


def reference_layout(per_row: np.ndarray) -> np.ndarray:
    legal = ~np.isnan(per_row)
    out = np.where(legal, 0.0, np.nan)
    vals = per_row[legal]
    out[: len(vals)] = vals
    return out
