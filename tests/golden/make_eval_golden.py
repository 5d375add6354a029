#!/usr/bin/env python3
"""Generate tests/golden/eval_background.npz and tests/golden/eval_precise.npz by running the REAL reference's evaluation code:
BGExtractor.calc_background (wtracker/dataset/bg_extractor.py:18-75) and ErrorCalculator.calculate_precise (wtracker/eval/error_calculator.py:64-160).

Runs only where a checkout of the reference is available (REF below; it never travels with the tests).  Nothing of the reference's source is
copied: the outputs are numeric data only (frames, boxes, probe ids, results).  The reference imports cv2, tkinter and seaborn at module import
time; none is needed on these paths (gray frames only), so placeholder modules are registered first — an attribute-tolerant cv2 (wtracker/eval/vlc.py
reads cv.MARKER_CROSS at import), tkinter with a Tk class, and an empty seaborn.

eval_background.npz
  gray [41, 24, 40] and bgr [20, 10, 12, 3] uint8 stacks whose pixel columns are built for the median's corner cases (middle pairs straddling the
  15 / 16 nibble boundary, 254 / 255, 0 / 1, constant columns) next to random ones; per case c: meta_* (frames, num_probes, sampling, method,
  seed; seed < 0 = no reseed), ids_c (the frame ids the reference read, in its order) and bg_c (its result).  Median and mean, odd and even n,
  n = 1 and 2, every frame, n > len, uniform and seeded random sampling.
eval_precise.npz
  frames [16, 48, 64] gray, background [48, 64], 240 log rows (frame numbers, worm and microscope xywh float64) with NaN rows, fractional
  corners, boxes over the bounds, boxes with no area after clipping, frame-sized boxes, microscope boxes disjoint from / overlapping / containing
  the worm box, rows on a frame equal to the background (empty masks); the first four rows are [legal, NaN, legal, legal].  Per case c:
  thresh_c, f32_c (boxes passed as float32) and ref_c = calculate_precise's return value in its own layout.

Usage: python tests/golden/make_eval_golden.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"


class _Tolerant(types.ModuleType):
    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return 0


def _register_placeholders():
    tk = types.ModuleType("tkinter")
    tk.Tk = type("Tk", (), {})
    fd = types.ModuleType("tkinter.filedialog")
    tk.filedialog = fd
    for name, mod in (("cv2", _Tolerant("cv2")), ("tkinter", tk), ("tkinter.filedialog", fd), ("seaborn", types.ModuleType("seaborn"))):
        sys.modules.setdefault(name, mod)
    if REF not in sys.path:
        sys.path.insert(0, REF)


class _Reader:
    """FrameReader stand-in over an array: records the ids it is asked for."""

    def __init__(self, frames):
        self.frames = frames
        self.read = []

    def __len__(self):
        return len(self.frames)

    @property
    def frame_shape(self):
        return self.frames.shape[1:]

    def __getitem__(self, i):
        self.read.append(int(i))
        return self.frames[i]


class _WormViews:
    """The worm views LoggingController would have saved (logging_controller.py:157-170: the discretised worm box's crop of the full frame),
    served in the order calculate_precise reads them (one per legal row), checked against the frame number it asks for."""

    def __init__(self, frames, worm, discretize):
        crops, legal = discretize(np.array(worm, copy=True), frames.shape[1:3])
        self.views = [(i, crops[i]) for i in np.flatnonzero(legal)]
        self.frames = frames
        self.frame_nums = None
        self.k = 0

    def __getitem__(self, frame_num):
        i, (x, y, w, h) = self.views[self.k]
        assert self.frame_nums[i] == frame_num
        self.k += 1
        return self.frames[frame_num][y:y + h, x:x + w]


def _columns(rng, F, n_px):
    """[F, n_px] uint8 time series: every kind of pixel column the median has to get right."""
    cols = np.empty((F, n_px), dtype=np.uint8)
    for p in range(n_px):
        kind = p % 8
        if kind == 0:
            cols[:, p] = rng.choice([15, 16], F)
        elif kind == 1:
            cols[:, p] = rng.choice([254, 255], F)
        elif kind == 2:
            cols[:, p] = rng.choice([0, 1], F)
        elif kind == 3:
            cols[:, p] = rng.integers(0, 256)
        elif kind == 4:
            cols[:, p] = rng.choice([31, 32, 47, 48], F)
        else:
            cols[:, p] = rng.integers(0, 256, F)
    return cols


def make_background(BGExtractor):
    rng = np.random.default_rng(2024)
    stacks = {"gray": _columns(rng, 41, 24 * 40).reshape(41, 24, 40), "bgr": _columns(rng, 20, 10 * 12 * 3).reshape(20, 10, 12, 3)}
    cases = [("gray", 1, "uniform", "median", -1), ("gray", 2, "uniform", "median", -1), ("gray", 2, "uniform", "mean", -1),
             ("gray", 7, "uniform", "median", -1), ("gray", 8, "uniform", "median", -1), ("gray", 8, "uniform", "mean", -1),
             ("gray", 41, "uniform", "median", -1), ("gray", 41, "uniform", "mean", -1), ("gray", 100, "uniform", "median", -1),
             ("gray", 10, "random", "median", 3), ("gray", 11, "random", "mean", 5), ("gray", 20, "random", "median", 7),
             ("bgr", 5, "uniform", "median", -1), ("bgr", 6, "uniform", "median", -1), ("bgr", 6, "uniform", "mean", -1),
             ("bgr", 20, "uniform", "median", -1), ("bgr", 4, "random", "median", 11), ("bgr", 9, "random", "mean", 13)]
    out = dict(stacks)
    for c, (key, n, sampling, method, seed) in enumerate(cases):
        if seed >= 0:
            np.random.seed(seed)
        reader = _Reader(stacks[key])
        bg = BGExtractor(reader).calc_background(n, sampling=sampling, method=method)
        out[f"ids_{c}"] = np.array(reader.read, dtype=np.int64)
        out[f"bg_{c}"] = bg
    out["meta_frames"] = np.array([c[0] for c in cases])
    out["meta_num_probes"] = np.array([c[1] for c in cases], dtype=np.int64)
    out["meta_sampling"] = np.array([c[2] for c in cases])
    out["meta_method"] = np.array([c[3] for c in cases])
    out["meta_seed"] = np.array([c[4] for c in cases], dtype=np.int64)
    np.savez_compressed(os.path.join(HERE, "eval_background.npz"), **out)


def _precise_inputs():
    rng = np.random.default_rng(77)
    F, H, W, N = 16, 48, 64, 240
    yy, xx = np.mgrid[0:H, 0:W]
    bg = (100 + 8 * np.sin(xx / 7.0) + 6 * np.cos(yy / 5.0) + rng.integers(-3, 4, (H, W))).astype(np.uint8)
    frames = np.empty((F, H, W), dtype=np.uint8)
    for f in range(F):
        img = bg.astype(np.int32) + rng.integers(-13, 14, (H, W))
        for _ in range(10):  # worm-like bright / dark blobs
            cx, cy, rx, ry = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(3, 14), rng.uniform(3, 10)
            blob = ((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2 < 1
            img[blob] += int(rng.choice([-1, 1])) * int(rng.integers(9, 60))
        frames[f] = np.clip(img, 0, 255)
    frames[3] = bg  # every mask on this frame is empty
    worm = np.empty((N, 4))
    mic = np.empty((N, 4))
    for i in range(N):
        x, y = rng.uniform(-8, W + 4), rng.uniform(-8, H + 4)
        w, h = rng.uniform(0.5, 24), rng.uniform(0.5, 24)
        worm[i] = x, y, w, h
        kind = i % 6
        if kind == 0:  # containing
            mic[i] = x - rng.uniform(0, 6), y - rng.uniform(0, 6), w + rng.uniform(6, 14), h + rng.uniform(6, 14)
        elif kind == 1:  # disjoint
            mic[i] = x + w + rng.uniform(1, 10), y + h + rng.uniform(1, 10), rng.uniform(3, 20), rng.uniform(3, 20)
        else:  # partial overlap, fractional corners
            mic[i] = x + rng.uniform(-10, 10), y + rng.uniform(-10, 10), rng.uniform(2, 30), rng.uniform(2, 30)
    special = {1: (np.nan, 3.0, 5.0, 5.0), 9: (W + 3.5, 4.0, 6.0, 6.0), 14: (10.0, -20.0, 5.0, 9.0), 21: (-3.2, -2.7, W + 9.1, H + 8.4),
               27: (12.0, 12.0, 0.0, 7.0), 33: (12.0, 12.0, -4.0, 7.0), 40: (3.0, np.inf, 5.0, 5.0), 46: (-0.5, -0.5, W + 1.0, H + 1.0),
               52: (W - 0.25, H - 0.25, 9.0, 9.0), 58: (np.nan,) * 4}
    for i, b in special.items():
        worm[i] = b
    for i in range(60, N, 17):
        worm[i] = np.nan
    mic[5] = np.nan
    mic[11] = (W + 2.0, 0.0, 10.0, 10.0)  # no area after clipping
    mic[21] = (-1.0, -1.0, W + 2.0, H + 2.0)
    for i in (0, 2, 3):  # rows 0..3: [legal, NaN, legal, legal]
        worm[i] = (10.3 + 7 * i, 11.6, 12.2, 9.9)
    frame_nums = rng.integers(0, F, N).astype(np.int64)
    frame_nums[[2, 30, 31, 32]] = 3
    return frames, bg, worm, mic, frame_nums


def make_precise(ErrorCalculator, BoxUtils, BoxFormat):
    frames, bg, worm, mic, frame_nums = _precise_inputs()

    def disc(b, bounds):
        return BoxUtils.discretize(b, bounds=bounds, box_format=BoxFormat.XYWH)

    out = dict(frames=frames, background=bg, worm=worm, mic=mic, frame_nums=frame_nums)
    for c, (thresh, f32) in enumerate([(10, False), (20, False), (12.5, False), (10, True)]):
        w = worm.astype(np.float32) if f32 else worm.copy()
        m = mic.astype(np.float32) if f32 else mic.copy()
        views = _WormViews(frames, w, disc)
        views.frame_nums = frame_nums
        ref = ErrorCalculator.calculate_precise(background=bg, worm_bboxes=w.copy(), mic_bboxes=m.copy(), frame_nums=frame_nums.copy(),
                                                worm_reader=views, diff_thresh=thresh)
        assert views.k == len(views.views)
        out[f"thresh_{c}"] = np.float64(thresh)
        out[f"f32_{c}"] = np.bool_(f32)
        out[f"ref_{c}"] = np.asarray(ref, dtype=np.float64)
    np.savez_compressed(os.path.join(HERE, "eval_precise.npz"), **out)


def main():
    _register_placeholders()
    from wtracker.dataset.bg_extractor import BGExtractor
    from wtracker.eval.error_calculator import ErrorCalculator
    from wtracker.utils.bbox_utils import BoxFormat, BoxUtils

    make_background(BGExtractor)
    make_precise(ErrorCalculator, BoxUtils, BoxFormat)
    for f in ("eval_background.npz", "eval_precise.npz"):
        print(f, os.path.getsize(os.path.join(HERE, f)), "bytes")


if __name__ == "__main__":
    main()
