"""Experiment evaluation on the MI355X: the experiment background and the precise tracking error.
  * BGExtractor.calc_background               wtracker/dataset/bg_extractor.py:18-75        -> background(), BGExtractor
  * ErrorCalculator.calculate_precise          wtracker/eval/error_calculator.py:64-160       -> precise_error()
  * DataAnalyzer.calc_precise_error            wtracker/eval/data_analyzer.py:289-324         -> precise_error_from_log()
  * BoxCalculator._calc_bounding_box           wtracker/dataset/box_calculator.py:75-101      -> boxes(), BoxCalculator (csrc/box_ops.hip)
Both steps run on frames already in device memory (csrc/eval_ops.hip): the background streams the probe frames once (mean) or twice (median) and
never stacks them on the host; the error is computed per log row from the full frames, so the worm-view images the reference's LoggingController
saves for it (logging_controller.py:157-170, save_wrm_view) are not needed.  Results are bit-exact to the reference's numpy code.

Row layout of the precise error.  `calculate_precise` marks illegal rows (non-finite worm box, or no area after clipping) NaN, drops them
(error_calculator.py:104-108) and then writes errors[i] with i counting the LEGAL rows only (:133-159): the legal rows' errors end up at the front
of the array, and every later row keeps its initial value (NaN if illegal, 0.0 if legal).  For rows [legal, NaN, legal, legal] it returns
[e0, e2, e3, 0.0], and DataAnalyzer stores that array against the log rows as it is.  layout="per_row" (the default) gives row i its own error, NaN
where the worm box is illegal; layout="reference" reproduces the reference's return value byte for byte (a permutation of the per-row result).
"""
from __future__ import annotations

import csv
import math
import os

import numpy as np

from . import hip

WORM_COLUMNS = ("wrm_x", "wrm_y", "wrm_w", "wrm_h")
MIC_COLUMNS = ("mic_x", "mic_y", "mic_w", "mic_h")
_METHODS = {"median": hip.BG_MEDIAN, "mean": hip.BG_MEAN}


def probe_indices(length: int, num_probes: int, sampling: str = "uniform") -> np.ndarray:
    """The frame ids calc_background samples (bg_extractor.py:38-48): "uniform" = unique(int(linspace(0, L - 1, min(n, L)))), "random" =
    np.random.choice(L, min(n, L), replace=False) on numpy's global generator (a seeded caller gets the reference's frames)."""
    if sampling not in ("random", "uniform"):
        raise ValueError(f"sampling must be 'random' or 'uniform', not {sampling!r}")
    size = min(num_probes, length)
    if sampling == "random":
        return np.random.choice(length, size=size, replace=False)
    return np.unique(np.linspace(0, length - 1, num=size).astype(int, copy=False))


def _is_cuda(x) -> bool:
    return bool(getattr(x, "is_cuda", False))


def _frame_shape(frames) -> tuple:
    """The shape of one frame of a tensor, an array or a reader (its frame_shape)."""
    return tuple(frames.frame_shape) if hasattr(frames, "frame_shape") else tuple(np.shape(frames)[1:])


def _host_stack(frames, ids, shape: tuple) -> np.ndarray:
    """The frames `ids` of a host array or reader as one uint8 array [len(ids), *shape]; only those frames are read."""
    stack = np.empty((len(ids),) + shape, dtype=np.uint8)
    for k, i in enumerate(ids):
        f = np.asarray(frames[int(i)])
        if f.dtype != np.uint8 or f.shape != shape:
            raise ValueError(f"frame {int(i)} is {f.dtype} {f.shape}, expected uint8 {shape}")
        stack[k] = f
    return stack


def _device_background(background, H: int, W: int, device=None, channel_axis: bool = False):
    """`background` as a contiguous uint8 [H, W] tensor on `device` (None: where it is, a host array on the current GPU); channel_axis: [H, W, 1] too."""
    import torch

    bg = background if _is_cuda(background) else torch.from_numpy(np.ascontiguousarray(background))
    gray = tuple(bg.shape[:2]) == (H, W) and bg.numel() == H * W if channel_axis else tuple(bg.shape) == (H, W)
    if bg.dtype != torch.uint8 or not gray:
        raise ValueError(f"background must be uint8 [{H},{W}] (gray)")
    if device is None:
        device = bg.device if bg.is_cuda else torch.device("cuda", torch.cuda.current_device())
    return bg.reshape(H, W).to(device).contiguous()


def background(frames, num_probes: int, sampling: str = "uniform", method: str = "median"):
    """Per-pixel median / mean of `num_probes` sampled frames as a CUDA uint8 tensor of one frame's shape, enqueued on the current torch stream.
    `frames`: a CUDA uint8 tensor [F,H,W] or [F,H,W,3] (the probes are read in place), a host array of that shape, or a reader with __len__,
    __getitem__ and frame_shape (only the probe frames are read and uploaded)."""
    import torch

    if method not in _METHODS:
        raise ValueError(f"method must be 'median' or 'mean', not {method!r}")
    length = len(frames)
    ids = probe_indices(length, num_probes, sampling)
    if len(ids) == 0:
        raise ValueError("no frames to sample the background from")
    shape = _frame_shape(frames)
    if _is_cuda(frames):
        if frames.dtype != torch.uint8 or frames.dim() not in (3, 4) or not frames.is_contiguous():
            raise ValueError("device frames must be a contiguous CUDA uint8 tensor [F,H,W] or [F,H,W,3]")
        src, n_frames, idx = frames, length, torch.from_numpy(ids.astype(np.int32)).to(frames.device)
    else:
        src, n_frames, idx = torch.from_numpy(_host_stack(frames, ids, shape)).cuda(), len(ids), None
    bg = torch.empty(shape, dtype=torch.uint8, device=src.device)
    with torch.cuda.device(src.device):
        hip.background(src, n_frames, math.prod(shape), idx, len(ids), _METHODS[method], bg, torch.cuda.current_stream().cuda_stream)
    return bg


class BGExtractor:
    """BGExtractor (bg_extractor.py:7-75) with the median / mean on the device.  `frames_or_reader`: what background() accepts."""

    def __init__(self, frames_or_reader):
        self.reader = frames_or_reader

    def calc_background(self, num_probes: int, sampling: str = "uniform", method: str = "median") -> np.ndarray:
        return background(self.reader, num_probes, sampling, method).cpu().numpy()


BOXES_SCRATCH_BYTES = 256 << 20  # boxes() works through a selection in chunks whose scratch stays within this (one frame's, if that alone is larger)


def _boxes_threshold(diff_thresh) -> int:
    assert diff_thresh > 0, "Difference threshold must be greater than 0."
    thr = min(int(math.floor(diff_thresh)), 255)  # |frame - bg| is an integer of at most 255: > t is > floor(t), and nothing exceeds 255
    if thr < 1:
        raise ValueError("diff_thresh below 1 marks every differing pixel: not a threshold boxes() takes")
    return thr


def boxes(frames, background, diff_thresh=20, frame_indices=None, return_area: bool = False, return_mask: bool = False, fault_count=None):
    """BoxCalculator's box of every selected frame as a CUDA int32 [n, 4] tensor (x, y, w, h), enqueued on the current torch stream with no host
    synchronisation: threshold |frame - background| > diff_thresh, 5 x 5 opening, 11 x 11 dilation, the bounding box of the contour with the largest
    cv.contourArea; (0, 0, 0, 0) without foreground (DESIGN.md section 18 states the semantics and what is left unpinned).
    frames         a contiguous CUDA uint8 [F,H,W] tensor (read in place), or a host array / reader as background() takes them (only the selected frames
                   are read and uploaded).  [F,H,W,3] is refused: the colour branch goes through cv.cvtColor and is out of scope.
    background     uint8 [H,W], CUDA or host
    frame_indices  None (every frame), a sequence, or a CUDA int32 tensor.  On device frames an index outside [0, F) gives the row (-1, -1, -1, -1)
                   (and area -1, a zero mask) instead of an error, since raising would need a synchronisation; fault_count, a CUDA int32 [1] tensor of the
                   caller's, has the number of such rows added to it.
    return_area    also the int64 [n] A2 = twice the winning contour's area;  return_mask  also the uint8 [n,H,W] mask after the morphology (0 / 255).
    Scratch is 8 + 4 H ceil(W / 32) bytes per frame.  A selection is processed in chunks of max(1, BOXES_SCRATCH_BYTES // that) frames (256 MiB: 951 frames
    of 1500 x 1500), so 60 000 frames of 1500 x 1500 take 64 calls on one 256 MiB buffer; frame offsets are 64-bit throughout."""
    import torch

    thr = _boxes_threshold(diff_thresh)
    on_device, shape = _is_cuda(frames), _frame_shape(frames)
    if len(shape) == 3:
        raise ValueError("boxes takes gray frames [F,H,W] only: the reference's colour branch goes through cv.cvtColor and is out of scope")
    if len(shape) != 2:
        raise ValueError(f"frames must be uint8 [F,H,W], not frames of shape {shape}")
    if on_device and (frames.dtype != torch.uint8 or not frames.is_contiguous()):
        raise ValueError("device frames must be a contiguous CUDA uint8 tensor [F,H,W]")
    H, W = (int(v) for v in shape)
    F = len(frames)
    bg = _device_background(background, H, W, frames.device if on_device else None)
    dev = bg.device
    idx_dev = idx_host = None
    if frame_indices is None:
        n = F
    elif _is_cuda(frame_indices):
        if not on_device:
            raise ValueError("device frame indices need device frames")
        idx_dev = frame_indices.to(dtype=torch.int32).contiguous()
        n = int(idx_dev.shape[0])
    else:
        idx_host = np.asarray(list(frame_indices) if not isinstance(frame_indices, np.ndarray) else frame_indices).astype(np.int64).reshape(-1)
        n = len(idx_host)
        if on_device:
            idx_dev = torch.from_numpy(np.clip(idx_host, -1, 2 ** 31 - 1).astype(np.int32)).to(dev)  # (any index outside [0, F) stays outside)
    out = torch.empty((n, 4), dtype=torch.int32, device=dev)
    area = torch.empty(n, dtype=torch.int64, device=dev) if return_area else None
    mask = torch.empty((n, H, W), dtype=torch.uint8, device=dev) if return_mask else None
    if n:
        if fault_count is None:
            fault_count = torch.zeros(1, dtype=torch.int32, device=dev)
        per_frame = hip.boxes_scratch_bytes(H, W, 1)
        wpr = (W + 31) // 32
        blocks = max(((H + 63) // 64) * ((wpr + 61) // 62), ((H + 31) // 32) * ((wpr + 63) // 64))  # an upper bound of either launch's blocks per frame
        chunk = max(1, min(BOXES_SCRATCH_BYTES // per_frame, (2 ** 31 - 1) // blocks))
        scratch = torch.empty(hip.boxes_scratch_bytes(H, W, min(chunk, n)), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            for lo in range(0, n, chunk):
                k = min(chunk, n - lo)
                if on_device:
                    src, n_src, idx = (frames, F, idx_dev[lo:lo + k]) if idx_dev is not None else (frames[lo:lo + k], k, None)
                else:
                    ids = range(lo, lo + k) if idx_host is None else idx_host[lo:lo + k]
                    src, n_src, idx = torch.from_numpy(_host_stack(frames, ids, (H, W))).to(dev), k, None
                hip.boxes(src, n_src, H, W, bg, idx, k, thr, out[lo:lo + k], None if area is None else area[lo:lo + k],
                          None if mask is None else mask[lo:lo + k], fault_count, scratch, scratch.numel(), stream)
    res = (out,) + ((area,) if return_area else ()) + ((mask,) if return_mask else ())
    return res if len(res) > 1 else out


class BoxCalculator:
    """BoxCalculator (box_calculator.py:11-161) with the per-frame image step on the device.  `frames_or_reader`: what boxes() accepts; gray frames only.
    Boxes are host int64 rows (x, y, w, h), (-1, -1, -1, -1) until computed; num_workers and chunk_size are accepted and ignored."""

    def __init__(self, frames_or_reader, background, diff_thresh: int = 20) -> None:
        assert diff_thresh > 0, "Difference threshold must be greater than 0."
        fr, shape = frames_or_reader, _frame_shape(frames_or_reader)
        assert shape == tuple(background.shape), "Background shape must match frame shape."
        if len(shape) == 3 and shape[2] == 3:
            raise ValueError("BoxCalculator takes gray frames only: the reference's colour branch goes through cv.cvtColor and is out of scope")
        if len(shape) != 2:
            raise ValueError("background must be either a gray or a color image.")
        self._frame_reader = fr
        self._background = background
        self._diff_thresh = diff_thresh
        self._all_bboxes = np.full((len(fr), 4), -1, dtype=int)

    def all_bboxes(self) -> np.ndarray:
        return self._all_bboxes

    def get_bbox(self, frame_idx: int) -> np.ndarray:
        if self._all_bboxes[frame_idx][0] == -1:
            self.calc_specified_boxes([frame_idx])
        return self._all_bboxes[frame_idx]

    def calc_specified_boxes(self, frame_indices, num_workers=None, chunk_size: int = 50) -> np.ndarray:
        import torch

        idx = np.asarray(list(frame_indices), dtype=np.int64).reshape(-1)
        if idx.size and (idx.min() < -len(self._frame_reader) or idx.max() >= len(self._frame_reader)):
            raise IndexError(f"frame index outside the {len(self._frame_reader)} frames")
        idx = np.where(idx < 0, idx + len(self._frame_reader), idx)
        todo = np.unique(idx[self._all_bboxes[idx, 0] == -1])
        if todo.size:
            faults = torch.zeros(1, dtype=torch.int32, device="cuda" if not _is_cuda(self._frame_reader) else self._frame_reader.device)
            got = boxes(self._frame_reader, self._background, self._diff_thresh, todo, fault_count=faults).cpu().numpy()
            if int(faults.item()):
                raise RuntimeError(f"{int(faults.item())} frame(s) exceeded the border trace's step bound")
            self._all_bboxes[todo] = got
        return self._all_bboxes[idx, :]

    def calc_all_boxes(self, num_workers=None, chunk_size: int = 50) -> np.ndarray:
        return self.calc_specified_boxes(range(len(self._frame_reader)), num_workers, chunk_size)


def reference_layout(per_row):
    """calculate_precise's return value from the per-row errors (torch or numpy): the legal rows' errors first, then each remaining row's initial
    value — NaN where the row is illegal, 0.0 where it is legal (error_calculator.py:99-108, 133-159)."""
    if isinstance(per_row, np.ndarray):
        legal = ~np.isnan(per_row)
        out = np.where(legal, 0.0, np.nan)
    else:
        import torch

        legal = ~torch.isnan(per_row)
        out = torch.where(legal, torch.zeros_like(per_row), torch.full_like(per_row, float("nan")))
    vals = per_row[legal]
    out[: len(vals)] = vals
    return out


def _boxes(x, dtype, device):
    import torch

    t = x if hasattr(x, "dim") else torch.from_numpy(np.asarray(x))
    if t.dim() != 2 or t.shape[1] != 4:
        raise ValueError(f"boxes must be [N, 4] xywh, not {tuple(t.shape)}")
    return t.to(device=device, dtype=dtype).contiguous()  # a copy wherever the caller's array could be touched: inputs are never modified


def _frame_nums(x, device):
    import torch

    if _is_cuda(x) and x.dtype == torch.int32:
        return x.contiguous()
    a = np.asarray(x.cpu() if hasattr(x, "cpu") else x)
    if a.ndim != 1:
        raise ValueError("frame_nums must be one-dimensional")
    if a.size and (a.min() < -(2 ** 31) or a.max() >= 2 ** 31):
        raise IndexError("frame number outside the int32 range")
    return torch.from_numpy(a.astype(np.int32)).to(device)


def precise_error(frames, background, worm_xywh, mic_xywh, frame_nums, diff_thresh: float = 10, layout: str = "per_row", return_counts: bool = False):
    """ErrorCalculator.calculate_precise on the device: a CUDA float64 [N] (and, with return_counts, the int32 [N, 2] (total, inside) foreground
    pixel counts), enqueued on the current torch stream.
    frames      CUDA (or host) uint8 [F,H,W] gray full frames; row i's worm view is the worm box's crop of frames[frame_nums[i]]
    background  uint8 [H,W] (background())
    worm_xywh, mic_xywh  [N, 4] boxes in full-frame pixels (float32 if both are float32, float64 otherwise)
    layout      "per_row" or "reference" (see the module docstring)
    Frame numbers outside [0, F) on a row with a legal worm box raise IndexError, as the reference's reader would (this check synchronises)."""
    import torch

    if layout not in ("per_row", "reference"):
        raise ValueError(f"layout must be 'per_row' or 'reference', not {layout!r}")
    if not hasattr(frames, "dim"):
        frames = np.asarray(frames)
    if frames.ndim == 4 and frames.shape[-1] != 1:
        raise ValueError("precise_error takes gray frames only (C = 1): the reference's colour branch goes through cv.cvtColor")
    if frames.dtype not in (np.uint8, torch.uint8) or frames.ndim not in (3, 4):
        raise ValueError("frames must be uint8 [F,H,W]")
    if not _is_cuda(frames):
        frames = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    frames = frames.reshape(frames.shape[:3]).contiguous()
    F, H, W = (int(s) for s in frames.shape)
    dev = frames.device
    bg = _device_background(background, H, W, dev, channel_axis=True)
    f32 = all(str(getattr(b, "dtype", "")).endswith("float32") for b in (worm_xywh, mic_xywh))  # float32 boxes keep the reference's float32 x + w
    dtype = torch.float32 if f32 else torch.float64
    worm, mic = _boxes(worm_xywh, dtype, dev), _boxes(mic_xywh, dtype, dev)
    fn = _frame_nums(frame_nums, dev)
    n = int(fn.shape[0])
    if worm.shape[0] != n or mic.shape[0] != n:
        raise ValueError(f"{n} frame numbers, {worm.shape[0]} worm boxes, {mic.shape[0]} microscope boxes")
    err = torch.empty(n, dtype=torch.float64, device=dev)
    counts = torch.zeros((n, 2), dtype=torch.int32, device=dev) if return_counts else None
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        hip.precise_error(frames, F, H, W, bg, worm, mic, fn, n, float(diff_thresh), err, counts, bad, torch.cuda.current_stream().cuda_stream)
    n_bad = int(bad.item())
    if n_bad:
        raise IndexError(f"{n_bad} log row(s) name a frame outside [0, {F})")
    if layout == "reference":
        err = reference_layout(err)
    return (err, counts) if return_counts else err


def read_log(rows_or_csv):
    """(frame numbers int32 [N], worm boxes float64 [N, 4], microscope boxes float64 [N, 4]) of TrackLogger.rows or a 17-column log CSV, in row
    order — the columns DataAnalyzer.calc_precise_error takes from the log (data_analyzer.py:307-309)."""
    if isinstance(rows_or_csv, (str, os.PathLike)):
        with open(rows_or_csv, newline="") as f:
            rows = list(csv.DictReader(f))
    else:
        rows = list(rows_or_csv)
    frames = np.array([int(float(r["frame"])) for r in rows], dtype=np.int64).astype(np.int32)
    worm = np.array([[float(r[k]) for k in WORM_COLUMNS] for r in rows], dtype=np.float64).reshape(-1, 4)
    mic = np.array([[float(r[k]) for k in MIC_COLUMNS] for r in rows], dtype=np.float64).reshape(-1, 4)
    return frames, worm, mic


def precise_error_from_log(rows_or_csv, frames, background, diff_thresh: float = 20, layout: str = "per_row", return_counts: bool = False):
    """DataAnalyzer.calc_precise_error (data_analyzer.py:289-324; its default diff_thresh is 20) over TrackLogger.rows or a log CSV, on the
    device frames instead of saved worm views."""
    fn, worm, mic = read_log(rows_or_csv)
    return precise_error(frames, background, worm, mic, fn, diff_thresh, layout, return_counts)
