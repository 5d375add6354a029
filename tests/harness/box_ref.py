"""TEST INFRASTRUCTURE: numpy-only restatement of the background-subtraction worm box (the reference's
BoxCalculator._calc_bounding_box, dataset/box_calculator.py:75-101, for gray frames), the yardstick of csrc/box_ops.hip.

  1. m0 = |frame - bg| > t
  2. erode 5 x 5: a pixel stays set iff every in-image pixel of its window is set
  3. dilate 15 x 15: a pixel is set iff any in-image pixel within Chebyshev distance 7 is set
  4. per 8-connected component A2 = twice the area of the polygon through the pixel centres of its outer border (Moore tracing from the raster-first
     pixel, closed when the start pixel is about to be left by its first move again), and the extent of that border
  5. the winner has the largest A2; among equal A2 the one whose raster-first pixel comes LAST in raster order
  6. box = (min x, min y, width, height); (0, 0, 0, 0) without foreground

The morphology is shifted AND / OR of padded arrays; the contours are found without labelling: every set pixel whose W, NW, N and NE neighbours are clear
is traced, and a trace is kept iff no pixel of it precedes its start in raster order."""
from __future__ import annotations

import numpy as np

# the eight neighbours clockwise on the screen (y down) from east: E SE S SW W NW N NE
DX = (1, 1, 0, -1, -1, -1, 0, 1)
DY = (0, 1, 1, 1, 0, -1, -1, -1)


def threshold(frame: np.ndarray, bg: np.ndarray, t: int) -> np.ndarray:
    return np.abs(frame.astype(np.int16) - bg.astype(np.int16)) > t


def _window(m: np.ndarray, k: int, erode: bool) -> np.ndarray:
    """AND (erode) or OR of the k x k window over its in-image pixels: rows then columns (the window and the padding are both products)."""
    r = k // 2
    out = m
    for axis in (1, 0):
        pad = [(0, 0), (0, 0)]
        pad[axis] = (r, r)
        p = np.pad(out, pad, constant_values=erode)  # out-of-image pixels never erode and never dilate
        n = out.shape[axis]
        acc = np.full(out.shape, erode)
        for d in range(k):
            sl = [slice(None), slice(None)]
            sl[axis] = slice(d, d + n)
            acc = (acc & p[tuple(sl)]) if erode else (acc | p[tuple(sl)])
        out = acc
    return out


def erode(m: np.ndarray, k: int) -> np.ndarray:
    return _window(m, k, True)


def dilate(m: np.ndarray, k: int) -> np.ndarray:
    return _window(m, k, False)


def morphology(m0: np.ndarray) -> np.ndarray:
    return dilate(erode(m0, 5), 15)


def candidates(m: np.ndarray) -> np.ndarray:
    """(y, x) of the set pixels whose W, NW, N and NE neighbours are clear, in raster order."""
    H, W = m.shape
    p = np.pad(m, 1, constant_values=False)
    c = m & ~p[1:H + 1, 0:W] & ~p[0:H, 0:W] & ~p[0:H, 1:W + 1] & ~p[0:H, 2:W + 2]
    return np.argwhere(c)


def trace(m: np.ndarray, sy: int, sx: int, early_exit: bool = True):
    """Moore trace of the border through (sx, sy), whose W neighbour is clear: (kept, A2, (x0, y0, x1, y1), pixels).  kept: no pixel of the trace precedes
    the start in raster order (with early_exit the trace stops at the first that does, and the other values are None)."""
    H, W = m.shape
    x, y, b, d0, s = sx, sy, 4, -1, 0
    kept = True
    pix = [(sx, sy)]
    for _ in range(8 * H * W + 1):
        d = -1
        for k in range(1, 9):
            dd = (b + k) & 7
            nx, ny = x + DX[dd], y + DY[dd]
            if 0 <= nx < W and 0 <= ny < H and m[ny, nx]:
                d = dd
                break
        if d < 0:
            break  # a single pixel
        if (x, y) == (sx, sy):
            if d0 < 0:
                d0 = d
            elif d == d0:
                break
        s += x * ny - nx * y
        x, y = nx, ny
        b = (d - 2 - (d & 1)) & 7
        if (y, x) < (sy, sx):
            kept = False
            if early_exit:
                return False, None, None, None
        pix.append((x, y))
    else:
        raise AssertionError("trace exceeded 8 H W steps")
    xs, ys = [p[0] for p in pix], [p[1] for p in pix]
    return kept, abs(s), (min(xs), min(ys), max(xs), max(ys)), pix


def contours(m: np.ndarray) -> list:
    """One (A2, root raster index, (x, y, w, h)) per 8-connected component of the boolean mask, in raster order of the roots."""
    H, W = m.shape
    out = []
    for sy, sx in candidates(m):
        kept, a2, ext, _ = trace(m, int(sy), int(sx))
        if kept:
            out.append((a2, int(sy) * W + int(sx), (ext[0], ext[1], ext[2] - ext[0] + 1, ext[3] - ext[1] + 1)))
    return out


def select(cs: list):
    """(box, A2, second-best A2 or -1) of the contour list: the largest A2, among equals the last root."""
    if not cs:
        return (0, 0, 0, 0), 0, -1
    order = sorted(cs, key=lambda c: (c[0], c[1]))
    return order[-1][2], order[-1][0], (order[-2][0] if len(order) > 1 else -1)


def box_of_mask(m: np.ndarray):
    return select(contours(m))


def box_ref(frame: np.ndarray, bg: np.ndarray, t: int):
    """(box int64 [4], A2, mask uint8 [H, W] 0 / 255, second-best A2 or -1) of one gray frame.  A tie for the largest area shows as second == A2."""
    m = morphology(threshold(frame, bg, t))
    box, a2, second = box_of_mask(m)
    return np.array(box, dtype=np.int64), a2, m.astype(np.uint8) * 255, second


def boxes_ref(frames: np.ndarray, bg: np.ndarray, t: int, indices=None):
    """box_ref over frames[indices]: (boxes int64 [n, 4], A2 int64 [n], masks uint8 [n, H, W], second int64 [n])."""
    idx = range(len(frames)) if indices is None else indices
    res = [box_ref(frames[i], bg, t) for i in idx]
    return (np.stack([r[0] for r in res]), np.array([r[1] for r in res], dtype=np.int64), np.stack([r[2] for r in res]),
            np.array([r[3] for r in res], dtype=np.int64))
