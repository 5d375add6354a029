"""What lies in front of and behind the network, stated without the library: letterbox geometry, an ideal bilinear resize, the inverse box map,
a stem that makes the network input readable, and the frame shapes at which any of this can go wrong.

Reading the network input.  The stem (model.0) is a 3x3 conv of stride 2 and padding 1: output (i, j) reads input rows 2i-1 .. 2i+1 and columns
2j-1 .. 2j+1, so its taps (1,1), (1,2), (2,1), (2,2) read input pixels (2i, 2j), (2i, 2j+1), (2i+1, 2j), (2i+1, 2j+1) — the four pixels of a
2x2 cell, never the padding.  `probe_weights` gives model.0 a zero bias and twelve output channels that each hold a single 1.0 at one of these
taps of one colour (every other weight and channel 0), so the stored model.0 blob (HipYolo.debug_tensor(0, B)) is silu(p / 255) for every pixel
p and colour of the network input, and `decode_network_input` turns it back into the uint8 image.  The rest of the network keeps its synthetic
weights and is ignored.

Why the decoder cannot be silently wrong.  silu(x) = x * sigma(x) has silu'(x) = sigma(x) * (1 + x * (1 - sigma(x))) >= sigma(0) = 0.5 for
x >= 0, so two neighbouring candidates silu(p / 255), silu((p + 1) / 255) lie at least 0.5 / 255 = 1.96e-3 apart.  The decoder takes the nearest
of the 256 float64 candidates and RAISES unless every residual is below a quarter of the smallest gap (4.9e-4): a value that passes is closer to
its candidate than to any other by a factor of three.  fp32 handles (errors ~1e-7) and f16x3 handles (a hi + lo pair, ~1e-6) pass with three
orders of magnitude to spare.  fp16 handles are left out: the blob is stored as ONE fp16 of the log2(e)-scaled activation (up to 1.05, spacing
2^-10 there), i.e. a rounding of up to 3.4e-4 — most of the allowed residual, so a correct handle could raise.
"""
from __future__ import annotations

import functools
import math
from typing import NamedTuple

import numpy as np

from wtracker_amd import yolo_spec as ys

PROBE_TAPS = ((1, 1), (1, 2), (2, 1), (2, 2))  # tap t of colour c is output channel 3 * t + c; tap (ky, kx) reads pixel (2i + ky - 1, 2j + kx - 1)
BORDER = 114


# ---- the probe stem and its decoder ------------------------------------------------------------------------------------------------------
def probe_weights(scale: str = "n", nc: int = 1, seed: int = 0) -> dict:
    """Synthetic weights of `scale` with model.0 replaced by the probe stem (module docstring).  Weight layout [cout][kh][kw][cin], cin in RGB order."""
    w = dict(ys.synthetic_weights(scale, nc, seed=seed))
    w0, b0 = w["model.0"]
    assert w0.shape[1:] == (3, 3, 3) and w0.shape[0] >= 12
    p = np.zeros_like(w0)
    for t, (ky, kx) in enumerate(PROBE_TAPS):
        for c in range(3):
            p[3 * t + c, ky, kx, c] = 1.0
    w["model.0"] = (p, np.zeros_like(b0))
    return w


@functools.lru_cache(maxsize=None)
def _candidates() -> np.ndarray:
    x = np.arange(256, dtype=np.float64) / 255.0
    return x / (1.0 + np.exp(-x))


def candidate_gap() -> float:
    """Smallest distance between two candidates; >= 0.5 / 255 by the slope bound of the module docstring."""
    gap = float(np.diff(_candidates()).min())
    assert gap >= 0.5 / 255
    return gap


class ProbeDecodeError(AssertionError):
    pass


def decode_network_input(blob: np.ndarray) -> np.ndarray:
    """model.0 blob [B, S_h / 2, S_w / 2, cout >= 12] of a probe-stem handle -> the uint8 network input [B, S_h, S_w, 3] in RGB order.
    Raises ProbeDecodeError when a value is not within a quarter of the candidate gap of a candidate, or an unused channel is not 0."""
    blob = np.asarray(blob, dtype=np.float64)
    if blob.ndim != 4 or blob.shape[3] < 12:
        raise ProbeDecodeError(f"not a probe blob: shape {blob.shape}")
    cand = _candidates()
    tol = candidate_gap() / 4
    v = blob[..., :12]
    if not np.isfinite(blob).all():
        raise ProbeDecodeError("non-finite values in the probe blob")
    hi = np.clip(np.searchsorted(cand, v), 1, 255)
    idx = np.where(np.abs(v - cand[hi - 1]) <= np.abs(v - cand[hi]), hi - 1, hi)
    res = np.abs(v - cand[idx])
    if res.max() >= tol:
        at = np.unravel_index(int(res.argmax()), res.shape)
        raise ProbeDecodeError(f"probe value {v[at]!r} at {at} is {res.max():.3e} from the nearest candidate (allowed {tol:.3e})")
    rest = np.abs(blob[..., 12:])
    if rest.size and rest.max() >= tol:
        raise ProbeDecodeError(f"unused probe channel holds {rest.max():.3e}")
    B, h2, w2 = blob.shape[:3]
    out = np.empty((B, 2 * h2, 2 * w2, 3), dtype=np.uint8)
    for t, (ky, kx) in enumerate(PROBE_TAPS):
        out[:, ky - 1 :: 2, kx - 1 :: 2, :] = idx[..., 3 * t : 3 * t + 3]
    return out


# ---- geometry -----------------------------------------------------------------------------------------------------------------------------
class Geometry(NamedTuple):
    net_h: int
    net_w: int
    new_h: int
    new_w: int
    top: int
    left: int


def letterbox_geometry(h: int, w: int, imgsz: int, stride: int = 32) -> Geometry:
    """LetterBox(auto=True, center=True) in Python floats, as oracle/yolo_oracle.py:letterbox_geometry states it."""
    r = min(imgsz / h, imgsz / w)
    new_w, new_h = int(round(w * r)), int(round(h * r))
    dw, dh = ((imgsz - new_w) % stride) / 2, ((imgsz - new_h) % stride) / 2
    top, left = int(round(dh - 0.1)), int(round(dw - 0.1))
    bottom, right = int(round(dh + 0.1)), int(round(dw + 0.1))
    return Geometry(new_h + top + bottom, new_w + left + right, new_h, new_w, top, left)


def exact_pad_geometry(h: int, w: int, net_h: int, net_w: int) -> Geometry:
    """A handle whose shape is not letterbox_shape(h, w, imgsz): r = min(S_h / H, S_w / W), padded to exactly (S_h, S_w) — what wtk_yolo_predict
    documents for such handles (LetterBox(auto=False))."""
    r = min(net_h / h, net_w / w)
    new_w, new_h = int(round(w * r)), int(round(h * r))
    dw, dh = (net_w - new_w) / 2, (net_h - new_h) / 2
    return Geometry(net_h, net_w, new_h, new_w, int(round(dh - 0.1)), int(round(dw - 0.1)))


def handle_geometry(h: int, w: int, net_h: int, net_w: int) -> Geometry:
    """The rule a handle of ANY shape follows (csrc/wtk_run.hip:letterbox_geom restated): r from S = max(S_h, S_w) when the resized image fits
    the handle, the pad-to-exactly rule otherwise.  tests/test_input_ref.py checks over the swept shapes that this is letterbox_geometry on every
    letterbox_shape handle."""
    S = max(net_h, net_w)
    r = min(S / h, S / w)
    new_w, new_h = int(round(w * r)), int(round(h * r))
    if new_h > net_h or new_w > net_w:
        return exact_pad_geometry(h, w, net_h, net_w)
    dw, dh = (net_w - new_w) / 2, (net_h - new_h) / 2
    return Geometry(net_h, net_w, new_h, new_w, int(round(dh - 0.1)), int(round(dw - 0.1)))


def back_map(net_hw: tuple, img_hw: tuple) -> tuple:
    """(gain, pad_x, pad_y) of scale_boxes, in Python floats exactly as oracle/yolo_oracle.py:scale_boxes states them."""
    gain = min(net_hw[0] / img_hw[0], net_hw[1] / img_hw[1])
    pad_x = round((net_hw[1] - img_hw[1] * gain) / 2 - 0.1)
    pad_y = round((net_hw[0] - img_hw[0] * gain) / 2 - 0.1)
    return gain, pad_x, pad_y


def back_map_float_gain(net_hw: tuple, img_hw: tuple) -> tuple:
    """The same with the padding computed from the gain AFTER its rounding to float32: the defect of class (g)."""
    gain = float(np.float32(min(net_hw[0] / img_hw[0], net_hw[1] / img_hw[1])))
    pad_x = round((net_hw[1] - img_hw[1] * gain) / 2 - 0.1)
    pad_y = round((net_hw[0] - img_hw[0] * gain) / 2 - 0.1)
    return gain, pad_x, pad_y


def scale_boxes64(net_hw: tuple, xyxy, img_hw: tuple, pad_shift: tuple = (0, 0)) -> tuple:
    """scale_boxes in float64 -> (boxes before the clip, boxes after it).  pad_shift: a planted error of the padding (tests only)."""
    gain, pad_x, pad_y = back_map(net_hw, img_hw)
    b = np.array(xyxy, dtype=np.float64).reshape(-1, 4)
    b[:, [0, 2]] -= pad_x + pad_shift[0]
    b[:, [1, 3]] -= pad_y + pad_shift[1]
    b /= gain
    c = b.copy()
    c[:, [0, 2]] = c[:, [0, 2]].clip(0, img_hw[1])
    c[:, [1, 3]] = c[:, [1, 3]].clip(0, img_hw[0])
    return b, c


def box_tolerance(net_hw: tuple, img_hw: tuple) -> float:
    """The suite's tolerance of a decoded box against the restatement on given logits (1e-3 px at gain 1), times max(1, 1 / gain) for the division."""
    return 1e-3 * max(1.0, 1.0 / back_map(net_hw, img_hw)[0])


def decode_anchor64(box_logits_row, anchor: int, net_hw: tuple) -> np.ndarray:
    """DFL + dist2bbox of ONE anchor in float64 -> xyxy in network pixels (anchors level-major, x fastest, as the head stores them)."""
    a = int(anchor)
    for s in ys.STRIDES:
        lh, lw = net_hw[0] // s, net_hw[1] // s
        if a < lh * lw:
            break
        a -= lh * lw
    else:
        raise AssertionError("anchor index beyond the last level")
    ax, ay = (a % lw) + 0.5, (a // lw) + 0.5
    z = np.asarray(box_logits_row, dtype=np.float64).reshape(4, ys.REG_MAX)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    d = (e / e.sum(axis=1, keepdims=True)) @ np.arange(ys.REG_MAX, dtype=np.float64)
    return np.array([(ax - d[0]) * s, (ay - d[1]) * s, (ax + d[2]) * s, (ay + d[3]) * s])


# ---- pixels -------------------------------------------------------------------------------------------------------------------------------
def ideal_bilinear(img: np.ndarray, new_h: int, new_w: int) -> np.ndarray:
    """Bilinear interpolation from its definition, in float64: destination pixel i samples the source at (i + 0.5) * n_src / n_dst - 0.5 (pixel
    centres at half-integers of both grids), coordinates clamped to [0, n_src - 1]; no fixed point, no rounding.  [h, w(, C)] -> float64."""
    img = np.asarray(img, dtype=np.float64)
    h, w = img.shape[:2]

    def axis(n_dst, n_src):
        x = np.clip((np.arange(n_dst, dtype=np.float64) + 0.5) * (n_src / n_dst) - 0.5, 0.0, n_src - 1.0)
        i0 = np.floor(x).astype(np.int64)
        return i0, np.minimum(i0 + 1, n_src - 1), x - i0

    y0, y1, fy = axis(new_h, h)
    x0, x1, fx = axis(new_w, w)
    fy = fy.reshape((-1, 1) + (1,) * (img.ndim - 2))
    fx = fx.reshape((1, -1) + (1,) * (img.ndim - 2))
    top = img[y0][:, x0] * (1 - fx) + img[y0][:, x1] * fx
    bot = img[y1][:, x0] * (1 - fx) + img[y1][:, x1] * fx
    return top * (1 - fy) + bot * fy


def _bgr(frames: np.ndarray) -> np.ndarray:
    f = np.asarray(frames)
    return np.repeat(f[..., None], 3, axis=3) if f.ndim == 3 else f  # cv.COLOR_GRAY2BGR


def expected_input(frames: np.ndarray, geom: Geometry, resize) -> np.ndarray:
    """uint8 frames [B,H,W] (gray) or [B,H,W,3] (BGR) -> the uint8 network input [B, net_h, net_w, 3] in RGB order for `geom`, resized by
    `resize(img, new_h, new_w)` (oracle/yolo_oracle.py:resize_bilinear_u8 for the expected image)."""
    f = _bgr(frames)
    out = np.full((len(f), geom.net_h, geom.net_w, 3), BORDER, dtype=np.uint8)
    for n, img in enumerate(f):
        if (geom.new_h, geom.new_w) != img.shape[:2]:
            img = resize(img, geom.new_h, geom.new_w)
        out[n, geom.top : geom.top + geom.new_h, geom.left : geom.left + geom.new_w] = img
    return out[..., ::-1]


def ideal_distance(net_in: np.ndarray, frames: np.ndarray, geom: Geometry) -> float:
    """Largest distance, in grey levels, of the pasted region of a uint8 network input [B, net_h, net_w, 3] (RGB) to the ideal bilinear resize."""
    f = _bgr(frames)[..., ::-1]
    worst = 0.0
    for n, img in enumerate(f):
        got = net_in[n, geom.top : geom.top + geom.new_h, geom.left : geom.left + geom.new_w].astype(np.float64)
        if got.shape[:2] != (geom.new_h, geom.new_w):
            return math.inf
        if got.size:
            worst = max(worst, float(np.abs(got - ideal_bilinear(img, geom.new_h, geom.new_w)).max()))
    return worst


def check_network_input(net_in: np.ndarray, frames: np.ndarray, geom: Geometry, expected: np.ndarray) -> float:
    """THE pixel comparison: `net_in` equals `expected` exactly (border included) and every resized pixel is strictly within one grey level of the
    ideal bilinear.  Returns the measured distance to the ideal."""
    assert net_in.shape == expected.shape, (net_in.shape, expected.shape)
    bad = np.argwhere(net_in != expected)
    assert len(bad) == 0, f"{len(bad)} of {net_in.size} network-input values differ from the oracle's, first at [n, y, x, c] = {bad[0].tolist()}: " \
                          f"{net_in[tuple(bad[0])]} != {expected[tuple(bad[0])]} (geometry {geom})"
    d = ideal_distance(net_in, frames, geom)
    assert d < 1.0, f"a resized pixel is {d:.3f} grey levels from the ideal bilinear (geometry {geom})"
    return d


# ---- frame shapes at which the input path can go wrong -----------------------------------------------------------------------------------------
CLASSES = ("a_up", "b_down_gt2", "c_down_2x", "d_odd_pad", "e_round_down", "f_resized_size", "g_pad_tie_x", "g_pad_tie_y", "h_thin_source", "i_pad_only")


def _dyadic(num: int, den: int) -> bool:
    """num / den is a power of two."""
    g = math.gcd(num, den)
    num, den = num // g, den // g
    return (num == 1 and den & (den - 1) == 0) or (den == 1 and num & (num - 1) == 0)


def classify(h: int, w: int, imgsz: int) -> set:
    """The classes of CLASSES that a frame shape falls in (one detector call at `imgsz` on a letterbox_shape handle)."""
    g = letterbox_geometry(h, w, imgsz)
    if g.new_h < 1 or g.new_w < 1:
        return set()
    net = (g.net_h, g.net_w)
    long_side = max(h, w)
    out = set()
    if long_side < imgsz and not _dyadic(imgsz, long_side):
        out.add("a_up")
    if long_side > 2 * imgsz and not _dyadic(imgsz, long_side):
        out.add("b_down_gt2")
    if long_side == 2 * imgsz:
        out.add("c_down_2x")
    if (g.net_h - g.new_h) % 2 or (g.net_w - g.new_w) % 2:
        out.add("d_odd_pad")
    r = min(imgsz / h, imgsz / w)
    for side, new in ((h, g.new_h), (w, g.new_w)):
        frac = side * r - math.floor(side * r)
        if 0.45 <= frac <= 0.5 and new == math.floor(side * r):
            out.add("e_round_down")
    if exact_pad_geometry(h, w, *net)[2:4] != g[2:4]:
        out.add("f_resized_size")
    _, px, py = back_map(net, (h, w))
    _, qx, qy = back_map_float_gain(net, (h, w))
    if px != qx:
        out.add("g_pad_tie_x")
    if py != qy:
        out.add("g_pad_tie_y")
    if min(h, w) <= 2:
        out.add("h_thin_source")
    if long_side == imgsz and min(h, w) < imgsz and net != (h, w):
        out.add("i_pad_only")
    return out


@functools.lru_cache(maxsize=None)
def select_shapes(imgsz: int = 160, max_side: int = 340, per_class: int = 2) -> dict:
    """Sweeps the shapes (h, w) up to max_side on the CPU in a fixed pseudo-random order -> {class: [(h, w), ...]}: per class the first
    `per_class` wide or square shapes and the first `per_class` tall ones (a fault in the row arithmetic must not hide behind column-only picks).
    Every class but (h) draws from ordinary cameras (short side >= 24 px, aspect <= 2.5); (h) draws from the shapes with a side of 1 or 2 pixels.
    A shape may serve several classes.  One more entry, "j_net_shape", holds the first `per_class` shapes (short side >= 24 px, any aspect) of every
    network shape, so that each of the network shapes of `imgsz` (nine at 160: 160 x 160 and a short side of 32 .. 128 either way) is visited."""
    rng = np.random.default_rng(imgsz)
    picks = {c: {False: [], True: []} for c in CLASSES}
    per_net: dict = {}
    for k in rng.permutation(max_side * max_side):
        h, w = int(k) // max_side + 1, int(k) % max_side + 1
        thin = min(h, w) <= 2
        if not thin and min(h, w) >= 24:
            g = letterbox_geometry(h, w, imgsz)
            if len(per_net.setdefault((g.net_h, g.net_w), [])) < per_class:
                per_net[(g.net_h, g.net_w)].append((h, w))
        if not thin and (min(h, w) < 24 or max(h, w) > 2.5 * min(h, w)):
            continue
        for c in classify(h, w, imgsz):
            if thin == (c == "h_thin_source") and len(picks[c][h > w]) < per_class:
                picks[c][h > w].append((h, w))
    out = {c: v[False] + v[True] for c, v in picks.items()}
    out["j_net_shape"] = [s for _, v in sorted(per_net.items()) for s in v]
    return out


def selected_by_net_shape(imgsz: int = 160) -> dict:
    """{network shape: sorted [(h, w), ...]} over every class of select_shapes."""
    out: dict = {}
    for v in select_shapes(imgsz).values():
        for h, w in v:
            g = letterbox_geometry(h, w, imgsz)
            out.setdefault((g.net_h, g.net_w), set()).add((h, w))
    return {k: sorted(v) for k, v in sorted(out.items())}
