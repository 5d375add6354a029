"""An independent model of the Detect head's decisions (csrc/head.hip: head_scan, head_row, head_select_kernel, head_nms_kernel and the range-guard
flag) in NumPy, and the case lists that tests/test_head_ref.py (CPU: the model against oracle/yolo_oracle.py, planted defects) and
tests/test_gpu_head.py (the kernels against the model) both run.  It shares nothing with the oracle (torch fp32) or with the library; boxes come from
harness/input_ref.py (decode_anchor64, scale_boxes64).

What the model states:
  select  the survivor of one frame: the best class logit of every anchor over the nc real classes, the score 1 / (1 + exp(-m)) in float32, the highest
          score (lowest anchor index among equal scores), kept iff score > conf; the decision margin min(l_best - max logit over all OTHER anchors,
          |l_best - logit(conf)|) in float32 arithmetic on the logits.  An anchor whose best logit is NaN never wins and is no runner-up.
  nms     greedy class-aware NMS: first maximum as the class, candidates score > conf, boxes in float64 rounded to float32 and shifted by
          float32(class) * 7680 in float32, highest score first (lower index on ties), suppress iff IoU > iou, stop at max_det.  Every pair it evaluates
          with a non-empty intersection also yields its GUARD: |IoU - iou| over the pair's sensitivity 8 ulp / shortest side (an upper estimate of the IoU
          change from moving each of the eight coordinates by one float32 ulp at their shifted magnitude).
  status  whether the range-guard flag must be raised: a non-finite class logit anywhere in the rows, or a non-finite box logit of an anchor whose box the
          path decodes (select: the survivor; nms: every candidate).

`defect` plants ONE changed line (DEFECTS); tests/test_head_ref.py shows that every one of them changes the expected result of a named case below.

Input conditions of the case lists (check_conditions; they keep the comparison well defined whatever expf a device has):
  * within a frame any two unequal best logits are both >= 17 (score exactly 1.0f: the tie goes by index) or their float64 sigmoids differ by more than
    2^-21; all logits lie on the fp16 grid, none in (9, 17), no finite one below -80;
  * every evaluated NMS pair lies at least 2 sensitivities from iou (but the pairs of iou_threshold_cases, built to sit on it exactly);
  * at most 400 candidates per frame."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import NamedTuple

import numpy as np

from harness import input_ref as ir
from wtracker_amd import yolo_spec as ys

F32 = np.float32
NMS_MAX_WH = F32(7680.0)
NET_SHAPES = ((32, 32), (256, 256), (224, 352), (640, 640))
MAX_BATCH = 8
MAX_CANDIDATES = 400
MIN_GUARD = 2.0

DEFECTS = ("order_by_logit", "tie_highest_index", "second_same_thread_only", "second_same_wave_only", "second_same_pass_only", "score_ge_conf", "iou_ge",
           "no_class_offset", "last_max_class", "max_over_cls_ld", "square_level_split")


# ---- geometry ------------------------------------------------------------------------------------------------------------------------------------
def level_sizes(net_hw: tuple) -> tuple:
    """(A0, A1, A2): anchors per level, level-major as the head stores them."""
    return tuple((net_hw[0] // s) * (net_hw[1] // s) for s in ys.STRIDES)


def n_anchors(net_hw: tuple) -> int:
    return sum(level_sizes(net_hw))


def _split_net(net_hw: tuple, defect) -> tuple:
    return (net_hw[1], net_hw[1]) if defect == "square_level_split" else net_hw  # planted: the level split of a square map


def _decode(box_row, anchor: int, net_hw: tuple, defect) -> np.ndarray:
    try:
        with np.errstate(invalid="ignore"):  # (a non-finite box logit gives a NaN box)
            return ir.decode_anchor64(box_row, anchor, _split_net(net_hw, defect))
    except AssertionError:
        return np.full(4, np.nan)


def xywh_rows(box, anchors, net_hw: tuple, img_hw: tuple, defect=None) -> np.ndarray:
    """float64 rows [x, y, w, h] of `anchors` (-1: the NaN row) of frames box [B, A, 64]: DFL decode, scale_boxes, clip."""
    out = np.full((len(anchors), 4), np.nan)
    for n, a in enumerate(anchors):
        if a >= 0:
            b = ir.scale_boxes64(net_hw, _decode(box[n][int(a)], int(a), net_hw, defect), img_hw)[1][0]
            out[n] = [b[0], b[1], b[2] - b[0], b[3] - b[1]]
    return out


# ---- the decisions -------------------------------------------------------------------------------------------------------------------------------
def score32(m) -> np.ndarray:
    """The library's expression in float32."""
    m = np.asarray(m, dtype=F32)
    with np.errstate(over="ignore", invalid="ignore"):
        return (F32(1) / (F32(1) + np.exp(-m))).astype(F32)


def conf_logit(conf: float) -> np.float32:
    c = F32(conf)
    if c <= 0:
        return F32(-np.inf)
    if c >= 1:
        return F32(np.inf)
    return F32(np.log(c / (F32(1) - c)))


def _stored(cls, defect) -> np.ndarray:
    cls = np.asarray(cls, dtype=F32)
    if defect == "max_over_cls_ld":  # planted: the zero-filled padding columns of the stored row take part
        ld = (cls.shape[1] + 7) // 8 * 8
        return np.concatenate([cls, np.zeros((cls.shape[0], ld - cls.shape[1]), F32)], axis=1)
    return cls


class Sel(NamedTuple):
    anchor: int      # -1: none kept
    conf: np.float32 # 0: none kept
    margin: np.float32
    gap: np.float32  # l_best - best other logit
    thr: np.float32  # |l_best - logit(conf)|
    l_best: np.float32
    winner: int      # the anchor the margin speaks of, kept or not (-1: every anchor NaN)


def select(cls, conf: float, defect=None) -> Sel:
    """cls [A, nc] float32 of ONE frame."""
    c = _stored(cls, defect)
    m = np.fmax.reduce(c, axis=1)  # NaN only where every class is NaN
    s = score32(m)
    valid = ~np.isnan(m)
    nan = F32(np.nan)
    if not valid.any():
        return Sel(-1, F32(0), nan, nan, nan, nan, -1)
    key = np.where(valid, m if defect == "order_by_logit" else s, -np.inf)
    w = int(len(key) - 1 - np.argmax(key[::-1])) if defect == "tie_highest_index" else int(np.argmax(key))
    idx = np.arange(len(m))
    others = valid & (idx != w)
    if defect == "second_same_thread_only":
        others &= idx % 1024 == w % 1024
    if defect == "second_same_wave_only":
        others &= (idx % 1024) // 64 == (w % 1024) // 64
    if defect == "second_same_pass_only":
        others &= idx // 1024 == w // 1024
    second = m[others].max() if others.any() else F32(-np.inf)
    with np.errstate(invalid="ignore"):
        gap = F32(m[w] - second)
        thr = F32(np.abs(F32(m[w] - conf_logit(conf))))
    margin = F32(np.fmin(gap, thr))
    keep = s[w] >= F32(conf) if defect == "score_ge_conf" else s[w] > F32(conf)
    return Sel(w if keep else -1, s[w] if keep else F32(0), margin, gap, thr, m[w], w)


class Nms(NamedTuple):
    anchors: np.ndarray     # kept, in order
    classes: np.ndarray
    scores: np.ndarray
    xyxy: np.ndarray        # float64 [k, 4] network pixels, unshifted
    candidates: np.ndarray  # every anchor whose box the path decodes
    guards: np.ndarray      # per evaluated pair with a non-empty intersection: |IoU - iou| / sensitivity


def nms(box, cls, net_hw: tuple, conf: float, iou: float, max_det: int, defect=None) -> Nms:
    """box [A, 64], cls [A, nc] of ONE frame."""
    c = _stored(cls, defect)
    k = c.shape[1] - 1 - np.argmax(c[:, ::-1], axis=1) if defect == "last_max_class" else np.argmax(c, axis=1)
    s = score32(c[np.arange(len(c)), k])
    with np.errstate(invalid="ignore"):
        cand = np.flatnonzero(s >= F32(conf) if defect == "score_ge_conf" else s > F32(conf))
    order = cand[np.argsort(-s[cand].astype(np.float64), kind="stable")]
    if len(order) == 0:
        return Nms(np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, F32), np.zeros((0, 4)), cand, np.zeros(0))
    b64 = np.stack([_decode(box[a], int(a), net_hw, defect) for a in order])
    shift = np.zeros(len(order), F32) if defect == "no_class_offset" else k[order].astype(F32) * NMS_MAX_WH
    off = (b64.astype(F32) + shift[:, None]).astype(np.float64)  # the float32 sum, then exact
    thr = float(F32(iou))
    alive = np.ones(len(order), dtype=bool)
    kept, guards = [], []
    for i in range(len(order)):
        if not alive[i]:
            continue
        kept.append(i)
        if len(kept) >= max_det:
            break
        rest = np.flatnonzero(alive[i + 1 :]) + i + 1
        if len(rest) == 0:
            continue
        a, bs = off[i], off[rest]
        iw = np.minimum(a[2], bs[:, 2]) - np.maximum(a[0], bs[:, 0])
        ih = np.minimum(a[3], bs[:, 3]) - np.maximum(a[1], bs[:, 1])
        inter = iw.clip(min=0) * ih.clip(min=0)
        with np.errstate(invalid="ignore", divide="ignore"):
            v = inter / ((a[2] - a[0]) * (a[3] - a[1]) + (bs[:, 2] - bs[:, 0]) * (bs[:, 3] - bs[:, 1]) - inter)
            ulp = np.spacing(np.maximum(np.abs(a).max(), np.abs(bs).max(axis=1)).astype(F32)).astype(np.float64)
            shortest = np.minimum(min(a[2] - a[0], a[3] - a[1]), np.minimum(bs[:, 2] - bs[:, 0], bs[:, 3] - bs[:, 1]))
            g = np.abs(v - thr) / (8 * ulp / shortest)
            guards.extend(g[inter > 0].tolist())
            alive[rest[v >= thr if defect == "iou_ge" else v > thr]] = False
    kept = np.array(kept, dtype=np.int64)
    return Nms(order[kept], k[order][kept], s[order][kept], b64[kept], cand, np.array(guards))


def status(box, cls, read) -> bool:
    """box [B, A, 64], cls [B, A, nc]; read[n]: the anchors of row n whose box logits the path decodes."""
    if not np.isfinite(np.asarray(cls)).all():
        return True
    return any(not np.isfinite(box[n][np.asarray(r, dtype=np.int64)]).all() for n, r in enumerate(read) if len(r))


def check_conditions(cls) -> None:
    """The input conditions on the class logits of frames cls [B, A, nc] (module docstring)."""
    cls = np.asarray(cls, dtype=F32)
    fin = cls[np.isfinite(cls)]
    assert (fin.astype(np.float16).astype(F32) == fin).all(), "a logit is not on the fp16 grid"
    assert not ((fin > 9) & (fin < 17)).any() and not (fin < -80).any(), "a logit in (9, 17) or below -80"
    for n in range(cls.shape[0]):
        m = np.fmax.reduce(cls[n], axis=1)
        u = np.unique(m[~np.isnan(m)]).astype(np.float64)
        if len(u) < 2:
            continue
        with np.errstate(over="ignore"):
            sg = 1.0 / (1.0 + np.exp(-u))
        bad = ~((u[:-1] >= 17) | (np.diff(sg) > 2.0**-21))
        assert not bad.any(), f"row {n}: best logits {u[:-1][bad][:3]} and their successors have float64 sigmoids within 2^-21"


# ---- case lists ----------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    """Frames of one handle shape.  box is [rows, A, 64] or [1, A, 64] (every row the same); a detector call takes at most MAX_BATCH rows (calls())."""
    name: str
    net: tuple
    nc: int
    conf: float
    cls: np.ndarray
    box: np.ndarray
    rows: list = field(default_factory=list)  # a name per row
    img: tuple = None
    nms: tuple = ()  # the (max_det, iou) of its NMS calls; empty: a case of the select path
    batch: int = MAX_BATCH

    def __post_init__(self):
        if self.img is None:
            self.img = (2 * self.net[0] - 6, 2 * self.net[1])  # gain 0.5, pad_y 1: a back map that is not the identity
        if not self.rows:
            self.rows = [f"row {n}" for n in range(len(self.cls))]
        assert self.cls.shape[1:] == (n_anchors(self.net), self.nc) and len(self.rows) == len(self.cls)

    def calls(self):
        """(first row, box [B, A, 64], cls [B, A, nc]) per detector call."""
        for lo in range(0, len(self.cls), self.batch):
            c = self.cls[lo : lo + self.batch]
            b = self.box[lo : lo + self.batch] if len(self.box) == len(self.cls) else np.broadcast_to(self.box, (len(c),) + self.box.shape[1:])
            yield lo, np.ascontiguousarray(b), np.ascontiguousarray(c)


def _grid(x):
    return np.asarray(x).astype(np.float16).astype(F32)


def _grid256(x):
    """Multiples of 2^-8 on the fp16 grid: two unequal values within [-9, 9] have sigmoids more than 2^-21 apart (at 9 the grid is 2^-7 and the slope
    1.2e-4; the bare fp16 grid is far finer than that near zero)."""
    return _grid(np.round(np.asarray(x) * 256) / 256)


def _box_table(net, seed, sd=2.0):
    return _grid(np.random.default_rng(seed).normal(0, sd, size=(1, n_anchors(net), 64)))


def placement_pairs(net: tuple) -> list:
    """(name, winner, runner-up) of the placement matrix of one shape: every way the two can lie in the 1024-thread scan."""
    A0, A1, _ = level_sizes(net)
    A = n_anchors(net)
    out = []

    def add(name, w, r):
        if 0 <= w < A and 0 <= r < A and w != r and (w, r) not in [(p[1], p[2]) for p in out]:
            out.append((f"{name}: w = {w}, r = {r}", w, r))

    for k in range(1, (A + 1023) // 1024):  # the same thread, k passes apart
        add(f"same thread, {k} passes later", 5, 5 + 1024 * k)
        add(f"same thread, {k} passes earlier", 5 + 1024 * k, 5)
    w0 = 1024 + 64 * 3 + 21 if A > 1024 + 64 * 4 else 5
    for off in (1, 2, 4, 8, 16, 32):  # the butterfly's six steps
        add(f"lane ^ {off}", w0, w0 ^ off)
        add(f"lane ^ {off}, reversed", w0 ^ off, w0)
    add("same wave, other lane", 64 * 2 + 3, 64 * 2 + 60)
    add("same wave, other lane, other pass", 64 * 2 + 3, 1024 + 64 * 2 + 60)
    add("wave 0 against wave 15", 7, 15 * 64 + 9)
    add("wave 15 against wave 0", 15 * 64 + 9, 7)
    add("wave 15 against wave 0 of the next pass", 15 * 64 + 9, 1024 + 7)
    add("wave 3 against wave 9 of the last pass", (A - 1) // 1024 * 1024 + 3 * 64 + 1, 9 * 64 + 2)
    for b in (A0 - 1, A0, A0 + A1 - 1, A0 + A1, A - 1):  # both sides of every level boundary
        other = (b + 517) % A
        add("winner at a level boundary", b, other)
        add("runner-up at a level boundary", other, b)
    add("across the P3 / P4 boundary", A0 - 1, A0)
    add("across the P3 / P4 boundary, reversed", A0, A0 - 1)
    add("across the P4 / P5 boundary", A0 + A1 - 1, A0 + A1)
    add("across the P4 / P5 boundary, reversed", A0 + A1, A0 + A1 - 1)
    add("winner in the partial last pass", A - 3, 100 % A)
    add("runner-up in the partial last pass", 100 % A, A - 3)
    add("small shape: neighbours", 2, 3)
    add("small shape: far apart", A - 2, 0)
    return out


def placement_case(net: tuple) -> Case:
    """Case a: a constant background of -8, one (winner, runner-up) pair per row with the top-2 gap binding (3.0 against 1.5 at conf 0.25), the same pairs
    with the threshold term binding (-0.5 against -6), exact ties and saturated scores in different passes."""
    A = n_anchors(net)
    pairs = placement_pairs(net)
    rows, cls = [], []

    def row(name, values):
        c = np.full((A, 1), -8.0, F32)
        for a, v in values.items():
            c[a % A, 0] = v
        rows.append(name)
        cls.append(c)

    for name, w, r in pairs:
        row(name, {w: 3.0, r: 1.5})
    for name, w, r in pairs[:: max(1, len(pairs) // 6)]:
        row("threshold binds, " + name, {w: -0.5, r: -6.0})
    row("three-way tie across the passes", {A - 1: 3.0, A // 2: 3.0, 3: 3.0})
    row("tie of the last anchor of a pass with the first of the next", {min(1023, A - 2): 2.5, min(1024, A - 1): 2.5})
    row("tie within a wave", {64 * 2 + 40 if A > 200 else 9: 4.0, 64 * 2 + 11 if A > 200 else 4: 4.0})
    row("saturated scores in different passes: the lowest index wins, the margin is negative", {A - 2: 25.0, 1030: 17.0, 2060 + 13: 18.0, 3 * 1024 + 500: 17.5})
    row("one saturated anchor at the end against ordinary ones", {A - 1: 30.0, 0: 9.0})
    row("nothing above conf", {A // 3: -3.0})
    return Case(f"placement {net[0]}x{net[1]}", net, 1, 0.25, np.stack(cls), _box_table(net, 11), rows)


RANDOM_CHUNKS = (8, 8, 8, 8, 8, 8, 8, 8, 5)  # 69 rows per (shape, nc), 207 per shape; the last call has B < max_batch


def random_cases(net: tuple, nc: int) -> list:
    """Case b: fp16-grid logits (_grid256) from N(-4, 2) clipped to [-9, 9] (the input conditions), conf 0.25 and 0.9 by turns; for nc = 20 (stored as cls_ld = 24) one
    more case whose every real logit is negative at conf 0.1."""
    A = n_anchors(net)
    rng = np.random.default_rng(1000 * net[0] + net[1] + nc)
    n = sum(RANDOM_CHUNKS)
    out = []
    for k, conf in enumerate((0.25, 0.9)):
        rows = 40 if k == 0 else n - 40  # 40 = 5 full calls, 29 = 3 full calls and one of 5
        cls = _grid256(rng.normal(-4, 2, size=(rows, A, nc)).clip(-9, 9))
        out.append(Case(f"random {net[0]}x{net[1]} nc {nc} conf {conf}", net, nc, conf, cls, _box_table(net, 17 + k)))
    if nc == 20:
        cls = _grid256(rng.normal(-4, 2, size=(16, A, nc)).clip(-9, -0.5))
        out.append(Case(f"random {net[0]}x{net[1]} nc {nc}, every real logit negative", net, nc, 0.1, cls, _box_table(net, 19)))
    return out


HALF_BELOW = float(np.nextafter(F32(0.5), F32(0)))


def threshold_cases() -> list:
    """Case c: the strictness of score > conf.  Logit 0 has the score 0.5 exactly."""
    net = (256, 256)
    A = n_anchors(net)
    cls = np.full((4, A, 1), -8.0, F32)
    cls[0, 1100, 0] = 0.0
    cls[1, 77, 0], cls[1, 1300, 0] = 3.0, 1.0
    cls[2, 500, 0] = 20.0
    rows = ["logit 0 in the second pass", "an ordinary frame", "a saturated score", "background only"]
    return [Case(f"thresholds conf {c!r}", net, 1, c, cls, _box_table(net, 23), rows) for c in (0.5, HALF_BELOW, 0.0, 1.0)]


def _sharp(box, n, a, bins):
    box[n, a] = -8.0
    for side, b in enumerate(bins):
        box[n, a, 16 * side + b] = 8.0


NMS_PLANS = ((300, 0.6), (5, 0.45), (1, 0.6))


def nms_case(net: tuple, nc: int) -> Case:
    """Case d: six frames, two calls of B = 3.  iou is 0.6 (0.45 for max_det 5): 3-bin boxes one anchor apart have IoU 0.714, two apart 0.5, diagonal 0.532."""
    A0, A1, A2 = level_sizes(net)
    A = A0 + A1 + A2
    lw0, lw1, lw2 = (net[1] // s for s in ys.STRIDES)
    hi, mid = (79, 40) if nc == 80 else (0, 0)
    rng = np.random.default_rng(31)
    box = _grid(rng.normal(0, 1, size=(6, A, 64)))
    cls = np.full((6, A, nc), -9.0, F32)
    small = net[0] < 64
    if small:  # 32 x 32: A = 21, every anchor a candidate, max_det 300 > A
        for a in range(A):
            _sharp(box, 0, a, (0, 0, 1, 1))
            cls[0, a, 0] = _grid(3.0 - 0.125 * ((a * 5) % A))
        cls[1, [2, 17, 20], 0] = 2.0
        _sharp(box, 1, 2, (0, 0, 1, 1)), _sharp(box, 1, 17, (0, 0, 1, 1)), _sharp(box, 1, 20, (0, 0, 1, 1))
        box[4, 5] = box[4, 6] = 0.0
        cls[4, 5, 0], cls[4, 6, 0] = 4.0, 3.5
        cls[5, 20, 0], cls[5, 0, 0] = 20.0, 18.0
        _sharp(box, 5, 20, (0, 0, 1, 1)), _sharp(box, 5, 0, (0, 0, 1, 1))
    else:
        # frame 0: clusters of 3 x 2 neighbouring anchors with 3-bin boxes: classes 0, 40, 79 on P3, one more on P4 (class 40)
        for (cx, cy, s0, kc, first, lw) in ((4, 4, 4.0, 0, 0, lw0), (20, 10, 3.0, mid, 0, lw0), (34, 20, 2.0, hi, 0, lw0), (5, 10, 5.0, mid, A0, lw1)):
            for dx in range(3):
                for dy in range(2):
                    a = first + (cy + dy) * lw + cx + dx
                    _sharp(box, 0, a, (3, 3, 3, 3))
                    cls[0, a, kc] = s0 - 0.25 * (dx + 2 * dy)
        # frame 1: exact score ties across the passes and the levels, 2-bin boxes far apart
        for a in (17, 1041, 600, A0 + 30, A - 1):
            _sharp(box, 1, a, (2, 2, 2, 2))
            cls[1, a, 0] = 2.0
        # frame 2: no candidate.  frame 3: 320 > max_det candidates of distinct scores, each box its own 8-pixel cell, every other P3 anchor
        for k in range(320):
            _sharp(box, 3, 2 * k, (0, 0, 1, 1))
            cls[3, 2 * k, (k % 3) * (nc // 3)] = _grid(8.0 - 7.0 * ((k * 131) % 320) / 320)
        # frame 4: the same box (uniform DFL, one anchor apart: IoU 0.875) under two classes; a tie of two classes in one anchor
        box[4, 100] = box[4, 101] = 0.0
        cls[4, 100, 0], cls[4, 101, hi] = 4.0, 3.5
        if nc > 1:
            cls[4, 500, 3] = cls[4, 500, 7] = 3.0
        else:
            cls[4, 500, 0] = 3.0
        _sharp(box, 4, 500, (1, 1, 1, 1))
        # frame 5: a P5 cluster at the end of the last pass (class 40), two saturated scores in index order, a lone box on P4
        for d in range(3):
            _sharp(box, 5, A - 1 - d, (3, 3, 3, 3))
            cls[5, A - 1 - d, mid] = 6.0 - 0.5 * d
        cls[5, 1500, 0], cls[5, 70, 0] = 20.0, 18.0
        _sharp(box, 5, 1500, (2, 2, 2, 2)), _sharp(box, 5, 70, (2, 2, 2, 2))
        cls[5, A0 + A1 // 2, hi] = 1.0
        _sharp(box, 5, A0 + A1 // 2, (1, 2, 3, 4))
    rows = ["clusters", "score ties", "no candidate", "more candidates than max_det", "one box under two classes", "last pass, saturated"]
    return Case(f"nms {net[0]}x{net[1]} nc {nc}", net, nc, 0.25, cls, box, rows, nms=NMS_PLANS, batch=3)


NMS_SHAPES = (((32, 32), 1), ((224, 352), 1), ((224, 352), 80), ((640, 640), 1), ((640, 640), 80))


def iou_threshold_cases() -> list:
    """Case e: uniform DFL logits (every side exactly 7.5 bins in fp32), two P3 anchors five columns apart in class 0: 120 px boxes 40 px apart,
    IoU = 80 / 160 = 0.5 exactly.  Both are kept at iou 0.5, the second is suppressed just below."""
    net = (256, 256)
    A = n_anchors(net)
    cls = np.full((2, A, 1), -9.0, F32)
    cls[0, 10 * 32 + 10, 0], cls[0, 10 * 32 + 15, 0] = 3.0, 2.0
    cls[1, 12 * 32 + 20, 0], cls[1, 12 * 32 + 15, 0] = 3.0, 2.0  # the later anchor first
    box = np.zeros((1, A, 64), F32)
    rows = ["five columns apart", "five columns apart, the higher index first"]
    return [Case(f"iou threshold {t!r}", net, 1, 0.25, cls, box, rows, img=net, nms=((300, t),), batch=2) for t in (0.5, HALF_BELOW)]


# Every case list with finite logits by key (the non-finite frames: nonfinite_cases): built on demand, the largest holds 100 MB of logits.
CASE_KEYS = ([("placement", net, 1) for net in NET_SHAPES] + [("random", net, nc) for net in NET_SHAPES for nc in (1, 20, 80)] + [("thresholds", (256, 256), 1)] +
             [("nms", net, nc) for net, nc in NMS_SHAPES] + [("iou_threshold", (256, 256), 1)])


def key_id(key) -> str:
    return f"{key[0]}-{key[1][0]}x{key[1][1]}-nc{key[2]}"


def build_cases(key) -> list:
    kind, net, nc = key
    if kind == "placement":
        return [placement_case(net)]
    if kind == "random":
        return random_cases(net, nc)
    if kind == "thresholds":
        return threshold_cases()
    if kind == "nms":
        return [nms_case(net, nc)]
    assert kind == "iou_threshold"
    return iou_threshold_cases()


NONFINITE_NET = (256, 256)


def nonfinite_cases() -> list:
    """Case f: (name, cls [3, A, 1], box [3, A, 64]) of B = 3 rows on a 256 x 256 handle (A = 1344: a full pass and a partial one).  The clean frames hold
    two candidates each but row 0: row 1 has 77 (3.0) and 1300 (1.0), row 2 has 1200 (4.0) and 3 (3.5); everything else is background (-8)."""
    A = n_anchors(NONFINITE_NET)
    inf, nan = F32(np.inf), F32(np.nan)
    base_cls = np.full((3, A, 1), -8.0, F32)
    base_cls[0, 40, 0], base_cls[1, 77, 0], base_cls[1, 1300, 0], base_cls[2, 1200, 0], base_cls[2, 3, 0] = 2.0, 3.0, 1.0, 4.0, 3.5
    base_box = np.broadcast_to(_box_table(NONFINITE_NET, 29), (3, A, 64)).copy()
    out = [("clean", base_cls.copy(), base_box.copy())]

    def case(name, edits_cls=(), edits_box=()):
        c, b = base_cls.copy(), base_box.copy()
        for n, a, v in edits_cls:
            c[n, a, 0] = v
        for n, a, k, v in edits_box:
            b[n, a, k] = v
        out.append((name, c, b))

    case("NaN in the first pass of row 0", [(0, 3, nan)])
    case("NaN where the winner would be: the selection steps over it", [(1, 77, nan)])
    case("+inf in the last pass of row 1 behind a saturated score: the index rule", [(1, 1100, inf), (1, 50, 18.0)])
    case("+inf alone wins", [(2, 1343, inf)])
    case("-inf at the last anchor of the last row never wins", [(2, A - 1, -inf)])
    case("an all-NaN frame", [(1, a, nan) for a in range(A)])
    case("+inf in a box logit of the survivor", (), [(1, 77, 17, inf)])
    case("NaN in a box logit of the survivor of the last row", (), [(2, 1200, 63, nan)])
    case("-inf in a box logit of the runner-up: a candidate of the NMS path, never read by the select path", (), [(1, 1300, 5, -inf)])
    case("NaN in a box logit of a background anchor: no path reads it", (), [(0, 0, 0, nan), (2, A - 1, 63, inf)])
    return out
