"""The kernels that decide which rows get the second look and where its rows land (csrc/track_ops.hip: recheck_select / _merge / _enqueue_plan /
_enqueue_copy / _scatter / _gather_views), called through the C ABI on device tensors and held to the host model tests/harness/recheck_ref.py
(itself pinned on hand-written cases by tests/test_recheck_ref.py).

Every comparison is EXACT and made on raw bits: float buffers are kept, uploaded and read back as unsigned integers, so NaN payloads, the sign of a
zero and sentinel patterns all count.  Every buffer a call may write is the inner part of a larger allocation whose GUARD rows before and after it hold a
sentinel and must come back untouched (_Buf.check compares the whole allocation)."""

import numpy as np
import pytest
import torch

from harness import recheck_ref as rr
from wtracker_amd import hip
from wtracker_amd import yolo_spec as ys
from wtracker_amd.hybrid import HybridDetector

pytestmark = pytest.mark.gpu

GUARD = 3
NAN, INF, FLT_MAX = float("nan"), float("inf"), float(np.finfo(np.float32).max)
SPECIALS = [NAN, INF, -INF, FLT_MAX, 3.4e38, -0.0, 0.0]
_UNSIGNED = {1: np.uint8, 4: np.uint32, 8: np.uint64}
_SIGNED = {1: np.uint8, 4: np.int32, 8: np.int64}  # what torch moves
_GUARD_FILL = {1: 0xA5, 4: 0xA5A5A5A5, 8: 0xA5A5A5A5A5A5A5A5}


class _Buf:
    """A device buffer as the inner rows of a larger allocation.  `host` is the EXPECTED content of the whole allocation as unsigned integers
    (guard rows included); a test changes `inner` as the model says and check() compares the device's bits with it."""

    def __init__(self, inner: np.ndarray):
        size = inner.dtype.itemsize
        raw = np.ascontiguousarray(inner).view(_UNSIGNED[size])
        guard = np.full((GUARD,) + raw.shape[1:], _GUARD_FILL[size], dtype=raw.dtype)
        self.host = np.concatenate([guard, raw, guard])
        self.dev = torch.from_numpy(self.host.view(_SIGNED[size]).copy()).cuda()
        self.t = self.dev[GUARD : GUARD + len(raw)]  # what the call sees (a view: data_ptr() lies inside the allocation)

    @property
    def inner(self) -> np.ndarray:
        return self.host[GUARD : len(self.host) - GUARD]

    @property
    def ptr(self) -> int:
        return self.t.data_ptr()

    def read(self) -> np.ndarray:
        return self.dev.cpu().numpy().view(self.host.dtype)

    def check(self, what=""):
        np.testing.assert_array_equal(self.read(), self.host, err_msg=str(what))

    def value(self) -> int:
        """a one-element counter, as a signed integer"""
        return int(self.read()[GUARD].astype(np.int32 if self.host.dtype == np.uint32 else np.int64))


def _filled(shape, value, dtype=np.uint32):
    return np.full(shape, value, dtype=dtype)


def _counter(value=0):
    return _Buf(np.asarray([value], dtype=np.int32))


def _pattern(rows, cols, base):
    """distinct 32-bit patterns, one per element"""
    shape = (rows, cols) if cols else (rows,)
    return (np.uint32(base) + np.arange(int(np.prod(shape)), dtype=np.uint32)).reshape(shape)


def _f32(v):
    return np.asarray(v, dtype=np.float32)


def _ks(B):
    return sorted({k for k in (1, B // 2, B - 1, B) if 1 <= k <= B})


def _five_values(rng, B):
    return rng.choice(_f32([-1.5, 0.0, 0.25, 0.75, 7.0]), size=B)


def _vectors(kind, B, seed):
    """The margin vectors of one kind for a batch of B (a list: B = 1 takes every special value on its own)."""
    rng = np.random.default_rng(seed)
    if kind == "normals":
        return [_f32(3.0 * rng.standard_normal(B))]
    if kind == "ties":
        return [_five_values(rng, B)]
    if kind == "equal":
        return [_filled(B, 0.125, np.float32)]
    if kind == "descending":
        m = _f32(np.linspace(5.0, -5.0, B))
        assert B == 1 or (np.diff(m) < 0).all()
        return [m]
    assert kind == "special"
    if B == 1:
        return [_f32([v]) for v in SPECIALS]
    m = _five_values(rng, B)
    fixed = [0, B - 1, B // 2, 63 % B, 64 % B, 255 % B, 256 % B]  # ends, middle, either side of a wave and of the 256-thread stride
    for i, row in enumerate(rng.choice(B, size=min(B, 2 * len(SPECIALS)), replace=False).tolist()):
        m[row] = SPECIALS[i % len(SPECIALS)]
    for i, row in enumerate(fixed):
        m[row] = SPECIALS[(i + 2) % len(SPECIALS)]
    return [m]


def _thresholds(m):
    """0, a value of the vector (strict <), a value below every margin, 1e9, +inf"""
    finite = np.sort(m[np.isfinite(m)])
    present = float(finite[len(finite) // 2]) if len(finite) else (0.25 if np.isnan(m[0]) else float(m[0]))
    lowest = np.nanmin(m) if not np.isnan(m).all() else np.float32(0)
    below = float(np.nextafter(np.float32(lowest), np.float32(-INF)))  # (-inf stays -inf: nothing is below it)
    return [0.0, present, below, 1e9, INF]


def _select(margins, B, K, thr, slots, n_weak=None, overflow=None):
    hip.recheck_select(margins.t, B, K, thr, slots.t, None if n_weak is None else n_weak.t, n_overflow_dev=None if overflow is None else overflow.t)


SLOT_FILL = 0x5EEDFACE


@pytest.mark.parametrize("kind", ["normals", "ties", "equal", "descending", "special"])
@pytest.mark.parametrize("B", [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024])
def test_select(hip_lib, B, kind):
    for m in _vectors(kind, B, seed=1000 + B):
        margins = _Buf(m)
        for thr in _thresholds(m):
            for K in _ks(B):
                what = f"B {B} K {K} {kind} thr {thr!r}" + (f" margins {m.tolist()}" if B <= 2 else "")
                want_slots, want_weak, inc = rr.select(m, K, thr)
                slots, n_weak, overflow = _Buf(_filled(K, SLOT_FILL)), _counter(-77), _counter(1000)
                _select(margins, B, K, thr, slots, n_weak, overflow)
                _select(margins, B, K, thr, slots, n_weak, overflow)  # the counter ACCUMULATES, everything else is written again
                plain = _Buf(_filled(K, SLOT_FILL))  # wtk_recheck_select: no overflow counter, and here no n_weak either
                hip._check(hip_lib.wtk_recheck_select(hip._ptr(margins.t), B, K, thr, hip._ptr(plain.t), None, None), "wtk_recheck_select")
                torch.cuda.synchronize()
                slots.inner[:] = want_slots.view(np.uint32)
                plain.inner[:] = want_slots.view(np.uint32)
                n_weak.inner[0], overflow.inner[0] = want_weak, 1000 + 2 * inc
                slots.check(what + ": slots")
                plain.check(what + ": slots of wtk_recheck_select")
                n_weak.check(what + ": n_weak")
                overflow.check(what + ": overflow counter after two calls")
        margins.check("the margins are read only")


def _handmade_slots(rng, B, K):
    """K distinct rows in random order, some of them replaced by -1, B and B + 1 (out of range: the merge skips them)"""
    s = rng.permutation(B)[:K].astype(np.int32)
    n_bad = min(3, K - 1) if K > 1 else int(rng.integers(0, 2))  # K > 1: at least one row stays
    for i, bad in zip(rng.choice(K, size=n_bad, replace=False).tolist(), rng.permutation([-1, B, B + 1]).tolist()):
        s[i] = bad
    return s


@pytest.mark.parametrize("kind", ["ties", "special"])
@pytest.mark.parametrize("B", [1, 64, 65, 257, 1024])
def test_merge(hip_lib, B, kind):
    rng = np.random.default_rng(2000 + B)
    case = 0
    for m in _vectors(kind, B, seed=3000 + B):
        margins = _Buf(m)
        thrs = _thresholds(m)
        for thr in (thrs[1], thrs[3], thrs[4]):  # a value of the vector, 1e9, +inf
            for K in sorted({1, max(B // 2, 1), B}):
                for handmade in (False, True):
                    what = f"B {B} K {K} {kind} thr {thr!r} {'hand-made' if handmade else 'selected'} slots, case {case}"
                    if handmade:
                        slots = _Buf(_handmade_slots(rng, B, K))
                    else:
                        slots = _Buf(_filled(K, SLOT_FILL))
                        _select(margins, B, K, thr, slots)
                        torch.cuda.synchronize()
                        slots.host[:] = slots.read()  # whatever select wrote (test_select judges it): the merge must leave it alone
                    slot_list = slots.inner.view(np.int32)
                    src = [_Buf(_pattern(K, 4, 0x50000000)), _Buf(_pattern(K, 0, 0x60000000)), _Buf(_pattern(K, 0, 0x70000000))]
                    dst = [_Buf(_pattern(B, 4, 0xD0000000)), _Buf(_pattern(B, 0, 0xE0000000)), _Buf(_pattern(B, 0, 0xF0000000))]
                    counter = _counter(7)
                    # one optional output is missing in three of every four cases
                    use = [True, case % 4 != 1, case % 4 != 2]
                    count = case % 4 != 3
                    args = (margins.t, slots.t, B, K, thr, src[0].t, src[1].t, src[2].t, dst[0].t, dst[1].t if use[1] else None, dst[2].t if use[2] else None,
                            counter.t if count else None)
                    hip.recheck_merge(*args)
                    hip.recheck_merge(*args)  # the same rows again: same bits, the counter accumulates
                    torch.cuda.synchronize()
                    n = rr.merge(m, slot_list, thr, [s.inner for s in src], [d.inner if u else None for d, u in zip(dst, use)])
                    if count:
                        counter.inner[0] = 7 + 2 * n
                    for b, nm in zip(dst + src + [slots, counter], ("dst_xywh", "dst_conf", "dst_anchor", "src_xywh", "src_conf", "src_anchor", "slots", "n_replaced")):
                        b.check(f"{what}: {nm}")
                    # said once more without the model: a row whose margin is not below the threshold (NaN included) keeps its bits
                    with np.errstate(invalid="ignore"):
                        strong = ~(m < np.float32(thr))
                    for d, base, cols in zip(dst, (0xD0000000, 0xE0000000, 0xF0000000), (4, 0, 0)):
                        np.testing.assert_array_equal(d.read()[GUARD:-GUARD][strong], _pattern(B, cols, base)[strong], err_msg=what)
                    case += 1
        margins.check("the margins are read only")
    assert case >= 4  # every null-output variant was used


@pytest.mark.parametrize("kind", ["normals", "ties", "special"])
@pytest.mark.parametrize("B", [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024])
def test_select_then_merge_with_k_equal_b_replaces_exactly_the_weak_rows(hip_lib, B, kind):
    """With K = B no row can be cut off: the rows replaced by select + merge are {b : margins[b] < thr} — a NaN row never, at thr = +inf every
    number but +inf — and *n_weak is their count.  Stated on the raw margins, without the model."""
    for m in _vectors(kind, B, seed=4000 + B):
        margins = _Buf(m)
        for thr in _thresholds(m):
            what = f"B {B} {kind} thr {thr!r}" + (f" margins {m.tolist()}" if B <= 2 else "")
            slots, n_weak, overflow, replaced = _Buf(_filled(B, SLOT_FILL)), _counter(-1), _counter(0), _counter(0)
            src, dst = _Buf(_pattern(B, 4, 0x50000000)), _Buf(_pattern(B, 4, 0xD0000000))
            _select(margins, B, B, thr, slots, n_weak, overflow)
            hip.recheck_merge(margins.t, slots.t, B, B, thr, src.t, None, None, dst.t, None, None, replaced.t)
            torch.cuda.synchronize()
            got = np.nonzero((dst.read()[GUARD:-GUARD] != _pattern(B, 4, 0xD0000000)).any(axis=1))[0]
            with np.errstate(invalid="ignore"):
                want = np.nonzero(m < np.float32(thr))[0]
            np.testing.assert_array_equal(got, want, err_msg=what + ": rows replaced")
            assert n_weak.value() == len(want) == replaced.value(), (what, "n_weak", n_weak.value(), "rows with margin < thr", len(want), "n_replaced", replaced.value())
            assert overflow.value() == 0, what
            np.testing.assert_array_equal(dst.read()[:GUARD], dst.host[:GUARD], err_msg=what + ": guard rows before")
            np.testing.assert_array_equal(dst.read()[-GUARD:], dst.host[-GUARD:], err_msg=what + ": guard rows after")


# ---- deferred form -------------------------------------------------------------------------------------------------------------------------------
FRAME_FILL, PTR_FILL = 0xC3, 0x1111111111111111


class _DeviceQueue:
    """The device side of one queue next to its model."""

    def __init__(self, q_cap, frame_bytes):
        self.q_cap, self.frame_bytes = q_cap, frame_bytes
        self.model = rr.Queue(q_cap, frame_bytes, fill=FRAME_FILL, ptr_fill=PTR_FILL)
        self.frames = _Buf(_filled((q_cap, frame_bytes), FRAME_FILL, np.uint8))
        self.ptrs = [_Buf(_filled(q_cap, PTR_FILL, np.uint64)) for _ in range(3)]
        self.q_len, self.overflow, self.replaced = _counter(0), _counter(5), _counter(11)
        self.pos = _Buf(_filled(1024, 0x0BADF00D))
        self.memory = rr.Memory()

    def enqueue(self, m, thr, frames, dst, what):
        """dst: [xywh, conf, anchor] _Bufs of this batch's outputs, conf / anchor may be None"""
        B = len(m)
        margins, fr_buf = _Buf(m), _Buf(frames)
        for d in dst:
            if d is not None:
                self.memory.add(d.ptr, d.inner)
        hip.recheck_enqueue(margins.t, B, thr, fr_buf.t, self.frame_bytes, self.frames.t, self.q_cap, self.q_len.t, self.ptrs[0].t, self.ptrs[1].t, self.ptrs[2].t,
                            dst[0].t, None if dst[1] is None else dst[1].t, None if dst[2] is None else dst[2].t, self.pos.t, self.overflow.t)
        torch.cuda.synchronize()
        pos = self.model.enqueue(m, thr, frames, [0 if d is None else d.ptr for d in dst])
        self.pos.inner[:B] = pos.view(np.uint32)
        self.check(what)
        margins.check(what + ": margins")
        fr_buf.check(what + ": frames")
        return pos

    def check(self, what):
        self.q_len.inner[0], self.overflow.inner[0], self.replaced.inner[0] = self.model.q_len, 5 + self.model.overflow, 11 + self.model.replaced
        self.frames.inner[:] = self.model.frames
        for t in range(3):
            self.ptrs[t].inner[:] = self.model.ptrs[t]
        self.q_len.check(what + ": q_len")
        self.pos.check(what + ": pos_scratch")
        self.overflow.check(what + ": overflow counter")
        for t, nm in enumerate(("xywh", "conf", "anchor")):
            self.ptrs[t].check(f"{what}: {nm} address table")
        self.frames.check(what + ": queued frames and the sentinel bytes of the free slots")
        self.replaced.check(what + ": n_replaced")

    def scatter(self, src):
        hip.recheck_scatter(self.q_len.t, self.q_cap, src[0].t, src[1].t, src[2].t, self.ptrs[0].t, self.ptrs[1].t, self.ptrs[2].t, self.replaced.t)
        torch.cuda.synchronize()


def test_enqueue_and_scatter_one_queue_over_two_rounds(hip_lib):
    frame_bytes, thr = 48, 0.5
    rng = np.random.default_rng(7)
    batches = (1, 64, 257, 1024)

    def margins_of(B, first):
        m = _f32(rng.uniform(0.0, 1.0, size=B))
        m[rng.choice(B, size=max(B // 8, 1), replace=False)] = np.float32(thr)  # AT the threshold: not weak
        if B > 1:
            m[rng.choice(B, size=max(B // 16, 1), replace=False)] = NAN
            m[B - 1] = 0.25  # the last row is weak: the plan kernel takes the batch's total from it
        else:
            m[0] = 0.125 if first else NAN  # one row cannot be weak and NaN at once: round one queues it, round two brings the NaN row
        return m

    ms = [margins_of(B, True) for B in batches]
    weak = [int((m < np.float32(thr)).sum()) for m in ms]  # (NaN < thr is False)
    q_cap = weak[0] + weak[1] + weak[2] // 2  # the third call fills the queue part-way through its weak rows, the fourth finds it full
    assert weak[0] == 1 and weak[1] > 8 and weak[2] > 16 and weak[3] > 64
    q = _DeviceQueue(q_cap, frame_bytes)
    every_dst = []
    for rnd in range(2):
        if rnd:
            ms = [margins_of(B, False) for B in batches]  # other margins (and now the B = 1 batch is a NaN row: the round starts with nothing queued)
        dsts = []
        for call, (B, m) in enumerate(zip(batches, ms)):
            what = f"round {rnd} call {call} (B {B})"
            base = 0x01000000 * (4 * rnd + call + 1)
            dst = [_Buf(_pattern(B, 4, base)), None if call == 1 else _Buf(_pattern(B, 0, base + 0x00400000)), None if call == 2 else _Buf(_pattern(B, 0, base + 0x00800000))]
            dsts.append(dst)
            frames = rng.integers(0, 256, size=(B, frame_bytes), dtype=np.uint8)
            pos = q.enqueue(m, thr, frames, dst, what)
            if rnd == 0 and call == 2:
                queued = pos[m < np.float32(thr)]
                assert (queued >= 0).any() and (queued < 0).any() and q.model.q_len == q_cap, "the third call must fill the queue mid-batch"
            if rnd == 0 and call == 3:
                assert (pos < 0).all() and q.model.overflow == weak[2] - weak[2] // 2 + weak[3]
        every_dst += [d for dst in dsts for d in dst if d is not None]
        src = [_Buf(_pattern(q_cap, 4, 0x80000000 + 0x08000000 * rnd)), _Buf(_pattern(q_cap, 0, 0x90000000 + 0x08000000 * rnd)), _Buf(_pattern(q_cap, 0, 0xA0000000 + 0x08000000 * rnd))]
        old_len = q.model.q_len
        assert old_len > 0
        for again in range(2):  # the second scatter finds an empty queue and changes nothing
            what = f"round {rnd} scatter {again}"
            q.scatter(src)
            n = q.model.scatter(src[0].inner, src[1].inner, src[2].inner, q.memory)
            assert n == (0 if again else old_len) and q.model.q_len == 0
            q.check(what)
            for s in src:
                s.check(what + ": src")
            for i, d in enumerate(every_dst):  # round one's outputs too: an address left over from it must not be written again
                d.check(f"{what}: output buffer {i}")


@pytest.mark.parametrize("n16", [1, 2049, 64 * 2048 + 1], ids=["one-uint4", "second-block", "past-the-64-block-cap"])
def test_enqueue_copies_whole_frames(hip_lib, n16):
    """The frame copy: 16 bytes per thread and step, at most 64 blocks of 256 threads per frame with at least 8 steps each."""
    frame_bytes, B = 16 * n16, 3
    rng = np.random.default_rng(n16)
    q = _DeviceQueue(B + 1, frame_bytes)  # one free slot behind the last queued frame, then the guard rows
    frames = rng.integers(0, 256, size=(B, frame_bytes), dtype=np.uint8)
    dst = [_Buf(_pattern(B, 4, 0x01000000)), _Buf(_pattern(B, 0, 0x02000000)), _Buf(_pattern(B, 0, 0x03000000))]
    pos = q.enqueue(_f32([0.0, -1.0, 0.25]), 0.5, frames, dst, f"frame_bytes {frame_bytes}")
    assert pos.tolist() == [0, 1, 2] and q.model.q_len == 3
    np.testing.assert_array_equal(q.frames.read()[GUARD : GUARD + B], frames)
    for d in dst:
        d.check("enqueue writes no output row")


# ---- views form of the hybrid object -------------------------------------------------------------------------------------------------------------
def test_hybrid_views_gather_frame_index_and_view_centres(hip_lib):
    """wtk_hybrid_predict_views with a frame_index (a permutation with a repeat) and distinct view centres, one view hanging over the frame's
    edge: the second look must read the frame and the centre of ITS batch row.  Rows are compared with each handle's own predict_views rows.
    Scale s is the smallest network an f16x3 handle exists for (channel widths in multiples of 64: wtk_yolo_create refuses scale n)."""
    S, H, W, B, conf = 128, 200, 260, 5, 0.0
    w = ys.synthetic_weights("s", 1, seed=0)
    depth, width, maxch = ys.SCALES["s"]
    mk = lambda dtype: hip.HipYolo(w, (S, S), B, dtype=dtype, nc=1, width=width, depth=depth, max_channels=maxch)
    fast, exact = mk("fp16"), mk("f16x3")
    rng = np.random.default_rng(5)
    frames = np.clip(rng.integers(0, 256, size=(4, H, W)) * 0.5 + np.linspace(0, 127, W)[None, None, :] * np.asarray([1.0, 0.2, 0.6, 0.0])[:, None, None], 0, 255).astype(np.uint8)
    dev = torch.from_numpy(frames).cuda()
    idx = torch.tensor([3, 0, 3, 1, 2], dtype=torch.int32, device="cuda")
    pos = torch.tensor([[130, 100], [90, 70], [180, 120], [10, 190], [140, 64]], dtype=torch.int32, device="cuda")  # (x, y); the fourth view leaves the frame on two sides

    def outs():
        return [_Buf(_filled((B, 4), 0xFFC0DEAD)), _Buf(_filled(B, 0xFFC0DEAD)), _Buf(_filled(B, 0x0BADF00D))]

    def own_rows(det):
        o = outs()
        det.predict_views(dev, 4, H, W, 1, idx, pos, B, S, S, o[0].t, o[1].t, o[2].t, conf=conf)
        torch.cuda.synchronize()
        return [b.read()[GUARD:-GUARD].copy() for b in o]

    # each handle standalone, BEFORE a hybrid object owns the exact one
    fast_rows = own_rows(fast)
    margins = fast.last_margins(B)
    exact_rows = own_rows(exact)
    assert np.isfinite(margins).all()
    differ = (fast_rows[0] != exact_rows[0]).any(axis=1) | (fast_rows[1] != exact_rows[1])
    assert differ.all(), ("every row must tell the two handles apart for the comparisons below to mean anything", differ)

    def run(hyb, want, counters, what):
        o = outs()
        hyb.predict_views(dev, 4, H, W, 1, idx, pos, B, S, S, o[0].t, o[1].t, o[2].t, conf=conf)
        torch.cuda.synchronize()
        for b, rows, nm in zip(o, want, ("xywh", "conf", "anchor")):
            b.inner[:] = rows
            b.check(f"{what}: {nm}")
        assert hyb._counters() == counters, (what, hyb._counters(), counters)

    hyb = HybridDetector(fast, exact, margin=1e9)
    assert hyb.k == B
    run(hyb, exact_rows, (5, 0), "margin 1e9: every row is the exact handle's")
    hyb.margin = 0.0
    run(hyb, fast_rows, (5, 0), "margin 0: every row is the fast handle's")  # the counters are cumulative: this call replaced 0 rows
    hyb._release()
    # a ceiling of two rows: the two weakest rows get the second look, three are cut off and counted
    hyb = HybridDetector(fast, exact, margin=1e9, k=2)
    slots, n_weak, inc = rr.select(margins, 2, 1e9)
    assert (n_weak, inc) == (2, 3)
    mixed = [np.where((np.isin(np.arange(B), slots))[(slice(None),) + (None,) * (f.ndim - 1)], e, f) for f, e in zip(fast_rows, exact_rows)]
    run(hyb, mixed, (2, 3), f"k = 2: rows {slots.tolist()} are the exact handle's")
    hyb.close()
