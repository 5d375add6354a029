"""TEST INFRASTRUCTURE: plain numpy / Python model of the second-look control primitives, written from their contract in include/wtk_hip.h
(wtk_recheck_select[_counted], wtk_recheck_merge, wtk_recheck_enqueue, wtk_recheck_scatter) and not from the kernels in csrc/track_ops.hip.

  select(margins, K, thr)              slot list of the K smallest margins, n_weak, what a call adds to the overflow counter
  merge(margins, slots, thr, src, dst) rows of the second look into the batch's rows; number of rows replaced
  Queue                                the deferred form: enqueue() appends weak rows (frame copy + output addresses), scatter() writes rows back
  Memory                               address -> host copy of a device buffer, so that scatter() can be followed to the byte

One reading of "weak" holds everywhere: a row is weak iff margin < thr on the RAW margin.  NaN < thr is false for every thr, and +inf < +inf is
false, so a NaN row is never weak and with thr = +inf every row but the NaN and +inf ones is.  For the ORDER of select a NaN margin counts as
+inf (it ties with a real +inf, lower row first).

It is pinned, not trusted: tests/test_recheck_ref.py holds it to hand-written slot lists, counts and queue contents; tests/test_gpu_recheck.py
then holds the kernels to it, bit for bit."""
from __future__ import annotations

import math

import numpy as np


def _weak(margins, thr) -> np.ndarray:
    """margin < thr on the raw float32 margins (NaN: False)."""
    m = np.asarray(margins, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return m < np.float32(thr)


def select(margins, K: int, thr: float):
    """-> (slots [K] int32, n_weak, overflow_increment).  slots[k] = row of the k-th smallest margin; ties (equal floats, -0.0 and +0.0 among
    them) go to the lower row; NaN ranks as +inf."""
    m = np.asarray(margins, dtype=np.float32)
    B = len(m)
    assert 1 <= K <= B
    key = [math.inf if math.isnan(float(v)) else float(v) for v in m]
    order = sorted(range(B), key=lambda i: (key[i], i))  # (-0.0, i) and (0.0, j) compare by the row: the floats are equal
    n = int(_weak(m, thr).sum())
    return np.asarray(order[:K], dtype=np.int32), min(K, n), max(n - K, 0)


def merge(margins, slots, thr: float, src, dst) -> int:
    """Row k of every array in `src` goes to row slots[k] of the array of the same position in `dst` (None entries on either side are skipped)
    where 0 <= slots[k] < B and margins[slots[k]] < thr.  `dst` arrays are changed in place; returns the number of rows copied."""
    weak = _weak(margins, thr)
    B, n = len(weak), 0
    for k, row in enumerate(np.asarray(slots).tolist()):
        if not (0 <= row < B) or not weak[row]:
            continue
        for s, d in zip(src, dst):
            if s is not None and d is not None:
                d[row] = s[k]
        n += 1
    return n


class Memory:
    """Host copies of device buffers by address: add(base, array) registers a C-contiguous numpy array as the bytes at [base, base + nbytes);
    write(addr, data) stores the bytes of `data` there.  A write that does not lie inside ONE registered buffer raises."""

    def __init__(self):
        self._regions = []

    def add(self, base: int, array: np.ndarray):
        assert array.flags["C_CONTIGUOUS"]
        self._regions.append((int(base), array.reshape(-1).view(np.uint8)))
        return array

    def write(self, addr: int, data):
        raw = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
        for base, buf in self._regions:
            if base <= addr and addr + raw.size <= base + buf.size:
                buf[addr - base : addr - base + raw.size] = raw
                return
        raise AssertionError(f"write of {raw.size} bytes at {addr:#x} lies in no registered buffer")


class Queue:
    """The device-side queue of the deferred second look.  frames [q_cap][frame_bytes] and the three address tables keep whatever an earlier
    round left in the slots past q_len (so does the device); `fill` is what they hold before the first use."""

    XYWH, CONF, ANCHOR = 0, 1, 2
    STRIDE = (16, 4, 4)  # bytes per row of dst_xywh, dst_conf, dst_anchor

    def __init__(self, q_cap: int, frame_bytes: int, fill: int = 0, ptr_fill: int = 0):
        self.q_cap, self.frame_bytes = int(q_cap), int(frame_bytes)
        self.frames = np.full((q_cap, frame_bytes), fill, dtype=np.uint8)
        self.ptrs = np.full((3, q_cap), ptr_fill, dtype=np.uint64)
        self.q_len = 0
        self.overflow = 0
        self.replaced = 0

    def enqueue(self, margins, thr: float, frames, dst_addresses) -> np.ndarray:
        """Appends, in row order, every row with margin < thr until the queue holds q_cap rows; the weak rows after that count as overflow.
        frames: uint8 [B][frame_bytes]; dst_addresses: (xywh, conf, anchor) base addresses of the batch's outputs, 0 = null (conf / anchor).
        -> pos [B] int32: the row's queue position, or -1."""
        weak = _weak(margins, thr)
        frames = np.asarray(frames, dtype=np.uint8).reshape(len(weak), self.frame_bytes)
        pos = np.full(len(weak), -1, dtype=np.int32)
        for b in np.nonzero(weak)[0].tolist():
            if self.q_len >= self.q_cap:
                self.overflow += 1
                continue
            p = self.q_len
            self.frames[p] = frames[b]
            for t, (base, stride) in enumerate(zip(dst_addresses, self.STRIDE)):
                self.ptrs[t, p] = base + stride * b if base else 0
            pos[b] = p
            self.q_len += 1
        return pos

    def scatter(self, src_xywh, src_conf, src_anchor, memory: Memory) -> int:
        """Rows 0 .. q_len - 1 of src_* go to the recorded addresses (null address or None source: skipped); replaced += q_len; the queue is
        empty afterwards.  -> rows written."""
        n = self.q_len
        for k in range(n):
            memory.write(int(self.ptrs[self.XYWH, k]), src_xywh[k])
            if self.ptrs[self.CONF, k] and src_conf is not None:
                memory.write(int(self.ptrs[self.CONF, k]), src_conf[k])
            if self.ptrs[self.ANCHOR, k] and src_anchor is not None:
                memory.write(int(self.ptrs[self.ANCHOR, k]), src_anchor[k])
        self.replaced += n
        self.q_len = 0
        return n
