"""The host model of the second-look control primitives (tests/harness/recheck_ref.py) against hand-written cases: every expected slot list,
count and queue content below is a literal worked out from the contract in include/wtk_hip.h, so the model is not validated only against the
kernels it judges (tests/test_gpu_recheck.py).  CPU only."""
import numpy as np
import pytest

from harness import recheck_ref as rr

NAN, INF, FLT_MAX = float("nan"), float("inf"), float(np.finfo(np.float32).max)


def f32(*v):
    return np.asarray(v, dtype=np.float32)


def test_select_orders_by_margin():
    m = f32(0.5, 0.1, 0.9, 0.3)
    slots, n_weak, over = rr.select(m, 4, 0.4)
    assert slots.tolist() == [1, 3, 0, 2] and slots.dtype == np.int32 and (n_weak, over) == (2, 0)
    slots, n_weak, over = rr.select(m, 1, 0.4)  # the ceiling cuts one weak row off
    assert slots.tolist() == [1] and (n_weak, over) == (1, 1)
    slots, n_weak, over = rr.select(m, 3, 0.0)
    assert slots.tolist() == [1, 3, 0] and (n_weak, over) == (0, 0)


def test_select_ties_go_to_the_lower_row():
    slots, n_weak, over = rr.select(f32(2, 1, 2, 1, 1, 2), 5, 1.5)
    assert slots.tolist() == [1, 3, 4, 0, 2] and (n_weak, over) == (3, 0)
    # -0.0 and +0.0 are equal: rows 0, 2, 3 tie, whatever their sign bit
    slots, n_weak, over = rr.select(f32(0.0, 1.0, -0.0, 0.0, -1.0), 5, 0.0)
    assert slots.tolist() == [4, 0, 2, 3, 1] and (n_weak, over) == (1, 0)
    slots, _, _ = rr.select(f32(-0.0, 0.0), 2, 1.0)
    assert slots.tolist() == [0, 1]
    slots, _, _ = rr.select(f32(0.0, -0.0), 2, 1.0)
    assert slots.tolist() == [0, 1]


def test_select_margin_equal_to_the_threshold_is_not_weak():
    m = f32(0.25, 0.5, 0.25, 0.75)
    assert rr.select(m, 4, 0.25)[1:] == (0, 0)
    assert rr.select(m, 4, 0.5)[1:] == (2, 0)
    assert rr.select(m, 1, 0.5)[1:] == (1, 1)
    assert rr.select(m, 4, float(np.nextafter(np.float32(0.5), np.float32(1))))[1:] == (3, 0)


def test_select_nan_ranks_as_plus_inf_and_is_never_weak():
    #            0    1    2        3    4    5     6
    m = f32(NAN, INF, FLT_MAX, 1.0, NAN, -INF, INF)
    slots, n_weak, over = rr.select(m, 7, 1e9)
    # -inf, 1.0, FLT_MAX, then NaN = +inf: rows 0, 1, 4, 6 tie and go by row
    assert slots.tolist() == [5, 3, 2, 0, 1, 4, 6] and (n_weak, over) == (2, 0)
    # 3.4e38 is an ordinary number below FLT_MAX (3.4028235e38): it ranks before FLT_MAX, +inf and NaN
    slots, n_weak, over = rr.select(f32(NAN, FLT_MAX, 3.4e38, INF), 4, FLT_MAX)
    assert slots.tolist() == [2, 1, 0, 3] and (n_weak, over) == (1, 0)


def test_select_threshold_plus_inf_looks_twice_at_every_number():
    m = f32(NAN, INF, FLT_MAX, 1.0, NAN, -INF, INF)
    slots, n_weak, over = rr.select(m, 7, INF)  # weak: FLT_MAX, 1.0, -inf; +inf < +inf and NaN < +inf are false
    assert slots.tolist() == [5, 3, 2, 0, 1, 4, 6] and (n_weak, over) == (3, 0)
    slots, n_weak, over = rr.select(m, 2, INF)
    assert slots.tolist() == [5, 3] and (n_weak, over) == (2, 1)
    assert rr.select(f32(NAN, NAN), 2, INF)[1:] == (0, 0)
    assert rr.select(f32(1.0, 2.0), 2, NAN)[1:] == (0, 0)  # nothing is below a NaN threshold


def test_merge_copies_weak_rows_only():
    m = f32(0.1, 0.9, NAN, 0.3, 0.5)
    src = np.arange(100, 120, dtype=np.float32).reshape(5, 4), f32(10, 11, 12, 13, 14), np.arange(20, 25, dtype=np.int32)
    dst = np.zeros((5, 4), dtype=np.float32), np.zeros(5, dtype=np.float32), np.zeros(5, dtype=np.int32)
    # slots: weak row 3, a row at the threshold (4), the NaN row, out-of-range entries, weak row 0
    n = rr.merge(m, [3, 4, 2, -1, 5], 0.5, src[:2] + (None,), dst)  # ... and no source for the anchors
    assert n == 1  # K = 5 slots, B = 5: only slots[0] names a weak row in range (row 0 is not in the list)
    assert dst[0].tolist() == [[0, 0, 0, 0]] * 3 + [[100, 101, 102, 103]] + [[0, 0, 0, 0]]
    assert dst[1].tolist() == [0, 0, 0, 10, 0] and dst[2].tolist() == [0] * 5
    n = rr.merge(m, [0, 3, 1], 0.5, src, (dst[0], None, dst[2]))
    assert n == 2
    assert dst[0].tolist() == [[100, 101, 102, 103], [0, 0, 0, 0], [0, 0, 0, 0], [104, 105, 106, 107], [0, 0, 0, 0]]
    assert dst[1].tolist() == [0, 0, 0, 10, 0] and dst[2].tolist() == [20, 0, 0, 21, 0]
    assert rr.merge(m, [2, 1, 4], INF, src, dst) == 2  # thr = +inf: rows 1 and 4 are numbers, the NaN row stays
    assert dst[2].tolist() == [20, 21, 0, 21, 22]


def test_queue_fills_mid_batch_and_scatters():
    q = rr.Queue(q_cap=3, frame_bytes=2, fill=0xEE, ptr_fill=7)
    # batch 1 at addresses 0x1000 / 0x2000 / 0x3000: rows 0 and 2 are weak (row 1 sits AT the threshold, row 3 is NaN)
    pos = q.enqueue(f32(0.1, 0.5, 0.2, NAN), 0.5, np.asarray([[1, 2], [3, 4], [5, 6], [7, 8]], dtype=np.uint8), (0x1000, 0x2000, 0x3000))
    assert pos.tolist() == [0, -1, 1, -1] and pos.dtype == np.int32 and (q.q_len, q.overflow) == (2, 0)
    assert q.frames.tolist() == [[1, 2], [5, 6], [0xEE, 0xEE]]
    assert q.ptrs.tolist() == [[0x1000, 0x1020, 7], [0x2000, 0x2008, 7], [0x3000, 0x3008, 7]]
    # batch 2 (no conf output): rows 1, 2, 3 are weak, the queue has room for one
    pos = q.enqueue(f32(0.9, 0.0, -1.0, -INF), 0.5, np.asarray([[9, 9], [10, 11], [12, 13], [14, 15]], dtype=np.uint8), (0x5000, 0, 0x6000))
    assert pos.tolist() == [-1, 2, -1, -1] and (q.q_len, q.overflow) == (3, 2)
    assert q.frames.tolist() == [[1, 2], [5, 6], [10, 11]]
    assert q.ptrs.tolist() == [[0x1000, 0x1020, 0x5010], [0x2000, 0x2008, 0], [0x3000, 0x3008, 0x6004]]
    # batch 3 finds the queue full
    pos = q.enqueue(f32(0.0, 0.6), 0.5, np.zeros((2, 2), dtype=np.uint8), (0x7000, 0x7100, 0x7200))
    assert pos.tolist() == [-1, -1] and (q.q_len, q.overflow) == (3, 3)
    # scatter: rows 0, 1, 2 of src to batch 1 rows 0 and 2, batch 2 row 1
    mem = rr.Memory()
    x1, c1, a1 = mem.add(0x1000, np.zeros((4, 4), np.float32)), mem.add(0x2000, np.zeros(4, np.float32)), mem.add(0x3000, np.zeros(4, np.int32))
    x2, a2 = mem.add(0x5000, np.zeros((4, 4), np.float32)), mem.add(0x6000, np.zeros(4, np.int32))
    src = np.arange(1, 13, dtype=np.float32).reshape(3, 4), f32(0.5, 0.25, 0.125), np.asarray([70, 80, 90], dtype=np.int32)
    assert q.scatter(*src, mem) == 3 and (q.q_len, q.replaced) == (0, 3)
    assert x1.tolist() == [[1, 2, 3, 4], [0, 0, 0, 0], [5, 6, 7, 8], [0, 0, 0, 0]] and c1.tolist() == [0.5, 0, 0.25, 0] and a1.tolist() == [70, 0, 80, 0]
    assert x2.tolist() == [[0, 0, 0, 0], [9, 10, 11, 12], [0, 0, 0, 0], [0, 0, 0, 0]] and a2.tolist() == [0, 90, 0, 0]
    # the queue is reused: positions start at 0 again, the slots past q_len keep the last round's frames and addresses
    pos = q.enqueue(f32(0.6, 0.4), 0.5, np.asarray([[20, 21], [22, 23]], dtype=np.uint8), (0x5000, 0, 0))
    assert pos.tolist() == [-1, 0] and (q.q_len, q.overflow) == (1, 3)
    assert q.frames.tolist() == [[22, 23], [5, 6], [10, 11]] and q.ptrs[:, 0].tolist() == [0x5010, 0, 0] and q.ptrs[0, 1:].tolist() == [0x1020, 0x5010]


def test_scatter_on_an_empty_queue_changes_nothing():
    q = rr.Queue(q_cap=2, frame_bytes=1)
    q.ptrs[:] = 0x1000  # stale addresses of an earlier round must not be followed
    mem = rr.Memory()
    x = mem.add(0x1000, np.zeros((1, 4), np.float32))
    assert q.scatter(np.ones((2, 4), np.float32), f32(1, 1), np.ones(2, np.int32), mem) == 0
    assert (q.q_len, q.replaced) == (0, 0) and x.tolist() == [[0, 0, 0, 0]]
    q.enqueue(f32(0.0), 1.0, np.zeros((1, 1), np.uint8), (0x1000, 0, 0))
    assert q.scatter(np.ones((2, 4), np.float32), None, None, mem) == 1 and q.scatter(np.full((2, 4), 5, np.float32), None, None, mem) == 0
    assert (q.q_len, q.replaced) == (0, 1) and x.tolist() == [[1, 1, 1, 1]]


def test_memory_refuses_a_write_outside_its_buffers():
    mem = rr.Memory()
    mem.add(0x100, np.zeros(4, np.float32))
    mem.write(0x10C, np.float32(1))
    for addr in (0xFC, 0x10D, 0x110, 0):
        with pytest.raises(AssertionError):
            mem.write(addr, np.float32(1))
