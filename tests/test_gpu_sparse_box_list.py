"""The LIST form of the sparse Detect box towers (DESIGN.md "Sparse box towers"): head_select_kernel_sparse lists the live 128-pixel tiles of the three
levels per tower stage, and each stage is ONE launch of halo_list_kernel over that list (split 64-cout x 128-pixel tiles on every level) instead of three
full-grid launches whose blocks look their units up in a mask (WTK_SPARSE_LIST=0, the masked form: 256-pixel blocks on P3 / P4).  A pixel's value is one
fixed MFMA chain over chunks x taps whichever block computes it, so everything here is assert_array_equal between the list form, the masked form and
WTK_NO_SPARSE_BOX=1 (dense).

Geometry (csrc/conv3x3_halo.hip: halo_geometry_stacked): a level's map is cut into column strips of <= 85 columns; inside a strip the N images are stacked
with one shared zero row, pitch = S + 1 columns for one strip, S + 2 for more; pixel (n, y, x) has flat index (n (H + 1) + y) pitch + x - strip S, and a
unit is 128 consecutive flat indices of one strip.  At 640 x 640 and at 96 x 160 every level is ONE strip (P3 is 80 resp. 20 columns wide), so the
two-strip case runs on a third shape, 64 x 704 (P3: 8 x 88, two strips of 44), with the batch of 328 at which such a call goes sparse."""
import numpy as np
import pytest
import torch

from test_gpu_sparse_box import SPARSE_CLASS, _frames, _mk, _place, _probe_frames, _rows, _same, _weights
from wtracker_amd import yolo_spec as ys

pytestmark = pytest.mark.gpu

SMALL = ((96, 160), 1024, 961)
BENCH = ((640, 640), 64, 64)
WIDE = ((64, 704), 328, 328)


def _mk_form(monkeypatch, hw, max_batch, form, w=None):
    """form: "list" (the default), "masked" (WTK_SPARSE_LIST=0) or "dense" (WTK_NO_SPARSE_BOX=1); the switches are read when the handle is created"""
    if form == "masked":
        monkeypatch.setenv("WTK_SPARSE_LIST", "0")
    else:
        monkeypatch.delenv("WTK_SPARSE_LIST", raising=False)
    det = _mk(monkeypatch, hw, max_batch, form == "dense", w=w)
    monkeypatch.delenv("WTK_SPARSE_LIST", raising=False)
    return det


def _geom(hw, lvl):
    h, w = hw[0] // (8 << lvl), hw[1] // (8 << lvl)
    strips = -(-w // 85)
    S = -(-w // strips)
    return h, w, S, (S + 1 if strips == 1 else S + 2), strips


def _unit(hw, lvl, n, y, x):
    h, w, S, pitch, _ = _geom(hw, lvl)
    s = x // S
    return lvl, s, ((n * (h + 1) + y) * pitch + x - s * S) >> 7


def _units(hw, anchors):
    """What the select kernel must mark for a batch's survivors: (units of box.0 = the 3 x 3 neighbourhoods inside the map, units of box.1 + box.2)"""
    u0, u1 = set(), set()
    for n, a in enumerate(anchors):
        if a < 0:
            continue
        lvl, y, x, h, w = _place(hw, int(a))
        u1.add(_unit(hw, lvl, n, y, x))
        u0 |= {_unit(hw, lvl, n, yy, xx) for yy in range(max(y - 1, 0), min(y + 2, h)) for xx in range(max(x - 1, 0), min(x + 2, w))}
    return u0, u1


def _launches(det, frames, conf=0.05):
    det.set_profiling(True)
    det.predict_host(frames, conf=conf)
    n = det.get_kernel_profile()[SPARSE_CLASS]["launches"]
    det.set_profiling(False)
    return n


@pytest.mark.parametrize("hw,max_batch,B", [SMALL, BENCH], ids=["96x160-b961of1024", "640x640-b64"])
def test_list_masked_and_dense_give_the_same_bits(hip_lib, monkeypatch, hw, max_batch, B):
    """(a) box.0 and box.2 of the three levels AS THE SPARSE PASS LEFT THEM (raw read: no dense completion) at the survivors' pixels — box.0 on the 3 x 3
    neighbourhood box.1 reads, box.2 on the survivor's pixel — and the rows.  640 x 640 is where P3 / P4 change from 256- to 128-pixel blocks."""
    frames = _frames(hw, B, 1234)
    names = [t["name"] for t in ys.conv_table("s", 1)]
    got = {}
    for form in ("list", "masked", "dense"):
        det = _mk_form(monkeypatch, hw, max_batch, form)
        assert _launches(det, frames) == (0 if form == "dense" else 6)
        rows = _rows(det, frames, 0.05)
        tens = {(lvl, part): det.debug_tensor(names.index(f"model.22.cv2.{lvl}.{part}"), B, raw=True) for lvl in range(3) for part in ("0", "2")}
        got[form] = (rows, tens)
        det.close()
    ref_rows, ref_t = got["dense"]
    assert (ref_rows[2] >= 0).any()
    for form in ("list", "masked"):
        rows, tens = got[form]
        _same(rows, ref_rows, form)
        for n, a in enumerate(ref_rows[2]):
            if a < 0:
                continue
            lvl, y, x, h, w = _place(hw, int(a))
            ys_, xs_ = slice(max(y - 1, 0), min(y + 2, h)), slice(max(x - 1, 0), min(x + 2, w))
            np.testing.assert_array_equal(tens[(lvl, "0")][n, ys_, xs_], ref_t[(lvl, "0")][n, ys_, xs_], err_msg=f"{form} box.0 frame {n} level {lvl}")
            np.testing.assert_array_equal(tens[(lvl, "2")][n, y, x], ref_t[(lvl, "2")][n, y, x], err_msg=f"{form} box.2 frame {n} level {lvl}")


def _scan(dense, hw, B, make, want, batches):
    """frames (from make(seed)) whose dense survivor satisfies want(lvl, y, x, h, w) -> list of (frame, lvl, y, x)"""
    hits = []
    for seed in range(batches):
        f = make(seed)
        an = _rows(dense, f, 0.0)[2]
        for i, a in enumerate(an):
            if a >= 0:
                lvl, y, x, h, w = _place(hw, int(a))
                if want(lvl, y, x, h, w):
                    hits.append((f[i], lvl, y, x))
    return hits


def test_two_survivors_in_one_unit(hip_lib, monkeypatch):
    """(b) duplicates: a last-row survivor of image n and a first-row survivor of image n + 1 on the same level fall into ONE 128-pixel unit of the stacked
    layout (asserted from the anchors the dense handle returns for the very batch), which the list must name once.  On the 640 x 640 handle: the seed-0
    network gives no first-row survivor at 96 x 160 whatever the frame shows (tests/test_gpu_sparse_box.py)."""
    hw, max_batch, B = BENCH
    dense, lst = _mk_form(monkeypatch, hw, max_batch, "dense"), _mk_form(monkeypatch, hw, max_batch, "list")
    hits = _scan(dense, hw, B, lambda s: _probe_frames(hw, B, 5000 + s), lambda lvl, y, x, h, w: y in (0, h - 1), 12)
    fill = _frames(hw, B, 1000)
    batch = None
    for fa, la, ya, xa in hits:  # last row of image n ...
        for fb, lb, yb, xb in hits:  # ... first row of image n + 1
            if la != lb or ya == 0 or yb != 0:
                continue
            for n in range(B - 1):
                if _unit(hw, la, n, ya, xa) == _unit(hw, lb, n + 1, yb, xb):
                    batch = fill.copy()
                    batch[n], batch[n + 1] = fa, fb
                    break
            if batch is not None:
                break
        if batch is not None:
            break
    assert batch is not None, f"no last-row / first-row pair on one level among {len(hits)} border survivors"
    ref = _rows(dense, batch, 0.0)
    _, u1 = _units(hw, ref[2])
    assert len(u1) < int((ref[2] >= 0).sum()), "the batch holds no two survivors in one unit"
    _same(_rows(lst, batch, 0.0), ref, "shared unit")
    c0, c1, g0, g1 = lst.sparse_counts()
    u0, u1 = _units(hw, ref[2])
    assert (c0, c1) == (len(u0), len(u1)) and c0 <= g0 and c1 <= g1  # every marked unit listed once
    dense.close(), lst.close()


def test_neighbourhood_over_two_units_and_two_strips(hip_lib, monkeypatch):
    """(b) neighbours: a survivor on P3 of the 64 x 704 input next to the border between its two column strips (x = 43 or 44 of 88), whose 3 x 3
    neighbourhood therefore lies in two strips and, three rows of pitch 46 apart, in more than one unit of each.  Frames: a blob next to the border column."""
    hw, max_batch, B = WIDE
    assert _geom(hw, 0)[2:] == (44, 46, 2) and all(_geom(hw, lvl)[4] == 1 for lvl in (1, 2))
    assert all(_geom(s[0], lvl)[4] == 1 for s in (SMALL, BENCH) for lvl in range(3))  # why this shape: the other two have one strip on every level
    w0 = _weights(0, 0)  # class bias pulls the survivors onto P3
    dense, lst = _mk_form(monkeypatch, hw, max_batch, "dense", w=w0), _mk_form(monkeypatch, hw, max_batch, "list", w=w0)

    def make(seed):
        rng = np.random.default_rng(7000 + seed)
        out = np.empty((B, hw[0], hw[1]), dtype=np.uint8)
        for i in range(B):
            dark = bool(rng.integers(0, 2))
            img = np.full(hw, int(rng.integers(120, 256) if dark else rng.integers(0, 100)), dtype=np.int32) + rng.integers(-10, 11, size=hw)
            cy, cx, ry, rx = int(rng.integers(0, hw[0])), 352 + int(rng.integers(-28, 29)), int(rng.integers(2, 14)), int(rng.integers(2, 14))
            img[max(cy - ry, 0) : cy + ry + 1, cx - rx : cx + rx + 1] = int(rng.integers(0, 100) if dark else rng.integers(120, 256))
            out[i] = np.clip(img, 0, 255).astype(np.uint8)
        return out

    hits = _scan(dense, hw, B, make, lambda lvl, y, x, h, w: lvl == 0 and x in (43, 44), 4)
    assert hits, "no P3 survivor next to the strip border"
    batch = make(99)
    for i, (f, _, _, _) in enumerate(hits[:B]):
        batch[(i * 7) % B] = f
    ref = _rows(dense, batch, 0.0)
    spans = []
    for n, a in enumerate(ref[2]):
        lvl, y, x, h, w = _place(hw, int(a))
        u0, _ = _units(hw, [-1] * n + [a])
        spans.append((len({u[1] for u in u0}), len(u0)))
    assert any(s == 2 and u > 2 for s, u in spans), "no neighbourhood over two strips and more than one unit per strip"
    assert _launches(lst, batch, 0.0) == 6
    _same(_rows(lst, batch, 0.0), ref, "two strips")
    c0, c1, g0, g1 = lst.sparse_counts()
    u0, u1 = _units(hw, ref[2])
    assert (c0, c1) == (len(u0), len(u1)) and c0 <= g0 and c1 <= g1
    dense.close(), lst.close()


def test_live_counts_stay_inside_the_grids(hip_lib, monkeypatch):
    """(c) the device-side counts of listed tiles against the grids the host launched: a count above its grid would mean tiles nobody ran.  Full batch and a
    dynamic-batch call (n_dyn < B: frames beyond it list nothing).  The counts are also the sizes of the unit sets the survivors imply."""
    hw, max_batch, B = SMALL
    dense, lst = _mk_form(monkeypatch, hw, max_batch, "dense"), _mk_form(monkeypatch, hw, max_batch, "list")
    frames = _frames(hw, B, 1000)
    ref = _rows(dense, frames, 0.0)
    _same(_rows(lst, frames, 0.0), ref)
    c0, c1, g0, g1 = lst.sparse_counts()
    print(f"{hw} B={B}: listed {c0} / {c1} tiles, grids {g0} / {g1}")
    assert 0 < c0 <= g0 and 0 < c1 <= g1
    u0, u1 = _units(hw, ref[2])
    assert (c0, c1) == (len(u0), len(u1))
    n_dyn = 23
    dev = torch.from_numpy(frames).cuda()
    n_dev = torch.tensor([n_dyn], dtype=torch.int32, device="cuda")
    outs = []
    for det in (dense, lst):
        det.set_dynamic_batch(n_dev)
        o = (torch.zeros((B, 4), device="cuda"), torch.zeros((B,), device="cuda"), torch.zeros((B,), dtype=torch.int32, device="cuda"))
        det.predict(dev, B, hw[0], hw[1], 1, *o, conf=0.0)
        torch.cuda.synchronize()
        outs.append([t.cpu().numpy()[:n_dyn] for t in o])
        det.set_dynamic_batch(None)
    for x, y in zip(*outs):
        np.testing.assert_array_equal(x, y)
    d0, d1, g0, g1 = lst.sparse_counts()
    u0, u1 = _units(hw, list(outs[0][2]))
    print(f"{hw} n_dyn={n_dyn} of {B}: listed {d0} / {d1} tiles, grids {g0} / {g1}")
    assert 0 < d0 <= g0 and 0 < d1 <= g1 and (d0, d1) == (len(u0), len(u1)) and d1 <= n_dyn
    dense.close(), lst.close()


def test_calls_in_a_row_without_a_mask_clear(hip_lib, monkeypatch):
    """(d) the list form has no memset between calls: the decode kernel leaves mask and counters zero.  Two calls whose survivors sit on other levels, then
    a call that keeps nothing (conf above every score: no tile listed, every row NaN), then a call with survivors again."""
    hw, max_batch, B = SMALL
    dense, lst = _mk_form(monkeypatch, hw, max_batch, "dense"), _mk_form(monkeypatch, hw, max_batch, "list")
    fa, fb = _frames(hw, B, 1000), _probe_frames(hw, B, 5003)
    ra, rb = _rows(dense, fa, 0.0), _rows(dense, fb, 0.0)
    la, lb = [_place(hw, int(a))[0] for a in ra[2]], [_place(hw, int(a))[0] for a in rb[2]]
    assert sum(x != y for x, y in zip(la, lb)) > 0, "no frame index whose survivor changes level between the two calls"
    _same(_rows(lst, fa, 0.0), ra, "first call")
    _same(_rows(lst, fb, 0.0), rb, "second call")
    u0, u1 = _units(hw, rb[2])
    assert lst.sparse_counts()[:2] == (len(u0), len(u1))  # nothing of the first call's units in the second call's lists
    none = _rows(lst, fb, 2.0)
    _same(none, _rows(dense, fb, 2.0), "no survivor")
    assert np.isnan(none[0]).all() and (none[2] == -1).all() and lst.sparse_counts()[:2] == (0, 0)
    _same(_rows(lst, fa, 0.0), ra, "after the empty call")
    dense.close(), lst.close()
