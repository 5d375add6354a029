"""Sparse Detect box towers (DESIGN.md "Sparse box towers"): on max_det = 1 calls a throughput-plan f16x3 handle runs the box towers
(model.22.cv2.*) only on the window-kernel tiles under each frame's surviving anchor.  Per-pixel arithmetic is the dense launches' — same
kernel instantiation, same packed weights, same K order — so every output row must keep its BITS: everything here is assert_array_equal
against a handle created with WTK_NO_SPARSE_BOX=1 (NaN rows compare equal as NaN).

Which calls go sparse (csrc/wtk_run.hip: resolve_sparse): f16x3, throughput plan, every box op on the window kernel with the fused 1x1 tail, and a
call of at least four rounds of P3 blocks over the 256 CUs (B x (H/8 + 1) x (W/8 + 1) >= 262 144: below that the six dependent sparse launches cost more
than the skipped tiles save — measured, profiles/r07_notes.md section 6).  fp16 and fp32 handles stay DENSE (they run the shared first conv of a tower
pair as one 192-cout tile, whose halves would be other instantiations) and so do latency-plan handles; test_dense_modes_stay_dense names them and
asserts it.  Four shapes of the list below are therefore DENSE at the batch the list gives them (named and asserted as such, rows still compared), and
run once more at a batch that is large enough, where the same maps (down to the 1 x 1 map of 32 x 32) go through the sparse launches.  With the fused tail, box.1's own
output is never materialised (dense or sparse), so the dense-on-demand check compares box.0 (the shared conv's tensor) and box.2 (the logits)."""
import numpy as np
import pytest
import torch

from wtracker_amd import frames as fr
from wtracker_amd import hip
from wtracker_amd import yolo_spec as ys
from wtracker_amd.hybrid import HybridDetector

pytestmark = pytest.mark.gpu

SPARSE_CLASS = "conv3x3_halo_kernel(sparse box towers)"
# (H, W) of the network input, max_batch of the handle, batch of the calls, whether such a call goes sparse
CONFIGS = [((640, 640), 64, 64, True), ((640, 512), 40, 33, False), ((384, 384), 16, 15, False), ((96, 160), 3, 3, False), ((32, 32), 1, 1, False),
           ((640, 512), 64, 50, True), ((384, 384), 128, 110, True), ((96, 160), 1024, 961, True), ((32, 32), 10486, 10486, True)]
IDS = ["640x640-b64", "640x512-b33of40-dense", "384x384-b15of16-dense", "96x160-b3-dense", "32x32-b1-dense", "640x512-b50of64", "384x384-b110of128",
       "96x160-b961of1024", "32x32-b10486"]


def _weights(seed=0, force_level=None):
    """Synthetic YOLOv8s weights; force_level: +12 on the class logit bias of that Detect level (the levels' biases lie 1.4 apart, the logits' spread is of
    order one), so every frame's survivor lies on that level's map while its score stays well inside fp32's resolution below 1."""
    w = dict(ys.synthetic_weights("s", 1, seed=seed))
    if force_level is not None:
        nm = f"model.22.cv3.{force_level}.2"
        w[nm] = (w[nm][0], w[nm][1] + np.float32(12.0))
    return w


BORDER = {"first-row", "last-row", "side-border", "corner"}
LEVELS = {"level0", "level1", "level2"}


def _mk(monkeypatch, hw, max_batch, dense, dtype="f16x3", plan="auto", w=None):
    w = w if w is not None else _weights()
    depth, width, maxch = ys.SCALES["s"]
    if dense:
        monkeypatch.setenv("WTK_NO_SPARSE_BOX", "1")  # read once, when the handle is created
    else:
        monkeypatch.delenv("WTK_NO_SPARSE_BOX", raising=False)
    det = hip.HipYolo(w, hw, max_batch, dtype=dtype, nc=1, width=width, depth=depth, max_channels=maxch, plan=plan)
    monkeypatch.delenv("WTK_NO_SPARSE_BOX", raising=False)
    return det


def _rows(det, frames, conf):
    xywh, cf, an = det.predict_host(frames, conf=conf)
    return xywh, cf, an, det.last_margins(len(frames))


def _same(a, b, what=""):
    for x, y, nm in zip(a, b, ("xywh", "conf", "anchor", "margin")):
        np.testing.assert_array_equal(x, y, err_msg=f"{what} {nm}")  # (NaN == NaN here)


def _runs_sparse(det, frames, conf=0.05):
    """True iff a max_det = 1 call of `det` launches sparse box towers (profile class 7 counts them; profiling does not change results)."""
    det.set_profiling(True)
    det.predict_host(frames, conf=conf)
    n = det.get_kernel_profile()[SPARSE_CLASS]["launches"]
    det.set_profiling(False)
    assert n in (0, 6), n  # box.0 and box.1 + box.2 of the three levels
    return n == 6


def _frames(hw, n, seed):
    """n frames for a handle of input hw: worm frames where the generator has room (letterboxed by the library when hw is not square), noise otherwise."""
    size = max(hw)
    if size >= 96:
        return fr.diverse_frames(n, size, seed=seed)
    return np.random.default_rng(seed).integers(0, 256, size=(n, hw[0], hw[1]), dtype=np.uint8)


def _probe_frames(hw, n, seed):
    """Frames that pull survivors towards chosen places: a flat or noisy background of either polarity with one blob at a corner, on an edge or
    inside (random-weight networks respond where the picture changes), and plain noise."""
    rng = np.random.default_rng(seed)
    H, W = hw
    out = np.empty((n, H, W), dtype=np.uint8)
    for i in range(n):
        kind = rng.integers(0, 6)
        if kind == 0:
            out[i] = rng.integers(0, 256, size=(H, W), dtype=np.uint8)
            continue
        lo, hi = (0, 100), (120, 256)
        if kind % 2:
            lo, hi = hi, lo  # bright blob on a dark background
        img = np.full((H, W), int(rng.integers(*hi)), dtype=np.int32)
        if kind >= 4:
            img = img + rng.integers(-20, 21, size=(H, W))
        ry, rx = int(rng.integers(1, max(2, H // 3))), int(rng.integers(1, max(2, W // 3)))
        cy = int(rng.choice([0, H - 1, rng.integers(0, H)], p=[0.4, 0.4, 0.2]))
        cx = int(rng.choice([0, W - 1, rng.integers(0, W)], p=[0.4, 0.4, 0.2]))
        img[max(cy - ry, 0) : cy + ry + 1, max(cx - rx, 0) : cx + rx + 1] = int(rng.integers(*lo))
        out[i] = np.clip(img, 0, 255).astype(np.uint8)
    return out


def _place(hw, anchor):
    """anchor index -> (level, y, x, h, w) on that level's map"""
    a0 = 0
    for lvl, s in enumerate((8, 16, 32)):
        h, w = hw[0] // s, hw[1] // s
        if anchor < a0 + h * w:
            j = anchor - a0
            return lvl, j // w, j % w, h, w
        a0 += h * w
    raise AssertionError(anchor)


def _border_batch(dense, hw, B, max_frames=6000):
    """Scan seeds on the DENSE handle for frames whose survivor sits on a border / in a corner / in the first or last row of its level's map, and on each
    level; returns a batch of B such frames (padded with other scanned frames) and the set of categories it holds."""
    picked, cats, spare = [], set(), []
    for seed in range((max_frames + B - 1) // B):
        f = _probe_frames(hw, B, 5000 + seed)
        _, _, an, _ = _rows(dense, f, 0.0)
        for i, a in enumerate(an):
            if a < 0:
                continue
            lvl, y, x, h, w = _place(hw, int(a))
            c = {f"level{lvl}"}
            if y == 0:
                c.add("first-row")
            if y == h - 1:
                c.add("last-row")
            if x == 0 or x == w - 1:
                c.add("side-border")
            if y in (0, h - 1) and x in (0, w - 1):
                c.add("corner")
            if c - cats and len(picked) < B:
                picked.append(f[i])
                cats |= c
            elif len(spare) < B:
                spare.append(f[i])
        if len(cats) == 7:
            break
    batch = np.stack((picked + spare)[:B])
    return batch, cats


@pytest.mark.parametrize("hw,max_batch,B,goes_sparse", CONFIGS, ids=IDS)
def test_rows_keep_their_bits(hip_lib, monkeypatch, hw, max_batch, B, goes_sparse):
    dense, sparse = _mk(monkeypatch, hw, max_batch, True), _mk(monkeypatch, hw, max_batch, False)
    frames = _frames(hw, B, 1000)
    assert _runs_sparse(sparse, frames) == goes_sparse and not _runs_sparse(dense, frames)
    # diverse frames, every frame kept
    ref = _rows(dense, frames, 0.0)
    _same(_rows(sparse, frames, 0.0), ref, "diverse")
    assert (ref[2] >= 0).all()
    # frames without a detection in one batch with frames that have one: a threshold between the batch's scores (B = 1: one call each side of the score)
    scores = np.sort(ref[1])
    for thr in ([float(scores[0]) * 0.5, 0.5 * (float(scores[0]) + 1.0)] if B == 1 else [0.5 * float(scores[(B - 1) // 2] + scores[(B - 1) // 2 + 1])]):
        r = _rows(dense, frames, thr)
        _same(_rows(sparse, frames, thr), r, f"conf {thr}")
        if B > 1 and scores[0] != scores[-1]:
            assert (r[2] < 0).any() and (r[2] >= 0).any() and np.isnan(r[0][r[2] < 0]).all()
    if B == 1:
        assert _rows(dense, frames, 0.5 * (float(scores[0]) + 1.0))[2][0] == -1
    # survivors on borders, in corners, in the first and last row of an image (next to the shared zero row of the stacked layout), on every level
    batch, cats = _border_batch(dense, hw, B)
    print(f"{hw} B={B}: border batch holds {sorted(cats)}")
    # What the scan must find.  The shapes of 384 pixels and more: every category (corner, first and last row, side border, each of the
    # three levels).  The two tiny shapes (at either batch): the survivors of the seed-0 network do not reach every place there whatever the frame shows — on an MI355X,
    # 6 000 probe frames at 96 x 160 (B = 3) gave last-row and side-border survivors on levels 0 and 1 only, never a first-row or corner one; the single
    # frame at 32 x 32 gave a first-row corner on level 1 — so there this test asks for a border survivor, and
    # test_tiny_maps_every_place_on_the_sparse_path covers every category on every level of those maps with other weights, on calls that go sparse.
    if min(hw) >= 384:
        assert BORDER | LEVELS <= cats, (sorted(cats), "scanning found no survivor in: " + str(sorted((BORDER | LEVELS) - cats)))
    else:
        assert BORDER & cats, sorted(cats)
    _same(_rows(sparse, batch, 0.0), _rows(dense, batch, 0.0), "border batch")
    dense.close(), sparse.close()


@pytest.mark.parametrize("hw,max_batch,B", [((96, 160), 1024, 961), ((32, 32), 10486, 10486)], ids=["96x160-b961of1024", "32x32-b10486"])
def test_tiny_maps_every_place_on_the_sparse_path(hip_lib, monkeypatch, hw, max_batch, B):
    """The small maps (32 x 32: P5 is 1 x 1, every neighbour is padding; P4 2 x 2, all corners) at a batch large enough to go sparse.  Where a random-weight
    network's survivors sit on such maps is decided by its weights far more than by the frame, so the scan runs over weight seeds and, per seed, over
    networks whose class bias forces the survivor onto one level: every (weights, level) pair is a dense / sparse handle pair whose border batch must keep
    its bits, and TOGETHER the compared batches must hold every category — corner, first row, last row, side border — on each of the three levels."""
    found = {lvl: set() for lvl in range(3)}
    for seed in range(6):
        for lvl in range(3):
            if BORDER <= found[lvl]:
                continue
            w = _weights(seed, lvl)
            dense, sparse = _mk(monkeypatch, hw, max_batch, True, w=w), _mk(monkeypatch, hw, max_batch, False, w=w)
            batch, _ = _border_batch(dense, hw, B, max_frames=3 * B)
            ref = _rows(dense, batch, 0.0)
            assert _runs_sparse(sparse, batch) and not _runs_sparse(dense, batch)
            _same(_rows(sparse, batch, 0.0), ref, f"weights {seed} level {lvl}")
            for a in ref[2]:  # every row of the batch was compared: count each under the level its survivor is really on (the bias pulls, it does not bind)
                al, y, x, h, w = _place(hw, int(a))
                found[al] |= ({"first-row"} if y == 0 else set()) | ({"last-row"} if y == h - 1 else set()) | ({"side-border"} if x in (0, w - 1) else set()) | (
                    {"corner"} if y in (0, h - 1) and x in (0, w - 1) else set())
            dense.close(), sparse.close()
        if all(BORDER <= f for f in found.values()):
            break
    print(f"{hw} B={B}: compared border categories per level {[sorted(f) for f in found.values()]}")
    for lvl in range(3):
        assert BORDER <= found[lvl], (lvl, "no compared survivor in: " + str(sorted(BORDER - found[lvl])))


def test_nothing_stale_leaks_between_calls(hip_lib, monkeypatch):
    hw = (640, 640)
    dense, sparse = _mk(monkeypatch, hw, 64, True), _mk(monkeypatch, hw, 64, False)
    for seed, B in ((1000, 64), (2000, 64), (3000, 5), (4000, 64), (4000, 64)):
        frames = _frames(hw, B, seed)
        _same(_rows(sparse, frames, 0.05), _rows(dense, frames, 0.05), f"seed {seed} B {B}")
    dense.close(), sparse.close()


@pytest.mark.parametrize("hw,max_batch,B,goes_sparse", [CONFIGS[0], CONFIGS[7]], ids=[IDS[0], IDS[7]])
def test_dense_on_demand(hip_lib, monkeypatch, hw, max_batch, B, goes_sparse):
    dense, sparse = _mk(monkeypatch, hw, max_batch, True), _mk(monkeypatch, hw, max_batch, False)
    frames = _frames(hw, B, 1234)
    ref = _rows(dense, frames, 0.05)
    _same(_rows(sparse, frames, 0.05), ref)
    box_d, cls_d = dense.debug_head(B)
    box_s, cls_s = sparse.debug_head(B)
    np.testing.assert_array_equal(cls_s, cls_d)
    np.testing.assert_array_equal(box_s, box_d)  # all anchors, not the survivors alone
    names = [t["name"] for t in ys.conv_table("s", 1)]
    frames2 = _frames(hw, B, 4321)
    ref2 = _rows(dense, frames2, 0.05)
    _same(_rows(sparse, frames2, 0.05), ref2)  # a sparse call after the dense completion still matches ...
    for lvl in range(3):  # ... and the box-tower tensors are completed again on demand: box.0 (the shared first conv's tensor, class half included), box.2
        for part in ("0", "2"):
            i = names.index(f"model.22.cv2.{lvl}.{part}")
            np.testing.assert_array_equal(sparse.debug_tensor(i, B), dense.debug_tensor(i, B), err_msg=names[i])
    _same(_rows(sparse, frames, 0.05), ref)
    dense.close(), sparse.close()


def test_composes_with_dynamic_batch_and_nms(hip_lib, monkeypatch):
    hw, B = (640, 640), 64
    dense, sparse = _mk(monkeypatch, hw, B, True), _mk(monkeypatch, hw, B, False)
    frames = torch.from_numpy(_frames(hw, B, 777)).cuda()
    n_dev = torch.tensor([23], dtype=torch.int32, device="cuda")
    outs = []
    for det in (dense, sparse):
        det.set_dynamic_batch(n_dev)
        o = (torch.zeros((B, 4), device="cuda"), torch.zeros((B,), device="cuda"), torch.zeros((B,), dtype=torch.int32, device="cuda"))
        det.predict(frames, B, hw[0], hw[1], 1, *o, conf=0.05)
        torch.cuda.synchronize()
        outs.append([t.cpu().numpy()[:23] for t in o])  # the rows that matter
        det.set_dynamic_batch(None)
    for x, y in zip(*outs):
        np.testing.assert_array_equal(x, y)
    # max_det = 3 on the same handles: every box is needed, the call is dense and unchanged
    res = []
    for det in (dense, sparse):
        o = (torch.zeros((B, 3, 4), device="cuda"), torch.zeros((B, 3), device="cuda"), torch.zeros((B, 3), dtype=torch.int32, device="cuda"),
             torch.zeros((B, 3), dtype=torch.int32, device="cuda"), torch.zeros((B,), dtype=torch.int32, device="cuda"))
        det.predict_nms(frames, B, hw[0], hw[1], 1, 3, *o, conf=0.05)
        torch.cuda.synchronize()
        res.append([t.cpu().numpy() for t in o])
        box, _ = det.debug_head(B)  # complete after an NMS call without any completion pass
        res[-1].append(box)
    for x, y in zip(*res):
        np.testing.assert_array_equal(x, y)
    dense.close(), sparse.close()


@pytest.mark.parametrize("defer", [1, 2], ids=["immediate", "deferred"])
def test_hybrid_rows_unchanged(hip_lib, monkeypatch, defer):
    hw, B = (640, 640), 64
    frames = torch.from_numpy(_frames(hw, B, 999)).cuda()
    rows = []
    for dense in (True, False):
        hyb = HybridDetector(_mk(monkeypatch, hw, B, dense, dtype="fp16"), _mk(monkeypatch, hw, B * defer, dense), margin=0.5, defer=defer)
        o = (torch.zeros((B, 4), device="cuda"), torch.zeros((B,), device="cuda"), torch.zeros((B,), dtype=torch.int32, device="cuda"))
        for _ in range(defer):
            hyb.predict(frames, B, hw[0], hw[1], 1, *o, conf=0.05)
        hyb.flush()
        torch.cuda.synchronize()
        assert hyb.overflow_count() == 0 and hyb.pending == 0 and int(hyb.replaced.item()) > 0
        rows.append([t.cpu().numpy() for t in o] + [int(hyb.replaced.item())])
        hyb.close()
    for x, y in zip(*rows):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("dtype,plan,max_batch", [("fp16", "throughput", 17), ("fp32", "throughput", 17), ("f16x3", "latency", 17), ("fp32", "latency", 17),
                                                  ("f16x3", "throughput", 16), ("f16x3", "throughput", 3)])
def test_dense_modes_stay_dense(hip_lib, monkeypatch, dtype, plan, max_batch):
    """The modes that do NOT go sparse, by name: fp16 / fp32 (192-cout tile of the shared conv), the latency plan (grouped split-K launches) and f16x3
    throughput-plan handles whose calls are too small for the sparse tail to pay."""
    hw, B = (96, 160), 3
    det = _mk(monkeypatch, hw, max_batch, False, dtype=dtype, plan=plan)
    frames = _frames(hw, B, 5)
    assert det.plan == plan and not _runs_sparse(det, frames)
    det.close()
