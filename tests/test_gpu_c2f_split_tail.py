"""model.2.cv2 in the epilogue of model.2.m.0.cv2 on f16x3 throughput-plan handles above 16 frames (DESIGN.md "C2f tail of the split thin-layer kernel";
csrc/conv3x3_c32.hip: conv3x3_c32_split_kernel_cv2).  The fused kernel forms z = SiLU(conv) + y1 in registers and multiplies [y0 | y1 | z] by the 1x1's packed
weights with the arithmetic and the K order of the split implicit GEMM, so it must keep the BITS of the two launches it replaces: everything here is
assert_array_equal between a fused handle and a handle of the same weights created with WTK_NO_C2F_SPLIT_TAIL=1 (hip.HipYolo asks for the fusion in its create call) — the model.2.cv2 tensor, z (which the fused
pass never stores: the debug read runs the unfused launch on demand), the head logits and the rows.

Shapes: the smallest at which the kernel can go wrong.  A tile is 256 flat outputs of one image's column strip (strips of <= 45 columns, pitch = strip + 2):
32 x 32 (8 x 8 map: one partial tile per image, most of it junk positions), 96 x 160 (24 x 40: non-square, three tiles per image, the last partial),
64 x 704 (16 x 176: four strips of 44 columns), 640 x 640 at B = 18 (160 x 160, four strips, 29 tiles per strip; with a device-side batch of 5 and of 0)."""
import numpy as np
import pytest
import torch

from wtracker_amd import frames as fr
from wtracker_amd import hip
from wtracker_amd import yolo_spec as ys

pytestmark = pytest.mark.gpu

NAMES = [t["name"] for t in ys.conv_table("s", 1)]
CV2, Z = NAMES.index("model.2.cv2"), NAMES.index("model.2.m.0.cv2")
C32_CLASS, IGEMM_CLASS = "conv3x3_c32_kernel", "conv_igemm_kernel+conv1x1_wide_kernel"


def _pair(monkeypatch, hw, max_batch):
    """(fused handle, two-launch handle) of the same synthetic weights; the switch is read when a handle is created"""
    w = ys.synthetic_weights("s", 1, seed=0)
    depth, width, maxch = ys.SCALES["s"]
    out = []
    for unfused in (False, True):
        if unfused:
            monkeypatch.setenv("WTK_NO_C2F_SPLIT_TAIL", "1")
        else:
            monkeypatch.delenv("WTK_NO_C2F_SPLIT_TAIL", raising=False)
        out.append(hip.HipYolo(w, hw, max_batch, dtype="f16x3", nc=1, width=width, depth=depth, max_channels=maxch, plan="throughput"))
    monkeypatch.delenv("WTK_NO_C2F_SPLIT_TAIL", raising=False)
    return out


def _noise(B, hw, seed, channels=None):
    shape = (B, hw[0], hw[1]) if channels is None else (B, hw[0], hw[1], channels)
    return np.random.default_rng(seed).integers(0, 256, size=shape, dtype=np.uint8)


def _launches(det, frames):
    det.set_profiling(True)
    det.predict_host(frames, conf=0.05)
    prof, kern = det.get_profile(), det.get_kernel_profile()
    det.set_profiling(False)
    return prof, kern


def _same_call(fused, plain, frames, what):
    """one call of both handles on `frames`: rows, head logits, model.2.cv2 and z; before it, the proof that the fusion applied to this pair at this
    shape and batch (the fused handle's pass has one conv launch fewer), without which equal tensors would say nothing"""
    B = len(frames)
    assert _launches(fused, frames)[0]["conv"]["launches"] == _launches(plain, frames)[0]["conv"]["launches"] - 1, f"{what}: the pair did not run fused"
    got = []
    for det in (fused, plain):
        rows = det.predict_host(frames, conf=0.05)
        got.append((rows, det.last_margins(B), det.debug_head(B), det.debug_tensor(CV2, B), det.debug_tensor(Z, B)))
        assert det.status() == 0
    (rf, mf, hf, cf, zf), (rp, mp, hp, cp, zp) = got
    assert np.isfinite(cp).all() and np.abs(cp).max() > 0 and np.abs(zp).max() > 0
    np.testing.assert_array_equal(cf, cp, err_msg=f"{what}: model.2.cv2")
    np.testing.assert_array_equal(zf, zp, err_msg=f"{what}: z on demand")
    for x, y, nm in zip(hf, hp, ("box logits", "class logits")):
        np.testing.assert_array_equal(x, y, err_msg=f"{what}: {nm}")
    for x, y, nm in zip(rf + (mf,), rp + (mp,), ("xywh", "conf", "anchor", "margin")):
        np.testing.assert_array_equal(x, y, err_msg=f"{what}: {nm}")  # (NaN == NaN here)


@pytest.mark.parametrize("hw", [(32, 32), (96, 160), (64, 704)], ids=["32x32", "96x160", "64x704"])
def test_fused_tail_keeps_the_bits(hip_lib, monkeypatch, hw):
    """B = 17 (the smallest handle the fusion applies to), two calls in a row with different frames: nothing is carried from tile to tile or call to call."""
    fused, plain = _pair(monkeypatch, hw, 17)
    assert fused.plan == plain.plan == "throughput" and fused.macs_per_frame == plain.macs_per_frame
    _same_call(fused, plain, _noise(17, hw, 1), "first call")
    _same_call(fused, plain, _noise(17, hw, 2), "second call")
    _same_call(fused, plain, _noise(5, hw, 3), "a call smaller than the handle")
    fused.close(), plain.close()


@pytest.mark.parametrize("channels", [3, None], ids=["bgr", "gray"])
def test_both_input_forms(hip_lib, monkeypatch, channels):
    """the fused front that feeds the pair, from BGR and from gray frames, 64 x 64"""
    fused, plain = _pair(monkeypatch, (64, 64), 17)
    _same_call(fused, plain, _noise(17, (64, 64), 4, channels), "bgr" if channels else "gray")
    fused.close(), plain.close()


def test_dynamic_batch_at_640(hip_lib, monkeypatch):
    """640 x 640, B = 18: a full call, then the same batch size with a device-side count of 5 (tiles beyond it are skipped) and of 0 (an empty call)."""
    hw, B = (640, 640), 18
    fused, plain = _pair(monkeypatch, hw, B)
    _same_call(fused, plain, fr.diverse_frames(B, 640, seed=11), "full call")
    dev = torch.from_numpy(fr.diverse_frames(B, 640, seed=12)).cuda()
    for n_dyn in (5, 0):
        n_dev = torch.tensor([n_dyn], dtype=torch.int32, device="cuda")
        outs = []
        for det in (fused, plain):
            det.set_dynamic_batch(n_dev)
            o = (torch.zeros((B, 4), device="cuda"), torch.zeros((B,), device="cuda"), torch.zeros((B,), dtype=torch.int32, device="cuda"))
            det.predict(dev, B, hw[0], hw[1], 1, *o, conf=0.05)
            torch.cuda.synchronize()
            det.set_dynamic_batch(None)
            live = slice(0, n_dyn)  # (n_dyn = 0: empty, the tensor comparisons compare nothing; the rows are compared whole)
            rows = slice(0, n_dyn) if n_dyn else slice(None)  # the empty call: every row as the call left it (both handles have the same history)
            outs.append([t.cpu().numpy()[rows] for t in o] + [det.debug_tensor(CV2, B)[live], det.debug_tensor(Z, B)[live], det.debug_head(B)[1][live]])
            assert det.status() == 0
        for x, y, nm in zip(*outs, ("xywh", "conf", "anchor", "model.2.cv2", "z", "class logits")):
            np.testing.assert_array_equal(x, y, err_msg=f"n_dyn = {n_dyn}: {nm}")
        if n_dyn:
            assert np.abs(outs[1][3]).max() > 0
    fused.close(), plain.close()


def test_one_launch_where_there_were_two(hip_lib, monkeypatch):
    """The profile: one conv launch fewer, out of the implicit-GEMM class; the thin-layer class keeps its two launches and gains the 1x1's FLOP credit, so
    the total is what it was.  Handles of at most 16 frames keep both launches."""
    hw = (96, 160)
    fused, plain = _pair(monkeypatch, hw, 17)
    frames = _noise(17, hw, 5)
    (pf, kf), (pp, kp) = _launches(fused, frames), _launches(plain, frames)
    assert pf["conv"]["launches"] == pp["conv"]["launches"] - 1
    assert kf[IGEMM_CLASS]["launches"] == kp[IGEMM_CLASS]["launches"] - 1 and kf[C32_CLASS]["launches"] == kp[C32_CLASS]["launches"] == 2
    cv2_flops = 2.0 * 17 * (hw[0] // 4) * (hw[1] // 4) * 96 * 64
    assert kf[C32_CLASS]["flops"] == kp[C32_CLASS]["flops"] + cv2_flops and kf[IGEMM_CLASS]["flops"] == kp[IGEMM_CLASS]["flops"] - cv2_flops
    assert sum(k["flops"] for k in kf.values()) == sum(k["flops"] for k in kp.values())
    fused.close(), plain.close()
    small_a, small_b = _pair(monkeypatch, hw, 16)
    (pa, _), (pb, _) = _launches(small_a, frames[:16]), _launches(small_b, frames[:16])
    assert pa["conv"]["launches"] == pb["conv"]["launches"]
    small_a.close(), small_b.close()
