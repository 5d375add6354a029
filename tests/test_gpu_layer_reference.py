"""Every conv kernel, layer by layer, against float64 arithmetic the library does not share (tests/harness/layer_ref.py).

Each configuration runs one forward pass on seeded synthetic weights and distinct frames in every batch row, then checks every conv blob from
the GPU's own input tensors: a per-element forward-error bound of the handle's dtype and a per-layer rms ceiling (derivation: the docstring of
layer_ref.py, calibrated by tests/test_layer_ref.py).  Blobs a plan keeps on chip are listed per configuration (layer_ref.unobservable_blobs)
and checked as composites through their consumers.  At large batches a subset of the rows is checked (first, second, both sides of a 32-row
boundary, last), which keeps the float64 reference within minutes."""
import os

import numpy as np
import pytest

from harness import layer_ref as lr
from wtracker_amd import frames as fr
from wtracker_amd import hip
from wtracker_amd import yolo_spec as ys

pytestmark = pytest.mark.gpu

# tests/conftest.py keeps small handles on the throughput kernels; product-default configurations remove these
SUITE_ONLY = ("WTK_LATENCY_PLAN", "WTK_NO_SK_MIXED", "WTK_SMALL_NARROW")
NO_FUSION = {"WTK_NO_FUSED_FRONT": "1", "WTK_NO_FUSED_C2F": "1", "WTK_NO_FUSED_TAIL": "1", "WTK_NO_IGEMM_TAIL": "1"}


def _frames(B, H, W, seed):
    if H == W:
        return fr.diverse_frames(B, H, seed=seed)
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, size=(B, H, W, 3) if seed % 2 else (B, H, W), dtype=np.uint8)  # gray and BGR frames


def _family(scale, nc):
    geo = {t["name"]: t for t in ys.conv_table(scale, nc)}

    def fam(name):
        t = geo[name]
        return "stem" if name == "model.0" else f"{t['k']}x{t['k']}/s{t['stride']}"
    return fam


HALO, IGEMM, FUSED, C32 = "conv3x3_halo_kernel", "conv_igemm_kernel+conv1x1_wide_kernel", "front_fused_kernel+c2f32_fused_kernel", "conv3x3_c32_kernel"


def _kernel_profile(det, frames, label):
    """One more, profiled pass after the checked one (profiling runs a pass on one stream: the checked pass stays the product's) -> launches per
    kernel class.  The classes are per source file: they tell the window kernels from the implicit GEMM, not a kernel's forms from each other."""
    det.set_profiling(True)
    det.predict_host(frames, conf=0.1)
    kp = det.get_kernel_profile()
    det.set_profiling(False)
    print(f"[kernel profile] {label}\n" + "\n".join(f"  {k:<42} launches {v['launches']:>4}  {v['total_ms']:8.3f} ms  {v['flops'] / 1e9:10.3f} GFLOP"
                                                     for k, v in kp.items()))
    return {k: v["launches"] for k, v in kp.items()}


def _check(monkeypatch, H, W, B, max_batch, dtype, plan="throughput", env=None, product=False, scale="s", nc=1, rows=None, weights=None, seed=0,
           wide_scale=False):
    if product:
        for k in SUITE_ONLY:
            monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    depth, width, maxch = ys.SCALES[scale]
    w = weights if weights is not None else ys.synthetic_weights(scale, nc, seed=seed)
    frames = _frames(B, H, W, 100 + H + 7 * W + B)
    det = hip.HipYolo(w, (H, W), max_batch, dtype=dtype, nc=nc, width=width, depth=depth, max_channels=maxch, plan=plan)
    try:
        det.predict_host(frames, conf=0.1)
        assert det.status() == 0
        rows = list(range(B)) if rows is None else sorted(set(r % B for r in rows))
        wtk_env = {k: v for k, v in os.environ.items() if k.startswith("WTK_")}
        unobs = lr.unobservable_blobs(scale, nc, dtype, det.plan, wtk_env)
        label = f"{scale} nc={nc} {H}x{W} B={B}/{max_batch} {dtype} {det.plan} rows {rows} env {sorted((env or {}).items())}" + (" product defaults" if product else "")
        rep = lr.check_network(lr.HandleSource(det, B, rows, scale, nc), w, frames[rows], scale, nc, dtype, unobs, label=label,
                               family=_family(scale, nc))
        print("\n" + rep.table())
        launches = _kernel_profile(det, frames, label) if wide_scale else None
        rep.assert_ok()
        if wide_scale:
            # what a scale m / l case exists for: its 3x3 layers run on the window kernel and its odd widths on the implicit GEMM (every conv of a
            # latency-plan handle, and every 3x3 under WTK_NO_HALO=1, is an implicit-GEMM launch), and no layer is 32 channels wide
            assert launches[IGEMM] > 0 and launches[FUSED] == 0 and launches[C32] == 0, launches
            if det.plan == "throughput":
                assert (launches[HALO] == 0) == ((env or {}).get("WTK_NO_HALO") == "1"), launches
    finally:
        det.close()


TINY = [(32, 32, 1), (64, 32, 3), (32, 64, 2)]


@pytest.mark.parametrize("dtype", ["fp32", "f16x3", "fp16"])
@pytest.mark.parametrize("H,W,B", TINY)
def test_tiny_networks_throughput(monkeypatch, H, W, B, dtype):
    """The smallest legal networks: P5 maps of 1 x 1 / 1 x 2, every 3x3 tap but the centre reads padding there."""
    _check(monkeypatch, H, W, B, B, dtype)


@pytest.mark.parametrize("dtype", ["fp32", "f16x3"])
@pytest.mark.parametrize("H,W,B", TINY)
def test_tiny_networks_latency(monkeypatch, H, W, B, dtype):
    _check(monkeypatch, H, W, B, B, dtype, plan="latency")


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "every-blob"])
@pytest.mark.parametrize("dtype", ["fp32", "f16x3", "fp16"])
@pytest.mark.parametrize("H,W,B", [(96, 160, 3), (352, 224, 2), (128, 128, 3)])
def test_small_maps_throughput(monkeypatch, H, W, B, dtype, fused):
    """... with a twin that switches every fusion off, so that every blob is observable."""
    _check(monkeypatch, H, W, B, B, dtype, env=None if fused else NO_FUSION)


@pytest.mark.parametrize("plan", ["auto", "latency"])
@pytest.mark.parametrize("dtype", ["fp32", "f16x3"])
@pytest.mark.parametrize("H,W,B,mb,rows", [(384, 384, 15, 16, (0, 7, 14)), (640, 640, 7, 8, (0, 6)), (128, 128, 3, 4, None)])
def test_small_handles_product_defaults(monkeypatch, H, W, B, mb, rows, dtype, plan):
    """A controller's handles as the product plans them: split-K layers on small maps, narrow tiles, the latency plan."""
    _check(monkeypatch, H, W, B, mb, dtype, plan=plan, product=True, rows=rows)


@pytest.mark.parametrize("env", [{}, {"WTK_NO_HALO": "1", "WTK_NO_S2WIN": "1"}], ids=["defaults", "no-halo-no-s2win"])
@pytest.mark.parametrize("dtype", ["fp16", "f16x3", "fp32"])
@pytest.mark.parametrize("H,W,B,mb,rows", [(640, 512, 33, 40, (0, 31, 32)), (640, 640, 64, 64, (0, 1, 31, 32, 63))])
def test_large_batches_throughput(monkeypatch, H, W, B, mb, rows, dtype, env):
    """Persistent window kernels, ws64, wide 1x1, the stride-2 window — and their implicit-GEMM twins."""
    _check(monkeypatch, H, W, B, mb, dtype, env=env, rows=rows)


@pytest.mark.parametrize("dtype", ["f16x3", "fp32"])
def test_1280x736(monkeypatch, dtype):
    _check(monkeypatch, 1280, 736, 2, 2, dtype, rows=(1,))


def test_call_smaller_than_the_handle(monkeypatch):
    _check(monkeypatch, 384, 384, 5, 8, "f16x3", rows=(0, 4))


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_scale_n(monkeypatch, dtype):
    _check(monkeypatch, 160, 160, 2, 2, dtype, scale="n")


@pytest.mark.parametrize("dtype", ["f16x3", "fp32"])
@pytest.mark.parametrize("nc", [20, 80])
def test_class_tails(monkeypatch, nc, dtype):
    """Fused (nc = 20: cls_ld 24 of a 32-wide tile, padding channels must stay 0) and launched (nc = 80) class tails."""
    _check(monkeypatch, 352, 224, 2, 2, dtype, nc=nc)


def _rescaled(pairs, scale="s"):
    w = dict(ys.synthetic_weights(scale, 1, seed=0))
    for name, f, with_bias in pairs:
        W, b = w[name]
        w[name] = (W * np.float32(f), b * np.float32(f) if with_bias else b)
    return w


@pytest.mark.parametrize("dtype", ["fp16", "f16x3"])
def test_subnormal_range_of_the_hi_half(monkeypatch, dtype):
    """model.4.m.0.cv1 scaled by 2^-8 (its output sits at and below the fp16 normal range), model.4.m.0.cv2 by 2^8."""
    w = _rescaled([("model.4.m.0.cv1", 2.0 ** -8, True), ("model.4.m.0.cv2", 2.0 ** 8, False)])
    _check(monkeypatch, 128, 128, 2, 2, dtype, weights=w)


@pytest.mark.parametrize("dtype", ["fp16", "f16x3"])
def test_activations_near_2_to_13(monkeypatch, dtype):
    """model.5 scaled by 2^11 (stored activations up to ~2^13, inside the range guard), model.6.cv1 by 2^-11."""
    w = _rescaled([("model.5", 2.0 ** 11, True), ("model.6.cv1", 2.0 ** -11, False)])
    _check(monkeypatch, 128, 128, 2, 2, dtype, weights=w)


# ---- scales m and l ----------------------------------------------------------------------------------------------------------------------
# m: widths 48, 96, 192, 384, 576 (bottlenecks 48, 96, 192, 288), C2f depths [2, 4, 4, 2].  What no n / s handle runs: the window kernel with three, six
# and nine 64-channel chunks per tap (fp16: cin 192, 384, 576) and three and nine 32-channel chunks (fp32: cin 96, 288); its 192-cout tile with three
# chunks; 64-cout tiles whose last one is partial (fp32: 96 stored as 128, 288 as 320); the implicit GEMM's K tail 9 * 48 = 432 -> 448 (fp16), its
# 256 x 32 tile at 48 and 288 couts, the 64-wide configuration at 576 = 4.5 x 128 couts; concat buffers 4c and 6c wide with channel offsets 48, 96,
# 144, ...; four bottlenecks on one scratch tensor; SPPF over 288 channels; the materialised upsample as the product default (c[2] % 128 != 0).
# l: widths 64, 128, 256, 512, 512, depths [3, 6, 6, 3]: six bottlenecks on one C2f, 256-wide class towers (no fused class tail), a 64 / 128 front
# (not the fused one), and f16x3 on layers the split kernels have only seen at s widths.
# Which kernel FORM a shape reaches is not visible in the per-file kernel profile the cases print; the shapes below were confirmed with the launch
# lines of the host stub (tests/hostsan: hip_stub.cpp with WTK_STUB_VERBOSE=1, one handle and one call per shape, 256 CUs) — named per test.
WIDE_MODES = [("m", "fp32"), ("m", "fp16"), ("l", "fp32"), ("l", "f16x3"), ("l", "fp16")]


@pytest.mark.parametrize("scale,dtype", WIDE_MODES)
def test_wide_scales_tiny_network(monkeypatch, scale, dtype):
    """32 x 64, B = 2: P5 is 1 x 2, every window block is a 128-pixel one."""
    _check(monkeypatch, 32, 64, 2, 2, dtype, scale=scale, wide_scale=True)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "every-blob"])
@pytest.mark.parametrize("scale,dtype", WIDE_MODES)
def test_wide_scales_small_maps_throughput(monkeypatch, scale, dtype, fused):
    """96 x 160 (B = 3 at m, 2 at l), as the throughput plan fuses it (the box towers' last 1x1 in the 3x3 before it: fp16, f16x3) and with every
    blob stored."""
    _check(monkeypatch, 96, 160, 3 if scale == "m" else 2, 3 if scale == "m" else 2, dtype, env=None if fused else NO_FUSION, scale=scale, wide_scale=True)


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_scale_m_2d_pixel_tiles(monkeypatch, dtype):
    """64 x 256: the stride-4 maps are 16 x 64, so the implicit GEMM's 3x3 layers there (model.1, and model.2's 48-channel bottlenecks, which no window
    kernel takes) run on 2-D pixel tiles (Planner::conv: wo >= 64, wo % 16 == 0, ho % (bm / 16) == 0 with bm = 256 -> tile_w = 16)."""
    _check(monkeypatch, 64, 256, 2, 2, dtype, scale="m", wide_scale=True)


@pytest.mark.parametrize("scale,dtype,plan", [("m", "fp32", "auto"), ("m", "fp16", "auto"), ("m", "fp32", "latency"),
                                              ("l", "fp32", "auto"), ("l", "f16x3", "auto"), ("l", "fp32", "latency"), ("l", "f16x3", "latency")])
def test_wide_scales_small_handles_product_defaults(monkeypatch, scale, dtype, plan):
    """A controller's handle (max_batch 4, B = 3) as the product plans it.  fp32 / f16x3: the latency plan, every conv with rows of 32 input channels on
    the split-K kernel (stub listing: conv_sk_kernel in four tile shapes + sk_finish_kernel; m's 48-channel layers and its materialised-upsample
    1x1s stay on conv_igemm_kernel); fp16 (m, plan auto): the throughput plan with the product's switches."""
    size = 160 if scale == "m" else 128
    _check(monkeypatch, size, size, 3, 4, dtype, plan=plan, product=True, scale=scale, wide_scale=True)


@pytest.mark.parametrize("env", [{}, {"WTK_NO_HALO": "1", "WTK_NO_S2WIN": "1"}], ids=["defaults", "no-halo-no-s2win"])
@pytest.mark.parametrize("dtype,B", [("fp32", 96), ("fp16", 344)])
def test_scale_m_large_batches(monkeypatch, dtype, B, env):
    """192 x 160 with the smallest batch at which the stub listing shows the persistent window form on a 128-cout tile with SIX chunks per tap
    (launch_conv3x3_halo: 2 * tiles >= 3 * CUs):
      fp32, B = 96:  conv3x3_halo_pkernel<float, 128, 432> x 1 — the P3 Detect towers' first conv, 192 -> 64 + 192 couts, six 32-channel chunks (B = 88: none);
      fp16, B = 344: conv3x3_halo_pkernel<_Float16, 128, 432> x 1 — the P4 towers' first conv, 384 -> 256, six 64-channel chunks (B = 336: none), and
                     conv1x1_wide_kernel x 5 (the 384-cout 1x1s of the stride-16 maps; from B = 272 on), 256-pixel window blocks, conv3x3_s2_kernel<256>.
    The layers with an odd chunk count (192 -> 192: three fp16 chunks; 96 -> 96 and 288 -> 288: three and nine fp32 chunks) stay on the one-tile-per-block
    form at every batch.  With the switches the 3x3 layers run as implicit GEMMs (25 launches on the 256 x 64 tile) and the wide 1x1 still runs.
    Rows: first, both sides of the 32-row boundary, 63, last."""
    _check(monkeypatch, 192, 160, B, B, dtype, env=env, rows=(0, 31, 32, 63, -1), scale="m", wide_scale=True)


@pytest.mark.parametrize("dtype", ["fp32", "f16x3", "fp16"])
def test_scale_l_large_batch(monkeypatch, dtype):
    """160 x 128, B = 33 of 40: 256-pixel window blocks on the stride-4 / stride-8 maps, 128-pixel ones behind them, conv3x3_s2_kernel<256> (f16x3);
    57 launches of the 128-cout window tile per pass.  (No persistent form at this size: it takes B >= 138 here; scale s reaches it on the same tile.)"""
    _check(monkeypatch, 160, 128, 33, 40, dtype, rows=(0, 31, 32), scale="l", wide_scale=True)


@pytest.mark.parametrize("dtype", ["fp16", "f16x3"])
def test_subnormal_range_of_the_hi_half_deep_in_scale_l(monkeypatch, dtype):
    """test_subnormal_range_of_the_hi_half on the sixth bottleneck of model.6 at scale l (64 x 96): model.6.m.5.cv1 scaled by 2^-8, its cv2 by 2^8 — the
    residual it is added to has passed five bottlenecks."""
    w = _rescaled([("model.6.m.5.cv1", 2.0 ** -8, True), ("model.6.m.5.cv2", 2.0 ** 8, False)], scale="l")
    _check(monkeypatch, 64, 96, 2, 2, dtype, weights=w, scale="l", wide_scale=True)
