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


def _check(monkeypatch, H, W, B, max_batch, dtype, plan="throughput", env=None, product=False, scale="s", nc=1, rows=None, weights=None, seed=0):
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
        rep.assert_ok()
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


def _rescaled(pairs):
    w = dict(ys.synthetic_weights("s", 1, seed=0))
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
