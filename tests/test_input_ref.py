"""The input-path harness (tests/harness/input_ref.py) on the CPU: the probe decoder, the geometry restatements, the oracle's fixed-point resize
against an ideal bilinear, and planted defects that the GPU test's pixel and box comparisons must catch."""
import numpy as np
import pytest
import torch

from harness import input_ref as ir
from oracle import yolo_oracle as yo
from wtracker_amd import yolo_spec as ys

IMGSZ = 160


def _images(h, w, seed):
    """random, checkerboard and constant BGR images of one shape, plus a random gray one"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    check = np.where((yy + xx) % 2 == 0, 255, 0).astype(np.uint8)
    return [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8), np.repeat(check[..., None], 3, axis=2), np.full((h, w, 3), 201, dtype=np.uint8),
            rng.integers(0, 256, size=(h, w), dtype=np.uint8)]


def _all_shapes():
    return sorted({s for v in ir.select_shapes(IMGSZ).values() for s in v})


# ---- decoder ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale,H,W", [("n", 32, 64), ("s", 96, 32)])
def test_decoder_recovers_random_inputs_from_the_oracle_stem(scale, H, W):
    """YoloOracle's own float32 stem on the probe weights: the blob decodes to the input, every level 0 .. 255 present."""
    depth, width, maxch = ys.SCALES[scale]
    oracle = yo.YoloOracle(ir.probe_weights(scale), ys.model_dims(width, depth, maxch, 1))
    rng = np.random.default_rng(H + W)
    x = rng.integers(0, 256, size=(2, H, W, 3), dtype=np.uint8)
    x[0, :16, :16, 1] = np.arange(256, dtype=np.uint8).reshape(16, 16)
    with torch.no_grad():
        blob = oracle.conv("model.0", torch.from_numpy(x).permute(0, 3, 1, 2).float() / 255, 2).permute(0, 2, 3, 1).numpy()
    assert blob.dtype == np.float32 and blob.shape == (2, H // 2, W // 2, 16 if scale == "n" else 32)
    np.testing.assert_array_equal(ir.decode_network_input(blob), x)


def test_decoder_refuses_what_it_cannot_read():
    gap = ir.candidate_gap()
    assert 0.5 / 255 <= gap < 0.51 / 255
    cand = ir._candidates()
    blob = np.zeros((1, 2, 2, 16))
    blob[..., :12] = cand[200]
    assert (ir.decode_network_input(blob) == 200).all()
    for delta in (0.2 * gap, -0.2 * gap):  # inside the allowed residual: still level 200
        assert (ir.decode_network_input(blob + np.where(np.arange(16) < 12, delta, 0.0)) == 200).all()
    for bad in (0.26 * gap, -0.4 * gap, 0.5 * gap):  # a value between two candidates is refused, never rounded to one of them
        b = blob.copy()
        b[0, 1, 0, 5] += bad
        with pytest.raises(ir.ProbeDecodeError):
            ir.decode_network_input(b)
    b = blob.copy()
    b[0, 0, 0, 13] = 0.01  # an unused channel must be silu(0) = 0
    with pytest.raises(ir.ProbeDecodeError):
        ir.decode_network_input(b)
    b = blob.copy()
    b[0, 0, 1, 3] = np.nan
    with pytest.raises(ir.ProbeDecodeError):
        ir.decode_network_input(b)
    with pytest.raises(ir.ProbeDecodeError):
        ir.decode_network_input(blob + 1.0)  # beyond silu(1)
    # an fp16 blob is not readable with this margin: the rounding of one fp16 of the log2(e)-scaled value takes most of the allowed residual
    assert 2.0 ** -11 / np.log2(np.e) > 0.5 * gap / 4


# ---- geometry --------------------------------------------------------------------------------------------------------------------------------
def test_geometry_restatements_equal_the_oracle():
    for h, w in _all_shapes() + [(360, 360), (96, 160), (435, 579)]:
        for imgsz in (IMGSZ, 384):
            g = ir.letterbox_geometry(h, w, imgsz)
            if min(g.new_h, g.new_w) < 1:
                continue
            assert tuple(g) == yo.letterbox_geometry(h, w, imgsz) and (g.net_h, g.net_w) == ys.letterbox_shape(h, w, imgsz)
            net = (g.net_h, g.net_w)
            box = np.array([[g.left + 0.25 * g.new_w, g.top + 0.25 * g.new_h, g.left + 0.75 * g.new_w, g.top + 0.5 * g.new_h], [-50.0, -60.0, 900.0, 800.0]])
            want = yo.scale_boxes(net, torch.from_numpy(box), (h, w)).numpy()
            raw, clipped = ir.scale_boxes64(net, box, (h, w))
            np.testing.assert_allclose(clipped, want, rtol=0, atol=1e-12)
            assert (clipped[1] == [0, 0, w, h]).all() and (raw[1] != clipped[1]).all()


def test_the_two_findings_as_the_restatements_show_them():
    """Finding 1: r taken from the handle's short side resizes 435 x 579 to 288 x 383 where the reference resizes to 288 x 384.  Finding 2: the
    padding computed from the float32 gain is 10 at 260 x 300 -> 352 x 384 where scale_boxes has 9."""
    for h, w, imgsz, net, new_ref, new_short in ((435, 579, 384, (288, 384), (288, 384), (288, 383)), (536, 492, 384, (384, 352), (384, 352), (383, 352)),
                                                 (320, 639, 384, (192, 384), (192, 384), (192, 383)), (554, 499, 640, (640, 576), (640, 576), (639, 576))):
        assert ys.letterbox_shape(h, w, imgsz) == net and ir.letterbox_geometry(h, w, imgsz)[2:4] == new_ref
        assert ir.exact_pad_geometry(h, w, *net)[2:4] == new_short and "f_resized_size" in ir.classify(h, w, imgsz)
        assert ir.handle_geometry(h, w, *net) == ir.letterbox_geometry(h, w, imgsz)
    for h, w, imgsz, axis in ((260, 300, 384, "y"), (600, 570, 384, "x"), (469, 670, 384, "y"), (261, 300, 640, "y"), (500, 360, 640, "x")):
        net = ys.letterbox_shape(h, w, imgsz)
        assert "g_pad_tie_" + axis in ir.classify(h, w, imgsz)
        assert ir.back_map(net, (h, w))[1:] != ir.back_map_float_gain(net, (h, w))[1:]
    assert ys.letterbox_shape(260, 300, 384) == (352, 384) and ir.back_map((352, 384), (260, 300))[2] == 9 and ir.back_map_float_gain((352, 384), (260, 300))[2] == 10


def test_handle_rule_is_the_oracle_on_letterbox_shape_handles_and_pad_to_exactly_elsewhere():
    """csrc/wtk_run.hip:letterbox_geom as handle_geometry restates it.  Every shape up to 340 px at imgsz 160, 40 000 drawn shapes of 100 .. 999 px at
    384 and at 640: on the letterbox_shape handle the rule is letterbox_geometry.  Drawn (frame, handle) pairs whose handle is not the frame's
    letterbox_shape handle: the rule is the documented pad-to-exactly geometry."""
    n_f = 0
    for h in range(1, 341):
        for w in range(1, 341):
            g = ir.letterbox_geometry(h, w, IMGSZ)
            assert ir.handle_geometry(h, w, g.net_h, g.net_w) == g, (h, w)
            n_f += ir.exact_pad_geometry(h, w, g.net_h, g.net_w) != g
    assert n_f > 100  # the sweep does reach the shapes on which the two rules differ
    rng = np.random.default_rng(0)
    for imgsz in (384, 640):
        for h, w in rng.integers(100, 1000, size=(40000, 2)).tolist():
            g = ir.letterbox_geometry(h, w, imgsz)
            assert ir.handle_geometry(h, w, g.net_h, g.net_w) == g, (h, w, imgsz)
    n_other = 0
    for h, w, sh, sw in np.concatenate([rng.integers(1, 700, size=(60000, 2)), 32 * rng.integers(1, 21, size=(60000, 2))], axis=1).tolist():
        if (sh, sw) != ys.letterbox_shape(h, w, max(sh, sw)):
            n_other += 1
            assert ir.handle_geometry(h, w, sh, sw) == ir.exact_pad_geometry(h, w, sh, sw), (h, w, sh, sw)
    assert n_other > 50000
    assert ir.handle_geometry(100, 100, 128, 160) == (128, 160, 128, 128, 0, 16) and ir.handle_geometry(50, 100, 128, 160) == (128, 160, 80, 160, 24, 0)


# ---- selector ----------------------------------------------------------------------------------------------------------------------------------
def test_selector_fills_every_class():
    sel = ir.select_shapes(IMGSZ)
    assert set(sel) == set(ir.CLASSES) | {"j_net_shape"}
    for c in ir.CLASSES:
        assert len(sel[c]) >= 2, (c, sel[c])
        for h, w in sel[c]:
            assert c in ir.classify(h, w, IMGSZ) and max(h, w) <= 340
    assert any(h > w for h, w in sel["f_resized_size"]) and any(h < w for h, w in sel["f_resized_size"])
    nets = ir.selected_by_net_shape(IMGSZ)
    assert len(nets) == 9 and all(len(v) >= 2 for v in nets.values())


# ---- pixels ------------------------------------------------------------------------------------------------------------------------------------
def test_oracle_resize_stays_within_one_level_of_the_ideal_bilinear():
    """oracle/yolo_oracle.py:resize_bilinear_u8 (float32 coordinates, 11-bit coefficients, two truncating shifts) against ideal_bilinear on every
    geometry the GPU test uses, with random, checkerboard, constant and gray images.  Measured worst distance: 0.8012 grey levels (random BGR image,
    151 x 96 -> 160 x 102; the figure is printed); the condition is the strict `< 1`: a result never leaves the two integers around the ideal value."""
    worst, at = 0.0, None
    for h, w in _all_shapes():
        g = ir.letterbox_geometry(h, w, IMGSZ)
        if (g.new_h, g.new_w) == (h, w):
            continue
        for k, img in enumerate(_images(h, w, h * 1000 + w)):
            d = float(np.abs(yo.resize_bilinear_u8(img, g.new_h, g.new_w).astype(np.float64) - ir.ideal_bilinear(img, g.new_h, g.new_w)).max())
            if d > worst:
                worst, at = d, (h, w, k)
    print(f"\nworst distance of resize_bilinear_u8 to the ideal bilinear: {worst:.4f} grey levels at (h, w, image) = {at}")
    assert 0.4 < worst < 1.0


def test_ideal_bilinear_from_its_definition():
    """Identity at equal size, exact 2x2 box means at exactly 2x down, a linear ramp stays linear away from the clamped ends."""
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, size=(12, 18, 3)).astype(np.float64)
    np.testing.assert_array_equal(ir.ideal_bilinear(img, 12, 18), img)
    np.testing.assert_allclose(ir.ideal_bilinear(img, 6, 9), img.reshape(6, 2, 9, 2, 3).mean(axis=(1, 3)), rtol=0, atol=1e-12)
    ramp = np.tile(np.arange(30, dtype=np.float64) * 3.0, (4, 1))
    out = ir.ideal_bilinear(ramp, 4, 47)
    xs = (np.arange(47) + 0.5) * 30 / 47 - 0.5
    inner = (xs >= 0) & (xs <= 29)
    np.testing.assert_allclose(out[0, inner], 3.0 * xs[inner], rtol=0, atol=1e-10)
    assert out[0, 0] == 0.0 and out[0, -1] == 87.0  # clamped to the image
    np.testing.assert_allclose(ir.ideal_bilinear(np.array([[10.0, 20.0]]), 3, 5)[1], [10, 11, 15, 19, 20], rtol=0, atol=1e-12)  # a one-row source


def _resize_variant(img, new_h, new_w, half_pixel=True, round_coeff=True):
    """The arithmetic of resize_bilinear_u8 with two switches for planted defects (both on: the same result, asserted below)."""
    h, w = img.shape[:2]
    im = img.reshape(h, w, -1).astype(np.int64)

    def coeffs(n_dst, n_src):
        s = np.float32(n_src) / np.float32(n_dst)
        i = np.arange(n_dst, dtype=np.float32)
        f = ((i + np.float32(0.5)) * s - np.float32(0.5)).astype(np.float32) if half_pixel else (i * s).astype(np.float32)
        i0 = np.floor(f).astype(np.int64)
        f = (f - i0.astype(np.float32)).astype(np.float32)
        lo = i0 < 0
        i0[lo], f[lo] = 0, 0
        hi = i0 >= n_src - 1
        i0[hi], f[hi] = n_src - 1, 0
        a1 = (np.rint(f * np.float32(2048.0)) if round_coeff else np.floor(f * np.float32(2048.0))).astype(np.int64)
        return i0, np.minimum(i0 + 1, n_src - 1), 2048 - a1, a1

    x0, x1, ax0, ax1 = coeffs(new_w, w)
    y0, y1, ay0, ay1 = coeffs(new_h, h)
    rows = im[:, x0, :] * ax0[None, :, None] + im[:, x1, :] * ax1[None, :, None]
    v = (((ay0[:, None, None] * (rows[y0] >> 4)) >> 16) + ((ay1[:, None, None] * (rows[y1] >> 4)) >> 16) + 2) >> 2
    return np.clip(v, 0, 255).astype(np.uint8).reshape(new_h, new_w, *img.shape[2:])


@pytest.mark.parametrize("h,w", [(65, 133), (151, 96), (313, 332), (331, 241)])
def test_planted_pixel_defects_fail_the_comparison(h, w):
    """One up- and one down-scaling shape of each orientation (classes (a), (b) of the selector): the honest image passes check_network_input, an
    image pasted one pixel off, fx / fy without the half-pixel term, truncated coefficients and BGR in place of RGB each fail it."""
    assert {"a_up", "b_down_gt2"} & ir.classify(h, w, IMGSZ)
    rng = np.random.default_rng(h + w)
    frames = rng.integers(0, 256, size=(2, h, w, 3), dtype=np.uint8)
    g = ir.letterbox_geometry(h, w, IMGSZ)
    with torch.no_grad():
        x, _ = yo.preprocess(list(frames), IMGSZ)
    want = np.ascontiguousarray((x * 255).round().to(torch.uint8).permute(0, 2, 3, 1).numpy())
    honest = ir.expected_input(frames, g, _resize_variant)
    np.testing.assert_array_equal(honest, want)
    ir.check_network_input(honest, frames, g, want)
    shifted = g._replace(left=g.left + 1) if g.net_w - g.new_w >= 2 else g._replace(top=g.top + 1)
    assert shifted.top + shifted.new_h <= g.net_h and shifted.left + shifted.new_w <= g.net_w
    defects = {
        "pasted one pixel off": ir.expected_input(frames, shifted, yo.resize_bilinear_u8),
        "no half-pixel term": ir.expected_input(frames, g, lambda im, nh, nw: _resize_variant(im, nh, nw, half_pixel=False)),
        "truncated coefficients": ir.expected_input(frames, g, lambda im, nh, nw: _resize_variant(im, nh, nw, round_coeff=False)),
        "BGR for RGB": np.ascontiguousarray(honest[..., ::-1]),
    }
    for name, img in defects.items():
        with pytest.raises(AssertionError):
            ir.check_network_input(img, frames, g, want)
            pytest.fail(f"planted defect '{name}' passed the pixel comparison")
    # the one-level condition alone (no oracle): a shifted paste and a missing half-pixel term are beyond it on random pixels
    assert ir.ideal_distance(defects["pasted one pixel off"], frames, g) > 1 and ir.ideal_distance(defects["no half-pixel term"], frames, g) > 1


def test_planted_pad_defects_move_a_box_beyond_the_tolerance():
    """A padding off by one moves every box by 1 / gain; at the selected shapes that is at least 50 x the box tolerance, and the float-gain
    padding of class (g) is such a defect."""
    for h, w in _all_shapes():
        g = ir.letterbox_geometry(h, w, IMGSZ)
        net = (g.net_h, g.net_w)
        gain, px, py = ir.back_map(net, (h, w))
        box = [g.left + 0.4 * g.new_w, g.top + 0.4 * g.new_h, g.left + 0.6 * g.new_w, g.top + 0.6 * g.new_h]
        good = ir.scale_boxes64(net, box, (h, w))[0]
        tol = ir.box_tolerance(net, (h, w))
        assert tol == 1e-3 * max(1.0, 1.0 / gain)
        for shift in ((1, 0), (0, 1), (-1, 0), (0, -1)):
            moved = np.abs(ir.scale_boxes64(net, box, (h, w), pad_shift=shift)[0] - good).max()
            assert moved > 50 * tol, (h, w, shift, moved, tol)
        _, qx, qy = ir.back_map_float_gain(net, (h, w))
        cls = ir.classify(h, w, IMGSZ)
        assert (abs(qx - px) == 1) == ("g_pad_tie_x" in cls) and (abs(qy - py) == 1) == ("g_pad_tie_y" in cls)
