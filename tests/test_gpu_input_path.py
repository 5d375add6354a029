"""What lies in front of and behind the network, at every kind of frame shape: the letterbox resize (letterbox_kernel, view_letterbox_kernel), its
geometry (csrc/wtk_run.hip:letterbox_geom) and the inverse map of the boxes (csrc/head.hip).

The network input is read back pixel for pixel through a probe stem (tests/harness/input_ref.py) and must equal the oracle's letterbox exactly and
stay within one grey level of an ideal float64 bilinear; the boxes of given logits must equal the restated scale_boxes, in float32 as the oracle
computes it and in float64.  The frame shapes come from a CPU sweep that names, per class, shapes at which a coefficient, an offset or a padding can
be wrong (input_ref.select_shapes): scale n, imgsz 160, frames up to 340 px."""
import os

import numpy as np
import pytest
import torch

from harness import input_ref as ir
from oracle import view_oracle as vo
from oracle import yolo_oracle as yo
from wtracker_amd import frames as fr
from wtracker_amd import hip
from wtracker_amd import yolo_spec as ys

pytestmark = pytest.mark.gpu

IMGSZ = 160
NET_SHAPES = [(32, 160), (64, 160), (96, 160), (128, 160), (160, 160), (160, 128), (160, 96), (160, 64), (160, 32)]  # every network shape of imgsz 160
F32_BOX_ATOL = 2e-2  # pixels: tests/test_gpu_yolo.py's bound of an fp32 handle's boxes against the oracle's


def _handle(weights, net, max_batch, dtype="fp32", scale="n"):
    depth, width, maxch = ys.SCALES[scale]
    return hip.HipYolo(weights, net, max_batch, dtype=dtype, nc=1, width=width, depth=depth, max_channels=maxch)


def _frames(B, h, w, C, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, size=(B, h, w) if C == 1 else (B, h, w, 3), dtype=np.uint8)


def _oracle_input(frames, imgsz):
    with torch.no_grad():
        x, _ = yo.preprocess(list(frames), imgsz)
    return np.ascontiguousarray((x * 255).round().to(torch.uint8).permute(0, 2, 3, 1).numpy())  # [B, net_h, net_w, 3] RGB


def _run(det, frames, entry):
    """One detector call through the host or the device entry point -> the decoded network input."""
    B, H, W = frames.shape[:3]
    C = 1 if frames.ndim == 3 else 3
    if entry == "host":
        det.predict_host(frames, conf=0.1)
    else:
        out = torch.empty((B, 4), dtype=torch.float32, device="cuda")
        det.predict(torch.from_numpy(frames).cuda(), B, H, W, C, out, conf=0.1, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    return ir.decode_network_input(det.debug_tensor(0, B))


def test_the_selector_named_shapes_of_every_class():
    sel = ir.select_shapes(IMGSZ)
    for c in ir.CLASSES:
        assert len(sel[c]) >= 2, (c, sel[c])
    assert sorted(ir.selected_by_net_shape(IMGSZ)) == sorted(NET_SHAPES)  # ... and every one of them is visited by the tests below


@pytest.mark.parametrize("net", NET_SHAPES, ids=lambda n: f"{n[0]}x{n[1]}")
def test_network_input_pixel_for_pixel(hip_lib, net):
    """Every selected frame shape of this network shape on ONE fp32 handle of max_batch 4, call after call: gray frames (B = 2, below max_batch) through
    predict_host, BGR frames (B = 4) through the device entry, then gray through the device entry and BGR through predict_host at another batch size.
    Each call's input must equal the oracle's, so nothing of the staging image may survive from the call before (another shape, a larger batch)."""
    shapes = ir.selected_by_net_shape(IMGSZ)[net]
    det = _handle(ir.probe_weights("n"), net, 4)
    worst = 0.0
    try:
        for k, (h, w) in enumerate(shapes + shapes[:1]):
            g = ir.letterbox_geometry(h, w, IMGSZ)
            assert (g.net_h, g.net_w) == net
            for C, B, entry in ((1, 2, "host"), (3, 4, "device")) if k % 2 == 0 else ((1, 3, "device"), (3, 1, "host")):
                frames = _frames(B, h, w, C, 1000 * h + w + C)
                got = _run(det, frames, entry)
                try:
                    worst = max(worst, ir.check_network_input(got, frames, g, _oracle_input(frames, IMGSZ)))
                except AssertionError as e:
                    raise AssertionError(f"frames {h} x {w} x {C}, B = {B}, {entry} entry, classes {sorted(ir.classify(h, w, IMGSZ))}: {e}") from None
    finally:
        det.close()
    print(f"\nnet {net}: {len(shapes)} frame shapes, worst distance to the ideal bilinear {worst:.4f} grey levels")


@pytest.mark.parametrize("front", ["fused", "unfused"])
def test_network_input_of_f16x3_fronts(hip_lib, monkeypatch, front):
    """The fused front (front_fused_split_kernel) and its unfused twin read the staging image themselves: f16x3 handles at scale s, one shape of the
    resized-size class, one of each pad-tie class, an up- and a more-than-2x-down-scaling one."""
    monkeypatch.setenv("WTK_FRONT_DEBUG" if front == "fused" else "WTK_NO_FUSED_FRONT", "1")
    sel = ir.select_shapes(IMGSZ)
    w = ir.probe_weights("s")
    for c in ("f_resized_size", "g_pad_tie_x", "g_pad_tie_y", "a_up", "b_down_gt2"):
        h, wd = sel[c][0]
        g = ir.letterbox_geometry(h, wd, IMGSZ)
        det = _handle(w, (g.net_h, g.net_w), 3, dtype="f16x3", scale="s")
        try:
            for C, B, entry in ((1, 3, "device"), (3, 2, "host")):
                frames = _frames(B, h, wd, C, h + 1000 * wd + C)
                ir.check_network_input(_run(det, frames, entry), frames, g, _oracle_input(frames, IMGSZ))
        finally:
            det.close()


def test_handles_of_another_shape_pad_to_exactly_their_shape(hip_lib):
    """Frames into a handle that is not their letterbox_shape handle: r = min(S_h / H, S_w / W), padded to exactly (S_h, S_w), as wtk_yolo_predict documents."""
    net = (128, 160)
    det = _handle(ir.probe_weights("n"), net, 3)
    try:
        for h, w in ((100, 100), (50, 100), (301, 200), (77, 333), (128, 160), (64, 64)):
            assert (h, w) == net or ys.letterbox_shape(h, w, IMGSZ) != net
            g = ir.exact_pad_geometry(h, w, *net)
            assert ir.handle_geometry(h, w, *net) == g
            for C, B, entry in ((3, 2, "host"), (1, 3, "device")):
                frames = _frames(B, h, w, C, h * w + C)
                ir.check_network_input(_run(det, frames, entry), frames, g, ir.expected_input(frames, g, yo.resize_bilinear_u8))
    finally:
        det.close()


@pytest.mark.parametrize("frame_shape,cam,C", [((200, 260), (100, 100), 1), ((300, 340), (233, 177), 3), ((180, 220), (90, 121), 3), ((300, 330), (251, 251), 1)])
def test_view_letterbox_pixel_for_pixel(hip_lib, frame_shape, cam, C):
    """wtk_yolo_predict_views: camera view + letterbox in one kernel, at view sizes whose ratio is neither 1 nor 15/16 (1.6 and 1.32 up, 0.69 and
    0.64 down), square and non-square (rows = w, cols = h), gray and BGR, windows over each border and each corner, frame_index with repeats and None.
    The decoded input equals the letterbox of oracle/view_oracle.py:camera_view."""
    H, W = frame_shape
    frames = _frames(5, H, W, C, H + W)
    pos = np.array([[0, 0], [W - 1, H - 1], [W // 2, 2], [3, H // 2], [W - 2, H // 2], [W // 3, H - 1], [W - 1, 0], [0, H - 1]], dtype=np.int32)
    if cam[0] != cam[1]:
        # non-square views: near the right / bottom border the reference's slice runs out of its padded frame and comes back truncated, where the
        # device kernel replicates the border (tests/test_gpu_yolo.py::test_fused_view_crop_letterbox_matches_oracle_views); both agree on full views
        pos[:, 0] = np.minimum(pos[:, 0], W + 2 * (cam[0] // 2) - cam[1])
        pos[:, 1] = np.minimum(pos[:, 1], H + 2 * (cam[1] // 2) - cam[0])
    n = len(pos)
    over = [(p[0] - cam[0] // 2 < 0, p[1] - cam[1] // 2 < 0, p[0] - cam[0] // 2 + cam[1] > W, p[1] - cam[1] // 2 + cam[0] > H) for p in pos.tolist()]
    assert all(any(o[k] for o in over) for k in range(4)) and any(o[0] and o[1] for o in over)  # left, top, right, bottom; a corner
    g = ir.letterbox_geometry(cam[0], cam[1], IMGSZ)
    assert (g.new_h, g.new_w) != cam and cam[0] * 16 != g.new_h * 15
    det = _handle(ir.probe_weights("n"), (g.net_h, g.net_w), n)
    out = torch.empty((n, 4), dtype=torch.float32, device="cuda")
    f_dev, p_dev = torch.from_numpy(frames).cuda(), torch.from_numpy(pos).cuda()
    try:
        for fidx in (np.array([3, 1, 0, 4, 2, 2, 4, 0], dtype=np.int32), None):
            rows = fidx if fidx is not None else np.arange(5)
            m = len(rows)
            views = np.stack([vo.camera_view(frames[f], tuple(int(v) for v in p), cam) for f, p in zip(rows, pos)])
            assert views.shape[1:3] == cam  # full views: rows = w, cols = h
            det.predict_views(f_dev, len(frames), H, W, C, None if fidx is None else torch.from_numpy(fidx).cuda(), p_dev, m, cam[0], cam[1], out,
                              conf=0.1, stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            ir.check_network_input(ir.decode_network_input(det.debug_tensor(0, m)), views, g, _oracle_input(views, IMGSZ))
    finally:
        det.close()


# ---- the inverse map on given logits -----------------------------------------------------------------------------------------------------------
def _given_logits(net, img_hw, A):
    """Seven rows: per level the anchor nearest the centre of the pasted image, with a sharp DFL peak per side chosen so that the box stays inside the
    image where the anchor's centre is inside it by a quarter pixel (`inside`; a sharp peak still leaves ~1e-5 bins of mass elsewhere), and four rows
    whose box leaves the image on the left, top, right, bottom.  Every row has a second, weaker candidate at the far end of its level (the general
    NMS keeps it as its second box)."""
    gain, pad_x, pad_y = ir.back_map(net, img_hw)
    lo = (pad_x, pad_y)
    hi = (pad_x + img_hw[1] * gain, pad_y + img_hw[0] * gain)
    box = np.full((7, A, 64), -8.0, dtype=np.float32)
    cls = np.full((7, A, 1), -10.0, dtype=np.float32)
    winners, inside = [], []
    for row in range(7):
        lvl = row if row < 3 else 0
        s = ys.STRIDES[lvl]
        lh, lw = net[0] // s, net[1] // s
        first = sum((net[0] // t) * (net[1] // t) for t in ys.STRIDES[:lvl])
        ij = [int(np.clip(round((lo[k] + hi[k]) / 2 / s - 0.5), 0, (lw, lh)[k] - 1)) for k in range(2)]
        c = [(ij[k] + 0.5) * s for k in range(2)]
        inside.append(row < 3 and all(lo[k] + 0.25 <= c[k] <= hi[k] - 0.25 for k in range(2)))
        bins = [int(np.clip((c[0] - lo[0] - 0.5) // s, 0, 3)), int(np.clip((c[1] - lo[1] - 0.5) // s, 0, 3)),
                int(np.clip((hi[0] - c[0] - 0.5) // s, 0, 3)), int(np.clip((hi[1] - c[1] - 0.5) // s, 0, 3))]
        if row >= 3:
            bins[row - 3] = 15  # 120 px beyond the anchor: further than any pasted image of imgsz 160 reaches
        a = first + ij[1] * lw + ij[0]
        for side, b in enumerate(bins):
            box[row, a, 16 * side + b] = 8.0
        cls[row, a, 0] = 5.0
        far = first + (0 if a - first >= lh * lw // 2 else lh * lw - 1)
        if far != a:
            cls[row, far, 0] = 2.0
        winners.append(a)
    return box, cls, np.array(winners, dtype=np.int32), inside


def _xywh(b):
    return np.stack([b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], axis=1)


@pytest.mark.parametrize("net", NET_SHAPES, ids=lambda n: f"{n[0]}x{n[1]}")
def test_boxes_of_given_logits_map_back_like_scale_boxes(hip_lib, net):
    """decode_host(box, cls, H, W) and decode_nms_host (max_det 1 and 5) for every selected frame shape (H, W) of this network shape: the anchor is
    yo.postprocess's, the boxes are yo.postprocess's (float32 scale_boxes) and a float64 restatement's within the suite's tolerance for this comparison,
    1e-3 px times max(1, 1 / gain).  A padding off by one moves a box by 1 / gain, at least 50 x that (tests/test_input_ref.py)."""
    det = _handle(ys.synthetic_weights("n", 1, seed=0), net, 8)
    A = det.anchors
    levels_inside = set()
    try:
        for H, W in ir.selected_by_net_shape(IMGSZ)[net]:
            tol = ir.box_tolerance(net, (H, W))
            box, cls, winners, inside = _given_logits(net, (H, W), A)
            thin = min(H, W) <= 2
            assert thin or inside[0], (H, W, inside)
            levels_inside |= {k for k in range(3) if inside[k]}
            tag = f"frames {H} x {W} on net {net}, classes {sorted(ir.classify(H, W, IMGSZ))}, (gain, pad_x, pad_y) = {ir.back_map(net, (H, W))}"
            xywh, conf, anchor = det.decode_host(box, cls, H, W, conf=0.25)
            xywh_o, _, anchor_o = yo.postprocess(torch.from_numpy(box), torch.from_numpy(cls), net, (H, W), conf=0.25)
            np.testing.assert_array_equal(anchor, anchor_o)
            np.testing.assert_array_equal(anchor, winners)
            np.testing.assert_allclose(xywh, xywh_o, rtol=0, atol=tol, err_msg=tag)
            raw, clipped = ir.scale_boxes64(net, np.stack([ir.decode_anchor64(box[n, a], a, net) for n, a in enumerate(winners)]), (H, W))
            for n in range(3):
                if inside[n]:
                    np.testing.assert_array_equal(raw[n], clipped[n], err_msg=tag)  # the restatement's box is not clipped
            for side in range(4):
                assert raw[3 + side, side] != clipped[3 + side, side], (tag, side)  # ... and these are, on their side
            np.testing.assert_allclose(xywh, _xywh(clipped), rtol=0, atol=tol, err_msg=tag)
            dec, scores = yo.decode(torch.from_numpy(box), torch.from_numpy(cls), net)
            for max_det in (1, 5):
                xywh_n, cf_n, _, an_n, cnt_n = det.decode_nms_host(box, cls, H, W, max_det, conf=0.25, iou=0.7)
                for n in range(7):
                    xyxy, sc, _, idx = yo.nms(dec[n], scores[n], 0.25, 0.7, max_det)
                    assert cnt_n[n] == len(idx) == min(max_det, 2) and an_n[n, 0] == winners[n], (tag, n, max_det)
                    np.testing.assert_array_equal(an_n[n, : cnt_n[n]], idx.numpy())
                    np.testing.assert_allclose(xywh_n[n, : cnt_n[n]], _xywh(yo.scale_boxes(net, xyxy, (H, W)).numpy()), rtol=0, atol=tol, err_msg=tag)
                    r64 = ir.scale_boxes64(net, np.stack([ir.decode_anchor64(box[n, a], a, net) for a in idx.tolist()]), (H, W))[1]
                    np.testing.assert_allclose(xywh_n[n, : cnt_n[n]], _xywh(r64), rtol=0, atol=tol, err_msg=tag)
                np.testing.assert_array_equal(xywh_n[:, 0], xywh)  # first row == the max_det = 1 path
    finally:
        det.close()
    assert levels_inside == {0, 1, 2}, (net, levels_inside)  # unclipped boxes were decoded on every level


# ---- end to end --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls_name,pick", [("f_resized_size", 0), ("g_pad_tie_y", 1)])
def test_findings_end_to_end(hip_lib, tmp_path, cls_name, pick):
    """A frame shape of the resized-size class and one of the pad-tie class with the ordinary synthetic weights, through HipYoloController.predict and
    through HipYolo.predict_host on the letterbox_shape handle: the oracle's survivors, boxes within F32_BOX_ATOL of the oracle's.  (The picks are
    those whose oracle decisions are well apart: best against second-best anchor and against the conf threshold by 0.04 logits or more, and no saturated
    scores.  The pad tie is taken on the y axis: the synthetic weights' boxes span a narrow frame's whole width, where the clip hides a shifted x; the x axis
    is held by the given-logits test above.)"""
    from wtracker_amd.controllers import HipYoloController, YoloConfig
    from wtracker_amd.sim import ExperimentConfig, TimingConfig

    H, W = ir.select_shapes(IMGSZ)[cls_name][pick]
    assert cls_name in ir.classify(H, W, IMGSZ)
    B = 4
    y0, x0 = (340 - H) // 2, (340 - W) // 2
    frames = np.ascontiguousarray(fr.diverse_frames(B, 340, seed=1500, per_seed=1)[:, y0 : y0 + H, x0 : x0 + W])
    w = ys.synthetic_weights("n", 1, seed=0)
    oracle = yo.YoloOracle(w, ys.model_dims(0.25, 0.33, 1024, 1))
    xywh_o, conf_o, anchor_o = yo.predict(oracle, list(frames), imgsz=IMGSZ, conf=0.1)
    assert (anchor_o >= 0).sum() >= 2, anchor_o  # there are boxes to compare
    ok = anchor_o >= 0
    if cls_name == "g_pad_tie_y":  # a box edge that the clip does not hold: a shifted padding shows
        assert ((xywh_o[ok, 1] > 0) | (xywh_o[ok, 1] + xywh_o[ok, 3] < H - 1e-3)).any()
    net = ys.letterbox_shape(H, W, IMGSZ)
    det = _handle(w, net, B)
    try:
        xywh, conf, anchor = det.predict_host(frames, conf=0.1)
    finally:
        det.close()
    print(f"\n{cls_name} {H} x {W} -> net {net}: anchors {anchor.tolist()} (oracle {anchor_o.tolist()}), largest box difference {np.abs(xywh[ok] - xywh_o[ok]).max():.4f} px")
    np.testing.assert_array_equal(anchor, anchor_o)
    np.testing.assert_allclose(xywh[ok], xywh_o[ok], rtol=0, atol=F32_BOX_ATOL)
    path = os.path.join(tmp_path, "n.wtk")
    ys.save_weights(path, w, "n", 1)
    cfg = YoloConfig(model_path=path, pred_kwargs={"imgsz": IMGSZ, "conf": 0.1}, dtype="fp32", scale="n")
    ec = ExperimentConfig("synthetic", B, 60, (W, H), 32, (W, H))
    ctl = HipYoloController(TimingConfig(ec, 100, 40, 50, (4, 4), (0.5, 0.5)), cfg)
    try:
        rows = ctl.predict(list(frames))
    finally:
        cfg.model.close()
    assert (np.isnan(rows).all(axis=1) == ~ok).all()
    np.testing.assert_allclose(rows[ok], xywh_o[ok], rtol=0, atol=F32_BOX_ATOL)
