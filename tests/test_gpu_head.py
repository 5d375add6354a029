"""The Detect head's decisions on given logits at real anchor counts: csrc/head.hip's head_scan, head_row, head_select_kernel, head_nms_kernel and the
range-guard flag through HipYolo.decode_host / decode_nms_host, against the NumPy model of tests/harness/head_ref.py (which tests/test_head_ref.py holds
to the oracle and arms with planted defects).  Handles are scale n with synthetic weights (only the head buffers matter), max_batch 8.

Shapes, and why each is there:
  32 x 32    A = 21     less than a wave; P5 is 1 x 1; max_det = 300 > A
  256 x 256  A = 1344   A0 = 1024: the P3 / P4 boundary coincides with the thread stride of the 1024-thread scan
  224 x 352  A = 1617   non-square (a level split computed for square maps shows); P5 is 7 x 11
  640 x 640  A = 8400   the product's shape: 8 full passes plus 208 anchors, eight or nine anchors per thread

Input conditions (head_ref.check_conditions, asserted on the fixed seeds by tests/test_head_ref.py; they keep the comparison well defined whatever expf
the device has): all logits on the fp16 grid, none in (9, 17), no finite one below -80; within a frame two unequal best logits are both >= 17 (score
exactly 1.0f, the tie goes by index) or have float64 sigmoids more than 2^-21 apart; every NMS pair evaluated lies at least 2 sensitivities
(8 ulp / shortest side at the class-shifted magnitude) from iou, but the two pairs built to sit on it exactly; at most 400 candidates per frame.

Measured on the CPU (tests/test_head_ref.py): the model's boxes lie within 1.78e-4 px of the oracle's (at gain 0.5; the tolerance there is 2e-3 px), the
smallest NMS guard is 6.54 sensitivities (the class-79 cluster at iou 0.6).  Measured on an MI355X: the largest device-against-model box deviation is
1.81e-4 px (same tolerance).

What is compared: anchors, classes, counts and kept order exactly; conf within 1e-6; the margin bit-equal to the model's where the top-2 gap binds and
within 4 float32 ulps of max(|l_best|, |logit(conf)|) where the threshold term binds (the host's logf may differ by an ulp); boxes within
input_ref.box_tolerance of decode_anchor64 + scale_boxes64."""
import numpy as np
import pytest

from harness import head_ref as hr
from harness import input_ref as ir
from wtracker_amd import hip
from wtracker_amd import yolo_spec as ys

pytestmark = pytest.mark.gpu

F32 = np.float32
MEASURED = {"box_dev": 0.0}


def _handle(net, nc, dtype="fp32"):
    depth, width, maxch = ys.SCALES["n"]
    return hip.HipYolo(ys.synthetic_weights("n", nc, seed=0), net, hr.MAX_BATCH, dtype=dtype, nc=nc, width=width, depth=depth, max_channels=maxch)


def _check_margin(got, s, conf, tag):
    """The margin of one frame against the model's (module docstring)."""
    if s.winner < 0:  # every anchor NaN: not asserted
        return
    if got == s.margin or (np.isnan(got) and np.isnan(s.margin)):
        return
    cl = hr.conf_logit(conf)
    tol = 4 * float(np.spacing(F32(max(abs(s.l_best), abs(cl) if np.isfinite(cl) else 0.0))))
    assert np.isfinite(s.thr), f"{tag}: margin {got!r}, the model's top-2 gap {s.gap!r} (no threshold term)"
    if s.gap < s.thr - tol:
        raise AssertionError(f"{tag}: margin {got!r} is not the top-2 gap {s.gap!r} (winner {s.winner}, threshold term {s.thr!r})")
    want = s.thr if s.gap > s.thr + tol else min(s.gap, s.thr)
    assert abs(float(got) - float(want)) <= tol, f"{tag}: margin {got!r}, the model's {want!r} (gap {s.gap!r}, threshold term {s.thr!r}, allowed {tol:.2e})"


def _check_boxes(xywh, box, anchors, case_net, img, tag):
    """Rows of decode_host against decode_anchor64 + scale_boxes64; rows without a survivor are NaN.  Rows whose survivor has a non-finite box logit
    are left out (the clip turns a NaN coordinate into 0 on the device and leaves it in NumPy)."""
    tol = ir.box_tolerance(case_net, img)
    want = hr.xywh_rows(box, anchors, case_net, img)
    for n, a in enumerate(anchors):
        if a < 0:
            assert np.isnan(xywh[n]).all(), (tag, n, xywh[n])
        elif np.isfinite(box[n][a]).all():
            d = float(np.abs(xywh[n].astype(np.float64) - want[n]).max())
            assert d <= tol, f"{tag}, row {n}: box {xywh[n]} of anchor {a}, the model's {want[n]} ({d:.2e} px apart, allowed {tol:.2e})"
            MEASURED["box_dev"] = max(MEASURED["box_dev"], d)


def _run_select_case(det, case):
    """Every call of a case of the select path: anchor, conf, margin, box of every row.  Returns the model's result per row."""
    every = []
    for lo, box, cls in case.calls():
        B = len(cls)
        xywh, conf, anchor = det.decode_host(box, cls, case.img[0], case.img[1], conf=case.conf)
        margins = det.last_margins(B)
        sel = [hr.select(c, case.conf) for c in cls]
        for n, s in enumerate(sel):
            tag = f"{case.name}, row {lo + n} ({case.rows[lo + n]})"
            assert anchor[n] == s.anchor, f"{tag}: anchor {anchor[n]}, the model's {s.anchor} (winner {s.winner}, logit {s.l_best!r}, margin {s.margin!r})"
            assert abs(float(conf[n]) - float(s.conf)) <= 1e-6, (tag, conf[n], s.conf)
            if s.anchor < 0:
                assert conf[n] == 0
            _check_margin(margins[n], s, case.conf, tag)
        _check_boxes(xywh, box, anchor, case.net, case.img, f"{case.name}, rows from {lo}")
        every += sel
    return every


# ---- a. the placement matrix --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", hr.NET_SHAPES, ids=lambda n: f"{n[0]}x{n[1]}")
def test_winner_and_runner_up_anywhere_in_the_scan(hip_lib, net):
    """A constant background, a winner and a runner-up, one pair per row (head_ref.placement_pairs): the same thread k passes apart, lanes one butterfly
    step apart, the same wave, wave 0 against wave 15, both sides of every level boundary, the partial last pass, r < w and r > w; the same with the
    threshold term binding; exact ties (margin 0, lowest index); saturated scores in different passes (lowest index, negative margin)."""
    case = hr.placement_case(net)
    det = _handle(net, 1)
    try:
        sel = _run_select_case(det, case)
    finally:
        det.close()
    by_name = dict(zip(case.rows, sel))
    tie = by_name["three-way tie across the passes"]
    assert (tie.anchor, tie.margin) == (3, 0.0)
    sat = next(s for n, s in by_name.items() if n.startswith("saturated"))
    assert sat.conf == 1.0 and sat.margin < 0
    assert sum(s.gap > s.thr for s in sel) >= 6 and sum(s.gap < s.thr for s in sel) >= len(hr.placement_pairs(net))  # both terms bound somewhere


# ---- b. random differential ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc", [1, 20, 80])
@pytest.mark.parametrize("net", hr.NET_SHAPES, ids=lambda n: f"{n[0]}x{n[1]}")
def test_random_logits_against_the_model(hip_lib, net, nc):
    """69 frame rows per (shape, nc), 207 per shape, in calls of 8 and one of 5 (B < max_batch); nc = 20 is stored as cls_ld = 24, and in its third case
    every real logit is negative at conf 0.1: the zero-filled padding columns would win if read."""
    det = _handle(net, nc)
    kept = rows = 0
    try:
        for case in hr.random_cases(net, nc):
            sel = _run_select_case(det, case)
            kept += sum(s.anchor >= 0 for s in sel)
            rows += len(sel)
            if "negative" in case.name:
                assert all(s.l_best < 0 for s in sel) and any(s.anchor >= 0 for s in sel)
    finally:
        det.close()
    assert rows >= sum(hr.RANDOM_CHUNKS) and kept > 0
    print(f"\n{net} nc {nc}: {rows} rows, {kept} with a survivor")


# ---- c. thresholds --------------------------------------------------------------------------------------------------------------------------------
def test_score_against_conf_is_strict(hip_lib):
    """Logit 0 has the score 0.5 exactly: NaN row at conf 0.5, kept just below.  conf 0 keeps every ordinary frame and the margin is the top-2 gap; conf 1
    keeps nothing, not even the score 1.0f."""
    det = _handle((256, 256), 1)
    try:
        out = {c.conf: (c, _run_select_case(det, c)) for c in hr.threshold_cases()}
    finally:
        det.close()
    assert out[0.5][1][0].anchor == -1 and out[0.5][1][0].margin == 0 and out[hr.HALF_BELOW][1][0].anchor == 1100 and out[hr.HALF_BELOW][1][0].conf == 0.5
    assert [s.anchor for s in out[0.0][1]] == [1100, 77, 500, 0] and all(s.margin == s.gap for s in out[0.0][1])
    assert [s.anchor for s in out[1.0][1]] == [-1] * 4 and out[1.0][1][2].l_best == 20.0


# ---- d, e. NMS --------------------------------------------------------------------------------------------------------------------------------------
def _xywh(b):
    return np.stack([b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], axis=1)


def _run_nms_case(det, case):
    tol = ir.box_tolerance(case.net, case.img)
    counts = {}
    for lo, box, cls in case.calls():
        B = len(cls)
        for max_det, iou in case.nms:
            xywh, cf, kc, an, cnt = det.decode_nms_host(box, cls, case.img[0], case.img[1], max_det, conf=case.conf, iou=iou)
            for n in range(B):
                tag = f"{case.name}, row {lo + n} ({case.rows[lo + n]}), max_det {max_det}, iou {iou!r}"
                want = hr.nms(box[n], cls[n], case.net, case.conf, iou, max_det)
                k = len(want.anchors)
                assert cnt[n] == k, f"{tag}: {cnt[n]} boxes kept, the model keeps {k}: {an[n, : cnt[n]].tolist()} against {want.anchors.tolist()}"
                np.testing.assert_array_equal(an[n, :k], want.anchors, err_msg=tag)
                np.testing.assert_array_equal(kc[n, :k], want.classes, err_msg=tag)
                np.testing.assert_allclose(cf[n, :k], want.scores, rtol=0, atol=1e-6, err_msg=tag)
                if k:
                    d = float(np.abs(xywh[n, :k].astype(np.float64) - _xywh(ir.scale_boxes64(case.net, want.xyxy, case.img)[1])).max())
                    assert d <= tol, f"{tag}: a box lies {d:.2e} px from the model's (allowed {tol:.2e})"
                    MEASURED["box_dev"] = max(MEASURED["box_dev"], d)
                assert np.isnan(xywh[n, k:]).all() and (an[n, k:] == -1).all() and (kc[n, k:] == -1).all() and (cf[n, k:] == 0).all(), tag  # tail rows
                counts[(lo + n, max_det)] = k
            if max_det == 1:  # the row of the thresholded arg-max path, bit for bit
                x1, c1, a1 = det.decode_host(box, cls, case.img[0], case.img[1], conf=case.conf)
                np.testing.assert_array_equal(a1, an[:, 0])
                np.testing.assert_array_equal(x1, xywh[:, 0])
                np.testing.assert_array_equal(c1, cf[:, 0])
    return counts


@pytest.mark.parametrize("net,nc", hr.NMS_SHAPES, ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else f"nc{v}")
def test_greedy_nms_against_the_model(hip_lib, net, nc):
    """Six frames in two consecutive calls of B = 3 on one handle (head_ref.nms_case): clusters in classes 0, 40 and 79, exact score ties across passes and
    levels, no candidate, 320 candidates (max_det 300 cuts them off; on 32 x 32 max_det = 300 > A), one box under two classes, a cluster at the end of the
    last pass; max_det 300 and 1 at iou 0.6, 5 at iou 0.45."""
    case = hr.nms_case(net, nc)
    det = _handle(net, nc)
    try:
        counts = _run_nms_case(det, case)
    finally:
        det.close()
    assert counts[(2, 300)] == 0 and counts[(0, 1)] == 1 and counts[(0, 5)] == 5
    if net[0] >= 64:
        assert counts[(3, 300)] == 300 and 4 <= counts[(0, 300)] < 24 and counts[(1, 300)] == 5
        assert counts[(4, 300)] == (3 if nc == 80 else 2)  # the same box under two classes is kept twice
    else:
        assert counts[(0, 300)] == 21


def test_iou_on_the_threshold_is_strict(hip_lib):
    """Uniform DFL logits, two P3 anchors five columns apart: IoU = 80 / 160 = 0.5 exactly in fp32.  Both are kept at iou 0.5, the second is suppressed at
    the next float32 below."""
    det = _handle((256, 256), 1)
    try:
        at, below = (_run_nms_case(det, c) for c in hr.iou_threshold_cases())
    finally:
        det.close()
    assert at == {(0, 300): 2, (1, 300): 2} and below == {(0, 300): 1, (1, 300): 1}


# ---- f. non-finite logits ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_non_finite_logits_raise_the_flag(hip_lib, dtype):
    """wtk_yolo_status on the head itself (B = 3 of max_batch 8).  A NaN, +inf or -inf class logit of any anchor of any row raises STATUS_NONFINITE, sticky
    until cleared; the selection steps over NaN anchors, +inf is a saturated score (the index rule applies), -inf never wins, an all-NaN frame gives the
    NaN row (its margin is not asserted).  Box logits: the select path reads only the survivor's, so a non-finite one there raises the flag and one in
    any other anchor does not; the NMS path decodes every candidate's box and flags those — the runner-up's, which max_det = 1 never keeps, included."""
    net = hr.NONFINITE_NET
    det = _handle(net, 1, dtype)
    cases = hr.nonfinite_cases()
    _, clean_cls, clean_box = cases[0]
    flagged = {"select": [], "nms": []}
    try:
        det.status(clear=True)
        for name, cls, box in cases:
            # the select path
            assert det.status(clear=True) == 0, name
            case = hr.Case(f"non-finite ({name})", net, 1, 0.25, cls, box, batch=3)
            sel = _run_select_case(det, case)
            want = hr.status(box, cls, [[s.anchor] if s.anchor >= 0 else [] for s in sel])
            assert (det.status() == hip.STATUS_NONFINITE) == want, f"select path, {name}: status {det.status()}, the model says {want}"
            if want:  # sticky: a clean call leaves it raised, reading with clear returns it once
                flagged["select"].append(name)
                det.decode_host(clean_box, clean_cls, *case.img, conf=0.25)
                assert det.status() == hip.STATUS_NONFINITE and det.status(clear=True) == hip.STATUS_NONFINITE
            assert det.status() == 0
            # the NMS path: max_det 1 (the runner-up is a candidate that is never kept) and 5
            for max_det in (1, 5):
                xywh, cf, kc, an, cnt = det.decode_nms_host(box, cls, *case.img, max_det, conf=0.25, iou=0.6)
                res = [hr.nms(box[n], cls[n], net, 0.25, 0.6, max_det) for n in range(3)]
                for n, r in enumerate(res):
                    np.testing.assert_array_equal(an[n, : cnt[n]], r.anchors, err_msg=f"NMS path, {name}, row {n}, max_det {max_det}")
                want = hr.status(box, cls, [r.candidates for r in res])
                assert (det.status(clear=True) == hip.STATUS_NONFINITE) == want, f"NMS path, max_det {max_det}, {name}: the model says {want}"
                if want and max_det == 1:
                    flagged["nms"].append(name)
    finally:
        det.close()
    names = [n for n, _, _ in cases]
    assert flagged["select"] == names[1:-2], flagged["select"]  # every case but the clean one and the two whose box logit the select path never reads
    assert flagged["nms"] == names[1:-1], flagged["nms"]        # ... the runner-up's box logit is read by the NMS path


def test_measured_device_numbers(hip_lib):
    """Runs behind the tests above: the number the module docstring records."""
    print(f"\nlargest device-against-model box deviation {MEASURED['box_dev']:.2e} px")
