"""The model of the Detect head's decisions (tests/harness/head_ref.py) against oracle/yolo_oracle.py on every case list that tests/test_gpu_head.py
runs, the input conditions of those lists, and planted defects: one-line mutants of the model, each of which must change the expected result of a named
case — so a kernel with that defect fails the GPU test.  CPU only.

The model and the oracle are independent statements of the same rules (NumPy float64 boxes against torch float32): anchors, classes, counts and kept
order must be equal, boxes within input_ref.box_tolerance.  The run prints the largest box deviation between the two and the smallest NMS guard."""
import numpy as np
import pytest
import torch

from harness import head_ref as hr
from harness import input_ref as ir
from oracle import yolo_oracle as yo

MEASURED = {"box_dev": 0.0, "guard": np.inf}


def _xywh(b):
    return np.stack([b[:, 0], b[:, 1], b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], axis=1)


def _check_select_case(case):
    tol = ir.box_tolerance(case.net, case.img)
    dev = 0.0
    for lo, box, cls in case.calls():
        hr.check_conditions(cls)
        sel = [hr.select(c, case.conf) for c in cls]
        anchors = np.array([s.anchor for s in sel], dtype=np.int32)
        xywh_o, conf_o, anchor_o = yo.postprocess(torch.from_numpy(box.copy()), torch.from_numpy(cls), case.net, case.img, conf=case.conf)
        np.testing.assert_array_equal(anchors, anchor_o, err_msg=f"{case.name}, rows from {lo}")
        np.testing.assert_allclose(np.array([s.conf for s in sel]), conf_o, rtol=0, atol=1e-6)
        ok = anchors >= 0
        assert np.isnan(np.asarray(xywh_o, dtype=np.float64)[~ok]).all()
        if ok.any():
            d = np.abs(hr.xywh_rows(box, anchors, case.net, case.img)[ok] - np.asarray(xywh_o, dtype=np.float64)[ok]).max()
            assert d <= tol, (case.name, lo, d, tol)
            dev = max(dev, float(d))
    return dev


def _check_nms_case(case):
    tol = ir.box_tolerance(case.net, case.img)
    dev, guard = 0.0, np.inf
    on_threshold = case.name.startswith("iou threshold")
    for lo, box, cls in case.calls():
        hr.check_conditions(cls)
        dec, scores = yo.decode(torch.from_numpy(box), torch.from_numpy(cls), case.net)
        for max_det, iou in case.nms:
            for n in range(len(cls)):
                tag = f"{case.name}, row {lo + n} ({case.rows[lo + n]}), max_det {max_det}, iou {iou!r}"
                got = hr.nms(box[n], cls[n], case.net, case.conf, iou, max_det)
                assert len(got.candidates) <= hr.MAX_CANDIDATES, tag
                xyxy, sc, cl, idx = yo.nms(dec[n], scores[n], case.conf, iou, max_det)
                np.testing.assert_array_equal(got.anchors, idx.numpy(), err_msg=tag)
                np.testing.assert_array_equal(got.classes, cl.numpy(), err_msg=tag)
                np.testing.assert_allclose(got.scores, sc.numpy(), rtol=0, atol=1e-6, err_msg=tag)
                if len(idx):
                    want = _xywh(yo.scale_boxes(case.net, xyxy, case.img).numpy().astype(np.float64))
                    d = np.abs(_xywh(ir.scale_boxes64(case.net, got.xyxy, case.img)[1]) - want).max()
                    assert d <= tol, (tag, d, tol)
                    dev = max(dev, float(d))
                if on_threshold:
                    assert len(got.guards) == 1 and (got.guards[0] == 0.0) == (iou == 0.5), (tag, got.guards)  # the pair sits on 0.5 exactly
                elif len(got.guards):
                    assert got.guards.min() >= hr.MIN_GUARD, f"{tag}: an evaluated pair lies {got.guards.min():.2f} sensitivities from iou"
                    guard = min(guard, float(got.guards.min()))
    return dev, guard


@pytest.mark.parametrize("key", hr.CASE_KEYS, ids=hr.key_id)
def test_model_equals_the_oracle_on_every_case_list(key):
    for case in hr.build_cases(key):
        if case.nms:
            dev, guard = _check_nms_case(case)
            MEASURED["guard"] = min(MEASURED["guard"], guard)
        else:
            dev = _check_select_case(case)
        MEASURED["box_dev"] = max(MEASURED["box_dev"], dev)
        print(f"\n{case.name}: {len(case.cls)} rows, largest oracle-against-model box deviation {dev:.2e} px" + (f", smallest NMS guard {guard:.2f} sensitivities" if case.nms else ""))


def test_measured_numbers():
    """Runs behind the cases above: the two numbers that tests/test_gpu_head.py's docstring records."""
    print(f"\nlargest oracle-against-model box deviation {MEASURED['box_dev']:.2e} px, smallest NMS guard {MEASURED['guard']:.2f} sensitivities")
    if MEASURED["guard"] < np.inf:  # (the whole module ran)
        assert MEASURED["guard"] >= hr.MIN_GUARD


def test_case_lists_are_what_the_gpu_test_needs():
    for net, A in zip(hr.NET_SHAPES, (21, 1344, 1617, 8400)):
        assert hr.n_anchors(net) == A
    assert hr.level_sizes((256, 256))[0] == 1024  # the level boundary coincides with the thread stride
    assert sum(len(c.cls) for nc in (1, 20, 80) for c in hr.random_cases((32, 32), nc)[:2]) == 3 * sum(hr.RANDOM_CHUNKS) >= 200  # rows per shape
    assert [len(c) for _, _, c in hr.random_cases((32, 32), 1)[1].calls()][-1] < hr.MAX_BATCH  # a call with B < max_batch
    names = [n for n, _, _ in hr.placement_pairs((640, 640))]
    for what in ("same thread, 8 passes later", "lane ^ 1:", "lane ^ 32:", "same wave", "wave 0 against wave 15", "partial last pass"):
        assert any(what in n for n in names), what
    A0, A1, _ = hr.level_sizes((224, 352))
    for b in (A0 - 1, A0, A0 + A1 - 1, A0 + A1, 1616):
        pairs = hr.placement_pairs((224, 352))
        assert any(w == b for _, w, _ in pairs) and any(r == b for _, _, r in pairs), b
    assert any(r < w for _, w, r in pairs) and any(r > w for _, w, r in pairs)
    neg = hr.random_cases((32, 32), 20)[2]
    assert neg.conf == 0.1 and (neg.cls < 0).all()


def test_margin_of_the_model_on_hand_written_frames():
    """Literals, so the model is not validated only against what it judges."""
    c = np.full((2000, 1), -8.0, np.float32)
    c[1500, 0], c[3, 0] = 3.0, 1.5
    s = hr.select(c, 0.25)
    assert (s.anchor, s.margin, s.gap) == (1500, np.float32(1.5), np.float32(1.5)) and abs(s.conf - 0.95257413) < 1e-6
    assert abs(s.thr - (3.0 + 1.0986123)) < 1e-6
    s = hr.select(c, 0.97)  # logit(0.97) = 3.4761: not kept, the threshold term binds
    assert s.anchor == -1 and s.conf == 0 and s.winner == 1500 and abs(s.margin - 0.47610) < 1e-5
    c[7, 0] = c[900, 0] = 17.0
    c[1999, 0] = 25.0
    s = hr.select(c, 0.25)  # saturated scores: the lowest index, and the margin is negative
    assert (s.anchor, s.conf, s.margin) == (7, np.float32(1.0), np.float32(-8.0))
    c[:] = np.nan
    assert hr.select(c, 0.25).anchor == -1
    c[5, 0] = -np.inf
    s = hr.select(c, 0.0)  # score 0 is not > 0
    assert s.anchor == -1 and s.winner == 5
    assert hr.conf_logit(1.0) == np.inf and hr.conf_logit(0.0) == -np.inf and hr.conf_logit(0.5) == 0.0


def test_status_of_the_model():
    A = 21
    box, cls = np.zeros((2, A, 64), np.float32), np.zeros((2, A, 1), np.float32)
    assert not hr.status(box, cls, [[3], []])
    box[1, 4, 7] = np.inf
    assert not hr.status(box, cls, [[3], [5]]) and not hr.status(box, cls, [[4], []]) and hr.status(box, cls, [[3], [5, 4]])
    cls[0, 20, 0] = -np.inf
    assert hr.status(box, cls, [[], []])


def test_non_finite_cases_select_like_the_oracle_and_flag_what_they_say():
    """The frames of case f: the oracle steps over NaN anchors and treats +inf as a saturated score too; which of them must raise the flag, on which path."""
    cases = hr.nonfinite_cases()
    flags = []
    for name, cls, box in cases:
        sel = [hr.select(c, 0.25) for c in cls]
        _, _, anchor_o = yo.postprocess(torch.from_numpy(box), torch.from_numpy(cls), hr.NONFINITE_NET, hr.NONFINITE_NET, conf=0.25)
        np.testing.assert_array_equal([s.anchor for s in sel], anchor_o, err_msg=name)
        res = [hr.nms(box[n], cls[n], hr.NONFINITE_NET, 0.25, 0.6, 1) for n in range(len(cls))]
        assert [r.anchors.tolist() for r in res] == [[s.anchor] if s.anchor >= 0 else [] for s in sel], name
        flags.append((hr.status(box, cls, [[s.anchor] if s.anchor >= 0 else [] for s in sel]), hr.status(box, cls, [r.candidates for r in res])))
    assert flags == [(False, False)] + [(True, True)] * (len(cases) - 3) + [(False, True), (False, False)]
    assert "runner-up" in cases[-2][0] and "background" in cases[-1][0]


# ---- planted defects -----------------------------------------------------------------------------------------------------------------------------
def _expected(case, defect):
    """Per row the expected result of the case as arrays: what tests/test_gpu_head.py compares."""
    out = []
    for lo, box, cls in case.calls():
        for n in range(len(cls)):
            if case.nms:
                for max_det, iou in case.nms:
                    r = hr.nms(box[n], cls[n], case.net, case.conf, iou, max_det, defect)
                    out.append((f"{case.rows[lo + n]}, max_det {max_det}", [r.anchors, r.classes, r.xyxy.round(2)]))
            else:
                s = hr.select(cls[n], case.conf, defect)
                out.append((case.rows[lo + n], [np.array([s.anchor]), np.array([s.margin]), hr.xywh_rows(box[n : n + 1], [s.anchor], case.net, case.img, defect).round(2)]))
    return out


# defect -> (case key, index of the case under the key, a word of the row's name)
TEETH = {
    "order_by_logit": (("placement", (256, 256), 1), 0, "saturated scores in different passes"),
    "tie_highest_index": (("placement", (640, 640), 1), 0, "three-way tie"),
    "second_same_thread_only": (("placement", (640, 640), 1), 0, "lane ^ 1:"),
    "second_same_wave_only": (("placement", (640, 640), 1), 0, "wave 0 against wave 15"),
    "second_same_pass_only": (("placement", (640, 640), 1), 0, "same thread, 3 passes later"),
    "score_ge_conf": (("thresholds", (256, 256), 1), 0, "logit 0"),
    "iou_ge": (("iou_threshold", (256, 256), 1), 0, "five columns apart"),
    "no_class_offset": (("nms", (224, 352), 80), 0, "one box under two classes, max_det 300"),
    "last_max_class": (("nms", (640, 640), 80), 0, "one box under two classes, max_det 5"),
    "max_over_cls_ld": (("random", (224, 352), 20), 2, "row 0"),
    "square_level_split": (("placement", (224, 352), 1), 0, "winner at a level boundary"),
}


@pytest.mark.parametrize("defect", hr.DEFECTS)
def test_planted_defect_changes_a_named_case(defect):
    key, k, word = TEETH[defect]
    assert key in hr.CASE_KEYS
    case = hr.build_cases(key)[k]
    good, bad = _expected(case, None), _expected(case, defect)
    changed = [name for (name, g), (_, b) in zip(good, bad) if not all(np.array_equal(x, y, equal_nan=True) for x, y in zip(g, b))]
    assert any(word in name for name in changed), f"the defect {defect} does not change the expected result of '{word}' in {case.name} (it changes: {changed[:5]})"
    print(f"\n{defect}: changes {len(changed)} of {len(good)} results of {case.name}, among them '{next(n for n in changed if word in n)}'")
