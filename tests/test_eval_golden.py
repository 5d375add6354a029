"""CPU checks of the experiment evaluation (wtracker_amd/evaluation.py, csrc/eval_ops.hip): the numpy restatement tests/harness/eval_ref.py
against the REAL reference's outputs (tests/golden/eval_*.npz, written by tests/golden/make_eval_golden.py), the probe ids, the two row layouts of
the precise error, the new C ABI entry points and the argument checks that run before any device work."""
import ctypes
import os

import numpy as np
import pytest

from harness import eval_ref
from wtracker_amd import evaluation as ev
from wtracker_amd import hip


def _bg_cases(golden_dir):
    z = np.load(os.path.join(golden_dir, "eval_background.npz"))
    for c in range(len(z["meta_frames"])):
        yield (z, c, z[str(z["meta_frames"][c])], int(z["meta_num_probes"][c]), str(z["meta_sampling"][c]), str(z["meta_method"][c]),
               int(z["meta_seed"][c]))


def _precise_cases(golden_dir):
    z = np.load(os.path.join(golden_dir, "eval_precise.npz"))
    c = 0
    while f"ref_{c}" in z:
        dt = np.float32 if bool(z[f"f32_{c}"]) else np.float64
        yield z, c, z["worm"].astype(dt), z["mic"].astype(dt), float(z[f"thresh_{c}"])
        c += 1


def test_probe_ids_equal_the_reference(golden_dir):
    n = 0
    for z, c, frames, num, sampling, method, seed in _bg_cases(golden_dir):
        if seed >= 0:
            np.random.seed(seed)
        ids = ev.probe_indices(len(frames), num, sampling)
        np.testing.assert_array_equal(ids, z[f"ids_{c}"])
        n += 1
    assert n >= 18


def test_background_restatement_equals_the_reference(golden_dir):
    kinds = set()
    for z, c, frames, num, sampling, method, seed in _bg_cases(golden_dir):
        bg = eval_ref.background(frames, z[f"ids_{c}"], method)
        assert bg.dtype == np.uint8 and bg.shape == frames.shape[1:]
        np.testing.assert_array_equal(bg, z[f"bg_{c}"])
        kinds.add((frames.ndim, method, len(z[f"ids_{c}"]) % 2))
    assert len(kinds) == 8  # gray / BGR x median / mean x odd / even n


def test_median_corner_cases_of_numpy():
    """np.median(...).astype(uint8) of an even count is floor((a + b) / 2) of the middle pair: the rule the device median implements."""
    for col, want in (([254, 255], 254), ([1, 3, 4, 200], 3), ([15, 16], 15), ([0, 1], 0), ([7], 7), ([16, 15, 15, 16], 15)):
        frames = np.array(col, dtype=np.uint8).reshape(-1, 1, 1)
        assert int(eval_ref.background(frames, range(len(col)), "median")[0, 0]) == want


def test_precise_restatement_equals_the_reference(golden_dir):
    n = 0
    for z, c, worm, mic, thr in _precise_cases(golden_dir):
        err, counts = eval_ref.precise(z["frames"], z["background"], worm, mic, z["frame_nums"], thr)
        np.testing.assert_array_equal(eval_ref.reference_layout(err), z[f"ref_{c}"])
        legal = ~np.isnan(err)
        assert (counts[~legal] == 0).all() and (counts[:, 1] <= counts[:, 0]).all()
        # the fixture exercises every branch: NaN rows, empty masks, errors strictly between 0 and 1, worms wholly outside the view
        assert (~legal).sum() > 20 and (err[legal] == 0).sum() > 10 and ((err > 0) & (err < 1)).sum() > 20 and (err == 1).sum() > 10
        n += 1
    assert n == 4


def test_reference_layout_is_a_shift_of_the_legal_rows(golden_dir):
    z, _, worm, mic, thr = next(_precise_cases(golden_dir))
    err, _ = eval_ref.precise(z["frames"], z["background"], worm, mic, z["frame_nums"], thr)
    ref = eval_ref.reference_layout(err)
    legal = ~np.isnan(err)
    L = int(legal.sum())
    np.testing.assert_array_equal(ref[:L], err[legal])
    tail = np.arange(L, len(err))
    assert np.isnan(ref[tail[~legal[tail]]]).all() and (ref[tail[legal[tail]]] == 0.0).all()
    # the issue's four-row example: [legal, NaN, legal, legal] -> [e0, e2, e3, 0.0]
    e4, _ = eval_ref.precise(z["frames"], z["background"], worm[:4], mic[:4], z["frame_nums"][:4], thr)
    assert np.isnan(e4[1]) and not np.isnan(e4[[0, 2, 3]]).any()
    np.testing.assert_array_equal(eval_ref.reference_layout(e4), [e4[0], e4[2], e4[3], 0.0])
    # the product's host form of the permutation is the same
    np.testing.assert_array_equal(ev.reference_layout(err), ref)


def test_read_log_takes_rows_and_csv(tmp_path):
    from wtracker_amd.sim import LOG_COLUMNS

    rows = [dict(frame=i, cycle=0, phase="imaging", plt_x=0, plt_y=0, cam_x=0, cam_y=0, cam_w=9, cam_h=9, mic_x=1.5 * i, mic_y=2.0, mic_w=3.0,
                 mic_h=4.0, wrm_x=0.1 * i, wrm_y=0.7, wrm_w=5.25, wrm_h=6.0) for i in range(5)]
    import csv

    path = tmp_path / "log.csv"
    with open(path, "w", newline="") as f:
        w = csv.DictWriter(f, LOG_COLUMNS)
        w.writeheader()
        w.writerows(rows)
    for src in (rows, str(path)):
        fn, worm, mic = ev.read_log(src)
        assert fn.dtype == np.int32 and worm.dtype == mic.dtype == np.float64
        np.testing.assert_array_equal(fn, np.arange(5))
        np.testing.assert_array_equal(worm[:, 0], 0.1 * np.arange(5))
        np.testing.assert_array_equal(mic[:, 0], 1.5 * np.arange(5))


def test_new_entry_points_are_exported(hip_lib):
    for name in ("wtk_background", "wtk_precise_error"):
        assert name in hip.SYMBOLS and hasattr(hip_lib, name)


def test_entry_points_reject_bad_arguments_before_any_launch(hip_lib):
    """Argument checks of the C ABI run on the host before anything is enqueued: a probe count beyond the counters' width is an error, never a
    wrapped result."""
    fake = 1 << 20  # never dereferenced: every call below fails its checks first
    with pytest.raises(hip.WtkError, match="65535"):
        hip.background(fake, 10, 64, fake, hip.BG_MEDIAN_MAX_PROBES + 1, hip.BG_MEDIAN, fake)
    with pytest.raises(hip.WtkError, match="2\\^24"):
        hip.background(fake, 10, 64, fake, hip.BG_MEAN_MAX_PROBES + 1, hip.BG_MEAN, fake)
    with pytest.raises(hip.WtkError, match="method"):
        hip.background(fake, 10, 64, None, 3, 7, fake)
    with pytest.raises(hip.WtkError, match="exceed n_frames"):
        hip.background(fake, 10, 64, None, 11, hip.BG_MEAN, fake)
    with pytest.raises(hip.WtkError, match="null"):
        hip.background(None, 10, 64, None, 3, hip.BG_MEAN, fake)
    lib = hip.load()
    assert lib.wtk_precise_error(ctypes.c_void_p(fake), 4, 0, 8, ctypes.c_void_p(fake), ctypes.c_void_p(fake), ctypes.c_void_p(fake), 1,
                                 ctypes.c_void_p(fake), 3, 10.0, ctypes.c_void_p(fake), None, None, None) != 0
    assert b"H x W" in lib.wtk_last_error()


def test_python_layer_rejects_what_it_cannot_compute():
    with pytest.raises(ValueError, match="sampling"):
        ev.probe_indices(10, 3, "stratified")
    with pytest.raises(ValueError, match="method"):
        ev.background(np.zeros((3, 4, 4), np.uint8), 2, method="mode")
    boxes = np.zeros((1, 4))
    with pytest.raises(ValueError, match="gray"):
        ev.precise_error(np.zeros((2, 4, 4, 3), np.uint8), np.zeros((4, 4, 3), np.uint8), boxes, boxes, [0])
    with pytest.raises(ValueError, match="layout"):
        ev.precise_error(np.zeros((2, 4, 4), np.uint8), np.zeros((4, 4), np.uint8), boxes, boxes, [0], layout="shifted")
