"""The numpy restatement of the replay kernels (tests/harness/replay_ref.py: per-cycle targets -> sequential scan over cycles -> expansion to frames)
reproduces what the REAL reference wrote: every row of its logs, every move list, and on the hard fixture every row, move and ErrorCalculator value
bit for bit.  CPU only; the GPU tests (tests/test_gpu_replay.py) hold the kernels to the same fixtures."""
import csv
import json
import math
import os

import numpy as np
import pytest

from harness import replay_ref as rr
from oracle import resmlp_oracle
from wtracker_amd.controllers import _read_track_csv
from wtracker_amd.sim import ExperimentConfig, TimingConfig

EXP0 = dict(name="exp0", num_frames=200, frames_per_sec=60, orig_resolution=(1600, 1400), px_per_mm=90, init_position=(1300, 1200))
LOG_KEYS = ["plt_x", "plt_y", "cam_x", "cam_y", "cam_w", "cam_h", "mic_x", "mic_y", "mic_w", "mic_h", "wrm_x", "wrm_y", "wrm_w", "wrm_h"]


def setup(golden_dir, timing=(100, 40, 50)):
    ec = ExperimentConfig(**EXP0)
    tc = TimingConfig(ec, *timing, (4, 4), (0.32, 0.32))
    return tc, rr.Geometry.of(tc, ec), _read_track_csv(os.path.join(golden_dir, "sim_init_bboxes.csv"))


def move_list(g, move, e=0):
    return [[c * g.L + g.I, int(move[c, e, 0]), int(move[c, e, 1])] for c in range(move.shape[0])]


def assert_log_equal(res, path):
    with open(path, newline="") as f:
        gold = list(csv.DictReader(f))
    rows = rr.log_rows(res)
    assert len(rows) == len(gold)
    for r, g in zip(rows, gold):
        assert r["frame"] == int(g["frame"]) and r["cycle"] == int(g["cycle"]) and r["phase"] == g["phase"]
        for k in LOG_KEYS:
            assert float(r[k]) == float(g[k]), (k, r["frame"], r[k], g[k])


def test_geometry_counts(golden_dir):
    _, g, track = setup(golden_dir)
    assert (g.L, g.I, g.M, g.P) == (9, 6, 3, 3) and g.n_log == 22 and g.n_cycles == 22 and g.frame_wh == (1400 + 360, 1600 + 360)


def test_csv_replay_matches_reference_log_and_moves(golden_dir):
    _, g, track = setup(golden_dir)
    pos, move = rr.scan(rr.CSV, g, track)
    assert move_list(g, move) == json.load(open(os.path.join(golden_dir, "sim_moves.json")))["sim_csv_bboxes.csv"]
    res = rr.rows(g, track, pos, move)
    assert_log_equal(res, os.path.join(golden_dir, "sim_csv_bboxes.csv"))
    assert len(res["rows"]) == 198


@pytest.mark.parametrize("tag,timing,name", [("100ms", (100, 40, 50), "sim_mlp_bboxes.csv"), ("200ms", (200, 40, 50), "sim_mlp200_bboxes.csv")])
def test_mlp_replay_matches_reference_log_and_moves(golden_dir, tag, timing, name):
    tc, g, track = setup(golden_dir, timing)
    st = resmlp_oracle.load_state(os.path.join(golden_dir, f"resmlp_{tag}.npz"))
    a, b, v = rr.targets_mlp(g, track, st, rr.max_dist_per_pred(tc, st["pred_frames"], 0.9))
    pos, move = rr.scan(rr.MLP, g, track, a[:, None], b[:, None], v[:, None])
    assert move_list(g, move) == json.load(open(os.path.join(golden_dir, "sim_moves.json")))[name]
    assert_log_equal(rr.rows(g, track, pos, move), os.path.join(golden_dir, name))


def test_optimal_and_polyfit_replay_match_reference_moves(golden_dir):
    _, g, track = setup(golden_dir)
    gold = json.load(open(os.path.join(golden_dir, "sim_moves.json")))
    a, v = rr.targets_optimal(g, track)
    assert move_list(g, rr.scan(rr.OPTIMAL, g, track, a[:, None], None, v[:, None])[1]) == gold["sim_optimal"]
    a, v = rr.targets_polyfit(g, track, 2, [-9, -6, -3, 0, 2, 4], [1, 1, 2, 3, 4, 5])
    assert move_list(g, rr.scan(rr.POLYFIT, g, track, a[:, None], None, v[:, None])[1]) == gold["sim_polyfit"]


@pytest.mark.parametrize("fixture", ["polyfit_cases.json", "polyfit_highdeg.json"])
def test_polyfit_population_matches_reference_moves(golden_dir, fixture):
    """All cases of a fixture as ONE population: the scan is vectorised over experiments."""
    _, g, track = setup(golden_dir)
    cases = json.load(open(os.path.join(golden_dir, fixture)))
    names = sorted(cases)
    tg = [rr.targets_polyfit(g, track, cases[n]["config"]["degree"], cases[n]["config"]["sample_times"], cases[n]["config"]["weights"]) for n in names]
    a, v = np.stack([t[0] for t in tg], axis=1), np.stack([t[1] for t in tg], axis=1)
    _, move = rr.scan(rr.POLYFIT, g, track, a, None, v, E=len(names))
    for e, n in enumerate(names):
        assert move_list(g, move, e) == cases[n]["moves"], n


# ------------------------------------------------------------------------------------------------- the hard fixture
def hard(golden_dir):
    z = np.load(os.path.join(golden_dir, "replay_hard.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    ec = ExperimentConfig("hard", meta["num_frames"], meta["frames_per_sec"], tuple(meta["orig_resolution"]), meta["px_per_mm"], tuple(meta["init_position"]))
    return z, meta, ec


def hard_targets(g, track, meta, name):
    if name == "csv":
        return rr.CSV, None, None
    if name == "optimal":
        a, v = rr.targets_optimal(g, track)
        return rr.OPTIMAL, a[:, None], v[:, None]
    a, v = rr.targets_polyfit(g, track, **meta["polyfit_configs"][int(name[-1])])
    return rr.POLYFIT, a[:, None], v[:, None]


@pytest.mark.parametrize("imaging", [100, 200])
@pytest.mark.parametrize("name", ["csv", "optimal", "polyfit0", "polyfit1", "polyfit2", "polyfit3"])
def test_hard_fixture_rows_moves_and_errors_bit_equal(golden_dir, name, imaging):
    z, meta, ec = hard(golden_dir)
    tc = TimingConfig(ec, imaging, 40, 50, meta["camera_size_mm"], meta["micro_size_mm"])
    g, track, key = rr.Geometry.of(tc, ec), z["track"], f"{name}_{imaging}"
    geo = meta["geometry"][str(imaging)]
    assert (g.L, g.I, g.M, g.P) == (geo["L"], geo["I"], geo["M"], geo["P"]) and g.M == 2
    kind, a, v = hard_targets(g, track, meta, name)
    pos, move = rr.scan(kind, g, track, a, None, v)
    assert move_list(g, move) == z[key + "/moves"].tolist()
    res = rr.rows(g, track, pos, move)
    r = res["rows"]
    assert np.array_equal(r[:, 0:2], z[key + "/plt"]) and np.array_equal(r[:, 2:4], z[key + "/cam"]) and np.array_equal(r[:, 6:8], z[key + "/mic"])
    assert np.array_equal(r[:, 10:14], z[key + "/wrm"]) and np.array_equal(r[:, 14], z[key + "/cycle"]) and np.array_equal(r[:, 15], z[key + "/phase"])
    assert (r[:, 4:6] == geo["camera_size_px"]).all() and (r[:, 8:10] == geo["micro_size_px"]).all()
    assert res["bbox_error"].tobytes() == z[key + "/bbox_error"].tobytes()
    assert res["mse_error"].tobytes() == z[key + "/mse_error"].tobytes()
    # summaries: the tree's rounding error is bounded by ceil(log2 R) * 2^-53 * sum |x|
    R = len(r)
    for q, x in ((0, res["bbox_error"]), (5, res["mse_error"])):
        assert abs(res["summary"][q] - math.fsum(x)) <= math.ceil(math.log2(R)) * 2.0 ** -53 * math.fsum(np.abs(x))
    assert res["summary"][1] == R and res["summary"][4] == (res["bbox_error"] > 1e-7).sum()


def test_hard_fixture_has_the_properties_it_exists_for(golden_dir):
    z, meta, ec = hard(golden_dir)
    track = z["track"]
    assert len(track) == 400 and np.isnan(track).any(axis=1).sum() >= 4
    for imaging in (100, 200):
        g = rr.Geometry.of(TimingConfig(ec, imaging, 40, 50, meta["camera_size_mm"], meta["micro_size_mm"]), ec)
        assert any(np.isnan(track[c * g.L + g.I - g.P]).any() for c in range(g.n_cycles))  # a NaN row at a prediction frame
        share, ties = rr.share_table(g.M), 0
        for name in ("csv", "optimal", "polyfit0", "polyfit1", "polyfit2", "polyfit3"):
            key = f"{name}_{imaging}"
            assert (z[key + "/bbox_error"] > 1e-7).mean() > 0.15
            for mv in z[key + "/moves"][:, 1:].reshape(-1).astype(float):  # the motor's `want` of every step of every move
                carry = 0.0
                for k in range(g.M):
                    want = share[k] * mv + carry
                    ties += abs(want - math.floor(want)) == 0.5
                    carry = want - round(want)
            plt, mv = z[key + "/plt"], z[key + "/moves"]
            gone = plt[g.L :: g.L] - plt[: -g.L : g.L]
            assert (gone[:, 0] != mv[: len(gone), 1]).any() and (gone[:, 1] != mv[: len(gone), 2]).any()  # the clamp binds on both axes
        assert ties > 0  # exact .5 ties: round-half-to-even decides


def test_the_long_tracks_sums_show_the_chunking(monkeypatch):
    """What test_gpu_replay.py::test_summary_sums_have_the_fixed_orders_bits_across_chunks rests on: on long_track (seed 77) at R = 8235 with that test's two
    Polyfit experiments, at least one of the three sums of _tree_sum changes its bits when ROW_CHUNK is halved (the bbox error sum of experiment 1 does),
    so a reduction in another order cannot pass the bit comparison."""
    ec = ExperimentConfig("long", 8236, 60, (1600, 1400), 90, (700, 600))
    g = rr.Geometry.of(TimingConfig(ec, 100, 40, 50, (4, 4), (0.32, 0.32)), ec)
    assert (g.L, g.n_log * g.L) == (9, 2 * rr.ROW_CHUNK + 43)
    track = rr.long_track(8236, 3)
    tg = [rr.targets_polyfit(g, track, 1, [-5, -3, -1, 0, 1]), rr.targets_polyfit(g, track, 2, [-8, -6, -4, -2, 0, 1], [1, 1, 2, 3, 4, 5])]
    pos, move = rr.scan(rr.POLYFIT, g, track, np.stack([a for a, _ in tg], axis=1), None, np.stack([v for _, v in tg], axis=1), E=2)
    differ = []
    for e in range(2):
        res = rr.rows(g, track, pos, move, e, summaries=False)
        r = res["rows"]
        trimmed = (r[:, 15] == 0) & (r[:, 14] != 0) & (r[:, 14] != g.n_log - 1)
        for name, x in (("bbox", res["bbox_error"]), ("trimmed", np.where(trimmed, res["bbox_error"], 0.0)), ("mse", res["mse_error"])):
            full = rr._tree_sum(x)
            with monkeypatch.context() as m:
                m.setattr(rr, "ROW_CHUNK", rr.ROW_CHUNK // 2)
                halved = rr._tree_sum(x)
            if np.float64(full).tobytes() != np.float64(halved).tobytes():
                differ.append((e, name))
    assert differ, "no sum of this track depends on the chunking: choose another seed"
    assert (1, "bbox") in differ


# ------------------------------------------------------------------------------------------------- the Python layer's shared rules (no GPU)
# (num_frames, (imaging, pred, moving) ms at 60 frames/s, hand-counted (n_cycles, n_log) or None)
GEOMETRY_CASES = [(7, (100, 40, 50), (1, 0)),      # I, M, P = 6, 3, 3: the decision frame 6 exists, no cycle ends: nothing is logged
                  (10, (100, 40, 50), (1, 1)),     # one logged cycle
                  (16, (100, 40, 50), (2, 1)),     # a second decision (frame 15) in a cycle that never ends
                  (200, (100, 40, 50), (22, 22)),
                  (10, (100, 0, 50), (1, 1)), (200, (100, 0, 50), None),     # P = 0
                  (4, (50, 40, 100), (1, 0)), (200, (50, 40, 100), None),    # I, M, P = 3, 6, 3
                  (13, (200, 200, 16), (1, 0)), (14, (200, 200, 16), (1, 1)), (200, (200, 200, 16), None)]  # I, M, P = 12, 1, 12


@pytest.mark.parametrize("num_frames,timing,counts", GEOMETRY_CASES)
def test_loop_geometry_equals_the_restatements(num_frames, timing, counts):
    from wtracker_amd.replay import LoopGeometry

    ec = ExperimentConfig(**{**EXP0, "num_frames": num_frames})
    tc = TimingConfig(ec, *timing, (4, 4), (0.32, 0.32))
    for frame_shape in (None, (300, 500)):
        g, ref = LoopGeometry.of(tc, ec, frame_shape), rr.Geometry.of(tc, ec, frame_shape)
        assert (g.L, g.I, g.M, g.P, g.n_cycles, g.n_log, g.n_rows) == (ref.L, ref.I, ref.M, ref.P, ref.n_cycles, ref.n_log, ref.n_log * ref.L)
        assert counts is None or (g.n_cycles, g.n_log) == counts
        assert (g.cam, g.mic, g.frame_shape) == (ref.cam, ref.mic, ref.frame_wh[::-1])
        assert g.decision_frames.tolist() == [c * ref.L + ref.I for c in range(ref.n_cycles)]
        want = dict(num_frames=ref.num_frames, imaging_frame_num=ref.I, moving_frame_num=ref.M, pred_frame_num=ref.P, cam_w=ref.cam[0], cam_h=ref.cam[1],
                    mic_w=ref.mic[0], mic_h=ref.mic[1], frame_w=ref.frame_wh[0], frame_h=ref.frame_wh[1], init_x=ref.init[0], init_y=ref.init[1])
        assert {name: getattr(g.config, name) for name, _ in g.config._fields_} == want
        with pytest.raises(AttributeError):  # (dataclasses.FrozenInstanceError is one)
            g.L = 1


def test_loop_geometry_refusals():
    from wtracker_amd.replay import LoopGeometry

    ec = ExperimentConfig(**EXP0)
    of = lambda *timing, cam=(4, 4), mic=(0.32, 0.32), ec=ec: LoopGeometry.of(TimingConfig(ec, *timing, cam, mic), ec)  # noqa: E731
    of(100, 40, 50)
    with pytest.raises(ValueError, match="moving_frame_num"):
        of(100, 40, 0)
    with pytest.raises(ValueError, match="imaging_frame_num"):
        of(0, 0, 50)
    with pytest.raises(ValueError, match="decision frame"):
        of(100, 40, 50, ec=ExperimentConfig(**{**EXP0, "num_frames": 6}))
    with pytest.raises(ValueError, match="pred_frame_num"):
        of(100, 140, 50)
    with pytest.raises(ValueError, match="smaller than the microscope"):
        of(100, 40, 50, cam=(0.2, 4))
    with pytest.raises(ValueError, match="smaller than the microscope"):
        of(100, 40, 50, cam=(4, 0.2))


@pytest.mark.parametrize("M", [1, 2, 9])
def test_sine_shares_are_the_restatements(M):
    from wtracker_amd.replay import sine_shares

    assert np.array_equal(sine_shares(M), rr.share_table(M)) and sine_shares(M).dtype == np.float64


def test_call_params_reads_pred_kwargs_once_and_refuses_max_det():
    from wtracker_amd.controllers import YoloConfig

    assert YoloConfig("m.wtk").call_params() == (384, 0.1, 0.7)  # the dataclass's own pred_kwargs
    assert YoloConfig("m.wtk", pred_kwargs={}).call_params() == (640, 0.25, 0.7)  # the reference's (ultralytics') defaults
    got = YoloConfig("m.wtk", pred_kwargs={"imgsz": 128.0, "conf": 1, "iou": 0.5, "half": False}).call_params()
    assert got == (128, 1.0, 0.5) and [type(v) for v in got] == [int, float, float]
    with pytest.raises(TypeError, match="max_det"):
        YoloConfig("m.wtk", pred_kwargs={"imgsz": 128, "max_det": 3}).call_params()


class _Frames:
    """A stand-in with a tensor's attributes: `check_device_frames` must refuse on each of them, and no GPU is needed to say so."""

    def __init__(self, shape, is_cuda=True, dtype="torch.uint8", contiguous=True):
        self.shape, self.is_cuda, self.dtype, self._contiguous = shape, is_cuda, dtype, contiguous

    def dim(self):
        return len(self.shape)

    def is_contiguous(self):
        return self._contiguous


def test_check_device_frames_refuses_what_the_library_cannot_read():
    import torch

    from wtracker_amd import hip
    from wtracker_amd.controllers import check_device_frames

    check_device_frames(_Frames((5, 8, 9)))
    check_device_frames(_Frames((5, 8, 9, 3)))
    bad = [torch.zeros((5, 8, 9), dtype=torch.uint8), np.zeros((5, 8, 9), np.uint8), _Frames((5, 8, 9), is_cuda=False),  # on the host
           torch.zeros((5, 8, 9), dtype=torch.float32), _Frames((5, 8, 9), dtype="torch.float32"),                        # not uint8
           _Frames((5, 8, 9, 4)), _Frames((5, 8, 9, 1)), _Frames((8, 9)), _Frames((5, 8, 9, 3, 1)),                        # [F,H,W,4] and other layouts
           _Frames((5, 8, 9), contiguous=False)]
    for fr in bad:
        with pytest.raises(hip.WtkError, match="device_frames"):
            check_device_frames(fr)


def test_nan_rows_keeps_float32_unless_a_frame_has_no_detection():
    from wtracker_amd.controllers import nan_rows

    xywh = np.arange(12, dtype=np.float32).reshape(3, 4)
    found = nan_rows(xywh, np.array([5, 0, 7], dtype=np.int32))
    assert found is xywh and found.dtype == np.float32
    got = nan_rows(xywh, np.array([5, -1, 7], dtype=np.int32))
    assert got.dtype == np.float64 and np.isnan(got[1]).all() and np.array_equal(got[[0, 2]], xywh[[0, 2]].astype(np.float64))
    assert np.array_equal(xywh, np.arange(12, dtype=np.float32).reshape(3, 4))  # the input is left alone
