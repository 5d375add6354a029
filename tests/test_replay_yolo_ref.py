"""The numpy restatement of the YOLO controller's device loop (tests/harness/replay_yolo_ref.py) against the host frame loop: harness Simulator + TrackLogger +
the oracle's YOLO controller.  No GPU: the detector is the CPU restatement (oracle/yolo_oracle.py) on both sides, so every difference is the loop's.

The fixture is the closed-loop one of tests/test_gpu_latency.py with another init position, (176, 116): from (128, 128) the host run makes one non-zero move
(0, 0), (0, 0), (0, 0), (0, 1), and the first condition below asks for two."""
import numpy as np
import pytest

from harness import replay_ref as rr
from harness import replay_yolo_ref as ry
from harness.sim_harness import ArrayReader, Simulator
from oracle import view_oracle
from oracle import yolo_oracle as yo
from oracle.controllers_oracle import OracleYoloController
from wtracker_amd import frames as fr
from wtracker_amd import yolo_spec as ys
from wtracker_amd.sim import ExperimentConfig, TimingConfig, TrackLogger

IMGSZ = 128


class RecordingController(OracleYoloController):
    """The oracle's controller, keeping the confidence of every row it predicted (0 for a miss): what the thresholds are chosen from."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.calls = []

    def predict(self, frames):
        xywh, conf, _ = yo.predict(self._model, list(frames), imgsz=self.imgsz, conf=self.conf)
        self.calls.append(np.array(conf))
        return xywh


@pytest.fixture(scope="module")
def fixture():
    w = ys.synthetic_weights("s", 1, seed=0)
    depth, width, maxch = ys.SCALES["s"]
    frames, _ = fr.synthetic_frames(40, 256, seed=8)
    ec = ExperimentConfig("synthetic", 40, 60, (256, 256), 32, ry.FIXTURE_INIT)
    tc = TimingConfig(ec, 100, 40, 50, (4, 4), (0.5, 0.5))
    return dict(frames=frames, ec=ec, tc=tc, oracle=yo.YoloOracle(w, ys.model_dims(width, depth, maxch, 1)))


def host_run(fx, conf):
    ctrl = RecordingController(fx["tc"], fx["oracle"], imgsz=IMGSZ, conf=conf)
    moves = []
    inner = ctrl.provide_movement_vector

    def wrapped(sim):
        m = inner(sim)
        moves.append((int(m[0]), int(m[1])))
        return m

    ctrl.provide_movement_vector = wrapped
    log = TrackLogger(ctrl)
    Simulator(fx["tc"], fx["ec"], log, reader=ArrayReader(fx["frames"])).run()
    return moves, log.rows, ctrl.calls[0::2], ctrl.calls[1::2]  # (confidence of every decision view, confidences of every logged cycle)


@pytest.mark.parametrize("which", [0, 1])
def test_restatement_equals_the_host_loop_move_for_move_and_row_for_row(fixture, which):
    fx, conf = fixture, ry.FIXTURE_CONFS[which]
    tc, frames = fx["tc"], fx["frames"]
    moves, rows, decision_conf, cycle_conf = host_run(fx, conf)
    print("conf", conf, "moves", moves, "decision", [[round(float(v), 4) for v in c] for c in decision_conf], "cycles",
          [[round(float(v), 4) for v in c] for c in cycle_conf])
    assert len(moves) == 4 and len(rows) == 36 and len(cycle_conf) == 4
    # what this threshold is for, asserted on the HOST run
    missed = [int((c == 0).sum()) for c in cycle_conf]
    if which == 0:  # (a) every detection is kept and at least two moves are non-zero
        assert missed == [0, 0, 0, 0] and all((c > 0).all() for c in decision_conf)
        assert sum(m != (0, 0) for m in moves) >= 2
    else:  # (b) a cycle with a miss and a cycle without one: both branches of the dtype rule; a decision view that misses: the (0, 0) move of a NaN row
        assert any(n > 0 for n in missed) and any(n == 0 for n in missed)
        assert any((c == 0).all() for c in decision_conf)
    # the thresholds stay clear of every confidence the run sees (the GPU tests use them with the device's detector, whose confidences differ by ~1e-5)
    seen = np.concatenate(decision_conf + cycle_conf)
    assert np.abs(seen[seen > 0] - conf).min() > 1e-3

    g = rr.Geometry.of(tc, fx["ec"], frame_shape=frames.shape[1:3])
    assert (g.L, g.I, g.M, g.P, g.n_cycles, g.n_log) == (9, 6, 3, 3, 4, 4)

    def predict_views(frame_numbers, positions):
        views = [view_oracle.camera_view(frames[f], p, g.cam) for f, p in zip(frame_numbers, positions)]
        return yo.predict(fx["oracle"], views, imgsz=IMGSZ, conf=conf)[0]

    res = ry.run(g, predict_views)
    assert [tuple(int(v) for v in m) for m in res["moves"][:, 0]] == moves
    mine = rr.log_rows(res)
    assert len(mine) == len(rows)
    for a, b in zip(mine, rows):
        assert (a["frame"], a["cycle"], a["phase"]) == (b["frame"], b["cycle"], b["phase"])
        for k in rr.ROW_COLUMNS[:14]:
            assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), (k, a["frame"], a[k], b[k])
    assert np.array_equal(res["positions"][:, 0], np.array([(r["plt_x"], r["plt_y"]) for r in rows[:: g.L]]))
    # the log's dtype per cycle is the host's: float32 sums where the cycle has no miss
    for c in range(4):
        x = [rows[c * g.L + i]["wrm_x"] for i in range(g.L)]
        assert all(isinstance(v, np.float32) for v in x) == (missed[c] == 0)


def _controller_expression(bbox, cam):
    """provide_movement_vector's lines (wtracker_amd/controllers.py), verbatim, on a numpy row."""
    if not np.isfinite(bbox).all():
        return 0, 0
    mid = bbox[0] + bbox[2] / 2, bbox[1] + bbox[3] / 2
    cam_mid = cam[0] / 2, cam[1] / 2
    return round(mid[0] - cam_mid[0]), round(mid[1] - cam_mid[1])


def test_move_rule_ties_nan_and_the_float32_subtraction():
    cam = (128, 129)
    # centres at exact .5 ties, both directions, and a negative zero
    ties = np.array([[60.0, 62.0, 13.0, 8.0], [61.0, 60.0, 13.0, 10.0], [63.0, 64.0, 1.0, 2.0], [10.25, 3.5, 100.5, 117.0]], dtype=np.float32)
    for row in ties:
        mid = row[:2].astype(np.float64) + row[2:].astype(np.float64) / 2 - np.array(cam) / 2
        assert (np.abs(mid - np.trunc(mid)) == 0.5).any() or (mid == np.trunc(mid)).all()
        assert ry.move_rule(row, cam) == _controller_expression(row, cam)
    assert ry.move_rule(ties[0], cam) == (2, 2)      # 2.5 -> 2 (half to even), 1.5 -> 2
    assert ry.move_rule(ties[1], cam) == (4, 0)      # 3.5 -> 4, 0.5 -> 0
    assert ry.move_rule(ties[2], cam) == (0, 0)      # -0.5 -> -0, 0.5 -> 0
    # a centre so small that the float32 difference rounds onto a tie the float64 difference misses: 0.5 + 2^-23 - 64 is -63.5 in float32
    small = np.array([np.float32(0.5) + np.float32(2.0 ** -23), 0.0, 0.0, 1.0], dtype=np.float32)
    assert float(small[0]) - 64.0 != -63.5 and np.float32(small[0] - np.float32(64.0)) == np.float32(-63.5)
    assert _controller_expression(small, cam) == (-64, -64)  # float64 would give -63 on x
    assert round(float(small[0]) - 64.0) == -63
    assert ry.move_rule(small, cam) == (-64, -64)
    for bad in (np.full(4, np.nan, dtype=np.float32), np.array([1, 2, np.inf, 4], dtype=np.float32), np.array([np.nan, 2, 3, 4], dtype=np.float64)):
        assert ry.move_rule(bad, cam) == _controller_expression(bad, cam) == (0, 0)
    # random rows: the restatement is the controller's expression
    rng = np.random.default_rng(3)
    for row in rng.uniform(0, 128, size=(200, 4)).astype(np.float32):
        assert ry.move_rule(row, cam) == _controller_expression(row, cam)


def test_decision_offset_is_the_deque_entry_the_controller_reads():
    from collections import deque

    for I in range(1, 8):
        for P in range(0, I + 1):
            d = deque(maxlen=I + 3)
            for f in range(I + 1):
                d.append(f)
            assert ry.decision_offset(I, P) == d[-P]
    assert ry.decision_offset(6, 3) == 4 and ry.decision_offset(6, 0) == 0


def test_track_dtype_rule_and_the_rows_round_trip():
    """Per cycle: float32 sums without a miss, float64 sums with one; and replay_ref.rows' (x - cam) + cam returns the track's values exactly."""
    g = rr.Geometry(num_frames=19, I=6, M=3, P=3, cam=(128, 128), mic=(16, 16), frame_wh=(256, 256), init=(3, 250))
    assert g.n_log == 2
    rng = np.random.default_rng(5)
    det = rng.uniform(0, 128, size=(18, 4)).astype(np.float32)
    det[:, 0] += np.float32(1e-3)
    det[12] = np.nan
    fpos = np.tile(np.array([[3, 250]], dtype=np.int32), (18, 1))  # a negative camera corner on x
    trk = ry.track(g, det, fpos)
    cam = np.array([3 - 64, 250 - 64])
    assert np.array_equal(trk[:9, :2], (det[:9, :2] + cam.astype(np.float32)).astype(np.float64))
    assert np.array_equal(trk[9:, :2][np.arange(9) != 3], (det[9:, :2].astype(np.float64) + cam)[np.arange(9) != 3])
    assert not np.array_equal(trk[:9, :2], det[:9, :2].astype(np.float64) + cam)  # the two rules differ on these rows
    assert np.isnan(trk[12]).all() and np.array_equal(trk[:, 2:][np.arange(18) != 12], det[:, 2:][np.arange(18) != 12].astype(np.float64))
    pos, move = np.tile(np.array([[[3, 250]]], dtype=np.int32), (2, 1, 1)), np.zeros((2, 1, 2), dtype=np.int32)
    out = rr.rows(g, trk, pos, move)["rows"]
    keep = np.arange(18) != 12
    assert out[keep, 10:14].tobytes() == trk[keep].tobytes() and (out[12, 10:14] == 0).all()
