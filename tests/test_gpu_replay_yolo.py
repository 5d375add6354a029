"""wtracker_amd.replay.YoloReplay on the MI355X: the YOLO controller's closed loop from device-resident state (csrc/replay_yolo.hip: wtk_replay_yolo_step,
_positions, _track) against the host frame loop it replaces (Simulator + TrackLogger + HipYoloController on device frames: same handles, same kernels, same
inputs, so the same BITS) and against the pinned numpy restatement (tests/harness/replay_yolo_ref.py, held to the host loop by tests/test_replay_yolo_ref.py)."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from harness import replay_ref as rr  # noqa: E402
from harness import replay_yolo_ref as ry  # noqa: E402
from harness.sim_harness import ArrayReader, Simulator  # noqa: E402
from wtracker_amd import frames as fr  # noqa: E402
from wtracker_amd import hip  # noqa: E402
from wtracker_amd import yolo_spec as ys  # noqa: E402
from wtracker_amd.controllers import HipYoloController, PolyfitConfig, YoloConfig  # noqa: E402
from wtracker_amd.sim import ExperimentConfig, TimingConfig, TrackLogger  # noqa: E402

IMGSZ = 128
SUMMARY_FIELDS = ("bbox_error_sum", "rows", "trimmed_bbox_error_sum", "trimmed_rows", "non_perfect_rows", "mse_error_sum")


@pytest.fixture(scope="module")
def torch_mod(hip_lib):
    import torch

    if hip.device_count() < 1:
        pytest.fail("no HIP device visible")
    return torch


@pytest.fixture(scope="module")
def fixture(torch_mod, tmp_path_factory):
    """The closed-loop fixture of tests/test_replay_yolo_ref.py (see replay_yolo_ref.FIXTURE_INIT), frames on the device."""
    path = str(tmp_path_factory.mktemp("yolo_replay") / "s.wtk")
    ys.save_weights(path, ys.synthetic_weights("s", 1, seed=0), "s", 1)
    frames, _ = fr.synthetic_frames(40, 256, seed=8)
    ec = ExperimentConfig("synthetic", 40, 60, (256, 256), 32, ry.FIXTURE_INIT)
    tc = TimingConfig(ec, 100, 40, 50, (4, 4), (0.5, 0.5))
    return dict(path=path, frames=frames, dev_frames=torch_mod.from_numpy(frames).cuda(), ec=ec, tc=tc, geo=rr.Geometry.of(tc, ec, frame_shape=frames.shape[1:3]))


def config(fx, conf, plan="auto", **kw):
    return YoloConfig(model_path=fx["path"], device="cuda", pred_kwargs={"imgsz": IMGSZ, "conf": conf}, dtype="f16x3", scale="s", plan=plan, **kw)


def plan_env(monkeypatch):
    """The handles as a user gets them: none of the suite's plan switches set (tests/conftest.py)."""
    for v in ("WTK_LATENCY_PLAN", "WTK_NO_SK_MIXED", "WTK_SMALL_NARROW"):
        monkeypatch.delenv(v, raising=False)


def host_loop(fx, cfg):
    ctrl = HipYoloController(fx["tc"], cfg, device_frames=fx["dev_frames"])
    moves = []
    inner = ctrl.provide_movement_vector

    def wrapped(sim):
        m = inner(sim)
        moves.append((int(m[0]), int(m[1])))
        return m

    ctrl.provide_movement_vector = wrapped
    log = TrackLogger(ctrl)
    Simulator(fx["tc"], fx["ec"], log, reader=ArrayReader(fx["frames"])).run()
    return moves, log.rows


def assert_rows_bit_equal(mine, rows):
    assert len(mine) == len(rows)
    for a, b in zip(mine, rows):
        assert (a["frame"], a["cycle"], a["phase"]) == (b["frame"], b["cycle"], b["phase"])
        for k in rr.ROW_COLUMNS[:14]:
            assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), (k, a["frame"], a[k], b[k])


def assert_summary_equal(a, b):
    for name in SUMMARY_FIELDS:
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name


# ------------------------------------------------------------------------------------------------- 1: the host loop
@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("plan", ["auto", "latency"])
def test_run_equals_the_host_loop_bit_for_bit(torch_mod, fixture, monkeypatch, plan, which):
    from wtracker_amd.replay import YoloReplay, _summary_of

    torch, fx, conf = torch_mod, fixture, ry.FIXTURE_CONFS[which]
    plan_env(monkeypatch)
    cfg = config(fx, conf, plan)
    moves, rows = host_loop(fx, cfg)
    missed = [sum(all(r[k] == 0 for k in ("wrm_x", "wrm_y", "wrm_w", "wrm_h")) for r in rows[c * 9:(c + 1) * 9]) for c in range(4)]
    print("conf", conf, "plan", plan, "host moves", moves, "missed rows per cycle", missed)
    if which == 0:  # the conditions of the CPU test, on this detector's host run
        assert missed == [0, 0, 0, 0] and sum(m != (0, 0) for m in moves) >= 2
    else:
        assert any(n > 0 for n in missed) and any(n == 0 for n in missed)
    yr = YoloReplay(fx["dev_frames"], fx["tc"], fx["ec"], cfg)
    assert yr.step_detector.plan == "latency" and yr.log_detector.plan == ("throughput" if plan == "auto" else "latency")
    assert (yr.step_detector is yr.log_detector) == (plan == "latency") and len(cfg.model._dets) == (2 if plan == "auto" else 1)
    res = yr.run()
    assert [tuple(int(v) for v in m) for m in res.moves[0]] == moves
    assert_rows_bit_equal(res.log(0), rows)
    assert np.array_equal(res.positions[0], np.array([(r["plt_x"], r["plt_y"]) for r in rows[::9]]))
    assert tuple(res.detections.shape) == (36, 4) and res.detections.dtype == torch.float32 and res.detections.is_cuda
    # the summary: wtk_replay_rows fed the HOST loop's positions, moves and track (the track as TrackLogger holds it before it zeroes the misses)
    g, dev = fx["geo"], fx["dev_frames"].device
    pos = np.array([(r["plt_x"], r["plt_y"]) for r in rows[::9]], dtype=np.int32).reshape(4, 1, 2)
    move = np.array(moves, dtype=np.int32).reshape(4, 1, 2)
    track = np.array([[float(r[k]) for k in ("wrm_x", "wrm_y", "wrm_w", "wrm_h")] for r in rows], dtype=np.float64)
    track[(track == 0).all(axis=1)] = np.nan
    summary = torch.zeros((1, 6), dtype=torch.float64, device=dev)
    scratch = torch.zeros((hip.replay_scratch_doubles(1, 36),), dtype=torch.float64, device=dev)
    share = torch.from_numpy(rr.share_table(g.M)).to(dev)
    hip.replay_rows(yr._cfg, 1, 4, torch.from_numpy(track).to(dev), 36, share, torch.from_numpy(pos).to(dev), torch.from_numpy(move).to(dev), None, 0, None, None,
                    None, summary, scratch, scratch.numel(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert_summary_equal(res.summary, _summary_of(summary.cpu().numpy()))
    assert res.summary.rows[0] == 36 and res.summary.non_perfect_rows[0] > 0
    # and the restatement's kernels on the device's own detections: positions, track, rows
    det = res.detections.cpu().numpy()
    fpos = ry.frame_positions(g, res.positions.transpose(1, 0, 2), res.moves.transpose(1, 0, 2))
    ref = rr.rows(g, ry.track(g, det, fpos), res.positions.transpose(1, 0, 2), res.moves.transpose(1, 0, 2))
    assert res.row_array(0).tobytes() == ref["rows"].tobytes()
    assert np.array_equal(yr._frame_pos.cpu().numpy(), fpos)


# ------------------------------------------------------------------------------------------------- 2: a large log batch
def test_log_batch_64_runs_a_partial_chunk_on_its_own_handle(torch_mod, fixture, monkeypatch):
    from wtracker_amd.replay import YoloReplay

    torch, fx = torch_mod, fixture
    plan_env(monkeypatch)
    cfg = config(fx, ry.FIXTURE_CONFS[0])
    base = YoloReplay(fx["dev_frames"], fx["tc"], fx["ec"], cfg).run()
    for log_batch in (64, 16):  # 36 of 64: one partial chunk; 16: two full chunks and a partial one
        yr = YoloReplay(fx["dev_frames"], fx["tc"], fx["ec"], cfg, log_batch=log_batch)
        assert yr.log_detector.plan == "throughput" and yr.log_detector.max_batch == log_batch and yr.log_detector not in cfg.model._dets.values()
        res = yr.run()
        assert np.array_equal(res.moves, base.moves) and np.array_equal(res.positions, base.positions)
        # direct calls on that same handle at res's positions
        g = fx["geo"]
        fpos = ry.frame_positions(g, res.positions.transpose(1, 0, 2), res.moves.transpose(1, 0, 2))
        dev = fx["dev_frames"].device
        out = torch.zeros((36, 4), dtype=torch.float32, device=dev)
        idx, pos = torch.arange(36, dtype=torch.int32, device=dev), torch.from_numpy(fpos).to(dev)
        f = fx["dev_frames"]
        for r0 in range(0, 36, log_batch):
            n = min(log_batch, 36 - r0)
            yr.log_detector.predict_views(f, f.shape[0], f.shape[1], f.shape[2], 1, idx[r0:r0 + n], pos[r0:r0 + n], n, 128, 128, out[r0:r0 + n], conf=ry.FIXTURE_CONFS[0],
                                          stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert res.detections.cpu().numpy().tobytes() == out.cpu().numpy().tobytes()
        yr.close()


# ------------------------------------------------------------------------------------------------- 3: the step kernel alone
def test_step_kernel_on_hand_made_rows(torch_mod):
    torch = torch_mod
    dev = torch.device("cuda", 0)
    nan = float("nan")
    # geometry of replay_hard.npz's timing (M = 2: shares 0.5 - 2^-54 and 0.5), a small frame so that moves reach the clamp
    geo = dict(num_frames=400, imaging_frame_num=3, moving_frame_num=2, pred_frame_num=2, camera_size=(360, 361), micro_size=(29, 29), frame_wh=(500, 400),
               init_position=(22, 14))
    g = rr.Geometry(400, 3, 2, 2, (360, 361), (29, 29), (500, 400), (22, 14))
    share_np = rr.share_table(2)
    assert share_np[0] < 0.5 and share_np[1] == 0.5 and 0.5 - share_np[0] < 2.0 ** -53
    cfg = hip.replay_config(**geo)
    C = g.n_cycles
    share = torch.from_numpy(share_np).to(dev)
    small = float(np.float32(0.5) + np.float32(2.0 ** -23))
    cases = [  # (row, position before)
        ([nan, nan, nan, nan], (22, 14)),                 # no detection
        ([1.0, nan, 3.0, 4.0], (250, 200)),               # one value not finite
        ([176.0, 180.0, 13.0, 8.0], (250, 200)),          # ties: 2.5 -> 2, 3.5 -> 4
        ([179.0, 180.0, 1.0, 2.0], (250, 200)),           # -0.5 -> 0, 0.5 -> 0
        ([small, 0.0, 0.0, 1.0], (250, 200)),             # float32 difference -179.5 (a tie) where float64 gives -179.4999999: -180
        ([0.0, 0.0, 2.0, 3.0], (60, 70)),                 # (-179, -179) from (60, 70): clamps at 0 on both axes
        ([355.0, 356.0, 5.0, 5.0], (450, 350)),           # (+178, +178) from (450, 350): clamps at 499 / 399
        ([200.0, 150.0, 7.0, 9.0], (250, 200)),           # odd moves through the 0.5 -/+ 1 ulp shares
        ([181.0, 180.0, 1.0, 4.0], (250, 200)),           # move 1 / 1: want = share * 1 on either side of the tie
    ]
    for row, p0 in cases:
        for c in (0, C - 2, C - 1):
            pos = torch.full((C, 1, 2), -77, dtype=torch.int32, device=dev)
            move = torch.full((C, 1, 2), -77, dtype=torch.int32, device=dev)
            pos[c, 0] = torch.tensor(p0, dtype=torch.int32, device=dev)
            xywh = torch.tensor(row, dtype=torch.float32, device=dev)
            hip.replay_yolo_step(cfg, C, c, xywh, share, pos, move, stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            mv, nxt = ry.step(g, share_np, np.array(row, dtype=np.float32), p0)
            pos_h, move_h = pos.cpu().numpy(), move.cpu().numpy()
            assert np.array_equal(move_h[c, 0], mv), (row, c)
            expect_pos = np.full((C, 1, 2), -77, dtype=np.int32)
            expect_pos[c, 0] = p0
            if c + 1 < C:
                expect_pos[c + 1, 0] = nxt
            assert np.array_equal(pos_h, expect_pos), (row, c)  # nothing else written: the last cycle has no next position
            move_h[c, 0] = -77
            assert (move_h == -77).all()
    assert np.array_equal(ry.step(g, share_np, np.array(cases[2][0], dtype=np.float32), (250, 200))[0], [2, 4])
    assert np.array_equal(ry.step(g, share_np, np.array(cases[4][0], dtype=np.float32), (250, 200))[0], [-180, -180])
    assert np.array_equal(ry.step(g, share_np, np.array(cases[5][0], dtype=np.float32), (60, 70))[1], [0, 0])
    assert np.array_equal(ry.step(g, share_np, np.array(cases[6][0], dtype=np.float32), (450, 350))[1], [499, 399])


# ------------------------------------------------------------------------------------------------- 4: the scan keeps its bits
@pytest.mark.parametrize("imaging", [100, 200])
def test_scan_and_rows_still_equal_the_restatement_on_the_hard_fixture(torch_mod, golden_dir, imaging):
    """The motor steps moved into a function the YOLO kernels share: wtk_replay_scan and wtk_replay_rows on replay_hard.npz's configurations, bit for bit
    the numpy restatement's positions, moves and rows (every kind but the MLP, whose targets need a model and whose motor is the same)."""
    from wtracker_amd.replay import Replay

    z = np.load(os.path.join(golden_dir, "replay_hard.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    ec = ExperimentConfig("hard", meta["num_frames"], meta["frames_per_sec"], tuple(meta["orig_resolution"]), meta["px_per_mm"], tuple(meta["init_position"]))
    tc = TimingConfig(ec, imaging, 40, 50, meta["camera_size_mm"], meta["micro_size_mm"])
    track = z["track"]
    rp, g = Replay(track, tc, ec), rr.Geometry.of(tc, ec)
    assert g.M == 2
    cfgs = [PolyfitConfig(**kw) for kw in meta["polyfit_configs"]]
    for tg, kind in ((rp.csv(), rr.CSV), (rp.optimal(), rr.OPTIMAL), (rp.polyfit(cfgs), rr.POLYFIT)):
        res = rp.run(tg, rows=range(tg.E))
        a = None if tg.a is None else tg.a.cpu().numpy()
        valid = None if tg.valid is None else tg.valid.cpu().numpy()
        pos, move = rr.scan(kind, g, track, a, None, valid, E=tg.E)
        assert np.array_equal(res.moves, move.transpose(1, 0, 2)) and np.array_equal(res.positions, pos.transpose(1, 0, 2))
        assert (move != 0).any()
        for e in range(tg.E):
            assert res.row_array(e).tobytes() == rr.rows(g, track, pos, move, e=e, summaries=False)["rows"].tobytes()


# ------------------------------------------------------------------------------------------------- 5: refusals
def test_refusals(torch_mod, fixture):
    from wtracker_amd.replay import YoloReplay

    torch, fx = torch_mod, fixture
    cfg = config(fx, 0.1)
    f, tc, ec = fx["dev_frames"], fx["tc"], fx["ec"]
    refused = (ValueError, hip.WtkError)
    with pytest.raises(refused, match="recheck_margin"):
        YoloReplay(f, tc, ec, config(fx, 0.1, recheck_margin=0.08))
    for bad in (fx["frames"], torch.from_numpy(fx["frames"]), f.to(torch.float32), f[:, :, ::2], f[:, None]):
        with pytest.raises(refused, match="device_frames"):
            YoloReplay(bad, tc, ec, cfg)
    with pytest.raises(refused, match="39 frames"):
        YoloReplay(f[:39].contiguous(), tc, ec, cfg)
    # what wtk_replay_rows refuses: a camera smaller than the microscope, no moving phase, pred_frame_num beyond the imaging phase
    with pytest.raises(refused, match="smaller than the microscope"):
        YoloReplay(f, TimingConfig(ec, 100, 40, 50, (0.4, 4), (0.5, 0.5)), ec, cfg)
    with pytest.raises(refused, match="moving_frame_num"):
        YoloReplay(f, TimingConfig(ec, 100, 40, 0, (4, 4), (0.5, 0.5)), ec, cfg)
    with pytest.raises(refused, match="pred_frame_num"):
        YoloReplay(f, TimingConfig(ec, 100, 140, 50, (4, 4), (0.5, 0.5)), ec, cfg)
    # the entry points: null pointers, c out of range, bad geometry; nothing is written
    dev = f.device
    geo = dict(num_frames=40, imaging_frame_num=6, moving_frame_num=3, pred_frame_num=3, camera_size=(128, 128), micro_size=(16, 16), frame_wh=(256, 256),
               init_position=(128, 128))
    share = torch.from_numpy(rr.share_table(3)).to(dev)
    pos, move = torch.full((4, 1, 2), -77, dtype=torch.int32, device=dev), torch.full((4, 1, 2), -77, dtype=torch.int32, device=dev)
    xywh = torch.zeros((36, 4), dtype=torch.float32, device=dev)
    fpos = torch.full((36, 2), -77, dtype=torch.int32, device=dev)
    track = torch.full((36, 4), -12345.5, dtype=torch.float64, device=dev)

    def step(c=0, n_cycles=4, **over):
        p = dict(xywh=xywh, share=share, pos=pos, move=move)
        cfg_over = {k: over.pop(k) for k in list(over) if k in geo}
        p.update(over)
        hip.replay_yolo_step(hip.replay_config(**{**geo, **cfg_over}), n_cycles, c, p["xywh"], p["share"], p["pos"], p["move"])

    def positions(n_cycles=4, **over):
        p = dict(share=share, pos=pos, move=move, fpos=fpos)
        cfg_over = {k: over.pop(k) for k in list(over) if k in geo}
        p.update(over)
        hip.replay_yolo_positions(hip.replay_config(**{**geo, **cfg_over}), n_cycles, p["share"], p["pos"], p["move"], p["fpos"])

    def to_track(n_cycles=4, **over):
        p = dict(xywh=xywh, fpos=fpos, track=track)
        cfg_over = {k: over.pop(k) for k in list(over) if k in geo}
        p.update(over)
        hip.replay_yolo_track(hip.replay_config(**{**geo, **cfg_over}), n_cycles, p["xywh"], p["fpos"], p["track"])

    bad_geo = [dict(moving_frame_num=0), dict(imaging_frame_num=0), dict(pred_frame_num=7), dict(camera_size=(8, 128)), dict(frame_wh=(0, 256)),
               dict(frame_wh=(9000, 256)), dict(n_cycles=3), dict(n_cycles=5)]
    for call, names in ((step, ("xywh", "share", "pos", "move")), (positions, ("share", "pos", "move", "fpos")), (to_track, ("xywh", "fpos", "track"))):
        for over in bad_geo:
            with pytest.raises(hip.WtkError):
                call(**over)
        for name in names:
            with pytest.raises(hip.WtkError):
                call(**{name: None})
    for c in (-1, 4):
        with pytest.raises(hip.WtkError, match="cycle outside"):
            step(c=c)
    with pytest.raises(hip.WtkError):
        hip.replay_yolo_step(None, 4, 0, xywh, share, pos, move)
    torch.cuda.synchronize()
    assert (pos == -77).all() and (move == -77).all() and (fpos == -77).all() and (track == -12345.5).all()


# ------------------------------------------------------------------------------------------------- 6: twice
def test_two_runs_give_equal_bits(torch_mod, fixture, monkeypatch):
    from wtracker_amd.replay import YoloReplay

    fx = fixture
    plan_env(monkeypatch)
    yr = YoloReplay(fx["dev_frames"], fx["tc"], fx["ec"], config(fx, ry.FIXTURE_CONFS[1]))
    a = yr.run()
    det_a = a.detections.cpu().numpy().copy()
    b = yr.run()
    assert a.moves.tobytes() == b.moves.tobytes() and a.positions.tobytes() == b.positions.tobytes()
    assert a.row_array(0).tobytes() == b.row_array(0).tobytes() and det_a.tobytes() == b.detections.cpu().numpy().tobytes()
    assert a.detections.cpu().numpy().tobytes() == det_a.tobytes()  # the first result's detections are its own copy
    assert_summary_equal(a.summary, b.summary)
    assert np.isnan(det_a).any() and not np.isnan(det_a).all()
