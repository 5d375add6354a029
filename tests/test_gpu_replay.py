"""wtracker_amd.replay on the MI355X: the closed loop of track-driven experiments (csrc/replay.hip) against the real reference's fixtures, the pinned
numpy restatement (tests/harness/replay_ref.py) and the host frame loop (tests/harness/sim_harness.py)."""
import csv
import json
import math
import os
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from harness import replay_ref as rr  # noqa: E402
from harness.sim_harness import Simulator  # noqa: E402
from wtracker_amd import hip, resmlp  # noqa: E402
from wtracker_amd.controllers import PolyfitConfig, PolyfitController, _read_track_csv  # noqa: E402
from wtracker_amd.sim import LOG_COLUMNS, ExperimentConfig, TimingConfig, TrackLogger  # noqa: E402

EXP0 = dict(name="exp0", num_frames=200, frames_per_sec=60, orig_resolution=(1600, 1400), px_per_mm=90, init_position=(1300, 1200))
POLY0 = dict(degree=2, sample_times=[-9, -6, -3, 0, 2, 4], weights=[1, 1, 2, 3, 4, 5])
NUM_KEYS = LOG_COLUMNS[3:]


@pytest.fixture(scope="module")
def torch_mod(hip_lib):
    import torch

    if hip.device_count() < 1:
        pytest.fail("no HIP device visible")
    return torch


def make_replay(golden_dir, timing):
    from wtracker_amd.replay import Replay

    ec = ExperimentConfig(**EXP0)
    tc = TimingConfig(ec, *timing, (4, 4), (0.32, 0.32))
    return Replay(os.path.join(golden_dir, "sim_init_bboxes.csv"), tc, ec), tc, ec


def moves_of(res, e=0):
    return [[int(f), int(m[0]), int(m[1])] for f, m in zip(res.decision_frames, res.moves[e])]


def assert_log_equals_csv(rows, path):
    with open(path, newline="") as f:
        gold = list(csv.DictReader(f))
    assert len(rows) == len(gold)
    for r, g in zip(rows, gold):
        assert r["frame"] == int(g["frame"]) and r["cycle"] == int(g["cycle"]) and r["phase"] == g["phase"]
        for k in NUM_KEYS:
            assert float(r[k]) == float(g[k]), (k, r["frame"], r[k], g[k])


def assert_rows_equal_ref(res, e, ref):
    assert np.array_equal(res.row_array(e), ref["rows"])


# ------------------------------------------------------------------------------------------------- goldens
def test_golden_replays_at_cycle_9_match_the_reference(torch_mod, golden_dir):
    """All four kinds at (100, 40, 50) ms, L = 9: every move the real reference recorded and every column of its logs."""
    rp, tc, ec = make_replay(golden_dir, (100, 40, 50))
    assert (rp.L, rp.n_cycles, rp.n_rows) == (9, 22, 198)
    gold = json.load(open(os.path.join(golden_dir, "sim_moves.json")))
    res = rp.run(rp.csv())
    assert moves_of(res) == gold["sim_csv_bboxes.csv"]
    assert_log_equals_csv(res.log(0), os.path.join(golden_dir, "sim_csv_bboxes.csv"))
    res = rp.run(rp.mlp(resmlp.load_npz(os.path.join(golden_dir, "resmlp_100ms.npz")), max_speed=0.9))
    assert moves_of(res) == gold["sim_mlp_bboxes.csv"]
    assert_log_equals_csv(res.log(0), os.path.join(golden_dir, "sim_mlp_bboxes.csv"))
    assert moves_of(rp.run(rp.optimal())) == gold["sim_optimal"]
    cases = {"sim_polyfit": dict(config=POLY0, moves=gold["sim_polyfit"])}
    for fixture in ("polyfit_cases.json", "polyfit_highdeg.json"):
        cases.update(json.load(open(os.path.join(golden_dir, fixture))))
    names = sorted(cases)
    res = rp.run(rp.polyfit([PolyfitConfig(**cases[n]["config"]) for n in names]), rows=[])
    for e, n in enumerate(names):
        assert moves_of(res, e) == cases[n]["moves"], n


def test_golden_replays_at_cycle_15_match_the_reference(torch_mod, golden_dir):
    """(200, 40, 50) ms, L = 15: the reference's MLP log and moves; the CSV, Optimal and Polyfit replays against the pinned numpy restatement (the
    reference wrote no fixture for them at this timing)."""
    rp, tc, ec = make_replay(golden_dir, (200, 40, 50))
    assert rp.L == 15
    gold = json.load(open(os.path.join(golden_dir, "sim_moves.json")))
    res = rp.run(rp.mlp(resmlp.load_npz(os.path.join(golden_dir, "resmlp_200ms.npz")), max_speed=0.9))
    assert moves_of(res) == gold["sim_mlp200_bboxes.csv"]
    assert_log_equals_csv(res.log(0), os.path.join(golden_dir, "sim_mlp200_bboxes.csv"))
    g, track = rr.Geometry.of(tc, ec), _read_track_csv(os.path.join(golden_dir, "sim_init_bboxes.csv"))
    a, v = rr.targets_optimal(g, track)
    pa, pv = rr.targets_polyfit(g, track, **POLY0)
    for tg, (kind, ra, rv) in ((rp.csv(), (rr.CSV, None, None)), (rp.optimal(), (rr.OPTIMAL, a[:, None], v[:, None])),
                               (rp.polyfit([PolyfitConfig(**POLY0)]), (rr.POLYFIT, pa[:, None], pv[:, None]))):
        res = rp.run(tg)
        pos, move = rr.scan(kind, g, track, ra, None, rv)
        assert np.array_equal(res.moves[0], move[:, 0]) and np.array_equal(res.positions[0], pos[:, 0])
        assert_rows_equal_ref(res, 0, rr.rows(g, track, pos, move, summaries=False))


# ------------------------------------------------------------------------------------------------- the hard fixture
@pytest.fixture(scope="module")
def hard(golden_dir):
    z = np.load(os.path.join(golden_dir, "replay_hard.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    ec = ExperimentConfig("hard", meta["num_frames"], meta["frames_per_sec"], tuple(meta["orig_resolution"]), meta["px_per_mm"], tuple(meta["init_position"]))
    return dict(z=z, meta=meta, ec=ec, track=z["track"])


def hard_replay(hard, imaging):
    from wtracker_amd.replay import Replay

    tc = TimingConfig(hard["ec"], imaging, 40, 50, hard["meta"]["camera_size_mm"], hard["meta"]["micro_size_mm"])
    return Replay(hard["track"], tc, hard["ec"]), tc


def assert_equals_hard_run(hard, res, e, key, geo):
    z = hard["z"]
    assert moves_of(res, e) == z[key + "/moves"].tolist(), key
    r = res.row_array(e)
    assert np.array_equal(r[:, 0:2], z[key + "/plt"]) and np.array_equal(r[:, 2:4], z[key + "/cam"]) and np.array_equal(r[:, 6:8], z[key + "/mic"]), key
    assert (r[:, 4:6] == geo["camera_size_px"]).all() and (r[:, 8:10] == geo["micro_size_px"]).all()
    assert np.array_equal(r[:, 10:14], z[key + "/wrm"]) and np.array_equal(r[:, 14], z[key + "/cycle"]) and np.array_equal(r[:, 15], z[key + "/phase"]), key
    L = geo["L"]
    assert np.array_equal(res.positions[e][: len(r) // L], z[key + "/plt"][::L]), key  # the position at every logged cycle's start
    # float64 + - * / only, no contraction: bit-equal to ErrorCalculator.calculate_bbox_error / calculate_mse_error of the reference's log
    assert res.bbox_error[e].tobytes() == z[key + "/bbox_error"].tobytes(), key
    assert res.mse_error[e].tobytes() == z[key + "/mse_error"].tobytes(), key


@pytest.mark.parametrize("imaging", [100, 200])
def test_hard_fixture_every_row_move_and_error_equals_the_reference(torch_mod, hard, imaging):
    rp, tc = hard_replay(hard, imaging)
    geo = hard["meta"]["geometry"][str(imaging)]
    assert (rp.L, rp.I, rp.M, rp.P) == (geo["L"], geo["I"], geo["M"], geo["P"])
    assert_equals_hard_run(hard, rp.run(rp.csv(), per_row_errors=True), 0, f"csv_{imaging}", geo)
    assert_equals_hard_run(hard, rp.run(rp.optimal(), per_row_errors=True), 0, f"optimal_{imaging}", geo)
    cfgs = [PolyfitConfig(**kw) for kw in hard["meta"]["polyfit_configs"]]
    res = rp.run(rp.polyfit(cfgs), rows=range(len(cfgs)), per_row_errors=True)
    for e in range(len(cfgs)):
        assert_equals_hard_run(hard, res, e, f"polyfit{e}_{imaging}", geo)


# ------------------------------------------------------------------------------------------------- population
POP, CHECKED = 70, (0, 63, 64, 69)  # one more than a wave and then some: experiments on both sides of the wave boundary


@pytest.fixture(scope="module")
def population(torch_mod, hard):
    rp, tc = hard_replay(hard, 100)
    rng = np.random.default_rng(7)
    weights = rng.uniform(0.05, 1.0, size=(POP, 6))
    cfgs = [PolyfitConfig(2, [-8, -6, -4, -2, 0, 1], [float(v) for v in w]) for w in weights]
    res = rp.run(rp.polyfit(cfgs), rows=CHECKED, per_row_errors=True)
    return dict(rp=rp, tc=tc, cfgs=cfgs, res=res)


def test_population_members_equal_the_host_frame_loop(population, hard, tmp_path):
    """Experiments 0, 63, 64 and 69 of 70: row for row what Simulator + TrackLogger + PolyfitController (host, numpy's polyfit) log."""
    path = tmp_path / "hard.csv"
    with open(path, "w") as f:
        f.write("frame,wrm_x,wrm_y,wrm_w,wrm_h\n")
        for i, r in enumerate(hard["track"]):
            f.write(f"{i}," + ",".join("" if not np.isfinite(v) else repr(float(v)) for v in r) + "\n")
    res = population["res"]
    assert len({res.moves[e].tobytes() for e in range(POP)}) > POP // 2  # the weights matter: the experiments differ
    for e in CHECKED:
        ctrl = PolyfitController(population["tc"], population["cfgs"][e], str(path))
        ctrl.track = hard["track"].copy()  # the fixture's own float64 values (the CSV parser is not round-trip exact)
        ctrl._table = np.vstack([ctrl.track, np.full((1, 4), np.nan)])
        log = TrackLogger(ctrl)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # numpy's RankWarning in the first cycles
            Simulator(population["tc"], hard["ec"], log).run()
        mine = res.log(e)
        assert len(mine) == len(log.rows) == population["rp"].n_rows
        for a, b in zip(mine, log.rows):
            assert a["frame"] == b["frame"] and a["cycle"] == b["cycle"] and a["phase"] == b["phase"]
            for k in NUM_KEYS:
                assert float(a[k]) == float(b[k]), (e, k, a["frame"], a[k], b[k])


def test_an_experiment_alone_gives_the_bits_it_gives_in_the_population(population):
    rp, res = population["rp"], population["res"]
    s = res.summary
    for e in CHECKED:
        one = rp.run(rp.polyfit([population["cfgs"][e]]), rows=[0], per_row_errors=True)
        assert np.array_equal(one.moves[0], res.moves[e]) and np.array_equal(one.positions[0], res.positions[e])
        assert one.bbox_error[0].tobytes() == res.bbox_error[e].tobytes() and one.mse_error[0].tobytes() == res.mse_error[e].tobytes()
        for name in ("bbox_error_sum", "rows", "trimmed_bbox_error_sum", "trimmed_rows", "non_perfect_rows", "mse_error_sum"):
            assert getattr(one.summary, name)[0].tobytes() == getattr(s, name)[e].tobytes(), (e, name)


def test_summaries_against_the_devices_own_rows(population):
    """Sums within the tree reduction's bound ceil(log2 R) * 2^-53 * sum |x| of math.fsum over the device's per-row values; counts exact."""
    rp, res = population["rp"], population["res"]
    R, s = rp.n_rows, res.summary
    depth = math.ceil(math.log2(R))
    r0 = np.arange(R)
    trimmed = (r0 % rp.L < rp.I) & (r0 // rp.L != 0) & (r0 // rp.L != rp.n_log - 1)
    assert 0 < trimmed.sum() < R
    for e in range(POP):
        err, mse = res.bbox_error[e], res.mse_error[e]
        for got, x in ((s.bbox_error_sum[e], err), (s.trimmed_bbox_error_sum[e], err[trimmed]), (s.mse_error_sum[e], mse)):
            assert abs(got - math.fsum(x)) <= depth * 2.0 ** -53 * math.fsum(np.abs(x)), e
        assert s.rows[e] == R and s.trimmed_rows[e] == trimmed.sum() and s.non_perfect_rows[e] == (err > 1e-7).sum()
    assert (s.non_perfect_rows > 0).all() and np.allclose(s.mean_bbox_error, res.bbox_error.mean(axis=1), rtol=1e-12)


def test_summary_sums_have_the_fixed_orders_bits_across_chunks(torch_mod):
    """R = 915 x 9 = 8235 = 2 x 4096 + 43 rows (harness long_track, seed 77; the Polyfit pair of test_gpu_replay_analysis.py's long run): two full chunks
    and a ragged one per experiment, so the finish launch adds three partials.  The three sums are the BYTES of replay_ref._tree_sum, the statement of
    the kernel's order, over the device's own per-row arrays; the counts are exact.  tests/test_replay_ref.py shows that on this track a sum changes
    its bits when the chunk is halved, so another order does not pass here."""
    from wtracker_amd.replay import Replay

    ec = ExperimentConfig("long", 8236, 60, (1600, 1400), 90, (700, 600))
    tc = TimingConfig(ec, 100, 40, 50, (4, 4), (0.32, 0.32))
    rp = Replay(rr.long_track(8236, 3), tc, ec)
    assert (rp.L, rp.n_rows) == (9, 8235)
    tg = rp.polyfit([PolyfitConfig(1, [-5, -3, -1, 0, 1], None), PolyfitConfig(2, [-8, -6, -4, -2, 0, 1], [1, 1, 2, 3, 4, 5])])
    res = rp.run(tg, per_row_errors=True)
    R, s = rp.n_rows, res.summary
    r0 = np.arange(R)
    trimmed = (r0 % rp.L < rp.I) & (r0 // rp.L != 0) & (r0 // rp.L != rp.n_log - 1)  # as replay_ref.rows masks the trimmed sum
    for e in range(2):
        err, mse = np.asarray(res.bbox_error[e]), np.asarray(res.mse_error[e])
        for name, x in (("bbox_error_sum", err), ("trimmed_bbox_error_sum", np.where(trimmed, err, 0.0)), ("mse_error_sum", mse)):
            got, want = float(getattr(s, name)[e]), rr._tree_sum(x)
            print(e, name, got.hex(), want.hex())
            assert np.float64(got).tobytes() == np.float64(want).tobytes(), (e, name)
        assert s.rows[e] == R and s.trimmed_rows[e] == trimmed.sum() and s.non_perfect_rows[e] == (err > 1e-7).sum()
        assert 0 < s.non_perfect_rows[e] < R


# ------------------------------------------------------------------------------------------------- refusals
def test_refusals_touch_no_memory(torch_mod, hard):
    torch = torch_mod
    dev = torch.device("cuda", 0)
    track = torch.from_numpy(hard["track"]).to(dev)
    N, E = int(track.shape[0]), 3
    good = dict(num_frames=400, imaging_frame_num=3, moving_frame_num=2, pred_frame_num=2, camera_size=(360, 360), micro_size=(29, 29), frame_wh=(1760, 1960),
                init_position=(22, 14))
    Cn, R = (400 - 1 - 3) // 5 + 1, (400 - 1) // 5 * 5
    share = torch.from_numpy(rr.share_table(2)).to(dev)
    a = torch.zeros((Cn, E, 2), dtype=torch.float64, device=dev)
    valid = torch.ones((Cn, E), dtype=torch.int32, device=dev)
    SENT_I, SENT_F = -77, -12345.5
    pos = torch.full((Cn, E, 2), SENT_I, dtype=torch.int32, device=dev)
    move = torch.full((Cn, E, 2), SENT_I, dtype=torch.int32, device=dev)
    outs = dict(rows=torch.full((1, R, 16), SENT_F, dtype=torch.float64, device=dev), bbox=torch.full((E, R), SENT_F, dtype=torch.float64, device=dev),
                mse=torch.full((E, R), SENT_F, dtype=torch.float64, device=dev), summary=torch.full((E, 6), SENT_F, dtype=torch.float64, device=dev),
                scratch=torch.full((hip.replay_scratch_doubles(E, R),), SENT_F, dtype=torch.float64, device=dev))
    slots = torch.tensor([0, -1, -1], dtype=torch.int32, device=dev)

    def scan(cfg=None, kind=hip.REPLAY_POLYFIT, E_=E, n_track=N, **over):
        p = dict(track=track, a=a, valid=valid, share=share, pos=pos, move=move)
        p.update(over)
        hip.replay_scan(hip.replay_config(**{**good, **(cfg or {})}), kind, E_, Cn, p["track"], n_track, p["a"], None, p["valid"], p["share"], p["pos"], p["move"])

    def rows(cfg=None, E_=E, n_track=N, **over):
        p = dict(track=track, share=share, pos=pos, move=move, summary=outs["summary"], scratch=outs["scratch"])
        p.update(over)
        hip.replay_rows(hip.replay_config(**{**good, **(cfg or {})}), E_, Cn, p["track"], n_track, p["share"], p["pos"], p["move"], slots, 1, outs["rows"],
                        outs["bbox"], outs["mse"], p["summary"], p["scratch"], outs["scratch"].numel())

    bad_cfgs = [dict(moving_frame_num=0), dict(pred_frame_num=4), dict(camera_size=(28, 360)), dict(camera_size=(360, 28)), dict(num_frames=10 ** 6)]
    for call in (scan, rows):
        for cfg in bad_cfgs:  # M < 1, P > I, camera smaller than the microscope (either axis), a track shorter than the logged rows
            with pytest.raises(hip.WtkError):
                call(cfg)
        with pytest.raises(hip.WtkError):
            call(E_=0)
        with pytest.raises(hip.WtkError):
            call(n_track=R - 1)  # the track is shorter than the logged rows
        for name in ("track", "share", "pos", "move"):
            with pytest.raises(hip.WtkError):
                call(**{name: None})
    with pytest.raises(hip.WtkError):
        scan(dict(pred_frame_num=0), kind=hip.REPLAY_CSV)  # P < 1 for the CSV kind
    for name in ("a", "valid"):
        with pytest.raises(hip.WtkError):
            scan(**{name: None})
    with pytest.raises(hip.WtkError):
        hip.replay_scan(hip.replay_config(**good), hip.REPLAY_MLP, E, Cn, track, N, a, None, valid, share, pos, move)  # MLP without its origins
    for name in ("summary", "scratch"):
        with pytest.raises(hip.WtkError):
            rows(**{name: None})
    with pytest.raises(hip.WtkError):
        hip.replay_scan(None, hip.REPLAY_POLYFIT, E, Cn, track, N, a, None, valid, share, pos, move)
    torch.cuda.synchronize()
    assert (pos == SENT_I).all() and (move == SENT_I).all()
    for t in outs.values():
        assert (t == SENT_F).all()
    scan()  # and the good call goes through
    rows()
    torch.cuda.synchronize()
    assert (pos != SENT_I).any() and (outs["summary"] != SENT_F).all() and (outs["bbox"] != SENT_F).all()


# ------------------------------------------------------------------------------------------------- hand-off
def test_csv_hands_off_to_the_precise_error(torch_mod, golden_dir, tmp_path):
    from wtracker_amd import evaluation

    torch = torch_mod
    rp, tc, ec = make_replay(golden_dir, (100, 40, 50))
    res = rp.run(rp.polyfit([PolyfitConfig(**POLY0)]))
    path = tmp_path / "bboxes.csv"
    res.to_csv(0, str(path))
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    assert list(rows[0].keys()) == LOG_COLUMNS and len(rows) == rp.n_rows
    H, W = rp.frame_shape
    frames = torch.full((ec.num_frames, H, W), 255, dtype=torch.uint8, device="cuda")
    err = evaluation.precise_error_from_log(str(path), frames, torch.full((H, W), 255, dtype=torch.uint8, device="cuda"))
    err = err.cpu().numpy()
    assert err.shape == (rp.n_rows,) and (err[np.isfinite(err)] == 0).all()  # blank frames: no foreground pixel anywhere
