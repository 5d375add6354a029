"""DataAnalyzer's statistics of a replayed population on the MI355X (csrc/replay_analysis.hip) against tests/golden/analysis.npz (the
real reference's DataAnalyzer and pandas on the logs of replay_hard.npz) and against the numpy restatement tests/harness/analysis_ref.py, which
tests/test_analysis_ref.py pins to that fixture.  The comparison rules are that file's (assert_same_analysis): order statistics, counts, maxima, masks and
the print_stats figures equal as float64 values (-0.0 == 0.0, NaN matches NaN); means within n 2^-52 mean|x|, standard deviations within n 2^-52
relative.  The device's float64 sqrt and division are the correctly rounded ones: no tolerance is spent on them.

On the parent commit `Replay.run` has no `analysis` argument: every test here fails there."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from harness import analysis_ref as ar  # noqa: E402
from harness import replay_precise_ref as pr  # noqa: E402
from harness import replay_ref as rr  # noqa: E402
from harness import replay_yolo_ref as ry  # noqa: E402
from test_analysis_ref import assert_same_analysis, golden_of, same, spec_of  # noqa: E402
from wtracker_amd import frames as fr  # noqa: E402
from wtracker_amd import hip  # noqa: E402
from wtracker_amd import yolo_spec as ys  # noqa: E402
from wtracker_amd.controllers import PolyfitConfig, YoloConfig  # noqa: E402
from wtracker_amd.sim import ExperimentConfig, TimingConfig  # noqa: E402

ARRAYS = ("describe", "cycle_max", "cycle_mean", "step_quantiles", "step_count", "anomaly_counts", "stats", "anomaly_mask")
LDS_ROWS = (0, 64, 7, 1000)  # the default (every segment sorted in LDS), two limits below every segment (radix select), one between the two segment kinds


@pytest.fixture(scope="module")
def torch_mod(hip_lib):
    import torch

    if hip.device_count() < 1:
        pytest.fail("no HIP device visible")
    return torch


def analysis_of(spec: ar.Spec, unit="frame", mask=True):
    """The product's Analysis of a harness Spec."""
    from wtracker_amd.replay import Analysis

    assert spec.min_width == spec.min_height
    return Analysis(period=spec.period, trim_cycles=spec.trim_cycles, imaging_only=spec.imaging_only, bounds=spec.bounds, unit=unit,
                    columns=list(spec.columns), percentiles=list(spec.percentiles), no_preds=spec.no_preds, min_bbox_error=spec.min_bbox_error,
                    min_dist_error=spec.min_dist_error, min_speed=spec.min_speed, min_size=spec.min_width, anomaly_mask=mask)


def device_dict(a, e: int) -> dict:
    return {n: (None if getattr(a, n) is None else np.asarray(getattr(a, n)[e])) for n in ARRAYS}


def assert_bits_equal(a, ea, b, eb, what=""):
    """Experiment ea of AnalysisResult a and experiment eb of b hold the same bits in every array."""
    for n in ARRAYS:
        x, y = getattr(a, n), getattr(b, n)
        assert (x is None) == (y is None)
        if x is not None:
            assert np.ascontiguousarray(x[ea]).tobytes() == np.ascontiguousarray(y[eb]).tobytes(), (what, n)


def assert_equals_harness(res, e, L, spec: ar.Spec, what="", precise=None):
    rows16 = res.row_array(e)
    want = ar.analyze(rows16, L, spec, precise)
    cols = [ar.COL[c] for c in spec.columns]
    assert_same_analysis(device_dict(res.analysis, e), want, ar.to_unit(want["table"], spec.factors)[:, cols], want["keep"], L, what)
    return want


# ------------------------------------------------------------------------------------------------- the reference's fixture
@pytest.fixture(scope="module")
def gold(golden_dir):
    z = np.load(os.path.join(golden_dir, "analysis.npz"))
    hard = np.load(os.path.join(golden_dir, "replay_hard.npz"))
    hm = json.loads(bytes(hard["meta"]).decode())
    ec = ExperimentConfig("hard", hm["num_frames"], hm["frames_per_sec"], tuple(hm["orig_resolution"]), hm["px_per_mm"], tuple(hm["init_position"]))
    return dict(z=z, hard=hard, meta=json.loads(bytes(z["meta"]).decode()), hm=hm, ec=ec)


def hard_replay(gold, imaging):
    from wtracker_amd.replay import Replay

    tc = TimingConfig(gold["ec"], imaging, 40, 50, gold["hm"]["camera_size_mm"], gold["hm"]["micro_size_mm"])
    return Replay(gold["hard"]["track"], tc, gold["ec"]), tc


@pytest.mark.parametrize("imaging", [100, 200])
def test_golden_populations_equal_the_reference_and_the_harness(torch_mod, gold, imaging):
    """csv, optimal and the four polyfit configs (one population) at both timings, configurations a, b, c0 and c1 of the fixture, all 29 columns and six
    percentiles: against the reference's own numbers where the fixture holds the run, against the harness on the replayed rows for every experiment."""
    rp, tc = hard_replay(gold, imaging)
    z, meta = gold["z"], gold["meta"]
    pops = {"csv": rp.csv(), "optimal": rp.optimal(), "polyfit": rp.polyfit([PolyfitConfig(**kw) for kw in gold["hm"]["polyfit_configs"]])}
    checked = 0
    for cname, cfg in meta["configs"].items():
        for kind, tg in pops.items():
            names = [f"polyfit{k}_{imaging}" for k in range(4)] if kind == "polyfit" else [f"{kind}_{imaging}"]
            spec = spec_of(meta, cname, names[0])
            res = rp.run(tg, rows=range(tg.E), analysis=analysis_of(spec, cfg["unit"]))
            a = res.analysis
            assert a.describe.shape == (tg.E, 29, 11) and a.step_quantiles.shape == (tg.E, rp.L, 29, 6) and a.anomaly_mask.shape == (tg.E, rp.n_rows)
            for e, run in enumerate(names):
                want = assert_equals_harness(res, e, rp.L, spec, f"{cname}/{run} vs harness")
                if run in meta["runs"]:
                    cols = [ar.COL[c] for c in spec.columns]
                    key = f"{cname}/{run}/"
                    assert np.array_equal(want["keep"], z[key + "keep"])
                    assert_same_analysis(device_dict(a, e), golden_of(z, key), ar.to_unit(want["table"], spec.factors)[:, cols], want["keep"], rp.L,
                                         key + " vs the reference")
                    checked += 1
    assert checked == (24 if imaging == 100 else 4)


def test_describe_table_and_print_stats(torch_mod, gold, capsys):
    rp, tc = hard_replay(gold, 100)
    spec = spec_of(gold["meta"], "a", "csv_100")
    res = rp.run(rp.csv(), analysis=analysis_of(spec))
    index, columns, values = res.analysis.describe_table(0)
    assert index == ["count", "mean", "std", "min", "5%", "25%", "50%", "75%", "95%", "99%", "max"] and columns == list(spec.columns)
    assert values.shape == (11, 29) and same(values[0], gold["z"]["a/csv_100/describe"][:, 0])
    res.analysis.print_stats(0)
    out = capsys.readouterr().out.splitlines()
    assert out == ["Count of Removed Frames: 275 (69.62%)", "Count of No-Pred Frames: 0 (0.0%)", "Total Num of Cycles: 40", "Non Perfect Predictions: 97.5%"]


# ------------------------------------------------------------------------------------------------- the precise_error column
def test_precise_error_column_is_the_unrounded_per_pair_error(torch_mod):
    """The scenario of tests/test_gpu_replay_precise.py (96 x 131 frames, 70 experiments, R = 120): the precise_error column's statistics equal the harness
    applied to res.precise_error, which is NOT rounded to five decimals (the reference assigns the column after its rounding)."""
    from wtracker_amd.replay import Replay, Targets

    torch, sc = torch_mod, pr.scenario_main()
    g = sc["g"]
    ec = ExperimentConfig("scenario", g.num_frames, 1000, sc["frame_shape"], 1, g.init)
    tc = TimingConfig(ec, g.I, g.P, g.M, g.cam, g.mic)
    rp = Replay(torch.from_numpy(sc["track"]), tc, ec, frame_shape=sc["frame_shape"])
    rp.attach_frames(torch.from_numpy(sc["frames"]).cuda(), sc["bg"], 20)
    tg = Targets("optimal", sc["a"].shape[1], torch.from_numpy(np.ascontiguousarray(sc["a"])).cuda(), None, torch.from_numpy(np.ascontiguousarray(sc["valid"])).cuda())
    checked = (0, 63, 64, 69)
    spec = ar.Spec(period=3, trim_cycles=True, imaging_only=True, columns=("precise_error", "bbox_error", "wrm_speed"), percentiles=(0.1, 0.5, 0.9),
                   min_bbox_error=0.25)
    with pytest.raises(ValueError, match="precise"):
        rp.run(tg, analysis=analysis_of(spec))
    res = rp.run(tg, rows=checked, per_row_errors=True, precise=True, analysis=analysis_of(spec))
    unrounded = 0
    for e in checked:
        perr = res.precise_error[e]
        assert_equals_harness(res, e, rp.L, spec, f"e = {e}", precise=perr)
        unrounded += int((ar.round5(perr) != perr)[~np.isnan(perr)].sum())
        assert res.analysis.describe[e, 0, 0] == float((~np.isnan(perr) & ar.keep_mask(ar.table(res.row_array(e), rp.L, 3), res.row_array(e)[:, 15], spec)).sum())
    assert unrounded > 0  # the column would change under the rounding: that it does not is what is checked


# ------------------------------------------------------------------------------------------------- determinism
def test_an_experiment_gives_the_same_bits_in_any_population(torch_mod, gold):
    rp, tc = hard_replay(gold, 100)
    cfgs = [PolyfitConfig(**kw) for kw in gold["hm"]["polyfit_configs"]]
    cfgs += [PolyfitConfig(1, [-4, -2, 0, 1], [1, 2, 3, 4]), PolyfitConfig(2, [-6, -4, -2, 0, 1], None)]
    spec = spec_of(gold["meta"], "a", "csv_100")
    ana = analysis_of(spec)
    six = rp.run(rp.polyfit(cfgs), rows=[], analysis=ana).analysis
    rev = rp.run(rp.polyfit(cfgs[::-1]), rows=[], analysis=ana).analysis
    assert len({six.describe[e].tobytes() for e in range(6)}) > 1  # the experiments differ
    for k in range(6):
        alone = rp.run(rp.polyfit([cfgs[k]]), rows=[], analysis=ana).analysis
        assert_bits_equal(six, k, alone, 0, f"experiment {k} alone")
        assert_bits_equal(six, k, rev, 5 - k, f"experiment {k} reversed")
    # Replay.analyze: the same arrays as device tensors, nothing waited for
    dev = rp.analyze(rp.polyfit(cfgs), ana)
    assert dev.describe.is_cuda and dev.stats.is_cuda
    torch_mod.cuda.synchronize()
    from wtracker_amd.replay import _analysis_to_host

    host = _analysis_to_host(dev)
    for k in range(6):
        assert_bits_equal(six, k, host, k, "Replay.analyze")


@pytest.fixture(scope="module")
def long_run(torch_mod):
    """R = 915 x 9 = 8235 = 2 x 4096 + 43 rows (R is a multiple of the cycle length, so 2 x 4096 + 37 cannot be had at L = 9; 8235 also crosses the rows
    kernel's 4096-row chunk twice and is no power of two), three experiments, once per `_max_lds_rows`.  Computed once, never modified."""
    from wtracker_amd.replay import Replay

    ec = ExperimentConfig("long", 8236, 60, (1600, 1400), 90, (700, 600))
    tc = TimingConfig(ec, 100, 40, 50, (4, 4), (0.32, 0.32))
    rp = Replay(rr.long_track(8236, 3), tc, ec)
    assert (rp.L, rp.n_rows) == (9, 8235)
    spec = ar.Spec(period=3, trim_cycles=True, imaging_only=False, bounds=(380, 380, 1020, 1020), columns=("wrm_speed_x", "wrm_speed", "worm_deviation_x",
                   "bbox_error", "wrm_w", "cycle_step"), percentiles=(0.0, 0.05, 0.5, 0.95, 0.999, 1.0), min_speed=4.0, min_bbox_error=0.5,
                   min_dist_error=10.0, min_width=14.5, min_height=14.5)
    tg = rp.polyfit([PolyfitConfig(1, [-5, -3, -1, 0, 1], None), PolyfitConfig(2, [-8, -6, -4, -2, 0, 1], [1, 1, 2, 3, 4, 5])])
    runs = {m: rp.run(tg, rows=[0, 1], analysis=analysis_of(spec), _max_lds_rows=m) for m in LDS_ROWS}
    return dict(rp=rp, spec=spec, runs=runs)


def test_results_do_not_depend_on_the_lds_limit(long_run):
    rp, spec, runs = long_run["rp"], long_run["spec"], long_run["runs"]
    for e in range(2):
        want = assert_equals_harness(runs[0], e, rp.L, spec, f"long run, e = {e}")
        tab = want["table"][want["keep"]]
        sx = tab[:, ar.COL["wrm_speed_x"]]
        assert np.isnan(want["table"][:3, ar.COL["wrm_speed"]]).all()  # NaN speed rows are there (and are kept: cycle 0 is trimmed, so look at the table)
        assert (np.signbit(sx) & (sx == 0)).any() and (~np.signbit(sx) & (sx == 0)).any()  # -0.0 and +0.0
        assert len(np.unique(tab[:, ar.COL["wrm_w"]])) < len(tab) // 50  # duplicates
        assert want["keep"].sum() > 4096 and not want["keep"].all()
        for m in LDS_ROWS[1:]:
            assert_bits_equal(runs[0].analysis, e, runs[m].analysis, e, f"_max_lds_rows = {m}, e = {e}")


def test_nan_rows_of_the_speed_column_are_skipped(long_run, torch_mod):
    """Without trim_cycles the first `period` rows are kept and their speed is NaN: they are counted by no statistic of the speed columns."""
    rp = long_run["rp"]
    spec = ar.Spec(period=7, columns=("wrm_speed", "wrm_speed_y", "frame"), percentiles=(0.5,))
    for m in (0, 64):
        res = rp.run(rp.csv(), analysis=analysis_of(spec), _max_lds_rows=m)
        assert res.analysis.describe[0, :, 0].tolist() == [8235 - 7, 8235 - 7, 8235]
        assert_equals_harness(res, 0, rp.L, spec, f"period 7, _max_lds_rows = {m}")


# ------------------------------------------------------------------------------------------------- segment sizes
@pytest.mark.parametrize("K", [0, 1, 2, 3, 63, 64, 65])
def test_segment_edge_sizes(torch_mod, K):
    """K kept rows in the whole-experiment segment (K in cycle step 0, or 64 there and one in step 1), every other segment empty; n_log = 64, so at
    `_max_lds_rows` = 64 a cycle step's segment fills the LDS buffer exactly while the whole experiment goes through the select."""
    from wtracker_amd.replay import Replay

    L, n_log = 9, 64
    R = L * n_log
    rank = np.concatenate([np.arange(n_log) * L, np.arange(n_log) * L + 1])  # the rows in the order they become kept
    rng = np.random.default_rng(3)
    track = np.empty((R + 1, 4))
    r = np.arange(R + 1)
    # (values spread so that |mean| / std stays far below 100 in every segment of two or more rows: the comparison's bound needs that)
    track[:, 0], track[:, 1], track[:, 2], track[:, 3] = 700.0 + 150.0 * (r % 4), 2.0, 10.0, 4.0 + 3.0 * (r % 5) + np.round(rng.uniform(0, 0.9, R + 1), 2)
    track[rank[:70], 0] = 50.0 + 2.0 * np.arange(70) + np.round(rng.uniform(0, 1, 70), 3)
    # y in [0, 21]: the 29-pixel microscope box never fits, so only the worm box decides; x up to the K-th kept row's right edge
    bounds = (40.0, 0.0, 50.0 + 2.0 * (K - 1) + 1.0 + 10.0 if K else 45.0, 21.0)
    ec = ExperimentConfig("edges", R + 1, 60, (1600, 1400), 90, (300, 200))
    tc = TimingConfig(ec, 100, 40, 50, (4, 4), (0.32, 0.32))
    rp = Replay(track, tc, ec)
    assert (rp.L, rp.n_rows) == (L, R)
    spec = ar.Spec(period=2, bounds=bounds, columns=("wrm_x", "wrm_h", "bbox_error", "wrm_speed_x"), percentiles=(0.0, 0.3, 0.5, 0.99, 1.0), min_bbox_error=0.5)
    base = None
    for m in (0, 64):
        res = rp.run(rp.csv(), analysis=analysis_of(spec), _max_lds_rows=m)
        want = assert_equals_harness(res, 0, L, spec, f"K = {K}, _max_lds_rows = {m}")
        assert int(want["keep"].sum()) == K and res.analysis.describe[0, 0, 0] == K
        assert res.analysis.step_count[0, :, 0].tolist() == [min(K, 64), max(K - 64, 0)] + [0] * 7
        if base is None:
            base = res.analysis
        else:
            assert_bits_equal(base, 0, res.analysis, 0, f"K = {K}")


# ------------------------------------------------------------------------------------------------- YoloReplay
def test_yolo_replay_analysis_equals_the_harness(torch_mod, tmp_path, monkeypatch):
    from wtracker_amd.replay import YoloReplay

    for v in ("WTK_LATENCY_PLAN", "WTK_NO_SK_MIXED", "WTK_SMALL_NARROW"):
        monkeypatch.delenv(v, raising=False)
    path = str(tmp_path / "s.wtk")
    ys.save_weights(path, ys.synthetic_weights("s", 1, seed=0), "s", 1)
    frames, _ = fr.synthetic_frames(40, 256, seed=8)
    ec = ExperimentConfig("synthetic", 40, 60, (256, 256), 32, ry.FIXTURE_INIT)
    tc = TimingConfig(ec, 100, 40, 50, (4, 4), (0.5, 0.5))
    cfg = YoloConfig(model_path=path, device="cuda", pred_kwargs={"imgsz": 128, "conf": ry.FIXTURE_CONFS[1]}, dtype="f16x3", scale="s", plan="auto")
    yr = YoloReplay(torch_mod.from_numpy(frames).cuda(), tc, ec, cfg)
    spec = ar.Spec(period=2, imaging_only=True, columns=("wrm_speed", "worm_deviation", "bbox_error", "wrm_w"), percentiles=(0.25, 0.5, 0.75),
                   factors=ar.sec_factors(tc.mm_per_px, tc.ms_per_frame), min_bbox_error=0.5, min_width=20.0, min_height=20.0)
    res = yr.run(analysis=analysis_of(spec, "sec"))
    assert res.analysis.describe.shape == (1, 4, 8) and (res.row_array(0)[:, 10:14] == 0).all(axis=1).any()  # (this confidence misses some frames)
    assert_equals_harness(res, 0, yr.L, spec, "YoloReplay")
    assert yr.run().analysis is None


# ------------------------------------------------------------------------------------------------- refusals
def test_refusals_touch_no_memory(torch_mod, gold):
    torch = torch_mod
    rp, tc = hard_replay(gold, 100)
    E, R, L, n_log, dev = 2, rp.n_rows, rp.L, rp.n_log, rp._dev
    pos = torch.zeros((rp.n_cycles, E, 2), dtype=torch.int32, device=dev)
    move = torch.zeros_like(pos)
    pair = torch.zeros((R, E), dtype=torch.float64, device=dev)
    n, Q = 3, 2
    outs = dict(describe=torch.full((E, n, 5 + Q), -7.0, dtype=torch.float64, device=dev), cycle_max=torch.full((E, n_log, n), -7.0, dtype=torch.float64, device=dev),
                cycle_mean=torch.full((E, n_log, n), -7.0, dtype=torch.float64, device=dev), step_q=torch.full((E, L, n, Q), -7.0, dtype=torch.float64, device=dev),
                step_count=torch.full((E, L, n), -7, dtype=torch.int32, device=dev), counts=torch.full((E, 7), -7, dtype=torch.int64, device=dev),
                mask=torch.full((E, R), 249, dtype=torch.uint8, device=dev), stats=torch.full((E, 4), -7, dtype=torch.int64, device=dev))
    scratch = torch.full((4,), -7.0, dtype=torch.float64, device=dev)
    good = dict(cfg=rp._cfg, acfg=hip.replay_analysis_config(3, True, (40, 40, 1500, 1300), True, (1, 1, 1), 4.5, 0.5, 15, 14.5, 14.5, True), E=E,
                n_cycles=rp.n_cycles, track=rp.track, n_track=rp.n_track, share=rp._share, pos=pos, move=move, pair=None, columns=[24, 27, 28],
                percentiles=[0.5, 0.95], max_lds_rows=0, scratch=scratch, scratch_doubles=4)

    def call(**kw):
        a = dict(good, **kw)
        hip.replay_analyze(a["cfg"], a["acfg"], a["E"], a["n_cycles"], a["track"], a["n_track"], a["share"], a["pos"], a["move"], a["pair"], a["columns"],
                           a["percentiles"], a["max_lds_rows"], outs["describe"], outs["cycle_max"], outs["cycle_mean"], outs["step_q"], outs["step_count"],
                           outs["counts"], outs["mask"], outs["stats"], a["scratch"], a["scratch_doubles"], stream=torch.cuda.current_stream().cuda_stream)

    bad_period = hip.replay_analysis_config(0, False, None, False, (1, 1, 1), 1, 1, 1, 1, 1, True)
    assert hip.replay_analysis_scratch_doubles(-1, 5, 1, 1) == -1 and hip.replay_analysis_scratch_doubles(5, 100, 3, 2) == 3
    for what, kw in (("unknown column", dict(columns=[24, 30])), ("unknown column", dict(columns=[-1])), ("percentile", dict(percentiles=[0.5, 1.5])),
                     ("percentile", dict(percentiles=[float("nan")])), ("period", dict(acfg=bad_period)), ("precise_pair_dev", dict(columns=[29])),
                     ("scratch", dict(scratch_doubles=0)), ("null", dict(pos=None)), ("null", dict(track=None)), ("null", dict(acfg=None)),
                     ("null", dict(cfg=None)), ("null", dict(scratch=None)), ("columns", dict(columns=list(range(30)) + [0, 1, 2])),
                     ("percentiles", dict(percentiles=[0.5] * 17)), ("E >= 1", dict(E=0)), ("n_cycles", dict(n_cycles=rp.n_log - 1)),
                     ("track is shorter", dict(n_track=R - 1)), ("max_lds_rows", dict(max_lds_rows=-1))):
        with pytest.raises(hip.WtkError, match=what):
            call(**kw)
    torch.cuda.synchronize()
    for name, t in outs.items():
        assert bool((t == (249 if name == "mask" else -7)).all()), name
    assert bool((scratch == -7.0).all())
    call(pair=pair, columns=[24, 29, 28])  # the same call, accepted: every output is written
    torch.cuda.synchronize()
    for name, t in outs.items():
        assert not bool((t == (249 if name == "mask" else -7)).any()), name
