"""wtracker_amd.replay.ReplaySet.analyze / run_analysis on the MI355X (csrc/replay_set_analysis.hip): DataAnalyzer's statistics of
a population replayed on several tracks, per log and pooled over the concatenation of the logs as the reference's Plotter concatenates them.

Yardsticks, none of them the code under test: per track the EXISTING single-track path `rs.replay(t).analyze` / `run(analysis=...)`, bit for bit; pooled
tests/golden/analysis_set.npz (the real DataAnalyzer, the Plotter's concatenation and pandas) and the numpy restatement
tests/harness/replay_set_analysis_ref.py, which tests/test_replay_set_analysis_ref.py pins to that fixture.  Against the fixture and the harness the
rules are that file's: counts, minima, maxima, percentiles, cycle maxima, step quantiles and counts, anomaly counts and stats equal as float64 bits but
for the sign of a zero (among -0.0 and 0.0 pandas returns whichever its sort left in place), pooled means within analysis_ref.mean_bound of the
concatenated values, pooled stds within std_bound(N).

On the parent commit a ReplaySet has no `analyze`: every test here fails there."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from harness import analysis_ref as ar  # noqa: E402
from harness import replay_set_analysis_ref as sr  # noqa: E402
from harness import replay_set_precise_ref as sp  # noqa: E402
from test_gpu_replay_analysis import analysis_of  # noqa: E402
from test_gpu_replay_set import BUILDERS, DEGREE, E, TIMES, build, nets, scene  # noqa: E402,F401  (the three tracks, E = 70, the six builders)
from test_gpu_replay_set_precise import make_set, slice_of, targets_of  # noqa: E402
from test_replay_set_analysis_ref import mismatches, same, spec_of  # noqa: E402
from wtracker_amd import hip  # noqa: E402
from wtracker_amd.controllers import PolyfitConfig  # noqa: E402

ARRAYS = ("describe", "cycle_max", "cycle_mean", "step_quantiles", "step_count", "anomaly_counts", "stats", "anomaly_mask")
POOLED = ("describe", "step_quantiles", "step_count", "anomaly_counts", "stats")


def spec_small(**kw):
    """A spec that uses every stage: both trims, bounds, unit "sec", thresholds, the mask; five columns, three percentiles."""
    from wtracker_amd.replay import Analysis

    base = dict(period=3, trim_cycles=True, imaging_only=True, bounds=(40, 40, 1500, 1300), unit="sec",
                columns=["wrm_speed", "worm_deviation", "bbox_error", "wrm_x", "time"], percentiles=[0.05, 0.5, 0.95], min_bbox_error=0.5, min_dist_error=15 * 11.1,
                min_speed=4.5 * 333.0, min_size=14.5 * 11.1, anomaly_mask=True)
    base.update(kw)
    return Analysis(**base)


def host(a):
    """An AnalysisResult of device tensors as contiguous numpy arrays, by name."""
    return {n: (None if getattr(a, n) is None else np.ascontiguousarray(getattr(a, n).cpu().numpy())) for n in ARRAYS}


def assert_same_bits(x: dict, y: dict, what="", names=ARRAYS):
    for n in names:
        assert (x[n] is None) == (y[n] is None), (what, n)
        if x[n] is not None:
            assert x[n].shape == y[n].shape and x[n].dtype == y[n].dtype and x[n].tobytes() == y[n].tobytes(), (what, n)


def set_host(res) -> dict:
    return dict(pooled=host(res.pooled), track=[host(a) for a in res.track])


def assert_sets_equal(x: dict, y: dict, what=""):
    assert_same_bits(x["pooled"], y["pooled"], (what, "pooled"))
    for t, (a, b) in enumerate(zip(x["track"], y["track"])):
        assert_same_bits(a, b, (what, t))


# ------------------------------------------------------------------------------------------------- 1. every track has the bits of its track alone
@pytest.mark.parametrize("name", BUILDERS)
def test_every_track_equals_the_analysis_of_its_track_alone(scene, nets, name):
    rs, per, spec = scene["rs"], scene["per"], spec_small()
    tg = build(rs, name, scene, nets)
    res = rs.analyze(tg, spec)
    n_exp = 1 if name in ("csv", "optimal", "mlp") else E
    assert len(res.track) == 3 and res.pooled.n_rows == 395 + 135 + 4125 and res.pooled.describe.shape == (n_exp, 5, 8)
    assert res.pooled.cycle_max.shape == (n_exp, 79 + 27 + 825, 5) and res.pooled.anomaly_mask.shape == (n_exp, 4655)
    got = set_host(res)
    for t, rp in enumerate(per):
        one = rp.analyze(build(rp, name, scene, nets), spec)
        assert res.track[t].n_rows == rp.n_rows and tuple(res.track[t].cycle_max.shape) == (n_exp, rp.n_log, 5)
        assert_same_bits(got["track"][t], host(one), (name, t))
    # the integer pooling, and the concatenated arrays
    for n in ("anomaly_counts", "stats"):
        assert np.array_equal(got["pooled"][n], sum(got["track"][t][n] for t in range(3))), n
    assert got["pooled"]["cycle_max"].tobytes() == np.concatenate([got["track"][t]["cycle_max"] for t in range(3)], axis=1).tobytes()
    assert got["pooled"]["anomaly_mask"].tobytes() == np.concatenate([got["track"][t]["anomaly_mask"] for t in range(3)], axis=1).tobytes()
    assert (got["pooled"]["describe"][:, :, 0] == sum(got["track"][t]["describe"][:, :, 0] for t in range(3))).all()
    assert got["pooled"]["describe"][:, 2, 0].min() > 2000  # bbox_error: the kept rows of all three logs


# ------------------------------------------------------------------------------------------------- 2. pooled: the reference's fixture and the harness
@pytest.fixture(scope="module")
def gold(golden_dir):
    z = np.load(os.path.join(golden_dir, "analysis_set.npz"))
    return dict(z=z, meta=json.loads(bytes(z["meta"]).decode()), scene=sr.the_scene(golden_dir))


def pooled_dict(a, e: int) -> dict:
    """Experiment e of a pooled AnalysisResult of numpy arrays, as the harness lays a pooled result out."""
    return {n: np.asarray(getattr(a, n)[e]) for n in ARRAYS if getattr(a, n) is not None}


def test_pooled_equals_the_reference_and_the_harness(scene, gold):
    """csv, optimal and a degree-1 Polyfit on the three tracks under configurations a, b and c (track 1 keeps no row) of the fixture, all 29 columns
    and six percentiles.  The logs the device replays are the CPU replay harness's (the moves are compared first), so the harness's keep masks and
    concatenated values give the bounds of the means."""
    rs, meta, sc = scene["rs"], gold["meta"], gold["scene"]
    pops = {"csv": rs.csv(), "optimal": rs.optimal(), "polyfit": rs.polyfit([PolyfitConfig(sr.DEGREE, sr.TIMES, None)])}
    for kind, tg in pops.items():
        plain = rs.run(tg)
        for t in range(3):  # the same logs as the fixture's: cycle and platform position of every row follow from the moves
            assert np.array_equal(plain.positions[t][0, :rs.n_log[t]], sc["logs"][kind][t][::rs.L, 0:2].astype(np.int32)), (kind, t)
    for cname, cfg in meta["configs"].items():
        spec = spec_of(meta, cname)
        for kind, tg in pops.items():
            res = rs.run_analysis(tg, analysis_of(spec, cfg["unit"]))
            want = sr.analyze_set(sc["logs"][kind], rs.L, spec)
            got = dict(pooled=dict(pooled_dict(res.analysis.pooled, 0), values=want["pooled"]["values"]), keep=want["keep"])
            assert mismatches(gold, cname, kind, got) == [], (cname, kind, "vs the reference")
            for n in ("describe", "step_quantiles", "cycle_max"):  # vs the harness: the order statistics, and the moments in the defined order
                g, w = got["pooled"][n], want["pooled"][n]
                if n == "describe":
                    assert same(g[:, [0] + list(range(3, g.shape[1]))], w[:, [0] + list(range(3, g.shape[1]))]), (cname, kind, n)
                    assert same(g[:, 1:3], w[:, 1:3]), (cname, kind, "mean and std in the harness's order")
                else:
                    assert same(g, w), (cname, kind, n)
            for n in ("step_count", "anomaly_counts", "stats", "anomaly_mask"):
                assert np.array_equal(got["pooled"][n], want["pooled"][n]), (cname, kind, n)
            assert res.analysis.pooled.n_rows == 4655
            for t in range(3):  # the per-track results of run_analysis too
                one = want["track"][t]
                assert same(np.asarray(res.analysis.track[t].describe[0])[:, 3:], one["describe"][:, 3:]) and np.array_equal(
                    res.analysis.track[t].stats[0], one["stats"]), (cname, kind, t)
    assert gold["z"]["c/csv/kept"][1] == 0


def test_describe_table_and_print_stats_on_the_pooled_result(scene, capsys):
    rs = scene["rs"]
    res = rs.run_analysis(rs.csv(), spec_small())
    idx, cols, tab = res.analysis.pooled.describe_table(0)
    assert idx == ["count", "mean", "std", "min", "5%", "50%", "95%", "max"] and cols == ["wrm_speed", "worm_deviation", "bbox_error", "wrm_x", "time"]
    assert tab.shape == (8, 5) and np.array_equal(tab, res.analysis.pooled.describe[0].T)
    res.analysis.pooled.print_stats(0)
    out = capsys.readouterr().out
    removed = int(res.analysis.pooled.stats[0, 0])
    assert f"Count of Removed Frames: {removed} ({round(100 * removed / 4655, 3)}%)" in out and "Total Num of Cycles" in out


# ------------------------------------------------------------------------------------------------- 3. the LDS limit
def test_results_do_not_depend_on_the_lds_limit(scene):
    """0: everything sorted; 4200: the per-track launches sorted (the longest track has 4125 rows), the pooled describe selected (4655 rows);
    64: everything selected but the step segments of track 1 (27 rows)."""
    rs = scene["rs"]
    tg = rs.polyfit_population(scene["weights"][:9], DEGREE, TIMES)
    spec = spec_small(columns=["wrm_speed_x", "bbox_error", "frame"], percentiles=[0.0, 0.33, 0.5, 1.0])
    ref = set_host(rs.analyze(tg, spec))
    assert ref["pooled"]["describe"][:, 1, 0].min() > 2000
    for limit in (4200, 64):
        assert_sets_equal(set_host(rs.analyze(tg, spec, _max_lds_rows=limit)), ref, limit)


# ------------------------------------------------------------------------------------------------- 4. independence of E, T, the place and the guard
def test_bits_do_not_depend_on_the_population_or_the_set(scene):
    from wtracker_amd.replay import ReplaySet

    rs, w, spec = scene["rs"], scene["weights"], spec_small()
    full = set_host(rs.analyze(rs.polyfit_population(w, DEGREE, TIMES), spec))
    again = set_host(rs.analyze(rs.polyfit_population(w, DEGREE, TIMES), spec))
    assert_sets_equal(again, full, "a second run")
    alone = set_host(rs.analyze(rs.polyfit_population(w[37:38], DEGREE, TIMES), spec))
    pick = lambda d, e: {n: (None if v is None else np.ascontiguousarray(v[e:e + 1])) for n, v in d.items()}  # noqa: E731
    assert_same_bits(alone["pooled"], pick(full["pooled"], 37), "experiment 37 alone, pooled")
    for t in range(3):
        assert_same_bits(alone["track"][t], pick(full["track"][t], 37), ("experiment 37 alone", t))
    # track 0 at another index with other companions, and a larger guard
    order = [2, 0]
    other = ReplaySet([scene["tracks"][t] for t in order], scene["tc"], [scene["ecs"][t] for t in order], [scene["shapes"][t] for t in order], reach=200)
    moved = set_host(other.analyze(other.polyfit_population(w, DEGREE, TIMES), spec))
    assert other.guard_cycles == 40
    for k, t in enumerate(order):
        assert_same_bits(moved["track"][k], full["track"][t], ("moved", t))
    # T = 1: the pooled result is the track's, and both are Replay.analyze's
    for t in (0, 1):
        one = ReplaySet([scene["tracks"][t]], scene["tc"], scene["ecs"][t], [scene["shapes"][t]])
        got = set_host(one.analyze(one.polyfit_population(w, DEGREE, TIMES), spec))
        rp = scene["per"][t]
        want = host(rp.analyze(rp.polyfit_population(w, DEGREE, TIMES), spec))
        assert_same_bits(got["track"][0], want, ("T = 1, track", t))
        assert_same_bits(got["pooled"], want, ("T = 1, pooled", t))


# ------------------------------------------------------------------------------------------------- 5. edge sizes
def harness_of(rs, tgs, spec: ar.Spec, e: int = 0):
    """The harness's analysis of experiment e from the rows the EXISTING per-track path logs (tgs: the per-track targets)."""
    logs = [rs.replay(t).run(tg, rows=[e]).row_array(e) for t, tg in enumerate(tgs)]
    return sr.analyze_set(logs, rs.L, spec)


def assert_pooled_equals_harness(pooled: dict, want: dict, spec: ar.Spec, what=""):
    g, w = pooled["describe"], want["pooled"]["describe"]
    assert same(g, w), (what, "describe", g, w)
    assert same(pooled["step_quantiles"], want["pooled"]["step_quantiles"]) and np.array_equal(pooled["step_count"], want["pooled"]["step_count"]), what
    assert np.array_equal(pooled["anomaly_counts"], want["pooled"]["anomaly_counts"]) and np.array_equal(pooled["stats"], want["pooled"]["stats"]), what


def test_segment_edge_sizes(scene):
    """Pooled kept counts 0, 1 and 2 (bounds: nothing; the rounded worm box of one logged row, as the fixture's configuration c1; the same box with that
    track twice in the set), a track shorter than `period`, and a track of two logged cycles, of which trim_cycles leaves nothing."""
    import dataclasses

    from wtracker_amd.replay import ReplaySet

    hard, tc, ec0 = scene["tracks"][0], scene["tc"], scene["ecs"][0]
    short, two = dataclasses.replace(ec0, num_frames=8), dataclasses.replace(ec0, num_frames=12)  # 1 logged cycle (5 rows < period), 2 logged cycles
    rs = ReplaySet([hard, hard[:8], hard, hard[:12]], tc, [ec0, short, ec0, two])
    assert rs.n_log == [79, 1, 79, 2]
    tg = rs.csv()
    tgs = [rs.replay(t).csv() for t in range(4)]
    row = ar.round5(rs.replay(0).run(tgs[0], rows=[0]).row_array(0)[200, 10:14])
    box = (float(row[0]), float(row[1]), float(row[0] + row[2]), float(row[1] + row[3]))
    cols, q = ("wrm_speed", "bbox_error", "wrm_x"), (0.25, 0.5)
    cases = {"none": ar.Spec(period=10, bounds=(-2, -2, -1, -1), trim_cycles=True, columns=cols, percentiles=q),
             "one box, twice": ar.Spec(period=10, bounds=box, columns=cols, percentiles=q),
             "short tracks": ar.Spec(period=10, trim_cycles=True, columns=cols, percentiles=q)}
    for what, spec in cases.items():
        res = rs.run_analysis(tg, analysis_of(spec))
        want = harness_of(rs, tgs, spec)
        assert_pooled_equals_harness(pooled_dict(res.analysis.pooled, 0), want, spec, what)
        for t in range(4):
            one = rs.replay(t).run(tgs[t], rows=[], analysis=analysis_of(spec)).analysis
            assert_same_bits({n: getattr(res.analysis.track[t], n) for n in ARRAYS}, {n: getattr(one, n) for n in ARRAYS}, (what, t))
        count = res.analysis.pooled.describe[0, 2, 0]
        if what == "none":
            assert count == 0 and np.isnan(res.analysis.pooled.describe[0, :, 1:]).all()
        elif what == "one box, twice":
            assert count == 2 and [a.describe[0, 2, 0] for a in res.analysis.track] == [1, 0, 1, 0]  # an empty track between two that keep a row
            assert not np.isnan(res.analysis.pooled.describe[0, 2, 2])
        else:
            assert [a.describe[0, 2, 0] for a in res.analysis.track] == [385, 0, 385, 0]  # nothing of the one- and two-cycle logs survives the trim
            assert np.isnan(res.analysis.track[1].describe[0, 0, 0:1]).sum() == 0 and res.analysis.track[1].describe[0, 0, 0] == 0
    # count 1: the same box with the track once
    one = ReplaySet([hard, hard[:8]], tc, [ec0, short])
    res = one.run_analysis(one.csv(), analysis_of(cases["one box, twice"]))
    assert res.analysis.pooled.describe[0, 2, 0] == 1 and np.isnan(res.analysis.pooled.describe[0, 2, 2]) and not np.isnan(res.analysis.pooled.describe[0, 2, 1])
    assert_pooled_equals_harness(pooled_dict(res.analysis.pooled, 0), harness_of(one, tgs[:2], cases["one box, twice"]), cases["one box, twice"], "count 1")


# ------------------------------------------------------------------------------------------------- 6. the precise_error column
def test_precise_error_column(scene):
    """On the small frames of the precise error's scene: per track equal to `rs.replay(t).run(precise=True, analysis=...)`, pooled exactly the harness's
    order statistics of the concatenated per-row errors."""
    import torch

    from wtracker_amd.replay import Analysis

    n_exp = 5
    sn = sp.scene(n_exp)
    rs = make_set(torch, sn)
    tg = targets_of(torch, sn)
    spec = Analysis(period=3, trim_cycles=True, imaging_only=True, columns=["precise_error", "bbox_error"], percentiles=[0.5, 0.9], anomaly_mask=True)
    with pytest.raises(ValueError, match="precise_error column needs precise=True"):
        rs.analyze(tg, spec)
    res = rs.run_analysis(tg, spec, precise=True, per_row_errors=True)
    dev = set_host(rs.analyze(tg, spec, precise=True))
    assert_same_bits(dev["pooled"], {n: getattr(res.analysis.pooled, n) for n in ARRAYS}, "analyze and run_analysis")
    hspec = ar.Spec(period=3, trim_cycles=True, imaging_only=True, columns=("precise_error", "bbox_error"), percentiles=(0.5, 0.9))
    for t in range(rs.T):
        one = rs.replay(t).run(slice_of(rs, tg, t), rows=[], precise=True, analysis=spec).analysis
        assert_same_bits({n: getattr(res.analysis.track[t], n) for n in ARRAYS}, {n: getattr(one, n) for n in ARRAYS}, ("precise", t))
    for e in (0, n_exp - 1):
        logs = [rs.replay(t).run(slice_of(rs, tg, t), rows=[e]).row_array(e) for t in range(rs.T)]
        want = sr.analyze_set(logs, rs.L, hspec, precise=[res.precise_error[t][e] for t in range(rs.T)])
        assert_pooled_equals_harness(pooled_dict(res.analysis.pooled, e), want, hspec, ("precise", e))
    assert res.analysis.pooled.describe[:, 0, 0].min() > 0


# ------------------------------------------------------------------------------------------------- 7. refusals
def test_refusals_touch_no_memory(scene):
    import torch

    rs, sp_ = scene["rs"], scene["rs"]._super
    tg = rs.optimal()
    buf = rs._objective_buffers(1)
    hip.replay_set_scan(sp_._cfg, rs._table, hip.REPLAY_OPTIMAL, 1, sp_.track, tg.a, None, tg.valid, sp_._share, buf["pos"], buf["move"])
    spec = spec_small()
    cols, q, n, Q = spec.column_ids(), list(spec.percentiles), 5, 3
    f64, dev = torch.float64, sp_.track.device
    fill = lambda shape, dtype=f64: torch.full(shape, 77, dtype=dtype, device=dev)  # noqa: E731
    per = [fill((3, 1, n, 5 + Q)), fill((1, 931, n)), fill((1, 931, n)), fill((3, 1, 5, n, Q)), fill((3, 1, 5, n), torch.int32), fill((3, 1, 7), torch.int64),
           fill((1, 4655), torch.uint8), fill((3, 1, 4), torch.int64)]
    pooled = [fill((1, n, 5 + Q)), fill((1, 5, n, Q)), fill((1, 5, n), torch.int32), fill((1, 7), torch.int64), fill((1, 4), torch.int64)]
    need = hip.replay_set_analysis_scratch_doubles(rs._table, 1, n, Q)
    scratch = fill((need,))
    acfg = spec.config(scene["tc"])

    def call(**kw):
        a = dict(cfg=sp_._cfg, acfg=acfg, table=rs._table, E=1, track=sp_.track, share=sp_._share, pos=buf["pos"], move=buf["move"], precise=None, cols=cols, q=q,
                 lds=0, per=per, pooled=pooled, scratch=scratch, n_scratch=need)
        a.update(kw)
        hip.replay_set_analyze(a["cfg"], a["acfg"], a["table"], a["E"], a["track"], a["share"], a["pos"], a["move"], a["precise"], a["cols"], a["q"], a["lds"],
                               a["per"], a["pooled"], a["scratch"], a["n_scratch"])

    bad_table = hip.ReplaySetTable([dict(cyc_off=o, n_track=rp.n_track, num_frames=int(rp.experiment_config.num_frames) + (1000 if t == 1 else 0),
                                         n_cycles=rp.n_cycles, n_log=rp.n_log, frame_wh=(rp.frame_shape[1], rp.frame_shape[0]),
                                         init_position=rp.experiment_config.init_position) for t, (rp, o) in enumerate(zip(rs._replays, rs.cyc_off))],
                                   rs.L, rs.guard_cycles, rs._table.n_super, device=dev)
    cases = [(dict(table=bad_table), "track 1"), (dict(cols=[99]), "unknown column"), (dict(cols=[hip.ANALYSIS_COLUMNS.index("precise_error")]), "precise_rows_dev"),
             (dict(q=[1.5]), r"percentile outside \[0, 1\]"), (dict(lds=-1), "max_lds_rows"), (dict(n_scratch=need - 1), "scratch smaller"),
             (dict(scratch=None), "null argument"), (dict(acfg=None), "null argument"), (dict(E=0), "at least one experiment")]
    for kw, message in cases:
        with pytest.raises(hip.WtkError, match=message):
            call(**kw)
    torch.cuda.synchronize()
    for t in per + pooled + [scratch]:
        assert bool((t == 77).all())
    call()  # the same arguments, accepted
    torch.cuda.synchronize()
    assert not bool((pooled[0] == 77).any()) and not bool((per[0] == 77).any())
    with pytest.raises(ValueError, match="the precise error and the analysis are per track"):
        rs.run(tg, analysis=spec)  # run keeps its refusal
    with pytest.raises(ValueError, match="unknown analysis columns"):
        rs.analyze(tg, spec_small(columns=["nope"]))
