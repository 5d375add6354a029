"""A ReplaySet whose tracks each have their own TimingConfig, on the MI355X (the geometry table of csrc/replay_set_device.h).
The yardstick everywhere is the EXISTING single-track path, `Replay(track_t, timing_config_t, experiment_config_t)` alone, compared bit for bit; it is
never the code under test.  The tracks are those of tests/golden/replay_set_scales.npz (three recordings at 88, 90 and 92 px/mm: cameras 352 x 361,
360 x 369, 368 x 377, microscopes 28 x 29, 29 x 30, 29 x 30; tests/test_replay_set_scales_ref.py pins the numpy harness to the reference's logs of
them), and for the CSV controller two long tracks more: 4100 frames (4095 logged rows at L = 9: one row short of a reduction chunk) and 4112 frames
(4104 logged rows: into the second chunk)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from harness import analysis_ref as ar  # noqa: E402
from harness import mlp_ref  # noqa: E402
from harness import replay_ref as rr  # noqa: E402
from harness import replay_set_scales_ref as sc  # noqa: E402
from test_gpu_replay_set import FIELDS, OBJECTIVES, bits, same, summary_array  # noqa: E402,F401
from test_gpu_replay_set_analysis import assert_same_bits, assert_sets_equal, host, set_host  # noqa: E402
from test_gpu_replay_set_precise import summary_array as precise_summary_array  # noqa: E402
from test_replay_set_analysis_ref import same as same_value  # noqa: E402  (the sign of a zero left out, as for every order statistic of the analysis)
from wtracker_amd import hip  # noqa: E402
from wtracker_amd.controllers import PolyfitConfig  # noqa: E402
from wtracker_amd.sim import ExperimentConfig, TimingConfig  # noqa: E402

E_MAX, TIMES, DEGREE = 65, [-9, -6, -3, 0, 2, 4], 2
SIZES = (1, 3, 65)  # one lane, a partial wave, a second wave
ORDERS = ((0, 1, 2), (2, 0, 1))
POPULATIONS = ("polyfit", "polyfit_population", "mlp_population")


@pytest.fixture(scope="module")
def scene(hip_lib, golden_dir):
    """The fixture's three recordings with their own configs, the scaled ReplaySet in two track orders, one plain Replay per track (the yardstick)."""
    import torch

    from wtracker_amd.replay import Replay, ReplaySet

    if hip.device_count() < 1:
        pytest.fail("no HIP device visible")
    fx = sc.load(golden_dir)
    m = fx["meta"]
    ecs = [ExperimentConfig(f"scale{t}", r["num_frames"], m["frames_per_sec"], tuple(m["orig_resolution"]), r["px_per_mm"], tuple(r["init_position"]))
           for t, r in enumerate(m["recordings"])]
    tcs = [TimingConfig(ec, *m["timing"], tuple(m["camera_size_mm"]), tuple(m["micro_size_mm"])) for ec in ecs]
    assert [tc.camera_size_px for tc in tcs] == [(352, 361), (360, 369), (368, 377)] and [tc.micro_size_px for tc in tcs] == [(28, 29), (29, 30), (29, 30)]
    tracks = fx["tracks"]
    sets = {order: ReplaySet.from_experiments([tracks[t] for t in order], [ecs[t] for t in order], *m["timing"], tuple(m["camera_size_mm"]),
                                              tuple(m["micro_size_mm"])) for order in ORDERS}
    rs = sets[ORDERS[0]]
    assert rs.T == 3 and rs.L == 9 and [tc.camera_size_px for tc in rs.timing_configs] == [tc.camera_size_px for tc in tcs] and rs.timing_config is rs.timing_configs[0]
    assert [rs.replay(t).timing_config for t in range(3)] == rs.timing_configs and rs.replay(2).geometry.mic == (29, 30)
    per = [Replay(tr, tc, ec) for tr, tc, ec in zip(tracks, tcs, ecs)]
    weights = np.random.default_rng(11).uniform(0.05, 1.0, size=(E_MAX, len(TIMES)))
    return dict(torch=torch, fx=fx, rs=rs, sets=sets, per=per, tracks=tracks, ecs=ecs, tcs=tcs, weights=weights, golden=golden_dir)


@pytest.fixture(scope="module")
def folded(scene):
    """E_MAX variants of the shipped 100 ms predictor (model 0 is the predictor itself), folded one by one."""
    from wtracker_amd.training import HipMLPTrainer

    path = os.path.join(scene["golden"], "resmlp_100ms.npz")
    sd, acts = mlp_ref.fixture_network(path)
    z = np.load(path)
    rng = np.random.default_rng(5)
    models = []
    for e in range(E_MAX):
        mdl = {k: np.array(v) for k, v in sd.items()}
        if e:
            for k in mdl:
                if k.endswith(".0.weight") or k == "model.output.weight":
                    mdl[k] = (mdl[k] * rng.uniform(0.8, 1.2, size=mdl[k].shape)).astype(np.float32)
        models.append(dict(mdl, activations=acts, input_frames=z["input_frames"].tolist(), pred_frames=z["pred_frames"].tolist()))
    t = HipMLPTrainer(models, max_batch=2)
    out = [t.folded(e) for e in range(E_MAX)]
    t.close()
    return out


def build(owner, name, scene, folded, E):
    """The targets of builder `name` with E experiments (csv, optimal and mlp have one) on a ReplaySet or a Replay."""
    w = scene["weights"][:E]
    if name == "csv":
        return owner.csv()
    if name == "optimal":
        return owner.optimal()
    if name == "polyfit":
        return owner.polyfit([PolyfitConfig(DEGREE, TIMES, [float(v) for v in row]) for row in w])
    if name == "polyfit_population":
        return owner.polyfit_population(w, DEGREE, TIMES)
    if name == "mlp":
        return owner.mlp(folded[0])
    return owner.mlp_population(folded[:E])


@pytest.fixture(scope="module")
def alone(scene, folded):
    """(builder, E) -> per track (the targets on that track's Replay, its run): the existing path, computed once."""
    cache = {}

    def get(name, E):
        if (name, E) not in cache:
            cache[name, E] = [(tg, rp.run(tg, rows=[])) for rp in scene["per"] for tg in [build(rp, name, scene, folded, E)]]
        return cache[name, E]

    return get


# ------------------------------------------------------------------------------------------------- 1. every pair has the bits of its track alone
CASES = [(n, 1) for n in ("csv", "optimal", "mlp")] + [(n, E) for n in POPULATIONS for E in SIZES]


@pytest.mark.parametrize("name,E", CASES)
def test_every_pair_equals_the_replay_of_its_track_with_its_own_config(scene, folded, alone, name, E):
    torch, ones = scene["torch"], alone(name, E)
    for order in ORDERS:
        rs = scene["sets"][order]
        tg = build(rs, name, scene, folded, E)
        res = rs.run(tg)
        assert tg.E == E and len(res.moves) == 3
        pooled = np.zeros((E, 6))
        for k, t in enumerate(order):
            one_tg, one = ones[t]
            rp = scene["per"][t]
            assert rs.n_cycles[k] == rp.n_cycles and res.moves[k].shape == (E, rp.n_cycles, 2)
            if name == "mlp":  # the clip binds, at this track's own bound
                from wtracker_amd.replay import mlp_clip_bound

                sl = slice(rs.cyc_off[k], rs.cyc_off[k] + rs.n_cycles[k])
                a, v = tg.a[sl].cpu().numpy(), tg.valid[sl].cpu().numpy().astype(bool)
                assert same(a[v], one_tg.a.cpu().numpy()[v])
                assert np.abs(a[v]).max() == float(np.float32(mlp_clip_bound(scene["tcs"][t], 0.9, folded[0].pred_frames))), (order, t)
            assert np.array_equal(res.moves[k], one.moves), (order, t, "moves")
            assert np.array_equal(res.positions[k], one.positions), (order, t, "positions")
            assert np.array_equal(bits(summary_array(res.track_summary[k])), bits(summary_array(one.summary))), (order, t, "summary")
            pooled = pooled + summary_array(one.summary)  # sequential float64 adds in THIS set's track order from 0.0
        assert np.array_equal(bits(summary_array(res.summary)), bits(pooled)), (order, "pooled")
        for kind, (num, den) in OBJECTIVES.items():
            each = rs.objective(tg, kind, per_track=True).cpu().numpy()
            got = rs.objective(tg, kind).cpu().numpy()
            assert each.shape == (3, E) and same(got, pooled[:, num] / pooled[:, den]), (order, kind)
            for k, t in enumerate(order):
                assert same(each[k], scene["per"][t].objective(ones[t][0], kind).cpu().numpy()), (order, t, kind)
        torch.cuda.synchronize()
    if E == E_MAX:
        assert len({ones[0][1].moves[e].tobytes() for e in range(E)}) > E // 2  # the experiments differ


def test_the_scales_matter(scene, folded, alone):
    """What a set built from ONE TimingConfig computes differs from the per-track configs on the tracks whose config it is not: the tests above would
    not pass on it."""
    from wtracker_amd.replay import ReplaySet

    uniform = ReplaySet(scene["tracks"], scene["tcs"][0], scene["ecs"])
    for name in ("csv", "mlp"):
        res, ones = uniform.run(build(uniform, name, scene, folded, 1)), alone(name, 1)
        assert np.array_equal(bits(summary_array(res.track_summary[0])), bits(summary_array(ones[0][1].summary)))
        for t in (1, 2):
            assert not np.array_equal(bits(summary_array(res.track_summary[t])), bits(summary_array(ones[t][1].summary))), (name, t)
    assert not np.array_equal(res.moves[2], ones[2][1].moves)  # (the MLP's clip bound)


def test_csv_on_long_tracks_across_a_reduction_chunk(scene):
    """The fixture's tracks plus two long ones, CSV only: 4095 logged rows (one chunk, all but its last row) and 4104 (a second chunk)."""
    from wtracker_amd.replay import Replay, ReplaySet

    long_a, long_b = rr.long_track(4130, 9)[:4100].copy(), rr.long_track(4130, 9)[:4112].copy()
    ec_a = ExperimentConfig("long_a", 4100, 60, (1600, 1400), 91, (700, 600))
    ec_b = ExperimentConfig("long_b", 4112, 60, (1600, 1400), 89, (700, 600))
    m = scene["fx"]["meta"]
    tracks, ecs = scene["tracks"] + [long_a, long_b], scene["ecs"] + [ec_a, ec_b]
    rs = ReplaySet.from_experiments(tracks, ecs, *m["timing"], tuple(m["camera_size_mm"]), tuple(m["micro_size_mm"]))
    assert rs.n_rows[3:] == [4095, 4104] and rs.timing_configs[3].camera_size_px == (364, 373) and rs.timing_configs[4].micro_size_px == (28, 29)
    res = rs.run(rs.csv())
    pooled = np.zeros((1, 6))
    for t in range(5):
        rp = Replay(tracks[t], rs.timing_configs[t], ecs[t])
        one = rp.run(rp.csv(), rows=[])
        assert np.array_equal(res.moves[t], one.moves) and np.array_equal(res.positions[t], one.positions), t
        assert np.array_equal(bits(summary_array(res.track_summary[t])), bits(summary_array(one.summary))), t
        pooled = pooled + summary_array(one.summary)
    assert np.array_equal(bits(summary_array(res.summary)), bits(pooled))


# ------------------------------------------------------------------------------------------------- 2. the precise error on small frames
def small_scene(torch):
    """Three recordings of a 9 x 7 blob on 96 x 96-class frames at 1, 1.1 and 1.25 px per unit: cameras 40 x 32, 44 x 35, 50 x 40 and microscopes
    14 x 10, 15 x 11, 18 x 12 from ONE (40, 32) / (14, 10); I = 4, P = 1, M = 2.  The blob alternates between slow and fast stretches."""
    from wtracker_amd.replay import ReplaySet

    rng = np.random.default_rng(29)
    shapes, n_frames, scale = [(96, 96), (96, 112), (104, 96)], [67, 55, 73], [1.0, 1.1, 1.25]
    tracks, frames, bgs, ecs = [], [], [], []
    for (H, W), n, s in zip(shapes, n_frames, scale):
        pos, heading = np.array([W / 2, H / 2]), rng.uniform(0, 2 * np.pi)
        tr, fr = np.empty((n, 4)), np.full((n, H, W), 100, dtype=np.uint8)
        for i in range(n):
            speed = 3.0 if (i // 11) % 2 else 0.4
            heading += rng.normal(0, 0.2)
            step = speed * np.array([np.cos(heading), np.sin(heading)])
            if not (14 < pos[0] + step[0] < W - 14 and 14 < pos[1] + step[1] < H - 14):
                heading += np.pi
                step = -step
            pos = pos + step
            w, h = 9 + rng.normal(0, 0.3), 7 + rng.normal(0, 0.3)
            tr[i] = (pos[0] - w / 2, pos[1] - h / 2, w, h)
            x0, y0 = int(np.floor(tr[i, 0])), int(np.floor(tr[i, 1]))
            fr[i, y0:y0 + int(np.ceil(h)), x0:x0 + int(np.ceil(w))] = 200
        tr[23] = np.nan
        tracks.append(tr), frames.append(torch.from_numpy(fr).cuda()), bgs.append(np.full((H, W), 100, dtype=np.uint8))
        ecs.append(ExperimentConfig("small", n, 1000, (H, W), s, (W // 2, H // 2)))
    rs = ReplaySet.from_experiments(tracks, ecs, 4, 1, 2, (40, 32), (14, 10), frame_shapes=shapes)
    assert [tc.camera_size_px for tc in rs.timing_configs] == [(40, 32), (44, 35), (50, 40)]
    assert [tc.micro_size_px for tc in rs.timing_configs] == [(14, 10), (15, 11), (18, 12)] and rs.L == 6
    rs.attach_frames(frames, bgs, 20)
    return rs


def test_precise_error_with_frames_attached(scene):
    from wtracker_amd.replay import PRECISE_OBJECTIVES

    rs = small_scene(scene["torch"])
    w, times = scene["weights"][:3, :4], [-4, -2, 0, 1]
    tg = rs.polyfit_population(w, 1, times)
    res = rs.run(tg, precise=True, per_row_errors=True)
    pooled = np.zeros((3, 6))
    for t in range(3):
        rp = rs.replay(t)
        one_tg = rp.polyfit_population(w, 1, times)
        one = rp.run(one_tg, rows=[], per_row_errors=True, precise=True)
        assert np.array_equal(res.moves[t], one.moves) and np.array_equal(res.positions[t], one.positions), t
        assert np.array_equal(res.precise_counts[t], one.precise_counts) and same(res.precise_error[t], one.precise_error), t
        assert np.array_equal(bits(precise_summary_array(res.track_precise_summary[t])), bits(precise_summary_array(one.precise_summary))), t
        pooled = pooled + precise_summary_array(one.precise_summary)
        err = one.precise_error[~np.isnan(one.precise_error)]
        assert (err == 0).any() and (err > 0).any(), t  # the microscope keeps the blob on some rows and loses part of it on others
        for kind in PRECISE_OBJECTIVES:
            assert same(rs.objective(tg, kind, per_track=True).cpu().numpy()[t], rp.objective(one_tg, kind).cpu().numpy()), (t, kind)
    assert np.array_equal(bits(precise_summary_array(res.precise_summary)), bits(pooled))
    slots = {"trimmed_precise_error": (2, 3), "precise_error": (0, 1), "precise_non_perfect": (4, 1)}
    for kind, (num, den) in slots.items():
        assert same(rs.objective(tg, kind).cpu().numpy(), pooled[:, num] / pooled[:, den]), kind


# ------------------------------------------------------------------------------------------------- 3. the analysis in seconds and micrometres
COLUMNS = ["wrm_speed", "worm_deviation", "bbox_error", "wrm_x", "time"]
PERCENTILES = [0.05, 0.5, 0.95]


def spec_sec(**kw):
    from wtracker_amd.replay import Analysis

    base = dict(period=10, unit="sec", columns=COLUMNS, percentiles=PERCENTILES, min_bbox_error=0.5, min_dist_error=15 * 11.1, min_speed=4.5 * 666.0,
                min_size=14.5 * 11.1, anomaly_mask=True)
    base.update(kw)
    return Analysis(**base)


@pytest.mark.parametrize("name,E", [("csv", 1), ("polyfit_population", 3), ("mlp", 1)])
def test_run_analysis_in_seconds_takes_every_tracks_own_factors(scene, folded, alone, name, E):
    rs, spec, ones = scene["rs"], spec_sec(), alone(name, E)
    factors = spec.factors(rs.timing_configs)
    assert len(factors) == 3 and len({f[1] for f in factors}) == 3 and factors[1] == spec.factors(scene["tcs"][1])
    res = rs.run_analysis(build(rs, name, scene, folded, E), spec)
    got = dict(pooled={n: (None if getattr(res.analysis.pooled, n) is None else np.ascontiguousarray(getattr(res.analysis.pooled, n)))
                       for n in ("describe", "step_quantiles", "step_count", "anomaly_counts", "stats")},
               track=[{n: (None if getattr(a, n) is None else np.ascontiguousarray(getattr(a, n))) for n in
                       ("describe", "cycle_max", "cycle_mean", "step_quantiles", "step_count", "anomaly_counts", "stats", "anomaly_mask")}
                      for a in res.analysis.track])
    logs = []
    for t, rp in enumerate(scene["per"]):
        one = host(rp.analyze(ones[t][0], spec))  # that track alone, with that track's TimingConfig
        assert_same_bits(got["track"][t], one, (name, t))
        logs.append([rp.run(ones[t][0], rows=[e]).row_array(e) for e in range(E)])
    th = dict(min_speed=spec.min_speed, min_bbox_error=spec.min_bbox_error, min_dist_error=spec.min_dist_error, min_width=spec.min_size, min_height=spec.min_size)
    specs = [ar.Spec(period=spec.period, factors=f, columns=tuple(COLUMNS), percentiles=tuple(PERCENTILES), **th) for f in factors]
    Q = len(PERCENTILES)
    order = [0] + list(range(3, 5 + Q))  # count, min, the percentiles, max
    for e in range(E):
        want = sc.analyze([logs[t][e] for t in range(3)], rs.L, specs)["pooled"]
        g = got["pooled"]["describe"][e]
        assert same_value(g[:, order], want["describe"][:, order]), (name, e, "count, min, percentiles, max")
        for j, v in enumerate(want["values"]):
            n = int((~np.isnan(v)).sum())
            assert abs(g[j, 1] - want["describe"][j, 1]) <= ar.mean_bound(v), (name, e, COLUMNS[j], "mean")
            assert abs(g[j, 2] - want["describe"][j, 2]) <= ar.std_bound(n) * want["describe"][j, 2], (name, e, COLUMNS[j], "std")
        assert same_value(got["pooled"]["step_quantiles"][e], want["step_quantiles"]) and np.array_equal(got["pooled"]["step_count"][e], want["step_count"])
        assert np.array_equal(got["pooled"]["anomaly_counts"][e], want["anomaly_counts"]) and np.array_equal(got["pooled"]["stats"][e], want["stats"])
    assert got["pooled"]["anomaly_counts"][:, 6].min() > 0  # the thresholds do flag rows
    # rs.analyze: the same as device tensors
    assert_sets_equal(set_host(rs.analyze(build(rs, name, scene, folded, E), spec)),
                      dict(pooled=dict(got["pooled"], cycle_max=np.ascontiguousarray(res.analysis.pooled.cycle_max),
                                       cycle_mean=np.ascontiguousarray(res.analysis.pooled.cycle_mean),
                                       anomaly_mask=np.ascontiguousarray(res.analysis.pooled.anomaly_mask)), track=got["track"]))


# ------------------------------------------------------------------------------------------------- 4. a list of equal configs is the one config
def test_a_list_of_equal_configs_gives_the_bits_of_one_config(scene, folded):
    from wtracker_amd.replay import ReplaySet

    tc = scene["tcs"][1]
    one, many = ReplaySet(scene["tracks"], tc, scene["ecs"]), ReplaySet(scene["tracks"], [tc] * 3, scene["ecs"])
    assert one._geom() is None and many._geom() is not None and many.timing_configs == [tc] * 3 == one.timing_configs
    spec = spec_sec()
    for name, E in (("csv", 1), ("polyfit_population", 65), ("mlp", 1), ("mlp_population", 3)):
        ta, tb = build(one, name, scene, folded, E), build(many, name, scene, folded, E)
        if name != "csv":
            assert same(ta.a.cpu().numpy(), tb.a.cpu().numpy()) and np.array_equal(ta.valid.cpu().numpy(), tb.valid.cpu().numpy()), name
        ra, rb = one.run_analysis(ta, spec), many.run_analysis(tb, spec)
        assert np.array_equal(bits(summary_array(ra.summary)), bits(summary_array(rb.summary))), name
        for t in range(3):
            assert np.array_equal(ra.moves[t], rb.moves[t]) and np.array_equal(ra.positions[t], rb.positions[t]), (name, t)
            assert np.array_equal(bits(summary_array(ra.track_summary[t])), bits(summary_array(rb.track_summary[t]))), (name, t)
        as_dict = lambda r: dict(pooled={n: getattr(r.analysis.pooled, n) for n in ("describe", "cycle_max", "cycle_mean", "step_quantiles", "step_count",  # noqa: E731
                                                                                  "anomaly_counts", "stats", "anomaly_mask")},
                                 track=[{n: getattr(a, n) for n in ("describe", "cycle_max", "cycle_mean", "step_quantiles", "step_count", "anomaly_counts",
                                                                    "stats", "anomaly_mask")} for a in r.analysis.track])
        assert_sets_equal(as_dict(ra), as_dict(rb), name)
        for kind in OBJECTIVES:
            assert same(one.objective(ta, kind).cpu().numpy(), many.objective(tb, kind).cpu().numpy()), (name, kind)
            assert same(one.objective(ta, kind, per_track=True).cpu().numpy(), many.objective(tb, kind, per_track=True).cpu().numpy()), (name, kind)


# ------------------------------------------------------------------------------------------------- 5. the search on the scaled set
def test_optimize_polyfit_on_the_scaled_set_reproduces(scene):
    rs = scene["rs"]
    kw = dict(pop_size=24, max_epoch=6, max_early_stop=6, seed=3, lb=0.05)
    best = rs.optimize_polyfit(DEGREE, TIMES, **kw)
    again = rs.optimize_polyfit(DEGREE, TIMES, **kw)
    assert np.array_equal(best.weights, again.weights) and best.mae == again.mae and np.isfinite(best.mae)
    res = rs.run(rs.polyfit([rs.to_config(DEGREE, best.weights)]))
    assert bits([res.summary.trimmed_mean_bbox_error[0]]) == bits([best.mae])
    pooled = np.zeros((1, 6))
    for t, rp in enumerate(scene["per"]):  # ... and through each track's own Replay
        pooled = pooled + summary_array(rp.run(rp.polyfit([rs.to_config(DEGREE, best.weights)]), rows=[]).summary)
    assert bits(pooled[:, 2] / pooled[:, 3]) == bits([best.mae])


# ------------------------------------------------------------------------------------------------- 6. the field-of-view sweep
def test_field_of_view_sweep_in_one_call(scene, folded):
    """Recording 0 entered four times with growing microscopes 26 x 27, 28 x 29, 32 x 33, 35 x 37 (both parities of size // 2): the controller sees the
    camera, so the moves are those of one entry; a larger microscope box about the same position contains the smaller one (its left edge
    p - w // 2 does not grow, its right edge p - w // 2 + w = p + ceil(w / 2) does not shrink), every row's bbox error is a monotone float64
    expression of the intersection, and float64 addition in one fixed order is monotone: the per-track mean error cannot increase."""
    from wtracker_amd.replay import ReplaySet

    ec, m = scene["ecs"][0], scene["fx"]["meta"]
    micro_mm = [(0.30, 0.31), (0.32, 0.33), (0.36, 0.37), (0.40, 0.42)]
    tcs = [TimingConfig(ec, *m["timing"], tuple(m["camera_size_mm"]), mm) for mm in micro_mm]
    assert [tc.micro_size_px for tc in tcs] == [(26, 27), (28, 29), (32, 33), (35, 37)]
    rs = ReplaySet([scene["tracks"][0]] * 4, tcs, ec)
    for name, E in (("csv", 1), ("polyfit_population", 65), ("mlp", 1)):
        tg = build(rs, name, scene, folded, E)
        res = rs.run(tg)
        for g in range(1, 4):
            assert np.array_equal(res.moves[g], res.moves[0]) and np.array_equal(res.positions[g], res.positions[0]), (name, g)
        each = rs.objective(tg, "bbox_error", per_track=True).cpu().numpy()
        assert each.shape == (4, E) and (np.diff(each, axis=0) <= 0).all() and (each[0] > each[3]).all(), (name, each[:, 0])
        assert same(each[1], scene["per"][0].objective(build(scene["per"][0], name, scene, folded, E), "bbox_error").cpu().numpy()), name


# ------------------------------------------------------------------------------------------------- 7. refusals
def test_refusals_name_the_track(scene):
    from wtracker_amd.replay import ReplaySet

    tracks, ecs, tcs, m = scene["tracks"], scene["ecs"], scene["tcs"], scene["fx"]["meta"]
    with pytest.raises(ValueError, match="3 tracks.*sequence of 3, got 2"):
        ReplaySet(tracks, tcs[:2], ecs)
    other = TimingConfig(ecs[2], 120, 40, 50, tuple(m["camera_size_mm"]), tuple(m["micro_size_mm"]))  # imaging 8 frames, not 6
    with pytest.raises(ValueError, match=r"track 2: .*\(8, 3, 3\), track 0 has \(6, 3, 3\)"):
        ReplaySet(tracks, [tcs[0], tcs[1], other], ecs)
    small_cam = TimingConfig(ecs[1], *m["timing"], (0.3, 4.1), tuple(m["micro_size_mm"]))
    with pytest.raises(ValueError, match="track 1: the camera .* is smaller than the microscope"):
        ReplaySet(tracks, [tcs[0], small_cam, tcs[2]], ecs)
    with pytest.raises(ValueError, match="track 1: .*TimingConfig"):
        ReplaySet(tracks, [tcs[0], None, tcs[2]], ecs)
    # the C ABI refuses the same of a geometry table, before anything is launched
    rs = scene["rs"]
    E, sp = 1, rs._super
    buf = rs._objective_buffers(E)
    good = [dict(cam=rp.geometry.cam, mic=rp.geometry.mic, factors=(1.0, 1.0, 1.0)) for rp in rs._replays]
    bad = [dict(g) for g in good]
    bad[1] = dict(bad[1], mic=(bad[1]["cam"][0] + 1, 5))
    before = buf["pos"].fill_(-7).clone()
    with pytest.raises(hip.WtkError, match="wtk_replay_set_scan_geom: track 1: the camera is smaller than the microscope"):
        hip.replay_set_scan(sp._cfg, rs._table, hip.REPLAY_CSV, E, sp.track, None, None, None, sp._share, buf["pos"], buf["move"],
                            geom=hip.ReplaySetGeometry(bad, device=rs._dev))
    with pytest.raises(hip.WtkError, match="one entry per track"):
        hip.replay_set_scan(sp._cfg, rs._table, hip.REPLAY_CSV, E, sp.track, None, None, None, sp._share, buf["pos"], buf["move"],
                            geom=hip.ReplaySetGeometry(good[:2], device=rs._dev))
    scene["torch"].cuda.synchronize()
    assert scene["torch"].equal(buf["pos"], before)
    with pytest.raises(hip.WtkError, match="wtk_replay_mlp_targets_bounds: null argument"):
        hip._check(hip.load().wtk_replay_mlp_targets_bounds(None, 0, 0, 0, None, 1, None, None, 1, None, 1, None, 1, None, None, None, None, None, None),
                   "wtk_replay_mlp_targets_bounds")
