"""The closed-loop error as the objective of the Polyfit weight search, on the MI355X (csrc/replay_targets.hip: wtk_replay_polyfit_targets, csrc/replay.hip: wtk_replay_objective;
wtracker_amd.replay: polyfit_population, objective, optimize_polyfit).  Everything runs on tests/golden/replay_hard.npz at 100 ms
imaging (L = 5, 80 cycles of which 79 are logged, NaN rows 6, 31, 33, 120, 251 and 388) and is held to what the existing per-config route gives: rp.polyfit(configs), rp.run and Summary."""
import json
import math
import os
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from harness import polyfit_opt_ref as por  # noqa: E402
from harness import replay_opt_ref as ro  # noqa: E402
from harness.sim_harness import Simulator  # noqa: E402
from wtracker_amd import hip  # noqa: E402
from wtracker_amd.controllers import PolyfitConfig, PolyfitController  # noqa: E402
from wtracker_amd.sim import LOG_COLUMNS, ExperimentConfig, TimingConfig, TrackLogger  # noqa: E402

POP, CHECKED = 70, (0, 63, 64, 69)  # one more than a wave and then some: particles on both sides of the wave boundary
TIMES = [-8, -6, -4, -2, 0, 1]
KINDS = {"trimmed_bbox_error": "trimmed_mean_bbox_error", "bbox_error": "mean_bbox_error", "mse_error": "mean_mse_error", "non_perfect": "non_perfect"}
NUM_KEYS = LOG_COLUMNS[3:]


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


@pytest.fixture(scope="module")
def torch_mod(hip_lib):
    import torch

    if hip.device_count() < 1:
        pytest.fail("no HIP device visible")
    return torch


@pytest.fixture(scope="module")
def hard(golden_dir):
    z = np.load(os.path.join(golden_dir, "replay_hard.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    ec = ExperimentConfig("hard", meta["num_frames"], meta["frames_per_sec"], tuple(meta["orig_resolution"]), meta["px_per_mm"], tuple(meta["init_position"]))
    return dict(meta=meta, ec=ec, track=z["track"])


def replay_of(hard, track=None, ec=None):
    from wtracker_amd.replay import Replay

    ec = hard["ec"] if ec is None else ec
    tc = TimingConfig(ec, 100, 40, 50, hard["meta"]["camera_size_mm"], hard["meta"]["micro_size_mm"])
    return Replay(hard["track"] if track is None else track, tc, ec), tc


@pytest.fixture(scope="module")
def pop(torch_mod, hard):
    """The 70 weight vectors, the Replay, and the parent route's result for degree 2 (computed once, read by several tests)."""
    rp, tc = replay_of(hard)
    assert (rp.L, rp.n_cycles, rp.n_log) == (5, 80, 79)
    weights = np.random.default_rng(7).uniform(0.05, 1.0, size=(POP, 6))
    cfgs = [PolyfitConfig(2, TIMES, [float(v) for v in w]) for w in weights]
    res = rp.run(rp.polyfit(cfgs), rows=[])
    return dict(rp=rp, tc=tc, weights=weights, cfgs=cfgs, res=res)


def assert_targets_equal(rp, weights, degree, times):
    """polyfit_population against one wtk_track_polyfit launch per config: every cycle and particle, values (NaN = NaN) and valid flags."""
    cfgs = [PolyfitConfig(degree, list(times), [float(v) for v in w]) for w in weights]
    want = rp.polyfit(cfgs)
    got = rp.polyfit_population(weights, degree, times)
    assert got.kind == "polyfit" and got.E == len(weights) and got.b is None
    a, v = got.a.cpu().numpy(), got.valid.cpu().numpy()
    wa, wv = want.a.cpu().numpy(), want.valid.cpu().numpy()
    assert a.shape == wa.shape == (rp.n_cycles, len(weights), 2) and v.dtype == np.int32
    assert np.array_equal(v, wv)
    same = np.array_equal(a, wa, equal_nan=True)
    if not same:
        c, p, q = np.argwhere(~((a == wa) | (np.isnan(a) & np.isnan(wa))))[0]
        raise AssertionError(f"degree {degree}: cycle {c} particle {p} axis {q}: {a[c, p, q]!r} != {wa[c, p, q]!r}")
    finite = np.isfinite(wa)
    assert np.array_equal(bits(a[finite]), bits(wa[finite]))  # the same bits, not just equal values
    return a, v


# ------------------------------------------------------------------------------------------------- 1. target bits
@pytest.mark.parametrize("degree", [1, 2, 3])
def test_population_targets_have_the_bits_of_one_launch_per_config(pop, hard, degree):
    rp = pop["rp"]
    a, v = assert_targets_equal(rp, pop["weights"], degree, TIMES)
    assert v.all() and len({a[:, p].tobytes() for p in range(POP)}) == POP  # the weights matter
    # rows blanked: cycle 40 (frames 192 ... 201) keeps no sample, cycle 60 (292 ... 301) keeps frame 301 alone: fewer than degree + 1
    track = hard["track"].copy()
    track[192:202] = np.nan
    track[292:301] = np.nan
    rp2, _ = replay_of(hard, track)
    a2, v2 = assert_targets_equal(rp2, pop["weights"], degree, TIMES)
    assert not v2[40].any() and (a2[40] == 0).all() and v2[60].all() and v2[39].all()
    cycle_class, class_mask = (t.cpu().numpy() for t in rp2.polyfit_class_table(TIMES))
    assert class_mask[cycle_class[40]] == 0 and class_mask[cycle_class[60]] == 0b100000


@pytest.mark.parametrize("degree,times", [(0, [0]), (7, list(range(-14, 2)))])
def test_population_targets_at_the_solver_limits(pop, degree, times):
    """The two ends of the admitted range (1 x 1 and 16 x 8) with a population that crosses the wave boundary.  The first cycles lack the samples
    before the track, so at degree 7 there are classes with fewer samples than coefficients."""
    rp = pop["rp"]
    weights = np.random.default_rng(13).uniform(0.05, 1.0, size=(66, len(times)))
    a, v = assert_targets_equal(rp, weights, degree, times)
    cycle_class, class_mask = (t.cpu().numpy() for t in rp.polyfit_class_table(times))
    kept = np.array([bin(int(m)).count("1") for m in class_mask])[cycle_class]
    assert v.any() and not v[kept == 0].any()
    if degree == 7:
        assert ((kept > 0) & (kept < degree + 1)).any() and (kept == 16).any()


def test_class_table_of_the_fixture(pop):
    """At least 4 classes: the first cycles lack the samples before the track (cycle 0 keeps t = 0 and t = 1 only; cycle 1 loses t = 1 to NaN row 6
    as well), the NaN rows cost single samples."""
    rp = pop["rp"]
    cycle_class, class_mask = (t.cpu().numpy() for t in rp.polyfit_class_table(TIMES))
    assert cycle_class.shape == (rp.n_cycles,) and len(class_mask) >= 4 and len(class_mask) < rp.n_cycles // 2
    assert class_mask[cycle_class[0]] == 0b110000 and class_mask[cycle_class[1]] == 0b011100 and class_mask[cycle_class[20]] == 0b111111
    want = ro.class_table(pop["rp"].track.cpu().numpy(), rp.L, rp.n_cycles, TIMES)
    assert np.array_equal(cycle_class, want[0]) and np.array_equal(class_mask, want[1])
    assert rp.polyfit_class_table(list(reversed(TIMES)))[0] is rp.polyfit_class_table(TIMES)[0]  # cached per sorted times


def test_population_targets_with_unsorted_times(pop):
    weights = np.random.default_rng(11).uniform(0.05, 1.0, size=(POP, 4))
    assert_targets_equal(pop["rp"], weights, 2, [1, -6, 0, -3])


def test_population_targets_with_a_zero_and_a_nan_weight(pop):
    weights = pop["weights"].copy()
    weights[3, 1] = 0.0
    weights[5, 2] = np.nan
    weights[64, :4] = 0.0  # two non-zero weights left: a rank-deficient quadratic
    a, v = assert_targets_equal(pop["rp"], weights, 2, TIMES)
    assert np.isfinite(a[:, 3]).all()


# ------------------------------------------------------------------------------------------------- 2. objective bits
def test_every_objective_equals_the_summary_property(pop):
    rp, s = pop["rp"], pop["res"].summary
    tg = rp.polyfit_population(pop["weights"], 2, TIMES)
    for kind, prop in KINDS.items():
        got = rp.objective(tg, kind).cpu().numpy()
        want = np.asarray(getattr(s, prop), dtype=np.float64)
        assert got.dtype == np.float64 and got.shape == (POP,)
        assert got.tobytes() == want.tobytes(), (kind, np.flatnonzero(bits(got) != bits(want))[:5])
        assert len(set(got.tolist())) > 1 and np.isfinite(got).all(), kind  # not a constant
    with pytest.raises(ValueError):
        rp.objective(tg, "no_such_error")


def test_a_particle_alone_gives_the_bits_it_gives_in_the_population(pop):
    rp = pop["rp"]
    tg = rp.polyfit_population(pop["weights"], 2, TIMES)
    whole = {kind: rp.objective(tg, kind).cpu().numpy() for kind in KINDS}
    for e in CHECKED:
        one = rp.polyfit_population(pop["weights"][e : e + 1], 2, TIMES)
        assert np.array_equal(one.a.cpu().numpy()[:, 0], tg.a.cpu().numpy()[:, e]) and np.array_equal(one.valid.cpu().numpy()[:, 0], tg.valid.cpu().numpy()[:, e])
        for kind in KINDS:
            assert rp.objective(one, kind).cpu().numpy().tobytes() == whole[kind][e : e + 1].tobytes(), (e, kind)


# ------------------------------------------------------------------------------------------------- 3. the gate
def low_level(torch, rp, weights, degree=2, times=TIMES):
    """Sentinel-filled buffers and the three calls of one epoch on them."""
    dev, f64, i32 = rp._dev, torch.float64, torch.int32
    P, N, C = len(weights), len(times), rp.n_cycles
    cycle_class, class_mask = rp.polyfit_class_table(times)
    K = int(class_mask.numel())
    SF, SI = -12345.5, -77
    b = dict(a=torch.full((C, P, 2), SF, dtype=f64, device=dev), valid=torch.full((C, P), SI, dtype=i32, device=dev),
             fit=torch.full((hip.replay_polyfit_targets_scratch_doubles(K, P, N, degree),), SF, dtype=f64, device=dev),
             pos=torch.full((C, P, 2), SI, dtype=i32, device=dev), move=torch.full((C, P, 2), SI, dtype=i32, device=dev),
             summary=torch.full((P, 6), SF, dtype=f64, device=dev), scratch=torch.full((hip.replay_scratch_doubles(P, rp.n_rows),), SF, dtype=f64, device=dev),
             out=torch.full((P,), SF, dtype=f64, device=dev))
    w = torch.from_numpy(np.ascontiguousarray(weights)).to(dev)

    def targets(stop=None, **over):
        p = dict(track=rp.track, n_track=rp.n_track, weights=w, P=P, times=sorted(times), degree=degree, cycle_class=cycle_class, class_mask=class_mask, K=K,
                 a=b["a"], valid=b["valid"], fit=b["fit"], fit_doubles=b["fit"].numel())
        p.update(over)
        hip.replay_polyfit_targets(p["track"], p["n_track"], C, rp.L, p["weights"], p["P"], p["times"], p["degree"], rp.L + rp.I // 2, p["cycle_class"],
                                   p["class_mask"], p["K"], p["a"], p["valid"], p["fit"], p["fit_doubles"], stop)

    def objective(stop=None, cfg=None, kind=0, **over):
        p = dict(a=b["a"], valid=b["valid"], pos=b["pos"], move=b["move"], summary=b["summary"], scratch=b["scratch"], out=b["out"], n_cycles=C)
        p.update(over)
        hip.replay_objective(rp._cfg if cfg is None else cfg, hip.REPLAY_POLYFIT, P, p["n_cycles"], rp.track, rp.n_track, p["a"], None, p["valid"], rp._share,
                             p["pos"], p["move"], p["summary"], p["scratch"], b["scratch"].numel(), kind, p["out"], stop)

    def untouched(names=None):
        torch.cuda.synchronize()
        return all(bool((b[k] == (SI if b[k].dtype == i32 else SF)).all()) for k in (names or b))

    return b, w, targets, objective, untouched


def test_a_raised_stop_flag_leaves_every_output_untouched(torch_mod, pop):
    torch = torch_mod
    rp = pop["rp"]
    b, w, targets, objective, untouched = low_level(torch, rp, pop["weights"])
    dev, P, N = rp._dev, POP, 6
    ctrl = torch.tensor([1, 0, 0, 0], dtype=torch.int32, device=dev)
    targets(stop=ctrl)
    objective(stop=ctrl)
    state = {k: torch.full(shape, -12345.5, dtype=torch.float64, device=dev)
             for k, shape in dict(vel=(P, N), pbest_pos=(P, N), pbest_val=(P,), gbest_pos=(N,), gbest_val=(1,), history=(4,)).items()}
    w0 = w.clone()
    hip.polyfit_swarm_step(b["out"], torch.zeros((2, P, N), dtype=torch.float64, device=dev), P, N, 0, 5, 0.9, 2.05, 2.05, 0.0, 1.0, 0.5, w, state["vel"],
                           state["pbest_pos"], state["pbest_val"], state["gbest_pos"], state["gbest_val"], ctrl, state["history"])
    assert untouched()
    assert all(bool((t == -12345.5).all()) for t in state.values()) and torch.equal(w, w0) and ctrl.cpu().tolist() == [1, 0, 0, 0]
    ctrl.zero_()  # the flag down: the same calls write
    targets(stop=ctrl)
    objective(stop=ctrl)
    torch.cuda.synchronize()
    assert not untouched(["a"]) and not untouched(["valid"]) and not untouched(["pos"]) and bool((b["out"] != -12345.5).all()) and bool((b["summary"] != -12345.5).all())
    assert b["out"].cpu().numpy().tobytes() == np.asarray(pop["res"].summary.trimmed_mean_bbox_error).tobytes()


# ------------------------------------------------------------------------------------------------- 4. the swarm
@pytest.fixture(scope="module")
def search(pop):
    trace = []
    kw = dict(pop_size=POP, max_epoch=12, seed=3)
    first = pop["rp"].optimize_polyfit(2, TIMES, _trace=trace, **kw)
    return dict(first=first, trace=trace, kw=kw)


def objective_of(rp, w, degree=2, kind="trimmed_bbox_error"):
    return float(rp.objective(rp.polyfit_population(np.asarray(w, dtype=np.float64)[None, :], degree, TIMES), kind).cpu().numpy()[0])


def test_search_is_reproducible_and_follows_the_documented_rule(pop, search):
    from wtracker_amd.polyfit_opt import WeightEvaluator as WE

    rp, first, trace = pop["rp"], search["first"], search["trace"]
    again = rp.optimize_polyfit(2, TIMES, **search["kw"])
    assert bits(again.weights).tolist() == bits(first.weights).tolist() and bits([again.mae])[0] == bits([first.mae])[0]
    assert again.epochs == first.epochs == 12 and np.array_equal(bits(again.history), bits(first.history))
    # the numpy replay of the rule, fed the device's objective values, reproduces every position and velocity
    P, E, N, lb, ub, c1, c2 = POP, 12, 6, 0.0, 1.0, 2.05, 2.05
    rng = np.random.default_rng(3)
    x0 = lb + (ub - lb) * rng.random((P, N))
    x0[0, :] = ub
    rand = rng.random((E, 2, P, N))
    st = dict(pos=x0.copy(), vel=np.zeros((P, N)), pbest_pos=x0.copy(), pbest_val=np.full(P, np.inf), gbest_pos=x0[0].copy(), gbest_val=np.inf, since=0, history=[])
    assert len(trace) == E
    moved = 0
    for e, (pos, vel, value) in enumerate(trace):
        assert np.array_equal(bits(pos.cpu().numpy()), bits(st["pos"])), e
        assert np.array_equal(bits(vel.cpu().numpy()), bits(st["vel"])), e
        before = st["pos"].copy()
        assert not por.swarm_step(st, value.cpu().numpy(), rand[e], WE.W_MAX - (WE.W_MAX - WE.W_MIN) * e / E, c1, c2, lb, ub, 100)
        moved += int((st["pos"] != before).sum())
    assert moved > 3 * P * N
    assert np.array_equal(bits(first.history), bits(st["history"])) and bits([first.mae])[0] == bits([st["gbest_val"]])[0]
    assert np.array_equal(bits(first.weights), bits(st["gbest_pos"]))


def test_search_result_is_never_worse_than_its_starting_points(pop, search):
    rp, first = pop["rp"], search["first"]
    assert (np.diff(first.history) <= 0).all() and first.history[-1] == first.mae
    assert first.history[0] <= objective_of(rp, np.ones(6))  # particle 0 starts at the uniform weights
    w = pop["weights"][int(np.argmin(np.asarray(pop["res"].summary.trimmed_mean_bbox_error)))]
    seeded = rp.optimize_polyfit(2, TIMES, start=[w], **search["kw"])
    assert seeded.mae <= objective_of(rp, w) and seeded.history[0] <= objective_of(rp, w)
    early = rp.optimize_polyfit(2, TIMES, pop_size=POP, max_epoch=12, seed=3, max_early_stop=2)
    assert early.epochs < 12 and len(early.history) == early.epochs and (early.history[-2:] == early.history[-3]).all()


def test_search_result_is_re_evaluable_bit_for_bit(pop, search):
    rp, first = pop["rp"], search["first"]
    cfg = rp.to_config(2, first.weights)
    assert cfg.sample_times == sorted(TIMES) and cfg.degree == 2
    again = rp.run(rp.polyfit([cfg]), rows=[]).summary.trimmed_mean_bbox_error[0]
    assert bits([first.mae])[0] == bits([again])[0], (first.mae, again)


# ------------------------------------------------------------------------------------------------- 5. the host frame loop
def test_best_weights_against_the_host_frame_loop(pop, hard, tmp_path):
    """lb = 0.05: six non-zero weights and, by the fixture's construction (its NaN rows are never neighbours), at least 5 finite samples per cycle with
    its full history: no rank-deficient fit where the device's convention differs from the reference's.  The log of the best weights equals the
    Simulator + TrackLogger + PolyfitController (numpy's polyfit) frame loop in every row; no row is excepted.  The trimmed mean of
    calculate_bbox_error over the host log's kept rows equals result.mae within ceil(log2 R) 2^-53 sum|x| (section 15's bound of the tree sum)."""
    rp, tc = pop["rp"], pop["tc"]
    best = rp.optimize_polyfit(2, TIMES, pop_size=POP, max_epoch=12, seed=3, lb=0.05)
    assert (best.weights >= 0.05).all()
    cfg = rp.to_config(2, best.weights)
    tg = rp.polyfit([cfg])
    res = rp.run(tg, rows=[0])
    path = tmp_path / "hard.csv"
    with open(path, "w") as f:
        f.write("frame,wrm_x,wrm_y,wrm_w,wrm_h\n")
        for i, r in enumerate(hard["track"]):
            f.write(f"{i}," + ",".join("" if not np.isfinite(v) else repr(float(v)) for v in r) + "\n")
    ctrl = PolyfitController(tc, cfg, str(path))
    ctrl.track = hard["track"].copy()  # the fixture's own float64 values (the CSV parser is not round-trip exact)
    ctrl._table = np.vstack([ctrl.track, np.full((1, 4), np.nan)])
    log = TrackLogger(ctrl)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # numpy's RankWarning in the first cycles
        Simulator(tc, hard["ec"], log).run()
    mine = res.log(0)
    assert len(mine) == len(log.rows) == rp.n_rows
    a = tg.a.cpu().numpy()[:, 0]
    for m, h in zip(mine, log.rows):
        assert m["frame"] == h["frame"] and m["cycle"] == h["cycle"] and m["phase"] == h["phase"]
        for k in NUM_KEYS:
            if float(m[k]) != float(h[k]):
                c = max(m["cycle"] - (1 if k.startswith(("plt", "cam", "mic")) else 0), 0)  # the move that put the platform here was decided a cycle earlier
                start = res.row_array(0)[c * rp.L]
                v = [(a[c, q] - start[2 + q]) - start[4 + q] / 2 for q in (0, 1)]
                tie = [abs(abs(x - math.floor(x)) - 0.5) for x in v]
                raise AssertionError(f"row {m['frame']} column {k}: device {m[k]!r}, host {h[k]!r}; cycle {c}: move expression {v}, distance to the .5 tie {tie}")
    err, kept = ro.log_bbox_error(log.rows), ro.kept_rows(log.rows)
    x = err[kept]
    assert len(x) == int(res.summary.trimmed_rows[0]) and len(x) > 0
    bound = math.ceil(math.log2(rp.n_rows)) * 2.0 ** -53 * math.fsum(np.abs(x))  # of the device's sum against the exact sum of its rows
    s_dev, n = float(res.summary.trimmed_bbox_error_sum[0]), len(x)
    print(f"host trimmed mean {math.fsum(x) / n!r}, device {best.mae!r}; sums differ by {abs(s_dev - math.fsum(x)):.3g}, bound {bound:.3g}")
    assert bits([best.mae])[0] == bits([s_dev / n])[0]  # the search's value is this log's sum, divided once
    assert abs(s_dev - math.fsum(x)) <= bound
    # ... so the means differ by at most bound / n and the two divisions' roundings (half an ulp of the mean each)
    assert abs(best.mae - math.fsum(x) / n) <= bound / n + 2.0 ** -52 * abs(best.mae)


# ------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_touch_no_memory(torch_mod, pop, hard):
    torch = torch_mod
    rp = pop["rp"]
    b, w, targets, objective, untouched = low_level(torch, rp, pop["weights"])
    with pytest.raises(hip.WtkError):
        targets(times=list(range(-16, 1)))  # 17 sample times
    with pytest.raises(hip.WtkError):
        targets(times=[])
    for degree in (8, -1):
        with pytest.raises(hip.WtkError):
            targets(degree=degree)
    for P in (0, -1, 65536):
        with pytest.raises(hip.WtkError):
            targets(P=P)
    for name in ("track", "weights", "cycle_class", "class_mask", "a", "valid", "fit"):
        with pytest.raises(hip.WtkError):
            targets(**{name: None})
    with pytest.raises(hip.WtkError):
        targets(fit_doubles=b["fit"].numel() - 1)  # scratch one double too small
    for K in (0, rp.n_cycles + 1):
        with pytest.raises(hip.WtkError):
            targets(K=K)
    # the objective: what the scan and the rows step refuse, an unknown objective, the trimmed objective with fewer than 3 logged cycles
    for name in ("a", "valid", "pos", "move", "summary", "scratch", "out"):
        with pytest.raises(hip.WtkError):
            objective(**{name: None})
    for kind in (-1, 4):
        with pytest.raises(hip.WtkError):
            objective(kind=kind)
    short = hip.replay_config(2 * rp.L + 1, rp.I, rp.M, rp.P, rp.timing_config.camera_size_px, rp.timing_config.micro_size_px,
                              (rp.frame_shape[1], rp.frame_shape[0]), hard["ec"].init_position)  # 2 logged cycles
    with pytest.raises(hip.WtkError, match="3 logged cycles"):
        objective(cfg=short, n_cycles=2)
    assert untouched()
    objective(cfg=short, n_cycles=2, kind=hip.REPLAY_OBJECTIVES["bbox_error"])  # ... while the untrimmed mean of the same short experiment is served
    assert not untouched(["out"])
    b["out"].fill_(-12345.5), b["pos"].fill_(-77), b["move"].fill_(-77), b["summary"].fill_(-12345.5), b["scratch"].fill_(-12345.5)
    # the Python layer refuses the same before anything is enqueued
    ec = hard["ec"]
    rp_short, _ = replay_of(hard, ec=ExperimentConfig("short", 2 * rp.L + 1, ec.frames_per_sec, ec.orig_resolution, ec.px_per_mm, ec.init_position))
    assert rp_short.n_log == 2
    with pytest.raises(ValueError, match="at least 3"):
        rp_short.optimize_polyfit(2, TIMES, pop_size=4, max_epoch=2)
    with pytest.raises(ValueError, match="at least 3"):
        rp_short.objective(rp_short.polyfit_population(np.ones((2, 6)), 2, TIMES))
    for bad in (dict(pop_size=0), dict(max_epoch=0), dict(max_early_stop=0), dict(lb=1.0, ub=1.0), dict(start=np.ones((POP, 6))), dict(start=np.full((1, 6), 2.0))):
        with pytest.raises(ValueError):
            rp.optimize_polyfit(2, TIMES, **{**dict(pop_size=POP, max_epoch=2), **bad})
    with pytest.raises(ValueError):
        rp.optimize_polyfit(8, TIMES)
    with pytest.raises(ValueError):
        rp.polyfit_population(np.ones((3, 5)), 2, TIMES)  # five weights for six times
    assert untouched()
    targets()  # and the good calls go through
    objective()
    assert not untouched(["a"]) and not untouched(["out"])
