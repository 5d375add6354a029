"""wtracker_amd.replay.ReplaySet on the MI355X (csrc/replay_set.hip): a population replayed on several tracks in one call, with a
pooled objective.  The yardstick everywhere is the EXISTING path, one `Replay` per track and a host loop around them, compared bit for bit; it is never
the code under test.

The scenario (tests/test_replay_set_ref.py shows the layout's properties on it in numpy): three tracks with different frame shapes and init positions,
so that the clamp binds differently — tests/golden/replay_hard.npz (400 frames at 100 ms imaging: L = 5, 80 cycles), its first 137 frames translated
into a small frame (not a whole number of cycles, 27 logged cycles), and replay_ref.long_track with R = 4125 logged rows (one track crosses a reduction
chunk).  E = 70 crosses a wavefront."""
import dataclasses
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from harness import mlp_ref  # noqa: E402
from harness import mlp_train_ref as tr  # noqa: E402
from harness import replay_ref as rr  # noqa: E402
from wtracker_amd import hip  # noqa: E402
from wtracker_amd.controllers import PolyfitConfig  # noqa: E402
from wtracker_amd.sim import ExperimentConfig, TimingConfig  # noqa: E402

E, TIMES, DEGREE = 70, [-8, -6, -4, -2, 0, 1], 2
FIELDS = ("bbox_error_sum", "rows", "trimmed_bbox_error_sum", "trimmed_rows", "non_perfect_rows", "mse_error_sum")
OBJECTIVES = {"trimmed_bbox_error": (2, 3), "bbox_error": (0, 1), "mse_error": (5, 1), "non_perfect": (4, 1)}  # summary[num] / summary[den]
BUILDERS = ("csv", "optimal", "polyfit", "polyfit_population", "mlp", "mlp_population")


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same(x, y):
    """Bit equality of two arrays, NaN matching NaN."""
    x, y = np.asarray(x), np.asarray(y)
    if x.shape != y.shape:
        return False
    if x.dtype.kind != "f":
        return bool(np.array_equal(x, y))
    n = np.isnan(x)
    return bool(np.array_equal(n, np.isnan(y)) and np.array_equal(bits(x[~n]), bits(y[~n])))


def summary_array(s) -> np.ndarray:
    """A Summary as the float64 [E, 6] array the device holds."""
    return np.stack([np.asarray(getattr(s, f), dtype=np.float64) for f in FIELDS], axis=1)


@pytest.fixture(scope="module")
def scene(hip_lib, golden_dir):
    """The three tracks, their configs, the ReplaySet, and one plain Replay per track (the yardstick)."""
    import torch

    from wtracker_amd.replay import Replay, ReplaySet

    if hip.device_count() < 1:
        pytest.fail("no HIP device visible")
    z = np.load(os.path.join(golden_dir, "replay_hard.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    ec0 = ExperimentConfig("hard", meta["num_frames"], meta["frames_per_sec"], tuple(meta["orig_resolution"]), meta["px_per_mm"], tuple(meta["init_position"]))
    tc = TimingConfig(ec0, 100, 40, 50, meta["camera_size_mm"], meta["micro_size_mm"])
    tracks = [z["track"].copy(), z["track"][:137] + np.array([150.0, 250.0, 0.0, 0.0]), rr.long_track(4130, 5)]
    ecs = [ec0, dataclasses.replace(ec0, num_frames=137, init_position=(500, 120)), dataclasses.replace(ec0, num_frames=4130, init_position=(700, 600))]
    shapes = [None, (300, 400), (1400, 1400)]
    rs = ReplaySet(tracks, tc, ecs, shapes)
    per = [Replay(t, tc, ec, fs) for t, ec, fs in zip(tracks, ecs, shapes)]
    assert rs.T == 3 and rs.L == 5 and rs.n_cycles == [80, 27, 826] and rs.n_log == [79, 27, 825] and rs.n_rows == [395, 135, 4125]
    assert rs.reach == 64 and rs.guard_cycles == 13 and rs.cyc_off == [0, 93, 134]
    weights = np.random.default_rng(7).uniform(0.05, 1.0, size=(E, len(TIMES)))
    return dict(torch=torch, rs=rs, per=per, tracks=tracks, ecs=ecs, shapes=shapes, tc=tc, weights=weights, golden=golden_dir)


@pytest.fixture(scope="module")
def nets(scene):
    """E variants of the shipped 100 ms predictor (model 0 is the predictor itself) in one trainer: a population, and folded models one by one."""
    from wtracker_amd.training import HipMLPTrainer

    path = os.path.join(scene["golden"], "resmlp_100ms.npz")
    sd, acts = mlp_ref.fixture_network(path)
    z = np.load(path)
    rng = np.random.default_rng(5)
    models = []
    for e in range(E):
        m = {k: np.array(v) for k, v in sd.items()}
        if e:
            for k in m:
                if k.endswith(".0.weight") or k == "model.output.weight":
                    m[k] = (m[k] * rng.uniform(0.8, 1.2, size=m[k].shape)).astype(np.float32)
        models.append(dict(m, activations=acts, input_frames=z["input_frames"].tolist(), pred_frames=z["pred_frames"].tolist()))
    t = HipMLPTrainer(models, max_batch=2)
    yield t
    t.close()


def build(owner, name, scene, nets):
    """The targets of builder `name` on a ReplaySet or a Replay."""
    w = scene["weights"]
    if name == "csv":
        return owner.csv()
    if name == "optimal":
        return owner.optimal()
    if name == "polyfit":
        return owner.polyfit([PolyfitConfig(DEGREE, TIMES, [float(v) for v in row]) for row in w])
    if name == "polyfit_population":
        return owner.polyfit_population(w, DEGREE, TIMES)
    if name == "mlp":
        return owner.mlp(nets.folded(3))
    return owner.mlp_population(nets)


@pytest.fixture(scope="module")
def runs(scene, nets):
    """builder -> (set targets, ReplaySet.run's result, per track (targets, Replay.run's result)): computed once, read by several tests."""
    cache = {}

    def get(name):
        if name not in cache:
            rs, per = scene["rs"], scene["per"]
            tg = build(rs, name, scene, nets)
            alone = [build(rp, name, scene, nets) for rp in per]
            cache[name] = (tg, rs.run(tg), [(one, rp.run(one, rows=[])) for one, rp in zip(alone, per)])
        return cache[name]

    return get


# ------------------------------------------------------------------------------------------------- 1. every pair has the bits of its track alone
@pytest.mark.parametrize("name", BUILDERS)
def test_every_pair_equals_the_replay_of_its_track_alone(scene, runs, name):
    rs = scene["rs"]
    tg, res, alone = runs(name)
    n_exp = 1 if name in ("csv", "optimal", "mlp") else E
    assert tg.E == n_exp and len(res.moves) == 3
    for t, (one_tg, one) in enumerate(alone):
        sl = slice(rs.cyc_off[t], rs.cyc_off[t] + rs.n_cycles[t])
        if name != "csv":
            valid = tg.valid[sl].cpu().numpy()
            assert valid.shape == (rs.n_cycles[t], n_exp) and np.array_equal(valid, one_tg.valid.cpu().numpy()), (t, "valid")
            assert valid.any()
            for key in ("a", "b"):
                if getattr(tg, key) is not None:  # (b is only defined where valid is 1)
                    got, want = getattr(tg, key)[sl].cpu().numpy(), getattr(one_tg, key).cpu().numpy()
                    m = valid.astype(bool)
                    assert same(got[m], want[m]), (t, key)
        assert res.moves[t].shape == (n_exp, rs.n_cycles[t], 2) and res.moves[t].dtype == np.int32
        assert np.array_equal(res.moves[t], one.moves), (t, "moves")
        assert np.array_equal(res.positions[t], one.positions), (t, "positions")
        assert np.array_equal(bits(summary_array(res.track_summary[t])), bits(summary_array(one.summary))), (t, "summary")
    if n_exp == E:
        assert len({res.moves[0][e].tobytes() for e in range(E)}) > E // 2  # the experiments differ
    if name.startswith("polyfit"):  # the clamp binds on the far side in track 1's small frame only
        assert res.positions[1][..., 0].max() == 399 and res.positions[1][..., 1].max() <= 299 and res.positions[0][..., 0].max() > 399


# ------------------------------------------------------------------------------------------------- 2. pooling and objectives
def test_pooled_summary_and_objectives(scene, runs):
    rs, per = scene["rs"], scene["per"]
    tg, res, alone = runs("polyfit_population")
    pooled = np.zeros((E, 6))
    for _, one in alone:  # sequential float64 adds in track order from 0.0
        pooled = pooled + summary_array(one.summary)
    assert np.array_equal(bits(summary_array(res.summary)), bits(pooled))
    assert res.summary.rows.tolist() == [395 + 135 + 4125] * E and res.summary.trimmed_rows.tolist() == [3 * (77 + 25 + 823)] * E
    for kind, (num, den) in OBJECTIVES.items():
        got = rs.objective(tg, kind).cpu().numpy()
        assert got.shape == (E,) and same(got, pooled[:, num] / pooled[:, den]), kind
        each = rs.objective(tg, kind, per_track=True).cpu().numpy()
        assert each.shape == (3, E)
        for t, (one_tg, _) in enumerate(alone):
            assert same(each[t], per[t].objective(one_tg, kind).cpu().numpy()), (kind, t)
    got = rs.objective(tg).cpu().numpy()
    assert np.isfinite(got).all() and len(set(got.tolist())) > E // 2
    assert same(got, res.summary.trimmed_mean_bbox_error)  # the Summary's own division


# ------------------------------------------------------------------------------------------------- 3. T = 1
def test_one_track_equals_replay(scene):
    from wtracker_amd.replay import ReplaySet

    w = scene["weights"]
    for t in (0, 1):
        rp = scene["per"][t]
        one = ReplaySet([scene["tracks"][t]], scene["tc"], scene["ecs"][t], [scene["shapes"][t]])
        tg = one.polyfit_population(w, DEGREE, TIMES)
        want_tg = rp.polyfit_population(w, DEGREE, TIMES)
        for kind in OBJECTIVES:
            assert same(one.objective(tg, kind).cpu().numpy(), rp.objective(want_tg, kind).cpu().numpy()), (t, kind)
    # (`one` and `rp` are track 1's: 27 logged cycles)
    kw = dict(pop_size=24, max_epoch=5, seed=3, lb=0.05, start=[w[0]])
    a, b = one.optimize_polyfit(DEGREE, TIMES, **kw), rp.optimize_polyfit(DEGREE, TIMES, **kw)
    assert same(a.weights, b.weights) and same([a.mae], [b.mae]) and same(a.history, b.history) and a.epochs == b.epochs == 5


# ------------------------------------------------------------------------------------------------- 4. independence of E, T and the place in the set
def test_an_experiment_and_a_track_give_their_bits_anywhere(scene, runs):
    from wtracker_amd.replay import ReplaySet

    rs, w = scene["rs"], scene["weights"]
    tg, res, _ = runs("polyfit_population")
    full = rs.objective(tg, per_track=True).cpu().numpy()
    for e in (0, 63, 64, 69):  # both sides of the wave boundary
        alone = rs.run(rs.polyfit_population(w[e:e + 1], DEGREE, TIMES))
        for t in range(3):
            assert np.array_equal(alone.moves[t][0], res.moves[t][e]) and np.array_equal(alone.positions[t][0], res.positions[t][e])
            assert np.array_equal(bits(summary_array(alone.track_summary[t])[0]), bits(summary_array(res.track_summary[t])[e])), (e, t)
    pick = lambda idx: ReplaySet([scene["tracks"][i] for i in idx], scene["tc"], [scene["ecs"][i] for i in idx], [scene["shapes"][i] for i in idx])  # noqa: E731
    for idx in ([2, 0], [1, 2, 0, 1]):  # another place, other companions, a track twice
        other = pick(idx)
        got = other.objective(other.polyfit_population(w, DEGREE, TIMES), per_track=True).cpu().numpy()
        for k, i in enumerate(idx):
            assert same(got[k], full[i]), (idx, k)
    # a larger reach moves every track but changes no bit
    wide = ReplaySet(scene["tracks"], scene["tc"], scene["ecs"], scene["shapes"], reach=201)
    assert wide.guard_cycles == 41 and wide.cyc_off != rs.cyc_off
    assert same(wide.objective(wide.polyfit_population(w, DEGREE, TIMES), per_track=True).cpu().numpy(), full)


# ------------------------------------------------------------------------------------------------- 5. stop flag, refusals
def raw_objective(scene, tg, stop=None, table=None, objective=0, scratch_doubles=None, with_tracks=True):
    """wtk_replay_set_objective with sentinel-filled outputs -> (outputs, error or None)."""
    torch, rs = scene["torch"], scene["rs"]
    from wtracker_amd.replay import KINDS

    sp, table = rs._super, table or rs._table
    n, C = int(tg.E), rs.n_super_cycles
    f = lambda shape, dt: torch.full(shape, -7, dtype=dt, device="cuda")  # noqa: E731
    outs = [f((C, n, 2), torch.int32), f((C, n, 2), torch.int32), f((rs.T, n, 6), torch.float64), f((n, 6), torch.float64),
            f((max(1, hip.replay_set_scratch_doubles(rs._table, n)),), torch.float64), f((n,), torch.float64), f((rs.T, n), torch.float64)]
    err = None
    try:
        hip.replay_set_objective(sp._cfg, table, KINDS[tg.kind], n, sp.track, tg.a, tg.b, tg.valid, sp._share, outs[0], outs[1], outs[2], outs[3], outs[4],
                                 outs[4].numel() if scratch_doubles is None else scratch_doubles, objective, outs[5], outs[6] if with_tracks else None, stop,
                                 stream=torch.cuda.current_stream().cuda_stream)
    except hip.WtkError as e:
        err = str(e)
    torch.cuda.synchronize()
    return outs, err


def untouched(outs):
    return all(bool((o == -7).all()) for o in outs)


def test_a_raised_stop_flag_leaves_every_output_untouched(scene, runs):
    torch = scene["torch"]
    tg, res, _ = runs("polyfit_population")
    outs, err = raw_objective(scene, tg, stop=torch.ones((1,), dtype=torch.int32, device="cuda"))
    assert err is None and untouched(outs)
    outs, err = raw_objective(scene, tg, stop=torch.zeros((1,), dtype=torch.int32, device="cuda"))
    assert err is None and not untouched(outs[:4]) and not untouched(outs[5:])
    assert same(outs[5].cpu().numpy(), res.summary.trimmed_mean_bbox_error)
    assert np.array_equal(bits(outs[3].cpu().numpy()), bits(summary_array(res.summary)))


def edited_table(scene, t, **fields):
    """The set's table with fields of entry t replaced (host and device copies alike)."""
    rs = scene["rs"]
    rows = []
    for k, (rp, off) in enumerate(zip(scene["per"], rs.cyc_off)):
        rows.append(dict(cyc_off=off, n_track=rp.n_track, num_frames=int(rp.experiment_config.num_frames), n_cycles=rp.n_cycles, n_log=rp.n_log,
                         frame_wh=(rp.frame_shape[1], rp.frame_shape[0]), init_position=rp.experiment_config.init_position))
    table = hip.ReplaySetTable(rows, rs.L, rs.guard_cycles, rs.n_super_cycles * rs.L)
    for k, v in fields.items():
        setattr(table.host[t], k, v)
    table.dev = scene["torch"].from_numpy(np.frombuffer(bytes(table.host), dtype=np.uint8).copy()).cuda()
    return table


def test_entry_point_refusals_touch_no_memory(scene, runs):
    rs = scene["rs"]
    tg, _, _ = runs("polyfit_population")
    base = edited_table(scene, 0)
    outs, err = raw_objective(scene, tg, table=base)
    assert err is None and not untouched(outs[:4])
    empty = hip.ReplaySetTable([], rs.L, rs.guard_cycles, rs.n_super_cycles * rs.L)
    empty.dev = base.dev
    cases = [
        (dict(table=empty), "at least one track"),
        (dict(table=edited_table(scene, 1, n_track=100)), "track 1: the track is shorter than the logged rows"),
        (dict(table=edited_table(scene, 2, cyc_off=rs.cyc_off[2] - 1)), "track 2: its slot overlaps"),
        (dict(table=edited_table(scene, 2, cyc_off=rs.cyc_off[2] + 1)), "track 2: its slot and guard end beyond the super-track"),
        (dict(table=edited_table(scene, 1, chunk0=0)), "track 1: chunk0"),
        (dict(table=edited_table(scene, 1, n_log=26)), "track 1: n_log and R"),
        (dict(table=edited_table(scene, 1, init_x=400)), "track 1: the init position"),
        (dict(objective=9), "unknown objective"),
        (dict(scratch_doubles=hip.replay_set_scratch_doubles(rs._table, E) - 1), "scratch smaller"),
    ]
    for kw, msg in cases:
        outs, err = raw_objective(scene, tg, **kw)
        assert err is not None and msg in err, (kw, err)
        assert untouched(outs), msg
    assert hip.replay_set_scratch_doubles(rs._table, E) == E * (1 + 1 + 2) * 6


def test_refusals(scene, runs, nets):
    from wtracker_amd.replay import Analysis, ReplaySet

    rs, tc, ec0 = scene["rs"], scene["tc"], scene["ecs"][0]
    tg, _, alone = runs("polyfit_population")
    with pytest.raises(ValueError, match="at least one track"):
        ReplaySet([], tc, ec0)
    with pytest.raises(ValueError, match="the track has 100 rows"):
        ReplaySet([scene["tracks"][0], scene["tracks"][0][:100]], tc, ec0)
    with pytest.raises(ValueError, match="experiment_configs must be one config or 2"):
        ReplaySet(scene["tracks"][:2], tc, scene["ecs"])
    # a track of 2 logged cycles: the plain objectives run, the trimmed one is refused by name, on the host and in the entry point
    two = ReplaySet([scene["tracks"][0], scene["tracks"][0][:40]], tc, [ec0, dataclasses.replace(ec0, num_frames=11)])
    assert two.n_log == [79, 2]
    tg2 = two.polyfit_population(scene["weights"][:3], DEGREE, TIMES)
    assert np.isfinite(two.objective(tg2, "bbox_error").cpu().numpy()).all()
    with pytest.raises(ValueError, match="track 1 logs 2"):
        two.objective(tg2, "trimmed_bbox_error")
    with pytest.raises(ValueError, match="track 1 logs 2"):
        two.optimize_polyfit(DEGREE, TIMES, pop_size=4, max_epoch=1)
    sp, buf = two._super, two._objective_buffers(3)
    with pytest.raises(hip.WtkError, match="at least 3 logged cycles of every track"):
        hip.replay_set_objective(sp._cfg, two._table, hip.REPLAY_POLYFIT, 3, sp.track, tg2.a, None, tg2.valid, sp._share, buf["pos"], buf["move"], buf["track_summary"],
                                 buf["summary"], buf["scratch"], buf["scratch"].numel(), 0, buf["summary"][:, 0].contiguous())
    # beyond the reach
    with pytest.raises(ValueError, match="sample_times lie up to 65 frames .* reach = 64"):
        rs.polyfit_population(scene["weights"], DEGREE, [-65, -6, -4, -2, 0, 1])
    with pytest.raises(ValueError, match="reach = 64"):
        rs.polyfit([PolyfitConfig(1, [-3, 0, 70], None)])
    with pytest.raises(ValueError, match="reach = 64"):
        rs.optimize_polyfit(1, [-80, 0])
    narrow = ReplaySet(scene["tracks"][:2], tc, scene["ecs"][:2], scene["shapes"][:2], reach=10)
    with pytest.raises(ValueError, match="input_frames lie up to .* reach = 10"):
        narrow.mlp_population(nets)
    with pytest.raises(ValueError, match="input_frames lie up to .* reach = 10"):
        narrow.mlp(nets.folded(0))
    # precise, analysis, foreign targets
    with pytest.raises(ValueError, match=r"rs\.replay\(t\)"):
        rs.objective(tg, "trimmed_precise_error")
    with pytest.raises(ValueError, match=r"rs\.replay\(t\)"):
        rs.run(tg, precise=True)
    with pytest.raises(ValueError, match=r"rs\.replay\(t\)"):
        rs.run(tg, analysis=Analysis())
    with pytest.raises(ValueError, match="unknown objective"):
        rs.objective(tg, "nope")
    with pytest.raises(ValueError, match="targets must be contiguous"):
        rs.objective(alone[0][0])  # a plain Replay's targets
    with pytest.raises(ValueError, match="targets must be contiguous"):
        rs.run(narrow.polyfit_population(scene["weights"], DEGREE, TIMES))  # another set's
    assert rs.replay(1).n_rows == 135 and rs.replay(1).frame_shape == (300, 400)


# ------------------------------------------------------------------------------------------------- 6. the search
def test_optimize_polyfit_on_the_set(scene):
    rs = scene["rs"]
    start = scene["weights"][:2]
    kw = dict(pop_size=30, max_epoch=6, seed=11, lb=0.05, start=start)
    a, b = rs.optimize_polyfit(DEGREE, TIMES, **kw), rs.optimize_polyfit(DEGREE, TIMES, **kw)
    assert same(a.weights, b.weights) and a.mae == b.mae and same(a.history, b.history)
    began = rs.objective(rs.polyfit_population(start, DEGREE, TIMES)).cpu().numpy()
    assert a.mae <= began.min() and (np.diff(a.history) <= 0).all()
    again = rs.objective(rs.polyfit([rs.to_config(DEGREE, a.weights)])).cpu().numpy()
    assert again.shape == (1,) and bits(again[0]) == bits(a.mae)
    print(f"\n[replay_set] pooled trimmed bbox error: start {began.tolist()}, after {a.epochs} epochs {a.mae!r}")


# ------------------------------------------------------------------------------------------------- 7. the trainer's closed loop
def test_fit_scores_every_epoch_on_the_set(scene):
    """Two epochs, three small models: FitResult.closed_loop holds rs.objective of the folded states of a second trainer stepped epoch by epoch."""
    from test_gpu_mlp_population import _models
    from wtracker_amd.training import HipMLPTrainer

    torch, rs = scene["torch"], scene["rs"]
    n_models, n, n_test, epochs = 3, 57, 38, 2
    _, _, X, y = tr.make_case(mlp_ref.arch_args("one-slice-edge"), n + n_test, 730)
    X, y = torch.from_numpy(np.array(X)).cuda(), torch.from_numpy(np.array(y) * 0.1).cuda()
    Xtr, ytr, Xte, yte = X[:n].contiguous(), y[:n].contiguous(), X[n:].contiguous(), y[n:].contiguous()

    def order(epoch):
        return torch.stack([torch.randperm(n, generator=torch.Generator().manual_seed(100 * epoch + e)) for e in range(n_models)]).to(torch.int32)

    make = lambda: HipMLPTrainer(_models("one-slice-edge", n_models, seed0=740), max_batch=19, lr=1e-3)  # noqa: E731
    t1, t2 = make(), make()
    r1 = t1.fit(Xtr, ytr, Xte, yte, epochs, batch_size=19, order=order, closed_loop=rs)
    slow = np.zeros((epochs, n_models))
    for ep in range(epochs):
        t2.train_epoch(Xtr, ytr, order(ep), 19)
        t2.test_epoch(Xte, yte, 19, track_best=True, reset_best=ep == 0)
        slow[ep] = rs.objective(rs.mlp_population([t2.folded(e) for e in range(n_models)])).cpu().numpy()
    assert np.isfinite(slow).all()
    for e in range(n_models):
        assert r1[e].closed_loop == [float(v) for v in slow[:, e]]
    best, has = t1.scores()
    assert has.tolist() == [1] * n_models and best.tolist() == slow.min(axis=0).tolist()
    assert rs.objective(rs.mlp_population(t1, which="scored")).cpu().numpy().tolist() == best.tolist()
    t1.close(), t2.close()
