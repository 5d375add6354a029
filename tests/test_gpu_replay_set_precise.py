"""The precise error of a population on a SET of tracks on the MI355X (the replay_set_precise kernels of csrc/replay_set.hip).  The
yardstick everywhere is the EXISTING path, `rs.replay(t)` with the same frames attached (wtk_replay_precise on one track), compared bit for bit, together
with the numpy harness (tests/harness/replay_set_precise_ref.py, pinned by tests/test_replay_set_precise_ref.py); it is never the code under test.

The scene: four tracks with different frame shapes, one timing (I = 4, M = 2, P = 1), camera (40, 32), microscope (14, 10): scenario_main (answered by the
table), scenario_ulp (the one-pixel grow and shrink rows), a 210 x 210 box on 256 x 256 frames (every pair walks), and 4104 rows on 48 x 64 frames (two
reduction chunks inside one track).  E = 70 crosses a wavefront; one case runs E = 300 on the first three tracks."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from harness import mlp_ref  # noqa: E402
from harness import mlp_train_ref as tr  # noqa: E402
from harness import replay_set_precise_ref as sp  # noqa: E402
from wtracker_amd import hip  # noqa: E402
from wtracker_amd.sim import ExperimentConfig, TimingConfig  # noqa: E402

E = 70
CHECKED = (0, 63, 64, 69)  # the experiments of the long track the harness is run for
TIMES, DEGREE = [-4, -2, 0, 1, 3], 2
FIELDS = ("precise_error_sum", "rows", "trimmed_precise_error_sum", "trimmed_rows", "non_perfect_rows", "nan_rows")


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
    """A PreciseSummary as the float64 [E, 6] array the device holds."""
    return np.stack([np.asarray(getattr(s, f), dtype=np.float64) for f in FIELDS], axis=1)


def make_set(torch, sn, attach=True, thresholds=None, frames=None):
    """The ReplaySet of a harness scene; `frames`: device frames per track to reuse."""
    from wtracker_amd.replay import ReplaySet

    ecs = [ExperimentConfig("scenario", g.num_frames, 1000, sc["frame_shape"], 1, g.init) for sc, g in zip(sn["tracks"], sn["geoms"])]
    g0 = sn["geoms"][0]
    tc = TimingConfig(ecs[0], g0.I, g0.P, g0.M, g0.cam, g0.mic)
    rs = ReplaySet([torch.from_numpy(sc["track"]) for sc in sn["tracks"]], tc, ecs, [sc["frame_shape"] for sc in sn["tracks"]])
    assert rs.reach == sp.REACH and rs.cyc_off == sn["st"].cyc_off and rs.n_rows == sn["R"] and rs.n_super_cycles == sn["st"].n_cycles
    if attach:
        frames = [torch.from_numpy(sc["frames"]).cuda() for sc in sn["tracks"]] if frames is None else frames
        rs.attach_frames(frames, [sc["bg"] for sc in sn["tracks"]], 20 if thresholds is None else thresholds)
    return rs


def targets_of(torch, sn, experiments=None):
    from wtracker_amd.replay import Targets

    a, valid = sn["a"], sn["valid"]
    if experiments is not None:
        a, valid = a[:, list(experiments)], valid[:, list(experiments)]
    return Targets("optimal", a.shape[1], torch.from_numpy(np.ascontiguousarray(a)).cuda(), None, torch.from_numpy(np.ascontiguousarray(valid)).cuda())


def slice_of(rs, tg, t):
    """Track t's cycles of a set's targets, as targets of rs.replay(t)."""
    from wtracker_amd.replay import Targets

    sl = slice(rs.cyc_off[t], rs.cyc_off[t] + rs.n_cycles[t])
    return Targets(tg.kind, tg.E, tg.a[sl].contiguous(), None, tg.valid[sl].contiguous())


def loop_form(rs, tg, **kw):
    """The existing path: one rs.replay(t).run per track."""
    return [rs.replay(t).run(slice_of(rs, tg, t), rows=[], per_row_errors=True, precise=True, **kw) for t in range(rs.T)]


def assert_tracks_equal(res, per, what=""):
    for t, one in enumerate(per):
        assert res.precise_counts[t].dtype == np.int32 and res.precise_error[t].dtype == np.float64
        assert np.array_equal(res.precise_counts[t], one.precise_counts), (what, t, np.argwhere(res.precise_counts[t] != one.precise_counts)[:5])
        assert same(res.precise_error[t], one.precise_error), (what, t)
        assert np.array_equal(bits(summary_array(res.track_precise_summary[t])), bits(summary_array(one.precise_summary))), (what, t)
        assert np.array_equal(res.moves[t], one.moves) and np.array_equal(res.positions[t], one.positions), (what, t)


def pooled_of(per_summaries) -> np.ndarray:
    pooled = np.zeros_like(per_summaries[0])
    for s in per_summaries:
        pooled = pooled + s
    return pooled


@pytest.fixture(scope="module")
def torch_mod(hip_lib):
    import torch

    if hip.device_count() < 1:
        pytest.fail("no HIP device visible")
    return torch


@pytest.fixture(scope="module")
def main(torch_mod):
    """The scene, its ReplaySet with frames, the set's run of all 70 experiments and the loop form of the same: computed once, never modified."""
    sn = sp.scene(E)
    rs = make_set(torch_mod, sn)
    tg = targets_of(torch_mod, sn)
    res = rs.run(tg, precise=True, per_row_errors=True)
    return dict(sn=sn, rs=rs, tg=tg, res=res, per=loop_form(rs, tg), plain=rs.run(tg), frames=[rp._frames for rp in rs._replays])


# ------------------------------------------------------------------------------------------------- 1. run
def test_every_pair_has_the_bits_of_its_track_alone(main):
    sn, rs, res, per = main["sn"], main["rs"], main["res"], main["per"]
    assert [e.shape for e in res.precise_error] == [(E, r) for r in sn["R"]] and [c.shape for c in res.precise_counts] == [(E, r, 2) for r in sn["R"]]
    assert_tracks_equal(res, per, "E = 70")
    assert np.array_equal(bits(summary_array(res.precise_summary)), bits(pooled_of([summary_array(one.precise_summary) for one in per])))
    # precise=True changes nothing else
    for t in range(rs.T):
        assert np.array_equal(res.moves[t], main["plain"].moves[t]) and np.array_equal(res.positions[t], main["plain"].positions[t])
    assert main["plain"].precise_summary is None and main["plain"].precise_error is None


def test_the_run_equals_the_harness(main):
    sn, res = main["sn"], main["res"]
    pos, move = sp.scan_of(sn)
    for t in (0, 1, 2):
        want = sp.track_alone(sn, t, pos, move)
        if t == 0:
            assert want["stats"]["table"] > 0 and want["stats"]["frame_walk"] == 0
        if t == 2:
            assert want["stats"]["frame_walk"] > 0
        assert np.array_equal(res.precise_counts[t], want["counts"]) and same(res.precise_error[t], want["err"]), t
        assert np.array_equal(bits(summary_array(res.track_precise_summary[t])), bits(want["summary"])), t
    pos, move = sp.scan_of(sn, CHECKED)  # the long track: the checked experiments (every experiment is checked against rs.replay(3) above)
    want = sp.track_alone(sn, 3, pos, move)
    assert (want["summary"][:, 5] > 100).all()  # NaN rows
    got = summary_array(res.track_precise_summary[3])[list(CHECKED)]
    assert np.array_equal(res.precise_counts[3][list(CHECKED)], want["counts"]) and same(res.precise_error[3][list(CHECKED)], want["err"])
    assert np.array_equal(bits(got), bits(want["summary"])), (got, want["summary"])


# ------------------------------------------------------------------------------------------------- 2. objectives
@pytest.mark.parametrize("kind", sorted(sp.OBJECTIVE_SLOTS))
def test_objectives_pooled_and_per_track(torch_mod, main, kind):
    rs, tg, res = main["rs"], main["tg"], main["res"]
    num, den = sp.OBJECTIVE_SLOTS[kind]
    pooled = summary_array(res.precise_summary)
    with np.errstate(invalid="ignore"):
        assert same(rs.objective(tg, kind).cpu().numpy(), pooled[:, num] / pooled[:, den])
    each = rs.objective(tg, kind, per_track=True).cpu().numpy()
    assert each.shape == (rs.T, E)
    for t in range(rs.T):
        assert same(each[t], rs.replay(t).objective(slice_of(rs, tg, t), kind).cpu().numpy()), t
    name = {"trimmed_precise_error": "trimmed_mean_precise_error", "precise_error": "mean_precise_error", "precise_non_perfect": "non_perfect"}[kind]
    assert same(getattr(res.precise_summary, name), pooled[:, num] / pooled[:, den])


def test_one_track_gives_replays_bits(torch_mod, main):
    sn1 = sp.scene(E, which=(0,))
    rs1 = make_set(torch_mod, sn1, frames=main["frames"][:1])
    tg1 = targets_of(torch_mod, sn1)
    for kind in sp.OBJECTIVE_SLOTS:
        want = rs1.replay(0).objective(slice_of(rs1, tg1, 0), kind).cpu().numpy()
        assert same(rs1.objective(tg1, kind).cpu().numpy(), want) and same(rs1.objective(tg1, kind, per_track=True).cpu().numpy()[0], want), kind


# ------------------------------------------------------------------------------------------------- 3. independence
def test_bits_do_not_depend_on_the_population_or_the_set(torch_mod, main):
    sn, rs, res = main["sn"], main["rs"], main["res"]
    again = rs.run(main["tg"], precise=True, per_row_errors=True)  # the call made twice
    assert_tracks_equal(again, main["per"], "twice")
    assert np.array_equal(bits(summary_array(again.precise_summary)), bits(summary_array(res.precise_summary)))
    for e in (0, 64):  # one experiment alone
        alone = rs.run(targets_of(torch_mod, sn, [e]), precise=True, per_row_errors=True)
        for t in range(rs.T):
            assert np.array_equal(alone.precise_counts[t][0], res.precise_counts[t][e]) and same(alone.precise_error[t][0], res.precise_error[t][e]), (e, t)
            assert np.array_equal(bits(summary_array(alone.track_precise_summary[t])), bits(summary_array(res.track_precise_summary[t])[e:e + 1])), (e, t)
        assert np.array_equal(bits(summary_array(alone.precise_summary)), bits(summary_array(res.precise_summary)[e:e + 1])), e
    # a track at another index of the set, with other companions
    for which in ((2, 0, 1), (1, 3)):
        sn2 = sp.scene(E, which=which)
        rs2 = make_set(torch_mod, sn2, frames=[main["frames"][i] for i in which])
        other = rs2.run(targets_of(torch_mod, sn2), precise=True, per_row_errors=True)
        for at, t in enumerate(which):
            assert np.array_equal(other.precise_counts[at], res.precise_counts[t]) and same(other.precise_error[at], res.precise_error[t]), (which, t)
            assert np.array_equal(bits(summary_array(other.track_precise_summary[at])), bits(summary_array(res.track_precise_summary[t]))), (which, t)


def test_a_population_beyond_the_block(torch_mod):
    """E = 300 on the first three tracks: phase 2 strides over the experiments 256 threads at a time."""
    sn = sp.scene(300, which=(0, 1, 2))
    rs = make_set(torch_mod, sn)
    tg = targets_of(torch_mod, sn)
    res = rs.run(tg, precise=True, per_row_errors=True)
    assert_tracks_equal(res, loop_form(rs, tg), "E = 300")
    pos, move = sp.scan_of(sn)
    for t in range(3):
        want = sp.track_alone(sn, t, pos, move)
        assert np.array_equal(res.precise_counts[t], want["counts"]) and same(res.precise_error[t], want["err"]), t
        assert np.array_equal(bits(summary_array(res.track_precise_summary[t])), bits(want["summary"])), t
    assert np.array_equal(bits(summary_array(res.precise_summary)), bits(pooled_of([summary_array(s) for s in res.track_precise_summary])))


# ------------------------------------------------------------------------------------------------- 4. the table limit
def test_forced_fallback_changes_nothing(main):
    """`_max_crop_px` = 64 keeps the table for the 1 x 1 crop's frame only: the direct walk and the table agree in every pair of every track."""
    res = main["rs"].run(main["tg"], precise=True, per_row_errors=True, _max_crop_px=64)
    assert_tracks_equal(res, main["per"], "limit 64")
    assert np.array_equal(bits(summary_array(res.precise_summary)), bits(summary_array(main["res"].precise_summary)))


# ------------------------------------------------------------------------------------------------- 5. per-track thresholds
def test_per_track_thresholds(torch_mod, main):
    sn = sp.scene(E, thresholds=sp.THRESHOLDS)
    rs = make_set(torch_mod, sn, thresholds=sp.THRESHOLDS, frames=main["frames"])
    assert [rs.replay(t)._diff_thresh for t in range(4)] == [20.0, 35.0, 20.0, 5.0]
    tg = targets_of(torch_mod, sn)
    res = rs.run(tg, precise=True, per_row_errors=True)
    assert_tracks_equal(res, loop_form(rs, tg), "thresholds")
    # the noise frames of track 1 segment differently at 35 (the painted frames of the others are far from their background: any threshold segments them alike)
    assert not np.array_equal(res.precise_counts[1], main["res"].precise_counts[1]) and np.array_equal(res.precise_counts[0], main["res"].precise_counts[0])
    pos, move = sp.scan_of(sn)
    want = sp.track_alone(sn, 1, pos, move)
    assert np.array_equal(res.precise_counts[1], want["counts"]) and same(res.precise_error[1], want["err"])


# ------------------------------------------------------------------------------------------------- 6. the stop flag
def test_a_raised_stop_flag_leaves_every_output_untouched(torch_mod, main):
    torch, rs, tg = torch_mod, main["rs"], main["tg"]
    sp_, rows = rs._super, sum(rs.n_rows)
    buf = rs._objective_buffers(E, True)
    for k in ("track_summary", "summary", "scratch", "pos", "move"):
        buf[k].fill_(-7)
    obj, tobj = torch.full((E,), -7.0, dtype=torch.float64, device="cuda"), torch.full((rs.T, E), -7.0, dtype=torch.float64, device="cuda")
    err = torch.full((E, rows), -7.0, dtype=torch.float64, device="cuda")
    counts = torch.full((E, rows, 2), -7, dtype=torch.int32, device="cuda")
    stop = torch.ones(1, dtype=torch.int32, device="cuda")
    rs._enqueue_objective(tg, 0, buf, obj, tobj, stop_dev=stop)
    hip.replay_set_precise(sp_._cfg, rs._table, rs._frames_table, E, sp_.track, sp_._share, buf["pos"], buf["move"], 0, err, counts, buf["track_summary"], buf["summary"], buf["scratch"], buf["scratch"].numel(), stop_dev=stop)
    torch.cuda.synchronize()
    for name, x in (("objective", obj), ("track objective", tobj), ("err", err), ("counts", counts), ("track_summary", buf["track_summary"]),
                    ("summary", buf["summary"]), ("scratch", buf["scratch"]), ("pos", buf["pos"]), ("move", buf["move"])):
        assert bool((x == -7).all()), name
    stop.zero_()  # and with the flag down the same call computes
    rs._enqueue_objective(tg, 0, buf, obj, tobj, stop_dev=stop)
    assert same(obj.cpu().numpy(), main["res"].precise_summary.trimmed_mean_precise_error)


# ------------------------------------------------------------------------------------------------- 7. the search
def test_optimize_polyfit_with_the_precise_objective(torch_mod, main):
    rs = main["rs"]
    kw = dict(objective="trimmed_precise_error", pop_size=20, max_epoch=5, seed=0)
    best = rs.optimize_polyfit(DEGREE, TIMES, **kw)
    again = rs.run(rs.polyfit([rs.to_config(DEGREE, best.weights)]), precise=True).precise_summary.trimmed_mean_precise_error
    assert again.shape == (1,) and np.isfinite(best.mae) and bits(again[0]) == bits(best.mae)
    assert (np.diff(best.history) <= 0).all()
    print(f"\n[replay_set precise] pooled trimmed precise error after {best.epochs} epochs: {best.mae!r}")
    sn1 = sp.scene(E, which=(0,))
    rs1 = make_set(torch_mod, sn1, frames=main["frames"][:1])
    a, b = rs1.optimize_polyfit(DEGREE, TIMES, **kw), rs1.replay(0).optimize_polyfit(DEGREE, TIMES, **kw)
    assert same(a.weights, b.weights) and bits(a.mae) == bits(b.mae) and same(a.history, b.history)


# ------------------------------------------------------------------------------------------------- 8. the trainer's closed loop
def test_fit_scores_every_epoch_with_the_precise_objective(torch_mod, main):
    """Two epochs, three small models: FitResult.closed_loop holds rs.objective(..., "trimmed_precise_error") of the folded states of a second trainer
    stepped epoch by epoch."""
    from test_gpu_mlp_population import _models
    from wtracker_amd.training import HipMLPTrainer

    torch, rs, kind = torch_mod, main["rs"], "trimmed_precise_error"
    n_models, n, n_test, epochs = 3, 57, 38, 2
    _, _, X, y = tr.make_case(mlp_ref.arch_args("one-slice-edge"), n + n_test, 730)
    X, y = torch.from_numpy(np.array(X)).cuda(), torch.from_numpy(np.array(y) * 0.1).cuda()
    Xtr, ytr, Xte, yte = X[:n].contiguous(), y[:n].contiguous(), X[n:].contiguous(), y[n:].contiguous()

    def order(epoch):
        return torch.stack([torch.randperm(n, generator=torch.Generator().manual_seed(100 * epoch + e)) for e in range(n_models)]).to(torch.int32)

    make = lambda: HipMLPTrainer(_models("one-slice-edge", n_models, seed0=740), max_batch=19, lr=1e-3)  # noqa: E731
    t1, t2 = make(), make()
    r1 = t1.fit(Xtr, ytr, Xte, yte, epochs, batch_size=19, order=order, closed_loop=rs, closed_loop_objective=kind)
    slow = np.zeros((epochs, n_models))
    for ep in range(epochs):
        t2.train_epoch(Xtr, ytr, order(ep), 19)
        t2.test_epoch(Xte, yte, 19, track_best=True, reset_best=ep == 0)
        slow[ep] = rs.objective(rs.mlp_population([t2.folded(e) for e in range(n_models)]), kind).cpu().numpy()
    assert np.isfinite(slow).all()
    for e in range(n_models):
        assert r1[e].closed_loop == [float(v) for v in slow[:, e]]
    t1.close(), t2.close()


# ------------------------------------------------------------------------------------------------- 9. refusals
def test_refusals(torch_mod, main):
    from wtracker_amd.replay import Analysis

    torch, sn, tg, frames = torch_mod, main["sn"], main["tg"], main["frames"]
    bgs = [sc["bg"] for sc in sn["tracks"]]
    bare = make_set(torch, sn, attach=False)
    for call in (lambda: bare.objective(tg, "trimmed_precise_error"), lambda: bare.run(tg, precise=True),
                 lambda: bare.optimize_polyfit(DEGREE, TIMES, objective="precise_error", pop_size=4, max_epoch=1)):
        with pytest.raises(ValueError, match=r"rs\.attach_frames.*rs\.replay\(t\)"):
            call()
    with pytest.raises(ValueError, match="must hold 4 entries"):
        bare.attach_frames(frames[:3], bgs[:3])
    with pytest.raises(ValueError, match="must hold 4 entries"):
        bare.attach_frames(frames, bgs, [20, 20])
    with pytest.raises(ValueError, match="track 1: the frames are 96 x 131"):
        bare.attach_frames([frames[0], frames[0], frames[2], frames[3]], bgs)
    with pytest.raises(ValueError, match="track 3: 4000 frames, the log has 4104 rows"):
        bare.attach_frames(frames[:3] + [frames[3][:4000]], bgs)
    with pytest.raises(ValueError, match="track 2: the frames must be a tensor on the set's device"):
        bare.attach_frames(frames[:2] + [frames[2].cpu()] + frames[3:], bgs)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError, match="track 0: the frames must be a tensor on the set's device"):
            bare.attach_frames([frames[0].to("cuda:1")] + frames[1:], bgs)
    with pytest.raises(ValueError, match="track 1: diff_thresh must be finite"):
        bare.attach_frames(frames, bgs, [20, float("nan"), 20, 20])
    with pytest.raises(ValueError, match=r"rs\.attach_frames"):  # no refusal above left a table behind
        bare.run(tg, precise=True)
    with pytest.raises(ValueError, match=r"rs\.replay\(t\)"):
        main["rs"].run(tg, analysis=Analysis())
    with pytest.raises(ValueError, match="unknown objective"):
        main["rs"].objective(tg, "nope")
