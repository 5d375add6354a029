"""The precise tracking error of a replayed population on the MI355X (replay_precise_kernel of csrc/replay_precise.hip) against its numpy
restatement (tests/harness/replay_precise_ref.py, pinned by tests/test_replay_precise_ref.py to the real reference) and against the per-row kernel that
was there before (evaluation.precise_error_from_log on the replayed log)."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from harness import eval_ref as ev  # noqa: E402
from harness import replay_precise_ref as pr  # noqa: E402
from wtracker_amd import hip  # noqa: E402
from wtracker_amd.sim import ExperimentConfig, TimingConfig  # noqa: E402

CHECKED = (0, 63, 64, 69)
TIMES = [-4, -2, 0, 1, 3]
W0 = [0.2, 0.4, 0.6, 0.8, 1.0]


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


@pytest.fixture(scope="module")
def torch_mod(hip_lib):
    import torch

    if hip.device_count() < 1:
        pytest.fail("no HIP device visible")
    return torch


def configs(sc):
    """1 ms per frame and 1 px per mm: the scenario's frame counts and pixel sizes are the configs' own numbers."""
    g = sc["g"]
    ec = ExperimentConfig("scenario", g.num_frames, 1000, sc["frame_shape"], 1, g.init)
    return TimingConfig(ec, g.I, g.P, g.M, g.cam, g.mic), ec


def make_replay(torch, sc, attach=True, frames=None, bg=None, thr=20):
    from wtracker_amd.replay import Replay

    tc, ec = configs(sc)
    rp = Replay(torch.from_numpy(sc["track"]), tc, ec, frame_shape=sc["frame_shape"])
    assert (rp.L, rp.I, rp.M, rp.P, rp.n_rows) == (sc["g"].L, sc["g"].I, sc["g"].M, sc["g"].P, sc["g"].n_log * sc["g"].L)
    if attach:
        rp.attach_frames(torch.from_numpy(sc["frames"]).cuda() if frames is None else frames, sc["bg"] if bg is None else bg, thr)
    return rp


def targets_of(torch, sc, experiments=None):
    from wtracker_amd.replay import Targets

    a, valid = sc["a"], sc["valid"]
    if experiments is not None:
        a, valid = a[:, list(experiments)], valid[:, list(experiments)]
    return Targets("optimal", a.shape[1], torch.from_numpy(np.ascontiguousarray(a)).cuda(), None, torch.from_numpy(np.ascontiguousarray(valid)).cuda())


def reference(sc, thr=20, experiments=None, bg=None):
    pos, move = pr.scan_of(sc, experiments)
    err, counts, stats = pr.precise(sc["g"], sc["track"], pos, move, sc["frames"], sc["bg"] if bg is None else bg, thr)
    return dict(err=err, counts=counts, stats=stats, summary=pr.summaries(sc["g"], err), pos=pos, move=move)


def assert_equals_reference(res, ref, what=""):
    assert res.precise_counts.dtype == np.int32 and res.precise_error.dtype == np.float64
    assert np.array_equal(res.precise_counts, ref["counts"]), (what, np.argwhere(res.precise_counts != ref["counts"])[:5])
    assert np.array_equal(bits(res.precise_error), bits(ref["err"])), (what, np.argwhere(bits(res.precise_error) != bits(ref["err"]))[:5])
    assert_summary_equals(res.precise_summary, ref["summary"], what)


def assert_summary_equals(s, want, what=""):
    got = np.stack([s.precise_error_sum, s.rows, s.trimmed_precise_error_sum, s.trimmed_rows, s.non_perfect_rows, s.nan_rows], axis=1).astype(np.float64)
    assert np.array_equal(bits(got), bits(want)), (what, got[:3], want[:3])


@pytest.fixture(scope="module")
def main(torch_mod):
    """The first scenario, its harness values and the device's run of all 70 experiments with the default table limit: computed once, never modified."""
    sc = pr.scenario_main()
    ref = reference(sc)
    assert ref["stats"]["table"] > 0 and ref["stats"]["frame_walk"] == 0
    rp = make_replay(torch_mod, sc)
    dev_frames = rp._frames
    res = rp.run(targets_of(torch_mod, sc), rows=CHECKED, per_row_errors=True, precise=True)
    return dict(sc=sc, ref=ref, rp=rp, res=res, dev_frames=dev_frames)


# ------------------------------------------------------------------------------------------------- the first scenario
def test_population_equals_the_harness_the_old_kernel_and_itself_alone(torch_mod, main):
    from wtracker_amd import evaluation

    sc, ref, rp, res = main["sc"], main["ref"], main["rp"], main["res"]
    assert np.array_equal(res.moves, ref["move"].transpose(1, 0, 2)) and np.array_equal(res.positions, ref["pos"].transpose(1, 0, 2))
    assert_equals_reference(res, ref, "E = 70")
    s = res.precise_summary
    assert np.array_equal(bits(s.mean_precise_error), bits(ref["summary"][:, 0] / ref["summary"][:, 1]))
    assert np.array_equal(bits(s.trimmed_mean_precise_error), bits(ref["summary"][:, 2] / ref["summary"][:, 3]))
    assert np.array_equal(bits(s.non_perfect), bits(ref["summary"][:, 4] / ref["summary"][:, 1])) and np.array_equal(s.nan_rows, ref["summary"][:, 5])
    bg = torch_mod.from_numpy(sc["bg"]).cuda()
    for e in CHECKED:
        # the per-row kernel on the log the replay wrote: the route that existed before
        old_err, old_counts = evaluation.precise_error_from_log(res.log(e), main["dev_frames"], bg, 20, return_counts=True)
        assert np.array_equal(old_counts.cpu().numpy(), res.precise_counts[e]), e
        assert np.array_equal(bits(old_err.cpu().numpy()), bits(res.precise_error[e])), e
        alone = rp.run(targets_of(torch_mod, sc, [e]), rows=[], per_row_errors=True, precise=True)
        assert np.array_equal(alone.precise_counts[0], res.precise_counts[e]) and np.array_equal(bits(alone.precise_error[0]), bits(res.precise_error[e])), e
        assert_summary_equals(alone.precise_summary, ref["summary"][e:e + 1], f"e = {e} alone")


@pytest.mark.parametrize("limit", [64, 1])
def test_forced_fallback_changes_nothing(torch_mod, main, limit):
    """`_max_crop_px` = 64 keeps the table for the 1 x 1 crop's frame only, 1 for none: the direct walk and the table agree in every pair."""
    forced = pr.precise(main["sc"]["g"], main["sc"]["track"], main["ref"]["pos"], main["ref"]["move"], main["sc"]["frames"], main["sc"]["bg"], 20, max_cells=limit)[2]
    assert forced["frame_walk"] > 0 and (forced["table"] > 0) == (limit == 64)
    res = main["rp"].run(targets_of(torch_mod, main["sc"]), rows=[], per_row_errors=True, precise=True, _max_crop_px=limit)
    assert np.array_equal(res.precise_counts, main["res"].precise_counts) and np.array_equal(bits(res.precise_error), bits(main["res"].precise_error))
    assert_summary_equals(res.precise_summary, main["ref"]["summary"], f"limit {limit}")


# ------------------------------------------------------------------------------------------------- other shapes
@pytest.mark.parametrize("E", [1, 63, 65, 257])
def test_population_sizes(torch_mod, E):
    sc = pr.scenario_main(E=E)
    res = make_replay(torch_mod, sc).run(targets_of(torch_mod, sc), rows=[], per_row_errors=True, precise=True)
    assert res.precise_error.shape == (E, 120)
    assert_equals_reference(res, reference(sc), f"E = {E}")


@pytest.mark.parametrize("thr", [20, 19.5, -1, 255])
def test_thresholds(torch_mod, main, thr):
    sc, five = main["sc"], [0, 17, 35, 63, 69]
    ref = reference(sc, thr, five)
    if thr == -1:
        assert (ref["counts"][:, :, 0] > 0).sum() == np.isfinite(ref["err"]).sum()  # every pixel of every crop is foreground
    if thr == 255:
        assert ref["counts"].sum() == 0
    rp = make_replay(torch_mod, sc, frames=main["dev_frames"], thr=thr)
    assert_equals_reference(rp.run(targets_of(torch_mod, sc, five), rows=[], per_row_errors=True, precise=True), ref, f"thr = {thr}")


def test_float_background_and_unaligned_frames(torch_mod, main):
    """A floating background is truncated as the reference's astype(int32) truncates it; the frames are a slice at an odd byte offset of a larger tensor
    (131 columns: no row of it is 4-byte aligned either)."""
    torch = torch_mod
    sc, five = main["sc"], [0, 17, 35, 63, 69]
    bg_f = sc["bg"].astype(np.float64) + 0.75
    ref = reference(sc, 20, five, bg=bg_f)
    assert np.array_equal(ref["counts"], main["ref"]["counts"][five])
    F, H, W = sc["frames"].shape
    flat = torch.zeros(F * H * W + 7, dtype=torch.uint8, device="cuda")
    flat[3:3 + F * H * W] = main["dev_frames"].reshape(-1)
    frames = flat[3:3 + F * H * W].view(F, H, W)
    assert frames.data_ptr() % 4 == 3 and frames.is_contiguous()
    for bg in (bg_f, bg_f.astype(np.float32), torch.from_numpy(bg_f).cuda()):
        rp = make_replay(torch, sc, frames=frames, bg=bg)
        assert_equals_reference(rp.run(targets_of(torch, sc, five), rows=[], per_row_errors=True, precise=True), ref, "float background")


def test_a_box_beyond_any_table(torch_mod):
    sc = pr.scenario_big_box()
    ref = reference(sc)
    assert ref["stats"]["table"] == 0 and ref["stats"]["frame_walk"] == 5 * 6  # 213 x 213 cells: no table at the default limit
    assert (ref["counts"][:, :, 0] > 5000).all() and ((ref["err"] > 0) & (ref["err"] < 1)).any()
    res = make_replay(torch_mod, sc).run(targets_of(torch_mod, sc), rows=[], per_row_errors=True, precise=True)
    assert_equals_reference(res, ref, "210 x 210 box")


def test_the_ulp_case_in_both_directions(torch_mod):
    """(x - cam) + cam moves an edge of the logged box by one pixel against the track's box, outwards and inwards: the padded table still answers."""
    from wtracker_amd import evaluation

    sc = pr.scenario_ulp()
    ref = reference(sc)
    assert ref["stats"]["pair_walk"] == 0 and ref["stats"]["frame_walk"] == 0
    rp = make_replay(torch_mod, sc)
    res = rp.run(targets_of(torch_mod, sc), rows=[0, 1, 2], per_row_errors=True, precise=True)
    H, W = sc["frame_shape"]
    tx1, ty1, tx2, ty2, _ = ev.discretize(sc["track"][:rp.n_rows], (H, W))
    grown = shrunk = 0
    for e in range(3):
        x1, y1, x2, y2, _ = ev.discretize(res.row_array(e)[:, 10:14], (H, W))
        assert (np.abs(x1 - tx1) <= 1).all() and (np.abs(x2 - tx2) <= 1).all() and (np.abs(y1 - ty1) <= 1).all() and (np.abs(y2 - ty2) <= 1).all()
        grown += int((x2 > tx2).sum() + (y2 > ty2).sum())
        shrunk += int((x1 > tx1).sum())
    assert grown > 0 and shrunk > 0
    assert_equals_reference(res, ref, "ulp")
    bg = torch_mod.from_numpy(sc["bg"]).cuda()
    for e in range(3):
        old_err, old_counts = evaluation.precise_error_from_log(res.log(e), rp._frames, bg, 20, return_counts=True)
        assert np.array_equal(old_counts.cpu().numpy(), res.precise_counts[e]) and np.array_equal(bits(old_err.cpu().numpy()), bits(res.precise_error[e])), e
    forced = rp.run(targets_of(torch_mod, sc), rows=[], per_row_errors=True, precise=True, _max_crop_px=1)
    assert np.array_equal(forced.precise_counts, res.precise_counts)


def test_the_reduction_across_a_chunk(torch_mod):
    """R = 4104 > 4096 rows: the summary has the harness's bits (the fixed order) and lies within the bound of pairwise summation of math.fsum."""
    sc = pr.scenario_long()
    ref = reference(sc)
    res = make_replay(torch_mod, sc).run(targets_of(torch_mod, sc), rows=[], per_row_errors=True, precise=True)
    assert res.precise_error.shape == (3, 4104)
    assert_equals_reference(res, ref, "R = 4104")
    cyc, step = np.divmod(np.arange(4104), sc["g"].L)
    trimmed = (step < sc["g"].I) & (cyc != 0) & (cyc != sc["g"].n_log - 1)
    s = res.precise_summary
    for e in range(3):
        v = ref["err"][e]
        has = ~np.isnan(v)
        assert 0 < s.nan_rows[e] == (~has).sum() and s.rows[e] == has.sum() and s.trimmed_rows[e] == (has & trimmed).sum()
        for got, rows in ((s.precise_error_sum[e], has), (s.trimmed_precise_error_sum[e], has & trimmed)):
            exact = math.fsum(v[rows])
            assert abs(got - exact) <= math.ceil(math.log2(4104)) * 2.0 ** -53 * math.fsum(np.abs(v[rows])), (e, got, exact)


# ------------------------------------------------------------------------------------------------- objective and search
def test_every_precise_objective_equals_the_summary_property(torch_mod, main):
    from wtracker_amd.replay import OBJECTIVES, PRECISE_OBJECTIVES

    assert PRECISE_OBJECTIVES is hip.REPLAY_PRECISE_OBJECTIVES and sorted(PRECISE_OBJECTIVES) == ["precise_error", "precise_non_perfect", "trimmed_precise_error"]
    assert OBJECTIVES == {"trimmed_bbox_error": 0, "bbox_error": 1, "mse_error": 2, "non_perfect": 3}
    rp, s, tg = main["rp"], main["res"].precise_summary, targets_of(torch_mod, main["sc"])
    for kind, prop in (("trimmed_precise_error", "trimmed_mean_precise_error"), ("precise_error", "mean_precise_error"), ("precise_non_perfect", "non_perfect")):
        got = rp.objective(tg, kind).cpu().numpy()
        want = np.asarray(getattr(s, prop), dtype=np.float64)
        assert got.dtype == np.float64 and got.shape == (70,)
        assert got.tobytes() == want.tobytes(), (kind, np.flatnonzero(bits(got) != bits(want))[:5])
        assert len(set(got.tolist())) > 1 and np.isfinite(got).all(), kind
    # the box proxy still answers, and it is another number
    assert rp.objective(tg, "trimmed_bbox_error").cpu().numpy().tobytes() == np.asarray(main["res"].summary.trimmed_mean_bbox_error).tobytes()
    with pytest.raises(ValueError, match="trimmed_precise_error.*|precise"):
        rp.objective(tg, "no_such_error")


def test_search_on_the_precise_error(torch_mod, main):
    rp = main["rp"]
    kw = dict(objective="trimmed_precise_error", pop_size=16, max_epoch=6, lb=0.05, start=[W0], seed=0)
    first = rp.optimize_polyfit(1, TIMES, **kw)
    start = float(rp.objective(rp.polyfit_population(np.asarray([W0]), 1, TIMES), "trimmed_precise_error").cpu().numpy()[0])
    assert np.isfinite(first.mae) and first.mae <= start
    again = rp.run(rp.polyfit([rp.to_config(1, first.weights)]), rows=[], precise=True).precise_summary.trimmed_mean_precise_error[0]
    assert bits([first.mae])[0] == bits([again])[0], (first.mae, again)
    second = rp.optimize_polyfit(1, TIMES, **kw)
    assert bits(second.weights).tolist() == bits(first.weights).tolist() and bits([second.mae])[0] == bits([first.mae])[0]


def test_a_raised_stop_flag_leaves_the_precise_objective_untouched(torch_mod, main):
    torch = torch_mod
    rp, sc, E = main["rp"], main["sc"], 70
    tg = targets_of(torch, sc)
    SF, SI = -12345.5, -77
    b = dict(pos=torch.full((rp.n_cycles, E, 2), SI, dtype=torch.int32, device="cuda"), move=torch.full((rp.n_cycles, E, 2), SI, dtype=torch.int32, device="cuda"),
             summary=torch.full((E, 6), SF, dtype=torch.float64, device="cuda"),
             scratch=torch.full((hip.replay_precise_scratch_doubles(E, rp.n_rows),), SF, dtype=torch.float64, device="cuda"),
             out=torch.full((E,), SF, dtype=torch.float64, device="cuda"))
    ctrl = torch.tensor([1], dtype=torch.int32, device="cuda")

    def call():
        fr = rp._frames
        hip.replay_precise_objective(rp._cfg, hip.REPLAY_OPTIMAL, E, rp.n_cycles, rp.track, rp.n_track, tg.a, None, tg.valid, rp._share, b["pos"], b["move"], fr,
                                     fr.shape[0], fr.shape[1], fr.shape[2], rp._background, 20.0, 0, b["summary"], b["scratch"], b["scratch"].numel(),
                                     hip.REPLAY_PRECISE_OBJECTIVES["trimmed_precise_error"], b["out"], ctrl)
        torch.cuda.synchronize()

    call()
    assert all(bool((t == (SI if t.dtype == torch.int32 else SF)).all()) for t in b.values())
    ctrl.zero_()
    call()
    assert b["out"].cpu().numpy().tobytes() == np.asarray(main["res"].precise_summary.trimmed_mean_precise_error).tobytes()


# ------------------------------------------------------------------------------------------------- refusals and non-interference
def test_refusals(torch_mod, main):
    torch = torch_mod
    sc, dev_frames = main["sc"], main["dev_frames"]
    bare = make_replay(torch, sc, attach=False)
    tg = targets_of(torch, sc, [0])
    with pytest.raises(ValueError, match="attach_frames"):
        bare.run(tg, precise=True)
    with pytest.raises(ValueError, match="attach_frames"):
        bare.objective(tg, "precise_error")
    with pytest.raises(ValueError, match="attach_frames"):
        bare.optimize_polyfit(1, TIMES, objective="trimmed_precise_error", pop_size=4, max_epoch=1)
    with pytest.raises(ValueError, match="96 x 130"):
        bare.attach_frames(dev_frames[:, :, :130].contiguous(), sc["bg"][:, :130])
    with pytest.raises(ValueError, match="119 frames"):
        bare.attach_frames(dev_frames[:119], sc["bg"])
    with pytest.raises(ValueError, match="background"):
        bare.attach_frames(dev_frames, sc["bg"][:-1])
    with pytest.raises(hip.WtkError):
        bare.attach_frames(dev_frames.cpu(), sc["bg"])
    assert bare._frames is None
    bare.attach_frames(dev_frames[:120], sc["bg"])  # F = n_rows is enough
    assert bare.run(tg, rows=[], precise=True).precise_summary.rows[0] == main["res"].precise_summary.rows[0]
    # the trimmed objective needs three logged cycles
    short = dict(sc, g=pr.rr.Geometry(13, 4, 2, 1, (40, 32), (14, 10), (131, 96), (30, 30)))
    rp2 = make_replay(torch, short, frames=dev_frames)
    assert rp2.n_log == 2
    tg2 = targets_of(torch, dict(short, a=sc["a"][:rp2.n_cycles], valid=sc["valid"][:rp2.n_cycles]), [0])
    with pytest.raises(ValueError, match="at least 3"):
        rp2.objective(tg2, "trimmed_precise_error")
    assert np.isfinite(rp2.objective(tg2, "precise_error").cpu().numpy()).all()
    # the C entry point says why
    rp, E = main["rp"], 1
    buf = rp._objective_buffers(E)
    pb = rp._precise_buffers(E)

    def call(n_frames=121, H=96, W=131, frames=dev_frames, limit=0, scratch_doubles=None):
        hip.replay_precise(rp._cfg, E, rp.n_cycles, rp.track, rp.n_track, rp._share, buf["pos"], buf["move"], frames, n_frames, H, W, rp._background, 20.0, limit,
                           None, None, pb["summary"], pb["scratch"], pb["scratch"].numel() if scratch_doubles is None else scratch_doubles)

    for kw, why in ((dict(n_frames=119), "fewer frames"), (dict(H=131, W=96), "differ"), (dict(frames=None), "null"), (dict(limit=-1), "max_crop_px"),
                    (dict(scratch_doubles=5), "scratch")):
        with pytest.raises(hip.WtkError, match=why):
            call(**kw)
    assert hip.replay_precise_scratch_doubles(3, 4104) == 3 * 4104 + 3 * 2 * 6 + 2052 and hip.replay_precise_scratch_doubles(-1, 1) == -1


def test_attached_frames_leave_the_plain_run_alone(torch_mod, main):
    sc = main["sc"]
    tg = targets_of(torch_mod, sc)
    plain = make_replay(torch_mod, sc, attach=False).run(tg, rows=CHECKED, per_row_errors=True)
    attached = main["rp"].run(tg, rows=CHECKED, per_row_errors=True)
    assert attached.precise_summary is None and attached.precise_error is None and attached.precise_counts is None
    for name in ("bbox_error_sum", "rows", "trimmed_bbox_error_sum", "trimmed_rows", "non_perfect_rows", "mse_error_sum"):
        assert np.asarray(getattr(plain.summary, name)).tobytes() == np.asarray(getattr(attached.summary, name)).tobytes(), name
        assert np.asarray(getattr(plain.summary, name)).tobytes() == np.asarray(getattr(main["res"].summary, name)).tobytes(), name
    assert np.array_equal(plain.moves, attached.moves) and np.array_equal(plain.positions, attached.positions)
    assert plain.bbox_error.tobytes() == attached.bbox_error.tobytes() and plain.mse_error.tobytes() == attached.mse_error.tobytes()
    for e in CHECKED:
        assert plain.row_array(e).tobytes() == attached.row_array(e).tobytes() == main["res"].row_array(e).tobytes()
