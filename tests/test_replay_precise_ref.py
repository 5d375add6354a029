"""The numpy restatement of replay_precise_kernel (tests/harness/replay_precise_ref.py) is pinned, not trusted: it equals, counts and error bits, the
composition that existed before (replay_ref.scan + replay_ref.rows -> eval_ref.precise on the rows' wrm / mic columns), and it equals bit for bit what the
real reference's ErrorCalculator.calculate_precise returned on the replayed logs of four experiments (tests/golden/replay_precise.npz,
tests/golden/make_replay_precise_golden.py).  No GPU."""
import os

import numpy as np
import pytest

from harness import eval_ref as ev
from harness import replay_precise_ref as pr
from harness import replay_ref as rr

SAMPLED = (0, 1, 35, 63, 64, 69)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


@pytest.fixture(scope="module")
def main():
    sc = pr.scenario_main()
    pos, move = pr.scan_of(sc)
    err, counts, stats = pr.precise(sc["g"], sc["track"], pos, move, sc["frames"], sc["bg"], 20)
    return dict(sc=sc, pos=pos, move=move, err=err, counts=counts, stats=stats)


def assert_equals_composition(sc, pos, move, err, counts, thr=20, experiments=None):
    comp = pr.composition(sc["g"], sc["track"], pos, move, sc["frames"], sc["bg"], thr, experiments)
    for e, (want_err, want_counts, _) in comp.items():
        assert np.array_equal(counts[e], want_counts), (e, np.argwhere(counts[e] != want_counts)[:5])
        assert np.array_equal(bits(err[e]), bits(want_err)), (e, np.flatnonzero(bits(err[e]) != bits(want_err))[:5])
    return comp


def test_the_scenario_is_not_trivial(main):
    """What keeps the equalities below from holding for an empty reason, on the sampled experiments."""
    sc, err, counts = main["sc"], main["err"], main["counts"]
    assert sc["frames"].shape == (121, 96, 131) and err.shape == (70, 120) and (sc["valid"] == 0).sum() > 70
    assert main["stats"] == dict(table=70 * 114, frame_walk=0, pair_walk=0)
    for e in SAMPLED:
        v, total = err[e], counts[e, :, 0]
        has = ~np.isnan(v)
        assert ((v > 0) & (v < 1)).sum() >= 0.6 * has.sum(), e
        assert (v == 1).any(), e
        assert (has & (total == 0)).any() and (~has).sum() == 6, e
    assert sum(int(((err[e] == 0) & (counts[e, :, 0] > 0)).sum()) for e in SAMPLED) > 0
    # the box proxy is another number
    prox = np.array([rr.rows(sc["g"], sc["track"], main["pos"], main["move"], e)["summary"] for e in SAMPLED])
    s = pr.summaries(sc["g"], err[list(SAMPLED)])
    assert (np.abs(prox[:, 2] / prox[:, 3] - s[:, 2] / s[:, 3]) > 0.005).all()


def test_harness_equals_the_composition(main):
    assert_equals_composition(main["sc"], main["pos"], main["move"], main["err"], main["counts"])


@pytest.mark.parametrize("thr", [19.5, -1, 255])
def test_harness_equals_the_composition_at_other_thresholds(main, thr):
    sc, five = main["sc"], [0, 17, 35, 63, 69]
    pos, move = pr.scan_of(sc, five)
    err, counts, _ = pr.precise(sc["g"], sc["track"], pos, move, sc["frames"], sc["bg"], thr)
    assert_equals_composition(sc, pos, move, err, counts, thr)


@pytest.mark.parametrize("limit", [64, 1])
def test_the_fallback_rule_changes_nothing(main, limit):
    sc = main["sc"]
    err, counts, stats = pr.precise(sc["g"], sc["track"], main["pos"], main["move"], sc["frames"], sc["bg"], 20, max_cells=limit)
    assert stats["frame_walk"] > 0 and (stats["table"] == 70) == (limit == 64)  # 64 cells hold the 1 x 1 crop's 4 x 5 table only
    assert np.array_equal(counts, main["counts"]) and np.array_equal(bits(err), bits(main["err"]))


def test_an_empty_intersection_is_decided_before_any_lookup(main):
    """Pairs whose intersection corner max(wl, ml) lies outside the padded region exist: indexing the table with it would leave the table."""
    sc, g = main["sc"], main["sc"]["g"]
    H, W = sc["frame_shape"]
    P = pr.frame_positions(g, main["pos"], main["move"])
    outside = 0
    for r in range(120):
        worm, mic = pr.logged_boxes(g, sc["track"][r], P[r])
        wl, wt, wr, wb, legal = ev.discretize(worm, (H, W))
        ml, mt, mr, mb, _ = ev.discretize(mic, (H, W))
        outside += int((legal & ((np.maximum(wl, ml) > wr + 1) | (np.maximum(wt, mt) > wb + 1))).sum())
    assert outside > 100


def test_the_ulp_scenario(main):
    sc = pr.scenario_ulp()
    g, (H, W) = sc["g"], sc["frame_shape"]
    pos, move = pr.scan_of(sc)
    assert pos[1:, 0, 0].tolist() == [11] * (g.n_cycles - 1) and pos[1:, 1, 0].tolist() == [16] * (g.n_cycles - 1) and pos[1:, 2].tolist() == [[20, 16]] * (g.n_cycles - 1)
    err, counts, stats = pr.precise(g, sc["track"], pos, move, sc["frames"], sc["bg"], 20)
    assert stats["pair_walk"] == 0 and stats["frame_walk"] == 0  # one pixel of padding is enough
    comp = assert_equals_composition(sc, pos, move, err, counts)
    tx1, ty1, tx2, ty2, _ = ev.discretize(sc["track"][:g.n_log * g.L], (H, W))
    x1, y1, x2, y2, _ = ev.discretize(comp[0][2][:, 10:14], (H, W))
    assert (x2 == tx2 + 1).sum() >= 10 and (x1 == tx1 + 1).sum() >= 10 and (y2 == ty2 + 1).sum() == 1  # cam = (-9, -8): both directions
    x1, y1, x2, y2, _ = ev.discretize(comp[2][2][6:, 10:14], (H, W))
    assert np.array_equal(x1, tx1[6:]) and np.array_equal(x2, tx2[6:])  # cam = (0, 0): the logged box is the track's
    assert ((err > 0) & (err < 1)).sum() > 40
    for limit in (64, 1):
        e2, c2, _ = pr.precise(g, sc["track"], pos, move, sc["frames"], sc["bg"], 20, max_cells=limit)
        assert np.array_equal(c2, counts) and np.array_equal(bits(e2), bits(err))


def test_the_other_scenarios_equal_the_composition():
    for sc, experiments in ((pr.scenario_big_box(), None), (pr.scenario_long(), [1])):
        pos, move = pr.scan_of(sc)
        err, counts, stats = pr.precise(sc["g"], sc["track"], pos, move, sc["frames"], sc["bg"], 20)
        assert_equals_composition(sc, pos, move, err, counts, experiments=experiments)
        assert (stats["table"] == 0) == (sc["frame_shape"] == (256, 256))


def test_summaries_follow_the_fixed_order(main):
    g, err = main["sc"]["g"], main["err"]
    s = pr.summaries(g, err)
    cyc, step = np.divmod(np.arange(120), g.L)
    trimmed = (step < g.I) & (cyc != 0) & (cyc != g.n_log - 1)
    for e in SAMPLED:
        v = err[e]
        has = ~np.isnan(v)
        assert s[e, 1] == has.sum() == 114 and s[e, 3] == (has & trimmed).sum() and s[e, 5] == 6 and s[e, 4] == (v[has] > 1e-7).sum()
        assert abs(s[e, 0] - np.sum(v[has])) < 1e-12 and abs(s[e, 2] - np.sum(v[has & trimmed])) < 1e-12
        assert s[e, 0] == rr._tree_sum(np.nan_to_num(v, nan=0.0))
        # pandas' mean of the column skips the NaN rows
        assert abs(s[e, 0] / s[e, 1] - np.nanmean(v)) < 1e-15
    long = np.tile(err[35], 40)[:4104]  # across a chunk
    g_long = rr.Geometry(4105, 4, 2, 1, (40, 32), (14, 10), (131, 96), (30, 30))
    assert pr.summaries(g_long, long[None])[0, 0] == rr._tree_sum(np.nan_to_num(long[:4096], nan=0.0)) + rr._tree_sum(np.nan_to_num(long[4096:], nan=0.0))


def test_harness_equals_the_real_reference(main, golden_dir):
    z = np.load(os.path.join(golden_dir, "replay_precise.npz"))
    sc = main["sc"]
    for key, name in (("track", "track"), ("frames", "frames"), ("bg", "background"), ("a", "a"), ("valid", "valid")):
        assert np.array_equal(sc[key], z[name], equal_nan=True), f"the scenario rebuilt from its seed differs from the recorded one in {key}"
    assert os.path.getsize(os.path.join(golden_dir, "replay_precise.npz")) < 256 * 1024
    comp = pr.composition(sc["g"], sc["track"], main["pos"], main["move"], sc["frames"], sc["bg"], float(z["diff_thresh"]), [int(e) for e in z["experiments"]])
    for e in (int(e) for e in z["experiments"]):
        assert np.array_equal(bits(comp[e][2][:, 10:14]), bits(z[f"worm_{e}"])) and np.array_equal(comp[e][2][:, 6:10], z[f"mic_{e}"]), e
        assert np.array_equal(bits(ev.reference_layout(main["err"][e])), bits(z[f"ref_{e}"])), e


def test_the_abi_additions(hip_lib):
    """Additive: three entry points behind the header's last section, a table of their own for the objectives, the ABI version unchanged."""
    from wtracker_amd import _build, hip, replay

    assert hip.SYMBOLS[-3:] == ["wtk_replay_precise_scratch_doubles", "wtk_replay_precise", "wtk_replay_precise_objective"]
    assert hip_lib.wtk_abi_version() == 7 and hip.REPLAY_OBJECTIVES == {"trimmed_bbox_error": 0, "bbox_error": 1, "mse_error": 2, "non_perfect": 3}
    assert replay.PRECISE_OBJECTIVES is hip.REPLAY_PRECISE_OBJECTIVES == {"trimmed_precise_error": 0, "precise_error": 1, "precise_non_perfect": 2}
    assert hip.REPLAY_PRECISE_SUMMARY_DOUBLES == 6 and "eval_device.h" in _build.HEADERS
    # E R pair errors, 6 doubles per (experiment, chunk of 4096 rows), R int32 flags
    assert hip_lib.wtk_replay_precise_scratch_doubles(3, 4104) == 3 * 4104 + 3 * 2 * 6 + 2052 and hip_lib.wtk_replay_precise_scratch_doubles(1, -1) == -1
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "wtk_hip.h")).read()
    for name, value in (("WTK_REPLAY_PRECISE_SUMMARY_DOUBLES", 6), ("WTK_REPLAY_POBJ_TRIMMED_PRECISE", 0), ("WTK_REPLAY_POBJ_MEAN_PRECISE", 1), ("WTK_REPLAY_POBJ_NON_PERFECT", 2)):
        assert f"#define {name} {value}\n" in header, name
    # the refusals are made before any device call: they answer without a GPU
    cfg = hip.replay_config(121, 4, 2, 1, (40, 32), (14, 10), (131, 96), (30, 30))
    with pytest.raises(hip.WtkError, match="null argument"):
        hip.replay_precise(cfg, 1, 20, None, 121, None, None, None, None, 121, 96, 131, None, 20.0, 0, None, None, None, None, 0)
