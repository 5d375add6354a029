"""harness.replay_set_scales_ref (the numpy statement of a ReplaySet with one TimingConfig per track) against
tests/golden/replay_set_scales.npz, which the real reference wrote on three recordings at 88, 90 and 92 px/mm
(tests/golden/make_replay_set_scales_golden.py).  No GPU.

Rows, moves and both errors are bit-equal; the pooled objective is the sum of the tracks' sums over the sum of their counts; the describe tables agree
as tests/test_replay_set_analysis_ref.py compares them (order statistics equal, means within analysis_ref.mean_bound, stds within std_bound).  The
planted defect (track 0's TimingConfig for every track, which is what a ReplaySet built from one config computes) is told from the fixture."""
import math

import numpy as np
import pytest

from harness import analysis_ref as ar
from harness import replay_set_ref as rset
from harness import replay_set_scales_ref as sc
from test_replay_set_analysis_ref import same

KINDS = ("csv", "polyfit", "mlp")


@pytest.fixture(scope="module")
def fx(golden_dir):
    f = sc.load(golden_dir)
    f["runs"] = {kind: sc.replay(f, kind) for kind in KINDS}
    return f


def test_the_fixture_has_what_it_exists_for(fx):
    """So that nothing below passes vacuously: three scales with both parities of size // 2, the clip binding on every track, a clipped value that
    depends on the scale, rows with and without bbox error on every track."""
    geo = fx["meta"]["geometry"]
    assert [g["camera_size_px"] for g in geo] == [[352, 361], [360, 369], [368, 377]] and [g["micro_size_px"] for g in geo] == [[28, 29], [29, 30], [29, 30]]
    assert {s % 2 for g in geo for s in g["camera_size_px"] + g["micro_size_px"]} == {0, 1}
    assert [r["px_per_mm"] for r in fx["meta"]["recordings"]] == [88, 90, 92] and all(300 <= r["num_frames"] <= 400 for r in fx["meta"]["recordings"])
    run = fx["runs"]["mlp"]
    st, raw, valid = run["st"], run["raw"], run["valid"][:, 0].astype(bool)
    differs = 0
    for t, g in enumerate(fx["geoms"]):
        sl = slice(st.cyc_off[t], st.cyc_off[t] + g.n_cycles)
        r = raw[sl][valid[sl]]
        assert len(r) and (np.abs(r.astype(np.float32)) > np.float32(fx["bounds"][t])).any(), f"the clip never binds on track {t}"
        differs += int((sc.clip_f32(r, fx["bounds"][0]) != sc.clip_f32(r, fx["bounds"][2])).sum())
        for kind in KINDS:
            err = fx["z"][f"t{t}/{kind}/bbox_error"]
            assert (err == 0).any() and (err > 1e-7).any(), (t, kind)
    assert differs > 0 and fx["bounds"][0] < fx["bounds"][1] < fx["bounds"][2]


def differences(fx, kind: str, run: dict) -> dict:
    """Per track: the number of moves, rows and errors of `run` that differ from the fixture's (bit for bit)."""
    z, st, out = fx["z"], run["st"], []
    for t, g in enumerate(run["geoms"]):
        key, lg = f"t{t}/{kind}/", run["logs"][t]
        mv = z[key + "moves"]
        sl = slice(st.cyc_off[t], st.cyc_off[t] + len(mv))
        assert len(mv) == g.n_cycles and (mv[:, 0] == np.arange(g.n_cycles) * g.L + g.I).all()
        rows = lg["rows"]
        want = np.concatenate([z[key + "plt"], z[key + "cam"], np.broadcast_to(fx["geoms"][t].cam, (len(rows), 2)), z[key + "mic"],
                               np.broadcast_to(fx["geoms"][t].mic, (len(rows), 2)), z[key + "wrm"], z[key + "cycle"][:, None], z[key + "phase"][:, None]],
                              axis=1).astype(np.float64)
        assert rows.shape == want.shape
        bits = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)  # noqa: E731
        out.append(dict(moves=int((run["move"][sl, 0] != mv[:, 1:]).any(axis=1).sum()), rows=int((bits(rows) != bits(want)).any(axis=1).sum()),
                        bbox=int((bits(lg["bbox_error"]) != bits(z[key + "bbox_error"])).sum()), mse=int((bits(lg["mse_error"]) != bits(z[key + "mse_error"])).sum())))
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_rows_moves_and_errors_equal_the_reference(fx, kind):
    for t, d in enumerate(differences(fx, kind, fx["runs"][kind])):
        assert d == dict(moves=0, rows=0, bbox=0, mse=0), (kind, t, d)


@pytest.mark.parametrize("kind", KINDS)
def test_pooled_objective_is_sum_of_sums_over_sum_of_counts(fx, kind):
    run, z, T = fx["runs"][kind], fx["z"], fx["T"]
    ts, pooled = run["track_summary"], run["summary"]
    for q in range(6):
        chain = 0.0
        for t in range(T):
            chain = chain + ts[t, 0, q]
        assert pooled[0, q] == chain
    errs = [z[f"t{t}/{kind}/bbox_error"] for t in range(T)]
    assert pooled[0, 1] == sum(len(e) for e in errs) and [ts[t, 0, 1] for t in range(T)] == [len(e) for e in errs]
    exact, bound = rset.pooled_sum_bound(errs, T)
    assert abs(pooled[0, 0] - exact) <= bound
    objective = pooled[0, 0] / pooled[0, 1]
    assert abs(objective - exact / pooled[0, 1]) <= bound / pooled[0, 1] + 2.0 ** -53 * objective
    # not the mean of the tracks' means: the tracks have different lengths
    assert objective != np.mean([ts[t, 0, 0] / ts[t, 0, 1] for t in range(T)])
    mse = [z[f"t{t}/{kind}/mse_error"] for t in range(T)]
    exact, bound = rset.pooled_sum_bound(mse, T)
    assert abs(pooled[0, 5] - exact) <= bound


def specs_of(fx, factors) -> list:
    m = fx["meta"]
    return [ar.Spec(period=m["period"], factors=f, columns=tuple(m["columns"]), percentiles=tuple(m["percentiles"])) for f in factors]


def describe_mismatches(got: np.ndarray, want: np.ndarray, values, Q: int) -> list:
    """Order statistics and counts equal; the mean within analysis_ref.mean_bound.  The std: analysis_ref.std_bound (relative, the two-pass variance
    about the exact mean) plus what the computed mean adds: a mean off by d adds n d^2 to the sum of squares, so at most sqrt(n / (n - 1)) |d| to
    the std; each side's mean lies within mean_bound / 2 of the exact one, which gives less than 2 mean_bound for both together.  The second term
    is what is left of a CONSTANT column in unit "sec" (cam_w = 352 * 11.36...: the exact std is 0, each side returns its own rounding of the mean)."""
    bad = []
    for name, sl in (("count", slice(0, 1)), ("min", slice(3, 4)), ("percentiles", slice(4, 4 + Q)), ("max", slice(4 + Q, 5 + Q))):
        if not same(got[:, sl], want[:, sl]):
            bad.append(name)
    for j, v in enumerate(values):
        n = int((~np.isnan(v)).sum())
        if n and not abs(got[j, 1] - want[j, 1]) <= ar.mean_bound(v):
            bad.append("mean")
        if n > 1 and not abs(got[j, 2] - want[j, 2]) <= ar.std_bound(n) * want[j, 2] + 2 * ar.mean_bound(v):
            bad.append("std")
    return sorted(set(bad))


@pytest.mark.parametrize("kind", KINDS)
def test_describe_in_seconds_per_log_and_of_the_concatenation(fx, kind):
    """Every log through change_unit with its own recording's factors; the concatenation over the values so converted."""
    z, L, Q = fx["z"], fx["geoms"][0].L, len(fx["meta"]["percentiles"])
    logs = [lg["rows"] for lg in fx["runs"][kind]["logs"]]
    res = sc.analyze(logs, L, specs_of(fx, fx["factors"]))
    cols = [ar.COL[c] for c in fx["meta"]["columns"]]
    for t in range(fx["T"]):
        one = res["track"][t]
        tab = ar.to_unit(one["table"], fx["factors"][t])
        assert describe_mismatches(one["describe"], z[f"t{t}/{kind}/describe"], [tab[:, c] for c in cols], Q) == [], (kind, t)
    assert describe_mismatches(res["pooled"]["describe"], z[f"pooled/{kind}/describe"], res["pooled"]["values"], Q) == [], kind
    assert res["pooled"]["n_rows"] == sum(len(r) for r in logs)
    # the factors do differ, and one pair for all logs is told from the fixture
    assert len({f[1] for f in fx["factors"]}) == 3
    wrong = sc.analyze(logs, L, specs_of(fx, [fx["factors"][0]] * fx["T"]))
    assert describe_mismatches(wrong["pooled"]["describe"], z[f"pooled/{kind}/describe"], wrong["pooled"]["values"], Q) != []
    assert describe_mismatches(wrong["track"][2]["describe"], z[f"t2/{kind}/describe"], [ar.to_unit(wrong["track"][2]["table"], fx["factors"][0])[:, c] for c in cols], Q) != []


def test_planted_defect_is_caught(fx):
    """Track 0's TimingConfig for every track: track 0 still equals the fixture; tracks 1 and 2 each differ from it in at least one move and in at
    least one error."""
    per_kind = {kind: differences(fx, kind, sc.replay(fx, kind, defect="config_track0")) for kind in KINDS}
    for kind in KINDS:
        assert per_kind[kind][0] == dict(moves=0, rows=0, bbox=0, mse=0), kind
    for t in (1, 2):
        assert sum(per_kind[kind][t]["moves"] for kind in KINDS) > 0, (t, "no move differs")
        assert per_kind["mlp"][t]["moves"] > 0, (t, "the clip bound of track 0 changes no move")
        for kind in KINDS:
            assert per_kind[kind][t]["bbox"] > 0 and per_kind[kind][t]["mse"] > 0 and per_kind[kind][t]["rows"] > 0, (t, kind)
    assert math.isfinite(sum(d["bbox"] for ds in per_kind.values() for d in ds))


def test_configs_of_a_set_are_checked_without_a_gpu(fx):
    """wtracker_amd.replay.check_timing_configs (what ReplaySet does with a sequence of configs before it touches the device) and Analysis.factors of
    a sequence: one triple per track, each the reference's change_unit factors of that recording."""
    from wtracker_amd.replay import Analysis, check_timing_configs, mlp_clip_bound
    from wtracker_amd.sim import ExperimentConfig, TimingConfig

    m = fx["meta"]
    ecs = [ExperimentConfig(f"scale{t}", r["num_frames"], m["frames_per_sec"], tuple(m["orig_resolution"]), r["px_per_mm"], tuple(r["init_position"]))
           for t, r in enumerate(m["recordings"])]
    tcs = [TimingConfig(ec, *m["timing"], tuple(m["camera_size_mm"]), tuple(m["micro_size_mm"])) for ec in ecs]
    assert check_timing_configs(tcs, 3) == tcs
    assert [list(tc.camera_size_px) for tc in tcs] == [g["camera_size_px"] for g in m["geometry"]]
    assert [list(tc.micro_size_px) for tc in tcs] == [g["micro_size_px"] for g in m["geometry"]]
    assert Analysis(unit="sec").factors(tcs) == fx["factors"] and Analysis(unit="frame").factors(tcs) == [(1.0, 1.0, 1.0)] * 3
    assert Analysis(unit="sec").factors(tcs[1]) == fx["factors"][1]
    assert [mlp_clip_bound(tc, m["max_speed"], fx["state"]["pred_frames"]) for tc in tcs] == [float(np.float32(b)) for b in fx["bounds"]]
    with pytest.raises(ValueError, match="3 tracks.*sequence of 3, got 2"):
        check_timing_configs(tcs[:2], 3)
    other = TimingConfig(ecs[2], 120, 40, 50, tuple(m["camera_size_mm"]), tuple(m["micro_size_mm"]))
    with pytest.raises(ValueError, match=r"track 2: .*\(8, 3, 3\), track 0 has \(6, 3, 3\)"):
        check_timing_configs([tcs[0], tcs[1], other], 3)
    with pytest.raises(ValueError, match="track 1: the camera .* is smaller than the microscope"):
        check_timing_configs([tcs[0], TimingConfig(ecs[1], *m["timing"], (0.3, 4.1), tuple(m["micro_size_mm"])), tcs[2]], 3)
