"""harness.replay_set_analysis_ref (the numpy restatement of the analysis of a set of logs) against tests/golden/analysis_set.npz,
which the reference's real DataAnalyzer, its Plotter's concatenation and pandas wrote (tests/golden/make_analysis_set_golden.py).  No GPU.

Counts, minima, maxima, percentiles, cycle maxima, step quantiles and counts, anomaly counts and stats are equal; pooled means lie within
analysis_ref.mean_bound of the concatenated values and pooled stds within std_bound(N): the bounds DESIGN.md section 20 derives for two summation orders."""
import json
import os

import numpy as np
import pytest

from harness import analysis_ref as ar
from harness import replay_set_analysis_ref as sr


def same(x, y):
    """Equality of two float arrays as float64 bits, NaN matching NaN, and the sign of a zero left out: among the equal values -0.0 and 0.0 (a speed
    of -1e-6 rounds to -0.0) pandas' max and percentile return whichever its sort left in that place, so the reference itself fixes no sign there
    (tests/test_analysis_ref.py compares the same way)."""
    x, y = np.asarray(x, dtype=np.float64) + 0.0, np.asarray(y, dtype=np.float64) + 0.0  # (-0.0 + 0.0 = 0.0)
    n = np.isnan(x)
    return x.shape == y.shape and bool(np.array_equal(n, np.isnan(y)) and np.array_equal(x[~n].view(np.uint64), y[~n].view(np.uint64)))


@pytest.fixture(scope="module")
def fx(golden_dir):
    z = np.load(os.path.join(golden_dir, "analysis_set.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    return dict(z=z, meta=meta, scene=sr.the_scene(golden_dir))


def spec_of(meta: dict, cname: str) -> ar.Spec:
    cfg, th = meta["configs"][cname], meta["thresholds"]
    clean = cfg["clean"] or {}
    factors = ar.sec_factors(**meta["sec_factors"]) if cfg["unit"] == "sec" else (1.0, 1.0, 1.0)
    return ar.Spec(period=cfg["period"], trim_cycles=bool(clean.get("trim_cycles")), imaging_only=bool(clean.get("imaging_only")),
                   bounds=tuple(clean["bounds"]) if clean else None, factors=factors, columns=tuple(meta["columns"]), percentiles=tuple(meta["percentiles"]),
                   min_speed=th["min_speed"], min_bbox_error=th["min_bbox_error"], min_dist_error=th["min_dist_error"], min_width=th["min_size"],
                   min_height=th["min_size"])


def mismatches(fx, cname: str, kind: str, res: dict) -> list:
    """The names of the fixture's arrays the pooled result `res` misses (the check of the fixture test, shared with the planted defects)."""
    z, meta, key, p = fx["z"], fx["meta"], f"{cname}/{kind}/", res["pooled"]
    Q, bad = len(meta["percentiles"]), []
    want = z[key + "describe"]
    if not np.array_equal(np.concatenate(res["keep"]), z[key + "keep"]):
        bad.append("keep")
    for name, sl in (("count", slice(0, 1)), ("min", slice(3, 4)), ("percentiles", slice(4, 4 + Q)), ("max", slice(4 + Q, 5 + Q))):
        if not same(p["describe"][:, sl], want[:, sl]):
            bad.append(name)
    for j in range(len(meta["columns"])):
        v = p["values"][j]
        n = int((~np.isnan(v)).sum())
        if n and not abs(p["describe"][j, 1] - want[j, 1]) <= ar.mean_bound(v):
            bad.append("mean")
        if n > 1 and not abs(p["describe"][j, 2] - want[j, 2]) <= ar.std_bound(n) * want[j, 2]:
            bad.append("std")
    cyc = [meta["columns"].index(c) for c in meta["cycle_columns"]]
    if not same(p["cycle_max"][:, cyc], z[key + "cycle_max"]):
        bad.append("cycle_max")
    got, ref = p["cycle_mean"][:, cyc], z[key + "cycle_mean"]
    if not (np.array_equal(np.isnan(got), np.isnan(ref)) and np.allclose(got, ref, rtol=5 * 2.0 ** -52, atol=0, equal_nan=True)):  # mean_bound of L = 5 non-negative values
        bad.append("cycle_mean")
    if not same(p["step_quantiles"], z[key + "step_quantiles"]):
        bad.append("step_quantiles")
    for name in ("step_count", "anomaly_counts", "stats"):
        if not np.array_equal(p[name], z[key + name]):
            bad.append(name)
    return sorted(set(bad))


@pytest.mark.parametrize("cname", ["a", "b", "c"])
def test_harness_equals_the_reference_on_three_logs(fx, cname):
    spec, sc = spec_of(fx["meta"], cname), fx["scene"]
    for kind in sr.KINDS:
        res = sr.analyze_set(sc["logs"][kind], sc["L"], spec)
        assert mismatches(fx, cname, kind, res) == [], (cname, kind)
        assert res["pooled"]["n_rows"] == 395 + 135 + 4125
        assert [int(k.sum()) for k in res["keep"]] == fx["z"][f"{cname}/{kind}/kept"].tolist()
    if cname == "c":  # track 1 keeps nothing and is no link of the chain
        assert fx["z"]["c/csv/kept"][1] == 0 and fx["z"]["c/csv/kept"][0] > 0 and fx["z"]["c/csv/kept"][2] > 0


def test_one_track_pooled_has_the_track_bits(fx):
    """T = 1: the chain starts from the track's own sum, so the pooled moments are the per-track kernel's; the order statistics are analysis_ref's."""
    sc = fx["scene"]
    spec = spec_of(fx["meta"], "a")
    for t in (0, 1):
        rows = sc["logs"]["polyfit"][t]
        res = sr.analyze_set([rows], sc["L"], spec)
        one, p = res["track"][0], res["pooled"]
        Q = len(spec.percentiles)
        assert same(p["describe"][:, [0] + list(range(3, 5 + Q))], one["describe"][:, [0] + list(range(3, 5 + Q))])
        assert same(p["step_quantiles"], one["step_quantiles"]) and np.array_equal(p["step_count"], one["step_count"])
        assert np.array_equal(p["anomaly_counts"], one["anomaly_counts"]) and np.array_equal(p["stats"], one["stats"])
        assert same(p["cycle_max"], one["cycle_max"]) and same(p["cycle_mean"], one["cycle_mean"])
        tab_u, keep = ar.to_unit(one["table"], spec.factors), one["keep"]
        for j, c in enumerate(spec.columns):
            v = tab_u[:, ar.COL[c]]
            use = keep & ~np.isnan(v)
            if use.any():
                assert same([p["describe"][j, 1]], [sr.kernel_sum(v, use) / int(use.sum())]), c


@pytest.mark.parametrize("defect,cname,caught", [("speed_across", "b", {"percentiles", "step_quantiles"}), ("trim_set", "a", {"keep", "count"}),
                                                  ("mean_of_percentiles", "a", {"percentiles"}), ("std_per_track", "b", {"std"})])
def test_planted_defects_are_caught(fx, defect, cname, caught):
    spec, sc = spec_of(fx["meta"], cname), fx["scene"]
    res = sr.analyze_set(sc["logs"]["csv"], sc["L"], spec, defect=defect)
    bad = set(mismatches(fx, cname, "csv", res))
    assert caught & bad, (defect, bad)
