"""tests/harness/analysis_ref.py (the numpy restatement the GPU analysis is held to) against tests/golden/analysis.npz, which the REAL reference's
DataAnalyzer and pandas wrote from the logs of tests/golden/replay_hard.npz (tests/golden/make_analysis_golden.py).  No GPU.

Exact (as float64 values, -0.0 == 0.0 and NaN == NaN): every rounded column, counts, minima, maxima, every percentile, the cycle maxima, the
per-cycle-step quantiles, the anomaly masks and counts, the print_stats figures.  Means: within n 2^-52 mean|x| (both sums lie within (n - 1) 2^-53 sum|x|
of the exact one).  Standard deviations: within n 2^-52 relative (first-order bound of a two-pass variance in any order: (n + 3) 2^-53; the second-order
term is below 1e-24 while |mean| / std < 100, which is asserted).  The bounds are derived, not measured."""
import json
import os

import numpy as np
import pytest

from harness import analysis_ref as ar


@pytest.fixture(scope="module")
def gold(golden_dir):
    z = np.load(os.path.join(golden_dir, "analysis.npz"))
    hard = np.load(os.path.join(golden_dir, "replay_hard.npz"))
    return dict(z=z, hard=hard, meta=json.loads(bytes(z["meta"]).decode()), hard_meta=json.loads(bytes(hard["meta"]).decode()))


def rows16_of(hard, hard_meta, run):
    """The [R, 16] rows of a pinned log, as ReplayResult.row_array gives them."""
    geo = hard_meta["geometry"][run.split("_")[1]]
    R = len(hard[run + "/cycle"])
    r = np.zeros((R, 16))
    r[:, 0:2], r[:, 2:4], r[:, 6:8], r[:, 10:14] = hard[run + "/plt"], hard[run + "/cam"], hard[run + "/mic"], hard[run + "/wrm"]
    r[:, 4:6], r[:, 8:10] = geo["camera_size_px"], geo["micro_size_px"]
    r[:, 14], r[:, 15] = hard[run + "/cycle"], hard[run + "/phase"]
    return r, geo["L"]


def spec_of(meta, cname, run):
    """The harness Spec of a fixture configuration (all of the fixture's columns and percentiles, its anomaly thresholds)."""
    cfg, thr = meta["configs"][cname], meta["thresholds"]
    f = meta["sec_factors"][run.split("_")[1]]
    clean = cfg["clean"] or {}
    return ar.Spec(period=cfg["period"], trim_cycles=bool(clean.get("trim_cycles")), imaging_only=bool(clean.get("imaging_only")),
                   bounds=tuple(clean["bounds"]) if clean.get("bounds") else None,
                   factors=ar.sec_factors(f["mm_per_px"], f["ms_per_frame"]) if cfg["unit"] == "sec" else (1.0, 1.0, 1.0),
                   columns=tuple(meta["columns"]), percentiles=tuple(meta["percentiles"]), min_speed=thr["min_speed"], min_bbox_error=thr["min_bbox_error"],
                   min_dist_error=thr["min_dist_error"], min_width=thr["min_size"], min_height=thr["min_size"], no_preds=True)


def same(a, b):
    """Equal as float64 values: -0.0 == 0.0, NaN matches NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def golden_of(z, key: str) -> dict:
    return {n: z[key + n] for n in ("describe", "cycle_max", "cycle_mean", "step_quantiles", "step_count", "anomaly_counts", "anomaly_mask", "stats")}


def assert_same_analysis(got: dict, want: dict, values: np.ndarray, keep: np.ndarray, L: int, what=""):
    """Two analyses of one experiment over the same columns (the harness's, the device's, the fixture's): everything equal as float64 values but the
    means and standard deviations, which stay within the derived bounds.  `values` [R, n_cols]: the final (unit-changed) column values."""
    d, g = np.asarray(got["describe"]), np.asarray(want["describe"])
    assert same(d[:, 0], g[:, 0]) and same(d[:, 3:], g[:, 3:]), (what, "count / min / percentiles / max")
    R = len(values)
    cyc = np.arange(R) // L
    for j in range(values.shape[1]):
        v = values[keep, j]
        v = v[~np.isnan(v)]
        n = len(v)
        if n == 0:
            assert np.isnan(d[j, 1]) and np.isnan(d[j, 2]) and np.isnan(g[j, 1]) and np.isnan(g[j, 2])
            continue
        assert abs(d[j, 1] - g[j, 1]) <= ar.mean_bound(v), (what, j, "mean", d[j, 1], g[j, 1])
        if n == 1:
            assert np.isnan(d[j, 2]) and np.isnan(g[j, 2])
        elif v.min() == v.max():
            # a constant column: the exact std is 0 and a computed one is the rounding error of the mean, |x - mean| <= n 2^-53 |x|, times sqrt(n / (n - 1))
            assert max(abs(d[j, 2]), abs(g[j, 2])) <= n * 2.0 ** -52 * abs(v[0]), (what, j, "std of a constant", d[j, 2], g[j, 2])
        else:
            assert abs(g[j, 1]) / g[j, 2] < 100, (what, j)  # the second-order term of the bound stays negligible
            assert abs(d[j, 2] - g[j, 2]) <= ar.std_bound(n) * g[j, 2], (what, j, "std", d[j, 2], g[j, 2])
    assert same(got["cycle_max"], want["cycle_max"]), (what, "cycle_max")
    gm, dm = np.asarray(want["cycle_mean"]), np.asarray(got["cycle_mean"])
    assert same(np.isnan(dm), np.isnan(gm)), (what, "cycle_mean")
    for k, j in np.argwhere(~np.isnan(gm)):
        assert abs(dm[k, j] - gm[k, j]) <= ar.mean_bound(values[keep & (cyc == k), j]), (what, k, j, "cycle_mean")
    assert same(got["step_quantiles"], want["step_quantiles"]), (what, "step_quantiles")
    assert np.array_equal(got["step_count"], want["step_count"]), (what, "step_count")
    assert np.array_equal(got["anomaly_counts"], want["anomaly_counts"]), (what, got["anomaly_counts"], want["anomaly_counts"])
    if got.get("anomaly_mask") is not None and want.get("anomaly_mask") is not None:
        assert np.array_equal(got["anomaly_mask"], want["anomaly_mask"]), (what, "anomaly_mask")
    assert np.array_equal(got["stats"], want["stats"]), (what, got["stats"], want["stats"])


def test_harness_reproduces_the_reference_analysis(gold):
    z, meta = gold["z"], gold["meta"]
    cols = [ar.COL[c] for c in meta["columns"]]
    for cname in meta["configs"]:
        for run in meta["runs"]:
            rows16, L = rows16_of(gold["hard"], gold["hard_meta"], run)
            spec = spec_of(meta, cname, run)
            got = ar.analyze(rows16, L, spec)
            key = f"{cname}/{run}/"
            if key + "table" in z:
                assert same(got["table"][:, cols], z[key + "table"]), key  # every rounded row column
            assert np.array_equal(got["keep"], z[key + "keep"]), key
            assert_same_analysis(got, golden_of(z, key), ar.to_unit(got["table"], spec.factors)[:, cols], got["keep"], L, "harness " + key)


def test_fixture_exercises_every_output(gold):
    """What the fixture was built for (its generator asserts the same before it writes)."""
    z, meta = gold["z"], gold["meta"]
    assert int(z["a/csv_100/keep"].sum()) == 120 and int(z["a/polyfit1_200/keep"].sum()) == 155
    assert all(int(z[f"c0/{r}/keep"].sum()) == 0 for r in meta["runs"]) and int(z["c1/csv_100/keep"].sum()) == 1
    assert (z["a/csv_100/anomaly_counts"][:3] > 0).all()
    cyc = meta["columns"].index("cycle")
    last = {int(z[f"a/{r}/table"][z[f"a/{r}/keep"], cyc].max()) for r in meta["runs"] if r.endswith("_100")}
    n_log = len(z["a/csv_100/keep"]) // 5
    assert max(last) < n_log - 2, last  # the bounds cut the tail: the trimmed cycle is the largest SURVIVING one, not n_log - 1
    d = z["c1/csv_100/describe"]
    assert (d[:, 0] <= 1).all() and np.isnan(d[d[:, 0] == 1, 2]).all()


def test_quantile_rule_and_rounding():
    v = np.array([-0.0, 0.0, 1.0, 1.0, 2.5, 7.0])
    for q in (0.0, 0.05, 0.25, 0.5, 0.75, 0.95, 0.99, 1.0):
        assert ar.quantile(v, q) == float(np.percentile(v, q * 100))
    x = np.concatenate([np.random.default_rng(5).normal(0, 300, 4000), [0.5, 1.5, 2.5, 1234.5, -0.4e-5, np.inf, -np.inf, np.nan]])
    r = ar.round5(x)
    assert same(r, np.round(x, 5)) and np.signbit(r[-4]) and r[-4] == 0.0  # numpy's own rule (half to even); -0.0 as the reference produces it