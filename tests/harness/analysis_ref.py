"""TEST INFRASTRUCTURE: float64 numpy restatement of the reference's analysis of ONE replayed log (wtracker/eval/data_analyzer.py: initialize, clean,
change_unit, describe, calc_anomalies, print_stats; wtracker/eval/plotter.py: the per-cycle and per-cycle-step aggregates), which
wtracker_amd/csrc/replay_analysis.hip computes for a whole population on the device.  No pandas, no import of the reference.

  table(rows16, L, period)     the columns DataAnalyzer.initialize derives, [R, 30] in the order of COLUMNS, rounded as DataFrame.round(5) rounds
  keep_mask(tab, phase, spec)  DataAnalyzer.clean: imaging_only, bounds, trim_cycles (cycle 0 and the LARGEST SURVIVING cycle), in that order
  analyze(rows16, L, spec)     every array of wtracker_amd.replay.AnalysisResult for one experiment

It is pinned, not trusted: tests/test_analysis_ref.py holds it to tests/golden/analysis.npz, which the real DataAnalyzer and pandas wrote.  Order
statistics, counts, maxima and the rounded columns are exact; sums are sequential here (np.add.reduce over a contiguous 1-d array adds pairwise: the
loops below are explicit) and the kernels add in another fixed order, so means and standard deviations agree within the bounds of mean_bound / std_bound."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

COLUMNS = ["frame", "cycle", "plt_x", "plt_y", "cam_x", "cam_y", "cam_w", "cam_h", "mic_x", "mic_y", "mic_w", "mic_h", "wrm_x", "wrm_y", "wrm_w", "wrm_h",
           "time", "cycle_step", "wrm_center_x", "wrm_center_y", "mic_center_x", "mic_center_y", "wrm_speed_x", "wrm_speed_y", "wrm_speed",
           "worm_deviation_x", "worm_deviation_y", "worm_deviation", "bbox_error", "precise_error"]
COL = {n: i for i, n in enumerate(COLUMNS)}
DIST_COLUMNS = COLUMNS[2:16] + COLUMNS[18:22] + COLUMNS[25:28]  # what change_unit multiplies by the distance factor
SPEED_COLUMNS = COLUMNS[22:25]
ANOMALIES = ["speed", "bbox_error", "dist_error", "width", "height", "no_pred", "any"]  # bit k of the mask, column k of the counts ("any": a count only)


@dataclass
class Spec:
    period: int = 10
    trim_cycles: bool = False
    imaging_only: bool = False
    bounds: tuple = None
    factors: tuple = (1.0, 1.0, 1.0)  # time, distance, speed = distance / time (change_unit("sec")); ones for unit "frame"
    columns: tuple = ("wrm_speed", "worm_deviation", "bbox_error")
    percentiles: tuple = (0.25, 0.5, 0.75)
    min_speed: float = math.inf
    min_bbox_error: float = math.inf
    min_dist_error: float = math.inf
    min_width: float = math.inf
    min_height: float = math.inf
    no_preds: bool = True


def sec_factors(mm_per_px: float, ms_per_frame: float) -> tuple:
    dist, tf = mm_per_px * 1000, ms_per_frame / 1000
    return (tf, dist, dist / tf)


def round5(v: np.ndarray) -> np.ndarray:
    """DataFrame.round(5) on a float column: rint(v * 1e5) / 1e5, non-finite values unchanged."""
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(v), np.rint(v * 1e5) / 1e5, v)


def table(rows16: np.ndarray, L: int, period: int, precise=None) -> np.ndarray:
    """[R, 30] float64: DataAnalyzer.initialize(period) of the log whose rows are `rows16` (ReplayResult.row_array), frame units."""
    r = np.asarray(rows16, dtype=np.float64)
    R = len(r)
    t = np.full((R, len(COLUMNS)), np.nan)
    frame = np.arange(R, dtype=np.float64)
    t[:, 0], t[:, 1], t[:, 2:16] = frame, r[:, 14], r[:, 0:14]
    t[:, COL["time"]], t[:, COL["cycle_step"]] = frame, np.arange(R) % L
    wx, wy, ww, wh = r[:, 10], r[:, 11], r[:, 12], r[:, 13]
    mx, my, mw, mh = r[:, 6], r[:, 7], r[:, 8], r[:, 9]
    wcx, wcy, mcx, mcy = wx + ww / 2, wy + wh / 2, mx + mw / 2, my + mh / 2
    sx, sy = np.full(R, np.nan), np.full(R, np.nan)
    if R > period:
        sx[period:], sy[period:] = (wcx[period:] - wcx[:-period]) / float(period), (wcy[period:] - wcy[:-period]) / float(period)
    dx, dy = wcx - mcx, wcy - mcy
    iw = np.maximum(0.0, np.minimum(wx + ww, mx + mw) - np.maximum(wx, mx))
    ih = np.maximum(0.0, np.minimum(wy + wh, my + mh) - np.maximum(wy, my))
    total = ww * wh
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.where(total == 0, 0.0, 1.0 - (iw * ih) / total)
    for name, v in (("wrm_center_x", wcx), ("wrm_center_y", wcy), ("mic_center_x", mcx), ("mic_center_y", mcy), ("wrm_speed_x", sx), ("wrm_speed_y", sy),
                    ("wrm_speed", np.sqrt(sx * sx + sy * sy)), ("worm_deviation_x", dx), ("worm_deviation_y", dy),
                    ("worm_deviation", np.sqrt(dx * dx + dy * dy)), ("bbox_error", err)):
        t[:, COL[name]] = v
    t = round5(t)
    if precise is not None:
        t[:, COL["precise_error"]] = precise  # assigned after the rounding (calc_precise_error)
    return t


def pre_mask(tab: np.ndarray, phase: np.ndarray, spec: Spec) -> np.ndarray:
    """The rows the first two filters of DataAnalyzer.clean keep."""
    keep = np.ones(len(tab), dtype=bool)
    if spec.imaging_only:
        keep &= np.asarray(phase) == 0
    if spec.bounds is not None:
        b = spec.bounds
        c = lambda n: tab[:, COL[n]]  # noqa: E731
        has_pred = np.isfinite(tab[:, 12:16]).all(axis=1)
        wrm = has_pred & (c("wrm_x") >= b[0]) & (c("wrm_x") + c("wrm_w") <= b[2]) & (c("wrm_y") >= b[1]) & (c("wrm_y") + c("wrm_h") <= b[3])
        # The reference writes `mask_wrm = has_pred; mask_wrm &= ...` on a numpy array, which updates has_pred in place: by the time it forms
        # `mask_mic = ~has_pred` that name holds the finished worm mask.  What it keeps is therefore (has_pred & worm inside) | microscope inside,
        # checked on the real DataAnalyzer with a seven-row frame; tests/golden/analysis.npz pins it (rows 120 and 251 of csv_100, configuration a).
        mic = (c("mic_x") >= b[0]) & (c("mic_x") + c("mic_w") <= b[2]) & (c("mic_y") >= b[1]) & (c("mic_y") + c("mic_h") <= b[3])
        keep &= wrm | (~wrm & mic)
    return keep


def keep_mask(tab: np.ndarray, phase: np.ndarray, spec: Spec) -> np.ndarray:
    keep = pre_mask(tab, phase, spec)
    if spec.trim_cycles and keep.any():
        cyc = tab[:, COL["cycle"]]
        keep &= (cyc != 0) & (cyc != cyc[keep].max())
    return keep


def to_unit(tab: np.ndarray, factors) -> np.ndarray:
    """DataAnalyzer.change_unit on the (rounded) table: one multiplication per value."""
    tf, dist, speed = (float(f) for f in factors)
    out = tab.copy()
    out[:, COL["time"]] *= tf
    for n in DIST_COLUMNS:
        out[:, COL[n]] *= dist
    for n in SPEED_COLUMNS:
        out[:, COL[n]] *= speed
    return out


def seq_sum(v) -> float:
    s = 0.0
    for x in v:
        s += float(x)
    return s


def quantile(sorted_v: np.ndarray, q: float) -> float:
    """numpy's `linear` percentile of an ascending array (what DataFrame.describe and quantile call)."""
    n = len(sorted_v)
    if n == 0:
        return math.nan
    pos = q * (n - 1)
    lo = int(math.floor(pos))
    t = pos - lo
    a, b = float(sorted_v[lo]), float(sorted_v[min(lo + 1, n - 1)])
    return a + (b - a) * t if t < 0.5 else b - (b - a) * (1 - t)


def describe(values: np.ndarray, percentiles) -> np.ndarray:
    """[5 + Q]: count of the non-NaN values, mean, std (ddof 1, two passes about the computed mean), min, the percentiles, max."""
    v = np.sort(values[~np.isnan(values)])
    n, Q = len(v), len(percentiles)
    out = np.full(5 + Q, np.nan)
    out[0] = n
    if n == 0:
        return out
    mean = seq_sum(v) / n
    out[1] = mean
    if n > 1:
        out[2] = math.sqrt(seq_sum((v - mean) * (v - mean)) / (n - 1))
    out[3], out[4 + Q] = v[0], v[-1]
    out[4:4 + Q] = [quantile(v, q) for q in percentiles]
    return out


def anomaly_bits(tab_u: np.ndarray, spec: Spec) -> np.ndarray:
    """uint8 [R] calc_anomalies' six masks as bits (on every row; the caller keeps the kept ones).  Comparisons with NaN are false."""
    c = lambda n: tab_u[:, COL[n]]  # noqa: E731
    with np.errstate(invalid="ignore"):
        bits = (c("wrm_speed") >= spec.min_speed) * 1 + (c("bbox_error") >= spec.min_bbox_error) * 2 + (c("worm_deviation") >= spec.min_dist_error) * 4
        bits = bits + (c("wrm_w") >= spec.min_width) * 8 + (c("wrm_h") >= spec.min_height) * 16
    no_pred = ~np.isfinite(tab_u[:, 12:16]).all(axis=1)
    if spec.no_preds:
        bits = bits + no_pred * 32
    return bits.astype(np.uint8)


def analyze(rows16: np.ndarray, L: int, spec: Spec, precise=None) -> dict:
    """One experiment's analysis: describe [n_cols, 5 + Q], cycle_max / cycle_mean [n_log, n_cols], step_quantiles [L, n_cols, Q], step_count
    [L, n_cols], anomaly_counts [7], anomaly_mask uint8 [R], stats [4] (removed rows, no-pred rows, distinct cycles kept, rows with bbox_error > 1e-7),
    and `table` (frame units, uncleaned), `keep`."""
    rows16 = np.asarray(rows16, dtype=np.float64)
    R = len(rows16)
    n_log = R // L
    tab = table(rows16, L, spec.period, precise)
    keep = keep_mask(tab, rows16[:, 15], spec)
    tab_u = to_unit(tab, spec.factors)
    cols = [COL[c] if isinstance(c, str) else int(c) for c in spec.columns]
    Q = len(spec.percentiles)
    step, cyc = np.arange(R) % L, np.arange(R) // L
    out = dict(table=tab, keep=keep)
    out["describe"] = np.stack([describe(tab_u[keep, c], spec.percentiles) for c in cols])
    cmax, cmean = np.full((n_log, len(cols)), np.nan), np.full((n_log, len(cols)), np.nan)
    for k in range(n_log):
        for j, c in enumerate(cols):
            v = tab_u[keep & (cyc == k), c]
            v = v[~np.isnan(v)]
            if len(v):
                cmax[k, j], cmean[k, j] = v.max(), seq_sum(v) / len(v)
    out["cycle_max"], out["cycle_mean"] = cmax, cmean
    sq, sc = np.full((L, len(cols), Q), np.nan), np.zeros((L, len(cols)), dtype=np.int64)
    for s in range(L):
        for j, c in enumerate(cols):
            d = describe(tab_u[keep & (step == s), c], spec.percentiles)
            sq[s, j], sc[s, j] = d[4:4 + Q], int(d[0])
    out["step_quantiles"], out["step_count"] = sq, sc
    bits = np.where(keep, anomaly_bits(tab_u, spec), 0).astype(np.uint8)
    out["anomaly_mask"] = bits
    out["anomaly_counts"] = np.array([int(((bits >> k) & 1).sum()) for k in range(6)] + [int((bits != 0).sum())], dtype=np.int64)
    kept = tab_u[keep]
    with np.errstate(invalid="ignore"):
        out["stats"] = np.array([R - len(kept), int(np.isnan(kept[:, 12:16]).any(axis=1).sum()), len(np.unique(kept[:, COL["cycle"]])),
                                 int((kept[:, COL["bbox_error"]] > 1e-7).sum())], dtype=np.int64)
    return out


def mean_bound(values: np.ndarray) -> float:
    """|mean_a - mean_b| of two summation orders: each sum is within (n - 1) 2^-53 sum|x| of the exact one, so the means differ by at most
    2 (n - 1) 2^-53 mean|x| plus the division's half ulp: n 2^-52 mean|x| covers it."""
    v = values[~np.isnan(values)]
    return len(v) * 2.0 ** -52 * float(np.abs(v).mean()) if len(v) else 0.0


def std_bound(n: int) -> float:
    """Relative: the first-order bound of a two-pass variance in any order is (n + 3) 2^-53; two implementations differ by at most twice that."""
    return n * 2.0 ** -52
