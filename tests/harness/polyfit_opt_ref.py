"""Float64 numpy restatement of the reference's WeightEvaluator (wtracker/sim/sim_controllers/polyfit_controller.py:87-221): test infrastructure,
not product.  The reference cannot travel to the GPU box, so the GPU tests of wtracker_amd.polyfit_opt lean on this module; it is pinned, not
trusted: tests/test_polyfit_opt_ref.py requires its datasets to equal the real reference's bit for bit and its MAE values to agree with the real
reference's `eval` within the tolerance of the fixture (tests/golden/polyfit_opt.npz).

  dataset(track, ...)     _extract_positions: per-cycle input / target centres, time / finiteness / speed filters, cycles in order
  prediction_row(...)     g with y_pred[m] = sum_n g[n] * y_input[n, m]: numpy's weighted polyfit (column scaling, rcond = N * eps) followed by
                          polyval at t_pred, folded into one row through the pseudo-inverse of the scaled weighted Vandermonde matrix
  mae(...)                mean |y_target - g @ y_input|
  swarm_step(...)         the update rule documented in WeightEvaluator.optimize, one epoch
"""
from __future__ import annotations

import numpy as np


def dataset(track: np.ndarray, cycle_frame_num: int, input_time_offsets, pred_time_offset: int, min_speed: float = 0.0, max_speed: float = np.inf):
    """(y_input [N, 2 * kept], y_target [2 * kept], kept) of one log; `track` [n_frames, 4] xywh (computed in float64 whatever its dtype)."""
    track = np.asarray(track).astype(np.float64)
    off = np.sort(np.asarray(input_time_offsets, dtype=np.int64))
    N, n = len(off), len(track)
    centers = np.stack([track[:, 0] + track[:, 2] / 2, track[:, 1] + track[:, 3] / 2], axis=1)
    starts = np.arange(0, n, cycle_frame_num, dtype=np.int64)
    t_in = starts[:, None] + off[None, :]
    t_tg = starts + pred_time_offset
    ok = (t_in >= 0).all(axis=1) & (t_tg < n)
    t_in, t_tg = t_in[ok], t_tg[ok]
    y_in = centers[t_in.reshape(-1)].reshape(-1, N, 2)
    y_tg = centers[t_tg].reshape(-1, 2)
    ok = np.isfinite(y_in).all(axis=(1, 2)) & np.isfinite(y_tg).all(axis=1)
    y_in, y_tg = y_in[ok], y_tg[ok]
    d = y_tg - y_in[:, 0, :]
    speed = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) / (pred_time_offset - off[0])
    ok = (speed >= min_speed) & (speed <= max_speed)
    y_in, y_tg = y_in[ok], y_tg[ok]
    return np.ascontiguousarray(y_in.swapaxes(0, 1).reshape(N, -1)), y_tg.reshape(-1), int(len(y_tg))


def prediction_row(times, weights, deg: int, t_pred: float) -> np.ndarray:
    t = np.asarray(times, dtype=np.float64)
    w = np.asarray(weights, dtype=np.float64)
    van = np.vander(t, deg + 1, increasing=True)
    A = van * w[:, None]
    scl = np.sqrt(np.square(A).sum(axis=0))
    scl[scl == 0] = 1
    pinv = np.linalg.pinv(A / scl, rcond=len(t) * np.finfo(np.float64).eps)  # [deg + 1, N]: singular values <= rcond * s_max dropped, as lstsq does
    v = np.vander(np.asarray([t_pred], dtype=np.float64), deg + 1, increasing=True)[0]
    return ((v / scl) @ pinv) * w


def mae(y_input: np.ndarray, y_target: np.ndarray, times, weights, deg: int, t_pred: float) -> float:
    if y_target.size == 0:
        return float("nan")
    g = prediction_row(times, weights, deg, t_pred)
    return float(np.mean(np.abs(y_target - g @ y_input)))


def swarm_step(state: dict, mae_values: np.ndarray, r: np.ndarray, w: float, c1: float, c2: float, lb: float, ub: float, max_early_stop: int) -> bool:
    """One epoch of the documented rule on `state` (pos, vel, pbest_pos, pbest_val, gbest_pos, gbest_val, since, history) in place, from the MAE
    values of state['pos']; r [2, P, N].  Returns True when the search stops after this epoch (the positions then stay as they are)."""
    better = mae_values < state["pbest_val"]
    state["pbest_val"] = np.where(better, mae_values, state["pbest_val"])
    state["pbest_pos"] = np.where(better[:, None], state["pos"], state["pbest_pos"])
    i = int(np.argmin(np.where(np.isnan(state["pbest_val"]), np.inf, state["pbest_val"])))  # first lowest
    state["since"] += 1
    if state["pbest_val"][i] < state["gbest_val"]:
        state["gbest_val"], state["gbest_pos"], state["since"] = state["pbest_val"][i], state["pbest_pos"][i].copy(), 0
    state["history"].append(state["gbest_val"])
    if state["since"] >= max_early_stop:
        return True
    x, vmax = state["pos"], 0.5 * (ub - lb)
    v = (w * state["vel"] + (c1 * r[0]) * (state["pbest_pos"] - x)) + (c2 * r[1]) * (state["gbest_pos"][None, :] - x)
    v = np.minimum(np.maximum(v, -vmax), vmax)
    state["vel"] = v
    state["pos"] = np.minimum(np.maximum(x + v, lb), ub)
    return False
