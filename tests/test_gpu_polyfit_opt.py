"""GPU tests of the Polyfit weight search (wtracker_amd/polyfit_opt.py, csrc/polyfit_opt.hip) against the REAL reference's WeightEvaluator through
tests/golden/polyfit_opt.npz, and against the numpy restatement that tests/test_polyfit_opt_ref.py pins to it.

Tolerance of every MAE value: 100 x the fixture's `restatement_dev` (7.8e-14 when the fixture was written, so 7.8e-12) relative to the reference's
value, never above 1e-10.  The tests print the worst deviation per configuration and degree before they assert (run with -s); figures measured
so far: DESIGN.md section 14 and profiles/r08_notes.md."""
import json
import os

import numpy as np
import pytest

from harness import polyfit_opt_ref as ref
from harness.sim_harness import Simulator
from test_polyfit_opt_ref import load_fixture, timing_of

pytestmark = pytest.mark.gpu

CHUNK = 4096  # kMaeChunk of csrc/polyfit_opt.hip


def evaluator(z, tag, tracks=None, **kw):
    from wtracker_amd.polyfit_opt import WeightEvaluator

    _, tc = timing_of(z, tag)
    speed = kw.pop("speed", tuple(z[f"{tag}_speed"]))
    return WeightEvaluator.from_tracks([z["track"]] if tracks is None else tracks, tc, z[f"{tag}_offsets_given"], int(z[f"{tag}_pred_time_offset"]),
                                       min_speed=speed[0], max_speed=speed[1], **kw)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------- 1. dataset
@pytest.mark.parametrize("tag", ["a", "b"])
def test_dataset_equals_the_reference(hip_lib, golden_dir, tag, tmp_path):
    import torch

    z, _ = load_fixture(golden_dir)
    ev = evaluator(z, tag)
    np.testing.assert_array_equal(ev.y_input.cpu().numpy(), z[f"{tag}_y_input"])
    np.testing.assert_array_equal(ev.y_target.cpu().numpy(), z[f"{tag}_y_target"])
    np.testing.assert_array_equal(ev.x_input.cpu().numpy(), z[f"{tag}_x_input"])
    np.testing.assert_array_equal(ev.x_target.cpu().numpy(), np.full_like(z[f"{tag}_y_target"], int(z[f"{tag}_pred_time_offset"])))
    kept, cand = int(z[f"{tag}_kept"]), -(-6000 // int(z[f"{tag}_cycle_frame_num"]))
    assert ev.cycle_stats == [(cand, kept, cand - kept)] and ev.n_series == 2 * kept
    # a track that is already on the device, and the csv constructor (the reference's signature)
    ev2 = evaluator(z, tag, tracks=[torch.from_numpy(z["track"]).cuda()])
    assert torch.equal(ev2.y_input, ev.y_input) and torch.equal(ev2.y_target, ev.y_target)
    csv = str(tmp_path / "bboxes.csv")
    with open(csv, "w") as f:
        f.write("frame,wrm_x,wrm_y,wrm_w,wrm_h\n")
        for i, r in enumerate(z["track"]):
            f.write(f"{i}," + ",".join("" if not np.isfinite(v) else repr(float(v)) for v in r) + "\n")
    from wtracker_amd.polyfit_opt import WeightEvaluator

    _, tc = timing_of(z, tag)
    ev3 = WeightEvaluator([csv], tc, z[f"{tag}_offsets_given"], int(z[f"{tag}_pred_time_offset"]), *z[f"{tag}_speed"])
    assert torch.equal(ev3.y_input, ev.y_input) and torch.equal(ev3.y_target, ev.y_target)


def test_dataset_two_logs_empty_and_float32(hip_lib, golden_dir):
    z, _ = load_fixture(golden_dir)
    tag = "a"
    L, off, pred, speed = int(z["a_cycle_frame_num"]), z["a_offsets_given"], int(z["a_pred_time_offset"]), tuple(z["a_speed"])
    # two logs append along the series axis, the second one shorter (its last candidate cycle is a partial one)
    short = z["track"][:3001]
    ev = evaluator(z, tag, tracks=[z["track"], short])
    y2, t2, k2 = ref.dataset(short, L, off, pred, *speed)
    np.testing.assert_array_equal(ev.y_input.cpu().numpy(), np.concatenate([z["a_y_input"], y2], axis=1))
    np.testing.assert_array_equal(ev.y_target.cpu().numpy(), np.concatenate([z["a_y_target"], t2]))
    assert [s[1] for s in ev.cycle_stats] == [int(z["a_kept"]), k2] and k2 > 0 and ev.cycle_stats[1][0] == -(-3001 // L)
    # no surviving cycle: M = 0, eval is NaN as np.mean of an empty array
    for empty in (evaluator(z, tag, speed=(1e9, 2e9)), evaluator(z, tag, tracks=[np.full((500, 4), np.nan)]), evaluator(z, tag, tracks=[z["track"][:10]])):
        assert empty.n_series == 0 and tuple(empty.y_input.shape) == (8, 0) and tuple(empty.y_target.shape) == (0,) and empty.cycle_stats[0][1] == 0
        assert np.isnan(empty.eval(np.ones(8), 2)) and np.isnan(empty.eval_many(np.ones((3, 8)), 1).cpu().numpy()).all()
    # float32 tracks are widened on the device: the harness on the float32-rounded track.  A seeded track OFF the fixture's 1/16 px grid, so that the
    # rounding to float32 changes values.
    rng = np.random.default_rng(5)
    t = np.cumsum(rng.normal(0.4, 0.3, size=(4000, 2)), axis=0) + [700.0, 500.0]
    t = np.concatenate([t, rng.normal((13.8, 14.6), 0.6, (4000, 2))], axis=1)
    t[rng.choice(4000, 20, replace=False)] = np.nan
    t32 = t.astype(np.float32)
    assert not np.array_equal(t32.astype(np.float64), t, equal_nan=True)
    for tr in (t32, t):
        ev = evaluator(z, tag, tracks=[tr])
        y, tg, k = ref.dataset(tr, L, off, pred, *speed)
        assert 0 < k < -(-4000 // L) - 3
        np.testing.assert_array_equal(ev.y_input.cpu().numpy(), y)
        np.testing.assert_array_equal(ev.y_target.cpu().numpy(), tg)


# ------------------------------------------------------------------------------------------------- 2. eval_many against the reference's eval
def test_eval_many_matches_the_reference_on_every_fixture_value(hip_lib, golden_dir):
    z, tol = load_fixture(golden_dir)
    worst, n_values = 0.0, 0
    for tag in ("a", "b"):
        ev = evaluator(z, tag)
        w = z[f"{tag}_weights"]
        for di, deg in enumerate(z["degrees"]):
            want = z[f"{tag}_mae"][di]
            got = ev.eval_many(w, int(deg)).cpu().numpy()
            assert got.shape == want.shape == (256,) and np.isfinite(got).all()
            dev = np.abs(got - want) / np.abs(want)
            print(f"config {tag} degree {deg}: worst relative deviation {dev.max():.3e} at row {int(dev.argmax())} (tolerance {tol:.3e})")
            worst, n_values = max(worst, float(dev.max())), n_values + got.size
            assert (dev <= tol).all(), (tag, int(deg), np.flatnonzero(dev > tol)[:8], dev.max())
            # eval(w) is the same arithmetic as its row in a population: the same bits
            for r in (0, 7, 203, 225, 240, 241, 245, 252):
                assert bits([ev.eval(w[r], int(deg))])[0] == bits(got)[r], (tag, int(deg), r)
            # ordering of the candidates, wherever the reference separates two of them by more than twice the tolerance
            gap = 2.0 * tol * np.maximum(np.abs(want)[:, None], np.abs(want)[None, :])
            apart = np.abs(want[:, None] - want[None, :]) > gap
            assert apart.sum() > 60000
            assert (np.sign(got[:, None] - got[None, :])[apart] == np.sign(want[:, None] - want[None, :])[apart]).all()
    assert n_values == 1536
    print(f"worst relative deviation of the device over all {n_values} values: {worst:.3e}")


# ------------------------------------------------------------------------------------------------- 3. determinism
def test_eval_many_is_deterministic_whatever_the_population(hip_lib, golden_dir):
    z, tol = load_fixture(golden_dir)
    rng = np.random.default_rng(9)
    # one chunk (M = 652) and several chunks with a remainder (16 copies of the log: M = 10 432 = 2 * 4096 + 2240)
    for tracks in ([z["track"]], [z["track"]] * 16):
        ev = evaluator(z, "a", tracks=tracks)
        assert ev.n_series % CHUNK != 0 and (len(tracks) == 1 or ev.n_series > 2 * CHUNK)
        w = rng.random((1000, 8))
        first = ev.eval_many(w, 2).cpu().numpy()
        again = ev.eval_many(w, 2).cpu().numpy()
        assert np.array_equal(bits(first), bits(again))
        assert np.array_equal(bits(ev.eval_many(w[:100], 2).cpu().numpy()), bits(first[:100]))
        assert np.array_equal(bits(ev.eval_many(w[417:418], 2).cpu().numpy()), bits(first[417:418]))
        y_in, y_tg = ev.y_input.cpu().numpy(), ev.y_target.cpu().numpy()
        for r in range(0, 1000, 37):  # and the values are the restatement's (the many-chunk path has no fixture of its own)
            want = ref.mae(y_in, y_tg, z["a_x_input"], w[r], 2, float(z["a_pred_time_offset"]))
            assert abs(first[r] - want) <= tol * abs(want), (len(tracks), r, first[r], want)
    # weights that are not finite give NaN, never a number
    bad = np.ones((3, 8))
    bad[0, 2], bad[1, 5] = np.nan, np.inf
    out = ev.eval_many(bad, 2).cpu().numpy()
    assert np.isnan(out[0]) and np.isnan(out[1]) and np.isfinite(out[2])


# ------------------------------------------------------------------------------------------------- 4. search
def test_search_is_reproducible_monotone_and_stops_early(hip_lib, golden_dir):
    z, _ = load_fixture(golden_dir)
    ev = evaluator(z, "a")
    a = ev.optimize(2, pop_size=40, max_epoch=60, max_early_stop=60, seed=3)
    b = ev.optimize(2, pop_size=40, max_epoch=60, max_early_stop=60, seed=3)
    assert np.array_equal(bits(a.weights), bits(b.weights)) and bits([a.mae])[0] == bits([b.mae])[0] and np.array_equal(bits(a.history), bits(b.history))
    assert a.epochs == b.epochs == 60 and a.history.shape == (60,) and np.isfinite(a.history).all()
    assert (np.diff(a.history) <= 0).all() and a.history[-1] < a.history[0]
    assert ((a.weights >= 0) & (a.weights <= 1)).all()
    c = ev.optimize(2, pop_size=40, max_epoch=60, max_early_stop=60, seed=4)
    assert not np.array_equal(c.weights, a.weights)
    # the result is what eval says of it, bit for bit, and never worse than uniform weights (particle 0 starts there)
    assert bits([ev.eval(a.weights, 2)])[0] == bits([a.mae])[0] == bits(a.history[-1:])[0]
    uniform = ev.eval(np.ones(8), 2)
    assert a.mae <= uniform and a.history[0] <= uniform
    # early stop on the device: fewer epochs than asked for, flat over the last 5
    s = ev.optimize(2, pop_size=10, max_epoch=300, max_early_stop=5, seed=1)
    assert 5 < s.epochs < 300 and s.history.shape == (s.epochs,)
    assert (s.history[-5:] == s.history[-6]).all() and bits([ev.eval(s.weights, 2)])[0] == bits([s.mae])[0]


def test_swarm_step_matches_a_numpy_replay_of_the_documented_rule(hip_lib, golden_dir):
    """The step kernel alone: the numpy replay is fed the device's own MAE values, so rounding in the evaluation plays no part.  Every operation of the
    rule is one IEEE-754 double operation on both sides (the library is built without contraction), so the states must agree bit for bit."""
    from wtracker_amd.polyfit_opt import WeightEvaluator

    z, _ = load_fixture(golden_dir)
    ev = evaluator(z, "b")
    P, E, N, seed, c1, c2, lb, ub = 10, 5, 6, 7, 2.05, 2.05, 0.0, 1.0
    trace = []
    res = ev.optimize(1, pop_size=P, c1=c1, c2=c2, max_epoch=E, max_early_stop=100, seed=seed, lb=lb, ub=ub, _trace=trace)
    rng = np.random.default_rng(seed)
    x0 = lb + (ub - lb) * rng.random((P, N))
    x0[0, :] = ub
    rand = rng.random((E, 2, P, N))
    st = dict(pos=x0, vel=np.zeros((P, N)), pbest_pos=x0.copy(), pbest_val=np.full(P, np.inf), gbest_pos=x0[0].copy(), gbest_val=np.inf, since=0, history=[])
    assert len(trace) == E and res.epochs == E
    moved = 0
    for e, (pos, vel, mae) in enumerate(trace):
        assert np.array_equal(bits(pos.cpu().numpy()), bits(st["pos"])), e
        assert np.array_equal(bits(vel.cpu().numpy()), bits(st["vel"])), e
        before = st["pos"].copy()
        stop = ref.swarm_step(st, mae.cpu().numpy(), rand[e], WeightEvaluator.W_MAX - (WeightEvaluator.W_MAX - WeightEvaluator.W_MIN) * e / E, c1, c2, lb, ub, 100)
        assert not stop
        moved += int((st["pos"] != before).sum())
    assert moved > 3 * P * N
    assert np.array_equal(bits(res.weights), bits(st["gbest_pos"])) and bits([res.mae])[0] == bits([st["gbest_val"]])[0]
    assert np.array_equal(bits(res.history), bits(np.asarray(st["history"])))


# ------------------------------------------------------------------------------------------------- 5. closing the loop
def _moves(ctrl_factory, tc, ec):
    ctrl = ctrl_factory(tc)
    moves = []
    inner = ctrl.provide_movement_vector

    def wrapped(sim):
        dx, dy = inner(sim)
        moves.append([int(sim.frame_number), int(dx), int(dy)])
        return dx, dy

    ctrl.provide_movement_vector = wrapped
    Simulator(tc, ec, ctrl).run()
    return moves


def test_search_result_drives_the_polyfit_controllers(hip_lib, golden_dir, tmp_path):
    import importlib.util
    import subprocess
    import sys

    from wtracker_amd.controllers import HipPolyfitController, PolyfitConfig, PolyfitController

    z, _ = load_fixture(golden_dir)
    n = 1500
    csv = str(tmp_path / "bboxes.csv")
    with open(csv, "w") as f:
        f.write("frame,wrm_x,wrm_y,wrm_w,wrm_h\n")
        for i, r in enumerate(z["track"][:n]):
            f.write(f"{i}," + ",".join("" if not np.isfinite(v) else repr(float(v)) for v in r) + "\n")
    ec, tc = timing_of(z, "a", num_frames=n)
    ev = evaluator(z, "a")
    res = ev.optimize(2, pop_size=30, max_epoch=40, max_early_stop=40, seed=0)
    cfg = ev.to_config(2, res.weights)
    assert isinstance(cfg, PolyfitConfig) and cfg.sample_times == [int(t) for t in z["a_x_input"]] and cfg.weights == [float(v) for v in res.weights]
    dev_moves = _moves(lambda t: HipPolyfitController(t, cfg, csv), tc, ec)
    host_moves = _moves(lambda t: PolyfitController(t, cfg, csv), tc, ec)
    assert dev_moves == host_moves and len(dev_moves) == n // tc.cycle_frame_num and any(m[1:] != [0, 0] for m in dev_moves)
    # the script: a JSON file with the three keys, from which PolyfitConfig(**json.load(f)) builds a config the device controller accepts
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "polyfit_config.json")
    run = subprocess.run([sys.executable, os.path.join(root, "tools", "optimize_polyfit_weights.py"), csv, "--out", out, "--degrees", "1", "2", "--pop-size", "20",
                          "--max-epoch", "30", "--seed", "2"], capture_output=True, text=True, timeout=900)
    assert run.returncode == 0, run.stderr[-3000:]
    raw = json.load(open(out))
    assert sorted(raw) == ["degree", "sample_times", "weights"] and raw["degree"] in (1, 2) and len(raw["weights"]) == 8
    for d in (1, 2):
        assert json.load(open(str(tmp_path / f"polyfit_config_deg{d}.json")))["degree"] == d
    cfg2 = PolyfitConfig(**raw)
    assert len(_moves(lambda t: HipPolyfitController(t, cfg2, csv), tc, ec)) == n // tc.cycle_frame_num
