"""CPU checks of the Polyfit weight search: the numpy restatement the GPU tests lean on (tests/harness/polyfit_opt_ref.py) is pinned to the REAL
reference's WeightEvaluator through tests/golden/polyfit_opt.npz, and the host-side argument checks of wtracker_amd.polyfit_opt raise before any
device work.  The tolerance is the fixture's own: 100 x the deviation measured between the reference's eval and the restatement when the fixture
was written (factor 100: a Jacobi SVD rounds differently from LAPACK's, and the sum over the series runs in another order), capped at 1e-10."""
import os

import numpy as np
import pytest

from harness import polyfit_opt_ref as ref
from wtracker_amd import hip
from wtracker_amd.sim import ExperimentConfig, TimingConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "polyfit_opt.npz"))
    tol = min(100.0 * float(z["restatement_dev"]), 1e-10)
    return z, tol


def timing_of(z, tag, num_frames=6000):
    ec = ExperimentConfig("exp", num_frames, 60, (1600, 1400), 90, (900, 700))
    tc = TimingConfig(ec, *[float(v) for v in z[f"{tag}_timing"]], (4, 4), (0.32, 0.32))
    assert tc.cycle_frame_num == int(z[f"{tag}_cycle_frame_num"])
    return ec, tc


def test_fixture_is_what_the_issue_asks_for(golden_dir):
    z, tol = load_fixture(golden_dir)
    assert 0.0 < float(z["restatement_dev"]) < 1e-12 and tol <= 1e-10
    assert z["track"].shape == (6000, 4) and 20 <= int(np.isnan(z["track"]).any(axis=1).sum()) <= 40
    assert list(z["degrees"]) == [1, 2, 3]
    for tag, n in (("a", 8), ("b", 6)):
        w = z[f"{tag}_weights"]
        assert w.shape == (256, n) and z[f"{tag}_mae"].shape == (3, 256) and np.isfinite(z[f"{tag}_mae"]).all()
        assert (w[240] == 1).all() and (w[241] == 0).all() and ((w != 0).sum(axis=1) <= 3).sum() >= 20
        assert list(z[f"{tag}_x_input"]) == sorted(z[f"{tag}_offsets_given"])
        candidates = -(-6000 // int(z[f"{tag}_cycle_frame_num"]))
        assert 0 < int(z[f"{tag}_kept"]) < candidates - 40  # the speed window removed the slow stretch, not only the NaN rows
    assert list(z["b_offsets_given"]) != sorted(z["b_offsets_given"])  # the sort quirk is exercised


@pytest.mark.parametrize("tag", ["a", "b"])
def test_harness_dataset_equals_the_reference_bit_for_bit(golden_dir, tag):
    z, _ = load_fixture(golden_dir)
    y_in, y_tg, kept = ref.dataset(z["track"], int(z[f"{tag}_cycle_frame_num"]), z[f"{tag}_offsets_given"], int(z[f"{tag}_pred_time_offset"]), *z[f"{tag}_speed"])
    np.testing.assert_array_equal(y_in, z[f"{tag}_y_input"])
    np.testing.assert_array_equal(y_tg, z[f"{tag}_y_target"])
    assert kept == int(z[f"{tag}_kept"])


@pytest.mark.parametrize("tag", ["a", "b"])
def test_harness_mae_agrees_with_the_reference(golden_dir, tag):
    z, tol = load_fixture(golden_dir)
    worst = 0.0
    for di, deg in enumerate(z["degrees"]):
        for r, w in enumerate(z[f"{tag}_weights"]):
            got = ref.mae(z[f"{tag}_y_input"], z[f"{tag}_y_target"], z[f"{tag}_x_input"], w, int(deg), float(z[f"{tag}_pred_time_offset"]))
            want = z[f"{tag}_mae"][di, r]
            worst = max(worst, abs(got - want) / abs(want))
    print(f"config {tag}: worst relative deviation of the restatement {worst:.3e} (tolerance {tol:.3e})")
    assert worst <= tol
    assert np.isnan(ref.mae(np.zeros((3, 0)), np.zeros(0), [0, 1, 2], [1, 1, 1], 1, 4.0))


def test_new_module_symbols_and_script_exist(hip_lib):
    from wtracker_amd import polyfit_opt

    for name in ("wtk_polyfit_dataset", "wtk_polyfit_mae_scratch_doubles", "wtk_polyfit_weight_mae", "wtk_polyfit_swarm_step"):
        assert name in hip.SYMBOLS and hasattr(hip_lib, name), name
    assert hip_lib.wtk_polyfit_mae_scratch_doubles(100, 4097) == 100 * (16 + 2) and hip_lib.wtk_polyfit_mae_scratch_doubles(-1, 0) == -1
    for attr in ("eval", "eval_many", "optimize", "to_config", "from_tracks"):
        assert hasattr(polyfit_opt.WeightEvaluator, attr), attr
    for tool in ("optimize_polyfit_weights.py", "polyfit_opt_timing.py"):
        assert os.path.exists(os.path.join(ROOT, "tools", tool)), tool
    from wtracker_amd import _build

    assert "polyfit_opt.hip" in _build.SOURCES and "polyfit_solve.h" in _build.HEADERS


def test_entry_points_refuse_bad_arguments_before_any_launch(hip_lib):
    import ctypes as C

    off = np.asarray([-3, 0, 2], dtype=np.int32)
    p, one = C.c_void_p(64), C.c_void_p(0)
    # null pointers, unsorted offsets, too many times, an input offset beyond the prediction offset, a zero speed span
    assert hip_lib.wtk_polyfit_dataset(one, 1, 10, 5, off.ctypes.data, 3, 4, 0.0, 1.0, p, p, 4, p, None) != 0
    bad = np.asarray([0, -3, 2], dtype=np.int32)
    assert hip_lib.wtk_polyfit_dataset(p, 1, 10, 5, bad.ctypes.data, 3, 4, 0.0, 1.0, p, p, 4, p, None) != 0 and b"sorted" in hip_lib.wtk_last_error()
    many = np.arange(17, dtype=np.int32)
    assert hip_lib.wtk_polyfit_dataset(p, 1, 10, 5, many.ctypes.data, 17, 40, 0.0, 1.0, p, p, 4, p, None) != 0 and b"16" in hip_lib.wtk_last_error()
    assert hip_lib.wtk_polyfit_dataset(p, 1, 10, 5, off.ctypes.data, 3, 1, 0.0, 1.0, p, p, 4, p, None) != 0 and b"beyond" in hip_lib.wtk_last_error()
    assert hip_lib.wtk_polyfit_weight_mae(p, p, 8, 8, off.ctypes.data, 3, 4, 8, p, 2, p, p, 1000, None, None) != 0 and b"degree" in hip_lib.wtk_last_error()
    assert hip_lib.wtk_polyfit_weight_mae(p, p, 8, 8, off.ctypes.data, 3, 4, 2, p, 2, p, p, 3, None, None) != 0 and b"scratch" in hip_lib.wtk_last_error()
    assert hip_lib.wtk_polyfit_weight_mae(p, p, 4, 8, off.ctypes.data, 3, 4, 2, p, 2, p, p, 1000, None, None) != 0
    assert hip_lib.wtk_polyfit_swarm_step(p, p, 4, 17, 0, 5, 0.9, 2.0, 2.0, 0.0, 1.0, 0.5, p, p, p, p, p, p, p, p, None) != 0
    assert hip_lib.wtk_polyfit_swarm_step(p, p, 4, 3, 0, 5, 0.9, 2.0, 2.0, 1.0, 1.0, 0.5, p, p, p, p, p, p, p, p, None) != 0 and b"lb < ub" in hip_lib.wtk_last_error()


def _bare_evaluator(offsets=(-6, -3, 0, 2), pred=9):
    """An evaluator with its configuration checked and no dataset: enough for the checks that must fire before the device is touched."""
    from wtracker_amd.polyfit_opt import WeightEvaluator

    ec = ExperimentConfig("exp", 100, 60, (1600, 1400), 90, (900, 700))
    ev = WeightEvaluator.__new__(WeightEvaluator)
    ev._setup(TimingConfig(ec, 100, 40, 50, (4, 4), (0.32, 0.32)), offsets, pred, 0.0, np.inf)
    return ev


def test_python_argument_checks_raise(hip_lib):
    from wtracker_amd.polyfit_opt import WeightEvaluator

    ec = ExperimentConfig("exp", 100, 60, (1600, 1400), 90, (900, 700))
    tc = TimingConfig(ec, 100, 40, 50, (4, 4), (0.32, 0.32))
    track = np.zeros((100, 4))
    with pytest.raises(ValueError, match="at most 16"):
        WeightEvaluator.from_tracks([track], tc, np.arange(-16, 1), 5)
    with pytest.raises(ValueError, match="beyond pred_time_offset"):
        WeightEvaluator.from_tracks([track], tc, [-3, 0, 7], 5)
    with pytest.raises(ValueError, match="after the first input offset"):
        WeightEvaluator.from_tracks([track], tc, [5], 5)
    with pytest.raises(ValueError, match="non-empty"):
        WeightEvaluator.from_tracks([track], tc, [], 5)
    with pytest.raises(ValueError, match=r"\[n_frames, 4\]"):
        WeightEvaluator.from_tracks([np.zeros((100, 3))], tc, [-3, 0], 5)
    with pytest.raises(ValueError, match="at least one log"):
        WeightEvaluator.from_tracks([], tc, [-3, 0], 5)
    ev = _bare_evaluator()
    assert list(_bare_evaluator(offsets=(2, -6, 0, -3)).input_time_offsets) == [-6, -3, 0, 2]  # sorted, as the reference does
    for deg in (8, -1, 1.5):
        with pytest.raises(ValueError, match="degree"):
            ev.eval_many(np.ones((2, 4)), deg=deg)
        with pytest.raises(ValueError, match="degree"):
            ev.optimize(deg=deg)
    with pytest.raises(ValueError, match="shape"):
        ev.eval_many(np.ones((2, 5)))
    with pytest.raises(ValueError, match="shape"):
        ev.eval_many(np.ones(4))
    with pytest.raises(ValueError, match="shape"):
        ev.eval(np.ones((1, 4)))
    for kw in (dict(lb=1.0, ub=1.0), dict(lb=0.0, ub=np.inf), dict(lb=2.0, ub=1.0), dict(pop_size=0), dict(max_epoch=0), dict(max_early_stop=0)):
        with pytest.raises(ValueError):
            ev.optimize(deg=2, **kw)
    with pytest.raises(ValueError, match="4 weights"):
        ev.to_config(2, [1, 2, 3])
    cfg = ev.to_config(2, [0.1, 0.2, 0.3, 0.4])
    assert (cfg.degree, cfg.sample_times, cfg.weights) == (2, [-6, -3, 0, 2], [0.1, 0.2, 0.3, 0.4])


def test_weight_evaluator_fails_loudly_without_gpu(hip_lib):
    """No CPU fallback: with no visible device the evaluator raises instead of computing (with one, it builds)."""
    from wtracker_amd.polyfit_opt import WeightEvaluator

    ec = ExperimentConfig("exp", 100, 60, (1600, 1400), 90, (900, 700))
    tc = TimingConfig(ec, 100, 40, 50, (4, 4), (0.32, 0.32))
    if hip.device_count() > 0:
        assert WeightEvaluator.from_tracks([np.zeros((100, 4))], tc, [-3, 0], 5).n_series >= 0
    else:
        with pytest.raises(hip.WtkError, match="GPU"):
            WeightEvaluator.from_tracks([np.zeros((100, 4))], tc, [-3, 0], 5)


def test_script_config_file_round_trip(tmp_path):
    """The JSON layout the script writes is the reference's PolyfitConfig.save_json layout: three keys, loadable with PolyfitConfig(**json.load(f))."""
    import importlib.util
    import json

    spec = importlib.util.spec_from_file_location("optimize_polyfit_weights", os.path.join(ROOT, "tools", "optimize_polyfit_weights.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from wtracker_amd.controllers import PolyfitConfig

    path = str(tmp_path / "polyfit_config.json")
    mod.save_config(PolyfitConfig(degree=2, sample_times=[0, -3, 2], weights=[0.5, 0.25, 1.0]), path)
    raw = json.load(open(path))
    assert list(raw) == ["degree", "sample_times", "weights"] and raw == {"degree": 2, "sample_times": [-3, 0, 2], "weights": [0.5, 0.25, 1.0]}
    cfg = mod.load_config(path)
    assert (cfg.degree, cfg.sample_times, cfg.weights) == (2, [-3, 0, 2], [0.5, 0.25, 1.0])
