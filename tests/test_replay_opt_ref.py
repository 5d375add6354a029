"""The class grouping behind wtk_replay_polyfit_targets, on the CPU (tests/harness/replay_opt_ref.py): the cycles of tests/golden/replay_hard.npz
grouped by the set of samples that exist and fitted ONCE per class give the targets of one numpy fit per cycle (replay_ref.targets_polyfit, which
tests/test_replay_ref.py pins to the real reference); the product's vectorised class table is the harness's; the new entry points are declared, bound
and built.  The GPU tests (tests/test_gpu_replay_opt.py) hold the kernels to wtk_track_polyfit bit for bit."""
import json
import os
import warnings

import numpy as np
import pytest

from harness import replay_opt_ref as ro
from harness import replay_ref as rr
from wtracker_amd.sim import ExperimentConfig, TimingConfig

EPS = float(np.finfo(np.float64).eps)


def hard(golden_dir, imaging):
    z = np.load(os.path.join(golden_dir, "replay_hard.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    ec = ExperimentConfig("hard", meta["num_frames"], meta["frames_per_sec"], tuple(meta["orig_resolution"]), meta["px_per_mm"], tuple(meta["init_position"]))
    tc = TimingConfig(ec, imaging, 40, 50, meta["camera_size_mm"], meta["micro_size_mm"])
    return z["track"], meta, rr.Geometry.of(tc, ec)


@pytest.mark.parametrize("imaging", [100, 200])
def test_class_table_covers_every_cycle_and_names_its_samples(golden_dir, imaging):
    from wtracker_amd.replay import polyfit_classes

    track, meta, g = hard(golden_dir, imaging)
    cen = rr._centers(track)
    for kw in meta["polyfit_configs"]:
        st = sorted(kw["sample_times"])
        cycle_class, class_mask = ro.class_table(track, g.L, g.n_cycles, st)
        assert cycle_class.shape == (g.n_cycles,) and cycle_class.min() == 0 and cycle_class.max() == len(class_mask) - 1  # every cycle has a class
        assert sorted(set(cycle_class.tolist())) == list(range(len(class_mask))) and (np.diff(class_mask) > 0).all()   # every class has a cycle
        for c in range(g.n_cycles):
            for j, t in enumerate(st):
                f = c * g.L + t
                assert bool((class_mask[cycle_class[c]] >> j) & 1) == bool(0 <= f < len(track) and np.isfinite(cen[f]).all()), (c, j)
        # the first cycles lack their history and the NaN rows cost single samples: several classes, far fewer than cycles
        assert 3 <= len(class_mask) < g.n_cycles // 2
        mine = polyfit_classes(track, g.L, g.n_cycles, st)
        assert mine[0].dtype == np.int32 and np.array_equal(mine[0], cycle_class) and np.array_equal(mine[1], class_mask)


@pytest.mark.parametrize("imaging", [100, 200])
def test_one_fit_per_class_gives_the_targets_of_one_fit_per_cycle(golden_dir, imaging):
    """Both sides are numpy's polyfit (LAPACK gelsd: x = V S^+ U^T b with the same cut): the same linear functional of the centres, rounded differently
    (one right-hand side against all of a class's).  A backward-stable solve is off by at most ~ (entries of the matrix) eps kappa per unit of
    |g|_1 max|y|, g the functional (fit, then evaluate at t_eval) and kappa the effective condition number of the scaled matrix; two solves, <= 16 x 8
    entries: bound = 256 eps kappa |g|_1 max|centre|.  The valid flags are equal."""
    from numpy.polynomial import polynomial as poly

    track, meta, g = hard(golden_dir, imaging)
    cen = rr._centers(track)
    top = float(np.nanmax(np.abs(cen)))
    worst = 0.0
    for kw in meta["polyfit_configs"]:
        st = np.array(sorted(kw["sample_times"]))
        wt = np.ones(len(st)) if kw.get("weights") is None else np.asarray(kw["weights"], dtype=float)
        a, v = rr.targets_polyfit(g, track, **kw)
        ga, gv = ro.targets_polyfit_grouped(g, track, **kw)
        assert np.array_equal(v, gv) and v.sum() > 0
        cycle_class, class_mask = ro.class_table(track, g.L, g.n_cycles, st)
        bound = np.zeros(len(class_mask))
        for k, mask in enumerate(class_mask):
            ok = np.array([(mask >> j) & 1 for j in range(len(st))], dtype=bool)
            if ok.any():
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    row = poly.polyval(g.L + g.I // 2, poly.polyfit(st[ok], np.eye(int(ok.sum())), deg=kw["degree"], w=wt[ok]))
                bound[k] = 256 * EPS * ro.condition(mask, kw["degree"], st, wt) * np.abs(row).sum() * top
        diff = np.abs(a - ga).max(axis=1)
        worst = max(worst, float((diff / np.maximum(bound[cycle_class], 1e-300)).max()))
        assert (diff <= bound[cycle_class]).all(), (kw, int(np.argmax(diff - bound[cycle_class])))
        assert bound.max() < 1e-4  # the bound itself stays four orders below the half pixel that decides a move
    print(f"imaging {imaging}: worst deviation / bound = {worst:.3g}")


def test_the_entry_points_are_declared_bound_and_built():
    from wtracker_amd import _build, hip

    for name in ("wtk_replay_polyfit_targets", "wtk_replay_polyfit_targets_scratch_doubles", "wtk_replay_objective"):
        assert name in hip.SYMBOLS
    assert "replay.hip" in _build.SOURCES and "replay_targets.hip" in _build.SOURCES and "polyfit_solve.h" in _build.HEADERS
    assert sorted(hip.REPLAY_OBJECTIVES.values()) == [0, 1, 2, 3]


def test_scratch_sizing(hip_lib):
    """n_classes records of n_times K + K K + 2 K + n_times + 1 doubles per particle; bad sizes give -1."""
    from wtracker_amd import hip

    assert hip.replay_polyfit_targets_scratch_doubles(5, 70, 6, 2) == 5 * 70 * (6 * 3 + 9 + 6 + 6 + 1)
    assert hip.replay_polyfit_targets_scratch_doubles(79, 65535, 16, 7) == 79 * 65535 * (16 * 8 + 64 + 16 + 16 + 1)  # beyond 2^31: int64
    for bad in ((-1, 1, 6, 2), (1, -1, 6, 2), (1, 1, 0, 2), (1, 1, 17, 2), (1, 1, 6, -1), (1, 1, 6, 8)):
        assert hip.replay_polyfit_targets_scratch_doubles(*bad) == -1, bad
