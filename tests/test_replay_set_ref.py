"""CPU: the layout behind wtracker_amd.replay.ReplaySet (csrc/replay_set.hip) restated in numpy (harness/replay_set_ref.py) and held to
harness/replay_ref.py on every track alone: a set of tracks in one guarded super-track gives every (track, experiment) pair the moves, positions and summary
bits of the track alone, every cycle its own class mask, and a pooled mean within the reduction's bound of math.fsum over all rows.  Each mistake the
layout invites is planted once and must be caught by the same comparison.

The scenario: tests/golden/replay_hard.npz at 100 ms imaging (L = 5; 400 rows: a whole number of cycles, so its last rows touch its guard), its first 137
rows translated into a small frame (not a whole number of cycles, 27 logged cycles, the clamp binds on the far side), and replay_ref.long_track with
R = 4125 logged rows (two reduction chunks)."""
import dataclasses
import json
import math
import os

import numpy as np
import pytest

from harness import replay_ref as rr
from harness import replay_set_ref as rs
from wtracker_amd.sim import ExperimentConfig, TimingConfig

TIMES = [-8, -6, -4, -2, 0, 1]
REACH = 14  # the farthest sample time of range(-14, 2): a guard of 3 cycles of 5 frames


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def scenario(golden_dir, long=True):
    z = np.load(os.path.join(golden_dir, "replay_hard.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    ec = ExperimentConfig("hard", meta["num_frames"], meta["frames_per_sec"], tuple(meta["orig_resolution"]), meta["px_per_mm"], tuple(meta["init_position"]))
    tc = TimingConfig(ec, 100, 40, 50, meta["camera_size_mm"], meta["micro_size_mm"])
    g0 = rr.Geometry.of(tc, ec)
    short = z["track"][:137] + np.array([150.0, 250.0, 0.0, 0.0])
    g1 = dataclasses.replace(g0, num_frames=137, frame_wh=(400, 300), init=(500, 120))  # (the init position lies outside the frame: it is clamped)
    tracks, geoms = [z["track"].copy(), short], [g0, g1]
    if long:
        tracks.append(rr.long_track(4130, g0.L))
        geoms.append(dataclasses.replace(g0, num_frames=4130, frame_wh=(1400, 1400), init=(700, 600)))
    assert g0.L == 5 and [g.n_log for g in geoms[:2]] == [79, 27] and len(tracks[0]) % g0.L == 0 and np.isfinite(tracks[0][-4:]).all()
    return tracks, geoms


def polyfit_targets(track, g, n_cycles, weights, times):
    """a [C, E, 2], valid [C, E] of one degree-2 fit per weight vector."""
    parts = [rr.targets_polyfit(g, track, 2, times, w, n_cycles) for w in weights]
    return np.stack([p[0] for p in parts], axis=1), np.stack([p[1] for p in parts], axis=1)


def alone(kind, tracks, geoms, weights, times=TIMES):
    """replay_ref on every track alone -> per track (pos, move, summaries [E, 6], per-row errors [E])."""
    out = []
    for tr, g in zip(tracks, geoms):
        a = v = None
        E = 1
        if kind == rr.POLYFIT:
            (a, v), E = polyfit_targets(tr, g, g.n_cycles, weights, times), len(weights)
        elif kind == rr.OPTIMAL:
            a, v = (x[:, None] for x in rr.targets_optimal(g, tr))
        pos, move = rr.scan(kind, g, tr, a, None, v, E)
        rows = [rr.rows(g, tr, pos, move, e) for e in range(E)]
        out.append((pos, move, np.stack([r["summary"] for r in rows]), [r["bbox_error"] for r in rows]))
    return out


def as_set(kind, tracks, geoms, weights, defect=None, reach=REACH, times=TIMES):
    """The same through the super-track: targets of ALL its cycles in one call each, the set's scan and rows."""
    st = rs.super_track(tracks, geoms, reach, defect)
    a = v = None
    E = 1
    if kind == rr.POLYFIT:
        (a, v), E = polyfit_targets(st.track, geoms[0], st.n_cycles, weights, times), len(weights)
    elif kind == rr.OPTIMAL:
        a, v = (x[:, None] for x in rr.targets_optimal(geoms[0], st.track, st.n_cycles))
    pos, move = rs.set_scan(kind, st, tracks, geoms, a, None, v, E, defect)
    ts, pooled, errs = rs.set_rows(st, tracks, geoms, pos, move, E, defect)
    return st, pos, move, ts, pooled, errs


def differences(st, geoms, pos, move, ts, want) -> list:
    """The (track, what) pairs in which the set differs from the tracks alone."""
    out = []
    for t, (g, (wpos, wmove, wsum, _)) in enumerate(zip(geoms, want)):
        sl = slice(st.cyc_off[t], st.cyc_off[t] + g.n_cycles)
        out += [(t, what) for what, same in (("pos", np.array_equal(pos[sl], wpos)), ("move", np.array_equal(move[sl], wmove)),
                                             ("summary", np.array_equal(bits(ts[t]), bits(wsum)))) if not same]
    return out


WEIGHTS = [[1, 1, 2, 3, 4, 5], [0.3, 1, 0.2, 1, 0.7, 1]]


@pytest.fixture(scope="module")
def full(golden_dir):
    tracks, geoms = scenario(golden_dir)
    return tracks, geoms, alone(rr.POLYFIT, tracks, geoms, WEIGHTS), as_set(rr.POLYFIT, tracks, geoms, WEIGHTS)


def test_every_pair_has_the_bits_of_its_track_alone(full):
    tracks, geoms, want, (st, pos, move, ts, pooled, _) = full
    assert st.guard_cycles == 3 and st.cyc_off == [0, 83, 114] and st.n_cycles == 114 + 826 + 3
    assert differences(st, geoms, pos, move, ts, want) == []
    # the clamp binds on the far side in track 1 only; track 2 crosses a reduction chunk
    assert pos[st.cyc_off[1]:st.cyc_off[1] + geoms[1].n_cycles, :, 0].max() == 399 and pos[st.cyc_off[0]:st.cyc_off[0] + 80, :, 0].max() > 399
    assert ts[2, 0, 1] == 4125 and [int(v) for v in ts[:, 0, 3]] == [77 * 3, 25 * 3, 823 * 3]  # every track drops its own first and last logged cycle
    # pooling: sequential float64 adds in track order from 0.0
    seq = np.zeros_like(pooled)
    for t in range(3):
        seq = seq + want[t][2]
    assert np.array_equal(bits(pooled), bits(seq))


@pytest.mark.parametrize("kind", [rr.CSV, rr.OPTIMAL])
def test_csv_and_optimal_pairs_have_the_bits_of_their_track_alone(golden_dir, kind):
    """CSV tests "inside the track" with the track's own row count; the median of the next imaging phase reads past a track's last cycle."""
    tracks, geoms = scenario(golden_dir, long=False)
    st, pos, move, ts, _, _ = as_set(kind, tracks, geoms, None, reach=1)  # one guard cycle is all these two kinds need
    assert st.guard_cycles == 1
    assert differences(st, geoms, pos, move, ts, alone(kind, tracks, geoms, None)) == []


def test_every_cycle_of_the_super_track_has_its_own_class_mask(golden_dir):
    """Sample times range(-14, 2): the first cycles of tracks t > 0 look back into the guard, the last cycles forward into the NaN fill."""
    tracks, geoms = scenario(golden_dir)
    times = list(range(-14, 2))
    st = rs.super_track(tracks, geoms, REACH)
    masks = rs.cycle_masks(st.track, st.L, st.n_cycles, times)
    covered = np.zeros(st.n_cycles, dtype=bool)
    for t, (tr, g) in enumerate(zip(tracks, geoms)):
        sl = slice(st.cyc_off[t], st.cyc_off[t] + g.n_cycles)
        own = rs.cycle_masks(tr, g.L, g.n_cycles, times)
        assert np.array_equal(masks[sl], own), t
        assert own[0] == 0b11 << 14  # the first cycle keeps the samples at 0 and 1 alone, also behind another track
        covered[sl] = True
    assert not covered[-st.guard_cycles:].any() and (masks[-st.guard_cycles:] >> 14 == 0).all()  # a guard cycle holds no row of its own (times 0, 1)
    short = rs.super_track(tracks, geoms, REACH, "short_guard")
    m1 = rs.cycle_masks(short.track, short.L, short.n_cycles, times)[short.cyc_off[1]]
    assert m1 != rs.cycle_masks(tracks[1], st.L, 1, times)[0]  # one guard cycle fewer: track 1's first cycle sees track 0's last rows


def test_pooled_mean_lies_within_the_reduction_bound_of_fsum(full):
    tracks, geoms, _, (st, _, _, ts, pooled, errs) = full
    T = len(tracks)
    for e in range(len(WEIGHTS)):
        exact, bound = rs.pooled_sum_bound([errs[t][e] for t in range(T)], T)
        n = sum(len(errs[t][e]) for t in range(T))
        assert pooled[e, 1] == n == 395 + 135 + 4125 and exact > 1.0
        print(f"\n[replay_set_ref] experiment {e}: pooled sum {pooled[e, 0]!r}, fsum {exact!r}, |difference| {abs(pooled[e, 0] - exact):.3e}, bound {bound:.3e}")
        assert abs(pooled[e, 0] - exact) <= bound
        mean = pooled[e, 0] / pooled[e, 1]
        assert abs(mean - exact / n) <= bound / n + 2.0 ** -53 * (exact / n)  # (and the one division's rounding)
        assert mean != ts[0, e, 0] / ts[0, e, 1]  # the pooled mean is not the first track's


@pytest.mark.parametrize("defect", rs.DEFECTS)
def test_planted_defects_are_caught(golden_dir, defect):
    """The two short tracks; the comparison of test_every_pair_has_the_bits_of_its_track_alone must name track 1 (and leave track 0 alone, except for the
    trimming, which the set's first track also gets wrong at its last cycle)."""
    tracks, geoms = scenario(golden_dir, long=False)
    # (the short guard shows only where the fit looks far enough back to see into the track before)
    weights, times = ([np.ones(16)], list(range(-14, 2))) if defect == "short_guard" else (WEIGHTS[:1], TIMES)
    want = alone(rr.POLYFIT, tracks, geoms, weights, times)
    st, pos, move, ts, _, _ = as_set(rr.POLYFIT, tracks, geoms, weights, defect, times=times)
    clean = as_set(rr.POLYFIT, tracks, geoms, weights, times=times)
    assert differences(clean[0], geoms, clean[1], clean[2], clean[3], want) == []
    found = differences(st, geoms, pos, move, ts, want)
    assert any(t == 1 for t, _ in found), (defect, found)
    if defect == "trim_set":
        assert found == [(0, "summary"), (1, "summary")]
    else:
        assert all(t == 1 for t, _ in found), (defect, found)
