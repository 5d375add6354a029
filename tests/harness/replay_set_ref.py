"""TEST INFRASTRUCTURE: float64 numpy restatement of the replay of a population on a SET of tracks (wtracker_amd/csrc/replay_set.hip, DESIGN.md section
26), built on harness.replay_ref: the guarded super-track, the global cycle list, the Polyfit class table over it, the set's scan and rows reduction as
replay_ref's on each track's slice, and the pooling of the tracks' summaries by sequential adds.

`defect` plants one of the mistakes the layout invites (tests/test_replay_set_ref.py shows that each is caught):
  "no_reset"      the position is not reset at a track's start (track t > 0 starts where track t - 1 stood at its last cycle)
  "trim_set"      only the set's first and last logged cycle are trimmed, not every track's
  "short_guard"   the guard is one cycle shorter than the reach asks for
  "clamp_track0"  every track's position is clamped to track 0's frame"""
from __future__ import annotations

import dataclasses
import math

import numpy as np

from harness import replay_ref as rr

DEFECTS = ("no_reset", "trim_set", "short_guard", "clamp_track0")


@dataclasses.dataclass
class SuperTrack:
    track: np.ndarray   # [n_super_cycles L, 4], NaN outside the tracks
    cyc_off: list       # first cycle of every track
    guard_cycles: int
    L: int

    @property
    def n_cycles(self) -> int:
        return len(self.track) // self.L

    def rows_of(self, t: int, n_track: int) -> np.ndarray:
        return self.track[self.cyc_off[t] * self.L: self.cyc_off[t] * self.L + n_track]


def super_track(tracks, geoms, reach: int, defect=None) -> SuperTrack:
    """Track t from cycle cyc_off[t]: its rows, NaN rows up to the end of its slot of max(n_cycles, ceil(n_track / L)) cycles, ceil(reach / L) guard cycles."""
    L = geoms[0].L
    assert all(g.L == L for g in geoms)
    guard = -(-reach // L) - (1 if defect == "short_guard" else 0)
    offs, off = [], 0
    for tr, g in zip(tracks, geoms):
        offs.append(off)
        off += max(g.n_cycles, -(-len(tr) // L)) + guard
    out = np.full((off * L, 4), np.nan)
    for tr, o in zip(tracks, offs):
        out[o * L: o * L + len(tr)] = tr
    return SuperTrack(out, offs, guard, L)


def cycle_masks(track: np.ndarray, L: int, n_cycles: int, sample_times) -> np.ndarray:
    """The class mask of every cycle (wtracker_amd.replay.polyfit_classes, the table the device call is given)."""
    from wtracker_amd.replay import polyfit_classes

    cycle_class, class_mask = polyfit_classes(track, L, n_cycles, sorted(sample_times))
    return class_mask[cycle_class]


def slice_of(st: SuperTrack, g: rr.Geometry, t: int, x):
    return None if x is None else x[st.cyc_off[t]: st.cyc_off[t] + g.n_cycles]


def set_scan(kind: int, st: SuperTrack, tracks, geoms, a=None, b=None, valid=None, E: int = 1, defect=None):
    """-> (pos, move) [n_super_cycles, E, 2] int32; cycles of no track hold -1.  a, b, valid are indexed by the super-track's cycle."""
    pos = np.full((st.n_cycles, E, 2), -1, dtype=np.int32)
    move = np.full((st.n_cycles, E, 2), -1, dtype=np.int32)
    for t, (tr, g) in enumerate(zip(tracks, geoms)):
        if defect == "clamp_track0":
            g = dataclasses.replace(g, frame_wh=geoms[0].frame_wh)
        sl = slice(st.cyc_off[t], st.cyc_off[t] + g.n_cycles)
        rows = st.rows_of(t, len(tr))  # (CSV: the "inside the track" test uses the track's own row count)
        if defect == "no_reset" and t > 0:
            last = st.cyc_off[t - 1] + geoms[t - 1].n_cycles - 1
            for e in range(E):  # (replay_ref.scan starts all experiments at one position)
                ge = dataclasses.replace(g, init=tuple(int(v) for v in pos[last, e]))
                p, m = rr.scan(kind, ge, rows, slice_of(st, g, t, a)[:, e:e + 1] if a is not None else None,
                               slice_of(st, g, t, b)[:, e:e + 1] if b is not None else None, slice_of(st, g, t, valid)[:, e:e + 1] if valid is not None else None, 1)
                pos[sl, e:e + 1], move[sl, e:e + 1] = p, m
            continue
        pos[sl], move[sl] = rr.scan(kind, g, rows, slice_of(st, g, t, a), slice_of(st, g, t, b), slice_of(st, g, t, valid), E)
    return pos, move


def set_rows(st: SuperTrack, tracks, geoms, pos, move, E: int, defect=None):
    """-> (track_summary [T, E, 6], summary [E, 6], per-row bbox errors [T][E] arrays): every track's rows reduced in the kernel's order by
    replay_ref.rows, the tracks' summaries added in track order from 0.0."""
    T = len(tracks)
    ts = np.zeros((T, E, 6))
    errs = [[None] * E for _ in range(T)]
    logged = [t for t in range(T) if geoms[t].n_log > 0]
    for t, (tr, g) in enumerate(zip(tracks, geoms)):
        if defect == "clamp_track0":
            g = dataclasses.replace(g, frame_wh=geoms[0].frame_wh)
        sl = slice(st.cyc_off[t], st.cyc_off[t] + g.n_cycles)
        for e in range(E):
            res = rr.rows(g, st.rows_of(t, len(tr)), pos[sl], move[sl], e)
            ts[t, e], errs[t][e] = res["summary"], res["bbox_error"]
            if defect == "trim_set":
                out, err = res["rows"], res["bbox_error"]
                keep = out[:, 15] == 0
                if t == logged[0]:
                    keep &= out[:, 14] != 0
                if t == logged[-1]:
                    keep &= out[:, 14] != g.n_log - 1
                ts[t, e, 2], ts[t, e, 3] = rr._tree_sum(np.where(keep, err, 0.0)), float(keep.sum())
    pooled = np.zeros((E, 6))
    for t in range(T):
        pooled = pooled + ts[t]
    return ts, pooled, errs


def pooled_sum_bound(errs_of_e, T: int) -> tuple:
    """(math.fsum of the concatenated per-row errors, the bound on the pooled sum's distance from it): ceil(log2 of the row count) roundings of the
    tree plus T - 1 additions of the pooling, each at most 2^-53 of the sum of the absolute values."""
    x = np.concatenate(errs_of_e)
    return math.fsum(x), (math.ceil(math.log2(len(x))) + T - 1) * 2.0 ** -53 * math.fsum(np.abs(x))
