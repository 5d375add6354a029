"""The numpy restatement of the precise error on a SET of tracks (tests/harness/replay_set_precise_ref.py) against the per-track
harness on each track alone (replay_precise_ref.precise / summaries, pinned to the real reference by tests/test_replay_precise_ref.py): global row ->
track, the per-track view, frames, shape and threshold, the chunk order through chunk0, the finish.  Five planted defects are each caught.  And the C ABI's
additions: names, the scratch formula, and the refusals, which are made before any device call and so answer without a GPU."""
import ctypes
import math

import numpy as np
import pytest

from harness import replay_set_precise_ref as sp

E = 70
T = 4


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


@pytest.fixture(scope="module")
def full():
    """The scene, its scan, the set form and every track alone: computed once, never modified."""
    sn = sp.scene(E)
    pos, move = sp.scan_of(sn)
    err, counts = sp.set_precise(sn, pos, move)
    ts, pooled = sp.set_summaries(sn, err)
    alone = [sp.track_alone(sn, t, pos, move) for t in range(T)]
    return dict(sn=sn, pos=pos, move=move, err=err, counts=counts, ts=ts, pooled=pooled, alone=alone)


def test_the_scene_reaches_every_path(full):
    sn, alone = full["sn"], full["alone"]
    assert [sc["frame_shape"] for sc in sn["tracks"]] == [(96, 131), (48, 64), (256, 256), (48, 64)]
    assert sn["R"] == [120, 24, 18, 4104] and [g.n_log for g in sn["geoms"]] == [20, 4, 3, 684]
    assert list(sn["row0"]) == [0, 120, 144, 162, 4266] and list(sn["chunk0"]) == [0, 1, 2, 3, 5]  # two chunks inside track 3
    assert alone[0]["stats"]["table"] > 0 and alone[0]["stats"]["frame_walk"] == 0  # answered by the table
    assert alone[2]["stats"]["frame_walk"] > 0 and alone[2]["stats"]["table"] == 0  # 213 x 213 cells: every pair walks
    nan_rows = np.isnan(sn["tracks"][3]["track"][:4104]).any(axis=1).mean()
    assert 0.02 < nan_rows < 0.04
    st = sn["st"]
    inside = np.zeros(st.n_cycles, dtype=bool)
    for g, off in zip(sn["geoms"], st.cyc_off):
        inside[off:off + g.n_cycles] = True
    assert (sn["valid"][~inside] == 0).all() and (~inside).sum() > 0  # cycles of no track are invalid
    # the ulp rows do what they are there for: the experiments that stay and move get different counts on the same frame
    c1 = full["alone"][1]["counts"]
    assert (c1[0, :, 0] != c1[2, :, 0]).any()


def test_every_pair_has_the_bits_of_its_track_alone(full):
    sn, row0 = full["sn"], full["sn"]["row0"]
    for t in range(T):
        sl = slice(int(row0[t]), int(row0[t + 1]))
        want = full["alone"][t]
        assert np.array_equal(full["counts"][:, sl], want["counts"]), (t, np.argwhere(full["counts"][:, sl] != want["counts"])[:5])
        assert np.array_equal(bits(full["err"][:, sl]), bits(want["err"])), t
        assert np.array_equal(bits(full["ts"][t]), bits(want["summary"])), (t, full["ts"][t][:2], want["summary"][:2])
    for kind in sp.OBJECTIVE_SLOTS:
        num, den = sp.OBJECTIVE_SLOTS[kind]
        each = sp.objective(full["ts"], full["pooled"], kind, per_track=True)
        for t in range(T):
            with np.errstate(invalid="ignore"):
                assert np.array_equal(bits(each[t]), bits(full["alone"][t]["summary"][:, num] / full["alone"][t]["summary"][:, den]))


def test_the_pooled_slots_are_the_track_sums_in_track_order(full):
    pooled = np.zeros((E, 6))
    for t in range(T):
        pooled = pooled + full["alone"][t]["summary"]
    assert np.array_equal(bits(full["pooled"]), bits(pooled))
    assert (full["pooled"][:, 1] + full["pooled"][:, 5] == sum(full["sn"]["R"])).all()  # rows with a value + NaN rows = all rows


def test_pooled_sum_lies_within_the_reduction_bound_of_fsum(full, capsys):
    """The two summation orders (a tree per chunk, chunks in order, tracks in order) against math.fsum over all rows: at most ceil(log2(sum R)) + T - 1
    roundings, each at most 2^-53 of the sum of the absolute values (DESIGN.md section 26's bound)."""
    rows = sum(full["sn"]["R"])
    worst = 0.0
    for e in range(E):
        x = full["err"][e][~np.isnan(full["err"][e])]
        exact, bound = math.fsum(x), (math.ceil(math.log2(rows)) + T - 1) * 2.0 ** -53 * math.fsum(np.abs(x))
        assert abs(full["pooled"][e, 0] - exact) <= bound, (e, full["pooled"][e, 0], exact, bound)
        worst = max(worst, abs(full["pooled"][e, 0] - exact) / bound if bound else 0.0)
    with capsys.disabled():
        print(f"\n[set precise] worst |pooled - fsum| / bound over {E} experiments: {worst:.3f}")


@pytest.mark.parametrize("defect", sp.DEFECTS)
def test_planted_defects_are_caught(full, defect):
    sn = full["sn"]
    if defect in ("frames_track0", "hw_track0", "global_row"):
        err, counts = sp.set_precise(sn, full["pos"], full["move"], defect=defect)
        assert np.array_equal(counts[:, :120], full["counts"][:, :120])  # track 0 is its own track 0
        assert not np.array_equal(counts, full["counts"])
        assert not np.array_equal(bits(sp.set_summaries(sn, err)[1]), bits(full["pooled"]))
    elif defect == "trim_set":
        ts, pooled = sp.set_summaries(sn, full["err"], defect=defect)
        assert not np.array_equal(bits(ts[:, :, 2:4]), bits(full["ts"][:, :, 2:4])) and (pooled[:, 3] > full["pooled"][:, 3]).all()
        assert np.array_equal(bits(pooled[:, [0, 1, 4, 5]]), bits(full["pooled"][:, [0, 1, 4, 5]]))
    else:
        good = sp.objective(full["ts"], full["pooled"], "trimmed_precise_error")
        bad = sp.objective(full["ts"], full["pooled"], "trimmed_precise_error", defect=defect)
        assert np.isfinite(good).all() and not np.array_equal(bits(good), bits(bad))


# ------------------------------------------------------------------------------------------------- the C ABI
def small_tables(hip):
    """Two tracks of the scene's timing as tables with HOST stand-ins for the device copies: nothing here is ever launched."""
    rows = [dict(cyc_off=0, n_track=121, num_frames=121, n_cycles=20, n_log=20, frame_wh=(131, 96), init_position=(30, 30)),
            dict(cyc_off=33, n_track=25, num_frames=25, n_cycles=4, n_log=4, frame_wh=(64, 48), init_position=(11, 8))]
    table = hip.ReplaySetTable(rows, 6, 11, (33 + 5 + 11) * 6)
    table.dev = np.frombuffer(bytes(table.host), dtype=np.uint8).copy()
    return table


def frames_of(hip, table, **change):
    fake = np.zeros(16, dtype=np.uint8)  # stands for device memory: the checks look at the pointers' values only
    entries = [dict(frames=fake.ctypes.data, bg=fake.ctypes.data, n_frames=121, H=96, W=131, diff_thresh=20.0),
               dict(frames=fake.ctypes.data, bg=fake.ctypes.data, n_frames=25, H=48, W=64, diff_thresh=20.0)]
    entries[1].update({k: v for k, v in change.items() if k != "row0"})
    fr = hip.ReplaySetFrames(table, entries)
    if "row0" in change:
        fr.host[1].row0 = change["row0"]
    fr.dev = np.frombuffer(bytes(fr.host), dtype=np.uint8).copy()
    fr._keep = fake
    return fr


def test_the_abi_additions(hip_lib):
    from wtracker_amd import _build, hip

    names = ["wtk_replay_set_precise_scratch_doubles", "wtk_replay_set_precise", "wtk_replay_set_precise_objective"]
    at = hip.SYMBOLS.index("wtk_replay_set_objective")
    assert hip.SYMBOLS[at + 1:at + 4] == names and all(hasattr(hip_lib, n) for n in names)  # the replay-set section, in the header's order
    assert hip.SYMBOLS[-3:] == ["wtk_replay_precise_scratch_doubles", "wtk_replay_precise", "wtk_replay_precise_objective"]
    assert hip_lib.wtk_abi_version() == 7 and "replay_precise_device.h" in _build.HEADERS
    assert ctypes.sizeof(hip._ReplaySetFrames) == 48
    table = small_tables(hip)
    # R = 120 and 24: 144 rows, 2 chunks; E = 3: 3 x 144 pair errors + 3 x 2 x 6 partials + 72 doubles of int32 flags
    assert hip.replay_set_precise_scratch_doubles(table, 3) == 3 * 144 + 3 * 2 * 6 + 72
    assert hip_lib.wtk_replay_set_precise_scratch_doubles(table.host, 0, 6, 3) == -1 and hip_lib.wtk_replay_set_precise_scratch_doubles(None, 2, 6, 3) == -1
    table.host[1].n_log = -1
    assert hip_lib.wtk_replay_set_precise_scratch_doubles(table.host, 2, 6, 3) == -1


def test_the_refusals_answer_without_a_device(hip_lib):
    from wtracker_amd import hip

    cfg = hip.replay_config(121, 4, 2, 1, (40, 32), (14, 10), (131, 96), (30, 30))
    table, E3 = small_tables(hip), 3
    n_scratch = hip.replay_set_precise_scratch_doubles(table, E3)
    C = table.n_super // 6
    track, share = np.zeros((table.n_super, 4)), np.zeros(2)
    pos, move = np.zeros((C, E3, 2), dtype=np.int32), np.zeros((C, E3, 2), dtype=np.int32)
    a, valid = np.zeros((C, E3, 2)), np.zeros((C, E3), dtype=np.int32)
    out = dict(err=np.full((E3, 144), -7.0), counts=np.full((E3, 144, 2), -7, dtype=np.int32), ts=np.full((2, E3, 6), -7.0), s=np.full((E3, 6), -7.0),
               scratch=np.full(n_scratch, -7.0), obj=np.full(E3, -7.0), tobj=np.full((2, E3), -7.0))

    def precise(tb=table, fr=None, crop=0, n=n_scratch, E=E3):
        hip.replay_set_precise(cfg, tb, fr if fr is not None else frames_of(hip, tb), E, track, share, pos, move, crop, out["err"], out["counts"], out["ts"],
                               out["s"], out["scratch"], n)

    def objective(tb=table, fr=None, obj=0, kind=hip.REPLAY_OPTIMAL, crop=0):
        hip.replay_set_precise_objective(cfg, tb, fr if fr is not None else frames_of(hip, tb), kind, E3, track, a, None, valid, share, pos, move, crop,
                                         out["ts"], out["s"], out["scratch"], n_scratch, obj, out["obj"], out["tobj"])

    for call in (precise, objective):
        with pytest.raises(hip.WtkError, match=r"track 1: the frames' \(H, W\) differ"):
            call(fr=frames_of(hip, table, H=64, W=48))
        with pytest.raises(hip.WtkError, match="track 1: fewer frames than logged rows"):
            call(fr=frames_of(hip, table, n_frames=23))
        with pytest.raises(hip.WtkError, match="track 1: row0 must be the sum of R"):
            call(fr=frames_of(hip, table, row0=121))
        with pytest.raises(hip.WtkError, match="track 1: null frames or background"):
            call(fr=frames_of(hip, table, bg=0))
        with pytest.raises(hip.WtkError, match="track 1: null frames or background"):
            call(fr=frames_of(hip, table, frames=0))
        for bad in (float("nan"), float("inf")):
            with pytest.raises(hip.WtkError, match="track 1: diff_thresh must be finite"):
                call(fr=frames_of(hip, table, diff_thresh=bad))
        with pytest.raises(hip.WtkError, match="negative max_crop_px"):
            call(crop=-1)
        # everything set_view refuses: a slot that overlaps the one before, named by its track
        over = small_tables(hip)
        over.host[1].cyc_off = 30
        with pytest.raises(hip.WtkError, match="track 1: its slot overlaps"):
            call(tb=over)
        no_dev = small_tables(hip)
        fr = frames_of(hip, no_dev)
        fr.dev = None
        with pytest.raises(hip.WtkError, match="null argument"):
            call(tb=no_dev, fr=fr)
    with pytest.raises(hip.WtkError, match="scratch smaller than wtk_replay_set_precise_scratch_doubles"):
        precise(n=n_scratch - 1)
    with pytest.raises(hip.WtkError, match="at least one experiment"):
        precise(E=0)
    with pytest.raises(hip.WtkError, match="unknown objective"):
        objective(obj=3)
    with pytest.raises(hip.WtkError, match="null targets"):
        hip.replay_set_precise_objective(cfg, table, frames_of(hip, table), hip.REPLAY_OPTIMAL, E3, track, None, None, None, share, pos, move, 0, out["ts"],
                                         out["s"], out["scratch"], n_scratch, 0, out["obj"])
    # a frame of more than 2^30 pixels (the track's own frame is that large, so the shapes agree)
    big = small_tables(hip)
    big.host[1].x_max, big.host[1].y_max = 2 ** 16 - 1, 2 ** 15
    big.dev = np.frombuffer(bytes(big.host), dtype=np.uint8).copy()
    with pytest.raises(hip.WtkError, match=r"track 1: frames must be H x W gray with H \* W <= 2\^30"):
        precise(tb=big, fr=frames_of(hip, big, H=2 ** 15 + 1, W=2 ** 16))
    # the trimmed objective where a track logs fewer than 3 cycles; the plain ones pass this check (and nothing else is left to refuse: not called)
    rows = [dict(cyc_off=0, n_track=121, num_frames=121, n_cycles=20, n_log=20, frame_wh=(131, 96), init_position=(30, 30)),
            dict(cyc_off=33, n_track=13, num_frames=13, n_cycles=2, n_log=2, frame_wh=(64, 48), init_position=(11, 8))]
    two = hip.ReplaySetTable(rows, 6, 11, table.n_super)
    two.dev = np.frombuffer(bytes(two.host), dtype=np.uint8).copy()
    with pytest.raises(hip.WtkError, match="at least 3 logged cycles of every track"):
        objective(tb=two, fr=frames_of(hip, two, n_frames=13))
    # too many blocks for one launch: S E >= 2^31 with S = 393216 chunks and E = 6000 (the table alone is checked: no row is ever read).  n_super is
    # an int32, so the rows of all tracks stay below 2^31 by the track table's own checks.
    L, n_log = 6, 2 ** 28
    huge_rows = [dict(cyc_off=0, n_track=n_log * L, num_frames=n_log * L + 1, n_cycles=n_log, n_log=n_log, frame_wh=(131, 96), init_position=(30, 30))]
    huge = hip.ReplaySetTable(huge_rows, L, 0, n_log * L)
    assert huge.n_chunks == 393216
    huge.dev = np.frombuffer(bytes(huge.host), dtype=np.uint8).copy()
    fake = np.zeros(16, dtype=np.uint8)
    hfr = hip.ReplaySetFrames(huge, [dict(frames=fake.ctypes.data, bg=fake.ctypes.data, n_frames=2 ** 31 - 1, H=96, W=131, diff_thresh=20.0)])
    hfr.dev = fake
    with pytest.raises(hip.WtkError, match="too many"):
        hip.replay_set_precise(cfg, huge, hfr, 6000, track, share, pos, move, 0, None, None, out["ts"], out["s"], out["scratch"], n_scratch)
    for k, v in out.items():  # refused before anything ran: no output was touched
        assert (v == -7).all(), k
