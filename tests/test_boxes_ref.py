"""CPU checks of the background-subtraction box: the numpy restatement (tests/harness/box_ref.py) on hand-derivable masks and against scipy.ndimage, the
morphology borders, and the C entry points' and BoxCalculator's argument checks (no GPU: every call below fails its checks before any launch)."""
import ctypes

import numpy as np
import pytest

from harness import box_ref as br
from wtracker_amd import evaluation as ev
from wtracker_amd import hip


def _mask(rows):
    return np.array([[ch == "#" for ch in r] for r in rows])


HAND = {
    # name: (mask, A2, box)
    "single pixel": (_mask([".....", "..#..", "....."]), 0, (2, 1, 1, 1)),
    "square 1": (_mask(["#"]), 0, (0, 0, 1, 1)),
    "square 2": (_mask(["....", ".##.", ".##."]), 2, (1, 1, 2, 2)),
    "square 4": (_mask(["......", ".####.", ".####.", ".####.", ".####.", "......"]), 18, (1, 1, 4, 4)),
    "L of three": (_mask(["....", ".#..", ".##.", "...."]), 1, (1, 1, 2, 2)),
    # 5 x 5 outline of a 3 x 3 hole: the polygon through the outline's centres is 4 x 4, whatever is inside (16 pixels would give less)
    "ring": (_mask([".......", ".#####.", ".#...#.", ".#...#.", ".#...#.", ".#####.", "......."]), 32, (1, 1, 5, 5)),
    "horizontal line": (_mask(["......", ".####.", "......"]), 0, (1, 1, 4, 1)),
    "diagonal line": (_mask(["#...", ".#..", "..#.", "...#"]), 0, (0, 0, 4, 4)),
    "vertical line at the border": (_mask(["...#", "...#", "...#"]), 0, (3, 0, 1, 3)),
    "empty": (_mask(["....", "....", "...."]), 0, (0, 0, 0, 0)),
}


@pytest.mark.parametrize("name", list(HAND))
def test_hand_derived_masks(name):
    m, a2, box = HAND[name]
    got_box, got_a2, second = br.box_of_mask(m)
    assert (got_a2, tuple(got_box)) == (a2, box)
    assert second == -1  # one component (or none)


@pytest.mark.parametrize("k", [1, 2, 3, 5, 9])
def test_square_area_formula(k):
    m = np.zeros((k + 3, k + 4), bool)
    m[2:2 + k, 1:1 + k] = True
    assert br.box_of_mask(m)[:2] == ((1, 2, k, k), 2 * (k - 1) ** 2)


def test_ring_beats_a_solid_blob_with_more_pixels():
    m = np.zeros((12, 24), bool)
    m[1:10, 1:10] = True
    m[2:9, 2:9] = False  # 9 x 9 ring: 32 pixels, outline area 64
    m[2:8, 14:21] = True  # 6 x 7 blob: 42 pixels, outline area 30
    box, a2, second = br.box_of_mask(m)
    assert (box, a2, second) == ((1, 1, 9, 9), 128, 60)


def test_tie_goes_to_the_last_root_and_shows_in_second():
    m = np.zeros((9, 20), bool)
    m[1:4, 2:6] = True
    m[5:8, 11:15] = True
    box, a2, second = br.box_of_mask(m)
    assert (box, a2, second) == ((11, 5, 4, 3), 12, 12)
    m[1:4, 11:15] = True  # the same row as the first: the later column wins
    m[5:8, 11:15] = False
    assert br.box_of_mask(m)[0] == (11, 1, 4, 3)


def test_component_inside_a_hole_and_spike_into_the_hole():
    m = np.zeros((13, 13), bool)
    m[1:12, 1:12] = True
    m[2:11, 2:11] = False  # 11 x 11 ring
    m[7:11, 8] = True  # a spike from the bottom edge into the hole: its tip is a local top, traced (along the hole's border) and rejected
    m[4:6, 3:6] = True  # a component inside the hole
    assert [7, 8] in br.candidates(m).tolist()
    cs = br.contours(m)
    assert [(a2, box) for a2, _, box in cs] == [(200, (1, 1, 11, 11)), (4, (3, 4, 3, 2))]
    assert br.select(cs)[:2] == ((1, 1, 11, 11), 200)


def _cell_sum(filled: np.ndarray) -> int:
    """Sum over all 2 x 2 pixel cells of 2 for a full cell and 1 for a cell with three pixels set."""
    f = filled.astype(np.int64)
    n = f[:-1, :-1] + f[:-1, 1:] + f[1:, :-1] + f[1:, 1:]
    return int(2 * (n == 4).sum() + (n == 3).sum())


def _random_mask(rng, H, W):
    m = rng.random((H, W)) < rng.choice([0.02, 0.08, 0.3, 0.55])
    if rng.random() < 0.6:
        m = br.dilate(m, int(rng.choice([3, 5])))
    if rng.random() < 0.3:
        m &= rng.random((H, W)) < 0.9  # pinholes
    return m


def test_traces_agree_with_scipy_on_random_masks():
    """Every kept trace is one labelled 8-connected component, every component has exactly one, and its A2 is the 2 x 2 cell sum of the hole-filled
    component."""
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(20240613)
    eight = np.ones((3, 3), bool)
    n_contours = n_holes = 0
    for _ in range(400):
        H, W = int(rng.integers(3, 28)), int(rng.integers(3, 40))
        m = _random_mask(rng, H, W)
        lab, n = ndi.label(m, structure=eight)
        cs = br.contours(m)
        assert sorted(int(lab.flat[root]) for _, root, _ in cs) == list(range(1, n + 1))
        for a2, root, box in cs:
            comp = lab == lab.flat[root]
            assert root == int(np.flatnonzero(comp)[0])
            filled = ndi.binary_fill_holes(comp)  # (4-connected background: what an 8-connected foreground border encloses)
            assert a2 == _cell_sum(filled), (H, W, root)
            ys, xs = np.nonzero(comp)
            assert box == (xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1)
            n_contours += 1
            n_holes += int(filled.sum() != comp.sum())
    assert n_contours > 2000 and n_holes > 50, (n_contours, n_holes)  # (the sweep is not vacuous)


def test_morphology_borders():
    m = np.zeros((20, 30), bool)
    m[0:5, 0:5] = True  # flush in the corner: survives the 5 x 5 erosion, since out-of-image pixels never erode
    m[10:14, 20:24] = True  # a 4 x 4 speck does not
    e = br.erode(m, 5)
    want = np.zeros_like(m)
    want[0:3, 0:3] = True  # every window that holds no clear in-image pixel
    np.testing.assert_array_equal(e, want)
    d = br.morphology(m)
    want = np.zeros_like(m)
    want[0:10, 0:10] = True
    np.testing.assert_array_equal(d, want)
    assert br.box_of_mask(d)[0] == (0, 0, 10, 10)


def test_one_15_dilation_equals_the_5_and_the_11():
    rng = np.random.default_rng(3)
    for _ in range(20):
        m = rng.random((23, 37)) < 0.01
        m[0, 0] = m[-1, -1] = True
        np.testing.assert_array_equal(br.dilate(br.dilate(m, 5), 11), br.dilate(m, 15))
        # ... and the reference's order of operations: opening (erode, dilate 5), then dilate 11
        np.testing.assert_array_equal(br.dilate(br.dilate(br.erode(m, 5), 5), 11), br.morphology(m))


def test_box_ref_thresholds_strictly():
    bg = np.full((16, 16), 100, np.uint8)
    f = bg.copy()
    f[4:10, 4:10] = 120  # |diff| = t: background
    assert tuple(br.box_ref(f, bg, 20)[0]) == (0, 0, 0, 0)
    f[4:10, 4:10] = 79  # |diff| = t + 1, darker than the background
    box, a2, mask, second = br.box_ref(f, bg, 20)
    # 6 x 6 erodes to 2 x 2 at (6, 6), which dilates by 7 to [-1, 14] clipped to the image
    assert tuple(box) == (0, 0, 15, 15) and a2 == 2 * 14 * 14 and second == -1
    assert mask.dtype == np.uint8 and (mask[:15, :15] == 255).all() and mask.sum() == 255 * 225


def test_entry_points_are_exported(hip_lib):
    for name in ("wtk_boxes_scratch_bytes", "wtk_boxes"):
        assert name in hip.SYMBOLS and hasattr(hip_lib, name)
    assert hip.boxes_scratch_bytes(61, 131, 12) == 12 * (8 + 4 * 61 * 5)
    assert hip.boxes_scratch_bytes(1500, 1500, 951) <= ev.BOXES_SCRATCH_BYTES < hip.boxes_scratch_bytes(1500, 1500, 952)
    for bad in ((0, 8, 1), (8, 0, 1), (8, 8, 0), (1 << 15, (1 << 15) + 1, 1)):
        assert hip_lib.wtk_boxes_scratch_bytes(*bad) == -1
        with pytest.raises(hip.WtkError):
            hip.boxes_scratch_bytes(*bad)


def test_wtk_boxes_rejects_bad_arguments_before_any_launch(hip_lib):
    fake = 1 << 20  # never dereferenced: every call below fails its checks first
    need = hip.boxes_scratch_bytes(8, 8, 2)

    def call(frames=fake, n_frames=4, H=8, W=8, bg=fake, idx=fake, n_sel=2, thr=20, boxes=fake, area=fake, mask=None, faults=fake, scratch=fake,
             scratch_bytes=need):
        hip.boxes(frames, n_frames, H, W, bg, idx, n_sel, thr, boxes, area, mask, faults, scratch, scratch_bytes)

    for kw in ({"frames": None}, {"bg": None}, {"faults": None}, {"scratch": None}, {"boxes": None}):
        with pytest.raises(hip.WtkError, match="null"):
            call(**kw)
    for kw in ({"n_frames": 0}, {"n_sel": 0}, {"n_sel": -3}):
        with pytest.raises(hip.WtkError, match="positive"):
            call(**kw)
    for kw in ({"H": 0}, {"W": -1}, {"H": 1 << 15, "W": (1 << 15) + 1, "scratch_bytes": 1 << 40}):
        with pytest.raises(hip.WtkError, match="H x W"):
            call(**kw)
    for thr in (0, -1, 256):
        with pytest.raises(hip.WtkError, match="1 .. 255"):
            call(thr=thr)
    with pytest.raises(hip.WtkError, match="exceed n_frames"):
        call(idx=None, n_sel=5, scratch_bytes=1 << 20)
    with pytest.raises(hip.WtkError, match="too small"):
        call(scratch_bytes=need - 1)
    with pytest.raises(hip.WtkError, match="aligned"):
        call(scratch=fake + 4)
    assert hip_lib.wtk_boxes(ctypes.c_void_p(fake), 4, 8, 8, ctypes.c_void_p(fake), None, 2, 0, ctypes.c_void_p(fake), None, None, ctypes.c_void_p(fake),
                             ctypes.c_void_p(fake), need, None) != 0
    assert b"diff_thresh" in hip_lib.wtk_last_error()


class _Reader:
    def __init__(self, frames):
        self.frames, self.frame_shape = frames, frames.shape[1:]

    def __len__(self):
        return len(self.frames)

    def __getitem__(self, i):
        return self.frames[i]


def test_box_calculator_makes_the_references_assertions():
    frames = np.zeros((5, 8, 9), np.uint8)
    bg = np.zeros((8, 9), np.uint8)
    for src in (frames, _Reader(frames)):
        with pytest.raises(AssertionError, match="greater than 0"):
            ev.BoxCalculator(src, bg, diff_thresh=0)
        with pytest.raises(AssertionError, match="Background shape"):
            ev.BoxCalculator(src, bg[:, :8])
        calc = ev.BoxCalculator(src, bg)
        assert calc.all_bboxes().shape == (5, 4) and calc.all_bboxes().dtype == np.int64 and (calc.all_bboxes() == -1).all()
        with pytest.raises(IndexError):
            calc.calc_specified_boxes([5])
    with pytest.raises(ValueError, match="colour"):
        ev.BoxCalculator(np.zeros((5, 8, 9, 3), np.uint8), np.zeros((8, 9, 3), np.uint8))
    with pytest.raises(ValueError, match="gray or a color"):
        ev.BoxCalculator(np.zeros((5, 8), np.uint8), np.zeros(8, np.uint8))


def test_boxes_rejects_what_it_cannot_compute():
    with pytest.raises(ValueError, match="colour"):
        ev.boxes(np.zeros((2, 8, 8, 3), np.uint8), np.zeros((8, 8), np.uint8))
    with pytest.raises(AssertionError, match="greater than 0"):
        ev.boxes(np.zeros((2, 8, 8), np.uint8), np.zeros((8, 8), np.uint8), diff_thresh=0)
    with pytest.raises(ValueError, match="background"):
        ev.boxes(np.zeros((2, 8, 8), np.uint8), np.zeros((8, 9), np.uint8))
