"""GPU checks of the background-subtraction worm boxes (csrc/box_ops.hip, wtracker_amd.evaluation.boxes): boxes, A2 and masks equal the numpy restatement
(tests/harness/box_ref.py) exactly -- on constructed frames that hit every border, word boundary and selection rule, on a random sweep, on one
user-shaped frame size -- plus selection, validation, stream order and the hand-over to Replay."""
import numpy as np
import pytest

from harness import box_ref as br
from wtracker_amd import evaluation as ev
from wtracker_amd import hip
from wtracker_amd.sim import ExperimentConfig, TimingConfig

pytestmark = pytest.mark.gpu
T = 20


@pytest.fixture(scope="module")
def torch_mod(hip_lib):
    import torch

    if hip.device_count() < 1:
        pytest.fail("no HIP device visible")
    return torch


def _rect(f, bg, x0, y0, w, h, d=40):
    f[y0:y0 + h, x0:x0 + w] = (bg[y0:y0 + h, x0:x0 + w].astype(np.int16) + d).astype(np.uint8)


def _ring(f, bg, x0, y0, w, h, wall):
    _rect(f, bg, x0, y0, w, h)
    _rect(f, bg, x0 + wall, y0 + wall, w - 2 * wall, h - 2 * wall, 0)


TIE_FRAMES = (9, 10)


def constructed():
    """12 frames of 61 x 131 (odd H W: every second frame starts on an odd byte; W spans four words and a 3-pixel tail) over a textured background."""
    H, W = 61, 131
    rng = np.random.default_rng(5)
    bg = rng.integers(60, 181, (H, W)).astype(np.uint8)
    fr = np.repeat(bg[None], 12, axis=0)
    _rect(fr[0], bg, 28, 10, 10, 8)    # 0: across the 32-bit word boundary at x = 32 ...
    _rect(fr[0], bg, 58, 30, 12, 10)   # ... and the 64-bit one at x = 64
    _rect(fr[1], bg, 50, 0, 7, 6)      # 1: flush with the top,
    _rect(fr[1], bg, 20, 55, 8, 6)     # the bottom,
    _rect(fr[1], bg, 0, 25, 6, 8)      # the left,
    _rect(fr[1], bg, 125, 20, 6, 9)    # the right border (in the 3-pixel tail word)
    _rect(fr[1], bg, 122, 52, 9, 9)    # and in the bottom-right corner
    _rect(fr[2], bg, 20, 20, 4, 4)     # 2: a 4 x 4 speck (opened away) next to
    _rect(fr[2], bg, 30, 20, 5, 5)     # a 5 x 5 one (survives as one pixel, dilated to 15 x 15)
    _ring(fr[3], bg, 5, 8, 40, 40, 5)  # 3: a ring, 2100 pixels after the morphology, outline 49 x 49,
    _rect(fr[3], bg, 75, 10, 37, 37)   # against a solid blob of 47 x 47 = 2209 pixels, outline 46 x 46: the ring must win
    _ring(fr[4], bg, 10, 2, 60, 56, 6)  # 4: a ring with
    _rect(fr[4], bg, 37, 30, 6, 22)    # a spike from its bottom wall into the hole (its tip is a local top)
    _ring(fr[5], bg, 10, 2, 60, 56, 6)  # 5: a ring with
    _rect(fr[5], bg, 37, 27, 7, 7)     # a component inside its hole
    #                                    6: an empty frame
    fr[7] = (bg.astype(np.int16) - 40).astype(np.uint8)  # 7: all foreground
    _rect(fr[8], bg, 10, 10, 8, 8, T)        # 8: |diff| = t: background
    _rect(fr[8], bg, 60, 10, 8, 8, T + 1)    # |diff| = t + 1: foreground
    _rect(fr[8], bg, 100, 40, 9, 9, -T - 1)  # ... and darker than the background
    _rect(fr[9], bg, 20, 10, 8, 8)     # 9: two identical blobs on different rows: the later one wins
    _rect(fr[9], bg, 90, 35, 8, 8)
    _rect(fr[10], bg, 10, 20, 8, 8)    # 10: ... and on the same rows
    _rect(fr[10], bg, 100, 20, 8, 8)
    speck = rng.random((H, W)) < 0.03  # 11: speckle over a disc
    fr[11][speck] = (bg[speck].astype(np.int16) + 40).astype(np.uint8)
    yy, xx = np.mgrid[:H, :W]
    disc = (yy - 30) ** 2 + (xx - 80) ** 2 <= 81
    fr[11][disc] = (bg[disc].astype(np.int16) - 40).astype(np.uint8)
    return fr, bg


@pytest.fixture(scope="module")
def built(torch_mod):
    fr, bg = constructed()
    ref = br.boxes_ref(fr, bg, T)
    for a in ref:
        a.setflags(write=False)
    return {"frames": fr, "bg": bg, "ref": ref, "dev": torch_mod.from_numpy(fr).cuda(), "bg_dev": torch_mod.from_numpy(bg).cuda()}


def _assert_equal(got, ref, rows=None):
    rows = slice(None) if rows is None else rows
    boxes, area, mask = (g.cpu().numpy() for g in got)
    np.testing.assert_array_equal(mask, ref[2][rows])
    np.testing.assert_array_equal(area, ref[1][rows])
    np.testing.assert_array_equal(boxes, ref[0][rows])
    assert boxes.dtype == np.int32 and area.dtype == np.int64 and mask.dtype == np.uint8


def test_constructed_frames_say_what_they_are_meant_to(built):
    """The harness's own view of the constructed frames: the cases are the ones the comments name."""
    boxes, a2, masks, second = built["ref"]
    assert [k for k in range(12) if second[k] == a2[k]] == list(TIE_FRAMES)
    assert tuple(boxes[2]) == (25, 15, 15, 15)  # the 5 x 5 speck alone
    assert tuple(boxes[3]) == (0, 3, 50, 50) and a2[3] == 2 * 49 * 49 and second[3] == 2 * 46 * 46  # the ring, with fewer pixels than the blob
    m3 = masks[3] > 0
    assert m3[:, :60].sum() == 2100 and m3[:, 60:].sum() == 2209
    assert tuple(boxes[6]) == (0, 0, 0, 0) and a2[6] == 0
    assert tuple(boxes[7]) == (0, 0, 131, 61) and a2[7] == 2 * 130 * 60
    assert tuple(boxes[8]) == (95, 35, 19, 19) and masks[8][:30, :50].sum() == 0  # the darker 9 x 9 (5 x 5 eroded) beats the 8 x 8; |diff| = t is nothing
    assert tuple(boxes[9]) == (85, 30, 18, 18) and tuple(boxes[10]) == (95, 15, 18, 18)  # ties: the last root
    assert len(br.contours(masks[5] > 0)) == 2 and len(br.contours(masks[4] > 0)) == 1
    assert len(br.candidates(masks[4] > 0)) == 2  # the ring's first pixel and the spike's tip


def test_constructed_frames(torch_mod, built):
    got = ev.boxes(built["dev"], built["bg_dev"], T, return_area=True, return_mask=True)
    _assert_equal(got, built["ref"])


def _sweep():
    """64 frames of 96 x 200: rectangles, discs and speckle over a textured background, brighter and darker than it."""
    rng = np.random.default_rng(11)
    H, W, F = 96, 200, 64
    bg = rng.integers(50, 200, (H, W)).astype(np.uint8)
    fr = np.repeat(bg[None], F, axis=0)
    yy, xx = np.mgrid[:H, :W]
    for f in fr:
        fg = rng.random((H, W)) < rng.choice([0.0, 0.01, 0.05])
        for _ in range(int(rng.integers(0, 6))):
            x0, y0 = int(rng.integers(-5, W)), int(rng.integers(-5, H))
            w, h = int(rng.integers(3, 40)), int(rng.integers(3, 30))
            fg[max(y0, 0):max(y0 + h, 0), max(x0, 0):max(x0 + w, 0)] = True
        for _ in range(int(rng.integers(0, 4))):
            cx, cy, r = int(rng.integers(0, W)), int(rng.integers(0, H)), int(rng.integers(2, 16))
            fg |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
        fg &= rng.random((H, W)) < 0.995  # pinholes
        d = np.where(rng.random((H, W)) < 0.5, 1, -1) * rng.integers(T + 1, 50, (H, W))
        f[fg] = (bg[fg].astype(np.int16) + d[fg]).astype(np.uint8)
    return fr, bg


def test_random_sweep(torch_mod):
    fr, bg = _sweep()
    ref = br.boxes_ref(fr, bg, T)
    assert int((ref[3] == ref[1]).sum()) == 0  # no frame of this seed has a tie for the largest area: every box is pinned
    assert int((ref[1] > 0).sum()) >= 48 and len({tuple(b) for b in ref[0]}) >= 40
    got = ev.boxes(torch_mod.from_numpy(fr).cuda(), torch_mod.from_numpy(bg).cuda(), T, return_area=True, return_mask=True)
    _assert_equal(got, ref)


def test_user_shaped_frames(torch_mod):
    """3 frames of 1080 x 1440: a curled worm 9 pixels thick and speckle noise, selected out of order."""
    rng = np.random.default_rng(2)
    H, W = 1080, 1440
    bg = rng.integers(90, 140, (H, W)).astype(np.uint8)
    fr = np.repeat(bg[None], 3, axis=0)
    yy, xx = np.mgrid[-4:5, -4:5]
    disc = yy ** 2 + xx ** 2 <= 16
    for k, f in enumerate(fr):
        noise = rng.random((H, W)) < 0.002
        f[noise] = 255
        s = np.linspace(0, 1, 400)
        cx = 300 + 400 * k + 60 * np.cos(4.5 * np.pi * s) * (1 - 0.7 * s)
        cy = 500 + 120 * k + 60 * np.sin(4.5 * np.pi * s) * (1 - 0.7 * s) + 90 * s
        for x, y in zip(cx.astype(int), cy.astype(int)):
            f[y - 4:y + 5, x - 4:x + 5][disc] = 20
    sel = [2, 0]
    ref = br.boxes_ref(fr, bg, T, sel)
    assert (ref[1] > 0).all() and (ref[3] != ref[1]).all()
    got = ev.boxes(torch_mod.from_numpy(fr).cuda(), torch_mod.from_numpy(bg).cuda(), T, frame_indices=sel, return_area=True, return_mask=True)
    _assert_equal(got, ref)


def test_out_of_range_and_repeated_indices(torch_mod, built):
    torch = torch_mod
    faults = torch.zeros(1, dtype=torch.int32, device="cuda")
    sel = [3, 99, 4, -1, 4, 12, 11]
    got = ev.boxes(built["dev"], built["bg_dev"], T, frame_indices=sel, return_area=True, return_mask=True, fault_count=faults)
    boxes, area, mask = (g.cpu().numpy() for g in got)
    assert int(faults.item()) == 3
    for row, f in enumerate(sel):
        if 0 <= f < 12:
            np.testing.assert_array_equal(boxes[row], built["ref"][0][f])
            assert area[row] == built["ref"][1][f]
            np.testing.assert_array_equal(mask[row], built["ref"][2][f])
        else:
            assert boxes[row].tolist() == [-1, -1, -1, -1] and area[row] == -1 and not mask[row].any()
    idx = torch.tensor([7, 7, 0], dtype=torch.int32, device="cuda")  # a device tensor of indices
    np.testing.assert_array_equal(ev.boxes(built["dev"], built["bg_dev"], T, frame_indices=idx).cpu().numpy(), built["ref"][0][[7, 7, 0]])


def test_small_scratch_is_refused_before_any_launch(torch_mod, built):
    torch = torch_mod
    H, W = built["bg"].shape
    need = hip.boxes_scratch_bytes(H, W, 12)
    out = torch.full((12, 4), 77, dtype=torch.int32, device="cuda")
    faults = torch.zeros(1, dtype=torch.int32, device="cuda")
    scratch = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda")
    with pytest.raises(hip.WtkError, match="too small"):
        hip.boxes(built["dev"], 12, H, W, built["bg_dev"], None, 12, T, out, None, None, faults, scratch, need - 1)
    torch.cuda.synchronize()
    assert (out == 77).all() and int(faults.item()) == 0 and (scratch == 0x5A).all()
    hip.boxes(built["dev"], 12, H, W, built["bg_dev"], None, 12, T, out, None, None, faults, scratch, need)
    np.testing.assert_array_equal(out.cpu().numpy(), built["ref"][0])
    # the mask stage alone leaves the bit-packed mask behind the keys
    scratch.zero_()
    hip.boxes(built["dev"], 12, H, W, built["bg_dev"], None, 12, T, None, None, None, faults, scratch, need)
    words = scratch[8 * 12:].cpu().numpy().view(np.uint32).reshape(12, H, (W + 31) // 32)
    bits = ((words[..., None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(12, H, -1)
    np.testing.assert_array_equal(bits[:, :, :W] * 255, built["ref"][2])
    assert not bits[:, :, W:].any() and int(faults.item()) == 0


def test_chunked_calls_equal_one_call(torch_mod, built, monkeypatch):
    H, W = built["bg"].shape
    monkeypatch.setattr(ev, "BOXES_SCRATCH_BYTES", hip.boxes_scratch_bytes(H, W, 5))  # chunks of 5, 5 and 2 frames
    _assert_equal(ev.boxes(built["dev"], built["bg_dev"], T, return_area=True, return_mask=True), built["ref"])
    sel = [11, 0, 3, 3, 9, 10, 1]
    _assert_equal(ev.boxes(built["dev"], built["bg_dev"], T, frame_indices=sel, return_area=True, return_mask=True), built["ref"], sel)
    # host frames: only the selection is uploaded, chunk by chunk
    _assert_equal(ev.boxes(built["frames"], built["bg"], T, frame_indices=sel, return_area=True, return_mask=True), built["ref"], sel)


def test_a_frame_alone_gives_the_bits_it_gives_in_a_selection(torch_mod, built):
    for f in range(12):
        _assert_equal(ev.boxes(built["dev"], built["bg_dev"], T, frame_indices=[f], return_area=True, return_mask=True), built["ref"], [f])


def test_box_calculator(torch_mod, built):
    class Reader:
        frame_shape = built["bg"].shape

        def __len__(self):
            return 12

        def __getitem__(self, i):
            return built["frames"][i]

    calc = ev.BoxCalculator(Reader(), built["bg"], T)
    np.testing.assert_array_equal(calc.get_bbox(3), built["ref"][0][3])
    np.testing.assert_array_equal(calc.calc_specified_boxes([5, 3, 5], num_workers=4, chunk_size=2), built["ref"][0][[5, 3, 5]])
    want = np.full((12, 4), -1)
    want[[3, 5]] = built["ref"][0][[3, 5]]
    np.testing.assert_array_equal(calc.all_bboxes(), want)
    got = ev.BoxCalculator(built["dev"], built["bg_dev"], T).calc_all_boxes()
    assert got.dtype == np.int64
    np.testing.assert_array_equal(got, built["ref"][0])


def test_boxes_run_in_stream_order(torch_mod, built):
    """boxes() enqueued on a side stream behind a device-side fill of the frames sees the filled frames (and never the zeros they held before)."""
    torch = torch_mod
    frames = torch.zeros_like(built["dev"])
    src = built["dev"].clone()
    a = torch.randn(2048, 2048, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(20):  # work that keeps the stream busy ahead of the fill
            a = a @ a * 1e-3
        frames.copy_(src)
        got = ev.boxes(frames, built["bg_dev"], T, return_area=True, return_mask=True)
    side.synchronize()
    _assert_equal(got, built["ref"])


def test_background_boxes_replay_end_to_end(torch_mod):
    """A moving blob through background() -> boxes() -> .double() -> Replay(...).run(rp.csv()): the log's worm columns are the harness's boxes."""
    from wtracker_amd.replay import Replay

    torch = torch_mod
    rng = np.random.default_rng(9)
    F, H, W = 60, 120, 160
    base = rng.integers(100, 130, (H, W)).astype(np.uint8)
    fr = np.repeat(base[None], F, axis=0)
    for k, f in enumerate(fr):
        x, y = 10 + 2 * k, 20 + k
        f[y:y + 9, x:x + 12] = 30
    dev = torch.from_numpy(fr).cuda()
    bg = ev.background(dev, 30, "uniform", "median")
    np.testing.assert_array_equal(bg.cpu().numpy(), base)
    track = ev.boxes(dev, bg, T)
    ref = br.boxes_ref(fr, base, T)[0]
    np.testing.assert_array_equal(track.cpu().numpy(), ref)
    ec = ExperimentConfig(name="boxes", num_frames=F, frames_per_sec=60, orig_resolution=(H, W), px_per_mm=10, init_position=(20, 20))
    tc = TimingConfig(ec, 100, 40, 50, (4, 4), (0.32, 0.32))
    rp = Replay(track.double(), tc, ec, frame_shape=(H, W))
    res = rp.run(rp.csv())
    rows = res.row_array(0)
    assert rows.shape[0] == rp.n_rows > 40
    np.testing.assert_array_equal(rows[:, 10:14], ref[:rp.n_rows].astype(np.float64))
    assert [r["wrm_w"] for r in res.log(0)] == ref[:rp.n_rows, 2].astype(float).tolist()
