"""Experiment evaluation on the MI355X (wtracker_amd/evaluation.py, csrc/eval_ops.hip): the device background and precise error bit for bit against
the real reference's outputs (tests/golden/eval_*.npz) and against the numpy restatement tests/harness/eval_ref.py at user scale, the counter-width
limits, stream ordering, and a closed-loop sim run evaluated end to end."""
import os

import numpy as np
import pytest
import torch

from harness import eval_ref
from wtracker_amd import evaluation as ev
from wtracker_amd import hip

pytestmark = pytest.mark.gpu


def _bits_equal(got: np.ndarray, want: np.ndarray):
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_array_equal(got.view(np.uint64)[~np.isnan(got)], want.view(np.uint64)[~np.isnan(want)])


class _Reader:
    def __init__(self, frames):
        self.frames = frames

    def __len__(self):
        return len(self.frames)

    @property
    def frame_shape(self):
        return self.frames.shape[1:]

    def __getitem__(self, i):
        return self.frames[i]


def test_background_equals_the_reference_fixtures(hip_lib, golden_dir):
    z = np.load(os.path.join(golden_dir, "eval_background.npz"))
    dev = {k: torch.from_numpy(z[k]).cuda() for k in ("gray", "bgr")}
    for c in range(len(z["meta_frames"])):
        key, n, sampling, method, seed = (str(z["meta_frames"][c]), int(z["meta_num_probes"][c]), str(z["meta_sampling"][c]),
                                          str(z["meta_method"][c]), int(z["meta_seed"][c]))
        for src in ("device", "host", "reader"):
            if seed >= 0:
                np.random.seed(seed)
            if src == "device":
                bg = ev.background(dev[key], n, sampling, method)
                assert bg.is_cuda and bg.dtype == torch.uint8
                bg = bg.cpu().numpy()
            elif src == "host":
                bg = ev.background(z[key], n, sampling, method).cpu().numpy()
            else:
                bg = ev.BGExtractor(_Reader(z[key])).calc_background(n, sampling=sampling, method=method)
            np.testing.assert_array_equal(bg, z[f"bg_{c}"], err_msg=f"case {c} ({key}, n={n}, {sampling}, {method}) from {src}")


@pytest.mark.parametrize("n_probes", [301, 300])
def test_background_at_user_scale_equals_numpy(hip_lib, n_probes):
    """301 frames of 1080 x 1440 gray: every frame (odd n) and 300 uniform probes (even n), median and mean against numpy on the host; the columns
    mix random bytes with nibble-boundary pairs and constants."""
    g = torch.Generator(device="cuda").manual_seed(n_probes)
    frames = torch.randint(0, 256, (301, 1080, 1440), dtype=torch.uint8, device="cuda", generator=g)
    frames[:, :, 0::7] = torch.randint(15, 17, frames[:, :, 0::7].shape, dtype=torch.uint8, device="cuda", generator=g)
    frames[:, :, 1::7] = torch.randint(254, 256, frames[:, :, 1::7].shape, dtype=torch.uint8, device="cuda", generator=g)
    frames[:, 5:9, :] = 37
    ids = ev.probe_indices(301, n_probes, "uniform")
    host = frames.cpu().numpy()[ids]
    for method in ("median", "mean"):
        got = ev.background(frames, n_probes, "uniform", method).cpu().numpy()
        want = np.median(host, axis=0).astype(np.uint8) if method == "median" else (host.sum(axis=0, dtype=np.int64) // len(ids)).astype(np.uint8)
        np.testing.assert_array_equal(got, want, err_msg=method)


def test_background_of_bgr_frames(hip_lib):
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, (33, 270, 361, 3), dtype=np.uint8)  # 292 410 bytes per frame: not a multiple of 4 -> the byte-wise path
    dev = torch.from_numpy(frames).cuda()
    for n in (33, 16):
        ids = ev.probe_indices(33, n, "uniform")
        got = ev.background(dev, n, "uniform", "median").cpu().numpy()
        np.testing.assert_array_equal(got, np.median(frames[ids], axis=0).astype(np.uint8))
        got = ev.background(dev, n, "uniform", "mean").cpu().numpy()
        np.testing.assert_array_equal(got, eval_ref.background(frames, ids, "mean"))


def test_probe_count_limits_are_exact(hip_lib):
    """The largest n each method accepts is exact at its counters' worst case (every probe in one bin / every byte 255); n + 1 is refused."""
    rng = np.random.default_rng(9)
    F, nbytes = 5, 256
    frames = rng.integers(0, 256, (F, nbytes), dtype=np.uint8)
    frames[:, :64] = 200  # constant columns: one median bin counts every probe
    frames[:, 64:80] = 255
    dev = torch.from_numpy(frames).cuda()
    bg = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    n = hip.BG_MEDIAN_MAX_PROBES
    ids = rng.integers(0, F, n).astype(np.int32)
    hip.background(dev, F, nbytes, torch.from_numpy(ids).cuda(), n, hip.BG_MEDIAN, bg, s)
    np.testing.assert_array_equal(bg.cpu().numpy(), np.median(frames[ids], axis=0).astype(np.uint8))
    with pytest.raises(hip.WtkError, match="65535"):
        hip.background(dev, F, nbytes, torch.from_numpy(np.zeros(n + 1, np.int32)).cuda(), n + 1, hip.BG_MEDIAN, bg, s)
    all255 = torch.full((2, nbytes), 255, dtype=torch.uint8, device="cuda")
    n = hip.BG_MEAN_MAX_PROBES
    ids_dev = torch.randint(0, 2, (n,), dtype=torch.int32, device="cuda")
    hip.background(all255, 2, nbytes, ids_dev, n, hip.BG_MEAN, bg, s)
    assert (bg.cpu().numpy() == 255).all()  # 255 * 2^24 = 4 278 190 080 < 2^32
    ids = ids_dev.cpu().numpy()
    counts = np.bincount(ids, minlength=F)
    want = (counts[:, None].astype(np.int64) * frames.astype(np.int64)).sum(axis=0) // n
    hip.background(dev, F, nbytes, ids_dev, n, hip.BG_MEAN, bg, s)
    np.testing.assert_array_equal(bg.cpu().numpy(), want.astype(np.uint8))
    with pytest.raises(hip.WtkError, match="2\\^24"):
        hip.background(dev, F, nbytes, ids_dev, n + 1, hip.BG_MEAN, bg, s)


def test_precise_error_equals_the_reference_fixtures(hip_lib, golden_dir):
    z = np.load(os.path.join(golden_dir, "eval_precise.npz"))
    frames = torch.from_numpy(z["frames"]).cuda()
    c = 0
    while f"ref_{c}" in z:
        dt = np.float32 if bool(z[f"f32_{c}"]) else np.float64
        worm, mic, thr = z["worm"].astype(dt), z["mic"].astype(dt), float(z[f"thresh_{c}"])
        worm_before = worm.copy()
        want_err, want_counts = eval_ref.precise(z["frames"], z["background"], worm, mic, z["frame_nums"], thr)
        err, counts = ev.precise_error(frames, z["background"], worm, mic, z["frame_nums"], thr, return_counts=True)
        assert err.is_cuda and err.dtype == torch.float64
        _bits_equal(err.cpu().numpy(), want_err)
        np.testing.assert_array_equal(counts.cpu().numpy(), want_counts)
        ref = ev.precise_error(frames, torch.from_numpy(z["background"]).cuda(), torch.from_numpy(worm).cuda(), torch.from_numpy(mic).cuda(),
                               torch.from_numpy(z["frame_nums"].astype(np.int32)).cuda(), thr, layout="reference")
        _bits_equal(ref.cpu().numpy(), z[f"ref_{c}"])
        np.testing.assert_array_equal(worm, worm_before)  # the reference's discretize zeroes NaN rows of the caller's array; this one does not
        c += 1
    assert c == 4


def test_precise_error_at_scale(hip_lib):
    """20 000 rows on 64 frames of 120 x 160: head-sized boxes, frame-sized boxes, NaN rows, boxes over every border; float64 and float32."""
    rng = np.random.default_rng(11)
    F, H, W, N = 64, 120, 160, 20000
    bg = rng.integers(90, 110, (H, W), dtype=np.uint8)
    frames = np.clip(bg[None].astype(np.int32) + rng.integers(-25, 26, (F, H, W)), 0, 255).astype(np.uint8)
    xy = rng.uniform(-20, 170, (N, 2))
    wh = rng.uniform(0, 30, (N, 2))
    worm = np.concatenate([xy, wh], axis=1)
    worm[::50] = (-2.5, -1.25, W + 4.0, H + 3.0)
    worm[7::97] = np.nan
    mic = worm + rng.uniform(-15, 15, (N, 4))
    mic[3::41] = (-1.0, -1.0, W + 2.0, H + 2.0)
    fn = rng.integers(0, F, N)
    dev = torch.from_numpy(frames).cuda()
    for dt in (np.float64, np.float32):
        want_err, want_counts = eval_ref.precise(frames, bg, worm.astype(dt), mic.astype(dt), fn, 20)
        err, counts = ev.precise_error(dev, bg, worm.astype(dt), mic.astype(dt), fn, 20, return_counts=True)
        _bits_equal(err.cpu().numpy(), want_err)
        np.testing.assert_array_equal(counts.cpu().numpy(), want_counts)
        _bits_equal(ev.precise_error(dev, bg, worm.astype(dt), mic.astype(dt), fn, 20, layout="reference").cpu().numpy(),
                    eval_ref.reference_layout(want_err))
    whole = (np.abs(frames[fn[::50]].astype(np.int32) - bg.astype(np.int32)) > 20).sum(axis=(1, 2))
    big = ~np.isnan(want_err[::50])  # (a few of them are NaN rows)
    assert big.sum() > 350
    np.testing.assert_array_equal(want_counts[::50, 0][big], whole[big])  # the frame-sized rows walked the whole frame


def test_frame_number_outside_the_frames_raises(hip_lib):
    frames = torch.zeros((4, 16, 16), dtype=torch.uint8, device="cuda")
    bg = torch.zeros((16, 16), dtype=torch.uint8, device="cuda")
    worm = np.array([[1.0, 1.0, 4.0, 4.0], [np.nan] * 4, [2.0, 2.0, 3.0, 3.0]])
    # an illegal row is never read, whatever its frame number (the reference drops it before the loop)
    ev.precise_error(frames, bg, worm, worm, [0, 99, 3])
    with pytest.raises(IndexError):
        ev.precise_error(frames, bg, worm, worm, [0, 1, 4])
    with pytest.raises(IndexError):
        ev.precise_error(frames, bg, worm, worm, [-1, 1, 2])


def test_frames_written_on_the_current_stream_just_before_the_call(hip_lib):
    """No synchronisation between a torch op that writes the frames and the evaluation calls: both run in order on the current stream."""
    rng = np.random.default_rng(3)
    F, H, W = 48, 512, 640
    new = torch.from_numpy(rng.integers(0, 256, (F, H, W), dtype=np.uint8)).cuda()
    worm = np.concatenate([rng.uniform(0, 600, (400, 2)), rng.uniform(5, 200, (400, 2))], axis=1)
    fn = rng.integers(0, F, 400)
    host = new.cpu().numpy()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        frames = torch.zeros((F, H, W), dtype=torch.uint8, device="cuda")
        for _ in range(4):
            frames.copy_(new.flip(2).flip(1))  # a long queue of writes in front ...
        frames.copy_(new)  # ... the last of which the evaluation must see
        bg = ev.background(frames, 25, "uniform", "median")
        err = ev.precise_error(frames, bg, worm, worm, fn, 10)
    side.synchronize()
    want_bg = eval_ref.background(host, ev.probe_indices(F, 25, "uniform"), "median")
    np.testing.assert_array_equal(bg.cpu().numpy(), want_bg)
    _bits_equal(err.cpu().numpy(), eval_ref.precise(host, want_bg, worm, worm, fn, 10)[0])


def test_closed_loop_sim_then_precise_error_from_the_log(hip_lib, tmp_path):
    """A short closed-loop sim over device_frames with TrackLogger, the background of the same device frames, then precise_error_from_log on the
    logger's rows and on its CSV: equal to the restatement on the same rows, in both layouts."""
    from harness.sim_harness import ArrayReader, Simulator
    from wtracker_amd import frames as fr
    from wtracker_amd import yolo_spec as ys
    from wtracker_amd.controllers import HipYoloController, YoloConfig
    from wtracker_amd.sim import ExperimentConfig, TimingConfig, TrackLogger

    w = ys.synthetic_weights("n", 1, seed=0)
    path = str(tmp_path / "n.wtk")
    ys.save_weights(path, w, "n", 1)
    frames, _ = fr.synthetic_frames(40, 256, seed=8)
    ec = ExperimentConfig("synthetic", 40, 60, (256, 256), 32, (128, 128))
    tc = TimingConfig(ec, 100, 40, 50, (4, 4), (0.5, 0.5))
    cfg = YoloConfig(model_path=path, device="cuda", pred_kwargs={"imgsz": 128, "conf": 0.1}, dtype="fp32", scale="n", max_batch=16)
    dev = torch.from_numpy(frames).cuda()
    csv_path = str(tmp_path / "bboxes.csv")
    log = TrackLogger(HipYoloController(tc, cfg, device_frames=dev), csv_path=csv_path)
    Simulator(tc, ec, log, reader=ArrayReader(frames)).run()
    assert len(log.rows) == 36
    bg = ev.background(dev, 1000, "uniform", "median")
    np.testing.assert_array_equal(bg.cpu().numpy(), np.median(frames, axis=0).astype(np.uint8))
    fn, worm, mic = ev.read_log(log.rows)
    want, _ = eval_ref.precise(frames, bg.cpu().numpy(), worm, mic, fn, 20)
    assert (~np.isnan(want)).sum() > 0
    for src in (log.rows, csv_path):
        _bits_equal(ev.precise_error_from_log(src, dev, bg).cpu().numpy(), want)
        _bits_equal(ev.precise_error_from_log(src, dev, bg, layout="reference").cpu().numpy(), eval_ref.reference_layout(want))
