"""The per-layer checker (tests/harness/layer_ref.py) on the CPU: its graph mirrors YoloOracle.forward, honest arithmetic of each mode passes its
bounds on the real layer shapes, and the defects a kernel plausibly has fail them."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from harness import layer_ref as lr
from oracle import yolo_oracle as yo
from wtracker_amd import yolo_spec as ys

KAPPA = np.float32(1.4426950408889634)  # the library stores SiLU outputs log2(e)-scaled


class _Recorder(yo.YoloOracle):
    """The oracle in float64, recording every conv blob as the library stores it (m.i.cv2 of a shortcut C2f: y[-1] + silu(conv))."""

    def __init__(self, weights, dims):
        super().__init__(weights, dims)
        self.w = {k: (w.double(), b.double()) for k, (w, b) in self.w.items()}
        self.rec = {}

    def conv(self, name, x, stride=1, act=True):
        y = super().conv(name, x, stride, act)
        self.rec[name] = y
        return y

    def c2f(self, p, x, n, shortcut):
        out = super().c2f(p, x, n, shortcut)
        if shortcut:
            y = self.rec[p + ".cv1"].chunk(2, 1)[1]
            for i in range(n):
                y = y + self.rec[f"{p}.m.{i}.cv2"]
                self.rec[f"{p}.m.{i}.cv2"] = y
        return out


def _dims(scale, nc):
    depth, width, maxch = ys.SCALES[scale]
    return ys.model_dims(width, depth, maxch, nc)


def _frames(B, H, W, seed=0):
    return np.random.default_rng(seed).integers(0, 256, size=(B, H, W), dtype=np.uint8)


@pytest.mark.parametrize("scale,nc", [("s", 1), ("s", 20), ("s", 80), ("n", 1), ("n", 80), ("m", 1), ("m", 20), ("l", 1), ("x", 1)])
def test_graph_mirror_checks_the_oracle_to_zero_error(scale, nc):
    w = ys.synthetic_weights(scale, nc, seed=0)
    frames = _frames(2, 64, 96, seed=1)
    o = _Recorder(w, _dims(scale, nc))
    with torch.no_grad():
        o.forward(lr.stem_input(frames))
    assert len(o.rec) == len(ys.conv_table(scale, nc))
    rep = lr.check_network(lr.DictSource(o.rec), w, frames, scale, nc, "fp32")
    assert len(rep.layers) == len(ys.conv_table(scale, nc))
    assert all(r.worst == 0.0 and r.rms == 0.0 for r in rep.layers), rep.table()


# ---- emulated honest arithmetic of each mode ---------------------------------------------------------------------------------------------
def _f16(t):
    return t.to(torch.float16).to(torch.float32)


def _split(t):
    hi = _f16(t)
    lo = _f16((t - hi) * 2048.0)
    return hi, lo


def _store(y, mode, act):
    """What a stored tensor reads back as (float32)."""
    if mode == "fp32" or not act:  # Detect outputs are fp32 in every mode
        return y
    if mode == "fp16":
        return _f16(y * KAPPA) * np.float32(1.0 / KAPPA)
    hi, lo = _split(y * KAPPA)
    return (hi + lo * np.float32(1.0 / 2048.0)) * np.float32(1.0 / KAPPA)


def _emul_conv(x, W, b, stride, mode, drop_lo=None):
    """x float32 (stored values), W float32 OIHW."""
    pad = W.shape[2] // 2
    if mode == "fp32":
        return F.conv2d(x, W, b, stride=stride, padding=pad)
    if mode == "fp16":
        return F.conv2d(_f16(x), _f16(W), b, stride=stride, padding=pad)
    xh, xl = _split(x)
    wh, wl = _split(W)
    if drop_lo == "w":
        wl = torch.zeros_like(wl)
    if drop_lo == "x":
        xl = torch.zeros_like(xl)
    hh = F.conv2d(xh, wh, b, stride=stride, padding=pad)
    cross = F.conv2d(xh, wl, None, stride=stride, padding=pad) + F.conv2d(xl, wh, None, stride=stride, padding=pad)
    return hh + cross * np.float32(1.0 / 2048.0)


def _inputs(L, t, x0, by):
    def one(s):
        if s[0] == "frame":
            return x0
        v = t[s[1]][:, : by[s[1]].cout]
        if s[0] == "blob":
            return v if s[2] is None else v[:, s[2]:s[3]]
        if s[0] == "up":
            return v.repeat_interleave(2, 2).repeat_interleave(2, 3)
        for _ in range(s[2]):
            v = F.max_pool2d(v, 5, 1, 2)
        return v
    return torch.cat([one(s) for s in L.src], 1), (one(L.res) if L.res else None)


def emulate(weights, frames, scale, nc, mode, drop_lo=None):
    """A forward pass with each mode's arithmetic, layer by layer on the previous layers' stored values -> name -> float32 [B,C,h,w]."""
    graph = lr.layer_graph(scale, nc)
    by = {L.name: L for L in graph}
    x0 = lr.stem_input(frames).float()
    t = {}
    with torch.no_grad():
        for L in graph:
            x, r = _inputs(L, t, x0, by)
            w, b = weights[L.name]
            W = torch.from_numpy(w).permute(0, 3, 1, 2).contiguous()
            z = _emul_conv(x, W, torch.from_numpy(b), L.stride, mode, drop_lo if drop_lo and drop_lo[0] == L.name else None)
            y = F.silu(z) if L.act else z
            if r is not None:
                y = y + r
            t[L.name] = _store(y, mode, L.act)
    return t


@pytest.fixture(scope="module")
def net():
    w = ys.synthetic_weights("s", 1, seed=3)
    frames = _frames(2, 96, 128, seed=5)
    return w, frames, {m: emulate(w, frames, "s", 1, m) for m in lr.MODES}


@pytest.mark.parametrize("mode", list(lr.MODES))
def test_honest_arithmetic_of_each_mode_passes_its_bounds(net, mode):
    w, frames, emu = net
    rep = lr.check_network(lr.DictSource(emu[mode]), w, frames, "s", 1, mode, label="emulated")
    print(rep.table())
    rep.assert_ok()
    assert max(r.K for r in rep.layers) == 4608
    # the constants are not vacuous: honest results use a small part of the per-element bound and of the rms ceiling
    assert max(r.worst for r in rep.layers) < 0.5 and max(r.rms / r.rho for r in rep.layers) < 0.5, rep.table()


def test_honest_arithmetic_of_each_mode_passes_with_composites(net):
    """Blobs kept on chip, checked through their consumer with the producer's bound carried through |W|."""
    w, frames, emu = net
    unobs = lr.unobservable_blobs("s", 1, "fp16", "throughput")
    assert "model.2.m.0.cv1" in unobs and "model.3" in unobs and "model.0" in unobs
    rep = lr.check_network(lr.DictSource(emu["fp16"]), w, frames, "s", 1, "fp16", unobservable=unobs)
    rep.assert_ok()
    assert sum(r.family == "unobservable" for r in rep.layers) == len(unobs)
    assert all(r.carried for r in rep.layers if r.name in ("model.2.cv1", "model.2.cv2", "model.4.cv1", "model.22.cv2.0.2", "model.22.cv3.2.2"))


# ---- scales m and l: widths that are no power of two (48 ... 576), C2f depths [2, 4, 4, 2] and [3, 6, 6, 3] ---------------------------------
WIDE = [("m", "fp32"), ("m", "fp16"), ("l", "fp32"), ("l", "f16x3"), ("l", "fp16")]  # f16x3 does not exist at m (ys.split_capable)
WIDE_MAX_K = {"m": 9 * 576, "l": 9 * 512}


@pytest.fixture(scope="module")
def wide():
    """scale -> (weights, frames, mode -> emulated tensors).  Seed 0: the draw the m and l gain tables were calibrated for."""
    frames = _frames(2, 64, 96, seed=5)
    out = {}
    for scale in ("m", "l"):
        w = ys.synthetic_weights(scale, 1, seed=0)
        out[scale] = (w, frames, {m: emulate(w, frames, scale, 1, m) for s, m in WIDE if s == scale})
    return out


@pytest.mark.parametrize("scale,mode", WIDE)
def test_honest_arithmetic_passes_its_bounds_at_scales_m_and_l(wide, scale, mode):
    """The MODES constants were derived at scale s; they hold unchanged through four (m) and six (l) chained bottlenecks."""
    w, frames, emu = wide[scale]
    rep = lr.check_network(lr.DictSource(emu[mode]), w, frames, scale, 1, mode, label="emulated")
    print(rep.table())
    rep.assert_ok()
    assert len(rep.layers) == len(ys.conv_table(scale, 1))
    assert max(r.K for r in rep.layers) == WIDE_MAX_K[scale] and (scale, WIDE_MAX_K[scale]) in (("m", 5184), ("l", 4608))
    # fp16 through six residual adds uses half of its per-element bound (0.50 measured at l): 0.6 here, 0.5 stays for scale s above
    assert max(r.worst for r in rep.layers) < 0.6 and max(r.rms / r.rho for r in rep.layers) < 0.5, rep.table()
    # the synthetic draw is calibrated: nothing near the fp16 range (uncalibrated, scale l reaches 3.5e5 behind model.15)
    assert max(float(t.abs().max()) for t in emu[mode].values()) < 64.0


@pytest.mark.parametrize("scale,dtype", [("m", "fp16"), ("l", "fp16"), ("l", "f16x3")])
def test_honest_arithmetic_passes_with_composites_at_scales_m_and_l(wide, scale, dtype):
    w, frames, emu = wide[scale]
    unobs = lr.unobservable_blobs(scale, 1, dtype, "throughput")
    rep = lr.check_network(lr.DictSource(emu[dtype]), w, frames, scale, 1, dtype, unobservable=unobs)
    rep.assert_ok()
    assert sum(r.family == "unobservable" for r in rep.layers) == len(unobs)
    # a chain of shared-scratch bottlenecks: every m.i.cv2 but the last reads a composite, and so does the box tail
    assert all(r.carried for r in rep.layers if r.name in ("model.4.m.0.cv2", "model.6.m.2.cv2", "model.22.cv2.1.2"))


@pytest.mark.parametrize("mode,c0,blk", [("fp32", 92, 4), ("fp16", 64, 32)])
def test_skipped_k_block_in_the_last_chunk_of_a_96_channel_3x3_fails(wide, mode, c0, blk):
    """model.4.m.2.cv1 at m: 96 input channels are three 32-channel chunks (fp32) or one and a half 64-channel chunks (fp16)."""
    name = "model.4.m.2.cv1"

    def plant(y, L, x, r, W, b):
        assert L.cin == 96 and L.cout == 96 and L.k == 3
        xs = x.clone()
        xs[:, c0:c0 + blk] = 0
        yy = F.silu(F.conv2d(xs, W, b, stride=L.stride, padding=L.k // 2))
        y[1, 80:96, :4, :4] = yy[1, 80:96, :4, :4].float()  # one tile: the last 16 couts x 4 x 4 pixels of frame 1
        return y
    net = wide["m"]
    _failing(*_planted(net, mode, name, plant, scale="m")[:1], net[0], net[1], mode, name, scale="m")


@pytest.mark.parametrize("mode", ["fp32", "fp16"])
def test_two_output_channels_swapped_in_the_last_partial_cout_tile_fails(wide, mode):
    """model.8.m.0.cv1 at m: 288 couts are four and a half 64-cout tiles (stored as 320) and nine 32-cout tiles; channels 256 ... 287 are the last."""
    name = "model.8.m.0.cv1"

    def plant(y, L, *_):
        assert L.cout == 288
        y[:, [259, 284]] = y[:, [284, 259]]
        return y
    net = wide["m"]
    _failing(*_planted(net, mode, name, plant, scale="m")[:1], net[0], net[1], mode, name, scale="m")


@pytest.mark.parametrize("mode", ["fp32", "fp16"])
def test_residual_not_added_on_the_fourth_bottleneck_fails(wide, mode):
    """model.6.m.3.cv2 at m: the residual is the third bottleneck's output, at channel offset 4 * 192 of a 6c-wide concat buffer."""
    name = "model.6.m.3.cv2"

    def plant(y, L, x, r, W, b):
        assert r is not None and L.cin == 192
        return (y.double() - r).float()
    net = wide["m"]
    _failing(*_planted(net, mode, name, plant, scale="m")[:1], net[0], net[1], mode, name, scale="m")


# ---- planted defects --------------------------------------------------------------------------------------------------------------------
def _ref_layer(emu, w, frames, name, x_override=None, scale="s"):
    graph = lr.layer_graph(scale, 1)
    by = {L.name: L for L in graph}
    L = by[name]
    x, r = _inputs(L, {k: v.double() for k, v in emu.items()}, lr.stem_input(frames), by)
    if x_override is not None:
        x = x_override(x)
    W, b = lr._w(w, name)
    return L, x, r, W, b


def _failing(emu, w, frames, mode, name, scale="s"):
    rep = lr.check_network(lr.DictSource(emu), w, frames, scale, 1, mode)
    bad = {r.name: r for r in rep.failed}
    assert name in bad, rep.table()
    assert rep.failed[0].name == name, rep.table()  # found where it is: no layer before it fails (its consumers read the defective tensor)
    return bad[name]


def _planted(net, mode, name, f, scale="s"):
    w, frames, emu = net
    t = dict(emu[mode])
    t[name] = f(t[name].clone(), *_ref_layer(t, w, frames, name, scale=scale))
    return t, w, frames


@pytest.mark.parametrize("mode,name", [("fp32", "model.2.m.0.cv1"), ("f16x3", "model.6.m.1.cv2"), ("fp16", "model.22.cv2.0.0")])
def test_bottom_halo_row_from_the_next_frame_fails(net, mode, name):
    def plant(y, L, x, r, W, b):
        xp = F.pad(x, (1, 1, 1, 1))
        xp[0, :, -1, 1:-1] = x[1, :, 0, :]  # frame 0's bottom padding row read from frame 1's top row
        z = F.conv2d(xp, W, b)[0:1, :, -1:, :]
        yy = F.silu(z) if L.act else z
        if r is not None:
            yy = yy + r[0:1, :, -1:, :]
        y[0:1, :, -1:, :] = yy.float()
        return y
    _failing(*_planted(net, mode, name, plant)[:1], net[0], net[1], mode, name)


@pytest.mark.parametrize("mode,name,blk", [("fp32", "model.4.m.0.cv1", 4), ("f16x3", "model.7", 16), ("fp16", "model.15.cv1", 32),
                                           ("f16x3", "model.9.cv2", 32)])
def test_one_skipped_k_block_in_one_tile_fails(net, mode, name, blk):
    def plant(y, L, x, r, W, b):
        xs = x.clone()
        xs[:, 32:32 + blk] = 0  # one K block of input channels missing ...
        z = F.conv2d(xs, W, b, stride=L.stride, padding=L.k // 2)
        yy = F.silu(z) if L.act else z
        if r is not None:
            yy = yy + r
        y[1, 16:32, :4, :4] = yy[1, 16:32, :4, :4].float()  # ... for one tile (16 channels x 4 x 4 pixels of frame 1)
        return y
    _failing(*_planted(net, mode, name, plant)[:1], net[0], net[1], mode, name)


@pytest.mark.parametrize("mode,name", [("fp32", "model.5"), ("f16x3", "model.12.cv2"), ("fp16", "model.2.cv1")])
def test_two_output_channels_swapped_in_one_group_fails(net, mode, name):
    def plant(y, *_):
        y[:, [19, 22]] = y[:, [22, 19]]
        return y
    _failing(*_planted(net, mode, name, plant)[:1], net[0], net[1], mode, name)


@pytest.mark.parametrize("mode,name", [("fp32", "model.8.m.0.cv2"), ("f16x3", "model.4.m.1.cv2"), ("fp16", "model.2.m.0.cv2")])
def test_residual_not_added_fails(net, mode, name):
    def plant(y, L, x, r, W, b):
        return (y.double() - r).float()
    _failing(*_planted(net, mode, name, plant)[:1], net[0], net[1], mode, name)


@pytest.mark.parametrize("mode,name", [("fp32", "model.1"), ("f16x3", "model.22.cv3.1.1"), ("fp16", "model.16")])
def test_last_ragged_pixel_tile_left_stale_fails(net, mode, name):
    def plant(y, *_):
        B, C, h, w = y.shape
        flat = y.permute(0, 2, 3, 1).reshape(B * h * w, C)
        n = (B * h * w) % 16 or 7  # the pixels of the last, partial 16-pixel tile ...
        flat[-n:] = flat[:n].clone()  # ... hold another tile's values (a previous call's)
        return flat.reshape(B, h, w, C).permute(0, 3, 1, 2).contiguous()
    _failing(*_planted(net, mode, name, plant)[:1], net[0], net[1], mode, name)


@pytest.mark.parametrize("name", ["model.1", "model.4.m.0.cv1", "model.21.cv2"])
def test_silu_with_1e_4_relative_error_fails_in_fp32(net, name):
    def plant(y, L, x, r, W, b):
        z = F.conv2d(x, W, b, stride=L.stride, padding=L.k // 2)
        yy = F.silu(z) * (1 + 1e-4)
        if r is not None:
            yy = yy + r
        return yy.float()
    _failing(*_planted(net, "fp32", name, plant)[:1], net[0], net[1], "fp32", name)


@pytest.mark.parametrize("name", ["model.1", "model.2.m.0.cv1", "model.6.cv1", "model.7", "model.9.cv2", "model.21.m.0.cv1", "model.22.cv3.2.1"])
@pytest.mark.parametrize("which", ["w", "x"])
def test_f16x3_lo_half_dropped_fails_the_rms_ceiling_by_10x(net, name, which):
    w, frames, emu = net
    t = dict(emu["f16x3"])
    bad = emulate_one(t, w, frames, name, which)
    t[name] = bad
    r = _failing(t, w, frames, "f16x3", name)
    assert r.rms >= 10 * r.rho, (name, which, r.rms / r.rho)


def emulate_one(t, w, frames, name, drop_lo):
    graph = lr.layer_graph("s", 1)
    by = {L.name: L for L in graph}
    L = by[name]
    x, r = _inputs(L, t, lr.stem_input(frames).float(), by)
    W = torch.from_numpy(w[name][0]).permute(0, 3, 1, 2).contiguous()
    z = _emul_conv(x, W, torch.from_numpy(w[name][1]), L.stride, "f16x3", drop_lo)
    y = F.silu(z) if L.act else z
    if r is not None:
        y = y + r
    return _store(y, "f16x3", L.act)


def test_padding_channels_must_be_zero(net):
    w, frames, emu = net
    t = dict(emu["fp32"])
    cls = t["model.22.cv3.0.2"]
    t["model.22.cv3.0.2"] = torch.cat([cls, torch.zeros((cls.shape[0], 7) + tuple(cls.shape[2:]))], 1)  # nc = 1 stored as cls_ld = 8
    lr.check_network(lr.DictSource(t), w, frames, "s", 1, "fp32").assert_ok()
    t["model.22.cv3.0.2"][1, 5, 0, 0] = 1e-30
    r = _failing(t, w, frames, "fp32", "model.22.cv3.0.2")
    assert not r.pad_ok


def test_unobservable_lists_follow_the_switches():
    shared = ["model.4.m.0.cv1", "model.6.m.0.cv1"]  # a C2f's bottlenecks share one m.i.cv1 scratch tensor: only the last survives the pass
    assert lr.unobservable_blobs("s", 1, "fp32", "throughput") == shared
    assert lr.unobservable_blobs("s", 1, "fp32", "latency") == shared
    off = {"WTK_NO_FUSED_FRONT": "1", "WTK_NO_FUSED_C2F": "1", "WTK_NO_FUSED_TAIL": "1", "WTK_NO_IGEMM_TAIL": "1"}
    for dt in ("fp16", "f16x3"):
        assert lr.unobservable_blobs("s", 1, dt, "throughput", off) == shared
    assert lr.unobservable_blobs("s", 1, "f16x3", "latency") == shared + ["model.0", "model.1"]
    assert "model.22.cv3.0.1" not in lr.unobservable_blobs("s", 80, "fp16", "throughput")
    assert lr.unobservable_blobs("n", 1, "fp16", "throughput") == shared + ["model.5"] + [f"model.22.cv2.{i}.1" for i in range(3)]
    # scales m and l: deeper C2f blocks (all bottlenecks of one C2f write ONE m.i.cv1 scratch tensor, Planner::c2f), a 64-wide box tower whose
    # last 1x1 is folded in the fp16 / f16x3 throughput plans (fuse_detect_tails), and at l in fp16 the implicit-GEMM tail on model.1 (128 couts,
    # stride 2) -> model.2.cv1 (128 -> 128), which fuse_strided_tails finds wherever it is (first seen on the GPU: model.1 read back stale and
    # failed with model.2.cv1 behind it until this list named it).  Nothing else: no 32 / 64 front, no one-bottleneck 32-wide C2f, class towers
    # 192 / 256 wide
    box = [f"model.22.cv2.{i}.1" for i in range(3)]
    tail = {("l", "fp16"): ["model.1"]}
    for scale, n in (("m", [2, 4, 4, 2]), ("l", [3, 6, 6, 3])):
        reps = zip(("model.2", "model.4", "model.6", "model.8", "model.12", "model.15", "model.18", "model.21"), n + [n[3]] * 4)
        shared = [f"{p}.m.{i}.cv1" for p, r in reps for i in range(r - 1)]
        assert len(shared) == sum(n) + 4 * n[3] - 8
        for plan in ("throughput", "latency"):
            assert lr.unobservable_blobs(scale, 1, "fp32", plan) == shared
        for dt in ("fp16",) + (("f16x3",) if ys.split_capable(scale) else ()):
            t = tail.get((scale, dt), [])
            assert lr.unobservable_blobs(scale, 1, dt, "throughput") == shared + t + box
            assert lr.unobservable_blobs(scale, 80, dt, "throughput") == shared + t + box
            assert lr.unobservable_blobs(scale, 1, dt, "throughput", off) == shared
            assert lr.unobservable_blobs(scale, 1, dt, "throughput", {"WTK_NO_HALO": "1"}) == shared + t  # (a strided 3x3 is an implicit GEMM anyway)
            assert lr.unobservable_blobs(scale, 1, dt, "throughput", {"WTK_NO_IGEMM_TAIL": "1"}) == shared + box
        if ys.split_capable(scale):
            assert lr.unobservable_blobs(scale, 1, "f16x3", "latency") == shared  # the front of a 64-wide stem is not the fused one
    assert ys.split_capable("l") and not ys.split_capable("m") and not ys.split_capable("x")
    assert [f"model.4.m.{i}.cv1" in lr.unobservable_blobs("m", 1, "fp32", "throughput") for i in range(4)] == [True, True, True, False]
    assert [f"model.6.m.{i}.cv1" in lr.unobservable_blobs("l", 1, "fp32", "throughput") for i in range(6)] == [True] * 5 + [False]
