"""GPU: mlp_kernel at every shape wtk_mlp_create admits, on both parameter paths, against the unfolded float64 network.

The shipped predictors (28 -> 40 / 60, four ReLU+BatchNorm layers per block, blobs of 8 320 and 26 352 floats) only ever ran the LDS path with
one 64-deep K slice.  The matrix (harness/mlp_ref.py: ARCHS) adds the global-memory path, the second K slice and its cut-off, every
layers_per_block parity, shrinking and growing widths, a layer without ReLU, 0 and 62 blocks, 1 and 16 input frames, three predicted frames.

Three checks per network: (a) device vs forward64 within mlp_ref.tolerance (8 x the deviation of a sequential fp32 forward: a number from the
reference alone); (b) ragged batches reproduce the same rows bit for bit; (c) the same layers plus all-zero residual blocks — which change no
value (h + 0 = h) but push the blob over the LDS limit — return bit-equal outputs, i.e. the LDS and the global path agree on identical
arithmetic.  If the global loop of mlp_layer<false> skipped its first k step, (c) and both global rows of (a) would fail."""
import os

import numpy as np
import pytest
import torch

from harness import mlp_ref
from wtracker_amd import hip, resmlp
from wtracker_amd.hip import WtkError

pytestmark = pytest.mark.gpu
BATCHES = (1, 15, 16, 17, 255, 256)  # one wave = 16 samples: below, at and above a wave, and the last partial / full block of 256


def _net(name):
    sd, acts, x = mlp_ref.matrix_network(name)
    n_in = mlp_ref.ARCHS[name]["in_dim"] // 4
    m = resmlp.fold_state_dict(sd, list(range(1 - n_in, 1)), list(range(1, 1 + mlp_ref.ARCHS[name]["out_dim"] // 2)), activations=acts)
    return sd, acts, x, m


@pytest.fixture(scope="module")
def nets():
    return {name: _net(name) for name in mlp_ref.ARCHS}


def _zero_block_handle(m):
    lpb = m.layers_per_block or 4  # a network without blocks leaves the block depth free
    z, added = mlp_ref.with_zero_block(m.layers, layers_per_block=lpb, until_global=True)
    assert mlp_ref.blob_floats(z) > mlp_ref.LDS_PARAM_FLOATS and len(z) <= mlp_ref.MAX_LAYERS
    return hip.HipMLP(z, m.n_blocks + added, lpb), len(z), mlp_ref.blob_floats(z)


@pytest.mark.parametrize("name", list(mlp_ref.ARCHS))
def test_forward_matches_float64_on_its_path_and_on_the_other(hip_lib, nets, name):
    sd, acts, x, m = nets[name]
    blob = mlp_ref.blob_floats(m.layers)
    path = "lds" if blob <= 32704 else "global"  # kMlpLdsParams: the matrix must not drift off the path it is there for
    assert path == mlp_ref.ARCHS[name]["path"], (name, blob)
    assert blob == mlp_ref.EXPECTED_BLOB.get(name, blob)
    assert x.shape[0] == 258 and not x[-1].any()
    y64 = mlp_ref.forward64(sd, acts, x)
    tol = mlp_ref.tolerance(sd, acts, x)
    g = hip.HipMLP(m.layers, m.n_blocks, m.layers_per_block)
    y = g.forward_host(x)
    assert y.shape == (258, mlp_ref.ARCHS[name]["out_dim"])
    rows = [mlp_ref.Row(name, path, len(m.layers), blob, float(np.abs(y - y64).max()), tol, float(np.abs(y64).max()))]
    bit_equal = None
    if path == "lds" and len(m.layers) < mlp_ref.MAX_LAYERS:  # the 64-layer network has no room for a zero block: float64 only
        gz, nz, bz = _zero_block_handle(m)
        yz = gz.forward_host(x)
        rows.append(mlp_ref.Row(name + " +0", "global", nz, bz, float(np.abs(yz - y64).max()), tol, float(np.abs(y64).max()),
                                note="bit-equal" if np.array_equal(yz, y) else "DIFFERS from the LDS path"))
        bit_equal = (yz, gz)
    print("\n" + mlp_ref.table(name, rows))
    assert np.isfinite(y).all()
    assert rows[0].dev <= tol, rows[0]
    for n in BATCHES:
        np.testing.assert_array_equal(g.forward_host(x[:n]), y[:n], err_msg=f"batch {n}")
    if bit_equal is not None:
        yz, gz = bit_equal
        np.testing.assert_array_equal(yz, y)
        for n in BATCHES:
            np.testing.assert_array_equal(gz.forward_host(x[:n]), y[:n], err_msg=f"zero block, batch {n}")
        gz.close()
    g.close()


@pytest.mark.parametrize("tag", ["100ms", "200ms"])
def test_shipped_predictors_agree_bit_for_bit_across_paths(hip_lib, golden_dir, tag):
    path = os.path.join(golden_dir, f"resmlp_{tag}.npz")
    z = np.load(path)
    m = resmlp.load_npz(path)
    assert mlp_ref.param_path(m.layers) == "lds"
    zl, added = mlp_ref.with_zero_block(m.layers, layers_per_block=m.layers_per_block)
    assert added == 1 and mlp_ref.blob_floats(zl) - mlp_ref.blob_floats(m.layers) > 40000 and mlp_ref.param_path(zl) == "global"
    g = hip.HipMLP(m.layers, m.n_blocks, m.layers_per_block)
    gz = hip.HipMLP(zl, m.n_blocks + 1, m.layers_per_block)
    y, yz = g.forward_host(z["x"]), gz.forward_host(z["x"])
    np.testing.assert_allclose(yz, z["y_batch"], rtol=1e-5, atol=2e-4)  # SURVEY.md §8 a2, as test_gpu_mlp.py
    np.testing.assert_array_equal(yz, y)
    np.testing.assert_array_equal(gz.forward_host(np.zeros((1, 28), np.float32)), g.forward_host(np.zeros((1, 28), np.float32)))


@pytest.mark.parametrize("name,n_in", [("hourglass", 16), ("hourglass-lds", 16), ("tiny-in", 1)])
def test_predict_track_gather(hip_lib, nets, name, n_in):
    sd, acts, _, m = nets[name]
    assert len(m.input_frames) == n_in and m.in_dim == 4 * n_in
    rng = np.random.default_rng(3)
    n = 400
    track = np.cumsum(rng.normal(0, 0.6, size=(n, 4)), axis=0).astype(np.float32)
    track[:, 2:] = 14 + rng.normal(0, 0.5, size=(n, 2))
    track[:, :2] += 300
    track[124] = np.nan   # a missed detection poisons every sample that gathers it
    track[250, 2] = np.inf  # and so does a box that is not finite
    anchors = np.arange(-20, n + 6, 3, dtype=np.int32)  # from before frame 0 to past the end
    t_dev, a_dev = torch.from_numpy(track).cuda(), torch.from_numpy(anchors).cuda()
    pred = torch.full((len(anchors), m.out_dim), 7.0, dtype=torch.float32, device="cuda")
    valid = torch.full((len(anchors),), -1, dtype=torch.int32, device="cuda")
    g = hip.HipMLP(m.layers, m.n_blocks, m.layers_per_block)
    g.predict_track(t_dev, n, a_dev, len(anchors), m.input_frames, pred, valid, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    pred, valid = pred.cpu().numpy(), valid.cpu().numpy()
    want_valid, X = [], []
    for t in anchors:
        idx = t + np.asarray(m.input_frames)
        ok = bool((idx >= 0).all() and (idx < n).all() and np.isfinite(track[np.clip(idx, 0, n - 1)]).all())
        want_valid.append(int(ok))
        if ok:
            b = track[idx].copy()  # float32 arithmetic, as the controller's
            b[:, 0] -= b[0, 0]
            b[:, 1] -= b[0, 1]
            X.append(b.reshape(-1))
    want_valid, X = np.asarray(want_valid), np.stack(X)
    np.testing.assert_array_equal(valid, want_valid)
    assert want_valid.sum() > 10 and (want_valid == 0).sum() > 3 * n_in // 4 + 3
    y64 = mlp_ref.forward64(sd, acts, X)
    tol = mlp_ref.tolerance(sd, acts, X)
    got = pred[want_valid == 1]
    row = mlp_ref.Row(f"{name} track", mlp_ref.param_path(m.layers), len(m.layers), mlp_ref.blob_floats(m.layers), float(np.abs(got - y64).max()), tol,
                      float(np.abs(y64).max()))
    print("\n" + mlp_ref.table(f"predict_track n_in={n_in}", [row]))
    assert row.dev <= tol, row
    assert (pred[want_valid == 0] == 0).all()
    # the gather feeds the kernel exactly what the host rule builds: same rows through forward_host, bit for bit
    np.testing.assert_array_equal(got, g.forward_host(X))


def _layers(dims, rng=None):
    """[(W, b, relu)] for consecutive (in, out) pairs."""
    rng = rng or np.random.default_rng(0)
    return [(rng.normal(size=(o, i)).astype(np.float32) * 0.1, np.zeros(o, np.float32), j < len(dims) - 1) for j, (i, o) in enumerate(dims)]


def test_create_rejects_what_the_kernel_cannot_run(hip_lib):
    ok = hip.HipMLP(_layers([(28, 16)] + [(16, 16)] * 62 + [(16, 2)]), 62, 1)  # 64 layers: admitted
    ok.close()
    with pytest.raises(WtkError, match="too many layers"):
        hip.HipMLP(_layers([(28, 16)] + [(16, 16)] * 63 + [(16, 2)]), 63, 1)
    with pytest.raises(WtkError, match="dim out of range"):
        hip.HipMLP(_layers([(28, 129), (129, 2)]), 0, 0)
    with pytest.raises(WtkError, match="dim out of range"):
        hip.HipMLP(_layers([(129, 40), (40, 2)]), 0, 0)
    with pytest.raises(WtkError, match="do not chain"):
        hip.HipMLP(_layers([(28, 40), (40, 24), (32, 40), (40, 2)]), 1, 2)
    with pytest.raises(WtkError, match="do not chain"):
        hip.HipMLP(_layers([(28, 40), (40, 24), (24, 24), (24, 2)]), 1, 2)  # the output layer reads the residual stream (40), not the block
    with pytest.raises(WtkError, match="residual dim"):
        hip.HipMLP(_layers([(28, 40), (40, 24), (24, 32), (40, 2)]), 1, 2)
    with pytest.raises(WtkError, match="n_layers"):
        hip.HipMLP(_layers([(28, 40), (40, 40), (40, 40), (40, 2)]), 1, 3)
    with pytest.raises(WtkError, match="n_layers"):
        hip.HipMLP(_layers([(28, 40), (40, 40), (40, 2)]), 0, 4)


def test_predict_track_rejects_a_gather_that_does_not_fit_the_model(hip_lib):
    track = torch.zeros((50, 4), dtype=torch.float32, device="cuda")
    anchors = torch.arange(20, 30, dtype=torch.int32, device="cuda")
    for in_dim, frames in ((28, list(range(-5, 1))), (28, list(range(-7, 1))), (68, list(range(-16, 1)))):  # 6 or 8 frames for 7; 17 frames
        g = hip.HipMLP(_layers([(in_dim, 16), (16, 2)]), 0, 0)
        pred = torch.full((10, 2), 7.0, dtype=torch.float32, device="cuda")
        valid = torch.full((10,), -1, dtype=torch.int32, device="cuda")
        with pytest.raises(WtkError, match="n_in"):
            g.predict_track(track, 50, anchors, 10, frames, pred, valid)
        torch.cuda.synchronize()
        assert (pred == 7.0).all() and (valid == -1).all()  # nothing ran
        g.close()
