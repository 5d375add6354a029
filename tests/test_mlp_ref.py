"""CPU: the ResMLP reference harness (tests/harness/mlp_ref.py) has teeth, and resmlp.fold_state_dict folds every layer kind RMLP builds.

The GPU suites (test_gpu_mlp_shapes.py, test_gpu_mlp.py) hold the device kernel to `mlp_ref.tolerance`.  Here the same tolerance is shown to
pass honest fp32 arithmetic in two summation orders and to fail four planted defects, for every architecture of the matrix."""
import os

import numpy as np
import pytest

from harness import mlp_ref
from harness.mlp_ref import Defect
from wtracker_amd import resmlp
from wtracker_amd.hip import WtkError

N_SAMPLES = 257


@pytest.fixture(scope="module")
def nets():
    """name -> (sd, acts, x, float64 truth, tolerance); built once, never modified."""
    out = {}
    for name in mlp_ref.ARCHS:
        sd, acts, x = mlp_ref.matrix_network(name, N_SAMPLES)
        y64 = mlp_ref.forward64(sd, acts, x)
        tol = mlp_ref.tolerance(sd, acts, x)
        y64.setflags(write=False)
        out[name] = (sd, acts, x, y64, tol)
    return out


def _dev(y, y64):
    return float(np.abs(y.astype(np.float64) - y64).max())


@pytest.mark.parametrize("name", list(mlp_ref.ARCHS))
def test_honest_fp32_orders_pass_the_tolerance(nets, name):
    sd, acts, x, y64, tol = nets[name]
    assert 0 < tol < 1e-2 * np.abs(y64).max()  # the yardstick itself is an fp32-sized number, not a loose one
    assert _dev(mlp_ref.forward32_seq(sd, acts, x), y64) <= tol
    d4 = _dev(mlp_ref.forward32_group4(sd, acts, x), y64)
    print(f"[mlp_ref] {name}: tol {tol:.3e}, grouped-by-four fp32 at {d4 / tol:.3f} of it")
    assert d4 <= tol


@pytest.mark.parametrize("name", list(mlp_ref.ARCHS))
def test_planted_defects_fail_the_tolerance(nets, name):
    sd, acts, x, y64, tol = nets[name]
    n_layers = len(acts)
    mid = n_layers // 2  # an MLPLayer in the middle of the stack (the input layer of the two-layer network)
    defects = {"last four k dropped": Defect(drop_last_k_of=mid), "bias row shifted": Defect(shift_bias_of=mid),
               "13 mantissa bits": Defect(cut_bits=13)}
    n_blocks = mlp_ref.ARCHS[name]["n_blocks"]
    if n_blocks:
        defects["residual add skipped"] = Defect(skip_residual_of=n_blocks // 2)
    for what, d in defects.items():
        dev = _dev(mlp_ref.forward32_seq(sd, acts, x, d), y64)
        print(f"[mlp_ref] {name}: {what}: {dev / tol:.1f} x tolerance")
        assert dev > tol, (name, what, dev, tol)


def test_blob_formula_and_paths_of_the_matrix(nets):
    for name, (sd, acts, *_rest) in nets.items():
        m = resmlp.fold_state_dict(sd, [0], [1], activations=acts)
        assert mlp_ref.param_path(m.layers) == mlp_ref.ARCHS[name]["path"], name
        if name in mlp_ref.EXPECTED_BLOB:
            assert mlp_ref.blob_floats(m.layers) == mlp_ref.EXPECTED_BLOB[name], name
        assert len(m.layers) == 2 + m.n_blocks * m.layers_per_block <= mlp_ref.MAX_LAYERS
        if mlp_ref.ARCHS[name]["path"] == "lds" and len(m.layers) < mlp_ref.MAX_LAYERS:
            z, added = mlp_ref.with_zero_block(m.layers, layers_per_block=m.layers_per_block or 4, until_global=True)
            assert mlp_ref.param_path(z) == "global" and len(z) == len(m.layers) + added * (m.layers_per_block or 4) <= mlp_ref.MAX_LAYERS
            x, y64 = nets[name][2], nets[name][3]
            got = mlp_ref.forward_folded64(z, m.n_blocks + added, m.layers_per_block or 4, x)
            np.testing.assert_array_equal(got, mlp_ref.forward_folded64(m.layers, m.n_blocks, m.layers_per_block, x))  # h + 0 = h


# -------------------------------------------------------------------------------------------------------------------------------------
# fold_state_dict against the unfolded float64 network
def _fold_check(sd, acts, x, activations):
    m = resmlp.fold_state_dict(sd, [0], [1], activations=activations)
    assert [bool(r) for _, _, r in m.layers] == [a == "relu" for a in acts] + [False]
    y = mlp_ref.forward_folded64(m.layers, m.n_blocks, m.layers_per_block, x)
    y64 = mlp_ref.forward64(sd, acts, x)
    tol = mlp_ref.tolerance(sd, acts, x)
    assert np.abs(y - y64).max() <= tol, (np.abs(y - y64).max(), tol)
    return m


def test_fold_bn_relu_layers(nets):
    for name in ("odd-pingpong", "hourglass", "no-blocks"):
        sd, acts, x, *_ = nets[name]
        m = _fold_check(sd, acts, x, None)
        assert (m.n_blocks, m.layers_per_block) == (mlp_ref.ARCHS[name]["n_blocks"], len(mlp_ref.ARCHS[name]["block_dims"]) if mlp_ref.ARCHS[name]["n_blocks"] else 0)


def test_fold_infers_no_relu_from_a_layer_without_batchnorm(nets):
    sd, acts, x, *_ = nets["none-in-block"]
    assert acts == ["none"] + ["none", "relu"] * 2 and "model.blocks.1.sequence.0.mlp_layer.1.running_mean" not in sd
    _fold_check(sd, acts, x, None)
    _fold_check(sd, acts, x, acts)


def test_fold_without_batchnorm_needs_and_uses_activations():
    sd, acts = mlp_ref.random_rmlp(28, 40, [24, 40], ["relu", "relu"], 2, 2, batch_norm=False, seed=31)
    assert not any(".mlp_layer.1." in k for k in sd)
    x = np.random.default_rng(2).normal(0, 6, size=(64, 28)).astype(np.float32)
    _fold_check(sd, acts, x, acts)
    # state dict alone: no BatchNorm reads as "no ReLU" (documented in resmlp._fold), which is a different network
    m = resmlp.fold_state_dict(sd, [0], [1])
    assert not any(r for _, _, r in m.layers)
    assert np.abs(mlp_ref.forward_folded64(m.layers, 2, 2, x) - mlp_ref.forward64(sd, acts, x)).max() > mlp_ref.tolerance(sd, acts, x)


@pytest.mark.parametrize("tag", ["100ms", "200ms"])
def test_fold_shipped_fixtures(golden_dir, tag):
    path = os.path.join(golden_dir, f"resmlp_{tag}.npz")
    sd, acts = mlp_ref.fixture_network(path)
    z = np.load(path)
    m = _fold_check(sd, acts, z["x"], None)
    assert (m.n_blocks, m.layers_per_block) == (resmlp.load_npz(path).n_blocks, 4)
    # the fixture's recorded outputs of the real reference (torch, fp32) are honest fp32 too
    y64 = mlp_ref.forward64(sd, acts, z["x"])
    assert np.abs(z["y_batch"] - y64).max() <= mlp_ref.tolerance(sd, acts, z["x"])


def test_fold_refuses_identity_input_and_wrong_activation_count(nets):
    sd, acts, *_ = nets["odd-pingpong"]
    no_input = {k: v for k, v in sd.items() if not k.startswith("model.input.")}
    with pytest.raises(WtkError, match="input layer"):
        resmlp.fold_state_dict(no_input, [0], [1])
    with pytest.raises(WtkError, match="activations"):
        resmlp.fold_state_dict(sd, [0], [1], activations=acts[:-1])
    with pytest.raises(WtkError, match="activations"):
        resmlp.fold_state_dict(sd, [0], [1], activations=acts + ["relu"])
