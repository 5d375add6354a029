"""CPU: the device's BatchNorm fold and blob layout (csrc/mlp_fold.h) through their host twin, wtk_mlp_fold_state_host — the same function the fold
kernel runs, compiled for the host — against resmlp.fold_state_dict and the padded packing restated in tests/harness/mlp_population_ref.py.  Bit for bit:
the population replay promises the bits of the per-model path, whose parameters are folded by resmlp._fold."""
import ctypes as C

import numpy as np
import pytest

from harness import mlp_population_ref as pr
from harness import mlp_ref
from harness import mlp_train_ref as tr
from wtracker_amd import hip

ARCHS = {**{name: mlp_ref.arch_args(name) for name in mlp_ref.ARCHS}, "odd": tr.ODD}


def _layers(sd, acts):
    rows, n_blocks, per_block = pr.rows(sd, acts)
    arr = (hip._MlpTrainLayer * len(rows))()
    for i, (_, b, relu, k, n) in enumerate(rows):
        arr[i] = hip._MlpTrainLayer(k, n, int(relu), int(b is not None))
    return arr, n_blocks, per_block


def _fold(hip_lib, sd, acts, fill=np.nan):
    """wtk_mlp_fold_state_host into a buffer prefilled with `fill`, so that a float the function does not write shows."""
    arr, n_blocks, per_block = _layers(sd, acts)
    F = hip_lib.wtk_mlp_folded_floats(arr, len(arr), n_blocks, per_block)
    assert F > 0
    blob = np.full(F, fill, np.float32)
    state = pr.pack_state(sd, acts)
    assert hip_lib.wtk_mlp_fold_state_host(arr, len(arr), n_blocks, per_block, hip._ptr(state), hip._ptr(blob)) == 0, hip_lib.wtk_last_error()
    return blob


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("batch_norm", [True, False], ids=["bn", "no-bn"])
@pytest.mark.parametrize("name", list(ARCHS))
def test_fold_equals_resmlp_fold_bit_for_bit(hip_lib, name, batch_norm):
    sd, acts = mlp_ref.random_rmlp(**ARCHS[name], batch_norm=batch_norm, seed=500 + list(ARCHS).index(name))
    assert bool(pr.bn_prefixes(sd)) == batch_norm
    want = pr.fold_blob(sd, acts)
    got = _fold(hip_lib, sd, acts)
    assert got.size == want.size == mlp_ref.blob_floats(hip_layers(sd, acts))
    assert np.array_equal(_bits(got), _bits(want))
    assert hip.mlp_fold_state_host(*_layers(sd, acts), pr.pack_state(sd, acts)).tobytes() == want.tobytes()  # the Python wrapper of the same call


def hip_layers(sd, acts):
    from wtracker_amd import resmlp

    return resmlp.fold_state_dict(sd, [], [], list(acts)).layers


@pytest.mark.parametrize("name", ["one-slice-edge", "odd", "none-in-block"])
def test_fold_at_extreme_running_variances(hip_lib, name):
    """running_var 0 (s = gamma / sqrt(1e-5)), 1e-12 (below the epsilon's last place) and 1e6."""
    sd, acts = mlp_ref.random_rmlp(**ARCHS[name], seed=520)
    sd = pr.with_variances(sd, (0.0, 1e-12, 1e6))
    assert all(np.asarray(sd[p + ".running_var"])[0] == 0.0 for p in pr.bn_prefixes(sd))
    got, want = _fold(hip_lib, sd, acts), pr.fold_blob(sd, acts)
    assert np.isfinite(want).all()
    assert np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("name", ["wide-lds", "odd"])
def test_fold_bias_is_a_product_and_a_sum_not_a_fused_multiply_add(hip_lib, name):
    """beta = -float32((b - mean) s): what is left is the product's rounding, which a fused multiply-add does not make.  The case is only worth something
    where the two differ, so that is asserted of the restatement first."""
    sd, acts = mlp_ref.random_rmlp(**ARCHS[name], seed=530)
    sd = pr.with_cancelling_beta(sd)
    want_layers = hip_layers(sd, acts)
    fused = pr.fused_biases(sd)
    rows, _, _ = pr.rows(sd, acts)
    differ = sum(int((_bits(fused[b]) != _bits(want_layers[i][1])).sum()) for i, (_, b, _, _, _) in enumerate(rows) if b)
    print(f"\n[mlp_fold] {name}: {differ} folded biases differ between two roundings and a fused multiply-add")
    assert differ > 0
    assert np.array_equal(_bits(_fold(hip_lib, sd, acts)), _bits(pr.pack(want_layers)))


@pytest.mark.parametrize("name", list(ARCHS))
def test_blob_size_and_zero_padding(hip_lib, name):
    sd, acts = mlp_ref.random_rmlp(**ARCHS[name], seed=540)
    layers = hip_layers(sd, acts)
    arr, n_blocks, per_block = _layers(sd, acts)
    assert hip_lib.wtk_mlp_folded_floats(arr, len(arr), n_blocks, per_block) == mlp_ref.blob_floats(layers)
    assert hip.mlp_folded_floats(arr, n_blocks, per_block) == mlp_ref.blob_floats(layers)
    if name in mlp_ref.EXPECTED_BLOB:
        assert mlp_ref.blob_floats(layers) == mlp_ref.EXPECTED_BLOB[name]
    got, mask = _fold(hip_lib, sd, acts, fill=np.nan), pr.padding_mask(layers)
    assert mask.size == got.size and (_bits(got)[mask] == 0).all()  # +0.0, not -0.0, not left unwritten
    assert np.isfinite(got).all()


def test_blob_size_refuses_what_mlp_create_refuses(hip_lib):
    L = hip._MlpTrainLayer
    ok = (L * 4)(L(28, 40, 1, 1), L(40, 24, 1, 1), L(24, 40, 1, 1), L(40, 2, 0, 0))
    assert hip_lib.wtk_mlp_folded_floats(ok, 4, 1, 2) == 48 * 28 + 48 + 32 * 40 + 32 + 48 * 24 + 48 + 16 * 40 + 16
    no_return = (L * 4)(L(28, 40, 1, 1), L(40, 24, 1, 1), L(24, 36, 1, 1), L(40, 2, 0, 0))  # the block ends 36 wide, the residual is 40
    assert hip_lib.wtk_mlp_folded_floats(no_return, 4, 1, 2) == -1
    assert hip_lib.wtk_mlp_folded_floats(ok, 4, 2, 1) == -1  # 24 does not chain into a block that reads the residual width
    assert hip_lib.wtk_mlp_folded_floats(ok, 4, 1, 3) == -1  # n_layers != 2 + n_blocks * layers_per_block
    wide = (L * 2)(L(28, 129, 1, 0), L(129, 2, 0, 0))
    assert hip_lib.wtk_mlp_folded_floats(wide, 2, 0, 0) == -1
    assert hip_lib.wtk_mlp_folded_floats(None, 2, 0, 0) == -1
    blob = np.zeros(16, np.float32)
    assert hip_lib.wtk_mlp_fold_state_host(no_return, 4, 1, 2, hip._ptr(blob), hip._ptr(blob)) != 0
    assert b"residual dim" in hip_lib.wtk_last_error()


def test_state_names_and_missing_frames_are_refused_without_a_device():
    from wtracker_amd.replay import mlp_clip_bound, population_frames
    from wtracker_amd.training import STATE_SLOTS, FitResult, state_slot

    assert STATE_SLOTS == {"current": 0, "best": 1, "scored": 4}
    assert [state_slot(w) for w in ("current", "best", "scored", False, True)] == [0, 1, 4, 0, 1]
    for bad in ("Best", "score", 2, None):
        with pytest.raises(ValueError, match="unknown state"):
            state_slot(bad)
    assert population_frames([0, -2, -9], (9,)) == ([0, -2, -9], [9])
    for xi, yi in ((None, [9]), ([0, -2], None), ([], [9]), ([0], [])):
        with pytest.raises(ValueError, match="input_frames and pred_frames"):
            population_frames(xi, yi)
    assert FitResult(3).closed_loop == []

    class TC:
        px_per_mm, frames_per_sec = 90, 60

    assert mlp_clip_bound(TC, 0.9, [9]) == float(np.float32(0.9 * (90 / 60) * 9))
