"""CPU: the numpy restatement of one RMLP training step (harness/mlp_train_ref.py) pinned two ways — against torch autograd in float64, and against
the real reference's RMLP + MLPTrainer.train_batch / test_batch run in float64 (tests/golden/mlp_train.npz, written by
tests/golden/make_mlp_train_golden.py).  In float64 both must agree to rounding: errors are relative to the model's LARGEST gradient / parameter
(the gradient of a Linear bias in front of a BatchNorm is exactly 0, so a per-tensor relative error means nothing).

Also here: the GPU gradient cases (tests/test_gpu_mlp_train.py) and shape cases (tests/test_gpu_mlp_train_shapes.py), built off the ReLU kinks by
clear_relu_kinks, have ZERO pre-ReLU values inside the guard band; the other input conditions of the shape tests; and a list of planted one-line defects,
each of which must fail the bound the GPU tests use on a named case."""
import os

import numpy as np
import pytest
import torch

from harness import mlp_ref
from harness import mlp_train_ref as tr

RTOL64 = 1e-10  # float64 rounding through ~20 layers, relative to the model's largest gradient or parameter


def _cases():
    yield "tiny", tr.TINY, True, 17
    yield "notebook", tr.NOTEBOOK, True, 33
    yield "notebook-no-bn", tr.NOTEBOOK, False, 17
    yield "none-in-block", mlp_ref.arch_args("none-in-block"), True, 19


@pytest.mark.parametrize("loss", ["mse", "l1"])
@pytest.mark.parametrize("name,arch,bn,batch", list(_cases()))
def test_step_matches_torch_autograd_in_float64(name, arch, bn, batch, loss):
    sd, acts, X, y = tr.make_case(arch, batch, seed=3, batch_norm=bn)
    r = tr.train_forward_backward(sd, acts, X, y, loss, np.float64)
    L, grads, T = tr.torch_train_step(sd, acts, X, y, loss, torch.float64)
    assert abs(float(r["loss"]) - L) <= RTOL64 * abs(L)
    assert set(grads) == set(r["grads"]) == set(tr.trainable_keys(sd, acts))
    assert tr.grad_error(r["grads"], grads) <= RTOL64
    assert bool(r["stats"]) == bn
    for k, v in r["stats"].items():
        np.testing.assert_allclose(v, T[k].numpy(), rtol=1e-12, atol=1e-12, err_msg=k)
    pred = tr.torch_forward(T, acts, torch.tensor(X).double(), True).detach().numpy()  # (a second train-mode pass: same batch, same prediction)
    assert r["num_correct"] == tr.num_correct(pred, y.astype(np.float64))


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("opt", tr.OPTIMIZERS)
def test_optimizer_steps_match_torch_in_float64(opt, wd):
    rng = np.random.default_rng(5)
    p0 = rng.normal(0, 1, size=(7, 5))
    p_t = torch.tensor(p0.copy(), requires_grad=True)
    o = tr.torch_optimizer(opt, [p_t], 1e-3, wd)
    p, state = p0.copy(), {}
    for _ in range(3):
        g = rng.normal(0, 1, size=p0.shape) * 10.0 ** rng.integers(-6, 1)
        p_t.grad = torch.tensor(g.copy())
        o.step()
        p = tr.optimizer_step(opt, p, g, state, 1e-3, wd)
        np.testing.assert_allclose(p, p_t.detach().numpy(), rtol=1e-13, atol=1e-15)


def test_eval_step_is_the_eval_mode_forward():
    sd, acts, X, y = tr.make_case(tr.NOTEBOOK, 21, seed=4)
    r = tr.eval_step(sd, acts, X, y, "mse")
    T = tr.torch_tensors(sd, acts, torch.float64)
    pred = tr.torch_forward(T, acts, torch.tensor(X).double(), False).detach().numpy()
    np.testing.assert_allclose(r["pred"], pred, rtol=1e-12, atol=1e-12)
    assert abs(float(r["loss"]) - float(((pred - y) ** 2).mean())) <= 1e-12 * float(r["loss"])


# ---------------------------------------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mlp_train.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.mark.parametrize("opt", tr.OPTIMIZERS)
def test_three_steps_match_the_real_reference_in_float64(golden, opt):
    """RMLP + MLPTrainer.train_batch in float64, three steps: losses, num_correct, the first step's gradients, the state after every step; then test_batch."""
    z = golden
    acts = [str(a) for a in z["acts"]]
    sd = {k[len("init::"):]: z[k] for k in z.files if k.startswith("init::")}
    X, y = z["X"], z["y"]
    lr, wd, loss = float(z["lr"]), float(z["weight_decay"]), str(z["loss"])
    keys = tr.trainable_keys(sd, acts)
    states = {k: {} for k in keys}
    for step in range(3):
        r = tr.train_forward_backward(sd, acts, X, y, loss, np.float64)
        assert abs(float(r["loss"]) - float(z[f"{opt}::loss"][step])) <= RTOL64 * abs(float(r["loss"]))
        assert r["num_correct"] == int(z[f"{opt}::num_correct"][step])
        if step == 0:
            ref = {k: z[f"grad::{k}"] for k in keys}
            assert tr.grad_error(r["grads"], ref) <= RTOL64
        new = dict(sd)
        for k in keys:
            new[k] = tr.optimizer_step(opt, np.asarray(sd[k], np.float64), r["grads"][k], states[k], lr, wd)
        new.update(r["stats"])
        top = max(float(np.abs(v).max()) for v in new.values())
        for k, v in new.items():
            want = z[f"{opt}::state{step}::{k}"]
            assert float(np.abs(np.asarray(v, np.float64) - want).max()) <= RTOL64 * top, (opt, step, k)
        sd = new
    e = tr.eval_step(sd, acts, X, y, loss)
    assert abs(float(e["loss"]) - float(z[f"{opt}::test_loss"])) <= RTOL64 * abs(float(e["loss"]))
    assert e["num_correct"] == int(z[f"{opt}::test_num_correct"])


# ---------------------------------------------------------------------------------------------------------------------------------
def test_gradient_cases_leave_the_guard_band_empty():
    """The GPU gradient test masks nothing: its recorded cases must leave no pre-ReLU value of the float64 run within 64 x the float32 / float64 difference."""
    for name, arch, bn, batch, loss, seed in tr.GRAD_CASES:
        inside, band = tr.guard_band(*tr.make_case(arch, batch, seed, bn, clear_kinks=True, loss=loss), loss)
        assert inside == 0, (name, batch, seed, inside, band)


def test_shape_cases_leave_the_guard_band_empty_and_sit_on_their_parameter_path():
    """tests/test_gpu_mlp_train_shapes.py masks nothing either.  The path is the TRAINER's (floats of the unfolded state against LDS_STATE_FLOATS)."""
    from wtracker_amd.training import LDS_STATE_FLOATS

    assert tr.LDS_STATE_FLOATS == LDS_STATE_FLOATS
    assert {c[0] for c in tr.SHAPE_CASES} >= set(mlp_ref.ARCHS) and len({tr.case_id(c) for c in tr.SHAPE_CASES}) == len(tr.SHAPE_CASES)
    floats = {}
    for case in tr.SHAPE_CASES:
        r = tr.case_refs(case)
        inside, band = tr.guard_band(r["sd"], r["acts"], r["X"], r["y"], case[4])
        assert inside == 0, (tr.case_id(case), inside, band)
        floats[case[0]] = n = tr.state_floats(r["sd"])
        assert ("global" if n > LDS_STATE_FLOATS else "lds") == tr.SHAPE_PATH[case[0]], (case[0], n)
    assert (floats["wide-global"], floats["wide"], floats["hourglass"], floats["notebook"]) == (38530, 72578, 35630, 35488)


def test_device_order_sums_are_the_kernels_orders():
    """Values on which the order of an fp32 sum shows.  chan_sums: sample s goes to part s % 8, the parts are added in the order 0 .. 7."""
    a = np.zeros((16, 1), np.float32)
    a[0], a[8], a[1], a[9] = 2.0 ** 24, 1.0, 1.0, 1.0  # part 0 = 2^24 + 1 -> 2^24, part 1 = 2, total 2^24 + 2; one sequential chain gives 2^24
    assert float(tr._chan_sum_device(a)[0]) == 2.0 ** 24 + 2.0
    s = np.float32(0)
    for v in a[:, 0]:
        s = np.float32(s + v)
    assert float(s) == 2.0 ** 24
    e = np.zeros((32, 1), np.float32)
    e[0], e[1], e[16], e[17] = 2.0 ** 24, 1.0, 1.0, 1.0  # loss: run 0 = 2^24 + 1 -> 2^24, run 1 = 2
    assert float(tr._loss_sum_device(e)) == 2.0 ** 24 + 2.0
    # the product chain: ascending k, one rounding per step (an fma): 2^24 + 1 * 1 -> 2^24, then - 2^24 -> 0; the exact sum is 1
    A = np.array([[2.0 ** 12, 1.0, -(2.0 ** 12)]], np.float32)
    Bt = np.array([[2.0 ** 12, 1.0, 2.0 ** 12]], np.float32)
    assert float(tr._fma_chain(A, Bt)[0, 0]) == 0.0 and float((A.astype(np.float64) @ Bt.astype(np.float64).T)[0, 0]) == 1.0
    rng = np.random.default_rng(0)
    A, Bt = rng.normal(size=(5, 37)).astype(np.float32), rng.normal(size=(7, 37)).astype(np.float32)
    assert float(np.abs(tr._fma_chain(A, Bt) - A.astype(np.float64) @ Bt.astype(np.float64).T).max()) < 37 * 2.0 ** -24 * 10


def test_device_order_restatement_is_an_honest_fp32_run():
    """The restatement in the device's order is the same step: in float32 it lands where float32 lands (within 64 x half a unit in the last place per
    gradient, relative to the model's largest; torch float32 sits at 1e-7 .. 3e-6 on the same cases), and switching the order on changes no float64 figure."""
    for case in tr.SHAPE_CASES[:11]:
        r = tr.case_refs(case)
        assert r["order32"]["grad"] <= 64 * 2.0 ** -24 * 16, (tr.case_id(case), r["order32"])
        assert set(r["rdev"]["grads"]) == set(r["r64"]["grads"]) and r["rdev"]["num_correct"] == r["r64"]["num_correct"]


# (defect, the case that catches it, the check of the GPU test that fails).  "tensor" is the per-tensor bound: a wrong last column of the input layer's dW
# can hide under the model-wide metric where the output layer's gradients dominate.
PLANTED = [
    ("dw_drop_last_sample", "no-blocks-b19-mse", "grad"), ("dw_drop_last_sample", "notebook-b1023-mse", "grad"),
    ("dw_drop_last_col", "odd-b19-mse", "tensor"), ("dw_drop_last_col", "notebook-b257-mse", "tensor"), ("dw_drop_last_col", "notebook-b17-mse", "tensor"),
    ("dx_drop_k_tail", "odd-b49-l1", "grad"), ("dx_drop_k_tail", "notebook-b513-mse", "grad"),
    ("biased_running_var", "notebook-b1024-mse", "stats"), ("biased_running_var", "wide-b1024-l1", "stats"),
    ("no_residual_grad", "one-slice-edge-b19-mse", "grad"), ("no_residual_grad", "odd-pingpong-b19-mse", "grad"),
    ("relu_mask_pre_bn", "wide-global-b19-mse", "grad"), ("bn_no_dbeta", "two-slices-b19-mse", "grad"),
    ("mean_tile_rounded_b", "hourglass-lds-b19-mse", "grad"), ("mean_tile_rounded_b", "notebook-b1023-mse", "grad"),
    ("l1_sign0_is_1", "l1-zero", "bias"), ("num_correct_le", "l1-zero", "num_correct"),
]


def test_every_defect_is_planted_somewhere():
    assert {d for d, _, _ in PLANTED} == set(tr.DEFECTS)


@pytest.mark.parametrize("defect,case_name,check", PLANTED, ids=[f"{d}@{c}" for d, c, _ in PLANTED])
def test_planted_defect_fails_the_gpu_tests_bound(defect, case_name, check):
    """The defect goes into the fp32 restatement in the device's order (what a device with that defect would compute); the result is judged by
    check_step, the function the GPU tests assert with."""
    if case_name == "l1-zero":
        sd, acts, X, y, cls = tr.make_l1_zero_case()
        want = tr.l1_zero_bias_gradient(cls).astype(np.float32)
        good = tr.train_forward_backward(sd, acts, X, y, "l1", np.float32, device_order=True)
        bad = tr.train_forward_backward(sd, acts, X, y, "l1", np.float32, device_order=True, defect=defect)
        r64 = tr.train_forward_backward(sd, acts, X, y, "l1", np.float64)
        assert np.array_equal(good["grads"]["model.output.bias"], want) and good["num_correct"] == r64["num_correct"]
        if check == "bias":
            assert (np.abs(bad["grads"]["model.output.bias"] - want) > np.spacing(np.abs(want))).any()
        else:
            assert bad["num_correct"] != r64["num_correct"]
        return
    case = next(c for c in tr.SHAPE_CASES + tr.GRAD_CASES if tr.case_id(c) == case_name)
    r = tr.case_refs(case)
    good = tr.check_step(r, r["rdev"]["loss"], r["rdev"]["grads"], r["rdev"]["stats"] or None, r["rdev"]["num_correct"])
    assert good["failed"] == [], (case_name, good)
    bad = tr.train_forward_backward(r["sd"], r["acts"], r["X"], r["y"], r["loss"], np.float32, device_order=True, defect=defect)
    res = tr.check_step(r, bad["loss"], bad["grads"], bad["stats"] or None, bad["num_correct"])
    print(f"\n[mlp_train_ref] {defect} @ {case_name}: error / bound {({k: round(v, 2) for k, v in res.items() if k != 'failed'})} failed {res['failed']}")
    assert check in res["failed"], (defect, case_name, res)


def test_l1_zero_case_and_torch_agree_that_sign_of_zero_is_zero():
    """A third of the entries each: residual exactly 0, -1, +1, in float32 and float64; distances exactly 0, 1 and sqrt 2 all occur; torch's L1Loss writes
    0 at a residual of 0, so its output bias gradient is (n_pos - n_neg) / n exactly, and non-zero in both columns (the check means something)."""
    sd, acts, X, y, cls = tr.make_l1_zero_case()
    want = tr.l1_zero_bias_gradient(cls)
    assert sorted(np.bincount(cls.ravel()).tolist()) == [21, 21, 22] and (want != 0).all()
    for dtype, tdt in ((np.float32, torch.float32), (np.float64, torch.float64)):
        r = tr.train_forward_backward(sd, acts, X, y, "l1", dtype)
        resid = r["pred"] - y.astype(dtype)
        assert np.array_equal(resid, np.where(cls == 1, -1.0, np.where(cls == 2, 1.0, 0.0)))
        _, g, _ = tr.torch_train_step(sd, acts, X, y, "l1", tdt)
        assert np.array_equal(g["model.output.bias"], want.astype(dtype)) and np.array_equal(r["grads"]["model.output.bias"], want.astype(dtype))
        dist = np.sqrt((resid ** 2).sum(axis=1))
        assert {0.0, 1.0} < set(dist.tolist()) and len(set(dist.tolist())) == 3
        assert r["num_correct"] == int((dist == 0).sum()) > 0 and int((dist == 1).sum()) > 0


@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("i", range(len(tr.NC_CASES)), ids=[f"{c[0]}-n{c[2]}-bs{c[3]}" for c in tr.NC_CASES])
def test_num_correct_cases_are_decided_and_mixed(i, mode):
    """Input conditions of the num_correct tests: every sample's distance is at least 64 x its own float32 / float64 difference away from 1.0 (no honest fp32
    run can count it differently), and in every batch some samples are correct and some are not."""
    _, arch, n, bs, _ = tr.NC_CASES[i]
    sd, acts, X, y, counts, margin = tr.nc_case(i, mode)
    assert margin >= 64.0, margin
    sizes = [min(bs, n - b0) for b0 in range(0, n, bs)]
    assert len(counts) == len(sizes) and all(0 < c < b for c, b in zip(counts, sizes)), (counts, sizes)
    if mode == "train" and bs == n:
        assert tr.train_forward_backward(sd, acts, X, y, "mse")["num_correct"] == counts[0]
    if mode == "eval":
        assert [tr.eval_step(sd, acts, X[b0:b0 + bs], y[b0:b0 + bs])["num_correct"] for b0 in range(0, n, bs)] == counts


def test_train_test_split_is_a_seeded_partition():
    from wtracker_amd.training import train_test_split

    a, b = train_test_split(614, 0.8, seed=42)
    a2, b2 = train_test_split(614, 0.8, seed=42)
    assert len(a) == 491 and len(b) == 123 and torch.equal(a, a2) and torch.equal(b, b2)
    assert sorted(torch.cat([a, b]).tolist()) == list(range(614))
    assert not torch.equal(a, train_test_split(614, 0.8, seed=43)[0])
    z = np.load(GOLDEN)  # the split the golden script recorded for the "it learns" test is this one
    assert np.array_equal(z["learn::train_idx"], a.numpy()) and np.array_equal(z["learn::test_idx"], b.numpy())
