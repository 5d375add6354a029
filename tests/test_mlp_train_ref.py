"""CPU: the numpy restatement of one RMLP training step (harness/mlp_train_ref.py) pinned two ways — against torch autograd in float64, and against
the real reference's RMLP + MLPTrainer.train_batch / test_batch run in float64 (tests/golden/mlp_train.npz, written by
tests/golden/make_mlp_train_golden.py).  In float64 both must agree to rounding: errors are relative to the model's LARGEST gradient / parameter
(the gradient of a Linear bias in front of a BatchNorm is exactly 0, so a per-tensor relative error means nothing).

Also here: the GPU gradient cases (tests/test_gpu_mlp_train.py), built off the ReLU kinks by clear_relu_kinks, have ZERO pre-ReLU values inside the guard band."""
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


def test_train_test_split_is_a_seeded_partition():
    from wtracker_amd.training import train_test_split

    a, b = train_test_split(614, 0.8, seed=42)
    a2, b2 = train_test_split(614, 0.8, seed=42)
    assert len(a) == 491 and len(b) == 123 and torch.equal(a, a2) and torch.equal(b, b2)
    assert sorted(torch.cat([a, b]).tolist()) == list(range(614))
    assert not torch.equal(a, train_test_split(614, 0.8, seed=43)[0])
    z = np.load(GOLDEN)  # the split the golden script recorded for the "it learns" test is this one
    assert np.array_equal(z["learn::train_idx"], a.numpy()) and np.array_equal(z["learn::test_idx"], b.numpy())
