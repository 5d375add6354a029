"""GPU: the ResMLP trainer (csrc/mlp_train.hip) beyond the notebook's shapes and batch 130 — everything the C ABI admits and tests/test_gpu_mlp_train.py
never ran: 0 blocks, 1 / 3 layers per block, a layer without ReLU / BatchNorm, widths 1, 17-ish (3, 33, 65, 127), 64 layers, batches up to the full 1024,
a handle larger than its call, populations larger than the number of CUs, per-model hyper-parameters, a caller's `active` mask.

  1  grad over harness/mlp_train_ref.SHAPE_CASES against the float64 restatement.  The bound is NOT torch float32 alone: it is 4 x the LARGER error of two
     honest fp32 runs of the same case, torch float32 (blocked sums) and the restatement in the device's own summation order (ascending-k fma chains, 8
     interleaved channel partials, 64 x 16 loss runs) — a sequential chain over 1024 samples is legitimately less accurate than a blocked sum.  Neither is
     the code under test.  Two metrics, both asserted: relative to the model's largest gradient, and per tensor (over the tensors whose true gradient is
     not identically zero), which a wrong column of a small tensor cannot hide under.  tests/test_mlp_train_ref.py asserts on the CPU that the cases are off
     every ReLU kink and that ten planted one-line defects each fail these bounds on a named case;
  2  a handle with max_batch 1024 called at 19, 1024, 19: both small calls equal a fresh max_batch-19 handle bit for bit (stale rows are masked);
  3  the optimizer step, teacher-forced, on the global-memory path, on the odd widths and at batch 1024;
  4  running statistics after one step at 1024;
  5  num_correct on targets built around the float64 prediction, so that the count lies strictly between 0 and B and no honest fp32 run can differ;
  6  test_epoch: loss, num_correct and predictions of EVERY batch (the partial one included), mse and l1;
  7  l1 at a residual of exactly 0, and num_correct at a distance of exactly 1;
  8  a population of 300 models;
  9  refusals at the exact boundary (65 layers, width 129) are in tests/test_gpu_mlp_train.py::test_refusals_name_the_limit already; 64 layers (tiny-in)
     and width 128 (wide-lds, wide) are admitted here."""
import functools

import numpy as np
import pytest
import torch

from harness import mlp_ref
from harness import mlp_train_ref as tr
from test_gpu_mlp_train import STEP_ULPS, _model, _teacher_forced_steps
from test_gpu_mlp_train import _dev as _to_dev
from wtracker_amd.training import LDS_STATE_FLOATS, HipMLPTrainer

pytestmark = pytest.mark.gpu
SHAPE_CASES = tr.SHAPE_CASES


def _dev(a):
    return _to_dev(np.array(a))  # (a copy: the harness hands its cases out read-only)


def _case(name_id):
    return next(c for c in SHAPE_CASES if tr.case_id(c) == name_id)


def _same_bits(a, b):
    return set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)


# ---------------------------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("i", range(len(SHAPE_CASES)), ids=[tr.case_id(c) for c in SHAPE_CASES])
def test_grad_matches_float64_within_four_times_the_larger_fp32_reference(hip_lib, i):
    name, arch, bn, batch, loss, seed = SHAPE_CASES[i]
    r = tr.case_refs(SHAPE_CASES[i])
    sd, acts, r64 = r["sd"], r["acts"], r["r64"]
    t = HipMLPTrainer(_model(sd, acts), loss_fn=loss, max_batch=batch)
    assert t.n_state == tr.state_floats(sd) and ("global" if t.n_state > LDS_STATE_FLOATS else "lds") == tr.SHAPE_PATH[name]
    Xd, yd = _dev(r["X"]), _dev(r["y"])
    Ld, gd = t.grad(Xd, yd)
    Ld2, gd2 = t.grad(Xd, yd)
    res = tr.check_step(r, Ld[0], gd[0])
    print(f"\n[mlp_train_shapes] grad {tr.case_id(SHAPE_CASES[i]):<26} {tr.SHAPE_PATH[name]:<6} max|g| {tr.max_grad(r64['grads']):9.3e}  model-wide: torch32 {r['torch32']['grad']:9.3e} "
          f"order32 {r['order32']['grad']:9.3e} device {res['grad'] * r['bounds']['grad']:9.3e} ratio {res['grad']:6.3f}  per tensor: torch32 {r['torch32']['tensor']:9.3e} "
          f"order32 {r['order32']['tensor']:9.3e} device {res['tensor'] * r['bounds']['tensor']:9.3e} ratio {res['tensor']:6.3f}  loss {float(r64['loss']):.6f} ratio {res['loss']:6.3f}")
    assert set(gd[0]) == set(r64["grads"])
    assert all(np.isfinite(v).all() for v in gd[0].values()) and np.isfinite(Ld[0])
    assert res["grad"] <= 1.0 and res["tensor"] <= 1.0 and res["loss"] <= 1.0, res
    assert Ld[0] == Ld2[0] and _same_bits(gd[0], gd2[0])  # the same call twice: the same bits
    before = t.state_dict(0)
    assert all(np.array_equal(before[k], np.asarray(sd[k]).astype(before[k].dtype)) for k in before), "grad must not touch the state"
    t.close()


# ---------------------------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("name,arch", [("notebook", tr.NOTEBOOK), ("odd", tr.ODD)])
def test_a_handle_larger_than_its_call_gives_the_bits_of_a_fitting_one(hip_lib, name, arch):
    """Rows 19 .. 1023 of every scratch buffer, left by the call at 1024, sit next to the 19 live rows of the third call."""
    sd, acts, X, y = tr.make_case(arch, 19, 301)
    _, _, Xbig, ybig = tr.make_case(arch, 1024, 302)
    big = HipMLPTrainer(_model(sd, acts), max_batch=1024)
    fit = HipMLPTrainer(_model(sd, acts), max_batch=19)
    want = fit.grad(_dev(X), _dev(y))
    first = big.grad(_dev(X), _dev(y))
    full = big.grad(_dev(Xbig), _dev(ybig))
    third = big.grad(_dev(X), _dev(y))
    assert np.isfinite(full[0]).all() and all(np.isfinite(v).all() for v in full[1][0].values())
    for got in (first, third):
        assert got[0][0] == want[0][0] and _same_bits(got[1][0], want[1][0])
    # ... and a step after them: the same state and running statistics
    (l_b, n_b), (l_f, n_f) = big.step(_dev(X), _dev(y)), fit.step(_dev(X), _dev(y))
    assert float(l_b[0]) == float(l_f[0]) and int(n_b[0]) == int(n_f[0]) and _same_bits(big.state_dict(0), fit.state_dict(0))
    big.close(), fit.close()


# ---------------------------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("opt", tr.OPTIMIZERS)
@pytest.mark.parametrize("case_name", ["wide-global-b19-mse", "odd-b19-mse"])
def test_step_teacher_forced_on_the_global_path_and_on_odd_widths(hip_lib, case_name, opt):
    """wide-global: parameters, moments and running statistics are updated in global memory.  Weight decay 1e-2: the longer formula of STEP_ULPS."""
    r = tr.case_refs(_case(case_name))
    lr, wd = 1e-3, 1e-2
    t = HipMLPTrainer(_model(r["sd"], r["acts"]), optimizer=opt, lr=lr, weight_decay=wd, max_batch=19)
    assert (t.n_state > LDS_STATE_FLOATS) == (case_name.startswith("wide-global"))
    worst = _teacher_forced_steps(t, r["sd"], r["acts"], _dev(r["X"]), _dev(r["y"]), opt, lr, wd)
    print(f"\n[mlp_train_shapes] step {case_name:<20} {opt:<8} worst {worst:.2f} ulp of max(|p|, |update|) (allowed {STEP_ULPS[opt]})")
    t.close()


def test_step_teacher_forced_at_the_full_batch(hip_lib):
    """This case found a defect.  With weight decay the gradient of one weight (-1.98752e-4) cancels against wd p (1.98730e-4); the kernel rounded wd p before
    adding, torch's grad.add(param, alpha=wd) is one fma, and Adam's m / (sqrt(v) + eps) at |g| ~ 2e-8 turned the extra rounding into 33 units in the last
    place of the parameter (allowed 15).  The kernel now computes fmaf(wd, p, g): worst 4."""
    r = tr.case_refs(_case("notebook-b1024-mse"))
    t = HipMLPTrainer(_model(r["sd"], r["acts"]), optimizer="adam", lr=1e-3, weight_decay=1e-2, max_batch=1024)
    worst = _teacher_forced_steps(t, r["sd"], r["acts"], _dev(r["X"]), _dev(r["y"]), "adam", 1e-3, 1e-2, steps=2)
    print(f"\n[mlp_train_shapes] step notebook-b1024-mse   adam     worst {worst:.2f} ulp of max(|p|, |update|) (allowed {STEP_ULPS['adam']})")
    t.close()


# ---------------------------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize("case_name", ["notebook-b1024-mse", "wide-b1024-l1"])
def test_running_statistics_after_a_step_at_the_full_batch(hip_lib, case_name):
    """The bound is built as in 1: 4 x the larger error of torch float32 and of the restatement in the device's order, relative to the largest statistic."""
    case = _case(case_name)
    r = tr.case_refs(case)
    sd, r64 = r["sd"], r["r64"]
    t = HipMLPTrainer(_model(sd, r["acts"]), loss_fn=case[4], max_batch=case[3])
    loss, _ = t.step(_dev(r["X"]), _dev(r["y"]))
    after = t.state_dict(0)
    err = tr.stats_error(after, r64["stats"])
    print(f"\n[mlp_train_shapes] running statistics {case_name}: bound / 4 {r['bounds']['stats'] / 4:.3e} device {err:.3e} ratio {err / r['bounds']['stats']:.3f}")
    assert err <= r["bounds"]["stats"]
    assert abs(float(loss[0]) - float(r64["loss"])) <= r["bounds"]["loss"]
    n = 0
    for k, v in r64["stats"].items():
        if k.endswith("num_batches_tracked"):
            assert after[k].dtype == np.int64 and int(after[k]) == int(v) == int(sd[k]) + 1
            n += 1
    assert n == len(tr.layer_table(sd, r["acts"])[0]) - 1
    t.close()


# ---------------------------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize("i", range(3), ids=[f"{c[0]}-n{c[2]}-bs{c[3]}" for c in tr.NC_CASES[:3]])
def test_num_correct_in_train_mode(hip_lib, i):
    """y = the float64 train-mode prediction of the batch + offsets of norm 0.2 .. 0.9 (about half) or 1.1 .. 3 (tests/test_mlp_train_ref.py: every distance
    is >= 64 x its fp32 / fp64 difference away from 1, both outcomes in every batch).  With several batches the epoch runs at lr = 0, weight_decay = 0 (sgd:
    p - 0 g = p), so every batch sees the initial parameters and its own batch statistics, as the restatement does."""
    _, arch, n, bs, _ = tr.NC_CASES[i]
    sd, acts, X, y, counts, _ = tr.nc_case(i, "train")
    sizes = [min(bs, n - b0) for b0 in range(0, n, bs)]
    Xd, yd = _dev(X), _dev(y)
    t = HipMLPTrainer(_model(sd, acts), optimizer="sgd", lr=0.0, weight_decay=0.0, max_batch=bs)
    _, nc = t.train_epoch(Xd, yd, None, batch_size=bs)
    got = nc[0].cpu().tolist()
    print(f"\n[mlp_train_shapes] num_correct train n {n} batch {bs}: device {got} restatement {counts} of {sizes}")
    assert got == counts and all(0 < c < b for c, b in zip(got, sizes))
    assert all(np.array_equal(v, np.asarray(sd[k]).astype(v.dtype)) for k, v in t.state_dict(0).items() if k in tr.trainable_keys(sd, acts))
    for bi, b0 in enumerate(range(0, n, bs)):  # ... and `step` on each batch, with the default optimizer on a fresh handle (the count is taken before the step)
        u = HipMLPTrainer(_model(sd, acts), max_batch=bs)
        _, n1 = u.step(Xd[b0:b0 + bs].contiguous(), yd[b0:b0 + bs].contiguous())
        assert int(n1[0]) == counts[bi]
        u.close()
    t.close()


@pytest.mark.parametrize("i", range(3), ids=[f"{c[0]}-n{c[2]}-bs{c[3]}" for c in tr.NC_CASES[:3]])
def test_num_correct_in_eval_mode(hip_lib, i):
    _, arch, n, bs, _ = tr.NC_CASES[i]
    sd, acts, X, y, counts, _ = tr.nc_case(i, "eval")
    sizes = [min(bs, n - b0) for b0 in range(0, n, bs)]
    t = HipMLPTrainer(_model(sd, acts), max_batch=bs)
    _, nc = t.test_epoch(_dev(X), _dev(y), batch_size=bs)
    got = nc[0].cpu().tolist()
    print(f"\n[mlp_train_shapes] num_correct eval  n {n} batch {bs}: device {got} restatement {counts} of {sizes}")
    assert got == counts and all(0 < c < b for c, b in zip(got, sizes))
    t.close()


# ---------------------------------------------------------------------------------------------------------------------------------- 6
@pytest.mark.parametrize("loss", ["mse", "l1"])
@pytest.mark.parametrize("i", [0, 3], ids=["notebook", "odd"])
def test_test_epoch_on_every_batch(hip_lib, i, loss):
    """45 rows at batch_size 16: batches of 16, 16 and 13, each against eval_step in float64.

    Tolerances.  Every prediction is within tol = mlp_ref.tolerance (8 x the deviation of a sequential fp32 forward, from the reference alone) of the
    float64 one: p = p64 + e with |e| <= tol.  Propagated through the mean over the batch's B x out entries, with d = p64 - y:
      l1   | mean|d + e| - mean|d| | <= mean|e| <= tol;
      mse  | mean (d + e)^2 - mean d^2 | = | mean (2 d e + e^2) | <= 2 max|d| tol + tol^2, plus half a unit in the last place of the loss for writing it
           as a float32."""
    _, arch, n, bs, _ = tr.NC_CASES[i]
    sd, acts, X, y, counts, _ = tr.nc_case(i, "eval")
    t = HipMLPTrainer(_model(sd, acts), loss_fn=loss, max_batch=bs)
    lossd, nc, pred = t.test_epoch(_dev(X), _dev(y), batch_size=bs, return_pred=True)
    lossd, nc, pred = lossd[0].cpu().numpy(), nc[0].cpu().tolist(), pred[0].cpu().numpy()
    tol = mlp_ref.tolerance(sd, acts, X)
    assert tuple(lossd.shape) == (3,) and [min(bs, n - b0) for b0 in range(0, n, bs)] == [16, 16, 13]
    for bi, b0 in enumerate(range(0, n, bs)):
        e = tr.eval_step(sd, acts, X[b0:b0 + bs], y[b0:b0 + bs], loss)
        d = np.abs(e["pred"] - y[b0:b0 + bs].astype(np.float64)).max()
        L64 = float(e["loss"])
        loss_tol = tol if loss == "l1" else 2.0 * d * tol + tol * tol + 0.5 * float(np.spacing(np.float32(L64)))
        perr = float(np.abs(pred[b0:b0 + bs] - e["pred"]).max())
        print(f"\n[mlp_train_shapes] test_epoch {tr.NC_CASES[i][0]:<8} {loss:<4} batch {bi} ({len(e['pred'])} rows): pred err {perr:.3e} tol {tol:.3e}  loss {L64:.6f} err {abs(float(lossd[bi]) - L64):.3e} "
              f"tol {loss_tol:.3e}  num_correct {nc[bi]} / {e['num_correct']}")
        assert perr <= tol
        assert abs(float(lossd[bi]) - L64) <= loss_tol
        assert nc[bi] == e["num_correct"] == counts[bi] and 0 < nc[bi] < len(e["pred"])
    t.close()


# ---------------------------------------------------------------------------------------------------------------------------------- 7
def test_l1_at_a_residual_of_exactly_zero_and_num_correct_at_a_distance_of_exactly_one(hip_lib):
    """harness.make_l1_zero_case: the prediction is the (dyadic) output bias exactly, a third of the residuals each are 0, -1 and +1, n = 64.  The kernel writes
    0 at a residual of 0, as torch does (asserted on the CPU): the output bias gradient is (n_pos - n_neg) / n, which float32 holds exactly.  A sample at
    distance exactly 1 is NOT correct (`<`)."""
    sd, acts, X, y, cls = tr.make_l1_zero_case()
    r = tr.refs_of(sd, acts, X, y, "l1")
    want = tr.l1_zero_bias_gradient(cls).astype(np.float32)
    t = HipMLPTrainer(_model(sd, acts), loss_fn="l1", max_batch=len(X))
    Ld, gd = t.grad(_dev(X), _dev(y))
    got = gd[0]["model.output.bias"]
    res = tr.check_step(r, Ld[0], gd[0])
    print(f"\n[mlp_train_shapes] l1 at 0: output bias gradient {got.tolist()} want {want.tolist()}; other gradients: model-wide ratio {res['grad']:.3f} per tensor {res['tensor']:.3f} loss {res['loss']:.3f}")
    assert (np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want))).all()
    assert res["failed"] == [], res
    assert all(not gd[0][k].any() for k in gd[0] if not k.startswith("model.output"))  # W_out = 0: nothing flows back, exactly
    _, nc = t.step(_dev(X), _dev(y))
    dist = np.sqrt(((r["r64"]["pred"] - y) ** 2).sum(axis=1))
    assert int(nc[0]) == r["r64"]["num_correct"] == int((dist == 0).sum()) and int((dist == 1).sum()) > 0
    t.close()


# ---------------------------------------------------------------------------------------------------------------------------------- 8
E_POP = 300  # more workgroups than the 256 CUs; scratch (5 + 2 x 4 + 1) x 16 x 128 + 4 x 128 floats = 114 KiB per model


@functools.lru_cache(maxsize=None)
def _population():
    """300 TINY models on 45 rows.  Models 0, 150 and 299 share initial state, lr, weight_decay and order; model 1 differs from them in weight_decay only,
    model 2 in lr only; every other model has its own state, order and hyper-parameters."""
    sd0, acts, X, y = tr.make_case(tr.TINY, 45, 401)
    models = [mlp_ref.random_rmlp(**tr.TINY, seed=1000 + e)[0] for e in range(E_POP)]
    rng = np.random.default_rng(402)
    lr = 10.0 ** rng.uniform(-4, -2, size=E_POP)
    wd = 10.0 ** rng.uniform(-6, -2, size=E_POP)
    g = torch.Generator().manual_seed(403)
    orders = torch.stack([torch.stack([torch.randperm(45, generator=g) for _ in range(E_POP)]) for _ in range(2)]).to(torch.int32)  # [epoch][model][n]
    for e in (0, 1, 2, 150, 299):
        models[e], lr[e], wd[e] = sd0, 1e-3, 1e-3
        orders[:, e] = orders[:, 0]
    wd[1], lr[2] = 1e-2, 3e-3
    return acts, X, y, models, lr, wd, orders


def _run(acts, X, y, models, lr, wd, orders, active=None):
    """Two epochs: (per-epoch losses [2][E, 3], per-epoch num_correct, states after each epoch [2][E, n_state], moments and steps at the end)."""
    t = HipMLPTrainer([_model(m, acts) for m in models], lr=lr, weight_decay=wd, max_batch=16)
    Xd, yd = _dev(X), _dev(y)
    losses, ncs, states = [], [], []
    for ep in range(2):
        l, c = t.train_epoch(Xd, yd, orders[ep].cuda(), batch_size=16, active=active)
        losses.append(l.cpu().numpy()), ncs.append(c.cpu().numpy()), states.append(t._get(0)[0].copy())
    (m, steps), (v, _) = t._get(2), t._get(3)
    t.close()
    return losses, ncs, states, m, v, steps


@functools.lru_cache(maxsize=None)
def _population_run():
    return _run(*_population())


@functools.lru_cache(maxsize=None)
def _solo(e):
    acts, X, y, models, lr, wd, orders = _population()
    return _run(acts, X, y, [models[e]], lr[e:e + 1], wd[e:e + 1], orders[:, e:e + 1])


def test_a_population_larger_than_the_device_keeps_every_models_bits(hip_lib):
    losses, ncs, states, m, v, steps = _population_run()
    assert steps.tolist() == [6] * E_POP and all(np.isfinite(l).all() for l in losses)
    for e in (0, 150, 299, 1, 2, 77):
        sl, sn, ss, sm, sv, _ = _solo(e)
        for ep in range(2):
            assert np.array_equal(losses[ep][e], sl[ep][0]) and np.array_equal(ncs[ep][e], sn[ep][0]) and np.array_equal(states[ep][e], ss[ep][0]), (e, ep)
        assert np.array_equal(m[e], sm[0]) and np.array_equal(v[e], sv[0])
    for e in (150, 299):  # the same model at three places of the grid
        assert all(np.array_equal(losses[ep][e], losses[ep][0]) and np.array_equal(states[ep][e], states[ep][0]) for ep in range(2))
    # per-model weight_decay (model 1) and lr (model 2): everything else is model 0's, the bits are not
    for e in (1, 2):
        assert np.array_equal(losses[0][e][0], losses[0][0][0])  # the first batch is computed before any step
        assert not np.array_equal(states[0][e], states[0][0]) and not np.array_equal(losses[1][e], losses[1][0])
    assert not np.array_equal(states[1][1], states[1][2])


def test_a_callers_active_mask_freezes_a_model_and_leaves_its_neighbours_alone(hip_lib):
    acts, X, y, models, lr, wd, orders = _population()
    active = torch.tensor([1, 0] * (E_POP // 2), dtype=torch.int32).cuda()
    t = HipMLPTrainer([_model(mo, acts) for mo in models], lr=lr, weight_decay=wd, max_batch=16)
    init, m0, v0 = t._get(0)[0].copy(), t._get(2)[0].copy(), t._get(3)[0].copy()
    loss, nc = t.train_epoch(_dev(X), _dev(y), orders[0].cuda(), batch_size=16, active=active)
    loss, nc, after = loss.cpu().numpy(), nc.cpu().numpy(), t._get(0)[0]
    (m1, steps), (v1, _) = t._get(2), t._get(3)
    off = np.arange(E_POP) % 2 == 1
    assert np.array_equal(after[off], init[off]) and np.array_equal(m1[off], m0[off]) and np.array_equal(v1[off], v0[off])
    assert not m1[off].any() and steps[off].tolist() == [0] * (E_POP // 2) and steps[~off].tolist() == [3] * (E_POP // 2)
    assert np.isnan(loss[off]).all() and not nc[off].any() and np.isfinite(loss[~off]).all()
    assert active.cpu().tolist() == [1, 0] * (E_POP // 2)  # train_epoch reads the mask, it does not write it
    for e in (0, 2, 150):  # active models between inactive ones: their solo runs' first epoch
        sl, sn, ss, _, _, _ = _solo(e)
        assert np.array_equal(loss[e], sl[0][0]) and np.array_equal(nc[e], sn[0][0]) and np.array_equal(after[e], ss[0][0]), e
    full = _population_run()
    assert np.array_equal(loss[~off], full[0][0][~off]) and np.array_equal(after[~off], full[2][0][~off])
    t.close()


def test_a_shared_order_is_the_same_order_for_every_model(hip_lib):
    acts, X, y, models, lr, wd, orders = _population()
    one = orders[0, 7].clone()
    out = []
    for o in (one, one.unsqueeze(0).repeat(E_POP, 1)):
        t = HipMLPTrainer([_model(mo, acts) for mo in models], lr=lr, weight_decay=wd, max_batch=16)
        l, c = t.train_epoch(_dev(X), _dev(y), o.cuda(), batch_size=16)
        out.append((l.cpu().numpy(), c.cpu().numpy(), t._get(0)[0].copy()))
        t.close()
    assert all(np.array_equal(a, b) for a, b in zip(*out)) and np.isfinite(out[0][0]).all()
    assert not np.array_equal(out[0][0], _population_run()[0][0])  # (and it is not the per-model orders' result)
