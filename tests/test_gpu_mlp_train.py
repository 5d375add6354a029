"""GPU: the ResMLP trainer (csrc/mlp_train.hip, wtracker_amd.training.HipMLPTrainer) — one workgroup per model.

fp32 training of this network is chaotic (torch float32 against torch float64 from the same numbers differs by 7.5e-2 in the loss after
60 Adam steps, and by a full lr in a parameter after ONE step, because a Linear bias in front of a BatchNorm has a true gradient of 0 whose fp32 rounding
noise Adam normalises into a step).  So nothing here follows a trajectory against another implementation:
  1  grad: loss and every gradient of ONE batch against the float64 restatement, within 4 x the error torch float32 shows on the same case, relative to
     the model's largest gradient (never per tensor); the cases are built off every ReLU kink on the CPU (harness/mlp_train_ref.clear_relu_kinks;
     tests/test_mlp_train_ref.py asserts that no pre-ReLU value is inside the guard band), nothing is masked here;
  2  step: teacher-forced — the DEVICE's gradient and moments go into the real torch.optim optimizer on a CPU copy of the device's parameters, and the
     two updates agree within a few units in the last place;
  3  running statistics after a step against the float64 restatement;
  4  train_epoch == repeated step, bit for bit, with a shuffled order and a partial last batch; a last batch of one sample is refused;
  5  a model's bits do not depend on E, its index, its neighbours or the run;
  6  LDS path == global path (zero residual blocks push the state over the LDS limit);
  7  eval_epoch against wtk_mlp_forward on the folded model, and the early-stopping state against a host replay of training.py:119-128;
  8  it learns: the final validation loss over 8 shuffle seeds lies in the (widened) range of the real MLPTrainer's on the same data and initial state;
  9  refusals."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from harness import mlp_ref
from harness import mlp_train_ref as tr
from wtracker_amd import hip, resmlp
from wtracker_amd.hip import WtkError
from wtracker_amd.training import LDS_STATE_FLOATS, FitResult, HipMLPTrainer

pytestmark = pytest.mark.gpu
GRAD_CASES, WIDE = tr.GRAD_CASES, tr.WIDE


def _model(sd, acts):
    return dict(sd, activations=list(acts))


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda", dtype)


@functools.lru_cache(maxsize=None)
def _grad_case(i):
    name, arch, bn, batch, loss, seed = GRAD_CASES[i]
    sd, acts, X, y = tr.make_case(arch, batch, seed, bn, clear_kinks=True, loss=loss)
    r64 = tr.train_forward_backward(sd, acts, X, y, loss, np.float64)
    L32, g32, T32 = tr.torch_train_step(sd, acts, X, y, loss, torch.float32)
    return sd, acts, X, y, r64, L32, g32, T32


@pytest.mark.parametrize("i", range(len(GRAD_CASES)), ids=[f"{c[0]}-b{c[3]}-{c[4]}" for c in GRAD_CASES])
def test_grad_matches_float64_within_four_times_torch_float32(hip_lib, i):
    name, arch, bn, batch, loss, seed = GRAD_CASES[i]
    sd, acts, X, y, r64, L32, g32, _ = _grad_case(i)
    L64 = float(r64["loss"])
    bound = 4.0 * tr.grad_error(g32, r64["grads"])
    # the loss is ONE number: torch's error on it can be 0 by luck, so its bound never goes below half a unit in the last place of the loss itself
    loss_bound = 4.0 * max(abs(L32 - L64), 2.0 ** -24 * abs(L64))
    t = HipMLPTrainer(_model(sd, acts), loss_fn=loss, max_batch=batch)
    assert (t.n_state > LDS_STATE_FLOATS) == (name == "wide-global")
    assert (t.n_state, t.n_train) == t.library_state_floats()
    Ld, gd = t.grad(_dev(X), _dev(y))
    Ld2, gd2 = t.grad(_dev(X), _dev(y))
    err = tr.grad_error(gd[0], r64["grads"])
    print(f"\n[mlp_train] grad {name:<15} B {batch:<4} {loss:<4} max|g| {tr.max_grad(r64['grads']):9.3e}  torch32 {bound / 4:9.3e}  device {err:9.3e}  ratio {err / bound:6.3f}"
          f"  loss {L64:.6f} torch32 err {abs(L32 - L64):8.2e} device err {abs(float(Ld[0]) - L64):8.2e}")
    assert set(gd[0]) == set(r64["grads"])
    assert all(np.isfinite(v).all() for v in gd[0].values())
    assert err <= bound
    assert abs(float(Ld[0]) - L64) <= loss_bound
    assert Ld[0] == Ld2[0] and all(np.array_equal(gd[0][k], gd2[0][k]) for k in gd[0])  # the same call twice: the same bits
    before = t.state_dict(0)
    assert all(np.array_equal(before[k], np.asarray(sd[k]).astype(before[k].dtype)) for k in before), "grad must not touch the state"
    t.close()


def test_batch_of_two_runs_finite_and_repeats(hip_lib):
    """B = 2 under BatchNorm is ill-conditioned (variance of the order of eps): no tolerance test, only "runs, finite, same bits twice"."""
    sd, acts, X, y = tr.make_case(tr.NOTEBOOK, 2, 11)
    t = HipMLPTrainer(_model(sd, acts), max_batch=2)
    a, b = t.grad(_dev(X), _dev(y)), t.grad(_dev(X), _dev(y))
    assert np.isfinite(a[0]).all() and all(np.isfinite(v).all() for v in a[1][0].values())
    assert a[0][0] == b[0][0] and all(np.array_equal(a[1][0][k], b[1][0][k]) for k in a[1][0])
    t.close()


# roundings between the inputs (p, g, moments) and the result, each worth one unit in the last place of max(|p|, |update|):
#   adam     g + wd p (2), exp_avg lerp (3), exp_avg_sq (4), sqrt, / bias_correction2_sqrt, + eps, m / denom, * step_size, p - update  = 15
#   adamw    p (1 - lr wd) (1), then adam without the decay term (13)                                                                   = 14
#   sgd      g + wd p (2), lr g, p - update                                                                                             = 4
#   rmsprop  g + wd p (2), square_avg (4), sqrt, + eps, g / avg, * lr, p - update                                                        = 11
STEP_ULPS = {"adam": 15, "adamw": 14, "sgd": 4, "rmsprop": 11}


def _ulp(x):
    return np.spacing(np.maximum(np.abs(x), np.float32(1e-30)).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("opt", tr.OPTIMIZERS)
def test_step_teacher_forced_against_torch_optim(hip_lib, opt, wd):
    sd, acts, X, y = tr.make_case(tr.NOTEBOOK, 17, 21)
    lr = 1e-3
    t = HipMLPTrainer(_model(sd, acts), optimizer=opt, lr=lr, weight_decay=wd, max_batch=17)
    worst = _teacher_forced_steps(t, sd, acts, _dev(X), _dev(y), opt, lr, wd)
    print(f"\n[mlp_train] step {opt:<8} wd {wd:<5} worst {worst:.2f} ulp of max(|p|, |update|) (allowed {STEP_ULPS[opt]})")
    t.close()


def _teacher_forced_steps(t, sd, acts, Xd, yd, opt, lr, wd, steps=3):
    """`steps` consecutive steps of handle t, each checked against the real torch.optim optimizer fed the device's own gradient and moments (shared with
    tests/test_gpu_mlp_train_shapes.py).  Returns the worst deviation in units in the last place of max(|p|, |update|)."""
    keys = tr.trainable_keys(sd, acts)
    worst = 0.0
    for step in range(steps):
        p0 = t.state_dict(0)
        m0, v0, n0 = t.moments(0)
        assert n0 == step
        _, g = t.grad(Xd, yd)
        t.step(Xd, yd)
        p1 = t.state_dict(0)
        m1, v1, n1 = t.moments(0)
        assert n1 == step + 1
        params = [torch.tensor(p0[k], requires_grad=True) for k in keys]
        o = tr.torch_optimizer(opt, params, lr, wd)
        for k, p in zip(keys, params):
            p.grad = torch.tensor(g[0][k])
            if step > 0 and opt in ("adam", "adamw"):
                o.state[p] = {"step": torch.tensor(float(step)), "exp_avg": torch.tensor(m0[k]), "exp_avg_sq": torch.tensor(v0[k])}
            elif step > 0 and opt == "rmsprop":
                o.state[p] = {"step": torch.tensor(float(step)), "square_avg": torch.tensor(v0[k])}
        o.step()
        for k, p in zip(keys, params):
            want = p.detach().numpy()
            scale = np.maximum(np.abs(p0[k]), np.abs(want.astype(np.float64) - p0[k]))
            ulps = np.abs(p1[k].astype(np.float64) - want) / _ulp(scale)
            worst = max(worst, float(ulps.max()))
            assert ulps.max() <= STEP_ULPS[opt], (opt, wd, step, k, float(ulps.max()))
            st = o.state[p] if opt != "sgd" else {}
            gk = np.maximum(np.abs(g[0][k].astype(np.float64)), np.abs(wd * p0[k]) * (opt != "adamw"))  # the larger term of g + wd p
            if "exp_avg" in st:
                u = np.abs(m1[k].astype(np.float64) - st["exp_avg"].numpy()) / _ulp(np.maximum(np.abs(m1[k]), np.abs(gk)))
                assert u.max() <= 5, (opt, step, k, "exp_avg", float(u.max()))
            for name in ("exp_avg_sq", "square_avg"):
                if name in st:
                    u = np.abs(v1[k].astype(np.float64) - st[name].numpy()) / _ulp(np.maximum(v1[k], gk * gk))
                    assert u.max() <= 8, (opt, step, k, name, float(u.max()))
    return worst


@pytest.mark.parametrize("i", [[c[0:1] + c[3:4] for c in GRAD_CASES].index(k) for k in (("tiny", 17), ("notebook", 128), ("wide-global", 17))],
                         ids=["tiny-b17", "notebook-b128", "wide-global-b17"])
def test_running_statistics_after_a_step(hip_lib, i):
    name, arch, bn, batch, loss, seed = GRAD_CASES[i]
    sd, acts, X, y, r64, _, _, T32 = _grad_case(i)
    t = HipMLPTrainer(_model(sd, acts), loss_fn=loss, max_batch=batch)
    t.step(_dev(X), _dev(y))
    after = t.state_dict(0)
    stats = {k: v for k, v in r64["stats"].items() if not k.endswith("num_batches_tracked")}
    top = max(float(np.abs(v).max()) for v in stats.values())
    torch_err = max(float(np.abs(T32[k].numpy().astype(np.float64) - v).max()) for k, v in stats.items()) / top
    dev_err = max(float(np.abs(after[k].astype(np.float64) - v).max()) for k, v in stats.items()) / top
    print(f"\n[mlp_train] running statistics {name} B {batch}: torch32 {torch_err:.3e} device {dev_err:.3e} ratio {dev_err / (4 * torch_err):.3f}")
    assert dev_err <= 4.0 * torch_err
    for k, v in r64["stats"].items():
        if k.endswith("num_batches_tracked"):
            assert after[k].dtype == np.int64 and int(after[k]) == int(v) == int(sd[k]) + 1
    t.close()


def test_train_epoch_is_repeated_step_bit_for_bit(hip_lib):
    sd, acts, X, y = tr.make_case(tr.NOTEBOOK, 45, 31)
    Xd, yd = _dev(X), _dev(y)
    order = torch.randperm(45, generator=torch.Generator().manual_seed(5)).to(torch.int32)
    a = HipMLPTrainer(_model(sd, acts), max_batch=16)
    b = HipMLPTrainer(_model(sd, acts), max_batch=16)
    loss, nc = a.train_epoch(Xd, yd, order.cuda(), batch_size=16)
    assert tuple(loss.shape) == (1, 3)
    idx = order.long().cuda()
    for bi in range(3):
        rows = idx[bi * 16:(bi + 1) * 16]
        assert len(rows) == (16, 16, 13)[bi]
        l1, n1 = b.step(Xd[rows].contiguous(), yd[rows].contiguous())
        assert float(l1[0]) == float(loss[0, bi]) and int(n1[0]) == int(nc[0, bi])
    sa, sb = a.state_dict(0), b.state_dict(0)
    assert all(np.array_equal(sa[k], sb[k]) for k in sa)
    assert any(not np.array_equal(sa[k], np.asarray(sd[k])) for k in sa)
    # a last batch of one sample: torch's reason, and the handle stays usable
    with pytest.raises(WtkError, match="more than 1 value per channel"):
        a.train_epoch(Xd[:33].contiguous(), yd[:33].contiguous(), None, batch_size=16)
    assert all(np.array_equal(a.state_dict(0)[k], sa[k]) for k in sa)
    l2, _ = a.train_epoch(Xd[:32].contiguous(), yd[:32].contiguous(), None, batch_size=16)
    assert np.isfinite(l2.cpu().numpy()).all()
    a.close(), b.close()


def test_a_models_bits_do_not_depend_on_the_population(hip_lib):
    nets = [tr.make_case(tr.NOTEBOOK, 45, s) for s in (41, 42, 43)]
    sd, acts, X, y = nets[0]
    Xd, yd = _dev(X), _dev(y)
    g = torch.Generator().manual_seed(9)
    orders = [torch.stack([torch.randperm(45, generator=g) for _ in range(2)]).to(torch.int32) for _ in range(3)]  # [model][epoch][n]

    def run(models, lrs, ords):
        t = HipMLPTrainer([_model(m[0], m[1]) for m in models], lr=lrs, max_batch=16)
        losses = []
        for ep in range(2):
            o = torch.stack([ords[j][ep] for j in range(len(models))]).cuda()
            losses.append(t.train_epoch(Xd, yd, o, batch_size=16)[0].cpu().numpy())
        out = [(t.state_dict(e), np.stack([l[e] for l in losses])) for e in range(len(models))]
        t.close()
        return out

    alone = run([nets[0]], [1e-3], [orders[0]])[0]
    first = run([nets[0], nets[1], nets[2]], [1e-3, 1e-2, 3e-3], [orders[0], orders[1], orders[2]])[0]
    last = run([nets[2], nets[1], nets[0]], [5e-3, 1e-4, 1e-3], [orders[1], orders[2], orders[0]])[2]
    again = run([nets[0]], [1e-3], [orders[0]])[0]
    for other in (first, last, again):
        assert np.array_equal(alone[1], other[1])
        assert all(np.array_equal(alone[0][k], other[0][k]) for k in alone[0])
    assert np.isfinite(alone[1]).all()


def _with_zero_blocks(sd, acts, arch):
    """The same network plus residual blocks whose Linear weights / biases and BatchNorm beta are 0: such a block returns relu(0) = 0, h + 0 = h, and its
    backward pass hands 0 to the residual gradient (the ReLU mask of an output of exactly 0 is off).  Enough of them to pass the LDS limit."""
    sd, acts = dict(sd), list(acts)
    res, nb, hidden = arch["block_in_dim"], arch["n_blocks"], 128
    lpb = len(arch["block_dims"])
    dims = [hidden] * (lpb - 1) + [res]

    def floats(d):
        return sum(int(np.size(v)) for k, v in d.items() if not k.endswith("num_batches_tracked"))

    while floats(sd) <= LDS_STATE_FLOATS:
        k = res
        for l, n in enumerate(dims):
            p = f"model.blocks.{nb}.sequence.{l}.mlp_layer"
            sd.update({p + ".0.weight": np.zeros((n, k), np.float32), p + ".0.bias": np.zeros(n, np.float32), p + ".1.weight": np.ones(n, np.float32),
                       p + ".1.bias": np.zeros(n, np.float32), p + ".1.running_mean": np.zeros(n, np.float32), p + ".1.running_var": np.ones(n, np.float32),
                       p + ".1.num_batches_tracked": np.asarray(0, np.int64)})
            acts.append("relu")
            k = n
        nb += 1
    return sd, acts


def test_lds_path_and_global_path_give_the_same_bits(hip_lib):
    """Both paths run the same code through flat pointers, so BOTH hold: the gradients of the shared layers are bit-equal, and every gradient of the added
    zero blocks is exactly 0 (their last ReLU's mask is off, so nothing flows back through them)."""
    sd, acts, X, y = tr.make_case(tr.TINY, 45, 51)
    big, big_acts = _with_zero_blocks(sd, acts, tr.TINY)
    Xd, yd = _dev(X), _dev(y)
    a = HipMLPTrainer(_model(sd, acts), max_batch=45)
    b = HipMLPTrainer(_model(big, big_acts), max_batch=45)
    assert a.n_state <= LDS_STATE_FLOATS < b.n_state and len(big_acts) + 1 <= mlp_ref.MAX_LAYERS
    (la, ga), (lb, gb) = a.grad(Xd, yd), b.grad(Xd, yd)
    assert la[0] == lb[0]
    for k in ga[0]:
        assert np.array_equal(ga[0][k], gb[0][k]), k
    for k in set(gb[0]) - set(ga[0]):
        assert not gb[0][k].any(), k
    # ... and a whole epoch: the same losses and the same shared parameters (sgd: a zero gradient leaves the zero blocks at zero)
    a2 = HipMLPTrainer(_model(sd, acts), optimizer="sgd", weight_decay=0.0, max_batch=16)
    b2 = HipMLPTrainer(_model(big, big_acts), optimizer="sgd", weight_decay=0.0, max_batch=16)
    l_a, _ = a2.train_epoch(Xd, yd, None, batch_size=16)
    l_b, _ = b2.train_epoch(Xd, yd, None, batch_size=16)
    assert torch.equal(l_a, l_b)
    sa, sb = a2.state_dict(0), b2.state_dict(0)
    assert all(np.array_equal(sa[k], sb[k]) for k in sa)
    for t in (a, b, a2, b2):
        t.close()


def _fp32_mean(losses) -> float:
    """The batch losses added in fp32 in batch order, divided by their number in fp32: the device's `curr`, bit for bit."""
    s = np.float32(0)
    for v in losses:
        s = np.float32(s + np.float32(v))
    return float(np.float32(s / np.float32(len(losses))))


def _host_early_stopping(epoch_losses, patience):
    """training.py:119-128 fed per-epoch lists of batch losses: (epochs run, index of the best epoch)."""
    best, without, best_epoch, ran = None, 0, -1, 0
    for ep, losses in enumerate(epoch_losses):
        ran += 1
        curr = _fp32_mean(losses)
        assert curr == pytest.approx(torch.Tensor([float(v) for v in losses]).mean().item(), rel=3e-7)  # torch's own fp32 mean: the same up to its summation order
        if best is None or curr < best:
            best, without, best_epoch = curr, 0, ep
        else:
            without += 1
            if patience is not None and without >= patience:
                break
    return ran, best_epoch, best, without


def test_eval_epoch_and_early_stopping(hip_lib):
    sd, acts, X, y = tr.make_case(tr.NOTEBOOK, 45, 61)
    Xd, yd = _dev(X), _dev(y)
    t = HipMLPTrainer([_model(sd, acts)] * 2, optimizer="sgd", lr=[1e-3, -1e-3], weight_decay=0.0, max_batch=16)  # model 1 ASCENDS its loss (negative lr): no epoch after the first improves
    # eval-mode predictions = wtk_mlp_forward on the folded model, within mlp_ref.tolerance
    loss, nc, pred = t.test_epoch(Xd, yd, batch_size=16, return_pred=True)
    m = t.folded(0, input_frames=list(range(-6, 1)), pred_frames=[1, 2, 3, 4])
    net = hip.HipMLP(m.layers, m.n_blocks, m.layers_per_block)
    want = net.forward_host(X)
    tol = mlp_ref.tolerance(sd, acts, X)
    assert float(np.abs(pred[0].cpu().numpy() - want).max()) <= tol
    y64 = mlp_ref.forward64(sd, acts, X)
    assert float(np.abs(pred[0].cpu().numpy() - y64).max()) <= tol
    e = tr.eval_step(sd, acts, X[:16], y[:16])
    assert abs(float(loss[0, 0]) - float(e["loss"])) <= 1e-5 * float(e["loss"]) and int(nc[0, 0]) == e["num_correct"]
    assert tuple(loss.shape) == (2, 3) and torch.equal(loss[0], loss[1])
    net.close()
    # fit with patience 2: per model, the device's decisions equal a host replay of training.py:119-128 fed the device's own losses
    res = t.fit(Xd, yd, Xd, yd, num_epochs=8, batch_size=16, early_stopping=2, seed=3)
    best_loss, has_best, without = t.stopping()
    assert all(isinstance(r, FitResult) for r in res)
    for e_, r in enumerate(res):
        per_epoch = [r.test_loss[i * 3:(i + 1) * 3] for i in range(len(r.test_loss) // 3)]
        ran, best_epoch, best, wo = _host_early_stopping(per_epoch, 2)
        assert ran == r.num_epochs == len(per_epoch) and len(r.train_loss) == 3 * ran and len(r.train_acc) == len(r.test_acc) == ran
        assert has_best[e_] == 1 and float(best_loss[e_]) == best and int(without[e_]) == wo
        assert int(t.state_dict(e_, best=True)[next(k for k in t.state_dict(e_) if k.endswith("num_batches_tracked"))]) == 1000 + 3 * (best_epoch + 1)
    assert res[0].num_epochs == 8 and res[1].num_epochs < 8, [r.num_epochs for r in res]
    assert t.active.cpu().tolist() == [1, 0]
    # the stopped model did not move after its last epoch; the best slot of model 1 is an earlier state than its current one
    cur, bst = t.state_dict(1), t.state_dict(1, best=True)
    assert any(not np.array_equal(cur[k], bst[k]) for k in cur)
    # a second fit starts its early stopping afresh, as Trainer.fit does (best_val_loss = None): model 1, still climbing, takes the new run's first epoch as
    # its best, although every loss of this run is above the first run's best
    old_best = float(best_loss[1])
    res2 = t.fit(Xd, yd, Xd, yd, num_epochs=2, batch_size=16, early_stopping=2, seed=4)
    best2, has2, without2 = t.stopping()
    first = _fp32_mean(res2[1].test_loss[:3])
    assert res2[1].num_epochs == 2 and first > old_best and has2[1] == 1 and float(best2[1]) == first and int(without2[1]) == 1
    # a caller's order with a row number outside [0, n) is refused before anything is launched
    bad = torch.arange(45, dtype=torch.int32)
    bad[7] = 45
    with pytest.raises(ValueError, match="outside"):
        t.train_epoch(Xd, yd, bad.cuda(), batch_size=16)
    t.close()


def test_it_learns_like_the_reference_trainer(hip_lib, golden_dir):
    sys.path.insert(0, golden_dir)
    from make_golden import synthetic_track

    z = np.load(os.path.join(golden_dir, "mlp_train.npz"))
    xi, yi = z["learn::input_frames"].tolist(), z["learn::pred_frames"].tolist()
    track = torch.from_numpy(synthetic_track(int(z["learn::track_frames"]), int(z["learn::track_seed"]))).cuda()
    X, y = resmlp.make_training_pairs_device(track, xi, yi)
    assert X.shape[0] == int(z["learn::n_pairs"])
    tr_idx, te_idx = torch.from_numpy(z["learn::train_idx"]).cuda(), torch.from_numpy(z["learn::test_idx"]).cuda()
    init = {k[len("learn::init::"):]: z[k] for k in z.files if k.startswith("learn::init::")}
    init.update(input_frames=xi, pred_frames=yi)
    ref = z["learn::final_val"].astype(np.float64)
    lo, hi = ref.min() - (ref.max() - ref.min()), ref.max() + (ref.max() - ref.min())
    t = HipMLPTrainer([init] * 8, lr=float(z["learn::lr"]), weight_decay=float(z["learn::weight_decay"]), max_batch=int(z["learn::batch_size"]))
    res = t.fit(X[tr_idx], y[tr_idx], X[te_idx], y[te_idx], num_epochs=int(z["learn::num_epochs"]), batch_size=int(z["learn::batch_size"]), seed=0)
    nb = -(-len(te_idx) // int(z["learn::batch_size"]))
    final = np.array([np.mean(np.asarray(r.test_loss[-nb:], np.float32)) for r in res], np.float64)
    first = np.array([np.mean(np.asarray(r.test_loss[:nb], np.float32)) for r in res], np.float64)
    print(f"\n[mlp_train] learns: reference final validation loss {ref.min():.3f} .. {ref.max():.3f} (first epoch {z['learn::first_val'].min():.3f} .. "
          f"{z['learn::first_val'].max():.3f}); device final {np.sort(final).round(3).tolist()} (first epoch {first.min():.3f} .. {first.max():.3f})")
    assert np.isfinite(final).all() and (final >= lo).all() and (final <= hi).all(), (final, lo, hi)
    assert (final < first).all()
    # the trained model goes through the closed loop
    from wtracker_amd.replay import Replay
    from wtracker_amd.sim import ExperimentConfig, TimingConfig

    folded = t.folded(int(np.argmin(final)))
    assert folded.in_dim == 28 and folded.out_dim == 8 and folded.input_frames == xi
    sd = t.state_dict(0)
    assert list(sd)[0] == "model.input.mlp_layer.0.weight" and list(sd)[-1] == "model.output.bias"
    ec = ExperimentConfig(name="exp0", num_frames=200, frames_per_sec=60, orig_resolution=(1600, 1400), px_per_mm=90, init_position=(1300, 1200))
    rp = Replay(track, TimingConfig(ec, 100, 40, 50, (4, 4), (0.32, 0.32)), ec)
    res = rp.run(rp.mlp(folded, max_speed=0.9))
    assert np.isfinite(np.asarray(res.moves[0], np.float64)).all()
    t.close()


def test_refusals_name_the_limit(hip_lib):
    sd, acts, X, y = tr.make_case(tr.TINY, 17, 71)
    with pytest.raises(ValueError, match="mse and l1"):
        HipMLPTrainer(_model(sd, acts), loss_fn="huber")
    with pytest.raises(ValueError, match="adam"):
        HipMLPTrainer(_model(sd, acts), optimizer="lion")
    with pytest.raises(ValueError, match="1024"):
        HipMLPTrainer(_model(sd, acts), max_batch=1025)
    with pytest.raises(WtkError, match="ReLU or none"):
        HipMLPTrainer(_model(sd, ["tanh"] + list(acts[1:])))
    wide, wacts = mlp_ref.random_rmlp(in_dim=28, block_in_dim=40, block_dims=[40], block_nonlins=["relu"], n_blocks=1, out_dim=2, seed=1)
    too_wide = {k: (np.zeros((v.shape[0], 129), np.float32) if k == "model.input.mlp_layer.0.weight" else v) for k, v in wide.items()}
    with pytest.raises(WtkError, match="kMlpMaxDim"):
        HipMLPTrainer(_model(too_wide, wacts))
    deep, dacts = mlp_ref.random_rmlp(in_dim=4, block_in_dim=16, block_dims=[16], block_nonlins=["relu"], n_blocks=63, out_dim=2, seed=1)
    with pytest.raises(WtkError, match="kMlpMaxLayers"):
        HipMLPTrainer(_model(deep, dacts))
    t = HipMLPTrainer(_model(sd, acts), max_batch=16)
    Xd, yd = _dev(X), _dev(y)
    with pytest.raises(WtkError, match="batch_size must be in"):
        t.step(Xd, yd)  # 17 rows on a handle of 16
    with pytest.raises(WtkError, match="batch_size must be in"):
        t.train_epoch(Xd, yd, None, batch_size=0)
    with pytest.raises(WtkError, match="more than 1 value per channel"):
        t.step(Xd[:1].contiguous(), yd[:1].contiguous())
    with pytest.raises(ValueError, match="CUDA float32"):
        t.step(Xd.double(), yd)
    nobn, nacts = mlp_ref.random_rmlp(**tr.TINY, batch_norm=False, seed=2)
    u = HipMLPTrainer(_model(nobn, nacts), max_batch=16)
    l, _ = u.step(Xd[:1].contiguous(), yd[:1].contiguous())  # a batch of one is fine without BatchNorm
    assert np.isfinite(float(l[0]))
    l3, _ = t.step(Xd[:16].contiguous(), yd[:16].contiguous())  # ... and the refused handle still trains
    assert np.isfinite(float(l3[0]))
    t.close(), u.close()
