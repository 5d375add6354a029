"""One training step of the reference's RMLP (wtracker/neural/mlp.py:51-188, train mode) restated in numpy, in float64 (the truth the device is
held to) and in float32 (an honest fp32 run, used for the ReLU guard band).  Forward with batch statistics, the running-statistics update, the
loss and num_correct of MLPTrainer.train_batch (training.py:304-319), the backward pass through Linear / BatchNorm1d / ReLU / the residual sum,
and one step of the four optimizers of neural/config.py:28-33 with torch's defaults.  tests/test_mlp_train_ref.py pins it against torch autograd
in float64 and against the real reference classes (tests/golden/mlp_train.npz).

Since r17 also: the same step in float32 with every sum in the ORDER of csrc/mlp_train.hip (device_order=True: the second fp32 reference of the shape tests,
next to torch float32), ten planted one-line defects (DEFECTS), the shape cases of tests/test_gpu_mlp_train_shapes.py (SHAPE_CASES) and the figures those tests
assert on (case_refs, check_step).

fp32 training of this network is chaotic: nothing here is meant to be compared along a trajectory, only step by step.
Errors of gradients are taken relative to the LARGEST gradient magnitude of the whole model: a Linear bias in front of a BatchNorm has a true
gradient of exactly 0, so a per-tensor relative error means nothing there.
"""
from __future__ import annotations

import numpy as np

from .mlp_ref import BN_EPS, _structure

BN_MOMENTUM = 0.1
NOTEBOOK = dict(in_dim=28, block_in_dim=80, block_dims=[40, 10, 40, 80], block_nonlins=["relu"] * 4, n_blocks=4, out_dim=8)  # predictor_training.ipynb
TINY = dict(in_dim=4, block_in_dim=16, block_dims=[8, 16], block_nonlins=["relu", "relu"], n_blocks=1, out_dim=2)
OPTIMIZERS = ("adam", "adamw", "sgd", "rmsprop")
WIDE = dict(in_dim=28, block_in_dim=128, block_dims=[128, 128], block_nonlins=["relu", "relu"], n_blocks=2, out_dim=2)  # 70 k floats: past the LDS limit of the trainer
# The gradient cases of tests/test_gpu_mlp_train.py (tests/test_mlp_train_ref.py checks their guard band on the CPU): name, RMLP arguments, batch_norm, batch,
# loss, seed.  Batches 17 / 128 / 130: one sample past a 16-sample tile, a tile edge, two past it.
GRAD_CASES = [
    ("tiny", TINY, True, 17, "mse", 0), ("tiny", TINY, True, 128, "mse", 1), ("tiny", TINY, True, 130, "l1", 2),
    ("notebook", NOTEBOOK, True, 17, "mse", 3), ("notebook", NOTEBOOK, True, 128, "mse", 4), ("notebook", NOTEBOOK, True, 130, "mse", 5),
    ("notebook", NOTEBOOK, True, 128, "l1", 6),
    ("notebook-no-bn", NOTEBOOK, False, 17, "mse", 7), ("notebook-no-bn", NOTEBOOK, False, 128, "mse", 10), ("notebook-no-bn", NOTEBOOK, False, 130, "mse", 8),
    ("wide-global", WIDE, True, 17, "mse", 9), ("wide-global", WIDE, True, 130, "mse", 11),
]


def layer_table(sd, acts):
    """[(prefix, weight key, bias key, bn prefix or None, relu)] in execution order, the output Linear last."""
    prefixes, n_blocks, per_block = _structure(sd)
    rows = [(p, p + ".0.weight", p + ".0.bias", (p + ".1") if (p + ".1.weight") in sd else None, acts[i] == "relu") for i, p in enumerate(prefixes)]
    rows.append(("model.output", "model.output.weight", "model.output.bias", None, False))
    return rows, n_blocks, per_block


def trainable_keys(sd, acts):
    keys = []
    for _, wk, bk, bn, _ in layer_table(sd, acts)[0]:
        keys += [wk, bk] + ([bn + ".weight", bn + ".bias"] if bn else [])
    return keys


def loss_and_grad(pred, y, loss: str, sign0: float = 0.0):
    d = pred - y
    n = d.size
    if loss == "mse":
        return (d * d).sum() / n, 2 * d / n
    assert loss == "l1", loss
    return np.abs(d).sum() / n, _sign(d, sign0) / n


def _sign(d, sign0: float = 0.0):
    return np.sign(d) if sign0 == 0.0 else np.where(d >= 0, 1.0, -1.0).astype(d.dtype)  # (sign0 = 1: the planted defect "l1_sign0_is_1")


def num_correct(pred, y, inclusive: bool = False) -> int:
    dist = np.sqrt(((pred - y) ** 2).sum(axis=1))
    return int((dist <= 1.0).sum() if inclusive else (dist < 1.0).sum())


# ---------------------------------------------------------------------------------------------------------------------------------
# the summation orders of csrc/mlp_train.hip (its header comment), in plain numpy on float32 arrays.  They make an honest fp32 run whose error is the
# device's KIND of error (a sequential chain over 1024 samples is less accurate than a blocked BLAS sum); nothing asserts that they give the device's bits
# (the element-wise code rounds every multiply and every add, as the library's build does: -ffp-contract=off).
def _fma_chain(A, Bt):
    """D[m][n] = sum_k A[m][k] Bt[n][k] as one fma chain in ascending k: the product of two float32 is exact in float64, so acc + a b rounds twice
    (to 53 bits, then to 24), which differs from the single rounding of an fma only on a tie of the second rounding."""
    acc = np.zeros((A.shape[0], Bt.shape[0]), np.float32)
    A64, B64 = A.astype(np.float64), Bt.astype(np.float64)
    for k in range(A.shape[1]):
        acc = (acc.astype(np.float64) + A64[:, k, None] * B64[None, :, k]).astype(np.float32)
    return acc


def _chan_sum_device(a):
    """Per-channel sum over the samples of a [B, C]: part j adds samples j, j + 8, ... in ascending order, then the 8 partial sums in the order j = 0 .. 7."""
    B, Cn = a.shape
    a = np.concatenate([a, np.zeros(((-B) % 8, Cn), np.float32)]).reshape(-1, 8, Cn)  # (x + 0 = x: the padding rows change nothing)
    part = np.zeros((8, Cn), np.float32)
    for r in range(a.shape[0]):
        part = part + a[r]
    total = np.zeros(Cn, np.float32)
    for j in range(8):
        total = total + part[j]
    return total


def _loss_sum_device(per_elem):
    """Sum of a [B, out]: per sample over the outputs in ascending order, then 64 runs of 16 samples, then the 64 partial sums."""
    s = np.zeros(per_elem.shape[0], np.float32)
    for o in range(per_elem.shape[1]):
        s = s + per_elem[:, o]
    s = np.concatenate([s, np.zeros(1024 - s.size, np.float32)]).reshape(64, 16)
    run = np.zeros(64, np.float32)
    for j in range(16):
        run = run + s[:, j]
    total = np.float32(0)
    for j in range(64):
        total = np.float32(total + run[j])
    return total


# One-line defects the restatement can switch on (tests/test_mlp_train_ref.py asserts that each one pushes a NAMED case over the bounds the GPU tests use):
DEFECTS = (
    "dw_drop_last_sample",   # dW = dz^T a leaves out the batch's last sample when B % 16 != 0
    "dw_drop_last_col",      # the last input column of dW is not written when in_dim % 16 != 0
    "dx_drop_k_tail",        # dx = dz W leaves out the outputs behind the last multiple of 4 when out_dim % 4 != 0
    "biased_running_var",    # running_var takes the biased batch variance
    "no_residual_grad",      # dh <- d(block input) instead of dh + d(block input)
    "relu_mask_pre_bn",      # the ReLU mask of a BatchNorm layer taken from the Linear's output
    "bn_no_dbeta",           # the BatchNorm backward without its dbeta term
    "mean_tile_rounded_b",   # the batch mean divided by B rounded up to a 16-sample tile
    "l1_sign0_is_1",         # l1: sign(0) = 1
    "num_correct_le",        # num_correct counts distance <= 1
)


def train_forward_backward(sd, acts, X, y, loss="mse", dtype=np.float64, device_order: bool = False, defect: str | None = None):
    """Train-mode forward + backward of one batch.  Returns dict(loss, num_correct, pred, grads {key: array}, stats {running_mean / running_var /
    num_batches_tracked key: value after the batch}, pre_relu [array per ReLU layer]).

    device_order (float32 only): every sum in the order of csrc/mlp_train.hip — products as ascending-k fma chains (forward over the inputs, dW over the
    batch's samples, dx over the outputs), per-channel sums over the samples as 8 interleaved partial sums added in the order j = 0 .. 7, the loss as 64 runs
    of 16 samples and then the 64 partial sums; loss scale and loss gradient through 1 / n rounded to fp32, running_var from sq / (B - 1).
    defect: one of DEFECTS."""
    assert defect is None or defect in DEFECTS, defect
    assert not device_order or dtype == np.float32
    rows, n_blocks, per_block = layer_table(sd, acts)
    P = lambda k: np.asarray(sd[k]).astype(dtype)  # noqa: E731
    X, y = np.asarray(X).astype(dtype), np.asarray(y).astype(dtype)
    B = X.shape[0]
    eps = dtype(BN_EPS)
    stats, pre_relu, caches = {}, [], []
    mm = _fma_chain if device_order else (lambda A, Bt: A @ Bt.T)  # D[m][n] = sum_k A[m][k] Bt[n][k]
    csum = _chan_sum_device if device_order else (lambda a: a.sum(axis=0))

    def fwd(i, h):
        _, wk, bk, bn, relu = rows[i]
        W = P(wk)
        z = mm(h, W) + P(bk)
        c = dict(i=i, inp=h, W=W, bn=bn, relu=relu)
        if bn:
            z_lin = z
            mean = csum(z) / dtype((B + 15) // 16 * 16 if defect == "mean_tile_rounded_b" else B)
            sq = csum((z - mean) ** 2)
            var = sq / dtype(B)
            inv = dtype(1) / np.sqrt(var + eps)
            xh = (z - mean) * inv
            g = P(bn + ".weight")
            z = xh * g + P(bn + ".bias")
            c.update(xh=xh, inv=inv, g=g)
            m = dtype(BN_MOMENTUM)
            unbiased = var if defect == "biased_running_var" else (sq / dtype(B - 1) if device_order else var * dtype(B) / dtype(B - 1))
            stats[bn + ".running_mean"] = (dtype(1) - m) * P(bn + ".running_mean") + m * mean
            stats[bn + ".running_var"] = (dtype(1) - m) * P(bn + ".running_var") + m * unbiased
            stats[bn + ".num_batches_tracked"] = np.asarray(int(sd[bn + ".num_batches_tracked"]) + 1, np.int64)
        if relu:
            pre_relu.append(z)
            c["mask"] = (z_lin > 0) if (bn and defect == "relu_mask_pre_bn") else (z > 0)
            z = np.maximum(z, dtype(0))
        caches.append(c)
        return z

    h = fwd(0, X)
    i = 1
    for _ in range(n_blocks):
        t = h
        for _ in range(per_block):
            t = fwd(i, t)
            i += 1
        h = h + t
    pred = fwd(i, h)
    sign0 = 1.0 if defect == "l1_sign0_is_1" else 0.0
    if device_order:
        d = pred - y
        inv_n = np.float32(1) / np.float32(d.size)
        L = _loss_sum_device(d * d if loss == "mse" else np.abs(d)) * inv_n
        dpred = np.float32(2) * d * inv_n if loss == "mse" else _sign(d, sign0) * inv_n
    else:
        L, dpred = loss_and_grad(pred, y, loss, sign0)
    grads = {}

    def bwd(c, d):
        _, wk, bk, bn, _ = rows[c["i"]]
        if c["relu"]:
            d = d * c["mask"]
        if bn:
            dg, dbeta = csum(d * c["xh"]), csum(d)
            grads[bn + ".weight"], grads[bn + ".bias"] = dg, dbeta
            d = c["g"] * c["inv"] / dtype(B) * (dtype(B) * d - (dtype(0) if defect == "bn_no_dbeta" else dbeta) - c["xh"] * dg)
        dz, inp, W = d, c["inp"], c["W"]
        if defect == "dw_drop_last_sample" and B % 16:
            dz, inp = dz[:-1], inp[:-1]
        grads[wk], grads[bk] = mm(dz.T, inp.T), csum(d)
        if defect == "dw_drop_last_col" and W.shape[1] % 16:
            grads[wk][:, -1] = 0
        if defect == "dx_drop_k_tail" and W.shape[0] % 4:
            keep = W.shape[0] // 4 * 4
            return mm(d[:, :keep], W.T[:, :keep])
        return mm(d, W.T)

    dh = bwd(caches[-1], dpred.astype(dtype))
    for b in reversed(range(n_blocks)):
        d = dh
        for l in reversed(range(per_block)):
            d = bwd(caches[1 + b * per_block + l], d)
        dh = d if defect == "no_residual_grad" else dh + d
    bwd(caches[0], dh)
    assert all(g.dtype == dtype for g in grads.values())
    return dict(loss=dtype(L), num_correct=num_correct(pred, y, inclusive=defect == "num_correct_le"), pred=pred, grads=grads, stats=stats, pre_relu=pre_relu)


def eval_step(sd, acts, X, y, loss="mse", dtype=np.float64):
    """MLPTrainer.test_batch: eval-mode forward on the running statistics, loss and num_correct."""
    from .mlp_ref import _dot64, _forward

    pred = _forward(sd, acts, X, dtype, _dot64)
    L, _ = loss_and_grad(pred, np.asarray(y).astype(dtype), loss)
    return dict(loss=dtype(L), num_correct=num_correct(pred, np.asarray(y).astype(dtype)), pred=pred)


def optimizer_step(opt: str, p, g, state: dict, lr: float, weight_decay: float):
    """One step of torch.optim.{Adam, AdamW, SGD, RMSprop}(lr=, weight_decay=) on one tensor, in p's dtype; `state` ({} at first) carries step,
    exp_avg, exp_avg_sq / square_avg.  Adam: L2 decay added to the gradient; AdamW: decoupled; SGD: no momentum; RMSprop: alpha 0.99, eps 1e-8."""
    dt = p.dtype.type
    g = g.astype(p.dtype)
    t = state["step"] = state.get("step", 0) + 1
    if opt == "adamw":
        p = p * dt(1 - lr * weight_decay)
    elif weight_decay != 0:
        g = g + dt(weight_decay) * p
    if opt in ("adam", "adamw"):
        b1, b2, eps = 0.9, 0.999, 1e-8
        m = state.get("exp_avg", np.zeros_like(p))
        v = state.get("exp_avg_sq", np.zeros_like(p))
        m = m + (g - m) * dt(1 - b1)
        v = v * dt(b2) + dt(1 - b2) * g * g
        state["exp_avg"], state["exp_avg_sq"] = m, v
        step_size = lr / (1 - b1 ** t)
        denom = np.sqrt(v) / dt((1 - b2 ** t) ** 0.5) + dt(eps)
        return p - dt(step_size) * (m / denom)
    if opt == "sgd":
        return p - dt(lr) * g
    assert opt == "rmsprop", opt
    v = state.get("square_avg", np.zeros_like(p))
    v = v * dt(0.99) + dt(0.01) * g * g
    state["square_avg"] = v
    return p - dt(lr) * (g / (np.sqrt(v) + dt(1e-8)))


def max_grad(grads) -> float:
    return max(float(np.abs(np.asarray(g, np.float64)).max()) for g in grads.values())


def grad_error(grads, truth) -> float:
    """Largest |g - truth| over every gradient of the model, relative to the model's largest gradient magnitude."""
    top = max_grad(truth)
    return max(float(np.abs(np.asarray(grads[k], np.float64) - np.asarray(truth[k], np.float64)).max()) for k in truth) / top


# ---------------------------------------------------------------------------------------------------------------------------------
# the same step by torch autograd (functional, from the state dict: no module classes needed)
def torch_forward(T, acts, X, train: bool):
    """T: {key: torch tensor}.  Train mode updates T's running statistics in place, as BatchNorm1d does."""
    import torch.nn.functional as F

    rows, n_blocks, per_block = layer_table(T, acts)

    def fwd(i, h):
        _, wk, bk, bn, relu = rows[i]
        z = F.linear(h, T[wk], T[bk])
        if bn:
            z = F.batch_norm(z, T[bn + ".running_mean"], T[bn + ".running_var"], T[bn + ".weight"], T[bn + ".bias"], training=train, momentum=BN_MOMENTUM, eps=BN_EPS)
            if train:
                T[bn + ".num_batches_tracked"] += 1
        return F.relu(z) if relu else z

    h = fwd(0, X)
    i = 1
    for _ in range(n_blocks):
        t = h
        for _ in range(per_block):
            t = fwd(i, t)
            i += 1
        h = h + t
    return fwd(i, h)


def torch_tensors(sd, acts, dtype):
    import torch

    keys = set(trainable_keys(sd, acts))
    T = {}
    for k, v in sd.items():
        t = torch.tensor(np.asarray(v))
        if t.is_floating_point():
            t = t.to(dtype)
        T[k] = t.requires_grad_(True) if k in keys else t
    return T


def torch_train_step(sd, acts, X, y, loss="mse", dtype=None):
    """(loss, {key: gradient}, T) of one batch by torch autograd; T holds the updated running statistics."""
    import torch

    dtype = dtype or torch.float64
    T = torch_tensors(sd, acts, dtype)
    pred = torch_forward(T, acts, torch.tensor(np.asarray(X)).to(dtype), True)
    fn = torch.nn.MSELoss() if loss == "mse" else torch.nn.L1Loss()
    L = fn(pred, torch.tensor(np.asarray(y)).to(dtype))
    L.backward()
    return float(L.detach()), {k: T[k].grad.numpy() for k in trainable_keys(sd, acts)}, T


def torch_optimizer(opt: str, params, lr: float, weight_decay: float):
    import torch

    cls = {"adam": torch.optim.Adam, "adamw": torch.optim.AdamW, "sgd": torch.optim.SGD, "rmsprop": torch.optim.RMSprop}[opt]
    return cls(params, lr=lr, weight_decay=weight_decay)


# ---------------------------------------------------------------------------------------------------------------------------------
# cases of the gradient test: built so that no pre-ReLU value of the float64 run lies inside the guard band
GUARD_FACTOR = 64.0


def make_case(arch: dict, batch: int, seed: int, batch_norm: bool = True, clear_kinks: bool = False, loss: str = "mse"):
    """(state dict, activations, X, y) of a seeded random network and batch.  clear_kinks: move the case off every ReLU kink (below)."""
    from .mlp_ref import random_rmlp

    sd, acts = random_rmlp(**arch, batch_norm=batch_norm, seed=seed)
    rng = np.random.default_rng(seed + 7919)
    X = rng.normal(0, 6, size=(batch, arch["in_dim"])).astype(np.float32)
    y = rng.normal(0, 2, size=(batch, arch["out_dim"])).astype(np.float32)
    if clear_kinks:
        sd = clear_relu_kinks(sd, acts, X, y, loss)
    return sd, acts, X, y


def _clear_shift(v: np.ndarray, margin: float) -> float:
    """The smallest |d| with |v + d| >= margin for every element of v."""
    if (np.abs(v) >= margin).all():
        return 0.0
    m = margin * (1 + 1e-6)
    cands = np.concatenate([-(v + m), -(v - m)])
    cands = cands[np.argsort(np.abs(cands), kind="stable")]
    for d in cands:
        if (np.abs(v + d) >= margin).all():
            return float(d)
    raise AssertionError("no shift clears the channel")


def clear_relu_kinks(sd, acts, X, y, loss="mse", margin_factor: float = 4.0):
    """A pre-ReLU value at 0 +- rounding flips a mask between two correct fp32 runs and breaks any gradient bound.  A seed search cannot avoid that on
    the notebook's model (97 000 pre-ReLU values at batch 128, ~100 of them inside the band for any seed), so the case is CONSTRUCTED off the kinks:
    layer by layer in execution order, every channel with a pre-ReLU value inside margin = 4 x band gets its additive parameter in front of the ReLU
    (the BatchNorm's beta, or the Linear's bias without one) moved by the smallest shift that takes all of the channel's values out.  A shift changes
    only the layers behind it, so one pass per ReLU layer suffices; guard_band() of the result is what the tests assert on."""
    rows = layer_table(sd, acts)[0]
    relu_rows = [r for r in rows if r[4]]
    sd = {k: np.array(v, copy=True) for k, v in sd.items()}
    margin = margin_factor * guard_band(sd, acts, X, y, loss)[1]
    for j, (_, _, bk, bn, _) in enumerate(relu_rows):
        pre = train_forward_backward(sd, acts, X, y, loss, np.float64)["pre_relu"][j]
        key = (bn + ".bias") if bn else bk
        for c in np.nonzero((np.abs(pre) < margin).any(axis=0))[0]:
            want = float(sd[key][c]) + _clear_shift(pre[:, c], 1.5 * margin)
            sd[key][c] = np.float32(want)
    return sd


def guard_band(sd, acts, X, y, loss="mse"):
    """(elements of the float64 pre-ReLU values inside the band, band): band = 64 x the largest float32 / float64 difference of a pre-ReLU value."""
    r64 = train_forward_backward(sd, acts, X, y, loss, np.float64)
    r32 = train_forward_backward(sd, acts, X, y, loss, np.float32)
    band = GUARD_FACTOR * max(float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(r32["pre_relu"], r64["pre_relu"]))
    inside = sum(int((np.abs(b) < band).sum()) for b in r64["pre_relu"])
    return inside, band


# ---------------------------------------------------------------------------------------------------------------------------------
# the shape cases of tests/test_gpu_mlp_train_shapes.py: name, RMLP arguments, batch_norm, batch, loss, seed (as GRAD_CASES).
#   every row of mlp_ref.ARCHS (each named for its hazard there) at batch 19 = one 16-sample tile and three samples
#   odd             widths 3, 65, 127, 1, 33: one past a 16-tile, one short of 128, a single column; at 19 and at 49 = 3 x 16 + 1
#   notebook 257 / 513 / 1023 / 1024   one past 2 and 4 x 128 samples (the 8-part channel sums and the 64 x 16 loss runs), one short of full, full
#   wide 1024 l1    the full batch on the global-memory parameter path; hourglass 1000: 62 full loss runs and one of 8
LDS_STATE_FLOATS = 36864  # wtracker_amd.training.LDS_STATE_FLOATS (kTrainLdsFloats): a state above this trains from global memory
ODD = dict(in_dim=3, block_in_dim=65, block_dims=[127, 1, 33, 65], block_nonlins=["relu"] * 4, n_blocks=2, out_dim=1)


def _arch(name):
    from .mlp_ref import arch_args

    return arch_args(name)


SHAPE_CASES = [(name, _arch(name), True, 19, "mse", 200 + i) for i, name in enumerate(
    ["no-blocks", "one-slice-edge", "two-slices", "wide-lds", "wide-global", "ragged-global", "hourglass", "hourglass-lds", "odd-pingpong", "none-in-block", "tiny-in"])] + [
    ("odd", ODD, True, 19, "mse", 220), ("odd", ODD, True, 49, "l1", 221),
    ("notebook", NOTEBOOK, True, 257, "mse", 230), ("notebook", NOTEBOOK, True, 513, "mse", 231), ("notebook", NOTEBOOK, True, 1023, "mse", 232),
    ("notebook", NOTEBOOK, True, 1024, "mse", 233), ("notebook-no-bn", NOTEBOOK, False, 1024, "mse", 234),
    ("wide", WIDE, True, 1024, "l1", 235), ("hourglass", _arch("hourglass"), True, 1000, "mse", 236),
]
# The parameter path of the TRAINER per architecture (not the inference kernel's, whose padded blob has another limit): floats of the unfolded state.
# hourglass (35 630) and the notebook's model (35 488) sit just under the limit, wide-global (38 530) and wide (72 578) above it.
SHAPE_PATH = {"no-blocks": "lds", "one-slice-edge": "lds", "two-slices": "lds", "wide-lds": "lds", "wide-global": "global", "ragged-global": "lds", "hourglass": "lds",
              "hourglass-lds": "lds", "odd-pingpong": "lds", "none-in-block": "lds", "tiny-in": "lds", "odd": "lds", "notebook": "lds", "notebook-no-bn": "lds",
              "wide": "global", "tiny": "lds"}


def case_id(case) -> str:
    return f"{case[0]}-b{case[3]}-{case[4]}"


def state_floats(sd) -> int:
    """Floats of the trainer's unfolded state: every tensor but num_batches_tracked."""
    return sum(int(np.size(v)) for k, v in sd.items() if not k.endswith("num_batches_tracked"))


def zero_gradient_keys(sd, acts):
    """The Linear biases whose true gradient is identically 0: a bias in front of a BatchNorm (the BatchNorm removes it), and the bias of a plain Linear
    (no BatchNorm, no ReLU) inside a block whose only reader is such a layer (mlp_ref's none-in-block: the next Linear turns it into a constant per
    channel, which that layer's BatchNorm removes as well)."""
    rows, n_blocks, per_block = layer_table(sd, acts)
    zero = [bool(bn) for _, _, _, bn, _ in rows]
    for b in range(n_blocks):
        for l in reversed(range(per_block - 1)):  # (the last layer of a block is read by the residual sum)
            i = 1 + b * per_block + l
            zero[i] = zero[i] or (not rows[i][4] and zero[i + 1])
    return {rows[i][2] for i in range(len(rows)) if zero[i]}


def tensor_grad_error(grads, truth, skip=()) -> float:
    """Largest |g - truth| of a tensor relative to THAT tensor's largest true gradient, over the tensors whose true gradient is not identically zero
    (`skip`: zero_gradient_keys; a tensor that is exactly 0 in the truth is left out too).  grad_error hides a wrong entry of a tensor whose gradients
    are small next to the model's largest one; this does not."""
    worst = 0.0
    for k, t in truth.items():
        top = float(np.abs(np.asarray(t, np.float64)).max())
        if k in skip or top == 0.0:
            continue
        worst = max(worst, float(np.abs(np.asarray(grads[k], np.float64) - np.asarray(t, np.float64)).max()) / top)
    return worst


def stats_error(stats, truth) -> float:
    """Largest |running statistic - truth| relative to the largest running statistic of the model."""
    keys = [k for k in truth if not k.endswith("num_batches_tracked")]
    top = max(float(np.abs(truth[k]).max()) for k in keys)
    return max(float(np.abs(np.asarray(stats[k], np.float64) - truth[k]).max()) for k in keys) / top


import functools  # noqa: E402


@functools.lru_cache(maxsize=None)
def _case_refs(case_key):
    name, arch, bn, batch, loss, seed = _CASES_BY_KEY[case_key]
    sd, acts, X, y = make_case(arch, batch, seed, bn, clear_kinks=True, loss=loss)
    for v in (X, y, *sd.values()):
        v.setflags(write=False)
    return refs_of(sd, acts, X, y, loss)


def refs_of(sd, acts, X, y, loss):
    """The float64 truth, the two fp32 references and the bounds of one batch (case_refs documents the fields)."""
    import torch

    r64 = train_forward_backward(sd, acts, X, y, loss, np.float64)
    L32, g32, T32 = torch_train_step(sd, acts, X, y, loss, torch.float32)
    rdev = train_forward_backward(sd, acts, X, y, loss, np.float32, device_order=True)
    skip = zero_gradient_keys(sd, acts)
    L64 = float(r64["loss"])
    b = dict(
        # 4 x the larger error of two honest fp32 runs of the same case, neither of them the code under test: torch float32 (blocked sums) and the
        # restatement in the device's summation order (sequential chains, which at 1024 samples are legitimately less accurate than torch's)
        grad=4.0 * max(grad_error(g32, r64["grads"]), grad_error(rdev["grads"], r64["grads"])),
        tensor=4.0 * max(tensor_grad_error(g32, r64["grads"], skip), tensor_grad_error(rdev["grads"], r64["grads"], skip)),
        # the loss is ONE number: an error of 0 by luck must not make the bound 0, so it never goes below half a unit in the last place of the loss
        loss=4.0 * max(abs(L32 - L64), abs(float(rdev["loss"]) - L64), 2.0 ** -24 * abs(L64)))
    if r64["stats"]:
        t32 = {k: T32[k].numpy() for k in r64["stats"]}
        b["stats"] = 4.0 * max(stats_error(t32, r64["stats"]), stats_error(rdev["stats"], r64["stats"]))
    torch32 = dict(grad=grad_error(g32, r64["grads"]), tensor=tensor_grad_error(g32, r64["grads"], skip))
    order32 = dict(grad=grad_error(rdev["grads"], r64["grads"]), tensor=tensor_grad_error(rdev["grads"], r64["grads"], skip))
    return dict(sd=sd, acts=acts, X=X, y=y, loss=loss, r64=r64, rdev=rdev, bounds=b, skip=skip, torch32=torch32, order32=order32)


_CASES_BY_KEY = {}


def case_refs(case):
    """Everything the GPU tests and the planted-defect tests need of a case of SHAPE_CASES / GRAD_CASES, built once per process and read-only:
    dict(sd, acts, X, y, loss, r64 = the float64 restatement, rdev = the fp32 restatement in the device's order, bounds {grad, tensor, loss, stats},
    skip = zero_gradient_keys, torch32 / order32 = the two references' own errors)."""
    key = (case_id(case), case[5], case[2])
    _CASES_BY_KEY[key] = case
    return _case_refs(key)


def check_step(refs, loss_value, grads, stats=None, n_correct=None) -> dict:
    """The figures the GPU tests assert on, of one result (the device's, or a planted defect's) against the float64 restatement of the case:
    {grad, tensor, loss, [stats]: error / bound}, plus `failed`: the names of the checks that do not hold."""
    r64, b = refs["r64"], refs["bounds"]
    out = dict(grad=grad_error(grads, r64["grads"]) / b["grad"], tensor=tensor_grad_error(grads, r64["grads"], refs["skip"]) / b["tensor"],
               loss=abs(float(loss_value) - float(r64["loss"])) / b["loss"])
    if stats is not None:
        out["stats"] = stats_error(stats, r64["stats"]) / b["stats"]
    out["failed"] = [k for k, v in list(out.items()) if not v <= 1.0]
    if n_correct is not None and int(n_correct) != r64["num_correct"]:
        out["failed"].append("num_correct")
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# l1 at a residual of exactly 0, and num_correct at a distance of exactly 1
def make_l1_zero_case(batch: int = 32, seed: int = 240):
    """(sd, acts, X, y, cls): TINY without BatchNorm and with an all-zero output weight, so the prediction IS the output bias in any precision and any
    summation order; the bias is dyadic (0.25, -0.5) and y = bias + {0, +1, -1} (cls 0 / 1 / 2, a third of the entries each, seeded), so every residual
    is exactly 0, -1 or +1 in float32 and in float64 and a sample's distance is exactly 0, 1 or sqrt 2.  n = batch x 2 = 64 is a power of two: 1 / n and
    every sum of +-1 / n are exact in float32, so the output bias gradient (n_pos - n_neg) / n has ONE float32 value whatever the order of the sum."""
    from .mlp_ref import random_rmlp

    sd, acts = random_rmlp(**TINY, batch_norm=False, seed=seed)
    sd = dict(sd)
    sd["model.output.weight"] = np.zeros_like(sd["model.output.weight"])
    sd["model.output.bias"] = np.array([0.25, -0.5], np.float32)
    rng = np.random.default_rng(seed + 1)
    X = rng.normal(0, 6, size=(batch, TINY["in_dim"])).astype(np.float32)
    cls = rng.permutation(np.arange(batch * 2) % 3).reshape(batch, 2)
    y = (sd["model.output.bias"][None, :] + np.where(cls == 1, 1.0, np.where(cls == 2, -1.0, 0.0))).astype(np.float32)
    return sd, acts, X, y, cls


def l1_zero_bias_gradient(cls) -> np.ndarray:
    """(n_pos - n_neg) / n per output column: cls 2 (y below the bias) is a positive residual, cls 1 a negative one."""
    return ((cls == 2).sum(axis=0) - (cls == 1).sum(axis=0)) / float(cls.size)


# ---------------------------------------------------------------------------------------------------------------------------------
# num_correct that means something: y = the float64 prediction + an offset whose norm is well inside or well outside 1
def _offsets(rng, n, out_dim):
    norms = np.where(np.arange(n) % 2 == 0, rng.uniform(0.2, 0.9, size=n), rng.uniform(1.1, 3.0, size=n))[rng.permutation(n)]
    v = rng.normal(size=(n, out_dim))
    return v / np.sqrt((v * v).sum(axis=1, keepdims=True)) * norms[:, None]


def _distances(pred, y):
    return np.sqrt(((pred.astype(np.float64) - np.asarray(y, np.float64)) ** 2).sum(axis=1))


NC_CASES = [("notebook", NOTEBOOK, 45, 16, 250), ("notebook", NOTEBOOK, 45, 45, 251), ("notebook", NOTEBOOK, 1024, 1024, 252),
            ("odd", ODD, 45, 16, 253)]  # name, arch, rows, batch_size, seed


@functools.lru_cache(maxsize=None)
def nc_case(i: int, mode: str):
    """(sd, acts, X, y, counts, margin) of NC_CASES[i]: the rows are walked in order in batches of batch_size (the last one partial); mode "train": the
    prediction of a batch is the train-mode one of the INITIAL parameters (batch statistics of that batch: what `step` sees, and every batch of a
    train_epoch whose learning rate and weight decay are 0); "eval": the eval-mode one.  counts: num_correct per batch of the float64 restatement;
    margin: the smallest | distance - 1 | / | float32 distance - float64 distance | over all samples (the input condition asks for >= 64)."""
    name, arch, n, bs, seed = NC_CASES[i]
    sd, acts, X, _ = make_case(arch, n, seed)
    rng = np.random.default_rng(seed + 104729)
    y = np.zeros((n, arch["out_dim"]), np.float32)
    counts, margin = [], np.inf
    for b0 in range(0, n, bs):
        rows = slice(b0, min(b0 + bs, n))
        if mode == "train":
            p64 = train_forward_backward(sd, acts, X[rows], y[rows], "mse", np.float64)["pred"]
            p32 = train_forward_backward(sd, acts, X[rows], y[rows], "mse", np.float32, device_order=True)["pred"]
        else:
            assert mode == "eval", mode
            p64 = eval_step(sd, acts, X[rows], y[rows])["pred"]
            p32 = eval_step(sd, acts, X[rows], y[rows], dtype=np.float32)["pred"]
        y[rows] = (p64 + _offsets(rng, p64.shape[0], p64.shape[1])).astype(np.float32)
        d64, d32 = _distances(p64, y[rows]), _distances(p32, y[rows])
        counts.append(int((d64 < 1.0).sum()))
        margin = min(margin, float((np.abs(d64 - 1.0) / np.maximum(np.abs(d32 - d64), 1e-300)).min()))
    for v in (X, y, *sd.values()):
        v.setflags(write=False)
    return sd, acts, X, y, counts, margin
