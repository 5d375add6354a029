#!/usr/bin/env python3
"""Generate tests/golden/mlp_train.npz by running the REAL reference's RMLP and MLPTrainer (wtracker/neural/mlp.py, training.py).

Like make_golden.py this runs only where the reference is present, and stores numeric data only.  `torch.utils.tensorboard` is not installed
here; training.py imports SummaryWriter from it at module level and only constructs it with log=True, so a placeholder module stands in.

Part 1 (tests/test_mlp_train_ref.py): a small RMLP (28 -> 24, two blocks [12, 6, 12, 24], out 8) and MLPTrainer.train_batch / test_batch CONVERTED TO
float64, three steps on one batch for each optimizer of neural/config.py's OPTIMIZERS (lr and weight_decay given, the rest torch's defaults):
    init::<key>                       the initial state dict            acts, X, y, lr, weight_decay, loss
    grad::<key>                       the first step's gradients (the same for every optimizer)
    <opt>::loss / ::num_correct       [3]
    <opt>::state<step>::<key>         the state dict after every step
    <opt>::test_loss / ::test_num_correct   test_batch on the same batch after the third step
Part 2 (tests/test_gpu_mlp_train.py, "it learns"): the notebook's model (28 -> 80, blocks [40, 10, 40, 80] x 4, out 8) trained in float32 by the real
MLPTrainer.fit for 10 epochs on training pairs of a synthetic track, over 8 shuffle seeds from the same initial state.  Losses only:
    learn::init::<key>, learn::train_idx, learn::test_idx, learn::final_val [8] (mean of the last epoch's test-batch losses), learn::first_val [8]
    and the settings (learn::lr, ::weight_decay, ::batch_size, ::num_epochs, ::track_frames, ::track_seed, ::input_frames, ::pred_frames)
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden import _register_placeholders, synthetic_track  # noqa: E402

SMALL = dict(block_in_dim=24, block_dims=[12, 6, 12, 24], block_nonlins=["relu"] * 4, n_blocks=2, out_dim=8, in_dim=28)
NOTEBOOK = dict(block_in_dim=80, block_dims=[40, 10, 40, 80], block_nonlins=["relu"] * 4, n_blocks=4, out_dim=8, in_dim=28)
LEARN = dict(lr=1e-2, weight_decay=1e-5, batch_size=64, num_epochs=10, track_frames=700, track_seed=11,
             input_frames=[0, -3, -15, -18, -30, -33, -45], pred_frames=[1, 10, 20, 30], seeds=list(range(8)), split_seed=42)


def pairs_from_track(track, input_frames, pred_frames):
    """NumpyDataset.create_from_config's arithmetic (wtracker/neural/dataset.py:42-96) on an xywh track: what wtracker_amd.resmlp.make_training_pairs
    computes from a bboxes.csv, and make_training_pairs_device bit for bit on the device."""
    boxes = np.asarray(track, np.float64)
    centers = np.stack([boxes[:, 0] + boxes[:, 2] / 2, boxes[:, 1] + boxes[:, 3] / 2], axis=1)
    xi, yi = np.asarray(input_frames, int), np.asarray(pred_frames, int)
    rows = np.arange(abs(int(xi.min())) + 1, len(boxes) - int(yi.max()) - 1)
    X = boxes[rows[:, None] + xi[None, :]].reshape(rows.size, -1)
    y = centers[rows[:, None] + yi[None, :]].reshape(rows.size, -1)
    keep = ~(np.isnan(X).any(axis=1) | np.isnan(y).any(axis=1))
    X, y = X[keep].astype(np.float32), y[keep].astype(np.float32)
    x0, y0 = X[:, 0:1].copy(), X[:, 1:2].copy()
    y[:, 0::2] -= x0
    y[:, 1::2] -= y0
    X[:, 0::4] -= x0
    X[:, 1::4] -= y0
    return X, y


def main():
    _register_placeholders()
    tb = types.ModuleType("torch.utils.tensorboard")
    tb.SummaryWriter = type("SummaryWriter", (), {})
    sys.modules.setdefault("torch.utils.tensorboard", tb)
    sys.path.insert(0, REF)
    import torch
    from torch.utils.data import DataLoader, TensorDataset

    torch.set_num_threads(1)
    from wtracker.neural.config import LOSSES, OPTIMIZERS, IOConfig
    from wtracker.neural.mlp import RMLP, WormPredictor
    from wtracker.neural.training import MLPTrainer

    out = {}
    # ---------------------------------------------------------------- part 1: three float64 steps per optimizer
    torch.manual_seed(0)
    io = IOConfig(LEARN["input_frames"], LEARN["pred_frames"])
    base = WormPredictor(RMLP(**SMALL), io).double()
    # fresh BatchNorm parameters are 1 / 0 and fresh statistics 0 / 1: move them off those values, so that a mix-up between them cannot pass
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for k, v in base.state_dict().items():
            if k.endswith(".1.weight") or k.endswith("running_var"):
                v.copy_(torch.rand(v.shape, generator=g, dtype=torch.float64) + 0.5)
            elif k.endswith(".1.bias") or k.endswith("running_mean"):
                v.copy_(torch.randn(v.shape, generator=g, dtype=torch.float64) * 0.3)
    init = {k: v.detach().clone() for k, v in base.state_dict().items()}
    rng = np.random.default_rng(2)
    X = rng.normal(0, 6, size=(33, 28))
    y = rng.normal(0, 2, size=(33, 8))
    lr, wd, loss = 1e-3, 1e-2, "mse"
    for k, v in init.items():
        out["init::" + k] = v.numpy()
    out.update(acts=np.array(["relu"] * (1 + SMALL["n_blocks"] * len(SMALL["block_dims"]))), X=X, y=y, lr=lr, weight_decay=wd, loss=loss)
    batch = (torch.tensor(X), torch.tensor(y))
    for name in sorted(OPTIMIZERS):
        model = WormPredictor(RMLP(**SMALL), io).double()
        model.load_state_dict(init)
        trainer = MLPTrainer(model, LOSSES[loss](), OPTIMIZERS[name](model.parameters(), lr=lr, weight_decay=wd), device=None, log=False)
        losses, ncs = [], []
        for step in range(3):
            model.train(True)
            r = trainer.train_batch(batch)
            losses.append(r.loss), ncs.append(r.num_correct)
            if step == 0:
                for k, p in model.named_parameters():
                    prev = out.setdefault("grad::" + k, p.grad.numpy().copy())
                    assert np.array_equal(prev, p.grad.numpy())
            for k, v in model.state_dict().items():
                out[f"{name}::state{step}::{k}"] = v.detach().numpy().copy()
        model.train(False)
        r = trainer.test_batch(batch)
        out[f"{name}::loss"], out[f"{name}::num_correct"] = np.array(losses), np.array(ncs)
        out[f"{name}::test_loss"], out[f"{name}::test_num_correct"] = r.loss, r.num_correct

    # ---------------------------------------------------------------- part 2: the distribution of a float32 fit over shuffle seeds
    track = synthetic_track(LEARN["track_frames"], LEARN["track_seed"])
    Xl, yl = pairs_from_track(track, LEARN["input_frames"], LEARN["pred_frames"])
    perm = torch.randperm(len(Xl), generator=torch.Generator().manual_seed(LEARN["split_seed"]))
    k = int(round(0.8 * len(Xl)))
    tr_idx, te_idx = perm[:k].numpy(), perm[k:].numpy()
    torch.manual_seed(3)
    init32 = {k_: v.detach().clone() for k_, v in WormPredictor(RMLP(**NOTEBOOK), io).state_dict().items()}
    for k_, v in init32.items():
        out["learn::init::" + k_] = v.numpy()
    final, first = [], []
    for seed in LEARN["seeds"]:
        model = WormPredictor(RMLP(**NOTEBOOK), io)
        model.load_state_dict(init32)
        trainer = MLPTrainer(model, LOSSES["mse"](), OPTIMIZERS["adam"](model.parameters(), lr=LEARN["lr"], weight_decay=LEARN["weight_decay"]), device=None, log=False)
        dl_train = DataLoader(TensorDataset(torch.tensor(Xl[tr_idx]), torch.tensor(yl[tr_idx])), batch_size=LEARN["batch_size"], shuffle=True,
                              generator=torch.Generator().manual_seed(seed))
        dl_test = DataLoader(TensorDataset(torch.tensor(Xl[te_idx]), torch.tensor(yl[te_idx])), batch_size=LEARN["batch_size"], shuffle=False)
        res = trainer.fit(dl_train, dl_test, LEARN["num_epochs"], print_every=0)
        nb = len(dl_test)
        final.append(float(np.mean(np.asarray(res.test_loss[-nb:], np.float32))))
        first.append(float(np.mean(np.asarray(res.test_loss[:nb], np.float32))))
        print(f"seed {seed}: validation loss {first[-1]:.4f} -> {final[-1]:.4f}")
    out.update({"learn::train_idx": tr_idx, "learn::test_idx": te_idx, "learn::final_val": np.array(final), "learn::first_val": np.array(first),
                "learn::n_pairs": len(Xl)})
    for k_ in ("lr", "weight_decay", "batch_size", "num_epochs", "track_frames", "track_seed", "input_frames", "pred_frames"):
        out["learn::" + k_] = np.asarray(LEARN[k_])
    path = os.path.join(HERE, "mlp_train.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; pairs", len(Xl), "train", len(tr_idx), "test", len(te_idx))


if __name__ == "__main__":
    main()
