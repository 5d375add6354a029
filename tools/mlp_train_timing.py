#!/usr/bin/env python3
"""Timing of the ResMLP trainer (wtracker_amd.training.HipMLPTrainer) against what a user would otherwise run: the reference's
MLPTrainer.train_batch loop (zero_grad, forward, MSELoss, backward, Adam step, num_correct; wtracker/neural/training.py:304-319) executed by torch on the
same device.  One process, one device; prints one JSON line.

  model     the notebook's: 28 -> 80, four blocks [40, 10, 40, 80] of Linear + BatchNorm1d + ReLU, out 8 (33 968 parameters); batch --batch (128)
  data      --rows seeded float32 rows (2048: 16 batches per epoch)
  device    per population size E of --experiments: one `step` (one batch of all E models, one launch) and one `train_epoch` (all batches of all E
            models, one launch), milliseconds by device events, median of --reps after one warm-up
  torch     one model: a train_batch step and an epoch of them, same events (host-bound: a step is a few hundred dependent launches).  A population of E
            is E such runs one after the other (`torch_population_*` = E x the measured single-model time, not measured separately)
Usage: python tools/mlp_train_timing.py [--experiments 1 16 256] [--batch 128] [--rows 2048] [--reps 5]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NOTEBOOK = dict(in_dim=28, block_in_dim=80, block_dims=[40, 10, 40, 80], n_blocks=4, out_dim=8)


def _time_ms(fn, reps: int) -> float:
    import torch

    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def torch_rmlp(in_dim, block_in_dim, block_dims, n_blocks, out_dim):
    """The notebook's RMLP with the reference's module and key names (Linear + BatchNorm1d + ReLU layers, h + block(h), a Linear output)."""
    from torch import nn

    class Layer(nn.Module):
        def __init__(self, k, n):
            super().__init__()
            self.mlp_layer = nn.Sequential(nn.Linear(k, n), nn.BatchNorm1d(n), nn.ReLU())

        def forward(self, x):
            return self.mlp_layer(x)

    class Block(nn.Module):
        def __init__(self):
            super().__init__()
            dims = [block_in_dim] + list(block_dims)
            self.sequence = nn.Sequential(*[Layer(dims[i], dims[i + 1]) for i in range(len(block_dims))])

        def forward(self, x):
            return self.sequence(x)

    class RMLP(nn.Module):
        def __init__(self):
            super().__init__()
            self.input = Layer(in_dim, block_in_dim)
            self.blocks = nn.ModuleList([Block() for _ in range(n_blocks)])
            self.output = nn.Linear(block_dims[-1], out_dim)

        def forward(self, x):
            x = self.input(x)
            for b in self.blocks:
                x = x + b(x)
            return self.output(x)

    class Predictor(nn.Module):
        def __init__(self):
            super().__init__()
            self.model = RMLP()

        def forward(self, x):
            return self.model(x)

    return Predictor()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--experiments", type=int, nargs="+", default=[1, 16, 256])
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()

    import torch

    from wtracker_amd import hip
    from wtracker_amd.training import LDS_STATE_FLOATS, HipMLPTrainer

    if hip.device_count() < 1:
        raise SystemExit("mlp_train_timing: no HIP device visible (nothing is timed on the CPU)")
    torch.manual_seed(0)
    B, n = args.batch, args.rows
    X = torch.randn((n, NOTEBOOK["in_dim"]), device="cuda") * 6
    y = torch.randn((n, NOTEBOOK["out_dim"]), device="cuda") * 2
    net = torch_rmlp(**NOTEBOOK).cuda()
    init = dict({k: v.detach().cpu().numpy() for k, v in net.state_dict().items()}, activations=["relu"] * 17)
    loss_fn = torch.nn.MSELoss()
    opt = torch.optim.Adam(net.parameters(), lr=1e-3, weight_decay=1e-5)
    net.train(True)

    def train_batch(xb, yb):  # MLPTrainer.train_batch, the .item() calls of _make_batch_result included
        opt.zero_grad()
        pred = net(xb)
        loss = loss_fn(pred, yb)
        loss.backward()
        opt.step()
        num_correct = torch.sum((pred - yb).norm(dim=1) < 1.0)
        return float(loss.item()), int(num_correct.item())

    def torch_epoch():
        for b0 in range(0, n, B):
            train_batch(X[b0:b0 + B], y[b0:b0 + B])

    out = dict(model="28-80-[40,10,40,80]x4-8", parameters=sum(p.numel() for p in net.parameters()), batch=B, rows=n, batches_per_epoch=-(-n // B), reps=args.reps,
               torch_step_ms=_time_ms(lambda: train_batch(X[:B], y[:B]), args.reps), torch_epoch_ms=_time_ms(torch_epoch, args.reps), cases=[])
    for E in args.experiments:
        t = HipMLPTrainer([init] * E, max_batch=B)
        xb, yb = X[:B].contiguous(), y[:B].contiguous()
        case = dict(experiments=E, lds=bool(t.n_state <= LDS_STATE_FLOATS), step_ms=_time_ms(lambda: t.step(xb, yb), args.reps),
                    epoch_ms=_time_ms(lambda: t.train_epoch(X, y, None, batch_size=B), args.reps),
                    eval_epoch_ms=_time_ms(lambda: t.test_epoch(X, y, batch_size=B), args.reps))
        case["epoch_ms_per_step"] = case["epoch_ms"] / out["batches_per_epoch"]
        case["torch_population_step_ms"] = E * out["torch_step_ms"]
        case["torch_population_epoch_ms"] = E * out["torch_epoch_ms"]
        case["torch_over_device_epoch"] = case["torch_population_epoch_ms"] / case["epoch_ms"]
        loss, _ = t.step(xb, yb)
        case["finite"] = bool(torch.isfinite(loss).all().item())
        out["cases"].append(case)
        t.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
