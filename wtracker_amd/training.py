"""Training the ResMLP predictor on the device: a population of models, one workgroup each (wtk_mlp_trainer_*, csrc/mlp_train.hip).

Replaces predictor_training.ipynb -> MLPTrainer.fit (wtracker/neural/training.py:61-130,267-333) for RMLP models (wtracker/neural/mlp.py).  E = 1 is
MLPTrainer; E > 1 trains E seeds / learning rates / initialisations side by side, each of which `Replay.mlp` can score in the closed loop.

Stated deviations from the notebook: its exact shuffles (DataLoader's RandomSampler, random_split) are not reproduced — the order is a seeded
torch.randperm per epoch and model, or the caller's; the test set is walked unshuffled; there is no tensorboard and no torch.save checkpoint, the
best state is kept on the device instead.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Mapping, Optional, Sequence

import numpy as np

from . import hip
from .hip import WtkError
from .resmlp import FoldedResMLP, fold_state_dict

LOSSES = {"mse": 0, "l1": 1}
OPTIMIZERS = {"adam": 0, "adamw": 1, "sgd": 2, "rmsprop": 3}  # the keys of the reference's OPTIMIZERS (neural/config.py:28-33)
MAX_BATCH = 1024
LDS_STATE_FLOATS = 36864  # kTrainLdsFloats (csrc/mlp_train.hip): a model state above this trains from global memory
DEFAULT_MAX_BATCH = 256  # the reference's TrainConfig.batch_size (neural/config.py:67)
# the states a trainer keeps per model, by name -> `which` of wtk_mlp_trainer_get_state / _fold: the current one, the one of the epoch with the lowest
# validation loss, the one of the lowest score handed to keep_scored (fit(closed_loop=...): the closed-loop error)
STATE_SLOTS = {"current": 0, "best": 1, "scored": 4}


def state_slot(which) -> int:
    """`which` of the library for a name of STATE_SLOTS; True / False keep their meaning of state_dict(best=...): best / current."""
    if isinstance(which, (bool, np.bool_)):
        return 1 if which else 0
    if which not in STATE_SLOTS:
        raise ValueError(f"unknown state {which!r}: one of {sorted(STATE_SLOTS)}")
    return STATE_SLOTS[which]


@dataclass
class FitResult:
    """The reference's FitResult (neural/train_results.py): per-batch losses over all epochs, per-epoch accuracies in percent."""

    num_epochs: int
    train_loss: list = field(default_factory=list)
    train_acc: list = field(default_factory=list)
    test_loss: list = field(default_factory=list)
    test_acc: list = field(default_factory=list)
    closed_loop: list = field(default_factory=list)  # fit(closed_loop=...): the closed-loop objective after every epoch the model ran


def train_test_split(n: int, fraction: float = 0.8, seed: int = 42, device=None):
    """(train, test) int64 index tensors: a seeded permutation of range(n), the first round(fraction * n) rows train."""
    import torch

    g = torch.Generator().manual_seed(int(seed))
    perm = torch.randperm(int(n), generator=g)
    k = int(round(fraction * n))
    tr, te = perm[:k], perm[k:]
    return (tr.to(device), te.to(device)) if device is not None else (tr, te)


def _state_dict_of(model):
    """(state dict of numpy arrays, activations or None, input_frames, pred_frames) of a live WormPredictor or of a dict."""
    if isinstance(model, Mapping):
        sd = {k: np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v) for k, v in model.items() if k not in ("activations", "input_frames", "pred_frames")}
        acts = model.get("activations")
        return sd, (list(acts) if acts is not None else None), model.get("input_frames"), model.get("pred_frames")
    sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    acts = []
    for name, mod in model.named_modules():
        seq = getattr(mod, "mlp_layer", None)
        if seq is None:
            continue
        kind = type(list(seq.children())[-1]).__name__
        if kind not in ("ReLU", "Identity"):
            raise WtkError(f"ResMLP layer {name}: activation {kind} is not supported by the trainer (ReLU or none only)")
        acts.append("relu" if kind == "ReLU" else "none")
    io = getattr(model, "io_config", None)
    return sd, acts or None, getattr(io, "input_frames", None), getattr(io, "pred_frames", None)


def _layer_rows(sd, acts):
    """[(linear prefix, bn prefix or None, relu)] in execution order with the output layer last, n_blocks, layers_per_block."""
    import re

    if "model.input.mlp_layer.0.weight" not in sd:
        raise WtkError("ResMLP: the state dict has no input layer (model.input.mlp_layer.0.weight is missing)")
    n_blocks = len({int(m.group(1)) for k in sd for m in [re.match(r"model\.blocks\.(\d+)\.", k)] if m})
    per_block = len({int(m.group(1)) for k in sd for m in [re.match(r"model\.blocks\.0\.sequence\.(\d+)\.", k)] if m}) if n_blocks else 0
    prefixes = ["model.input.mlp_layer"] + [f"model.blocks.{b}.sequence.{l}.mlp_layer" for b in range(n_blocks) for l in range(per_block)]
    if acts is not None and len(acts) != len(prefixes):
        raise WtkError(f"ResMLP: {len(acts)} activations given for {len(prefixes)} layers")
    rows = []
    for i, p in enumerate(prefixes):
        bn = (p + ".1") if (p + ".1.weight") in sd else None
        act = acts[i] if acts is not None else ("relu" if bn else "none")
        if act not in ("relu", "none"):
            raise WtkError(f"ResMLP layer {p}: activation {act!r} is not supported by the trainer (ReLU or none only)")
        rows.append((p + ".0", bn, act == "relu"))
    rows.append(("model.output", None, False))
    return rows, n_blocks, per_block


class HipMLPTrainer:
    """E models of one structure trained side by side.  `models`: one or a list of live `WormPredictor`s, or state dicts (numpy / torch values under the
    reference's key names; optional entries "activations" — 'relu' / 'none' per MLPLayer —, "input_frames", "pred_frames").

    `max_batch` (default 256, at most 1024) is the largest batch_size any later call may use; it sizes the per-model activation scratch, allocated once
    (TrainScratch in csrc/mlp_train.hip) — the notebook's model: 2.9 MB per model at 128, 5.9 MB at 256, 23.6 MB at 1024 (E = 256: 6 GB)."""

    def __init__(self, models, loss_fn: str = "mse", optimizer: str = "adam", lr=1e-3, weight_decay=1e-5, max_batch: int = DEFAULT_MAX_BATCH, device: int = 0):
        import torch

        if loss_fn not in LOSSES:
            raise ValueError(f"loss_fn {loss_fn!r}: the trainer has mse and l1")
        if optimizer not in OPTIMIZERS:
            raise ValueError(f"optimizer {optimizer!r}: the trainer has {', '.join(OPTIMIZERS)}")
        if not 1 <= int(max_batch) <= MAX_BATCH:
            raise ValueError(f"batch_size must be in [1, {MAX_BATCH}], got {max_batch}")
        models = list(models) if isinstance(models, (list, tuple)) else [models]
        if not models:
            raise ValueError("no model given")
        parsed = [_state_dict_of(m) for m in models]
        sd0, acts, self.input_frames, self.pred_frames = parsed[0]
        self._rows, self.n_blocks, self.layers_per_block = _layer_rows(sd0, acts)
        self.activations = [("relu" if r else "none") for _, _, r in self._rows[:-1]]
        self.E = len(models)
        self.loss_fn, self.optimizer = loss_fn, optimizer
        shapes = [tuple(np.shape(sd0[p + ".weight"])) for p, _, _ in self._rows]
        self._shapes = {p: s for (p, _, _), s in zip(self._rows, shapes)}
        self._nbt0 = []
        states = []
        for sd, a, _, _ in parsed:
            rows = _layer_rows(sd, a)[0]
            if [(p, b, r) for p, b, r in rows] != self._rows or [tuple(np.shape(sd[p + ".weight"])) for p, _, _ in rows] != shapes:
                raise ValueError("all models of a trainer must have the same structure")
            states.append(self._pack(sd))
            self._nbt0.append({b: int(sd[b + ".num_batches_tracked"]) for _, b, _ in rows if b})
        state = np.ascontiguousarray(np.stack(states), dtype=np.float32)
        self.n_state = state.shape[1]
        self.n_train = sum(int(np.prod(s)) + s[0] + (2 * s[0] if b else 0) for s, (_, b, _) in zip(shapes, self._rows))
        self.in_dim, self.out_dim = shapes[0][1], shapes[-1][0]
        self.has_bn = any(b for _, b, _ in self._rows)
        larr = (hip._MlpTrainLayer * len(shapes))()
        for i, (s, (_, b, r)) in enumerate(zip(shapes, self._rows)):
            larr[i] = hip._MlpTrainLayer(s[1], s[0], int(r), int(bool(b)))
        desc = hip._MlpTrainerDesc(device, self.E, len(shapes), self.n_blocks, self.layers_per_block, LOSSES[loss_fn], OPTIMIZERS[optimizer], int(max_batch), larr,
                                   state.ctypes.data_as(C.POINTER(C.c_float)))
        self._layers = larr
        if self.library_state_floats() != (self.n_state, self.n_train):  # _pack names the keys, the library lays them out (state_layout, csrc/mlp_train.hip)
            raise WtkError(f"ResMLP trainer: the packed state has (n_state, n_train) = {(self.n_state, self.n_train)}, the library lays out {self.library_state_floats()}")
        self._h = C.c_void_p()
        hip._check(hip.load().wtk_mlp_trainer_create(C.byref(self._h), C.byref(desc)), "wtk_mlp_trainer_create")
        self.max_batch = int(max_batch)
        self._dev = torch.device("cuda", device)
        self._lr = self._per_model(lr, "lr")
        self._wd = self._per_model(weight_decay, "weight_decay")
        self.active = torch.ones(self.E, dtype=torch.int32, device=self._dev)

    # ------------------------------------------------------------------ plumbing
    def library_state_floats(self):
        """(n_state, n_train) of this structure as the library lays a state out (wtk_mlp_trainer_state_floats; needs no device)."""
        desc = hip._MlpTrainerDesc(0, self.E, len(self._layers), self.n_blocks, self.layers_per_block, 0, 0, 1, self._layers, None)
        n_train = C.c_int64()
        return int(hip.load().wtk_mlp_trainer_state_floats(C.byref(desc), C.byref(n_train))), int(n_train.value)

    def _per_model(self, v, name):
        import torch

        a = np.broadcast_to(np.asarray(v, dtype=np.float64), (self.E,)) if np.ndim(v) == 0 else np.asarray(v, dtype=np.float64)
        if a.shape != (self.E,):
            raise ValueError(f"{name}: a scalar or one value per model ({self.E}), got shape {a.shape}")
        return torch.from_numpy(np.array(a, dtype=np.float64)).to(self._dev)  # (a copy: broadcast_to's view is read-only)

    def _pack(self, sd) -> np.ndarray:
        parts = []
        for p, b, _ in self._rows:
            parts += [sd[p + ".weight"], sd[p + ".bias"]] + ([sd[b + ".weight"], sd[b + ".bias"]] if b else [])
        for _, b, _ in self._rows:
            if b:
                parts += [sd[b + ".running_mean"], sd[b + ".running_var"]]
        return np.concatenate([np.asarray(v, dtype=np.float32).ravel() for v in parts])

    def _unpack(self, flat: np.ndarray, trainable_only: bool = False) -> dict:
        """The reference's key names over one model's flat state (or, trainable_only, over a gradient / moment vector)."""
        out, off = {}, 0

        def take(key, shape):
            nonlocal off
            n = int(np.prod(shape))
            out[key] = flat[off:off + n].reshape(shape).copy()
            off += n

        for p, b, _ in self._rows:
            o, k = self._shape(p)
            take(p + ".weight", (o, k))
            take(p + ".bias", (o,))
            if b:
                take(b + ".weight", (o,))
                take(b + ".bias", (o,))
        if not trainable_only:
            for p, b, _ in self._rows:
                if b:
                    o = self._shape(p)[0]
                    take(b + ".running_mean", (o,))
                    take(b + ".running_var", (o,))
        assert off == flat.size, (off, flat.size)
        return out

    def _shape(self, p):
        return self._shapes[p]

    def _stream(self):
        import torch

        return C.c_void_p(torch.cuda.current_stream(self._dev).cuda_stream)

    def _xy(self, X, y):
        import torch

        for t, d, name in ((X, self.in_dim, "X"), (y, self.out_dim, "y")):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == d):
                raise ValueError(f"{name} must be a CUDA float32 tensor [n, {d}]")
        if X.shape[0] != y.shape[0] or X.shape[0] == 0:
            raise ValueError("X and y must have the same, positive number of rows")
        return X.contiguous(), y.contiguous()

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            hip.load().wtk_mlp_trainer_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ the four device calls
    def grad(self, X, y):
        """(loss float32 [E], gradients: list of {key: array} per model) of ONE batch in train mode; no step, no statistics update."""
        import torch

        X, y = self._xy(X, y)
        g = torch.empty((self.E, self.n_train), dtype=torch.float32, device=self._dev)
        loss = torch.empty(self.E, dtype=torch.float32, device=self._dev)
        with torch.cuda.device(self._dev):
            hip._check(hip.load().wtk_mlp_trainer_grad(self._h, hip._ptr(X), hip._ptr(y), int(X.shape[0]), hip._ptr(g), hip._ptr(loss), self._stream()), "wtk_mlp_trainer_grad")
        gh = g.cpu().numpy()
        return loss.cpu().numpy(), [self._unpack(gh[e], trainable_only=True) for e in range(self.E)]

    def step(self, X, y):
        """One optimizer step of every model on the batch (X, y): (loss float32 [E], num_correct int32 [E]) device tensors."""
        import torch

        X, y = self._xy(X, y)
        loss = torch.empty(self.E, dtype=torch.float32, device=self._dev)
        nc = torch.empty(self.E, dtype=torch.int32, device=self._dev)
        with torch.cuda.device(self._dev):
            hip._check(hip.load().wtk_mlp_trainer_step(self._h, hip._ptr(X), hip._ptr(y), int(X.shape[0]), hip._ptr(self._lr), hip._ptr(self._wd), hip._ptr(loss), hip._ptr(nc),
                                                       self._stream()), "wtk_mlp_trainer_step")
        return loss, nc

    def train_epoch(self, X, y, order=None, batch_size: int = 128, active=None, check_order: bool = True):
        """One epoch of every active model in one launch.  `order`: int32 device tensor [E, n] (or [n], shared), None = rows in order.  Returns per-batch
        (loss float32 [E, n_batches], num_correct int32 [E, n_batches]) device tensors (rows of inactive models are NaN / 0).  A caller's order is checked
        for row numbers outside [0, n) (one readback; check_order=False skips it)."""
        import torch

        X, y = self._xy(X, y)
        n = int(X.shape[0])
        if order is not None:
            order = order.to(self._dev, torch.int32)
            if order.dim() == 1:
                order = order.unsqueeze(0).expand(self.E, n)
            if tuple(order.shape) != (self.E, n):
                raise ValueError(f"order must be [{self.E}, {n}] or [{n}]")
            order = order.contiguous()
            if check_order and (int(order.min().item()) < 0 or int(order.max().item()) >= n):  # (the kernel would clamp such an entry: duplicated rows, no error)
                raise ValueError(f"order holds row numbers outside [0, {n})")
        nb = (n + int(batch_size) - 1) // max(int(batch_size), 1)
        loss = torch.full((self.E, max(nb, 1)), float("nan"), dtype=torch.float32, device=self._dev)
        nc = torch.zeros((self.E, max(nb, 1)), dtype=torch.int32, device=self._dev)
        with torch.cuda.device(self._dev):
            hip._check(hip.load().wtk_mlp_trainer_train_epoch(self._h, hip._ptr(X), hip._ptr(y), n, hip._ptr(order), int(batch_size), hip._ptr(self._lr), hip._ptr(self._wd),
                                                              hip._ptr(active), hip._ptr(loss), hip._ptr(nc), self._stream()), "wtk_mlp_trainer_train_epoch")
        return loss, nc

    def test_epoch(self, X, y, batch_size: int = 128, patience: Optional[int] = None, track_best: bool = False, active=None, return_pred: bool = False,
                   reset_best: bool = False):
        """MLPTrainer.test_epoch for every active model in one launch: per-batch (loss, num_correct) device tensors [E, n_batches] (+ predictions [E, n, out]).
        track_best keeps the early-stopping state of Trainer.fit on the device; with `patience` it clears `active[e]` when model e runs out of it;
        reset_best forgets the state earlier epochs left first (the first test epoch of a fit)."""
        import torch

        X, y = self._xy(X, y)
        n = int(X.shape[0])
        nb = (n + int(batch_size) - 1) // max(int(batch_size), 1)
        loss = torch.full((self.E, max(nb, 1)), float("nan"), dtype=torch.float32, device=self._dev)
        nc = torch.zeros((self.E, max(nb, 1)), dtype=torch.int32, device=self._dev)
        pred = torch.zeros((self.E, n, self.out_dim), dtype=torch.float32, device=self._dev) if return_pred else None
        with torch.cuda.device(self._dev):
            hip._check(hip.load().wtk_mlp_trainer_eval_epoch(self._h, hip._ptr(X), hip._ptr(y), n, int(batch_size), int(patience or 0), (2 if reset_best else 1) if track_best else 0, hip._ptr(active),
                                                             hip._ptr(loss), hip._ptr(nc), hip._ptr(pred), self._stream()), "wtk_mlp_trainer_eval_epoch")
        return (loss, nc, pred) if return_pred else (loss, nc)

    # ------------------------------------------------------------------ fit
    def fit(self, X_train, y_train, X_test, y_test, num_epochs: int, batch_size: int = 128, early_stopping: Optional[int] = None, shuffle: bool = True, seed: int = 42,
            order=None, closed_loop=None, closed_loop_objective: str = "trimmed_bbox_error", max_speed: float = 0.9) -> list:
        """Trainer.fit for every model: one train launch and one test launch per epoch, one small readback per epoch (the `active` flags).  `order`: a callable
        epoch -> int32 [E, n] / [n] tensor, or a fixed tensor, instead of the seeded per-epoch, per-model torch.randperm.  Returns one FitResult per model.
        As the reference's fit, every call starts its early stopping afresh (best_val_loss = None); the parameters and optimizer moments carry on.

        `closed_loop`: a `Replay`.  After every test epoch the population is folded and replayed on it (Replay.mlp_population, Replay.objective with
        `closed_loop_objective`, a precise one where frames are attached) and the state with the lowest score so far is kept per model (keep_scored, with the
        epoch's `active` flags as they were before the test epoch: a model is scored for every epoch it trained): three more enqueues, no host wait.
        The scores come back once, at the end, in FitResult.closed_loop; state_dict / folded(best="scored") read the kept state.  Early stopping stays
        keyed to the validation loss.  The scores kept by earlier fits or keep_scored calls stay in the comparison."""
        import torch

        n, n_test = int(X_train.shape[0]), int(X_test.shape[0])
        gen = torch.Generator().manual_seed(int(seed))
        self.active.fill_(1)
        tr_loss, tr_nc, te_loss, te_nc, ran, cl = [], [], [], [], [], []
        for epoch in range(int(num_epochs)):
            own = order is None
            if order is not None:
                o = order(epoch) if callable(order) else order
            elif shuffle:
                o = torch.stack([torch.randperm(n, generator=gen) for _ in range(self.E)]).to(torch.int32)
            else:
                o = None
            was = self.active.clone()
            a, b = self.train_epoch(X_train, y_train, o, batch_size, active=self.active, check_order=not own)
            c, d = self.test_epoch(X_test, y_test, batch_size, patience=early_stopping, track_best=True, active=self.active, reset_best=epoch == 0)
            tr_loss.append(a), tr_nc.append(b), te_loss.append(c), te_nc.append(d), ran.append(was)
            if closed_loop is not None:
                score = closed_loop.objective(closed_loop.mlp_population(self, max_speed=max_speed, which="current"), closed_loop_objective)
                self.keep_scored(score, active=was)
                cl.append(score)
            if early_stopping is not None and not bool(self.active.any().item()):  # the one readback of the epoch
                break
        ran = torch.stack(ran).cpu().numpy().astype(bool)  # [epochs, E]
        tr_loss, te_loss = torch.stack(tr_loss).cpu().numpy(), torch.stack(te_loss).cpu().numpy()
        tr_nc, te_nc = torch.stack(tr_nc).cpu().numpy(), torch.stack(te_nc).cpu().numpy()
        cl = torch.stack(cl).cpu().numpy() if cl else None  # [epochs, E]
        results = []
        for e in range(self.E):
            r = FitResult(int(ran[:, e].sum()))
            for ep in np.nonzero(ran[:, e])[0]:
                r.train_loss += [float(v) for v in tr_loss[ep, e]]
                r.test_loss += [float(v) for v in te_loss[ep, e]]
                r.train_acc.append(100.0 * float(tr_nc[ep, e].sum()) / n)
                r.test_acc.append(100.0 * float(te_nc[ep, e].sum()) / n_test)
                if cl is not None:
                    r.closed_loop.append(float(cl[ep, e]))
            results.append(r)
        return results

    # ------------------------------------------------------------------ reading the models back
    def _get(self, which: int):
        per = self.n_state if which in (0, 1, 4) else self.n_train
        buf = np.empty((self.E, per), dtype=np.float32)
        steps = np.empty(self.E, dtype=np.int32)
        hip._check(hip.load().wtk_mlp_trainer_get_state(self._h, which, hip._ptr(buf), hip._ptr(steps), self._stream()), "wtk_mlp_trainer_get_state")
        return buf, steps

    def state_dict(self, e: int = 0, best=False) -> dict:
        """Model e under the reference's key names (numpy arrays): what fold_state_dict, a real WormPredictor's load_state_dict (through torch.as_tensor) and
        Replay.mlp (through .folded) take.  best: the state of the epoch with the lowest validation loss (the initial state before the first test epoch);
        best="scored": the state of the lowest score keep_scored was handed (the initial state before the first score)."""
        buf, steps = self._get(state_slot(best))
        sd = self._unpack(buf[e])
        for b, n0 in self._nbt0[e].items():
            sd[b + ".num_batches_tracked"] = np.asarray(n0 + int(steps[e]), dtype=np.int64)
        order = []
        for p, b, _ in self._rows:
            order += [p + ".weight", p + ".bias"] + ([b + ".weight", b + ".bias", b + ".running_mean", b + ".running_var", b + ".num_batches_tracked"] if b else [])
        return {k: sd[k] for k in order}

    # ------------------------------------------------------------------ the population as inference parameters; the best state by a caller's score
    def blob_structure(self) -> tuple:
        """(wtk_mlp_train_layer array, n_blocks, layers_per_block) of this structure, as wtk_mlp_folded_floats / wtk_replay_mlp_targets take it."""
        return self._layers, self.n_blocks, self.layers_per_block

    def folded_blob(self, which="current"):
        """Every model's padded inference blob as a device float32 [E, F] tensor (wtk_mlp_trainer_fold: BatchNorm folded on the device with
        resmlp._fold's bits, wtk_mlp_create's layout).  One launch on the current stream; nothing leaves the device, nothing is waited for."""
        import torch

        w = state_slot(which)
        F = hip.mlp_folded_floats(*self.blob_structure())
        if F < 0:
            raise WtkError("ResMLP trainer: the structure has no inference blob (wtk_mlp_folded_floats)")
        blob = torch.empty((self.E, F), dtype=torch.float32, device=self._dev)
        with torch.cuda.device(self._dev):
            hip._check(hip.load().wtk_mlp_trainer_fold(self._h, w, hip._ptr(blob), self._stream()), "wtk_mlp_trainer_fold")
        return blob

    def keep_scored(self, score, active=None) -> None:
        """Per model with active[e] != 0 (None: all): where score[e] (device float64 [E], lower is better) is finite and strictly below the kept one, or
        none is kept yet, keep the current state as the "scored" state.  One launch; the first call allocates the slot (E x n_state floats)."""
        import torch

        if not (isinstance(score, torch.Tensor) and score.is_cuda and score.dtype == torch.float64 and tuple(score.shape) == (self.E,) and score.is_contiguous()):
            raise ValueError(f"score must be a contiguous CUDA float64 tensor [{self.E}]")
        if active is not None and not (active.is_cuda and active.dtype == torch.int32 and tuple(active.shape) == (self.E,) and active.is_contiguous()):
            raise ValueError(f"active must be a contiguous CUDA int32 tensor [{self.E}]")
        with torch.cuda.device(self._dev):
            hip._check(hip.load().wtk_mlp_trainer_keep_scored(self._h, hip._ptr(score), hip._ptr(active), self._stream()), "wtk_mlp_trainer_keep_scored")

    def scores(self):
        """(kept score float64 [E], NaN where none is kept; has-score int32 [E]) as numpy arrays."""
        best, has = np.empty(self.E, np.float64), np.empty(self.E, np.int32)
        hip._check(hip.load().wtk_mlp_trainer_get_scores(self._h, hip._ptr(best), hip._ptr(has), self._stream()), "wtk_mlp_trainer_get_scores")
        return best, has

    def moments(self, e: int = 0):
        """(first, second) optimizer moment of model e as {key: array} (exp_avg, exp_avg_sq of Adam / AdamW; square_avg of RMSprop is the second), steps taken."""
        (m, steps), (v, _) = self._get(2), self._get(3)
        return self._unpack(m[e], True), self._unpack(v[e], True), int(steps[e])

    def stopping(self):
        """(best validation loss float32 [E], has-best int32 [E], epochs without improvement int32 [E]) as numpy arrays."""
        best, has, cnt = np.empty(self.E, np.float32), np.empty(self.E, np.int32), np.empty(self.E, np.int32)
        hip._check(hip.load().wtk_mlp_trainer_get_stopping(self._h, hip._ptr(best), hip._ptr(has), hip._ptr(cnt), self._stream()), "wtk_mlp_trainer_get_stopping")
        return best, has, cnt

    def folded(self, e: int = 0, best=False, input_frames: Optional[Sequence[int]] = None, pred_frames: Optional[Sequence[int]] = None) -> FoldedResMLP:
        xi = input_frames if input_frames is not None else (self.input_frames if self.input_frames is not None else [])
        yi = pred_frames if pred_frames is not None else (self.pred_frames if self.pred_frames is not None else [])
        return fold_state_dict(self.state_dict(e, best), list(xi), list(yi), self.activations)
