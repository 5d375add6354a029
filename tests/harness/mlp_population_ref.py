"""Host restatements for the population path of the ResMLP, none of them the code under test:

  the fold         wtracker_amd.resmlp.fold_state_dict (the reference of the issue: what Replay.mlp has always handed to wtk_mlp_create), then the padded
                   packing of wtk_mlp_create restated here in numpy: per layer W [ceil16(out)][ceil4(in)], zero padded, then b [ceil16(out)]
  the state        the trainer's unfolded layout restated from its description in include/wtk_hip.h: per layer W, b, [gamma, beta], then per BatchNorm
                   layer running_mean, running_var
  keep_scored      the rule of wtk_mlp_trainer_keep_scored as a few lines of Python
  the track        a synthetic worm track with the defects the gather has to survive
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

from wtracker_amd import resmlp

from . import mlp_ref


def _c(v, m):
    return (v + m - 1) // m * m


def pack(layers) -> np.ndarray:
    """The padded blob of folded layers [(W, b, relu)]."""
    parts = []
    for w, b, _ in layers:
        n, k = w.shape
        wp = np.zeros((_c(n, 16), _c(k, 4)), np.float32)
        wp[:n, :k] = w
        bp = np.zeros(_c(n, 16), np.float32)
        bp[:n] = b
        parts += [wp.ravel(), bp]
    blob = np.concatenate(parts)
    assert blob.size % 4 == 0 and blob.size == mlp_ref.blob_floats(layers)
    return blob


def padding_mask(layers) -> np.ndarray:
    """True at every float of the blob that is padding."""
    parts = []
    for w, _, _ in layers:
        n, k = w.shape
        wm = np.ones((_c(n, 16), _c(k, 4)), bool)
        wm[:n, :k] = False
        bm = np.ones(_c(n, 16), bool)
        bm[:n] = False
        parts += [wm.ravel(), bm]
    return np.concatenate(parts)


def fold_blob(sd, acts) -> np.ndarray:
    """The reference: resmlp.fold_state_dict, packed."""
    return pack(resmlp.fold_state_dict(sd, [], [], list(acts)).layers)


def rows(sd, acts):
    """([(linear prefix, bn prefix or None, relu, in, out)] with the output layer last, n_blocks, layers_per_block)."""
    prefixes, n_blocks, per_block = mlp_ref._structure(sd)
    out = []
    for p, a in zip(prefixes, acts):
        n, k = np.shape(sd[p + ".0.weight"])
        out.append((p + ".0", (p + ".1") if (p + ".1.running_mean") in sd else None, a == "relu", k, n))
    n, k = np.shape(sd["model.output.weight"])
    out.append(("model.output", None, False, k, n))
    return out, n_blocks, per_block


def pack_state(sd, acts) -> np.ndarray:
    r, _, _ = rows(sd, acts)
    parts = []
    for p, b, _, _, _ in r:
        parts += [sd[p + ".weight"], sd[p + ".bias"]] + ([sd[b + ".weight"], sd[b + ".bias"]] if b else [])
    for _, b, _, _, _ in r:
        if b:
            parts += [sd[b + ".running_mean"], sd[b + ".running_var"]]
    return np.concatenate([np.asarray(v, np.float32).ravel() for v in parts])


def bn_prefixes(sd):
    return sorted(k[: -len(".running_var")] for k in sd if k.endswith(".running_var"))


def with_variances(sd, values=(0.0, 1e-12, 1e6)):
    """A copy whose BatchNorm layers carry the given running_var values in their first channels (as many as fit)."""
    sd = {k: np.array(v) for k, v in sd.items()}
    for p in bn_prefixes(sd):
        v = sd[p + ".running_var"]
        v[: min(len(values), v.size)] = np.asarray(values, np.float32)[: v.size]
    return sd


def with_cancelling_beta(sd):
    """A copy whose beta is minus the float32 value of (b - mean) s, so that b' is what the two roundings of the product leave: a fused multiply-add
    keeps the product's low bits and lands elsewhere (the class of defect of the trainer's weight-decay term)."""
    sd = {k: np.array(v) for k, v in sd.items()}
    for p in bn_prefixes(sd):
        lin = p[:-2] + ".0"
        f = lambda k: np.asarray(sd[k], np.float64)  # noqa: E731
        s = f(p + ".weight") / np.sqrt(f(p + ".running_var") + 1e-5)
        sd[p + ".bias"] = (-((f(lin + ".bias") - f(p + ".running_mean")) * s)).astype(np.float32)
    return sd


def fused_biases(sd) -> dict:
    """bn prefix -> b' as a fused multiply-add would give it: (b - mean) s + beta with ONE rounding to float64 (exact rationals), cast to float32."""
    out = {}
    for p in bn_prefixes(sd):
        lin = p[:-2] + ".0"
        f = lambda k: np.asarray(sd[k], np.float64)  # noqa: E731
        s = f(p + ".weight") / np.sqrt(f(p + ".running_var") + 1e-5)
        d = f(lin + ".bias") - f(p + ".running_mean")
        vals = [float(Fraction(float(di)) * Fraction(float(si)) + Fraction(float(bi))) if math.isfinite(si) and math.isfinite(di) else float("nan")
                for di, si, bi in zip(d, s, f(p + ".bias"))]
        out[p] = np.asarray(vals, np.float64).astype(np.float32)
    return out


def keep_scored_model(states, steps, score, active, kept):
    """One call of the rule on host arrays.  kept: dict(state [E, n], steps [E], score [E], has [E]), updated in place."""
    for e in range(len(score)):
        if active is not None and not active[e]:
            continue
        s = float(score[e])
        if math.isfinite(s) and (not kept["has"][e] or s < kept["score"][e]):
            kept["state"][e], kept["steps"][e], kept["score"][e], kept["has"][e] = states[e], steps[e], s, 1


def synthetic_track(n_frames: int, seed: int = 0, nan_rows=(), inf_rows=()):
    """float64 [n_frames, 4] xywh of a slowly wandering worm; `nan_rows` are missed detections, `inf_rows` get an infinite width."""
    rng = np.random.default_rng(seed)
    xy = np.array([900.0, 700.0]) + np.cumsum(rng.normal(0, 1.5, size=(n_frames, 2)), axis=0)
    wh = rng.uniform(18, 30, size=(n_frames, 2))
    t = np.concatenate([xy, wh], axis=1)
    t[list(nan_rows)] = np.nan
    t[list(inf_rows), 2] = np.inf
    return t
