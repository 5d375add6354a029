"""A ResMLP reference the library does not share, and the yardstick the device kernel is held to.

`wtracker_amd.resmlp` folds BatchNorm into the Linear before the device sees a weight; the oracle (oracle/resmlp_oracle.c) runs the same
folded layers.  This module never folds: it walks the reference's *state dict* (keys `model.input.mlp_layer.{0,1}.*`,
`model.blocks.{b}.sequence.{l}.mlp_layer.{0,1}.*`, `model.output.*`) as Linear -> BatchNorm1d (eval) -> ReLU with `h + block(h)`, once in
float64 (the truth) and once in float32 with every dot product accumulated one k at a time (what an honest fp32 implementation costs).

    tolerance = 8 x max |forward32_seq - forward64|      one scalar per (network, input set), from the reference alone

Other fp32 summation orders (groups of four, BLAS) land at 0.5-1.3x of that deviation and folding adds one rounding per weight, which the
factor 8 covers; activations cut to 13 mantissa bits land 16-100x above the tolerance on the networks of ARCHS (tests/test_mlp_ref.py plants
that and three other defects and checks that each one fails).
"""
from __future__ import annotations

import re
from dataclasses import dataclass

import numpy as np

BN_EPS = 1e-5  # torch.nn.BatchNorm1d default
TOL_FACTOR = 8.0
LDS_PARAM_FLOATS = 32768 - 64  # kMlpLdsParams (csrc/mlp.hip): a padded blob above this runs from global memory
MAX_LAYERS, MAX_DIM, MAX_INPUT_FRAMES = 64, 128, 16  # kMlpMaxLayers, kMlpMaxDim, kMlpMaxInputFrames

# name -> RMLP constructor arguments, and the parameter path the padded blob size puts the handle on.  Every row is there for a reason:
#   no-blocks        n_blocks = 0: input layer straight into the output layer
#   one-slice-edge   in_pad = 64 exactly: the last shape whose K loop runs one 64-deep slice
#   two-slices       in_pad = 68: second slice with a single live MFMA, 60 over-read floats behind it
#   wide-lds/-global in_pad = 128 (two full slices) on either side of the LDS limit
#   ragged-global    widths that are no multiple of 16 (padded output columns) read from global memory
#   hourglass(-lds)  128 -> 8 -> 128: stale columns of a wider earlier layer sit next to the live ones in both ping-pong buffers; 16 input
#                    frames, three predicted frames.  The issue's shape is over the LDS limit, the 112-wide one just under it
#   odd-pingpong     three layers per block: the block's output is in the other ping-pong buffer than with four
#   none-in-block    a layer without ReLU / BatchNorm inside every block (and, as RMLP builds it, as the input layer)
#   tiny-in          one input frame and the most layers a handle admits
ARCHS = {
    "no-blocks": dict(in_dim=28, block_in_dim=40, block_dims=[], block_nonlins=["relu"], n_blocks=0, out_dim=2, path="lds"),
    "one-slice-edge": dict(in_dim=28, block_in_dim=64, block_dims=[64], block_nonlins=["relu"], n_blocks=2, out_dim=2, path="lds"),
    "two-slices": dict(in_dim=28, block_in_dim=68, block_dims=[68], block_nonlins=["relu"], n_blocks=1, out_dim=2, path="lds"),
    "wide-lds": dict(in_dim=28, block_in_dim=128, block_dims=[128], block_nonlins=["relu"], n_blocks=1, out_dim=2, path="lds"),
    "wide-global": dict(in_dim=28, block_in_dim=128, block_dims=[128], block_nonlins=["relu"], n_blocks=2, out_dim=2, path="global"),
    "ragged-global": dict(in_dim=28, block_in_dim=100, block_dims=[72, 100], block_nonlins=["relu", "relu"], n_blocks=2, out_dim=2, path="global"),
    "hourglass": dict(in_dim=64, block_in_dim=96, block_dims=[128, 8, 128, 96], block_nonlins=["relu"] * 4, n_blocks=1, out_dim=6, path="global"),
    "hourglass-lds": dict(in_dim=64, block_in_dim=96, block_dims=[112, 8, 112, 96], block_nonlins=["relu"] * 4, n_blocks=1, out_dim=6, path="lds"),
    "odd-pingpong": dict(in_dim=28, block_in_dim=40, block_dims=[24, 56, 40], block_nonlins=["relu"] * 3, n_blocks=3, out_dim=2, path="lds"),
    "none-in-block": dict(in_dim=28, block_in_dim=60, block_dims=[20, 60], block_nonlins=["none", "relu"], n_blocks=2, out_dim=2, path="lds"),
    "tiny-in": dict(in_dim=4, block_in_dim=16, block_dims=[16], block_nonlins=["relu"], n_blocks=62, out_dim=2, path="lds"),
}
EXPECTED_BLOB = {"no-blocks": 2048, "wide-lds": 22288, "wide-global": 38800, "ragged-global": 37376, "tiny-in": 17216}  # the figures of the issue


def arch_args(name: str) -> dict:
    return {k: v for k, v in ARCHS[name].items() if k != "path"}


def _structure(sd):
    """(prefixes of the MLPLayers in execution order, n_blocks, layers_per_block) read off the keys."""
    n_blocks = len({int(m.group(1)) for k in sd for m in [re.match(r"model\.blocks\.(\d+)\.", k)] if m})
    per_block = len({int(m.group(1)) for k in sd for m in [re.match(r"model\.blocks\.0\.sequence\.(\d+)\.", k)] if m}) if n_blocks else 0
    prefixes = ["model.input.mlp_layer"] + [f"model.blocks.{b}.sequence.{l}.mlp_layer" for b in range(n_blocks) for l in range(per_block)]
    return prefixes, n_blocks, per_block


def _mlp_layer_params(rng, prefix, k, n, nonlin, batch_norm, gain):
    """Linear(k, n) [+ BatchNorm1d(n)] as MLPLayer lays it out: the BatchNorm exists when batch_norm and the layer has a nonlinearity."""
    sd = {prefix + ".0.weight": (rng.normal(0, 1, size=(n, k)) * gain / np.sqrt(k)).astype(np.float32),
          prefix + ".0.bias": rng.normal(0, 0.3, size=n).astype(np.float32)}
    if batch_norm and nonlin not in ("none", None):
        sd[prefix + ".1.weight"] = rng.uniform(0.5, 1.5, size=n).astype(np.float32)
        sd[prefix + ".1.bias"] = rng.normal(0, 0.3, size=n).astype(np.float32)
        sd[prefix + ".1.running_mean"] = rng.normal(0, 0.5, size=n).astype(np.float32)
        sd[prefix + ".1.running_var"] = rng.uniform(0.3, 3.0, size=n).astype(np.float32)
        sd[prefix + ".1.num_batches_tracked"] = np.asarray(1000, dtype=np.int64)
    return sd


def random_rmlp(in_dim, block_in_dim, block_dims, block_nonlins, n_blocks, out_dim, batch_norm=True, seed=0):
    """State dict of RMLP(block_in_dim, block_dims, block_nonlins, n_blocks, out_dim, in_dim, batch_norm) with random parameters, and the
    activation ('relu' / 'none') of every MLPLayer in execution order.  As in RMLP the input layer takes block_nonlins[0].  With no block
    (block_dims = []) the output layer reads the residual width."""
    assert in_dim is not None and len(block_nonlins) >= 1 and (n_blocks == 0 or len(block_nonlins) == len(block_dims))
    assert all(a in ("relu", "none") for a in block_nonlins)
    rng = np.random.default_rng(seed)
    # the residual stream grows with every block: keep a deep stack (62 blocks) inside fp32's comfortable range
    block_gain = min(1.0, 2.0 / np.sqrt(max(n_blocks, 1)))
    sd = _mlp_layer_params(rng, "model.input.mlp_layer", in_dim, block_in_dim, block_nonlins[0], batch_norm, 1.0 / 6.0)
    acts = [block_nonlins[0]]
    for b in range(n_blocks):
        k = block_in_dim
        for l, n in enumerate(block_dims):
            sd.update(_mlp_layer_params(rng, f"model.blocks.{b}.sequence.{l}.mlp_layer", k, n, block_nonlins[l], batch_norm, block_gain))
            acts.append(block_nonlins[l])
            k = n
    res = block_dims[-1] if n_blocks else block_in_dim
    assert res == block_in_dim, "a block must return to the residual width"
    sd["model.output.weight"] = (rng.normal(0, 1, size=(out_dim, res)) / np.sqrt(res)).astype(np.float32)
    sd["model.output.bias"] = rng.normal(0, 0.3, size=out_dim).astype(np.float32)
    y = forward64(sd, acts, np.random.default_rng(seed + 1).normal(0, 6, size=(256, in_dim)))
    top = float(np.abs(y).max())
    assert np.isfinite(y).all() and 1e-2 <= top <= 1e3, f"random_rmlp: max|y| = {top:g} outside [1e-2, 1e3]"
    return sd, acts


def matrix_network(name: str, n_samples: int = 257):
    """(state dict, activations, x) of a row of ARCHS: fixed seeds, n_samples rows of N(0, 6^2) and one all-zero row, read-only."""
    i = list(ARCHS).index(name)
    sd, acts = random_rmlp(**arch_args(name), seed=100 + i)
    k = ARCHS[name]["in_dim"]
    x = np.concatenate([np.random.default_rng(7 + i).normal(0, 6, size=(n_samples, k)), np.zeros((1, k))]).astype(np.float32)
    for v in (x, *sd.values()):
        v.setflags(write=False)
    return sd, acts, x


def fixture_network(path):
    """(state dict, activations) of a shipped predictor fixture (tests/golden/resmlp_*.npz): every MLPLayer is ReLU with BatchNorm."""
    z = np.load(path)
    sd = {k[4:]: z[k] for k in z.files if k.startswith("sd::")}
    return sd, ["relu"] * len(_structure(sd)[0])


# ---------------------------------------------------------------------------------------------------------------------------------
# the unfolded forward pass
def _dot64(x, w):
    return x @ w.T


def _dot32_seq(x, w):
    acc = np.zeros((x.shape[0], w.shape[0]), np.float32)
    for k in range(w.shape[1]):  # one k at a time: every product and every add rounds to fp32
        acc += x[:, k, None] * w[None, :, k]
    return acc


def _dot32_group4(x, w):
    acc = np.zeros((x.shape[0], w.shape[0]), np.float32)
    for k0 in range(0, w.shape[1], 4):  # the four products of a group are summed first, then added to the running sum
        part = np.zeros_like(acc)
        for k in range(k0, min(k0 + 4, w.shape[1])):
            part += x[:, k, None] * w[None, :, k]
        acc += part
    return acc


def cut_mantissa(a, bits=13):
    """float32 values truncated to `bits` explicit mantissa bits."""
    a = np.ascontiguousarray(a, np.float32)
    return (a.view(np.uint32) & np.uint32(0xFFFFFFFF << (23 - bits) & 0xFFFFFFFF)).view(np.float32)


@dataclass
class Defect:
    """A deliberate error planted into the fp32 forward pass (tests/test_mlp_ref.py): the tolerance has to catch each of them."""

    drop_last_k_of: int | None = None  # MLPLayer index whose last four input columns are left out of the sum
    shift_bias_of: int | None = None   # MLPLayer index whose Linear bias is rotated by one row
    cut_bits: int | None = None        # activations truncated to this many mantissa bits after every layer
    skip_residual_of: int | None = None  # block index whose `h + block(h)` leaves out h


def _forward(sd, acts, x, dtype, dot, defect: Defect | None = None):
    prefixes, n_blocks, per_block = _structure(sd)
    assert len(acts) == len(prefixes), f"{len(acts)} activations for {len(prefixes)} layers"
    P = lambda k: np.asarray(sd[k]).astype(dtype)  # noqa: E731
    eps = dtype(BN_EPS)

    def layer(i, h):
        p = prefixes[i]
        w, b = P(p + ".0.weight"), P(p + ".0.bias")
        if defect is not None and defect.drop_last_k_of == i:
            h, w = h[:, :-4], w[:, :-4]
        if defect is not None and defect.shift_bias_of == i:
            b = np.roll(b, 1)
        y = dot(h, w) + b
        if (p + ".1.running_mean") in sd:
            y = (y - P(p + ".1.running_mean")) / np.sqrt(P(p + ".1.running_var") + eps) * P(p + ".1.weight") + P(p + ".1.bias")
        if acts[i] == "relu":
            y = np.maximum(y, dtype(0))
        else:
            assert acts[i] == "none", acts[i]
        if defect is not None and defect.cut_bits is not None:
            y = cut_mantissa(y, defect.cut_bits)
        return y

    h = layer(0, np.asarray(x).astype(dtype))
    i = 1
    for b in range(n_blocks):
        t = h
        for _ in range(per_block):
            t = layer(i, t)
            i += 1
        h = t if (defect is not None and defect.skip_residual_of == b) else h + t
    y = dot(h, P("model.output.weight")) + P("model.output.bias")
    assert y.dtype == dtype
    return y


def forward64(sd, acts, x):
    """The network as the reference's modules compute it (Linear, BatchNorm1d eval, ReLU, h + block(h)), in float64."""
    return _forward(sd, acts, x, np.float64, _dot64)


def forward32_seq(sd, acts, x, defect: Defect | None = None):
    """The same network in float32, every dot product accumulated one k at a time."""
    return _forward(sd, acts, x, np.float32, _dot32_seq, defect)


def forward32_group4(sd, acts, x):
    """float32 with the products summed in groups of four: another honest order, which has to pass the tolerance."""
    return _forward(sd, acts, x, np.float32, _dot32_group4)


def tolerance(sd, acts, x) -> float:
    return TOL_FACTOR * float(np.abs(forward32_seq(sd, acts, x).astype(np.float64) - forward64(sd, acts, x)).max())


def forward_folded64(layers, n_blocks, per_block, x):
    """float64 forward pass of FOLDED layers [(W, b, relu)] (what fold_state_dict hands to the device)."""
    def aff(i, h):
        w, b, relu = layers[i]
        y = h @ np.asarray(w, np.float64).T + np.asarray(b, np.float64)
        return np.maximum(y, 0.0) if relu else y

    h = aff(0, np.asarray(x, np.float64))
    i = 1
    for _ in range(n_blocks):
        t = h
        for _ in range(per_block):
            t = aff(i, t)
            i += 1
        h = h + t
    return aff(i, h)


# ---------------------------------------------------------------------------------------------------------------------------------
# the parameter blob and its two paths
def blob_floats(layers) -> int:
    """Floats of the padded parameter blob wtk_mlp_create builds: sum of ceil16(out) * ceil4(in) + ceil16(out)."""
    c = lambda v, m: (v + m - 1) // m * m  # noqa: E731
    return sum(c(w.shape[0], 16) * c(w.shape[1], 4) + c(w.shape[0], 16) for w, _, _ in layers)


def param_path(layers) -> str:
    return "lds" if blob_floats(layers) <= LDS_PARAM_FLOATS else "global"


def with_zero_block(layers, hidden=128, *, layers_per_block, until_global=False):
    """`layers` with one more residual block whose weights and biases are all zero: `layers_per_block` layers, hidden widths `hidden`,
    back to the residual width.  The block's output is exactly 0 and h + 0 = h, so the network's values do not change, but the blob
    grows.  A block of one layer has no hidden width (it is residual x residual), so one block does not always carry a small network
    over the LDS limit: until_global=True appends as many zero blocks as that takes.  Returns (layers, blocks added)."""
    assert layers_per_block >= 1
    res = layers[0][0].shape[0]
    dims = [hidden] * (layers_per_block - 1) + [res]
    body, out = list(layers[:-1]), layers[-1]
    added = 0
    while True:
        k = res
        for n in dims:
            body.append((np.zeros((n, k), np.float32), np.zeros(n, np.float32), True))
            k = n
        added += 1
        if not until_global or param_path(body + [out]) == "global":
            break
        assert len(body) + 1 + layers_per_block <= MAX_LAYERS, "no room for enough zero blocks"
    return body + [out], added


# ---------------------------------------------------------------------------------------------------------------------------------
@dataclass
class Row:
    name: str
    path: str
    layers: int
    blob: int
    dev: float  # max |device - forward64|
    tol: float
    top: float  # max |forward64|
    note: str = ""

    @property
    def ratio(self) -> float:
        return self.dev / self.tol


def table(title: str, rows) -> str:
    """Deviation / tolerance per network, in the manner of layer_ref.Report.table."""
    lines = [f"[mlp_ref] {title}: max |device - float64| over tolerance (8 x the deviation of a sequential fp32 forward)"]
    for r in rows:
        flag = "" if r.ratio <= 1.0 else "  <-- FAIL"
        lines.append(f"  {r.name:<22} {r.path:<7} layers {r.layers:<3} blob {r.blob:<6} max|y| {r.top:9.3e}  dev {r.dev:9.3e}  tol {r.tol:9.3e}"
                     f"  ratio {r.ratio:6.3f}{('  ' + r.note) if r.note else ''}{flag}")
    lines.append(f"  worst ratio: {max(r.ratio for r in rows):.3f}")
    return "\n".join(lines)
