"""Per-layer check of a detector forward pass against float64 arithmetic the library does not share.

Every conv blob L of a finished forward pass is checked in isolation: L's input is rebuilt from the tensors the GPU itself stored
(HipYolo.debug_tensor), following the graph of oracle/yolo_oracle.py:YoloOracle.forward (C2f chunk / cat, the bottleneck residual that the
library adds in m.i.cv2's epilogue, SPPF max-pools of the GPU's model.9.cv1, nearest upsample, the four concats; the stem reads the frame as
uint8 / 255 in RGB order), L is recomputed in float64 on the CPU from the blob's fp32 weights, and the GPU's output must lie within

    |y_gpu - y_ref| <= s * u(K) * M + u_out * |y_ref| + w_floor * sum|x| + a_floor            (every element)
    rms(|y_gpu - y_ref| / N) <= rho                                                           (every layer)

where K = cin * k * k, M = |b| + conv(|x|, |W|) is the magnitude of the sum, s = 1.1 (the largest |silu'|) for activated layers and 1 for
the Detect outputs, N = s * M + |r| (r: the residual, where there is one), sum|x| is the sum of |x| over the receptive field and a_floor the
subnormal spacing of the storage type.  Channels a blob stores beyond its real cout (the class tail's cls_ld padding) must hold exactly 0.0.

Blobs that a plan keeps on chip (fused front, the C2f tail's bottleneck, the fp16 implicit-GEMM tail, folded Detect 1x1 tails) are named by
the caller.  They are checked as COMPOSITES: their consumer reads the float64 reference of the blob instead of a GPU tensor, and the blob's own
bound E and normaliser N are carried through the consumer's |W| (bound += s * conv(E, |W|), N += s * conv(N, |W|); a residual adds its E / N
unchanged; slices, upsampling and max-pooling carry them the way they carry values).  Nothing is dropped silently.

Derivation of the constants (tests/test_layer_ref.py emulates each mode's arithmetic on the real layer shapes, K up to 4608, and checks that
honest results pass and planted defects fail):

  fp32   operands are the stored fp32 tensors (exact) and the fp32 weights (exact); MFMA f32 products are exact, the sum is accumulated in
         fp32 in steps of at most four products, so a blocked-summation bound gives (K/4 + 16) * 2^-24 relative to M (the 16 covers the bias,
         split-K slab sums and the epilogue).  u_out = 8 * 2^-24: SiLU (exp + reciprocal, a few ulps) and the unscaling of the log2(e)-scaled
         activations.  Emulated fp32 results use < 25 % of this bound; their rms(err / N) stays below 2^-25, rho = 2^-22.  The rms is a
         statistic of a layer's many outputs, checked where there are at least RMS_MIN_COUNT of them: the P5 class logits of a tiny map
         (4 outputs at 32 x 64, B = 2) are dominated by the Detect bias, whose fp32 partial sums alone put one logit at ~2^-22 of M.
  f16x3  activations are stored as hi + lo * 2^-11 pairs and read back exactly; weights are split the same way, so a weight is held to
         2^-22 relative.  A product is hi*hi + (hi*lo + lo*hi) / 2048 with lo*lo dropped: at most 2^-22 * |x||w| more.  u = u_fp32(K) + 2^-21.
         The output pair holds y to 2^-22 relative (lo is an fp16 of the hi's residual times 2048), plus fp32 SiLU and unscaling:
         u_out = 2^-20.  Small weights make the hi half subnormal; the pair still holds them to 2^-36 absolute: w_floor = 2^-35.
         Emulated rms(err / N) <= 2^-25; rho = 2^-22.  With the lo half of the weights or of the activations dropped a layer's products lose
         11 bits (2^-12 per product, rms(err / N) ~ 2^-12 / sqrt(K) ~ 2^-18 at K = 4608): at least 10 x rho on every layer shape.
  fp16   activations are fp16 (read back exactly), weights are rounded to fp16 (2^-11 relative; 2^-25 absolute below the normal range,
         w_floor = 2^-24 with the log2(e) scaling), products are exact in fp32 and summed in fp32: u = 2^-11 + u_fp32(K).  The output is rounded
         to fp16: u_out = 2^-10 (2^-11 rounding of the scaled value, SiLU and unscaling).  Emulated rms(err / N) <= 2^-13; rho = 2^-11.
  a_floor is the storage type's subnormal spacing: 2^-149 (fp32), 2^-24 (fp16, both halves' scale), 2^-35 (the lo half of a pair).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np
import torch
import torch.nn.functional as F

from wtracker_amd import yolo_spec as ys

SILU_SLOPE_MAX = 1.1  # max |silu'(z)| = 1.0998 (z ~ 2.4)
RMS_MIN_COUNT = 512  # the rms ceiling applies to layers with at least this many checked outputs


def u_fp32(K: int) -> float:
    return (K / 4 + 16) * 2.0 ** -24


MODES = {
    # mode: (u(K), u_out, w_floor, a_floor, rho)
    "fp32": (u_fp32, 8 * 2.0 ** -24, 0.0, 2.0 ** -149, 2.0 ** -22),
    "f16x3": (lambda K: u_fp32(K) + 2.0 ** -21, 2.0 ** -20, 2.0 ** -35, 2.0 ** -35, 2.0 ** -22),
    "fp16": (lambda K: u_fp32(K) + 2.0 ** -11, 2.0 ** -10, 2.0 ** -24, 2.0 ** -24, 2.0 ** -11),
}


# ---- the graph of YoloOracle.forward, blob by blob -------------------------------------------------------------------------------------
# a source is ("frame",), ("blob", name, c0, c1) (channel slice of a blob's output; None = all), ("up", name) (2x nearest) or ("pool", name, n)
# (n successive 5x5 / 1 / 2 max-pools)
@dataclass
class Layer:
    name: str
    index: int
    cin: int
    cout: int
    k: int
    stride: int
    act: int
    src: list
    res: tuple | None = None


def layer_graph(scale="s", nc: int = 1) -> list[Layer]:
    table = ys.conv_table(scale, nc)
    spec = {t["name"]: (i, t) for i, t in enumerate(table)}
    depth, width, maxch = ys.SCALES[scale] if isinstance(scale, str) else scale
    n = ys.model_dims(width, depth, maxch, nc)["n"]
    out: list[Layer] = []

    def B(name, c0=None, c1=None):
        return ("blob", name, c0, c1)

    def conv(name, src, res=None):
        i, t = spec[name]
        out.append(Layer(name, i, t["cin"], t["cout"], t["k"], t["stride"], t["act"], list(src), res))
        return B(name)

    def c2f(p, src, reps, shortcut):
        conv(p + ".cv1", src)
        ch = spec[p + ".cv1"][1]["cout"] // 2
        prev, ys_ = B(p + ".cv1", ch, 2 * ch), [B(p + ".cv1")]
        for i in range(reps):
            m = f"{p}.m.{i}"
            conv(m + ".cv1", [prev])
            prev = conv(m + ".cv2", [B(m + ".cv1")], res=prev if shortcut else None)  # stored blob: y[-1] + silu(conv)
            ys_.append(prev)
        return conv(p + ".cv2", ys_)

    x = conv("model.0", [("frame",)])
    x = conv("model.1", [x])
    x = c2f("model.2", [x], n[0], True)
    x = conv("model.3", [x])
    x4 = c2f("model.4", [x], n[1], True)
    x = conv("model.5", [x4])
    x6 = c2f("model.6", [x], n[2], True)
    x = conv("model.7", [x6])
    x = c2f("model.8", [x], n[3], True)
    conv("model.9.cv1", [x])
    x9 = conv("model.9.cv2", [B("model.9.cv1"), ("pool", "model.9.cv1", 1), ("pool", "model.9.cv1", 2), ("pool", "model.9.cv1", 3)])
    x12 = c2f("model.12", [("up", "model.9.cv2"), x6], n[3], False)
    x15 = c2f("model.15", [("up", "model.12.cv2"), x4], n[3], False)
    x16 = conv("model.16", [x15])
    x18 = c2f("model.18", [x16, x12], n[3], False)
    x19 = conv("model.19", [x18])
    x21 = c2f("model.21", [x19, x9], n[3], False)
    for i, f in enumerate((x15, x18, x21)):
        for br in ("cv2", "cv3"):
            p = f"model.22.{br}.{i}"
            conv(p + ".2", [conv(p + ".1", [conv(p + ".0", [f])])])
    assert sorted(L.index for L in out) == list(range(len(table)))
    return out  # in evaluation order


def stem_input(frames: np.ndarray) -> torch.Tensor:
    """uint8 [B,H,W] (gray) or [B,H,W,3] (BGR) frames at network size -> float64 [B,3,H,W] RGB in [0, 1]."""
    f = np.asarray(frames)
    if f.ndim == 3:
        f = np.repeat(f[..., None], 3, axis=3)
    return torch.from_numpy(np.ascontiguousarray(f[..., ::-1].transpose(0, 3, 1, 2))).double() / 255.0


# ---- where the "GPU" tensors come from ------------------------------------------------------------------------------------------------
class HandleSource:
    """The tensors of a HipYolo handle's last forward pass, for the batch rows `rows` only (one blob fetched at a time)."""

    def __init__(self, det, B: int, rows, scale="s", nc: int = 1):
        self.det, self.B, self.rows = det, B, list(rows)
        depth, width, maxch = ys.SCALES[scale] if isinstance(scale, str) else scale
        self.hb = ys.model_dims(width, depth, maxch, nc)["hb"]
        self.index = {t["name"]: i for i, t in enumerate(ys.conv_table(scale, nc))}

    def fetch(self, name: str) -> torch.Tensor:
        """-> float32 [len(rows), C_stored, h, w] (C_stored may exceed the blob's cout: padding channels)."""
        first = None
        if ".cv3." in name and name.endswith(".0"):  # the Detect towers' first 3x3 is ONE op with the box tower's: it reports under cv2.i.0
            first = name.replace(".cv3.", ".cv2.")
            t = self.det.debug_tensor(self.index[first], self.B)[self.rows][..., self.hb:]
        elif ".cv2." in name and name.startswith("model.22.") and name.endswith(".0"):
            t = self.det.debug_tensor(self.index[name], self.B)[self.rows][..., : self.hb]
        else:
            t = self.det.debug_tensor(self.index[name], self.B)[self.rows]
        return torch.from_numpy(np.ascontiguousarray(t)).permute(0, 3, 1, 2).contiguous()


class DictSource:
    """Tensors given as a dict name -> [B, C, h, w] (tests: the oracle's own intermediates, emulated results, planted defects)."""

    def __init__(self, tensors: dict):
        self.t = tensors

    def fetch(self, name: str) -> torch.Tensor:
        return self.t[name]


# ---- the check ------------------------------------------------------------------------------------------------------------------------
@dataclass
class LayerResult:
    name: str
    K: int
    family: str
    worst: float  # max |err| / bound (<= 1 passes); composite blobs: nan (checked through their consumer)
    rms: float    # rms(|err| / N)
    rho: float
    pad_ok: bool = True
    carried: bool = False  # the input holds a composite (an unobservable producer's bound carried through)
    note: str = ""

    @property
    def ok(self) -> bool:
        if self.family == "unobservable":
            return True
        return self.worst <= 1.0 and self.rms <= self.rho and self.pad_ok


@dataclass
class Report:
    label: str
    mode: str
    layers: list = field(default_factory=list)
    unobservable: tuple = ()

    @property
    def failed(self) -> list:
        return [r for r in self.layers if not r.ok]

    def table(self) -> str:
        lines = [f"[layer_ref] {self.label} ({self.mode}): worst |err|/bound and rms(|err|/N)/rho per layer"]
        for r in self.layers:
            if r.family == "unobservable":
                lines.append(f"  {r.name:<22} K={r.K:<5} {'on chip: checked through its consumer':<40}")
                continue
            flag = "" if r.ok else "  <-- FAIL" + (" (padding not 0)" if not r.pad_ok else "")
            lines.append(f"  {r.name:<22} K={r.K:<5} {r.family:<14} worst {r.worst:9.3e}  rms/rho {r.rms / r.rho:9.3e}"
                         f"{'  (composite)' if r.carried else ''}{flag}")
        fams = {}
        for r in self.layers:
            if r.family != "unobservable":
                fams[r.family] = max(fams.get(r.family, 0.0), r.worst)
        lines.append("  worst per family: " + ", ".join(f"{k} {v:.2e}" for k, v in sorted(fams.items())))
        return "\n".join(lines)

    def assert_ok(self):
        bad = self.failed
        assert not bad, self.table() + "\nfailed: " + ", ".join(r.name for r in bad)


def _w(weights, name):
    w, b = weights[name]
    return (torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32)).double().permute(0, 3, 1, 2).contiguous(),
            torch.from_numpy(np.ascontiguousarray(b, dtype=np.float32)).double())


def _up(t):
    return t.repeat_interleave(2, 2).repeat_interleave(2, 3)


def _pool(t, n):
    for _ in range(n):
        t = F.max_pool2d(t, 5, 1, 2)
    return t


def check_network(source, weights: dict, frames: np.ndarray, scale="s", nc: int = 1, mode: str = "fp32", unobservable=(), label: str = "",
                  family=None, only=None) -> Report:
    """Check every conv blob of the forward pass `source` holds (frames: the uint8 frames of the checked rows, at network size).
    unobservable: blob names the plan keeps on chip (checked as composites); family(name) -> str labels the kernel family of a blob;
    only: restrict the per-layer report to these blobs (their producers are still followed)."""
    u, u_out, w_floor, a_floor, rho = MODES[mode]
    unobs = set(unobservable)
    graph = layer_graph(scale, nc)
    by_name = {L.name: L for L in graph}
    for nm in unobs:
        assert nm in by_name, nm
    uses = {}
    for L in graph:
        for s in L.src + ([L.res] if L.res else []):
            if s[0] != "frame":
                uses[s[1]] = uses.get(s[1], 0) + 1
    gpu: dict = {}    # name -> float64 tensor (GPU values, or the fp64 reference of an unobservable blob)
    carry: dict = {}  # unobservable name -> (E, N)
    rep = Report(label, mode, unobservable=tuple(sorted(unobs)))
    x0 = stem_input(frames)

    def value(name):
        if name not in gpu:
            gpu[name] = source.fetch(name).double()
        return gpu[name]

    def resolve(s):
        """-> (value, E or None, N or None) of one source."""
        if s[0] == "frame":
            return x0, None, None
        name = s[1]
        v = value(name)
        E, N = carry.get(name, (None, None))
        if s[0] == "blob":
            c0, c1 = s[2], s[3]
            v = v[:, : by_name[name].cout] if c0 is None else v[:, c0:c1]
            if E is not None:
                E, N = (E, N) if c0 is None else (E[:, c0:c1], N[:, c0:c1])
            return v, E, N
        v = v[:, : by_name[name].cout]
        if s[0] == "up":
            return _up(v), None if E is None else _up(E), None if N is None else _up(N)
        return _pool(v, s[2]), None if E is None else _pool(E, s[2]), None if N is None else _pool(N, s[2])

    def release(name):
        uses[name] -= 1
        if uses[name] == 0 and name not in unobs:
            gpu.pop(name, None)

    with torch.no_grad():
        for L in graph:
            parts = [resolve(s) for s in L.src]
            x = torch.cat([p[0] for p in parts], 1)
            carried = any(p[1] is not None for p in parts)
            W, b = _w(weights, L.name)
            pad = L.k // 2
            z = F.conv2d(x, W, b, stride=L.stride, padding=pad)
            y = F.silu(z) if L.act else z
            s = SILU_SLOPE_MAX if L.act else 1.0
            Wa = W.abs()
            M = F.conv2d(x.abs(), Wa, b.abs(), stride=L.stride, padding=pad)
            K = L.cin * L.k * L.k
            bound = s * u(K) * M
            if w_floor:
                ones = torch.ones((1, 1, L.k, L.k), dtype=torch.float64)
                bound += s * w_floor * F.conv2d(x.abs().sum(1, keepdim=True), ones, stride=L.stride, padding=pad)
            N = s * M
            if carried:
                E_in = torch.cat([p[1] if p[1] is not None else torch.zeros_like(p[0]) for p in parts], 1)
                N_in = torch.cat([p[2] if p[2] is not None else torch.zeros_like(p[0]) for p in parts], 1)
                bound += s * F.conv2d(E_in, Wa, stride=L.stride, padding=pad)
                N += s * F.conv2d(N_in, Wa, stride=L.stride, padding=pad)
            if L.res is not None:
                r, Er, Nr = resolve(L.res)
                y = y + r
                N += r.abs()
                if Er is not None:
                    bound += Er
                    N += Nr
                    carried = True
            bound += u_out * y.abs() + a_floor
            for s_ in L.src + ([L.res] if L.res else []):
                if s_[0] != "frame":
                    release(s_[1])
            if L.name in unobs:
                gpu[L.name] = y
                carry[L.name] = (bound, N)
                rep.layers.append(LayerResult(L.name, K, "unobservable", math.nan, math.nan, rho, carried=carried))
                continue
            g = value(L.name)
            pad_ok = True
            if g.shape[1] > L.cout:  # channels stored beyond the real cout must be exactly zero
                pad_ok = bool((g[:, L.cout:] == 0).all())
            assert g.shape[0] == y.shape[0] and g.shape[2:] == y.shape[2:] and g.shape[1] >= L.cout, (L.name, tuple(g.shape), tuple(y.shape))
            err = (g[:, : L.cout] - y).abs()
            if uses.get(L.name, 0) == 0:
                gpu.pop(L.name, None)
            worst = float((err / bound).max())
            if not math.isfinite(worst):
                worst = math.inf
            # an rms over a handful of outputs is no statistic: one bias-dominated logit of fp32-rounded partial sums can sit at 2^-22 alone
            rms = float(torch.sqrt(torch.mean((err / N.clamp_min(1e-300)) ** 2))) if err.numel() >= RMS_MIN_COUNT else 0.0
            if only is None or L.name in only:
                rep.layers.append(LayerResult(L.name, K, family(L.name) if family else "conv", worst, rms, rho, pad_ok, carried))
    return rep


def unobservable_blobs(scale="s", nc: int = 1, dtype: str = "fp16", plan: str = "throughput", env: dict | None = None) -> list[str]:
    """The blobs a handle keeps on chip, by the planning rules of csrc/wtk_plan.hip (YOLOv8 s / n; env: the WTK_* switches in force).
      shared bottleneck scratch (every plan): m.i.cv1 of every bottleneck but a C2f's last;
      fused front (front_fused_kernel: fp16 at scale s; front_fused_split_kernel: f16x3): model.0, model.1 unless WTK_FRONT_DEBUG=1;
      fused C2f tail (c2f32_fused_kernel, fp16 at scale s): model.2.m.0.cv1 and model.2.m.0.cv2;
      fp16 implicit-GEMM tail (model.3 -> model.4.cv1 at scale s, model.5 -> model.6.cv1 at scale n, model.1 -> model.2.cv1 at scale l): the strided 3x3;
      folded Detect 1x1 tails (throughput plan, fp16 / f16x3, 64-wide box / 128-wide class towers): cv2.i.1 (box), cv3.i.1 (class;
      f16x3 unless WTK_NO_SPLIT_CLS_TAIL=1; nc <= 32)."""
    env = env or {}
    on = lambda k: str(env.get(k, "0")) == "1"  # noqa: E731
    # every plan: the bottlenecks of one C2f share ONE scratch tensor for their m.i.cv1 output, so all but the last are overwritten by the time
    # the pass ends (csrc/wtk_plan.hip, Planner::c2f)
    depth, width, maxch = ys.SCALES[scale] if isinstance(scale, str) else scale
    n = ys.model_dims(width, depth, maxch, nc)["n"]
    reps = {"model.2": n[0], "model.4": n[1], "model.6": n[2], "model.8": n[3], "model.12": n[3], "model.15": n[3], "model.18": n[3], "model.21": n[3]}
    out = [f"{p}.m.{i}.cv1" for p, r in reps.items() for i in range(r - 1)]
    dims = ys.model_dims(width, depth, maxch, nc)
    c = dims["c"]
    front = c[0] == 32 and c[1] == 64  # front_fused_eligible / front_fused_split_eligible (model.2.cv1 is 64 wide when model.1 is)
    if dtype in ("fp16", "f16x3") and front and not on("WTK_NO_FUSED_FRONT") and not on("WTK_FRONT_DEBUG"):
        out += ["model.0", "model.1"]
    if dtype == "fp16" and c[1] == 64 and n[0] == 1 and not on("WTK_NO_FUSED_C2F"):  # c2f_fused_eligible: hidden width 32, one bottleneck
        out += ["model.2.m.0.cv1", "model.2.m.0.cv2"]
    if dtype == "fp16" and not on("WTK_NO_IGEMM_TAIL"):  # a strided 3x3 of 128 couts whose only reader is the 1x1 128 -> 128 behind it
        # (fuse_strided_tails walks every op: model.1 -> model.2.cv1 qualifies too where model.1 has 128 couts — scale l; the 1x1 behind a strided
        # 3x3 of the backbone is a C2f's cv1, as wide as the 3x3, and the 3x3's only reader)
        out += [f"model.{i}" for i, ci in ((1, c[1]), (3, c[2]), (5, c[3]), (7, c[4])) if ci == 128]
    if dtype in ("fp16", "f16x3") and plan == "throughput" and not on("WTK_NO_FUSED_TAIL") and not on("WTK_NO_HALO") and str(env.get("WTK_HALO_SLABS", "3")) != "2":
        if dims["hb"] == 64:
            out += [f"model.22.cv2.{i}.1" for i in range(3)]
        if dims["hc"] == 128 and nc <= 32 and (dtype == "fp16" or not on("WTK_NO_SPLIT_CLS_TAIL")):
            out += [f"model.22.cv3.{i}.1" for i in range(3)]
    return out
