"""Weights for the polynomial-fit controller, searched on the device: the reference's `WeightEvaluator`
(wtracker/sim/sim_controllers/polyfit_controller.py:87-221) and the particle swarm `polyfit_optimizer.ipynb` runs over it.

All series of an evaluator share one time axis, so for one weight vector `w` and degree `d` the fit-then-extrapolate step is one linear
functional applied to every series: `y_pred[m] = sum_n g_n(w, d) * y_input[n, m]`.  The device computes `g` per candidate (a <= 16 x 8 SVD with
numpy's `rcond = N * eps` cut, csrc/polyfit_opt.hip) and then streams the dataset once per candidate; `eval` is the mean of `|y_target - y_pred|`.
The reduction has a fixed order: equal weights give equal bits in every call, alone or inside a population.

There is no CPU fallback: without a visible GPU the constructor raises.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import hip
from .controllers import PolyfitConfig, _read_track_csv
from .sim import TimingConfig

MAX_TIMES = 16  # kTrackMaxTimes
MAX_DEGREE = 7  # kTrackMaxCoef - 1
MAX_POP = 65535


@dataclass
class SwarmResult:
    weights: np.ndarray  # [N] best weight vector (weight i belongs to the i-th smallest offset)
    mae: float           # its MAE: bit-equal to WeightEvaluator.eval(weights, deg)  (Replay.optimize_polyfit: the closed-loop objective value instead)
    history: np.ndarray  # [epochs] best MAE (objective value) after every epoch run
    epochs: int          # epochs run (< max_epoch when the search stopped early)
    degree: int


def check_times(times, name: str) -> np.ndarray:
    """`times` (`name` to its caller): 1-D, 1 .. MAX_TIMES whole frame offsets -> int64, sorted as the reference sorts them (and not the weights)."""
    t = np.asarray(times)
    if t.ndim != 1 or t.size == 0:
        raise ValueError(f"{name} must be a non-empty 1-D sequence of frame offsets")
    if t.size > MAX_TIMES:
        raise ValueError(f"at most {MAX_TIMES} {name} (the device solver's limit), got {t.size}")
    if not np.all(t == np.round(t)):
        raise ValueError(f"{name} must be whole frame numbers")
    return np.sort(t.astype(np.int64))


def _check_offsets(input_time_offsets, pred_time_offset) -> np.ndarray:
    off = check_times(input_time_offsets, "input_time_offsets")
    if int(pred_time_offset) != pred_time_offset:
        raise ValueError("pred_time_offset must be a whole frame number")
    if off[-1] > pred_time_offset:
        raise ValueError(f"the largest input offset ({int(off[-1])}) lies beyond pred_time_offset ({int(pred_time_offset)}): the input frames of the last "
                         "cycles would lie past the end of the log (the reference raises IndexError there)")
    if off[0] >= pred_time_offset:
        raise ValueError("pred_time_offset must lie after the first input offset: the speed filter divides by that span")
    return off


def _check_degree(deg) -> int:
    if int(deg) != deg or not 0 <= int(deg) <= MAX_DEGREE:
        raise ValueError(f"the degree must be an integer in [0, {MAX_DEGREE}] (the device solver's limit), got {deg!r}")
    return int(deg)


def weights_to_device(owner, weights, N: int, per: str, min_rows: int = 0):
    """`weights` [P, N] (array: uploaded; tensor: used in place when it already is float64, contiguous and there) as a float64 tensor on the device
    of `owner` (a WeightEvaluator or a Replay; its `_dev` is read after the shape is checked).  `per` names what a weight belongs to in the error
    message; P must lie in [min_rows, MAX_POP]."""
    import torch

    if not isinstance(weights, torch.Tensor):
        weights = torch.from_numpy(np.ascontiguousarray(weights, dtype=np.float64))
    if weights.dim() != 2 or weights.shape[1] != N:
        raise ValueError(f"weights must have shape [P, {N}] (one weight per {per}), got {tuple(weights.shape)}")
    if not min_rows <= weights.shape[0] <= MAX_POP:
        raise ValueError(f"{min_rows}..{MAX_POP} weight vectors per call" if min_rows else f"at most {MAX_POP} weight vectors per call")
    return weights.to(device=owner._dev, dtype=torch.float64).contiguous()


def polyfit_config(degree, sample_times, weights) -> PolyfitConfig:
    """The PolyfitConfig of one weight vector over the (sorted) `sample_times`."""
    w = [float(v) for v in np.asarray(weights, dtype=np.float64).reshape(-1)]
    if len(w) != len(sample_times):
        raise ValueError(f"{len(sample_times)} weights expected, got {len(w)}")
    return PolyfitConfig(degree=_check_degree(degree), sample_times=[int(t) for t in sample_times], weights=w)


W_MAX, W_MIN = 0.9, 0.4  # inertia weight of the swarm at the first / after the last epoch


def check_swarm_args(pop_size, max_epoch, max_early_stop, lb, ub) -> tuple:
    """(P, E) as ints.  swarm_search calls it; a caller that sizes buffers by P calls it first, so that every refusal comes before the device is touched."""
    if int(pop_size) != pop_size or not 1 <= pop_size <= MAX_POP:
        raise ValueError(f"pop_size must be in [1, {MAX_POP}]")
    if int(max_epoch) != max_epoch or max_epoch < 1 or int(max_early_stop) != max_early_stop or max_early_stop < 1:
        raise ValueError("max_epoch and max_early_stop must be positive integers")
    if not (np.isfinite(lb) and np.isfinite(ub) and lb < ub):
        raise ValueError(f"need finite bounds lb < ub, got [{lb}, {ub}]")
    return int(pop_size), int(max_epoch)


def swarm_search(device, N: int, enqueue_value, degree: int, pop_size, c1, c2, max_epoch, max_early_stop, seed, lb, ub, start=None,
                 _trace: Optional[list] = None) -> SwarmResult:
    """The particle swarm of `WeightEvaluator.optimize` (its docstring states the rule) over any objective of N weights: `enqueue_value(pos, value,
    ctrl)` enqueues, on the current stream of `device`, the evaluation of the positions `pos` [P, N] into `value` [P] as a no-op once the stop flag
    `ctrl` is up.  `start` [K, N], K < P, already checked by the caller, replaces the random start of particles 1 .. K (drawn all the same, so the
    random numbers of the epochs do not depend on it).  Every epoch is enqueued at once; the host waits once, for the current stream."""
    import torch

    P, E = check_swarm_args(pop_size, max_epoch, max_early_stop, lb, ub)
    rng = np.random.default_rng(seed)
    x0 = lb + (ub - lb) * rng.random((P, N))
    x0[0, :] = ub
    if start is not None:
        x0[1 : 1 + len(start)] = start
    rand = rng.random((E, 2, P, N))
    vmax = 0.5 * (ub - lb)
    with torch.cuda.device(device):
        f64 = torch.float64
        stream = torch.cuda.current_stream(device)
        pos = torch.from_numpy(x0).to(device)
        rand_dev = torch.from_numpy(rand).to(device)
        vel = torch.zeros((P, N), dtype=f64, device=device)
        pbest_pos = pos.clone()
        pbest_val = torch.full((P,), float("inf"), dtype=f64, device=device)
        gbest_pos = pos[0].clone()
        gbest_val = torch.full((1,), float("inf"), dtype=f64, device=device)
        ctrl = torch.zeros((4,), dtype=torch.int32, device=device)
        history = torch.full((E,), float("nan"), dtype=f64, device=device)
        value = torch.empty((P,), dtype=f64, device=device)
        for e in range(E):
            enqueue_value(pos, value, ctrl)
            if _trace is not None:  # tests: the state every epoch starts from and the values it saw (stream-ordered copies)
                _trace.append((pos.clone(), vel.clone(), value.clone()))
            hip.polyfit_swarm_step(value, rand_dev[e], P, N, e, int(max_early_stop), W_MAX - (W_MAX - W_MIN) * e / E, c1, c2, lb, ub, vmax, pos, vel,
                                   pbest_pos, pbest_val, gbest_pos, gbest_val, ctrl, history, stream=stream.cuda_stream)
        stream.synchronize()  # the one host synchronisation
        epochs = int(ctrl[2].item())
        return SwarmResult(weights=gbest_pos.cpu().numpy(), mae=float(gbest_val.item()), history=history[:epochs].cpu().numpy(), epochs=epochs, degree=degree)


class WeightEvaluator:
    """Mean absolute error of the weighted polynomial fit over the cycles of one or more experiment logs, for one weight vector (`eval`, the
    reference's method) or a whole population (`eval_many`), and the swarm search over it (`optimize`).

    Same constructor as the reference's plus `device`.  `x_input`, `y_input`, `y_target`, `x_target` are device tensors whose `.cpu().numpy()`
    are the reference's arrays; `cycle_stats` holds per log `(candidate cycles, kept, removed)` (the reference prints them)."""

    def __init__(self, csv_paths: Sequence[str], timing_config: TimingConfig, input_time_offsets, pred_time_offset: int, min_speed: float = 0,
                 max_speed: float = np.inf, device: int = 0):
        self._setup(timing_config, input_time_offsets, pred_time_offset, min_speed, max_speed)
        self.csv_paths = list(csv_paths)
        tracks = [_read_track_csv(p) for p in self.csv_paths]
        self._build(tracks, device)

    @classmethod
    def from_tracks(cls, tracks: Sequence, timing_config: TimingConfig, input_time_offsets, pred_time_offset: int, min_speed: float = 0,
                    max_speed: float = np.inf, device: Optional[int] = None) -> "WeightEvaluator":
        """From tracks that are already arrays: [n_frames, 4] xywh, float32 or float64, device tensors (used in place) or numpy arrays (uploaded)."""
        self = cls.__new__(cls)
        self._setup(timing_config, input_time_offsets, pred_time_offset, min_speed, max_speed)
        self.csv_paths = []
        tracks = list(tracks)
        if device is None:
            devs = [t.device.index for t in tracks if hasattr(t, "device") and getattr(t.device, "type", "") == "cuda"]
            device = devs[0] if devs else 0
        self._build(tracks, device)
        return self

    def _setup(self, timing_config, input_time_offsets, pred_time_offset, min_speed, max_speed):
        self.input_time_offsets = _check_offsets(input_time_offsets, pred_time_offset)
        self.timing_config = timing_config
        self.pred_time_offset = int(pred_time_offset)
        self.min_speed = float(min_speed)
        self.max_speed = float(max_speed)
        if int(timing_config.cycle_frame_num) <= 0:
            raise ValueError("timing_config.cycle_frame_num must be positive")

    def _build(self, tracks, device: int):
        if not tracks:
            raise ValueError("at least one log is needed")
        for t in tracks:
            if len(t.shape) != 2 or t.shape[1] != 4:
                raise ValueError(f"a track must be [n_frames, 4] xywh, got {tuple(t.shape)}")
        if hip.device_count() < 1:
            raise hip.WtkError("WeightEvaluator needs a GPU: no HIP device visible (there is no CPU fallback)")
        import torch

        self._dev = torch.device("cuda", device)
        L = int(self.timing_config.cycle_frame_num)
        N = len(self.input_time_offsets)
        cand = [-(-int(t.shape[0]) // L) for t in tracks]
        cap = max(1, sum(cand))
        with torch.cuda.device(self._dev):
            stream = torch.cuda.current_stream(self._dev).cuda_stream
            y_in = torch.empty((N, 2 * cap), dtype=torch.float64, device=self._dev)
            y_tg = torch.empty((2 * cap,), dtype=torch.float64, device=self._dev)
            count = torch.zeros((1,), dtype=torch.int32, device=self._dev)
            after = torch.zeros((len(tracks),), dtype=torch.int32, device=self._dev)
            for i, t in enumerate(tracks):
                if isinstance(t, np.ndarray):
                    t = torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32 if t.dtype == np.float32 else np.float64))
                t = t.to(self._dev).contiguous()
                hip.polyfit_dataset(t, int(t.shape[0]), L, self.input_time_offsets, self.pred_time_offset, self.min_speed, self.max_speed, y_in, y_tg,
                                    cap, count, stream=stream)
                after[i : i + 1].copy_(count)
            torch.cuda.synchronize(self._dev)
            after = after.cpu().numpy().astype(np.int64)
            kept_total = int(after[-1])
            if kept_total > cap:
                raise hip.WtkError(f"wtk_polyfit_dataset kept {kept_total} cycles for a capacity of {cap}")
            kept = np.diff(np.concatenate([[0], after]))
            self.cycle_stats = [(int(c), int(k), int(c - k)) for c, k in zip(cand, kept)]
            self.y_input = y_in[:, : 2 * kept_total].contiguous()
            self.y_target = y_tg[: 2 * kept_total].contiguous()
            self.x_input = torch.from_numpy(self.input_time_offsets.copy()).to(self._dev)
            self.x_target = torch.full_like(self.y_target, float(self.pred_time_offset))
        self.n_series = 2 * kept_total

    # ------------------------------------------------------------------ evaluation
    def _enqueue_mae(self, w_dev, deg: int, mae_dev, scratch, stop_dev=None):
        import torch

        hip.polyfit_weight_mae(self.y_input, self.y_target, self.n_series, self.n_series, self.input_time_offsets, self.pred_time_offset, deg, w_dev,
                               int(w_dev.shape[0]), mae_dev, scratch, scratch.numel(), stop_dev, stream=torch.cuda.current_stream(self._dev).cuda_stream)

    def eval_many(self, weights, deg: int = 2):
        """MAE of every row of `weights` [P, N]: float64 device tensor [P], enqueued on the current torch stream (no synchronisation)."""
        import torch

        deg = _check_degree(deg)
        w = weights_to_device(self, weights, len(self.input_time_offsets), "input time offset")
        P = int(w.shape[0])
        with torch.cuda.device(self._dev):
            mae = torch.empty((P,), dtype=torch.float64, device=self._dev)
            scratch = torch.empty((max(1, hip.polyfit_mae_scratch_doubles(P, self.n_series)),), dtype=torch.float64, device=self._dev)
            self._enqueue_mae(w, deg, mae, scratch)
        return mae

    def eval(self, weights, deg: int = 2) -> float:
        """The reference's method: MAE of the fit with `weights` [N] (NaN when no cycle survived the filters)."""
        w = np.asarray(weights.detach().cpu().numpy() if hasattr(weights, "detach") else weights, dtype=np.float64)
        if w.ndim != 1:
            raise ValueError(f"weights must have shape [{len(self.input_time_offsets)}], got {w.shape}")
        return float(self.eval_many(w[None, :], deg).cpu().numpy()[0])

    # ------------------------------------------------------------------ search
    W_MAX, W_MIN = W_MAX, W_MIN  # the module's, under the names the rule below uses

    def optimize(self, deg: int = 2, pop_size: int = 100, c1: float = 2.05, c2: float = 2.05, max_epoch: int = 300, max_early_stop: int = 100, seed: int = 0,
                 lb: float = 0.0, ub: float = 1.0, _trace: Optional[list] = None) -> SwarmResult:
        """Particle-swarm search for the weight vector of lowest MAE in [lb, ub]^N; every epoch is enqueued at once, the host waits once at the end.

        The rule (the classic inertia-weight swarm; the notebook's mealpy `OriginalPSO` is NOT pinned and no trajectory equality with it is claimed):
          * random numbers: `rng = numpy.random.default_rng(seed)`; `x0 = lb + (ub - lb) * rng.random((P, N))`, then `r = rng.random((max_epoch, 2, P, N))`
          * particle 0 starts at `ub` in every coordinate (with the default bounds: the uniform all-ones weights of a default PolyfitConfig), so the
            result is never worse than uniform weights; velocities start at zero
          * epoch e = 0, 1, ...: evaluate all positions; a particle's personal best changes on a strictly lower MAE (a NaN never wins), the global best
            is the lowest personal best (lowest particle index among equals) when strictly lower than before; history[e] = global best MAE
          * the search stops after the epoch at which `max_early_stop` epochs in a row brought no new global best
          * otherwise, with `w_e = W_MAX - (W_MAX - W_MIN) * e / max_epoch` and `vmax = 0.5 * (ub - lb)`:
            `v = clip((w_e * v + (c1 * r[e, 0]) * (pbest - x)) + (c2 * r[e, 1]) * (gbest - x), -vmax, vmax)`, `x = clip(x + v, lb, ub)`
        A run is reproducible from its arguments bit for bit."""
        import torch

        deg = _check_degree(deg)
        P, _ = check_swarm_args(pop_size, max_epoch, max_early_stop, lb, ub)
        scratch = torch.empty((max(1, hip.polyfit_mae_scratch_doubles(P, self.n_series)),), dtype=torch.float64, device=self._dev)

        def enqueue_mae(pos, mae, ctrl):
            self._enqueue_mae(pos, deg, mae, scratch, stop_dev=ctrl)

        return swarm_search(self._dev, len(self.input_time_offsets), enqueue_mae, deg, pop_size, c1, c2, max_epoch, max_early_stop, seed, lb, ub, _trace=_trace)

    def to_config(self, deg: int, weights) -> PolyfitConfig:
        """The PolyfitConfig (sample times = the sorted offsets) that PolyfitController / HipPolyfitController take."""
        return polyfit_config(deg, self.input_time_offsets, weights)
