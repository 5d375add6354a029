"""Closed-loop replay of track-driven experiments on the device, with tracking error: what the reference's `Simulator` + `SineMotorController` +
`LoggingController` (sim/simulator.py:140-194, sim/motor_controllers.py:58-88, sim_controllers/logging_controller.py:145-185) produce frame by frame for
one experiment, for a whole population of controller configurations at once (csrc/replay.hip).

    rp = Replay(track, timing_config, experiment_config)
    res = rp.run(rp.polyfit([PolyfitConfig(2, [-9, -6, -3, 0, 2, 4], w) for w in weight_vectors]), rows=[0])
    res.moves, res.positions          # [E, C, 2] int32
    res.summary.mean_bbox_error       # [E]
    res.log(0); res.to_csv(0, "bboxes.csv")

During the imaging phase the platform stands still, so a controller's move is round(f(target_c, platform position)) with a per-cycle target that does not
depend on the platform.  The builders (`csv`, `optimal`, `polyfit`, `mlp`) compute the targets of all cycles with the existing device calls; `run` scans
the cycles (one lane per experiment) and expands to frames.  Everything is enqueued on the current torch stream; `run` synchronises once.

There is no CPU fallback: without a visible GPU the constructor raises.  Not covered: the YOLO controller (its targets depend on the camera view),
`StepMotorController`, DataAnalyzer's speed and unit columns.
"""
from __future__ import annotations

import csv as _csv
import os
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import hip
from .controllers import PolyfitConfig, _read_track_csv
from .resmlp import FoldedResMLP, from_torch_module
from .sim import LOG_COLUMNS, ExperimentConfig, TimingConfig

KINDS = {"csv": hip.REPLAY_CSV, "optimal": hip.REPLAY_OPTIMAL, "polyfit": hip.REPLAY_POLYFIT, "mlp": hip.REPLAY_MLP}


@dataclass
class Targets:
    """Per-cycle targets of E experiments, cycle-major on the device: a, b float64 [C, E, 2], valid int32 [C, E] (CSV: none of them)."""

    kind: str
    E: int
    a: object = None
    b: object = None
    valid: object = None
    keep: object = None  # what the enqueued work still reads (the MLP handle's weights)


@dataclass
class Summary:
    """Per-experiment figures of a replay ([E] arrays).  `trimmed`: imaging-phase rows without the first and the last logged cycle, as
    DataAnalyzer.clean(trim_cycles=True, imaging_only=True)."""

    bbox_error_sum: np.ndarray
    rows: np.ndarray
    trimmed_bbox_error_sum: np.ndarray
    trimmed_rows: np.ndarray
    non_perfect_rows: np.ndarray  # rows with bbox_error > 1e-7 (the reference's "non perfect predictions")
    mse_error_sum: np.ndarray

    @property
    def mean_bbox_error(self) -> np.ndarray:
        return self.bbox_error_sum / self.rows

    @property
    def trimmed_mean_bbox_error(self) -> np.ndarray:
        return self.trimmed_bbox_error_sum / self.trimmed_rows

    @property
    def non_perfect(self) -> np.ndarray:
        return self.non_perfect_rows / self.rows

    @property
    def mean_mse_error(self) -> np.ndarray:
        return self.mse_error_sum / self.rows


class ReplayResult:
    """moves, positions [E, C, 2] int32 (the move of cycle c and the platform position at its start); summary; bbox_error / mse_error [E, R] float64 when
    requested; the full log rows of the experiments named in `rows`."""

    def __init__(self, moves, positions, summary, decision_frames, row_ids, row_data, bbox_error, mse_error):
        self.moves, self.positions, self.summary, self.decision_frames = moves, positions, summary, decision_frames
        self.bbox_error, self.mse_error = bbox_error, mse_error
        self._slot = {int(e): k for k, e in enumerate(row_ids)}
        self._rows = row_data  # [slots, R, 16]

    def row_array(self, e: int) -> np.ndarray:
        """Experiment e's rows as float64 [R, 16]: plt_x, plt_y, cam xywh, mic xywh, wrm xywh, cycle, phase (0 imaging, 1 moving); row r is frame r."""
        if int(e) not in self._slot:
            raise KeyError(f"experiment {e} was not named in run(rows=...)")
        return self._rows[self._slot[int(e)]]

    def log(self, e: int) -> list:
        """Experiment e's rows as TrackLogger keeps them: dictionaries with the columns of sim.LOG_COLUMNS."""
        out = []
        for r, v in enumerate(self.row_array(e)):
            row = dict(frame=r, cycle=int(v[14]), phase="imaging" if v[15] == 0 else "moving")
            for k, name in enumerate(LOG_COLUMNS[3:13]):
                row[name] = int(v[k])
            for k, name in enumerate(LOG_COLUMNS[13:17]):
                row[name] = float(v[10 + k])
            out.append(row)
        return out

    def to_csv(self, e: int, path: str) -> None:
        """Experiment e's log as the bboxes.csv LoggingController writes: DataAnalyzer.load and evaluation.precise_error_from_log read it."""
        with open(path, "w", newline="") as f:
            w = _csv.DictWriter(f, LOG_COLUMNS, escapechar=",")
            w.writeheader()
            w.writerows(self.log(e))


class Replay:
    """The closed loop of one experiment geometry over one track, for populations of controller configurations.

    `track`: a bboxes.csv path (read as the reference reads it) or a device float64 [N, 4] xywh tensor with NaN rows for missed detections.
    `frame_shape` (H, W): the frame the platform position is clamped to; default DummyReader's, orig_resolution + camera_size // 2 * 2 element by element."""

    def __init__(self, track, timing_config: TimingConfig, experiment_config: ExperimentConfig, frame_shape: Optional[Sequence[int]] = None, device: int = 0):
        if hip.device_count() < 1:
            raise hip.WtkError("Replay needs a GPU: no HIP device visible (there is no CPU fallback)")
        import torch

        tc, ec = timing_config, experiment_config
        self.timing_config, self.experiment_config = tc, ec
        self._dev = torch.device("cuda", device)
        if isinstance(track, (str, os.PathLike)):
            track = torch.from_numpy(np.ascontiguousarray(_read_track_csv(track), dtype=np.float64))
        elif isinstance(track, np.ndarray):
            track = torch.from_numpy(np.ascontiguousarray(track, dtype=np.float64))
        if track.dim() != 2 or track.shape[1] != 4 or track.dtype != torch.float64:
            raise ValueError(f"the track must be float64 [n_frames, 4] xywh, got {track.dtype} {tuple(track.shape)}")
        self.track = track.to(self._dev).contiguous()
        self.n_track = int(self.track.shape[0])
        cam, mic = tuple(int(v) for v in tc.camera_size_px), tuple(int(v) for v in tc.micro_size_px)
        if frame_shape is None:
            frame_shape = tuple(a + b for a, b in zip(ec.orig_resolution, (cam[0] // 2 * 2, cam[1] // 2 * 2)))
        self.frame_shape = (int(frame_shape[0]), int(frame_shape[1]))
        self.L, self.I, self.M, self.P = int(tc.cycle_frame_num), int(tc.imaging_frame_num), int(tc.moving_frame_num), int(tc.pred_frame_num)
        F = int(ec.num_frames)
        if self.I < 1 or self.M < 1 or F - 1 < self.I:
            raise ValueError("the experiment needs imaging_frame_num >= 1, moving_frame_num >= 1 and at least one decision frame")
        self.n_cycles = (F - 1 - self.I) // self.L + 1  # cycles whose decision frame c L + I exists
        self.n_log = (F - 1) // self.L                  # logged cycles: the last cycle's end never arrives
        self.n_rows = self.n_log * self.L
        if self.n_rows > self.n_track:
            raise ValueError(f"the track has {self.n_track} rows, the log of {F} frames needs {self.n_rows}")
        self._cfg = hip.replay_config(F, self.I, self.M, self.P, cam, mic, (self.frame_shape[1], self.frame_shape[0]), ec.init_position)
        # SineMotorController's profile, with numpy's cos as the reference computes it (never on the device)
        share = np.array([(np.cos((k * np.pi) / self.M) - np.cos(((k + 1) * np.pi) / self.M)) / 2 for k in range(self.M)], dtype=np.float64)
        self._share = torch.from_numpy(share).to(self._dev)
        self._cycles = torch.arange(self.n_cycles, dtype=torch.int32, device=self._dev)
        self._track_f32 = None

    # ------------------------------------------------------------------ targets
    def _stream(self) -> int:
        import torch

        return torch.cuda.current_stream(self._dev).cuda_stream

    def _empty(self, E: int, with_b: bool = False):
        import torch

        a = torch.zeros((self.n_cycles, E, 2), dtype=torch.float64, device=self._dev)
        b = torch.zeros((self.n_cycles, E, 2), dtype=torch.float64, device=self._dev) if with_b else None
        return a, b, torch.zeros((self.n_cycles, E), dtype=torch.int32, device=self._dev)

    def csv(self) -> Targets:
        """CsvController: centre the camera on the head as seen pred_frame_num frames before the decision (one experiment: it has no parameters)."""
        return Targets("csv", 1)

    def optimal(self) -> Targets:
        """OptimalController: the median head centre of the next imaging phase (wtk_track_median_centers)."""
        import torch

        a, _, valid = self._empty(1)
        pred, ok = torch.zeros((self.n_cycles, 2), dtype=torch.float64, device=self._dev), torch.zeros((self.n_cycles,), dtype=torch.int32, device=self._dev)
        with torch.cuda.device(self._dev):
            hip.track_median_centers(self.track, self.n_track, self._cycles, self.n_cycles, self.L, self.I, pred, ok, stream=self._stream())
        a[:, 0], valid[:, 0] = pred, ok
        return Targets("optimal", 1, a, None, valid)

    def polyfit(self, configs: Sequence[PolyfitConfig]) -> Targets:
        """PolyfitController, one experiment per config (degree, times and weights may all differ): wtk_track_polyfit per config on absolute centres,
        HipPolyfitController's convention.  Where a cycle keeps fewer finite samples than the fit has coefficients, numpy returns the minimum-norm
        solution, which is not translation invariant: such cycles can differ from the reference, which fits camera-relative centres."""
        import torch

        configs = list(configs)
        if not configs:
            raise ValueError("at least one PolyfitConfig is needed")
        E = len(configs)
        a, _, valid = self._empty(E)
        pred, ok = torch.zeros((self.n_cycles, 2), dtype=torch.float64, device=self._dev), torch.zeros((self.n_cycles,), dtype=torch.int32, device=self._dev)
        t_eval = self.L + self.I // 2
        with torch.cuda.device(self._dev):
            for e, cfg in enumerate(configs):
                hip.track_polyfit(self.track, self.n_track, self._cycles, self.n_cycles, self.L, cfg.sample_times, cfg.weights, cfg.degree, t_eval, pred, ok,
                                  stream=self._stream())
                a[:, e], valid[:, e] = pred, ok  # stream-ordered copies: `pred` is free again for the next config
        return Targets("polyfit", E, a, None, valid)

    def mlp(self, model, max_speed: float = 0.9) -> Targets:
        """MLPController: the ResMLP on the boxes around the frame seen pred_frame_num frames before the decision (wtk_mlp_predict_track on the float32
        track), clipped in float32 as HipMLPController clips; the float64 add of the first box's corner and the rounding happen in the scan."""
        import torch

        folded: FoldedResMLP = model if isinstance(model, FoldedResMLP) else from_torch_module(model)
        tc = self.timing_config
        max_dist = max_speed * (tc.px_per_mm / tc.frames_per_sec) * list(folded.pred_frames)[0]
        net = hip.HipMLP(folded.layers, folded.n_blocks, folded.layers_per_block, device=self._dev.index)
        a, b, valid = self._empty(1, with_b=True)
        with torch.cuda.device(self._dev):
            if self._track_f32 is None:
                self._track_f32 = self.track.to(torch.float32).contiguous()
            anchors = (self._cycles * self.L + (self.I - self.P)).contiguous()
            pred = torch.zeros((self.n_cycles, 2), dtype=torch.float32, device=self._dev)
            ok = torch.zeros((self.n_cycles,), dtype=torch.int32, device=self._dev)
            net.predict_track(self._track_f32, self.n_track, anchors, self.n_cycles, list(folded.input_frames), pred, ok, stream=self._stream())
            bound = float(np.float32(max_dist))
            a[:, 0] = torch.clamp(pred, -bound, bound).to(torch.float64)
            first = (anchors.to(torch.int64) + int(list(folded.input_frames)[0])).clamp(0, self.n_track - 1)  # only read where the sample is valid
            b[:, 0] = self.track[first, :2]
            valid[:, 0] = ok
        return Targets("mlp", 1, a, b, valid, keep=net)  # nothing is waited for: the handle lives as long as its targets

    # ------------------------------------------------------------------ the loop
    def run(self, targets: Targets, rows: Sequence[int] = (0,), per_row_errors: bool = False) -> ReplayResult:
        """Replay the E experiments of `targets`.  `rows`: the experiments whose full log rows are kept (16 doubles per row each)."""
        import torch

        if targets.kind not in KINDS:
            raise ValueError(f"unknown kind {targets.kind!r}")
        E, C, R = int(targets.E), self.n_cycles, self.n_rows
        for t in (targets.a, targets.b, targets.valid):
            if t is not None and (t.shape[0] != C or t.shape[1] != E or not t.is_contiguous()):
                raise ValueError("targets must be contiguous [n_cycles, E, ...] tensors of this Replay")
        row_ids = sorted({int(e) for e in rows})
        if any(e < 0 or e >= E for e in row_ids):
            raise IndexError(f"rows names an experiment outside [0, {E})")
        dev, f64, i32 = self._dev, torch.float64, torch.int32
        with torch.cuda.device(dev):
            stream = self._stream()
            pos = torch.empty((C, E, 2), dtype=i32, device=dev)
            move = torch.empty((C, E, 2), dtype=i32, device=dev)
            hip.replay_scan(self._cfg, KINDS[targets.kind], E, C, self.track, self.n_track, targets.a, targets.b, targets.valid, self._share, pos, move,
                            stream=stream)
            slot_host = np.full((E,), -1, dtype=np.int32)
            slot_host[row_ids] = np.arange(len(row_ids), dtype=np.int32)
            slots = torch.from_numpy(slot_host).to(dev) if row_ids else None
            row_data = torch.empty((len(row_ids), R, hip.REPLAY_ROW_DOUBLES), dtype=f64, device=dev) if row_ids else None
            bbox = torch.empty((E, R), dtype=f64, device=dev) if per_row_errors else None
            mse = torch.empty((E, R), dtype=f64, device=dev) if per_row_errors else None
            summary = torch.empty((E, hip.REPLAY_SUMMARY_DOUBLES), dtype=f64, device=dev)
            n_scratch = hip.replay_scratch_doubles(E, R)
            scratch = torch.empty((max(1, n_scratch),), dtype=f64, device=dev)
            hip.replay_rows(self._cfg, E, C, self.track, self.n_track, self._share, pos, move, slots, len(row_ids), row_data, bbox, mse, summary, scratch,
                            scratch.numel(), stream=stream)
            torch.cuda.current_stream(dev).synchronize()  # the one host synchronisation
            s = summary.cpu().numpy()
            res = ReplayResult(
                moves=move.permute(1, 0, 2).contiguous().cpu().numpy(), positions=pos.permute(1, 0, 2).contiguous().cpu().numpy(),
                summary=Summary(s[:, 0].copy(), s[:, 1].astype(np.int64), s[:, 2].copy(), s[:, 3].astype(np.int64), s[:, 4].astype(np.int64), s[:, 5].copy()),
                decision_frames=np.arange(C, dtype=np.int64) * self.L + self.I, row_ids=row_ids,
                row_data=row_data.cpu().numpy() if row_ids else np.zeros((0, R, hip.REPLAY_ROW_DOUBLES)),
                bbox_error=bbox.cpu().numpy() if per_row_errors else None, mse_error=mse.cpu().numpy() if per_row_errors else None)
        return res
