"""Closed-loop replay of track-driven experiments on the device, with tracking error: what the reference's `Simulator` + `SineMotorController` +
`LoggingController` (sim/simulator.py:140-194, sim/motor_controllers.py:58-88, sim_controllers/logging_controller.py:145-185) produce frame by frame for
one experiment, for a whole population of controller configurations at once (csrc/replay.hip and the replay_*.hip files it names).

    rp = Replay(track, timing_config, experiment_config)
    res = rp.run(rp.polyfit([PolyfitConfig(2, [-9, -6, -3, 0, 2, 4], w) for w in weight_vectors]), rows=[0])
    res.moves, res.positions          # [E, C, 2] int32
    res.summary.mean_bbox_error       # [E]
    res.log(0); res.to_csv(0, "bboxes.csv")

During the imaging phase the platform stands still, so a controller's move is round(f(target_c, platform position)) with a per-cycle target that does not
depend on the platform.  The builders (`csv`, `optimal`, `polyfit`, `mlp`) compute the targets of all cycles with the existing device calls; `run` scans
the cycles (one lane per experiment) and expands to frames.  Everything is enqueued on the current torch stream; `run` synchronises once.

The closed-loop error is also the objective of a weight search:

    t = rp.polyfit_population(weights_dev, 2, [-9, -6, -3, 0, 2, 4])   # [P, N] device weights, one call
    rp.objective(t)                                                     # device float64 [P], no synchronisation
    best = rp.optimize_polyfit(2, [-9, -6, -3, 0, 2, 4], start=[open_loop.weights])

With the experiment's frames attached, the same calls give the reference's analysis metric, the precise error (ErrorCalculator.calculate_precise: the
share of the worm's segmented pixels outside the microscope view), for the whole population: the segmented mask of a frame is built
once, as a summed-area table in LDS, and every experiment is answered with two rectangle sums.

    rp.attach_frames(device_frames, background, diff_thresh=20)        # CUDA uint8 [F, H, W], F >= n_rows; row r is frame r
    res = rp.run(t, precise=True, per_row_errors=True)
    res.precise_summary.trimmed_mean_precise_error                      # [E]; res.precise_error [E, R], res.precise_counts [E, R, 2]
    rp.objective(t, "trimmed_precise_error")                            # and optimize_polyfit(..., objective="trimmed_precise_error")

The YOLO controller's targets depend on the camera view, so its loop cannot be a scan over precomputed targets: `YoloReplay` enqueues the detector's
single-frame call and a small control kernel per cycle, all on one stream, and the log's detections afterwards in batches:

    yr = YoloReplay(device_frames, timing_config, experiment_config, yolo_config)   # what HipYoloController(tc, cfg, device_frames=...) takes
    res = yr.run()                    # a ReplayResult with E = 1, bit for bit the host loop's moves and log; one host synchronisation
    res.detections                    # device float32 [R, 4], view pixels

The reference's analysis workflow (DataAnalyzer.initialize / clean / change_unit / describe / calc_anomalies / print_stats and the Plotter's per-cycle
and per-cycle-step aggregates) of every experiment of a population, on the device (csrc/replay_analysis.hip):

    spec = Analysis(period=10, trim_cycles=True, imaging_only=True, bounds=(40, 40, 1500, 1300), unit="sec",
                    columns=["wrm_speed", "worm_deviation", "bbox_error"], percentiles=[0.5, 0.95], min_bbox_error=0.5)
    res = rp.run(t, analysis=spec)                                      # also YoloReplay.run(analysis=spec)
    res.analysis.describe                                               # [E, n_cols, 5 + Q]; .describe_table(e), .print_stats(e)
    res.analysis.cycle_max, res.analysis.step_quantiles, res.analysis.anomaly_counts, res.analysis.stats
    rp.analyze(t, spec)                                                 # the same as device tensors, no synchronisation

Several recordings in one objective: a population replayed on T tracks of different lengths in a number of launches that
does not depend on T, the error pooled over the rows of all logs; the search and the trainer's closed loop run on the set unchanged:

    rs = ReplaySet([track0, "bboxes1.csv", track2], timing_config, [ec0, ec1, ec2])
    rs.objective(rs.polyfit_population(weights_dev, 2, times))          # device float64 [P]; per_track=True -> [T, P]
    rs.optimize_polyfit(2, times, start=[open_loop.weights]); trainer.fit(..., closed_loop=rs); rs.replay(t)   # the plain Replay of track t

With every track's frames attached the set gives the precise error too: each track with its own frames, background, frame shape
and threshold, five launches whatever T is, per-track summaries with `rs.replay(t)`'s bits and the objective pooled over the rows of all logs:

    rs.attach_frames([frames0, frames1, frames2], [bg0, bg1, bg2], diff_thresh=20)
    rs.objective(tg, "trimmed_precise_error")                           # also per_track=True, optimize_polyfit(..., objective=...), fit(closed_loop=rs, ...)
    rs.run(tg, precise=True).precise_summary                            # .track_precise_summary[t]; per_row_errors=True: .precise_error[t], .precise_counts[t]

The analysis of the set: every log through its own initialize / clean / change_unit, then the statistics of each log and of the
concatenation of all logs, as the reference's Plotter takes them; a percentile over all recordings is exact, not a combination of per-track ones:

    res = rs.run_analysis(tg, spec)                                     # res.analysis.pooled.describe [E, n_cols, 5 + Q]; .track[t] = rs.replay(t)'s bits
    rs.analyze(tg, spec)                                                # the same as device tensors, no synchronisation; precise=True: precise_error

Recordings taken at different scales: one TimingConfig per track, as the reference derives the camera and microscope sizes in
pixels, the MLP's clip bound and change_unit's factors from each recording's own px_per_mm; everything above works unchanged, pair by pair with the
bits of `Replay(track_t, timing_configs[t], experiment_configs[t])`.  The same recording entered with G microscope sizes is a field-of-view sweep:

    rs = ReplaySet.from_experiments(tracks, [ec0, ec1, ec2], 200, 40, 50, camera_size_mm=(4, 4), micro_size_mm=(0.32, 0.32))   # or ReplaySet(tracks, [tc0, tc1, tc2], ecs)
    ReplaySet([track] * 4, [tc_small, tc_mid, tc_large, tc_huge], ec).objective(tg, "bbox_error", per_track=True)              # [4, E]

There is no CPU fallback: without a visible GPU the constructors raise.  Not covered: `StepMotorController`, DataAnalyzer's `remove_cycle` and
`save` / `load`, the plots themselves, the YOLO controller's second look (YoloConfig.recheck_margin).
"""
from __future__ import annotations

import csv as _csv
import math
import os
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import hip, yolo_spec
from .controllers import PolyfitConfig, YoloConfig, _raise_on_overflow, _read_track_csv, check_device_frames
from .polyfit_opt import SwarmResult, _check_degree, check_swarm_args, check_times, polyfit_config, swarm_search, weights_to_device
from .resmlp import FoldedResMLP, from_torch_module, pack_blob
from .sim import LOG_COLUMNS, ExperimentConfig, TimingConfig

KINDS = {"csv": hip.REPLAY_CSV, "optimal": hip.REPLAY_OPTIMAL, "polyfit": hip.REPLAY_POLYFIT, "mlp": hip.REPLAY_MLP}
OBJECTIVES = hip.REPLAY_OBJECTIVES  # name -> WTK_REPLAY_OBJ_*; each is the Summary property of the same name prefixed with `mean_` / `trimmed_mean_`
# name -> WTK_REPLAY_POBJ_*: PreciseSummary.trimmed_mean_precise_error, .mean_precise_error, .non_perfect; they need attach_frames
PRECISE_OBJECTIVES = hip.REPLAY_PRECISE_OBJECTIVES


def polyfit_classes(track: np.ndarray, cycle_frame_num: int, n_cycles: int, sample_times) -> tuple:
    """The cycles of a track grouped by WHICH samples of the fit exist: -> (cycle_class int32 [n_cycles], class_mask int32 [K]).  Bit j of a mask:
    frame c L + sample_times[j] lies inside the track and its centre (x + w / 2, y + h / 2) is finite.  Classes are numbered by ascending mask."""
    st = np.asarray(sample_times, dtype=np.int64)
    frames = np.arange(n_cycles, dtype=np.int64)[:, None] * int(cycle_frame_num) + st[None, :]
    inside = (frames >= 0) & (frames < len(track))
    rows = track[np.where(inside, frames, 0)]
    with np.errstate(invalid="ignore", over="ignore"):
        finite = inside & np.isfinite(rows[..., 0] + rows[..., 2] / 2) & np.isfinite(rows[..., 1] + rows[..., 3] / 2)
    masks = (finite.astype(np.int64) << np.arange(len(st), dtype=np.int64)[None, :]).sum(axis=1)
    class_mask, cycle_class = np.unique(masks, return_inverse=True)
    return cycle_class.reshape(-1).astype(np.int32), class_mask.astype(np.int32)


def check_timing_configs(timing_configs, T: int) -> list:
    """The T TimingConfigs of a ReplaySet's tracks as a list.  The tracks of a set share ONE cycle structure (the super-track, the [n_super_cycles, E]
    arrays and every targets call rest on one cycle length), so the three frame counts must be equal; the sizes and px_per_mm may differ.  Refused,
    naming the track: another number of configs than tracks, frame counts that differ from track 0's, a camera smaller than the microscope."""
    tcs = list(timing_configs)
    if len(tcs) != T:
        raise ValueError(f"{T} tracks: timing_config must be one TimingConfig or a sequence of {T}, got {len(tcs)}")
    counts = lambda tc: (int(tc.imaging_frame_num), int(tc.moving_frame_num), int(tc.pred_frame_num))  # noqa: E731
    for t, tc in enumerate(tcs):
        if not isinstance(tc, TimingConfig):
            raise ValueError(f"track {t}: timing_config must hold TimingConfigs, got {type(tc).__name__}")
        if counts(tc) != counts(tcs[0]):
            raise ValueError(f"track {t}: (imaging_frame_num, moving_frame_num, pred_frame_num) = {counts(tc)}, track 0 has {counts(tcs[0])}: the tracks of a "
                             "set share one cycle structure (per-track frame counts are not supported)")
        cam, mic = tuple(int(v) for v in tc.camera_size_px), tuple(int(v) for v in tc.micro_size_px)
        if cam[0] < mic[0] or cam[1] < mic[1] or min(mic) < 0:
            raise ValueError(f"track {t}: the camera {cam} is smaller than the microscope {mic}")
    return tcs


def mlp_clip_bound(timing_config: TimingConfig, max_speed: float, pred_frames) -> float:
    """The float32 bound MLPController clips a prediction to: the distance a worm of `max_speed` mm/s covers until the first predicted frame."""
    max_dist = max_speed * (timing_config.px_per_mm / timing_config.frames_per_sec) * list(pred_frames)[0]
    return float(np.float32(max_dist))


def population_frames(input_frames, pred_frames) -> tuple:
    """(input_frames, pred_frames) of a population as int lists; refuses a population that does not say which frames its models read and predict."""
    if input_frames is None or pred_frames is None or len(input_frames) == 0 or len(pred_frames) == 0:
        raise ValueError("mlp_population needs the models' input_frames and pred_frames (a trainer built from state dicts takes them as entries of the dict)")
    return [int(v) for v in input_frames], [int(v) for v in pred_frames]


def sine_shares(M: int) -> np.ndarray:
    """SineMotorController's profile (the share of a move made in each of the M moving frames), with numpy's cos as the reference computes it."""
    return np.array([(np.cos((k * np.pi) / M) - np.cos(((k + 1) * np.pi) / M)) / 2 for k in range(M)], dtype=np.float64)


@dataclass(frozen=True, eq=False)
class LoopGeometry:
    """The closed loop's sizes, derived once from the configs and needing no GPU: cycle length L = I imaging + M moving frames, the decision looks P
    frames back; n_cycles cycles whose decision frame c L + I exists, n_log logged cycles (the last cycle's end never arrives), n_rows = n_log L rows."""

    L: int
    I: int
    M: int
    P: int
    cam: tuple          # (w, h), as mic
    mic: tuple
    frame_shape: tuple  # (H, W): the platform position is clamped to it
    n_cycles: int
    n_log: int
    n_rows: int
    decision_frames: np.ndarray  # int64 [n_cycles]
    config: object      # the wtk_replay_config of all that

    @classmethod
    def of(cls, timing_config: TimingConfig, experiment_config: ExperimentConfig, frame_shape: Optional[Sequence[int]] = None) -> "LoopGeometry":
        """`frame_shape` (H, W): default DummyReader's.  Refuses what wtk_replay_scan / wtk_replay_rows refuse about an experiment (they do so again)."""
        tc, ec = timing_config, experiment_config
        cam, mic = tuple(int(v) for v in tc.camera_size_px), tuple(int(v) for v in tc.micro_size_px)
        if frame_shape is None:
            frame_shape = tuple(a + b for a, b in zip(ec.orig_resolution, (cam[0] // 2 * 2, cam[1] // 2 * 2)))
        H, W = int(frame_shape[0]), int(frame_shape[1])
        L, I, M, P, F = int(tc.cycle_frame_num), int(tc.imaging_frame_num), int(tc.moving_frame_num), int(tc.pred_frame_num), int(ec.num_frames)
        if I < 1 or M < 1 or F - 1 < I:
            raise ValueError("the experiment needs imaging_frame_num >= 1, moving_frame_num >= 1 and at least one decision frame")
        if not 0 <= P <= I:
            raise ValueError(f"pred_frame_num = {P} lies outside [0, imaging_frame_num = {I}]")
        if cam[0] < mic[0] or cam[1] < mic[1] or min(mic) < 0:
            raise ValueError(f"the camera {cam} is smaller than the microscope {mic}")
        n_cycles, n_log = (F - 1 - I) // L + 1, (F - 1) // L
        return cls(L, I, M, P, cam, mic, (H, W), n_cycles, n_log, n_log * L, np.arange(n_cycles, dtype=np.int64) * L + I,
                   hip.replay_config(F, I, M, P, cam, mic, (W, H), ec.init_position))


def _adopt(owner, g: LoopGeometry) -> None:
    """Replay's and YoloReplay's public sizes are their geometry's."""
    owner.geometry, owner._cfg, owner.frame_shape = g, g.config, g.frame_shape
    owner.L, owner.I, owner.M, owner.P, owner.n_cycles, owner.n_log, owner.n_rows = g.L, g.I, g.M, g.P, g.n_cycles, g.n_log, g.n_rows


def _result_of(g: LoopGeometry, pos, move, summary, row_ids, row_data, bbox=None, mse=None, detections=None) -> "ReplayResult":
    """The ReplayResult of device pos / move [C, E, 2], summary [E, 6], kept rows [len(row_ids), R, 16], per-row errors [E, R] or None; after the wait."""
    host = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
    return ReplayResult(moves=host(move.permute(1, 0, 2).contiguous()), positions=host(pos.permute(1, 0, 2).contiguous()), summary=_summary_of(host(summary)),
                        decision_frames=g.decision_frames.copy(), row_ids=row_ids,
                        row_data=host(row_data) if row_ids else np.zeros((0, g.n_rows, hip.REPLAY_ROW_DOUBLES)), bbox_error=host(bbox), mse_error=host(mse),
                        detections=detections)


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


@dataclass
class PreciseSummary:
    """Per-experiment figures of the precise error ([E] arrays).  Rows whose logged worm box is illegal (a missed detection, no area inside the frame)
    have no value: they are counted in `nan_rows` and enter no sum, as in pandas' mean over DataAnalyzer's precise_error column.  `trimmed`: as Summary."""

    precise_error_sum: np.ndarray
    rows: np.ndarray  # rows with a value
    trimmed_precise_error_sum: np.ndarray
    trimmed_rows: np.ndarray
    non_perfect_rows: np.ndarray  # rows with precise_error > 1e-7
    nan_rows: np.ndarray

    @property
    def mean_precise_error(self) -> np.ndarray:
        return self.precise_error_sum / self.rows

    @property
    def trimmed_mean_precise_error(self) -> np.ndarray:
        return self.trimmed_precise_error_sum / self.trimmed_rows

    @property
    def non_perfect(self) -> np.ndarray:
        return self.non_perfect_rows / self.rows


ANALYSIS_COLUMNS = hip.ANALYSIS_COLUMNS  # the columns of DataAnalyzer's table; the position is the WTK_ANALYSIS_COL_* id
ANOMALY_KINDS = ("speed", "bbox_error", "dist_error", "width", "height", "no_pred")  # bit k of anomaly_mask, column k of anomaly_counts (column 6: any)


@dataclass
class Analysis:
    """What to compute of every replayed experiment, in the reference's terms: `period` of DataAnalyzer.initialize; `trim_cycles`, `imaging_only`,
    `bounds` (x0, y0, x1, y1) of clean (trim_cycles drops cycle 0 and the largest cycle that survives the other two filters); `unit` "frame" or "sec"
    of change_unit; `columns` (names of ANALYSIS_COLUMNS) and `percentiles` (in [0, 1]) of describe and of the per-cycle and per-cycle-step
    aggregates; the thresholds of calc_anomalies (`min_size` for both sides of the worm box; inf = off), applied to the unit-changed values.
    `anomaly_mask`: also return the per-row bit flags [E, R].  On a ReplaySet with one TimingConfig per track the unit factors are each track's own
    (`factors(rs.timing_configs)`), and the thresholds are compared with the values so converted; `bounds` stays ONE rectangle in pixels for all tracks
    (each recording's platform moves in its own frame: give bounds that fit all of them, or analyse a track alone with `rs.replay(t)`)."""

    period: int = 10
    trim_cycles: bool = False
    imaging_only: bool = False
    bounds: Optional[Sequence[float]] = None
    unit: str = "frame"
    columns: Sequence[str] = ("wrm_speed", "worm_deviation", "bbox_error")
    percentiles: Sequence[float] = (0.25, 0.5, 0.75)
    no_preds: bool = True
    min_bbox_error: float = math.inf
    min_dist_error: float = math.inf
    min_speed: float = math.inf
    min_size: float = math.inf
    anomaly_mask: bool = False

    def column_ids(self) -> list:
        unknown = [c for c in self.columns if c not in ANALYSIS_COLUMNS]
        if unknown or not self.columns:
            raise ValueError(f"unknown analysis columns {unknown}: one or more of {ANALYSIS_COLUMNS}")
        if len(self.columns) > hip.ANALYSIS_MAX_COLUMNS or len(self.percentiles) > hip.ANALYSIS_MAX_PERCENTILES:
            raise ValueError(f"at most {hip.ANALYSIS_MAX_COLUMNS} columns and {hip.ANALYSIS_MAX_PERCENTILES} percentiles")
        return [ANALYSIS_COLUMNS.index(c) for c in self.columns]

    def factors(self, timing_config) -> tuple:
        """(time, distance, speed) factors of change_unit(unit), as the reference computes them from the log's own TimingConfig.  A sequence of
        configs (a ReplaySet's `timing_configs`) gives the list of one triple per track: every log of a set is converted with its own."""
        if not isinstance(timing_config, TimingConfig):
            return [self.factors(tc) for tc in timing_config]
        if self.unit == "frame":
            return (1.0, 1.0, 1.0)
        if self.unit != "sec":
            raise ValueError(f"unit must be 'frame' or 'sec', got {self.unit!r}")
        dist, tf = timing_config.mm_per_px * 1000, timing_config.ms_per_frame / 1000
        return (tf, dist, dist / tf)

    def config(self, timing_config: TimingConfig):
        if self.bounds is not None and len(self.bounds) != 4:
            raise ValueError("bounds must be (x0, y0, x1, y1)")
        return hip.replay_analysis_config(self.period, self.imaging_only, self.bounds, self.trim_cycles, self.factors(timing_config), self.min_speed,
                                          self.min_bbox_error, self.min_dist_error, self.min_size, self.min_size, self.no_preds)


@dataclass
class AnalysisResult:
    """The analysis of E experiments (numpy arrays after `run`, device tensors from `Replay.analyze`): describe [E, n_cols, 5 + Q] (count, mean, std,
    min, the percentiles, max over the kept rows), cycle_max / cycle_mean [E, n_log, n_cols], step_quantiles [E, L, n_cols, Q], step_count
    [E, L, n_cols], anomaly_counts [E, 7] (ANOMALY_KINDS and any), stats [E, 4] (removed rows, kept rows without a prediction, distinct cycles kept,
    kept rows with bbox_error > 1e-7), anomaly_mask [E, R] uint8 bit flags or None.  NaN: no value (an empty segment, the std of a single row)."""

    columns: list
    percentiles: list
    n_rows: int
    describe: object
    cycle_max: object
    cycle_mean: object
    step_quantiles: object
    step_count: object
    anomaly_counts: object
    stats: object
    anomaly_mask: object = None

    @property
    def describe_index(self) -> list:
        """The row names of DataAnalyzer.describe's table."""
        return ["count", "mean", "std", "min"] + [f"{100 * q:g}%" for q in self.percentiles] + ["max"]

    def describe_table(self, e: int):
        """Experiment e's describe table as DataAnalyzer.describe lays it out: (row names, column names, values [5 + Q, n_cols])."""
        return self.describe_index, list(self.columns), np.asarray(self.describe[e]).T.copy()

    def print_stats(self, e: int) -> None:
        """DataAnalyzer.print_stats for experiment e."""
        removed, no_pred, cycles, non_perfect = (int(v) for v in self.stats[e])
        kept = self.n_rows - removed
        pct = lambda a, b: round(100 * a / b, 3) if b else float("nan")  # noqa: E731
        print(f"Count of Removed Frames: {removed} ({pct(removed, self.n_rows)}%)")
        print(f"Count of No-Pred Frames: {no_pred} ({pct(no_pred, kept)}%)")
        print(f"Total Num of Cycles: {cycles}")
        print(f"Non Perfect Predictions: {pct(non_perfect, kept)}%")


def _enqueue_analysis(geometry: "LoopGeometry", timing_config, spec: Analysis, E: int, track, n_track: int, share, pos, move, pair, stream: int,
                      max_lds_rows: int = 0) -> AnalysisResult:
    """wtk_replay_analyze on a scan's pos / move: an AnalysisResult of device tensors.  `pair`: the per-pair precise errors [R, E] or None."""
    import torch

    g, dev = geometry, pos.device
    cols, q = spec.column_ids(), [float(v) for v in spec.percentiles]
    n, Q, f64 = len(cols), len(q), torch.float64
    out = AnalysisResult(list(spec.columns), q, g.n_rows, torch.empty((E, n, 5 + Q), dtype=f64, device=dev), torch.empty((E, g.n_log, n), dtype=f64, device=dev),
                         torch.empty((E, g.n_log, n), dtype=f64, device=dev), torch.empty((E, g.L, n, Q), dtype=f64, device=dev),
                         torch.empty((E, g.L, n), dtype=torch.int32, device=dev), torch.empty((E, 7), dtype=torch.int64, device=dev),
                         torch.empty((E, 4), dtype=torch.int64, device=dev),
                         torch.empty((E, g.n_rows), dtype=torch.uint8, device=dev) if spec.anomaly_mask else None)
    scratch = torch.empty((max(1, hip.replay_analysis_scratch_doubles(E, g.n_rows, n, Q)),), dtype=f64, device=dev)
    hip.replay_analyze(g.config, spec.config(timing_config), E, g.n_cycles, track, n_track, share, pos, move, pair, cols, q, int(max_lds_rows), out.describe,
                       out.cycle_max, out.cycle_mean, out.step_quantiles, out.step_count, out.anomaly_counts, out.anomaly_mask, out.stats, scratch,
                       scratch.numel(), stream=stream)
    return out


def _analysis_to_host(a: AnalysisResult) -> AnalysisResult:
    host = lambda t: None if t is None else np.ascontiguousarray(t.cpu().numpy())  # noqa: E731  (a set's per-track cycle arrays and masks are slices)
    return AnalysisResult(a.columns, a.percentiles, a.n_rows, host(a.describe), host(a.cycle_max), host(a.cycle_mean), host(a.step_quantiles), host(a.step_count),
                          host(a.anomaly_counts), host(a.stats), host(a.anomaly_mask))


@dataclass
class SetAnalysisResult:
    """The analysis of E experiments replayed on T tracks (`ReplaySet.analyze` / `run_analysis`).  `track[t]`: the AnalysisResult
    of log t of every experiment, bit-equal to `rs.replay(t).analyze` on that track alone.  `pooled`: the same statistics over the concatenation of the T
    cleaned logs of an experiment in track order, as the reference's Plotter concatenates them: describe, step_quantiles and step_count over all kept
    rows (order statistics exact), anomaly_counts and stats summed over the tracks, n_rows the rows of all logs; its cycle_max / cycle_mean
    [E, sum n_log, n_cols] are groupby(["log_num", "cycle"]) (track t's cycles follow those of the tracks before it) and its anomaly_mask
    [E, sum R] the tracks' masks side by side."""

    pooled: AnalysisResult
    track: list


class ReplayResult:
    """moves, positions [E, C, 2] int32 (the move of cycle c and the platform position at its start); summary; bbox_error / mse_error [E, R] float64 when
    requested; the full log rows of the experiments named in `rows`; `detections` (YoloReplay only): device float32 [R, 4] xywh in view pixels.
    After `Replay.run(precise=True)`: `precise_summary`, and with per-row errors `precise_error` [E, R] float64 (NaN = no value) and `precise_counts`
    [E, R, 2] int32 (foreground pixels of the worm crop, those of them inside the microscope view); None otherwise.  After `run(analysis=spec)`:
    `analysis`, an AnalysisResult of numpy arrays."""

    precise_summary = precise_error = precise_counts = analysis = None

    def __init__(self, moves, positions, summary, decision_frames, row_ids, row_data, bbox_error, mse_error, detections=None):
        self.moves, self.positions, self.summary, self.decision_frames = moves, positions, summary, decision_frames
        self.bbox_error, self.mse_error, self.detections = bbox_error, mse_error, detections
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
        _adopt(self, LoopGeometry.of(tc, ec, frame_shape))
        if self.n_rows > self.n_track:
            raise ValueError(f"the track has {self.n_track} rows, the log of {int(ec.num_frames)} frames needs {self.n_rows}")
        self._share = torch.from_numpy(sine_shares(self.M)).to(self._dev)
        self._cycles = torch.arange(self.n_cycles, dtype=torch.int32, device=self._dev)
        self._track_f32 = None
        self._anchors = None  # mlp_population's anchor frames
        self._classes = {}  # sorted sample times -> (cycle_class, class_mask) on the device
        self._last_times = None  # of the last polyfit_population / optimize_polyfit call (to_config's default)
        self._frames = self._background = None  # attach_frames
        self._diff_thresh = 20.0

    def attach_frames(self, frames, background, diff_thresh: float = 20) -> None:
        """The experiment's frames, for the precise error (`run(precise=True)`, the precise objectives): `frames` a contiguous CUDA uint8 [F, H, W]
        tensor, read in place (row r of the log is frame r, so F >= n_rows; (H, W) is this Replay's frame_shape); `background` [H, W], host or device,
        uint8 (evaluation.background) or floating with values in [0, 256), which are truncated as the reference's astype(int32) truncates them; a
        pixel is segmented where |frame - background| > diff_thresh (DataAnalyzer.calc_precise_error's default: 20)."""
        import torch

        check_device_frames(frames)
        if frames.dim() != 3:
            raise ValueError("the precise error takes gray frames [F, H, W] only")
        F, H, W = (int(v) for v in frames.shape)
        if (H, W) != tuple(self.frame_shape):
            raise ValueError(f"the frames are {H} x {W}, this Replay's frame is {self.frame_shape[0]} x {self.frame_shape[1]}")
        if F < self.n_rows:
            raise ValueError(f"{F} frames, the log has {self.n_rows} rows (row r is frame r)")
        if H * W > 2 ** 30:
            raise ValueError("frames of at most 2^30 pixels")
        bg = background if hasattr(background, "dim") else torch.from_numpy(np.ascontiguousarray(background))
        if tuple(bg.shape) != (H, W):
            raise ValueError(f"the background must be [{H}, {W}], got {tuple(bg.shape)}")
        if bg.dtype != torch.uint8:
            if not bg.dtype.is_floating_point:
                raise ValueError("the background must be uint8 or floating")
            bg = bg.to(torch.float64).trunc()
            if not bool(((bg >= 0) & (bg <= 255)).all()):
                raise ValueError("a floating background must hold values in [0, 256)")
            bg = bg.to(torch.uint8)
        self._frames, self._background, self._diff_thresh = frames, bg.to(frames.device).contiguous(), float(diff_thresh)

    # ------------------------------------------------------------------ targets
    def _stream(self) -> int:
        import torch

        return torch.cuda.current_stream(self._dev).cuda_stream

    def _empty(self, E: int, with_b: bool = False, pred_dtype=None):
        """Zeroed targets a, b (or None), valid of E experiments, and one predictor call's outputs pred [C, 2] (float64 unless named), ok [C]."""
        import torch

        zeros = lambda shape, dtype: torch.zeros((self.n_cycles,) + shape, dtype=dtype, device=self._dev)  # noqa: E731
        return (zeros((E, 2), torch.float64), zeros((E, 2), torch.float64) if with_b else None, zeros((E,), torch.int32),
                zeros((2,), pred_dtype or torch.float64), zeros((), torch.int32))

    def csv(self) -> Targets:
        """CsvController: centre the camera on the head as seen pred_frame_num frames before the decision (one experiment: it has no parameters)."""
        return Targets("csv", 1)

    def optimal(self) -> Targets:
        """OptimalController: the median head centre of the next imaging phase (wtk_track_median_centers)."""
        import torch

        a, _, valid, pred, ok = self._empty(1)
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
        a, _, valid, pred, ok = self._empty(E)
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
        bound = self._mlp_bound(max_speed, folded.pred_frames)
        net = hip.HipMLP(folded.layers, folded.n_blocks, folded.layers_per_block, device=self._dev.index)
        a, b, valid, pred, ok = self._empty(1, with_b=True, pred_dtype=torch.float32)
        with torch.cuda.device(self._dev):
            if self._track_f32 is None:
                self._track_f32 = self.track.to(torch.float32).contiguous()
            anchors = (self._cycles * self.L + (self.I - self.P)).contiguous()
            net.predict_track(self._track_f32, self.n_track, anchors, self.n_cycles, list(folded.input_frames), pred, ok, stream=self._stream())
            if hasattr(bound, "data_ptr"):  # a set with per-track configs: one bound per cycle
                bound = bound[:, None]
            a[:, 0] = torch.clamp(pred, -bound, bound).to(torch.float64)
            first = (anchors.to(torch.int64) + int(list(folded.input_frames)[0])).clamp(0, self.n_track - 1)  # only read where the sample is valid
            b[:, 0] = self.track[first, :2]
            valid[:, 0] = ok
        return Targets("mlp", 1, a, b, valid, keep=net)  # nothing is waited for: the handle lives as long as its targets

    def mlp_population(self, models, max_speed: float = 0.9, which="current") -> Targets:
        """`mlp(model)` of every model of a population in one call and with the same bits (wtk_replay_mlp_targets).  `models`: a
        `HipMLPTrainer` — its states are folded on the device (`which`: "current", "best" by validation loss, "scored" by keep_scored / fit(closed_loop=...)),
        nothing leaves the device and nothing is waited for — or a list of `FoldedResMLP` / live `WormPredictor`s of one structure, folded on the host and
        uploaded once.  Experiment e of the result is model e."""
        import torch

        from .training import HipMLPTrainer, state_slot

        state_slot(which)
        if isinstance(models, HipMLPTrainer):
            xi, yi = population_frames(models.input_frames, models.pred_frames)
            (layers, n_blocks, per_block), E = models.blob_structure(), models.E
            if models.out_dim != 2:
                raise ValueError(f"the replay takes predictors of one frame (out_dim 2), the trainer's models have out_dim {models.out_dim}")
            blob = models.folded_blob(which)
        else:
            folded = [m if isinstance(m, FoldedResMLP) else from_torch_module(m) for m in models]
            if not folded:
                raise ValueError("at least one model is needed")
            f0, E = folded[0], len(folded)
            xi, yi = population_frames(f0.input_frames, f0.pred_frames)
            key = lambda f: ([(w.shape, bool(r)) for w, _, r in f.layers], f.n_blocks, f.layers_per_block, list(f.input_frames), list(f.pred_frames))  # noqa: E731
            if any(key(f) != key(f0) for f in folded[1:]):
                raise ValueError("all models of a population must have the same structure, input_frames and pred_frames")
            if f0.out_dim != 2:
                raise ValueError(f"the replay takes predictors of one frame (out_dim 2), the models have out_dim {f0.out_dim}")
            layers, n_blocks, per_block = hip.mlp_structure([(w.shape[1], w.shape[0], r) for w, _, r in f0.layers]), f0.n_blocks, f0.layers_per_block
            blob = torch.from_numpy(np.stack([pack_blob(f) for f in folded])).to(self._dev)
        bound = self._mlp_bound(max_speed, yi)
        dev, C = self._dev, self.n_cycles
        tg = Targets("mlp", E, torch.empty((C, E, 2), dtype=torch.float64, device=dev), torch.empty((C, E, 2), dtype=torch.float64, device=dev),
                     torch.empty((C, E), dtype=torch.int32, device=dev), keep=blob)
        with torch.cuda.device(dev):
            if self._track_f32 is None:
                self._track_f32 = self.track.to(torch.float32).contiguous()
            if self._anchors is None:
                self._anchors = (self._cycles * self.L + (self.I - self.P)).contiguous()
            hip.replay_mlp_targets(layers, n_blocks, per_block, blob, E, self._track_f32, self.track, self.n_track, self._anchors, C, xi, bound, tg.a, tg.b,
                                   tg.valid, stream=self._stream())
        return tg

    def _mlp_bound(self, max_speed: float, pred_frames):
        """The clip bound of `mlp` / `mlp_population`: one float for every cycle (a ReplaySet's super-track: a device float32 [n_cycles] tensor)."""
        return mlp_clip_bound(self.timing_config, max_speed, pred_frames)

    # ------------------------------------------------------------------ populations of weight vectors
    def _sample_times(self, sample_times) -> tuple:
        return tuple(int(t) for t in check_times(sample_times, "sample_times"))

    def polyfit_class_table(self, sample_times) -> tuple:
        """(cycle_class int32 [n_cycles], class_mask int32 [K]) device tensors for the sorted `sample_times`: derived from the track once (the first
        call copies the track to the host and waits for it) and cached, so nothing inside an epoch loop ever asks for it."""
        import torch

        st = self._sample_times(sample_times)
        if st not in self._classes:
            cycle_class, class_mask = polyfit_classes(self.track.cpu().numpy(), self.L, self.n_cycles, st)
            self._classes[st] = (torch.from_numpy(cycle_class).to(self._dev), torch.from_numpy(class_mask).to(self._dev))
        return self._classes[st]

    def _enqueue_population(self, w_dev, degree: int, st: tuple, classes, a, valid, scratch, stop_dev=None):
        cycle_class, class_mask = classes
        hip.replay_polyfit_targets(self.track, self.n_track, self.n_cycles, self.L, w_dev, int(w_dev.shape[0]), st, degree, self.L + self.I // 2, cycle_class,
                                   class_mask, int(class_mask.numel()), a, valid, scratch, scratch.numel(), stop_dev, stream=self._stream())

    def _population_buffers(self, P: int, st: tuple, degree: int, alloc) -> tuple:
        """For a population call: (Targets of P experiments with a / valid from `alloc`, the fit's scratch, the class table of the sample times `st`)."""
        import torch

        dev, C, classes = self._dev, self.n_cycles, self.polyfit_class_table(st)
        self._last_times = st
        n_scratch = hip.replay_polyfit_targets_scratch_doubles(int(classes[1].numel()), P, len(st), degree)
        return (Targets("polyfit", P, alloc((C, P, 2), dtype=torch.float64, device=dev), None, alloc((C, P), dtype=torch.int32, device=dev)),
                torch.empty((max(1, n_scratch),), dtype=torch.float64, device=dev), classes)

    def polyfit_population(self, weights, degree: int, sample_times) -> Targets:
        """`polyfit([PolyfitConfig(degree, sample_times, w) for w in weights])` in one call and with the same bits: `weights` [P, N] is a device float64
        tensor (used in place) or an array (uploaded); row p's weight j belongs to the j-th smallest sample time.  Two launches whatever P is; nothing
        is waited for (but the first call for a set of sample times derives the class table from the track, see polyfit_class_table)."""
        import torch

        degree, st = _check_degree(degree), self._sample_times(sample_times)
        w = weights_to_device(self, weights, len(st), "sample time", min_rows=1)
        tg, scratch, classes = self._population_buffers(int(w.shape[0]), st, degree, torch.empty)
        with torch.cuda.device(self._dev):
            self._enqueue_population(w, degree, st, classes, tg.a, tg.valid, scratch)
        return tg

    def _objective_kind(self, kind: str) -> int:
        """The WTK_REPLAY_OBJ_* value of a name of OBJECTIVES, the WTK_REPLAY_POBJ_* value of a name of PRECISE_OBJECTIVES."""
        if kind not in OBJECTIVES and kind not in PRECISE_OBJECTIVES:
            raise ValueError(f"unknown objective {kind!r}: one of {sorted(OBJECTIVES)}, or with attach_frames one of {sorted(PRECISE_OBJECTIVES)}")
        if kind in ("trimmed_bbox_error", "trimmed_precise_error") and self.n_log < 3:
            raise ValueError(f"the trimmed objective drops the first and the last logged cycle: the experiment logs {self.n_log}, at least 3 are needed")
        if kind in PRECISE_OBJECTIVES:
            self._need_frames()
            return PRECISE_OBJECTIVES[kind]
        return OBJECTIVES[kind]

    def _need_frames(self) -> None:
        if self._frames is None:
            raise ValueError("the precise error needs the experiment's frames: call attach_frames(frames, background) first")

    def _objective_buffers(self, E: int) -> dict:
        import torch

        dev, C = self._dev, self.n_cycles
        return dict(pos=torch.empty((C, E, 2), dtype=torch.int32, device=dev), move=torch.empty((C, E, 2), dtype=torch.int32, device=dev),
                    summary=torch.empty((E, hip.REPLAY_SUMMARY_DOUBLES), dtype=torch.float64, device=dev),
                    scratch=torch.empty((max(1, hip.replay_scratch_doubles(E, self.n_rows)),), dtype=torch.float64, device=dev))

    def _precise_buffers(self, E: int) -> dict:
        import torch

        return dict(summary=torch.empty((E, hip.REPLAY_PRECISE_SUMMARY_DOUBLES), dtype=torch.float64, device=self._dev),
                    scratch=torch.empty((max(1, hip.replay_precise_scratch_doubles(E, self.n_rows)),), dtype=torch.float64, device=self._dev))

    def _enqueue_objective(self, targets: Targets, kind: int, buf: dict, out, stop_dev=None):
        """`kind`: _objective_kind's value; a precise objective where `buf` holds the precise buffers (_all_objective_buffers)."""
        if "precise" in buf:
            fr, pb = self._frames, buf["precise"]
            hip.replay_precise_objective(self._cfg, KINDS[targets.kind], int(targets.E), self.n_cycles, self.track, self.n_track, targets.a, targets.b,
                                         targets.valid, self._share, buf["pos"], buf["move"], fr, int(fr.shape[0]), int(fr.shape[1]), int(fr.shape[2]),
                                         self._background, self._diff_thresh, 0, pb["summary"], pb["scratch"], pb["scratch"].numel(), kind, out, stop_dev,
                                         stream=self._stream())
            return
        hip.replay_objective(self._cfg, KINDS[targets.kind], int(targets.E), self.n_cycles, self.track, self.n_track, targets.a, targets.b, targets.valid,
                             self._share, buf["pos"], buf["move"], buf["summary"], buf["scratch"], buf["scratch"].numel(), kind, out, stop_dev,
                             stream=self._stream())

    def _check_targets(self, targets: Targets) -> int:
        """E of targets this Replay can scan."""
        if targets.kind not in KINDS:
            raise ValueError(f"unknown kind {targets.kind!r}")
        E = int(targets.E)
        for t in (targets.a, targets.b, targets.valid):
            if t is not None and (t.shape[0] != self.n_cycles or t.shape[1] != E or not t.is_contiguous()):
                raise ValueError("targets must be contiguous [n_cycles, E, ...] tensors of this Replay")
        return E

    def objective(self, targets: Targets, kind: str = "trimmed_bbox_error"):
        """The closed-loop error of every experiment of `targets` as a device float64 [E] tensor, enqueued on the current torch stream (no synchronisation):
        "trimmed_bbox_error" = Summary.trimmed_mean_bbox_error, "bbox_error" = mean_bbox_error, "mse_error" = mean_mse_error, "non_perfect" = non_perfect
        of `run(targets)`, bit for bit (the same sums, the same float64 division; 0 / 0 is NaN).  With attached frames also "trimmed_precise_error" =
        PreciseSummary.trimmed_mean_precise_error, "precise_error" = mean_precise_error, "precise_non_perfect" = non_perfect of `run(targets, precise=True)`."""
        import torch

        E, k = self._check_targets(targets), self._objective_kind(kind)
        with torch.cuda.device(self._dev):
            out = torch.empty((E,), dtype=torch.float64, device=self._dev)
            self._enqueue_objective(targets, k, self._all_objective_buffers(E, kind in PRECISE_OBJECTIVES), out)
        return out

    def _all_objective_buffers(self, E: int, precise: bool) -> dict:
        buf = self._objective_buffers(E)
        if precise:
            buf["precise"] = self._precise_buffers(E)
        return buf

    def optimize_polyfit(self, degree: int, sample_times, objective: str = "trimmed_bbox_error", pop_size: int = 100, c1: float = 2.05, c2: float = 2.05,
                         max_epoch: int = 300, max_early_stop: int = 100, seed: int = 0, lb: float = 0.0, ub: float = 1.0, start=None,
                         _trace: Optional[list] = None) -> SwarmResult:
        """Particle-swarm search for the Polyfit weights of lowest CLOSED-LOOP error of this experiment: WeightEvaluator.optimize's search
        (polyfit_opt.swarm_search; see that docstring for the rule) with `objective` (see `objective`) of the replayed population in the place of the
        open-loop MAE.  Per epoch: targets of the positions, objective, step; every epoch is enqueued at once and the host waits once.

        `start` [K, N] (K < pop_size) replaces the random start of particles 1 .. K; particle 0 stays at `ub`.  With the open-loop winner in `start` the
        result is never worse than it (nor than uniform weights).  In the returned SwarmResult `mae` holds the objective value of `weights` and `history`
        the best value after every epoch; `run(polyfit([to_config(degree, result.weights)]))` reproduces `mae` bit for bit.

        The objective is piecewise constant in the weights (a move is an integer number of pixels), so many particles tie and small steps change nothing.
        With `lb = 0` a particle can zero so many weights that fits become rank deficient, where the device's fit of absolute centres differs from the
        reference's (Limits); a positive `lb` avoids that."""
        import torch

        degree, st = _check_degree(degree), self._sample_times(sample_times)
        kind = self._objective_kind(objective)
        N, (P, _) = len(st), check_swarm_args(pop_size, max_epoch, max_early_stop, lb, ub)
        if start is not None:
            start = np.asarray(start, dtype=np.float64)
            if start.ndim != 2 or start.shape[1] != N or start.shape[0] > P - 1:
                raise ValueError(f"start must have shape [K, {N}] with K <= pop_size - 1, got {start.shape}")
            if not (np.isfinite(start).all() and (start >= lb).all() and (start <= ub).all()):
                raise ValueError(f"start must lie inside [{lb}, {ub}]")
        tg, fit_scratch, classes = self._population_buffers(P, st, degree, torch.zeros)
        buf = self._all_objective_buffers(P, objective in PRECISE_OBJECTIVES)

        def enqueue_error(pos, value, ctrl):
            self._enqueue_population(pos, degree, st, classes, tg.a, tg.valid, fit_scratch, stop_dev=ctrl)
            self._enqueue_objective(tg, kind, buf, value, stop_dev=ctrl)

        return swarm_search(self._dev, N, enqueue_error, degree, pop_size, c1, c2, max_epoch, max_early_stop, seed, lb, ub, start=start, _trace=_trace)

    def to_config(self, degree: int, weights, sample_times=None) -> PolyfitConfig:
        """The PolyfitConfig of a search result.  `sample_times` default to those of the last `optimize_polyfit` / `polyfit_population` call."""
        st = self._last_times if sample_times is None else self._sample_times(sample_times)
        if st is None:
            raise ValueError("no sample times yet: pass sample_times, or call optimize_polyfit / polyfit_population first")
        return polyfit_config(degree, st, weights)

    def analyze(self, targets: Targets, spec: Analysis, _max_lds_rows: int = 0) -> AnalysisResult:
        """DataAnalyzer's statistics of every experiment of `targets` as an AnalysisResult of DEVICE tensors, enqueued on the current torch stream (no
        synchronisation; `objective` is the pattern): the scan and wtk_replay_analyze, the arrays `run(targets, analysis=spec).analysis` holds, bit for
        bit.  The precise_error column is `run`'s (it needs wtk_replay_precise's per-pair errors)."""
        import torch

        E = self._check_targets(targets)
        if "precise_error" in spec.columns:
            raise ValueError("the precise_error column is computed by run(precise=True, analysis=...)")
        with torch.cuda.device(self._dev):
            stream, buf = self._stream(), self._objective_buffers(E)
            hip.replay_scan(self._cfg, KINDS[targets.kind], E, self.n_cycles, self.track, self.n_track, targets.a, targets.b, targets.valid, self._share,
                            buf["pos"], buf["move"], stream=stream)
            return _enqueue_analysis(self.geometry, self.timing_config, spec, E, self.track, self.n_track, self._share, buf["pos"], buf["move"], None, stream,
                                     _max_lds_rows)

    # ------------------------------------------------------------------ the loop
    def run(self, targets: Targets, rows: Sequence[int] = (0,), per_row_errors: bool = False, precise: bool = False,
            _max_crop_px: int = 0, analysis: Optional[Analysis] = None, _max_lds_rows: int = 0) -> ReplayResult:
        """Replay the E experiments of `targets`.  `rows`: the experiments whose full log rows are kept (16 doubles per row each).  `precise`: also the
        precise error of every experiment on the attached frames (`precise_summary`; with `per_row_errors` `precise_error` and `precise_counts`).
        `analysis`: also DataAnalyzer's statistics of every experiment (`res.analysis`; the precise_error column needs `precise`).
        `_max_crop_px` (tests): the table limit of wtk_replay_precise, 0 = the default; results do not depend on it.  `_max_lds_rows` (tests): the
        longest segment wtk_replay_analyze sorts in LDS, 0 = the default; results do not depend on it."""
        import torch

        if precise:
            self._need_frames()
        if analysis is not None and "precise_error" in analysis.columns and not precise:
            raise ValueError("the precise_error column needs run(precise=True) on attached frames")
        E, C, R = self._check_targets(targets), self.n_cycles, self.n_rows
        row_ids = sorted({int(e) for e in rows})
        if any(e < 0 or e >= E for e in row_ids):
            raise IndexError(f"rows names an experiment outside [0, {E})")
        dev, f64 = self._dev, torch.float64
        with torch.cuda.device(dev):
            stream, buf = self._stream(), self._objective_buffers(E)
            pos, move, summary, scratch = buf["pos"], buf["move"], buf["summary"], buf["scratch"]
            hip.replay_scan(self._cfg, KINDS[targets.kind], E, C, self.track, self.n_track, targets.a, targets.b, targets.valid, self._share, pos, move,
                            stream=stream)
            slot_host = np.full((E,), -1, dtype=np.int32)
            slot_host[row_ids] = np.arange(len(row_ids), dtype=np.int32)
            slots = torch.from_numpy(slot_host).to(dev) if row_ids else None
            row_data = torch.empty((len(row_ids), R, hip.REPLAY_ROW_DOUBLES), dtype=f64, device=dev) if row_ids else None
            bbox = torch.empty((E, R), dtype=f64, device=dev) if per_row_errors else None
            mse = torch.empty((E, R), dtype=f64, device=dev) if per_row_errors else None
            hip.replay_rows(self._cfg, E, C, self.track, self.n_track, self._share, pos, move, slots, len(row_ids), row_data, bbox, mse, summary, scratch,
                            scratch.numel(), stream=stream)
            if precise:
                fr, pb = self._frames, self._precise_buffers(E)
                perr = torch.empty((E, R), dtype=f64, device=dev) if per_row_errors else None
                pcounts = torch.empty((E, R, 2), dtype=torch.int32, device=dev) if per_row_errors else None
                hip.replay_precise(self._cfg, E, C, self.track, self.n_track, self._share, pos, move, fr, int(fr.shape[0]), int(fr.shape[1]), int(fr.shape[2]),
                                   self._background, self._diff_thresh, int(_max_crop_px), perr, pcounts, pb["summary"], pb["scratch"], pb["scratch"].numel(),
                                   stream=stream)
            ana = None
            if analysis is not None:  # (the per-pair errors [R, E] are the first R E doubles of wtk_replay_precise's scratch)
                ana = _enqueue_analysis(self.geometry, self.timing_config, analysis, E, self.track, self.n_track, self._share, pos, move,
                                        pb["scratch"] if precise else None, stream, _max_lds_rows)
            torch.cuda.current_stream(dev).synchronize()  # the one host synchronisation
            res = _result_of(self.geometry, pos, move, summary, row_ids, row_data, bbox, mse)
            if ana is not None:
                res.analysis = _analysis_to_host(ana)
            if precise:
                res.precise_summary = _precise_summary_of(pb["summary"].cpu().numpy())
                if per_row_errors:
                    res.precise_error, res.precise_counts = perr.cpu().numpy(), pcounts.cpu().numpy()
            return res


DEFAULT_REACH = 64  # frames from a cycle's start: beyond the notebook's Polyfit sample times and the shipped ResMLPs' input frames


@dataclass
class ReplaySetResult:
    """`ReplaySet.run`: `summary` the pooled Summary ([E] arrays: the sums and counts of all tracks' rows), `track_summary[t]` track t's Summary,
    `moves[t]` / `positions[t]` int32 [E, C_t, 2] of track t.  With `precise`: `precise_summary` the pooled PreciseSummary, `track_precise_summary[t]`
    track t's; with `per_row_errors` also `precise_error[t]` float64 [E, R_t] and `precise_counts[t]` int32 [E, R_t, 2]."""

    summary: Summary
    track_summary: list
    moves: list
    positions: list
    precise_summary: Optional[PreciseSummary] = None
    track_precise_summary: Optional[list] = None
    precise_error: Optional[list] = None
    precise_counts: Optional[list] = None
    analysis: Optional[SetAnalysisResult] = None  # run_analysis: a SetAnalysisResult of numpy arrays


class _SuperTrack(Replay):
    """The super-track of a ReplaySet as a Replay: every targets builder and the swarm of `optimize_polyfit` run on it unchanged, over all cycles of all
    tracks at once; the objective behind them is the set's (wtk_replay_set_objective).  Private to ReplaySet: it has no loop of its own."""

    def __init__(self, owner: "ReplaySet", track, timing_config, experiment_config, device: int):
        super().__init__(track, timing_config, experiment_config, None, device)
        self._set = owner

    def _objective_kind(self, kind: str) -> int:
        return self._set._objective_kind(kind)

    def _all_objective_buffers(self, E: int, precise: bool) -> dict:
        return self._set._objective_buffers(E, precise)

    def _enqueue_objective(self, targets: Targets, kind: int, buf: dict, out, stop_dev=None):
        self._set._enqueue_objective(targets, kind, buf, out, stop_dev=stop_dev)

    def _mlp_bound(self, max_speed: float, pred_frames):
        return self._set._mlp_bounds(max_speed, pred_frames)


class ReplaySet:
    """The closed loop of a population of controller configurations on SEVERAL tracks at once, with an objective pooled over them (DESIGN.md section
    26): what one `Replay` per track and a host loop around them compute, in a number of launches that does not depend on the number of tracks.

        rs = ReplaySet([track0_dev, "bboxes1.csv", track2], timing_config, experiment_configs)
        tg = rs.polyfit_population(weights_dev, 1, offsets)     # also csv(), optimal(), polyfit(cfgs), mlp(model), mlp_population(...)
        rs.objective(tg, "trimmed_bbox_error")                  # device float64 [E], pooled; per_track=True -> [T, E]
        res = rs.run(tg)                                        # res.summary (pooled), res.track_summary[t], res.moves[t], res.positions[t]
        rs.optimize_polyfit(1, offsets, start=[...], seed=0)    # Replay.optimize_polyfit's search over the pooled objective
        trainer.fit(..., closed_loop=rs)

    `tracks`: what `Replay` takes, one per track.  `timing_config` is one TimingConfig for all tracks or a sequence of one per track (DESIGN.md
    section 29; `from_experiments` builds them from the ExperimentConfigs): camera size, microscope size, the MLP's clip bound and the analysis' unit
    factors are then each track's own, while the three frame counts must be equal (one cycle structure: a set that differs in them is refused, naming
    the track).  `timing_configs` is the list, `timing_config` its first entry.  `experiment_configs` is one ExperimentConfig or one per track
    (num_frames, init_position and the default frame shape are each track's own), `frame_shapes` None or one (H, W) / None per track.  On the device
    the tracks lie in one float64 [N, 4] "super-track": track t from row cyc_off[t] L, NaN rows up to the end of its whole-cycle slot, then
    ceil(reach / L) all-NaN guard cycles.  The targets entry points treat a NaN row as a row outside the track, so one call over the super-track gives
    every cycle of every track the bits of the per-track call; `reach` (frames, default max(DEFAULT_REACH, L + I)) bounds how far from a cycle's start
    a sample time or an input frame may lie, and a call that reaches further is refused.  Targets are [n_super_cycles, E, ...]; track t's cycles are the
    slice from cyc_off[t].

    The pooled objective is sum of the tracks' sums / sum of their counts: the mean over the rows of all logs (the reference's Plotter concatenates
    them); the trimmed rows drop the first and the last logged cycle of EVERY track.  A (track, experiment) pair has the bits of `Replay` on that track
    alone.  After `attach_frames` the precise error works the same way: `rs.objective(tg, "trimmed_precise_error")`,
    `rs.run(tg, precise=True)`, the search and the trainer's closed loop with a precise objective.  The analysis of the set, per log and over the
    concatenation of all logs, is `rs.analyze(tg, spec)` / `rs.run_analysis(tg, spec)`.  Logs stay with `rs.replay(t)`."""

    def __init__(self, tracks, timing_config, experiment_configs, frame_shapes=None, reach: Optional[int] = None, device: int = 0):
        if hip.device_count() < 1:
            raise hip.WtkError("ReplaySet needs a GPU: no HIP device visible (there is no CPU fallback)")
        import dataclasses

        import torch

        tracks = list(tracks)
        if not tracks:
            raise ValueError("at least one track is needed")
        T = len(tracks)
        ecs = [experiment_configs] * T if isinstance(experiment_configs, ExperimentConfig) else list(experiment_configs)
        shapes = [None] * T if frame_shapes is None else list(frame_shapes)
        if len(ecs) != T or len(shapes) != T:
            raise ValueError(f"{T} tracks: experiment_configs must be one config or {T}, frame_shapes None or {T}")
        # one TimingConfig for all tracks, or one per track: then every kernel reads the track's sizes from a geometry table
        self._per_track = not isinstance(timing_config, TimingConfig)
        tcs = check_timing_configs(timing_config, T) if self._per_track else [timing_config] * T
        self.timing_configs, self.timing_config, self.experiment_configs, self.T = tcs, tcs[0], ecs, T
        self._dev = torch.device("cuda", device)
        self._replays = []
        for t, (tr, tc, ec, fs) in enumerate(zip(tracks, tcs, ecs, shapes)):
            try:
                self._replays.append(Replay(tr, tc, ec, fs, device))
            except ValueError as err:
                if not self._per_track:
                    raise
                raise ValueError(f"track {t}: {err}") from None
        self._geom_tables = {}  # unit -> hip.ReplaySetGeometry (per-track configs only)
        g0 = self._replays[0].geometry
        self.L, self.I, self.M, self.P = L, I, _, P = g0.L, g0.I, g0.M, g0.P
        self.n_cycles, self.n_log, self.n_rows = ([getattr(rp, k) for rp in self._replays] for k in ("n_cycles", "n_log", "n_rows"))
        self.frame_shapes = [rp.frame_shape for rp in self._replays]
        self.reach = max(DEFAULT_REACH, L + I) if reach is None else int(reach)
        if self.reach < 1:
            raise ValueError("reach must be at least 1 frame")
        self.guard_cycles = guard = -(-self.reach // L)
        rows, off = [], 0
        for rp in self._replays:
            rows.append(dict(cyc_off=off, n_track=rp.n_track, num_frames=int(rp.experiment_config.num_frames), n_cycles=rp.n_cycles, n_log=rp.n_log,
                             frame_wh=(rp.frame_shape[1], rp.frame_shape[0]), init_position=rp.experiment_config.init_position))
            off += max(rp.n_cycles, -(-rp.n_track // L)) + guard
        self.cyc_off, self.n_super_cycles = [r["cyc_off"] for r in rows], off
        with torch.cuda.device(self._dev):
            track = torch.full((off * L, 4), float("nan"), dtype=torch.float64, device=self._dev)
            for rp, o in zip(self._replays, self.cyc_off):
                track[o * L:o * L + rp.n_track] = rp.track
            self._table = hip.ReplaySetTable(rows, L, guard, off * L, device=self._dev)
        # the super-track as a Replay whose scanned cycles are all n_super_cycles: the targets builders and the swarm run on it
        ec = dataclasses.replace(ecs[0], num_frames=(off - 1) * L + I + 1)
        self._super = _SuperTrack(self, track, tcs[0], ec, device)
        self._frames_table = None

    @classmethod
    def from_experiments(cls, tracks, experiment_configs, imaging_time_ms: float, pred_time_ms: float, moving_time_ms: float, camera_size_mm, micro_size_mm,
                         **kwargs) -> "ReplaySet":
        """The set of T recordings with one TimingConfig per recording, each built from that recording's ExperimentConfig and ONE set of times (ms) and
        view sizes (mm), as the reference's notebooks build a TimingConfig per experiment: recordings at 88, 90 and 92 px/mm get cameras of 352, 360
        and 368 px for the same 4 mm.  `kwargs`: frame_shapes, reach, device."""
        ecs = list(experiment_configs)
        tcs = [TimingConfig(ec, imaging_time_ms, pred_time_ms, moving_time_ms, camera_size_mm, micro_size_mm) for ec in ecs]
        return cls(tracks, tcs, ecs, **kwargs)

    def _geom(self, unit: str = "frame"):
        """The geometry table the set's entry points take: None for a set built from one TimingConfig (every track the config's sizes: the entry
        points without a table), else every track's camera and microscope with its change_unit factors of `unit` (built once per unit)."""
        if not self._per_track:
            return None
        if unit not in self._geom_tables:
            import torch

            factors = Analysis(unit=unit).factors(self.timing_configs)
            entries = [dict(cam=rp.geometry.cam, mic=rp.geometry.mic, factors=f) for rp, f in zip(self._replays, factors)]
            with torch.cuda.device(self._dev):
                self._geom_tables[unit] = hip.ReplaySetGeometry(entries, device=self._dev)
        return self._geom_tables[unit]

    def _mlp_bounds(self, max_speed: float, pred_frames):
        """`mlp_clip_bound` of the super-track's cycles: one float for a set built from one TimingConfig, else a device float32 [n_super_cycles] tensor,
        track t's bound on the cycles of its slot and guard."""
        if not self._per_track:
            return mlp_clip_bound(self.timing_config, max_speed, pred_frames)
        import torch

        ends = self.cyc_off[1:] + [self.n_super_cycles]
        host = np.concatenate([np.full(e - o, mlp_clip_bound(tc, max_speed, pred_frames), dtype=np.float32)
                               for o, e, tc in zip(self.cyc_off, ends, self.timing_configs)])
        return torch.from_numpy(host).to(self._dev)

    def replay(self, t: int) -> Replay:
        """The plain `Replay` of track t: logs and per-row log output stay there (and the analysis and the precise error of one track alone)."""
        return self._replays[t]

    def attach_frames(self, frames, backgrounds, diff_thresh=20) -> None:
        """Every track's frames, for the precise error of the set (`run(precise=True)`, the precise objectives): `frames` and `backgrounds` are
        sequences of T entries, `diff_thresh` one threshold or T.  Entry t is what `Replay.attach_frames` of `rs.replay(t)` takes and is attached there
        too (its checks; that Replay then computes the same track alone); a refusal names the track.  All frames lie on the set's device; the set
        keeps the tensors alive."""
        frames, backgrounds = list(frames), list(backgrounds)
        thr = list(diff_thresh) if isinstance(diff_thresh, (list, tuple, np.ndarray)) else [diff_thresh] * self.T
        if len(frames) != self.T or len(backgrounds) != self.T or len(thr) != self.T:
            raise ValueError(f"{self.T} tracks: frames and backgrounds must hold {self.T} entries each, diff_thresh one value or {self.T}")
        for t, fr in enumerate(frames):  # (Replay.attach_frames takes frames of any device: the set's kernels read all tracks in one launch)
            if not hasattr(fr, "device") or fr.device != self._dev:
                raise ValueError(f"track {t}: the frames must be a tensor on the set's device {self._dev}, got {getattr(fr, 'device', type(fr).__name__)}")
            if not math.isfinite(float(thr[t])):
                raise ValueError(f"track {t}: diff_thresh must be finite")
        self._frames_table = None  # (its pointers are the tensors the per-track Replays hold: a refusal half way leaves no table behind)
        for t, (rp, fr, bg) in enumerate(zip(self._replays, frames, backgrounds)):
            try:
                rp.attach_frames(fr, bg, thr[t])
            except ValueError as err:
                raise ValueError(f"track {t}: {err}") from None
        entries = [dict(frames=rp._frames.data_ptr(), bg=rp._background.data_ptr(), n_frames=int(rp._frames.shape[0]), H=int(rp._frames.shape[1]),
                        W=int(rp._frames.shape[2]), diff_thresh=rp._diff_thresh) for rp in self._replays]
        import torch

        self._frame_tensors = [(rp._frames, rp._background) for rp in self._replays]  # the table's pointers stay valid whatever the Replays do later
        with torch.cuda.device(self._dev):
            self._frames_table = hip.ReplaySetFrames(self._table, entries, device=self._dev)

    def _need_frames(self) -> None:
        if self._frames_table is None:
            raise ValueError("the precise error of a set needs the frames of every track: call rs.attach_frames(frames, backgrounds) first "
                             "(or use rs.replay(t), which takes attach_frames, for one track)")

    # ------------------------------------------------------------------ targets: the super-track's, after the reach is checked
    def _check_reach(self, what: str, offsets) -> None:
        far = max(abs(int(o)) for o in offsets)
        if far > self.reach:
            raise ValueError(f"{what} lie up to {far} frames from a cycle's start, beyond this ReplaySet's reach = {self.reach} (the guard between two "
                             "tracks): build the set with a larger reach")

    def csv(self) -> Targets:
        return Targets("csv", 1)

    def optimal(self) -> Targets:
        """`Replay.optimal` of every track in one call (the median reads the next imaging phase: within any guard)."""
        return self._super.optimal()

    def polyfit(self, configs: Sequence[PolyfitConfig]) -> Targets:
        """`Replay.polyfit(configs)` of every track: one call per config, whatever T is."""
        configs = list(configs)
        for cfg in configs:
            self._check_reach("sample_times", cfg.sample_times)
        return self._super.polyfit(configs)

    def polyfit_population(self, weights, degree: int, sample_times) -> Targets:
        """`Replay.polyfit_population` of every track: two launches whatever P and T are."""
        self._check_reach("sample_times", check_times(sample_times, "sample_times"))
        return self._super.polyfit_population(weights, degree, sample_times)

    def _check_input_frames(self, input_frames) -> None:
        self._check_reach("input_frames", [self.I - self.P + int(f) for f in input_frames])

    def mlp(self, model, max_speed: float = 0.9) -> Targets:
        """`Replay.mlp(model)` of every track in one call."""
        folded = model if isinstance(model, FoldedResMLP) else from_torch_module(model)
        self._check_input_frames(folded.input_frames)
        return self._super.mlp(folded, max_speed)

    def mlp_population(self, models, max_speed: float = 0.9, which="current") -> Targets:
        """`Replay.mlp_population` of every track: one launch whatever E and T are."""
        from .training import HipMLPTrainer

        if not isinstance(models, HipMLPTrainer):
            models = [m if isinstance(m, FoldedResMLP) else from_torch_module(m) for m in models]
        frames = models.input_frames if isinstance(models, HipMLPTrainer) else (models[0].input_frames if models else None)
        if frames is not None:
            self._check_input_frames(frames)
        return self._super.mlp_population(models, max_speed, which)

    # ------------------------------------------------------------------ objective
    def _objective_kind(self, kind: str) -> int:
        """The WTK_REPLAY_OBJ_* value of a name of OBJECTIVES, the WTK_REPLAY_POBJ_* value of a name of PRECISE_OBJECTIVES."""
        if kind not in OBJECTIVES and kind not in PRECISE_OBJECTIVES:
            raise ValueError(f"unknown objective {kind!r}: one of {sorted(OBJECTIVES)}, or with attach_frames one of {sorted(PRECISE_OBJECTIVES)}")
        if kind in PRECISE_OBJECTIVES:
            self._need_frames()
        if kind in ("trimmed_bbox_error", "trimmed_precise_error") and min(self.n_log) < 3:
            t = int(np.argmin(self.n_log))
            raise ValueError(f"the trimmed objective drops the first and the last logged cycle of every track: track {t} logs {self.n_log[t]}, at least 3 are needed")
        return PRECISE_OBJECTIVES[kind] if kind in PRECISE_OBJECTIVES else OBJECTIVES[kind]

    def _objective_buffers(self, E: int, precise: bool = False) -> dict:
        """The scan's arrays and the summaries and scratch of the rows reduction, or (`precise`) of the precise error: _enqueue_objective tells by
        the "precise" entry which objective the buffers are for."""
        import torch

        dev, C, n = self._dev, self.n_super_cycles, hip.REPLAY_PRECISE_SUMMARY_DOUBLES if precise else hip.REPLAY_SUMMARY_DOUBLES
        n_scratch = hip.replay_set_precise_scratch_doubles(self._table, E) if precise else hip.replay_set_scratch_doubles(self._table, E)
        buf = dict(pos=torch.empty((C, E, 2), dtype=torch.int32, device=dev), move=torch.empty((C, E, 2), dtype=torch.int32, device=dev),
                   track_summary=torch.empty((self.T, E, n), dtype=torch.float64, device=dev), summary=torch.empty((E, n), dtype=torch.float64, device=dev),
                   scratch=torch.empty((max(1, n_scratch),), dtype=torch.float64, device=dev))
        if precise:
            buf["precise"] = True
        return buf

    def _enqueue_objective(self, targets: Targets, kind: int, buf: dict, out, track_out=None, stop_dev=None):
        """`kind`: _objective_kind's value; a precise objective where `buf` holds the precise buffers (_objective_buffers(E, precise=True))."""
        sp = self._super
        if "precise" in buf:
            hip.replay_set_precise_objective(sp._cfg, self._table, self._frames_table, KINDS[targets.kind], int(targets.E), sp.track, targets.a, targets.b,
                                             targets.valid, sp._share, buf["pos"], buf["move"], 0, buf["track_summary"], buf["summary"], buf["scratch"],
                                             buf["scratch"].numel(), kind, out, track_out, stop_dev, stream=sp._stream(), geom=self._geom())
            return
        hip.replay_set_objective(sp._cfg, self._table, KINDS[targets.kind], int(targets.E), sp.track, targets.a, targets.b, targets.valid, sp._share, buf["pos"],
                                 buf["move"], buf["track_summary"], buf["summary"], buf["scratch"], buf["scratch"].numel(), kind, out, track_out, stop_dev,
                                 stream=sp._stream(), geom=self._geom())

    def _check_targets(self, targets: Targets) -> int:
        return self._super._check_targets(targets)

    def objective(self, targets: Targets, kind: str = "trimmed_bbox_error", per_track: bool = False):
        """The closed-loop error of every experiment of `targets`, pooled over the tracks, as a device float64 [E] tensor, enqueued on the current torch
        stream (no synchronisation): the division of `run(targets).summary`'s slots, bit for bit.  `per_track`: instead the [T, E] tensor of each
        track's own error, `rs.replay(t).objective`'s bits.  After `attach_frames` also the names of PRECISE_OBJECTIVES: the division of
        `run(targets, precise=True).precise_summary`'s slots, pooled over the rows of all tracks' logs."""
        import torch

        E, k = self._check_targets(targets), self._objective_kind(kind)
        with torch.cuda.device(self._dev):
            out = torch.empty((E,), dtype=torch.float64, device=self._dev)
            each = torch.empty((self.T, E), dtype=torch.float64, device=self._dev) if per_track else None
            self._enqueue_objective(targets, k, self._objective_buffers(E, kind in PRECISE_OBJECTIVES), out, each)
        return each if per_track else out

    def optimize_polyfit(self, degree: int, sample_times, objective: str = "trimmed_bbox_error", **swarm) -> SwarmResult:
        """`Replay.optimize_polyfit` (its arguments, its search) for the weights of lowest POOLED closed-loop error over the set's tracks."""
        self._check_reach("sample_times", check_times(sample_times, "sample_times"))
        return self._super.optimize_polyfit(degree, sample_times, objective, **swarm)

    def to_config(self, degree: int, weights, sample_times=None) -> PolyfitConfig:
        return self._super.to_config(degree, weights, sample_times)

    # ------------------------------------------------------------------ the loop
    def run(self, targets: Targets, precise: bool = False, analysis: Optional[Analysis] = None, per_row_errors: bool = False,
            _max_crop_px: int = 0) -> ReplaySetResult:
        """Replay the E experiments of `targets` on every track: scan, rows reduction, one synchronisation.  `precise` (after `attach_frames`): also
        the precise error of every experiment on every track's frames (`precise_summary` pooled, `track_precise_summary[t]`; with `per_row_errors`
        `precise_error[t]` and `precise_counts[t]`).  Logs belong to one track: they are `rs.replay(t).run`'s; the analysis of the set is
        `run_analysis(targets, spec)` (this method's `analysis` argument stays refused).
        `_max_crop_px` (tests): the table limit of wtk_replay_set_precise, 0 = the default; results do not depend on it."""
        if analysis is not None:
            raise ValueError("the precise error and the analysis are per track: use rs.replay(t).run(..., precise=True / analysis=spec)")
        return self._run(targets, precise, per_row_errors, _max_crop_px, None, 0)

    def run_analysis(self, targets: Targets, spec: Analysis, precise: bool = False, per_row_errors: bool = False, _max_lds_rows: int = 0) -> ReplaySetResult:
        """`run(targets, precise, per_row_errors)` and, as `res.analysis`, the SetAnalysisResult of `analyze(targets, spec, precise)` as numpy arrays:
        one scan serves both, and the host synchronises once.  The precise_error column needs `precise` (after `attach_frames`)."""
        return self._run(targets, precise, per_row_errors, 0, spec, _max_lds_rows)

    def _check_analysis(self, spec: Analysis, precise: bool) -> None:
        if "precise_error" in spec.columns and not precise:
            raise ValueError("the precise_error column needs precise=True on attached frames (rs.attach_frames)")
        if precise:
            self._need_frames()

    def _enqueue_precise(self, E: int, buf: dict, per_row: bool, counts: bool, max_crop_px: int, stream: int) -> dict:
        """wtk_replay_set_precise behind a set scan: its summaries, and where asked for the per-row errors [E, sum R] and counts."""
        import torch

        n, rows, dev, sp = hip.REPLAY_PRECISE_SUMMARY_DOUBLES, self._frames_table.n_rows, self._dev, self._super
        out = dict(track=torch.empty((self.T, E, n), dtype=torch.float64, device=dev), pooled=torch.empty((E, n), dtype=torch.float64, device=dev),
                   scratch=torch.empty((max(1, hip.replay_set_precise_scratch_doubles(self._table, E)),), dtype=torch.float64, device=dev),
                   err=torch.empty((E, rows), dtype=torch.float64, device=dev) if per_row else None,
                   counts=torch.empty((E, rows, 2), dtype=torch.int32, device=dev) if counts else None)
        hip.replay_set_precise(sp._cfg, self._table, self._frames_table, E, sp.track, sp._share, buf["pos"], buf["move"], int(max_crop_px), out["err"],
                               out["counts"], out["track"], out["pooled"], out["scratch"], out["scratch"].numel(), stream=stream, geom=self._geom())
        return out

    def _enqueue_analysis(self, spec: Analysis, E: int, pos, move, precise_rows, stream: int, max_lds_rows: int) -> SetAnalysisResult:
        """wtk_replay_set_analyze on a set scan's pos / move: a SetAnalysisResult of device tensors.  `precise_rows`: the per-row precise errors
        [E, sum R] or None.  The per-track cycle aggregates and masks are slices of the packed arrays, which are the pooled result's."""
        import torch

        dev, T, L = self._dev, self.T, self.L
        cols, q = spec.column_ids(), [float(v) for v in spec.percentiles]
        n, Q, f64, i64 = len(cols), len(q), torch.float64, torch.int64
        rows, logs = int(sum(self.n_rows)), int(sum(self.n_log))
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)  # noqa: E731
        mask = new((E, rows), torch.uint8) if spec.anomaly_mask else None
        per = [new((T, E, n, 5 + Q), f64), new((E, logs, n), f64), new((E, logs, n), f64), new((T, E, L, n, Q), f64), new((T, E, L, n), torch.int32),
               new((T, E, 7), i64), mask, new((T, E, 4), i64)]
        pooled = [new((E, n, 5 + Q), f64), new((E, L, n, Q), f64), new((E, L, n), torch.int32), new((E, 7), i64), new((E, 4), i64)]
        scratch = new((max(1, hip.replay_set_analysis_scratch_doubles(self._table, E, n, Q)),), f64)
        sp = self._super
        hip.replay_set_analyze(sp._cfg, spec.config(self.timing_config), self._table, E, sp.track, sp._share, pos, move, precise_rows, cols, q,
                               int(max_lds_rows), per, pooled, scratch, scratch.numel(), stream=stream, geom=self._geom(spec.unit))
        row0, log0 = np.concatenate([[0], np.cumsum(self.n_rows)]), np.concatenate([[0], np.cumsum(self.n_log)])
        names = list(spec.columns)
        track = [AnalysisResult(names, q, self.n_rows[t], per[0][t], per[1][:, log0[t]:log0[t + 1]], per[2][:, log0[t]:log0[t + 1]], per[3][t], per[4][t],
                                per[5][t], per[7][t], None if mask is None else mask[:, row0[t]:row0[t + 1]]) for t in range(T)]
        return SetAnalysisResult(AnalysisResult(names, q, rows, pooled[0], per[1], per[2], pooled[1], pooled[2], pooled[3], pooled[4], mask), track)

    def analyze(self, targets: Targets, spec: Analysis, precise: bool = False, _max_lds_rows: int = 0) -> SetAnalysisResult:
        """DataAnalyzer's statistics of every experiment of `targets` on every track and over the concatenation of its T cleaned logs, as a
        SetAnalysisResult of DEVICE tensors, enqueued on the current torch stream (no synchronisation; `Replay.analyze` is the pattern): the set's scan,
        with `precise` wtk_replay_set_precise, and wtk_replay_set_analyze, in a number of launches that does not depend on T.  `track[t]` has
        `rs.replay(t).analyze(targets of t, spec)`'s bits; a pooled percentile is the percentile of all kept rows of all logs, which no combination of
        per-track results gives.  `precise` (after `attach_frames`): the precise_error column, from the set's per-row errors.  `_max_lds_rows` (tests):
        the longest segment wtk_replay_set_analyze sorts in LDS, 0 = the default; results do not depend on it."""
        import torch

        E, sp = self._check_targets(targets), self._super
        self._check_analysis(spec, precise)
        with torch.cuda.device(self._dev):
            stream, buf = sp._stream(), self._objective_buffers(E)
            hip.replay_set_scan(sp._cfg, self._table, KINDS[targets.kind], E, sp.track, targets.a, targets.b, targets.valid, sp._share, buf["pos"], buf["move"],
                                stream=stream, geom=self._geom())
            pr = self._enqueue_precise(E, buf, True, False, 0, stream) if precise else None
            return self._enqueue_analysis(spec, E, buf["pos"], buf["move"], pr["err"] if precise else None, stream, _max_lds_rows)

    def _run(self, targets: Targets, precise: bool, per_row_errors: bool, _max_crop_px: int, spec: Optional[Analysis], _max_lds_rows: int) -> ReplaySetResult:
        import torch

        if spec is not None:
            self._check_analysis(spec, precise)
        if precise:
            self._need_frames()
        E, sp = self._check_targets(targets), self._super
        with torch.cuda.device(self._dev):
            stream, buf = sp._stream(), self._objective_buffers(E)
            hip.replay_set_scan(sp._cfg, self._table, KINDS[targets.kind], E, sp.track, targets.a, targets.b, targets.valid, sp._share, buf["pos"], buf["move"],
                                stream=stream, geom=self._geom())
            hip.replay_set_rows(sp._cfg, self._table, E, sp.track, sp._share, buf["pos"], buf["move"], buf["track_summary"], buf["summary"], buf["scratch"],
                                buf["scratch"].numel(), stream=stream, geom=self._geom())
            if precise:
                pr = self._enqueue_precise(E, buf, per_row_errors or (spec is not None and "precise_error" in spec.columns), per_row_errors, _max_crop_px, stream)
                ptrack, ppooled, perr, pcounts = pr["track"], pr["pooled"], pr["err"], pr["counts"]
            ana = None
            if spec is not None:
                ana = self._enqueue_analysis(spec, E, buf["pos"], buf["move"], perr if precise else None, stream, _max_lds_rows)
            torch.cuda.current_stream(self._dev).synchronize()  # the one host synchronisation
            per = buf["track_summary"].cpu().numpy()
            cut = lambda x, t: x[self.cyc_off[t]:self.cyc_off[t] + self.n_cycles[t]].permute(1, 0, 2).contiguous().cpu().numpy()  # noqa: E731
            res = ReplaySetResult(_summary_of(buf["summary"].cpu().numpy()), [_summary_of(per[t]) for t in range(self.T)],
                                  [cut(buf["move"], t) for t in range(self.T)], [cut(buf["pos"], t) for t in range(self.T)])
            if precise:
                pper = ptrack.cpu().numpy()
                res.precise_summary, res.track_precise_summary = _precise_summary_of(ppooled.cpu().numpy()), [_precise_summary_of(pper[t]) for t in range(self.T)]
                if per_row_errors:
                    row0 = np.concatenate([[0], np.cumsum(self.n_rows)])
                    err, counts = perr.cpu().numpy(), pcounts.cpu().numpy()
                    res.precise_error = [np.ascontiguousarray(err[:, row0[t]:row0[t + 1]]) for t in range(self.T)]
                    res.precise_counts = [np.ascontiguousarray(counts[:, row0[t]:row0[t + 1]]) for t in range(self.T)]
            if ana is not None:
                res.analysis = SetAnalysisResult(_analysis_to_host(ana.pooled), [_analysis_to_host(a) for a in ana.track])
            return res


def _summary_of(s: np.ndarray) -> Summary:
    return Summary(s[:, 0].copy(), s[:, 1].astype(np.int64), s[:, 2].copy(), s[:, 3].astype(np.int64), s[:, 4].astype(np.int64), s[:, 5].copy())


def _precise_summary_of(s: np.ndarray) -> PreciseSummary:
    return PreciseSummary(s[:, 0].copy(), s[:, 1].astype(np.int64), s[:, 2].copy(), s[:, 3].astype(np.int64), s[:, 4].astype(np.int64), s[:, 5].astype(np.int64))


class YoloReplay:
    """The closed loop of HipYoloController on device-resident frames, without a host wait per cycle: what `Simulator` + `SineMotorController` +
    `TrackLogger(HipYoloController(timing_config, yolo_config, device_frames=device_frames))` produce, bit for bit (same handles, same kernels, same inputs).

    Phase 1, per scanned cycle on one stream: the single-frame detector call on the controller's decision view (`yolo_config.load_model().detector(net_hw, 1)`,
    frame and platform position read from device memory) and wtk_replay_yolo_step, which turns the row into the move and the next cycle's position where the
    next call reads it.  Phase 2: the platform position of every logged frame, the detector over the R logged frames in chunks of `log_batch`, the absolute
    track with TrackLogger's dtype rule, and wtk_replay_rows.  `run` is ordered behind the caller's current stream once and synchronises once, at the end;
    then the handles' range-guard words are checked.

    `log_batch`: None = cycle_frame_num on the handle `detector(net_hw, cycle_frame_num)` returns (the host loop's cycle batch: its bits).  Any other size
    takes a throughput-plan handle of that size owned by this object (large-batch kernels, the sparse box tail); the last chunk may be partial.  Handles on
    different plans agree within the tolerance both meet against the fp32 restatement, not bit for bit.

    The constructor makes one warm-up call per batch size it will use (a latency-plan handle times its launch candidates inside its first eager call at a
    batch size, which waits for the device) and waits for it, so `run` never does.  The model's handles are shared with every controller of the same
    YoloConfig: do not run one of those while a `run` is enqueued.

    Refused: `recheck_margin > 0` (the second look reads the margins on the host), frames that are not a contiguous CUDA uint8 [F, H, W] / [F, H, W, 3] tensor
    or fewer than `num_frames`, and every geometry wtk_replay_rows refuses."""

    def __init__(self, device_frames, timing_config: TimingConfig, experiment_config: ExperimentConfig, yolo_config: YoloConfig, log_batch: Optional[int] = None):
        if hip.device_count() < 1:
            raise hip.WtkError("YoloReplay needs a GPU: no HIP device visible (there is no CPU fallback)")
        import torch

        tc, ec, fr = timing_config, experiment_config, device_frames
        if yolo_config.recheck_margin > 0:
            raise ValueError("YoloReplay does not take recheck_margin > 0: the second look reads the first call's margins on the host, once per call")
        check_device_frames(fr)
        if int(fr.shape[0]) < int(ec.num_frames):
            raise ValueError(f"the frame tensor holds {int(fr.shape[0])} frames, the experiment needs num_frames = {int(ec.num_frames)}")
        self.timing_config, self.experiment_config, self.yolo_config = tc, ec, yolo_config
        self._frames, self._dev = fr, fr.device
        _adopt(self, LoopGeometry.of(tc, ec, fr.shape[1:3]))
        (H, W), cam, R = self.frame_shape, self.geometry.cam, self.n_rows
        if max(cam + (H, W)) > 8192:  # (the YOLO entry points' own limit, not the scan's)
            raise ValueError("camera and frame sides up to 8192 pixels (wtk_replay_yolo_track)")
        self.log_batch = self.L if log_batch is None else int(log_batch)
        if self.log_batch < 1:
            raise ValueError("log_batch must be at least 1")
        self._imgsz, self._conf, self._iou = yolo_config.call_params()
        net_hw = yolo_spec.letterbox_shape(cam[0], cam[1], self._imgsz)  # the view's shape is (rows = w, cols = h)
        model = self._model = yolo_config.load_model()
        # the cycle batch's handle first: where both calls share one handle (plan "latency") and it was too small for L, the model replaces it here
        self.log_detector = model.detector(net_hw, self.L) if self.log_batch == self.L else None
        self.step_detector = model.detector(net_hw, 1)
        self._own = None
        if self.log_detector is None:
            width, depth, maxch = yolo_spec.scale_params(yolo_config.scale)
            self.log_detector = self._own = hip.HipYolo(model.weights, net_hw, self.log_batch, dtype=self.step_detector.dtype, nc=model.nc, width=width, depth=depth,
                                                        max_channels=maxch, device=yolo_config.device_index(), plan="throughput")
        C, dev, i32, f32 = self.n_cycles, self._dev, torch.int32, torch.float32
        # the controller's deque holds the cycle's frames 0 .. I at the decision and it reads entry [-pred_frame_num] (entry 0 when that is 0)
        decision = list(range(self.I + 1))[-self.P]
        x0, y0 = (int(min(max(int(v), 0), m - 1)) for v, m in zip(ec.init_position, (W, H)))
        with torch.cuda.device(dev):
            self._stream = torch.cuda.Stream(device=dev)
            self._share = torch.from_numpy(sine_shares(self.M)).to(dev)
            self._pos0 = torch.tensor([x0, y0], dtype=i32, device=dev)
            self._decision_idx = (torch.arange(C, dtype=i32, device=dev) * self.L + decision).contiguous()
            self._log_idx = torch.arange(max(R, 1), dtype=i32, device=dev)
            self._pos, self._move = torch.zeros((C, 1, 2), dtype=i32, device=dev), torch.zeros((C, 1, 2), dtype=i32, device=dev)
            self._step_rows = torch.zeros((C, 4), dtype=f32, device=dev)  # the single-frame call's row of every cycle
            self._step_conf, self._step_anchor = torch.zeros((C,), dtype=f32, device=dev), torch.zeros((C,), dtype=i32, device=dev)
            self._frame_pos = self._pos0.repeat(max(R, 1), 1).contiguous()
            self._det = torch.zeros((max(R, 1), 4), dtype=f32, device=dev)
            self._det_conf, self._det_anchor = torch.zeros((max(R, 1),), dtype=f32, device=dev), torch.zeros((max(R, 1),), dtype=i32, device=dev)
            self._track = torch.zeros((max(R, 1), 4), dtype=torch.float64, device=dev)
            self._slots = torch.zeros((1,), dtype=i32, device=dev)
            self._rows = torch.empty((1, R, hip.REPLAY_ROW_DOUBLES), dtype=torch.float64, device=dev)
            self._summary = torch.empty((1, hip.REPLAY_SUMMARY_DOUBLES), dtype=torch.float64, device=dev)
            self._scratch = torch.empty((max(1, hip.replay_scratch_doubles(1, R)),), dtype=torch.float64, device=dev)
            # the warm-up calls: every batch size `run` will use, on the frames and at the position the run starts from
            self._pos[0, 0].copy_(self._pos0)
            self._stream.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(self._stream):
                self._step_call(0)
                for n in sorted({min(self.log_batch, R), R % self.log_batch} - {0}):
                    self._log_call(0, n)
            self._finish()

    def close(self):
        """Destroy the log handle this object owns (a `log_batch` other than the cycle length); the model's handles stay with the model."""
        if self._own is not None:
            self._stream.synchronize()
            self._own.close()
            self._own = None

    def _finish(self):
        self._stream.synchronize()  # the one host synchronisation
        for det in {self.step_detector, self.log_detector}:  # (one handle where both calls share it)
            _raise_on_overflow(det)

    def _call(self, det, idx, pos, n: int, rows, conf, anchor):
        fr, (vw, vh) = self._frames, self.geometry.cam
        det.predict_views(fr, fr.shape[0], fr.shape[1], fr.shape[2], fr.shape[3] if fr.dim() == 4 else 1, idx, pos, n, vw, vh, rows, conf, anchor,
                          conf=self._conf, iou=self._iou, max_det=1, stream=self._stream.cuda_stream)

    def _step_call(self, c: int):
        self._call(self.step_detector, self._decision_idx[c:c + 1], self._pos[c], 1, self._step_rows[c], self._step_conf[c:c + 1], self._step_anchor[c:c + 1])

    def _log_call(self, r0: int, n: int):
        r = slice(r0, r0 + n)
        self._call(self.log_detector, self._log_idx[r], self._frame_pos[r], n, self._det[r], self._det_conf[r], self._det_anchor[r])

    def run(self, analysis: Optional[Analysis] = None) -> ReplayResult:
        """Enqueue the whole experiment and wait for it once.  Two runs give the same bits.  `analysis`: also DataAnalyzer's statistics of the log
        (`res.analysis`, E = 1; the precise_error column is Replay's)."""
        import torch

        if analysis is not None and "precise_error" in analysis.columns:
            raise ValueError("YoloReplay has no precise_error column")
        C, R, dev = self.n_cycles, self.n_rows, self._dev
        with torch.cuda.device(dev):
            st = self._stream.cuda_stream
            self._stream.wait_stream(torch.cuda.current_stream(dev))  # a caller that refills device_frames in place has its writes on that stream
            with torch.cuda.stream(self._stream):
                self._pos[0, 0].copy_(self._pos0)
                for c in range(C):  # phase 1: nothing in this loop goes to the host
                    self._step_call(c)
                    hip.replay_yolo_step(self._cfg, C, c, self._step_rows[c], self._share, self._pos, self._move, stream=st)
                hip.replay_yolo_positions(self._cfg, C, self._share, self._pos, self._move, self._frame_pos, stream=st)
                for r0 in range(0, R, self.log_batch):
                    self._log_call(r0, min(self.log_batch, R - r0))
                hip.replay_yolo_track(self._cfg, C, self._det, self._frame_pos, self._track, stream=st)
                hip.replay_rows(self._cfg, 1, C, self._track, R, self._share, self._pos, self._move, self._slots, 1, self._rows, None, None, self._summary,
                                self._scratch, self._scratch.numel(), stream=st)
                detections = self._det[:R].clone()
                ana = None
                if analysis is not None:
                    ana = _enqueue_analysis(self.geometry, self.timing_config, analysis, 1, self._track, R, self._share, self._pos, self._move, None, st)
            self._finish()
            res = _result_of(self.geometry, self._pos, self._move, self._summary, [0], self._rows, detections=detections)
            if ana is not None:
                res.analysis = _analysis_to_host(ana)
            return res
