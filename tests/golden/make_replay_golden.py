#!/usr/bin/env python3
"""Generate tests/golden/replay_hard.npz by running the REAL reference (needs its checkout beside this repository's build container; it never
travels to the GPU box).  Nothing of the reference's source is copied: the output is numeric data only (a seeded input track, the reference's
log rows, its per-cycle moves and its ErrorCalculator values).  Placeholder modules stand in for tkinter / cv2 / ultralytics / seaborn
as in make_golden.py and make_eval_golden.py.

The fixture is a 400-frame track on which the closed loop is stressed, replayed by the reference's Simulator + LoggingController around its
CsvController, OptimalController and PolyfitController (four configs) at the timings (100, 40, 50) ms and (200, 40, 50) ms.  The experiment runs at
30 frames/s: the motor then takes M = 2 steps per move, whose half-cosine shares are 0.5 -+ one ulp, so odd moves put `want` on exact .5 ties
(at 60 frames/s, M = 3, no move of a plausible size does).  Before anything is written the script asserts, on the reference's own runs:
  * a sizeable share of the logged rows has a non-zero bbox error (head steps of several pixels per frame);
  * the track has NaN rows, one of them at a cycle's prediction frame (the CSV controller then stands still);
  * the position clamp binds on both axes (the track starts near the frame's corner and drifts out of it);
  * at least one motor step lands on an exact .5 tie.

Stored per run `<kind>_<imaging ms>`: moves [C, 3] (frame, dx, dy), plt / cam / mic corners [R, 2] int32, wrm [R, 4] float64, cycle, phase (0 imaging,
1 moving), bbox_error and mse_error [R] float64.  The log's text is parsed with Python's float (round-trip exact): the fixture pins the values the
reference computed, and ErrorCalculator is applied to exactly those.  `track` is the input as the reference's CsvController read it (pandas)."""
import csv
import json
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_eval_golden  # noqa: E402
import make_golden  # noqa: E402
from make_golden import REF  # noqa: E402

NUM_FRAMES, FPS, PX_PER_MM = 400, 30, 90
ORIG_RESOLUTION, INIT_POSITION = (1600, 1400), (22, 14)
TIMINGS = ((100, 40, 50), (200, 40, 50))
# 6, 31, 251 are prediction frames at L = 5 (c L + 1), 388 at L = 8 (c L + 4): asserted in main().  No two NaN rows are neighbours: a fit that is left with
# fewer finite samples than coefficients gets numpy's minimum-norm solution, which is not translation invariant, and the replay fits absolute centres where
# the reference fits camera-relative ones (limits).  Only the first cycles (history not there yet) are under-determined here, and
# there the sample at t = 0 pins the constant term, which is what the translation changes.
NAN_ROWS = (6, 31, 33, 120, 251, 388)
POLYFIT_CONFIGS = [
    dict(degree=1, sample_times=[-5, -3, -1, 0, 1], weights=None),
    dict(degree=2, sample_times=[-8, -6, -4, -2, 0, 1], weights=[1, 1, 2, 3, 4, 5]),
    dict(degree=2, sample_times=[1, -6, 0, -3], weights=[1, 2, 3, 4]),  # unsorted: the reference sorts the times, not the weights
    dict(degree=3, sample_times=[-10, -8, -6, -4, -2, -1, 0, 1], weights=None),
]


def hard_track(seed: int = 20) -> np.ndarray:
    """Seeded head track [400, 4] xywh: starts near the frame's (0, 0) corner, drifts out of the frame past it (the platform cannot follow: the
    clamp binds on x and y), turns and runs back in with steps of 2 - 5 px per frame and a wandering heading."""
    rng = np.random.default_rng(seed)
    pos = np.array([30.0, 24.0])
    heading = np.deg2rad(215.0)
    out = np.empty((NUM_FRAMES, 4))
    for i in range(NUM_FRAMES):
        if i == 45:
            heading = np.deg2rad(42.0)
        speed = max(0.5, rng.normal(3.5, 1.0))
        heading += rng.normal(0.0, 0.04)
        pos = pos + speed * np.array([np.cos(heading), np.sin(heading)])
        w, h = 13.8 + rng.normal(0, 0.6), 14.6 + rng.normal(0, 0.6)
        out[i] = (pos[0] - w / 2, pos[1] - h / 2, w, h)
    out[list(NAN_ROWS)] = np.nan
    return out


def main():
    make_eval_golden._register_placeholders()  # cv2 (tolerant), tkinter, seaborn
    make_golden._register_placeholders()  # + ultralytics
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import pandas as pd
    from wtracker.eval.error_calculator import ErrorCalculator
    from wtracker.sim.config import ExperimentConfig, TimingConfig
    from wtracker.sim.motor_controllers import SineMotorController
    from wtracker.sim.sim_controllers.csv_controller import CsvController
    from wtracker.sim.sim_controllers.logging_controller import LogConfig, LoggingController
    from wtracker.sim.sim_controllers.optimal_controller import OptimalController
    from wtracker.sim.sim_controllers.polyfit_controller import PolyfitConfig, PolyfitController
    from wtracker.sim.simulator import Simulator

    class RecordingMotor(SineMotorController):
        """The reference's motor, with the value every step rounds written down."""

        def __init__(self, tc):
            super().__init__(tc)
            self.wants = []

        def step(self):
            self.wants.append(tuple(float(v) for v in self.queue[0]))
            return super().step()

    work = tempfile.mkdtemp(prefix="wtk_replay_golden_")
    out = {}
    try:
        init_csv = os.path.join(work, "hard_bboxes.csv")
        with open(init_csv, "w") as f:
            f.write("frame,wrm_x,wrm_y,wrm_w,wrm_h\n")
            for i, r in enumerate(hard_track()):
                f.write(f"{i}," + ",".join("" if not np.isfinite(v) else repr(float(v)) for v in r) + "\n")
        track = pd.read_csv(init_csv, usecols=["wrm_x", "wrm_y", "wrm_w", "wrm_h"]).to_numpy(dtype=float)  # what the reference's controllers see
        out["track"] = track
        geometry = {}
        stats = dict(nonzero=[], tie=0, clamp_x=0, clamp_y=0, still_on_nan=0)
        for timing in TIMINGS:
            ec = ExperimentConfig(name="hard", num_frames=NUM_FRAMES, frames_per_sec=FPS, orig_resolution=ORIG_RESOLUTION, px_per_mm=PX_PER_MM,
                                  init_position=INIT_POSITION)
            tc = TimingConfig(ec, *timing, (4, 4), (0.32, 0.32))
            L, I, P = tc.cycle_frame_num, tc.imaging_frame_num, tc.pred_frame_num
            assert any((r - (I - P)) % L == 0 for r in NAN_ROWS), "no NaN row at a prediction frame"
            kinds = {"csv": lambda: CsvController(tc, init_csv), "optimal": lambda: OptimalController(tc, init_csv)}
            for k, kw in enumerate(POLYFIT_CONFIGS):
                kinds[f"polyfit{k}"] = lambda kw=kw: PolyfitController(tc, PolyfitConfig(**kw), init_csv)
            for name, make in kinds.items():
                ctrl = make()
                rec, orig = [], ctrl.provide_movement_vector

                def wrapped(sim, orig=orig, rec=rec):
                    dx, dy = orig(sim)
                    rec.append([int(sim.frame_number), int(dx), int(dy)])
                    return dx, dy

                ctrl.provide_movement_vector = wrapped
                tmp = tempfile.mkdtemp(prefix="wtk_replay_run_", dir=work)
                lc = LogConfig(root_folder=tmp, save_mic_view=False, save_cam_view=False, save_err_view=False, save_wrm_view=False)
                motor = RecordingMotor(tc)
                Simulator(tc, ec, LoggingController(ctrl, lc), motor_controller=motor).run()
                with open(lc.bbox_file_path, newline="") as f:
                    rows = list(csv.DictReader(f))
                num = lambda cols, dt: np.array([[float(r[c]) for c in cols] for r in rows], dtype=np.float64).astype(dt)  # noqa: E731
                assert [int(r["frame"]) for r in rows] == list(range(len(rows))) and len(rows) == (NUM_FRAMES - 1) // L * L
                cam_wh, mic_wh = num(["cam_w", "cam_h"], np.int32), num(["mic_w", "mic_h"], np.int32)
                assert (cam_wh == tc.camera_size_px).all() and (mic_wh == tc.micro_size_px).all()
                plt, cam, mic = num(["plt_x", "plt_y"], np.int32), num(["cam_x", "cam_y"], np.int32), num(["mic_x", "mic_y"], np.int32)
                wrm = num(["wrm_x", "wrm_y", "wrm_w", "wrm_h"], np.float64)
                mic_boxes = np.concatenate([mic, mic_wh], axis=1).astype(np.int64)
                bbox = ErrorCalculator.calculate_bbox_error(wrm.copy(), mic_boxes.copy())
                mse = ErrorCalculator.calculate_mse_error(wrm.copy(), mic_boxes.copy())
                key = f"{name}_{timing[0]}"
                out[key + "/moves"] = np.array(rec, dtype=np.int32)
                out[key + "/plt"], out[key + "/cam"], out[key + "/mic"], out[key + "/wrm"] = plt, cam, mic, wrm
                out[key + "/cycle"] = np.array([int(r["cycle"]) for r in rows], dtype=np.int32)
                out[key + "/phase"] = np.array([{"imaging": 0, "moving": 1}[r["phase"]] for r in rows], dtype=np.int8)
                out[key + "/bbox_error"], out[key + "/mse_error"] = bbox, mse
                # the properties the fixture exists for, on this run
                stats["nonzero"].append(float((bbox > 1e-7).mean()))
                stats["tie"] += sum(1 for w in motor.wants for v in w if abs(v - np.floor(v)) == 0.5)
                moves = np.array(rec)
                for c in range(len(rows) // L - 1):
                    gone = plt[(c + 1) * L] - plt[c * L]
                    stats["clamp_x"] += int(gone[0] != moves[c, 1])
                    stats["clamp_y"] += int(gone[1] != moves[c, 2])
                if name == "csv":
                    stats["still_on_nan"] += sum(1 for f, dx, dy in rec if f - P in NAN_ROWS and (dx, dy) == (0, 0))
                print(key, "rows", len(rows), "moves", len(rec), "non-zero bbox error %.3f" % stats["nonzero"][-1], "mean %.4f" % bbox.mean())
            geometry[str(timing[0])] = dict(timing=list(timing), L=L, I=I, M=tc.moving_frame_num, P=P, camera_size_px=list(tc.camera_size_px),
                                            micro_size_px=list(tc.micro_size_px))
        print(stats)
        assert min(stats["nonzero"]) > 0.15, "too few rows with a bbox error"
        assert stats["tie"] > 0, "no motor step on an exact .5 tie"
        assert stats["clamp_x"] > 0 and stats["clamp_y"] > 0, "the position clamp does not bind on both axes"
        assert stats["still_on_nan"] >= len(TIMINGS), "no CSV decision on a NaN prediction frame"
        assert np.isnan(track).any(axis=1).sum() == len(NAN_ROWS)
        out["meta"] = np.frombuffer(json.dumps(dict(num_frames=NUM_FRAMES, frames_per_sec=FPS, px_per_mm=PX_PER_MM, orig_resolution=list(ORIG_RESOLUTION),
                                                    init_position=list(INIT_POSITION), camera_size_mm=[4, 4], micro_size_mm=[0.32, 0.32],
                                                    polyfit_configs=POLYFIT_CONFIGS, geometry=geometry)).encode(), dtype=np.uint8)
        path = os.path.join(HERE, "replay_hard.npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < 1 << 20
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
