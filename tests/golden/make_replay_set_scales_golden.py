#!/usr/bin/env python3
"""Generate tests/golden/replay_set_scales.npz by running the REAL reference on three recordings taken at DIFFERENT scales (needs its checkout beside
this repository's build container; it never travels to the GPU box).  Nothing of the reference's source is copied: the output is numeric data only
(seeded input tracks, the reference's log rows, its per-cycle moves, its ErrorCalculator values and its DataAnalyzer tables).  Placeholder modules
stand in for tkinter / cv2 / ultralytics / seaborn as in make_replay_golden.py.

Three ExperimentConfigs at 88, 90 and 92 px/mm and 60 frames/s, as the reference's own experiments exp0..exp4 are recorded; ONE set of times
(100, 40, 50) ms and view sizes camera (4, 4.1) mm, microscope (0.32, 0.33) mm, from which the reference's TimingConfig derives for each recording
its own cameras 352 x 361, 360 x 369, 368 x 377 and microscopes 28 x 29, 29 x 30, 29 x 30 (both parities of size // 2 occur), its own MLP clip bound
max_speed px_per_mm / fps pred_frames[0] and its own change_unit factors.  Every recording has a seeded track of 300 - 400 frames that alternates
between slow stretches (the microscope keeps the worm: bbox error 0) and fast ones (several pixels per frame: the worm leaves the microscope and the
ResMLP's prediction exceeds the clip bound).

Stored per recording t and controller k in (csv, polyfit, mlp) under `t<t>/<k>/`: moves [C, 3] (frame, dx, dy), plt / cam / mic corners [R, 2] int32,
wrm [R, 4] float64, cycle, phase (0 imaging, 1 moving), bbox_error and mse_error [R] (ErrorCalculator), describe [29, 5 + Q] (DataAnalyzer: initialize
(period 10), change_unit("sec") with THAT recording's TimingConfig, describe).  Under `pooled/<k>/describe` the describe of the three cleaned frames
concatenated by the real Plotter.  `t<t>/track`: the input as the reference's controllers read it (pandas).  The log's text is parsed with Python's
float (round-trip exact).  tests/test_replay_set_scales_ref.py asserts the conditions the fixture exists for (the clip binds on every track, a clipped
value differs between the 88 and the 92 px/mm bound, rows with zero and with non-zero bbox error on every track).

Usage: python tests/golden/make_replay_set_scales_golden.py
"""
import csv
import json
import os
import shutil
import sys
import tempfile
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_eval_golden  # noqa: E402
import make_golden  # noqa: E402
from make_analysis_golden import PERCENTILES  # noqa: E402
from make_golden import REF  # noqa: E402

FPS, TIMING = 60, (100, 40, 50)
CAMERA_SIZE_MM, MICRO_SIZE_MM = (4, 4.1), (0.32, 0.33)
ORIG_RESOLUTION = (1600, 1400)
RECORDINGS = [  # px_per_mm, frames, init_position, seed, NaN rows (no two neighbours, none in the first cycles: make_replay_golden.py says why)
    dict(px_per_mm=88, num_frames=352, init_position=(640, 520), seed=881, nan_rows=(61, 203)),
    dict(px_per_mm=90, num_frames=318, init_position=(900, 700), seed=902, nan_rows=(94, 150, 262)),
    dict(px_per_mm=92, num_frames=391, init_position=(420, 860), seed=923, nan_rows=(47, 330)),
]
POLYFIT = dict(degree=2, sample_times=[-9, -6, -3, 0, 2, 4], weights=[1, 1, 2, 3, 4, 5])
MODEL, MAX_SPEED = "ResMLP(imaging-100ms_pred-40ms_moving-50ms).pt", 0.9
PERIOD = 10
KINDS = ("csv", "polyfit", "mlp")


def scaled_track(rec: dict) -> np.ndarray:
    """Seeded head track [num_frames, 4] xywh around the recording's init position: stretches of 25 - 60 frames, alternately slow (about 0.5 px per
    frame) and fast (about 3.5 px per frame), with a wandering heading."""
    rng = np.random.default_rng(rec["seed"])
    n = rec["num_frames"]
    pos = np.array(rec["init_position"], dtype=np.float64) + rng.normal(0, 2.0, 2)
    heading, fast, left = rng.uniform(0, 2 * np.pi), False, 30
    out = np.empty((n, 4))
    for i in range(n):
        if left == 0:
            fast, left = not fast, int(rng.integers(25, 60))
            heading += rng.normal(0.0, 0.8)
        left -= 1
        speed = max(0.1, rng.normal(3.5, 0.8)) if fast else max(0.05, rng.normal(0.5, 0.2))
        heading += rng.normal(0.0, 0.05)
        pos = pos + speed * np.array([np.cos(heading), np.sin(heading)])
        w, h = 13.8 + rng.normal(0, 0.6), 14.6 + rng.normal(0, 0.6)
        out[i] = (pos[0] - w / 2, pos[1] - h / 2, w, h)
    out[list(rec["nan_rows"])] = np.nan
    return out


def main():
    make_eval_golden._register_placeholders()  # cv2 (tolerant), tkinter, seaborn
    make_golden._register_placeholders()  # + ultralytics
    if REF not in sys.path:
        sys.path.insert(0, REF)
    import pandas as pd
    import torch
    from wtracker.eval.data_analyzer import DataAnalyzer
    from wtracker.eval.error_calculator import ErrorCalculator
    from wtracker.eval.plotter import Plotter
    from wtracker.sim.config import ExperimentConfig, TimingConfig
    from wtracker.sim.sim_controllers.csv_controller import CsvController
    from wtracker.sim.sim_controllers.logging_controller import LogConfig, LoggingController
    from wtracker.sim.sim_controllers.mlp_controllers import MLPController
    from wtracker.sim.sim_controllers.polyfit_controller import PolyfitConfig, PolyfitController
    from wtracker.sim.simulator import Simulator

    torch.manual_seed(0)
    torch.set_num_threads(1)
    model = torch.load(os.path.join(REF, "models", MODEL), weights_only=False, map_location="cpu")
    model.eval()
    columns = None
    work = tempfile.mkdtemp(prefix="wtk_scales_golden_")
    out, cleaned, geometry = {}, {k: [] for k in KINDS}, []
    try:
        for t, rec in enumerate(RECORDINGS):
            init_csv = os.path.join(work, f"track{t}.csv")
            with open(init_csv, "w") as f:
                f.write("frame,wrm_x,wrm_y,wrm_w,wrm_h\n")
                for i, r in enumerate(scaled_track(rec)):
                    f.write(f"{i}," + ",".join("" if not np.isfinite(v) else repr(float(v)) for v in r) + "\n")
            out[f"t{t}/track"] = pd.read_csv(init_csv, usecols=["wrm_x", "wrm_y", "wrm_w", "wrm_h"]).to_numpy(dtype=float)
            ec = ExperimentConfig(name=f"scale{t}", num_frames=rec["num_frames"], frames_per_sec=FPS, orig_resolution=ORIG_RESOLUTION,
                                  px_per_mm=rec["px_per_mm"], init_position=rec["init_position"])
            tc = TimingConfig(ec, *TIMING, CAMERA_SIZE_MM, MICRO_SIZE_MM)
            L = tc.cycle_frame_num
            geometry.append(dict(L=L, I=tc.imaging_frame_num, M=tc.moving_frame_num, P=tc.pred_frame_num, camera_size_px=list(tc.camera_size_px),
                                 micro_size_px=list(tc.micro_size_px), mm_per_px=tc.mm_per_px, ms_per_frame=tc.ms_per_frame,
                                 max_dist_per_pred=MAX_SPEED * (tc.px_per_mm / tc.frames_per_sec) * model.io_config.pred_frames[0]))
            makers = {"csv": lambda: CsvController(tc, init_csv), "polyfit": lambda: PolyfitController(tc, PolyfitConfig(**POLYFIT), init_csv),
                      "mlp": lambda: MLPController(tc, init_csv, model, max_speed=MAX_SPEED)}
            for kind in KINDS:
                ctrl = makers[kind]()
                rec_moves, orig = [], ctrl.provide_movement_vector

                def wrapped(sim, orig=orig, rec_moves=rec_moves):
                    dx, dy = orig(sim)
                    rec_moves.append([int(sim.frame_number), int(dx), int(dy)])
                    return dx, dy

                ctrl.provide_movement_vector = wrapped
                tmp = tempfile.mkdtemp(prefix="run_", dir=work)
                lc = LogConfig(root_folder=tmp, save_mic_view=False, save_cam_view=False, save_err_view=False, save_wrm_view=False)
                Simulator(tc, ec, LoggingController(ctrl, lc)).run()
                with open(lc.bbox_file_path, newline="") as f:
                    rows = list(csv.DictReader(f))
                num = lambda cols, dt: np.array([[float(r[c]) for c in cols] for r in rows], dtype=np.float64).astype(dt)  # noqa: E731
                assert [int(r["frame"]) for r in rows] == list(range(len(rows))) and len(rows) == (rec["num_frames"] - 1) // L * L
                cam_wh, mic_wh = num(["cam_w", "cam_h"], np.int32), num(["mic_w", "mic_h"], np.int32)
                assert (cam_wh == tc.camera_size_px).all() and (mic_wh == tc.micro_size_px).all()
                plt, cam, mic = num(["plt_x", "plt_y"], np.int32), num(["cam_x", "cam_y"], np.int32), num(["mic_x", "mic_y"], np.int32)
                wrm = num(["wrm_x", "wrm_y", "wrm_w", "wrm_h"], np.float64)
                mic_boxes = np.concatenate([mic, mic_wh], axis=1).astype(np.int64)
                key = f"t{t}/{kind}/"
                out[key + "moves"] = np.array(rec_moves, dtype=np.int32)
                out[key + "plt"], out[key + "cam"], out[key + "mic"], out[key + "wrm"] = plt, cam, mic, wrm
                out[key + "cycle"] = np.array([int(r["cycle"]) for r in rows], dtype=np.int32)
                out[key + "phase"] = np.array([{"imaging": 0, "moving": 1}[r["phase"]] for r in rows], dtype=np.int8)
                out[key + "bbox_error"] = ErrorCalculator.calculate_bbox_error(wrm.copy(), mic_boxes.copy())
                out[key + "mse_error"] = ErrorCalculator.calculate_mse_error(wrm.copy(), mic_boxes.copy())
                an = DataAnalyzer.load(tc, lc.bbox_file_path)  # the log through its OWN TimingConfig
                an.initialize(period=PERIOD)
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    an.change_unit("sec")
                if columns is None:
                    columns = [c for c in an.data.columns if c not in ("phase", "precise_error")]
                desc = an.describe(columns, percentiles=list(PERCENTILES))
                assert list(desc.index[:4]) == ["count", "mean", "std", "min"] and desc.index[-1] == "max", list(desc.index)
                out[key + "describe"] = desc.to_numpy(dtype=np.float64).T.copy()
                cleaned[kind].append(an.data)
                print(key, "rows", len(rows), "cam", tc.camera_size_px, "mic", tc.micro_size_px, "non-zero bbox error %.3f" % float((out[key + "bbox_error"] > 1e-7).mean()))
        assert [g["camera_size_px"] for g in geometry] == [[352, 361], [360, 369], [368, 377]], geometry
        assert [g["micro_size_px"] for g in geometry] == [[28, 29], [29, 30], [29, 30]], geometry
        assert len({(g["L"], g["I"], g["M"], g["P"]) for g in geometry}) == 1
        for kind in KINDS:
            data = Plotter(cleaned[kind]).data  # log_num and the concatenation are the Plotter's own
            desc = data[columns].describe(list(PERCENTILES))
            out[f"pooled/{kind}/describe"] = desc.to_numpy(dtype=np.float64).T.copy()
        out["meta"] = np.frombuffer(json.dumps(dict(
            frames_per_sec=FPS, timing=list(TIMING), camera_size_mm=list(CAMERA_SIZE_MM), micro_size_mm=list(MICRO_SIZE_MM), orig_resolution=list(ORIG_RESOLUTION),
            recordings=[dict(r, init_position=list(r["init_position"]), nan_rows=list(r["nan_rows"])) for r in RECORDINGS], polyfit=POLYFIT, max_speed=MAX_SPEED,
            model="resmlp_100ms.npz", kinds=list(KINDS), period=PERIOD, columns=columns, percentiles=list(PERCENTILES), geometry=geometry)).encode(), dtype=np.uint8)
        path = os.path.join(HERE, "replay_set_scales.npz")
        np.savez_compressed(path, **out)
        print(path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "replay_hard.npz"))
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
