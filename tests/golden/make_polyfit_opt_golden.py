#!/usr/bin/env python3
"""Generate tests/golden/polyfit_opt.npz by running the REAL reference's WeightEvaluator (wtracker/sim/sim_controllers/polyfit_controller.py:87-221).

Runs only where the reference is installed (it never travels to the GPU box); the reference is imported exactly as make_golden.py does (placeholder
`tkinter` / `cv2` / `ultralytics`).  Nothing of the reference's source is copied: the file holds numbers only.

  track                          [6000, 4] xywh float64 as the reference read it from its csv: seeded random walk (make_golden.synthetic_track), a slow stretch
                                 (frames 2400-3100 move at 8 % of their speed) so that the speed window removes cycles, 0.5 % NaN rows; values on a 1/16 px grid
                                 (keeps the compressed file small)
  per configuration c in (a, b)  c_timing (imaging, pred, moving ms), c_cycle_frame_num, c_offsets_given (as handed to the constructor, UNSORTED for b),
                                 c_x_input (the reference's sorted axis), c_pred_time_offset, c_speed (min, max), c_y_input, c_y_target, c_kept,
                                 c_mae [3, 256]: the reference's eval at degrees 1, 2, 3 for the 256 rows of c_weights
        a  the notebook's 8 offsets with 200/40/50 ms timing      b  6 offsets with 100/40/50 ms timing
  degrees                        (1, 2, 3)
  restatement_dev                worst relative deviation between the reference's eval and tests/harness/polyfit_opt_ref.mae over all 1 536 values
"""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden  # noqa: E402
from harness import polyfit_opt_ref as ref  # noqa: E402

DEGREES = (1, 2, 3)
N_FRAMES = 6000


def make_track() -> np.ndarray:
    t = make_golden.synthetic_track(N_FRAMES, seed=11, start=(900.0, 700.0), nan_rows=())
    c = np.stack([t[:, 0] + t[:, 2] / 2, t[:, 1] + t[:, 3] / 2], axis=1)
    step = np.diff(c, axis=0)
    step[2400:3100] *= 0.08
    c = np.concatenate([c[:1], c[:1] + np.cumsum(step, axis=0)])
    t[:, 0], t[:, 1] = c[:, 0] - t[:, 2] / 2, c[:, 1] - t[:, 3] / 2
    t = np.round(t * 16) / 16
    rng = np.random.default_rng(12)
    t[rng.choice(N_FRAMES, size=N_FRAMES // 200, replace=False)] = np.nan
    return t


def make_weights(n: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.0, 1.0, size=(256, n))
    for r in range(200, 220):  # exact zeros
        w[r, rng.choice(n, size=1 + r % 3, replace=False)] = 0.0
    for r in range(220, 240):  # 1, 2 or 3 non-zero weights: fewer than deg + 1 for the higher degrees
        keep = rng.choice(n, size=1 + r % 3, replace=False)
        row = np.zeros(n)
        row[keep] = w[r, keep]
        w[r] = row
    w[240] = 1.0
    w[241] = 0.0
    w[242:249] *= 1e-6
    w[249:256] *= 1e6
    return w


def main():
    make_golden._register_placeholders()
    sys.path.insert(0, make_golden.REF)
    import pandas as pd
    from wtracker.sim.config import ExperimentConfig, TimingConfig
    from wtracker.sim.sim_controllers.polyfit_controller import WeightEvaluator

    track = make_track()
    tmp = tempfile.mkdtemp(prefix="wtk_polyfit_opt_")
    csv = os.path.join(tmp, "bboxes.csv")
    with open(csv, "w") as f:
        f.write("frame,wrm_x,wrm_y,wrm_w,wrm_h\n")
        for i, r in enumerate(track):
            f.write(f"{i}," + ",".join("" if not np.isfinite(v) else repr(float(v)) for v in r) + "\n")
    track = pd.read_csv(csv, usecols=["wrm_x", "wrm_y", "wrm_w", "wrm_h"]).to_numpy(dtype=float)
    out = {"track": track, "degrees": np.asarray(DEGREES)}
    worst = 0.0
    for tag, timing, seed in (("a", (200, 40, 50), 21), ("b", (100, 40, 50), 22)):
        ec = ExperimentConfig(name="exp", num_frames=N_FRAMES, frames_per_sec=60, orig_resolution=(1600, 1400), px_per_mm=90, init_position=(900, 700))
        tc = TimingConfig(ec, *timing, (4, 4), (0.32, 0.32))
        L = tc.cycle_frame_num
        if tag == "a":
            offsets = [-3 * L, -3 * L + 6, -2 * L, -2 * L + 6, -L, -L + 6, 0, 3]
        else:
            offsets = [0, -2 * L + 4, 3, -L, -2 * L, -L + 4]
        pred = L + tc.imaging_frame_num // 2
        speed = (0.1, 2.0)
        ev = WeightEvaluator([csv], tc, np.asarray(offsets), pred, min_speed=speed[0], max_speed=speed[1])
        w = make_weights(len(offsets), seed)
        mae = np.array([[ev.eval(w[r], deg=d) for r in range(len(w))] for d in DEGREES])
        for di, d in enumerate(DEGREES):
            for r in range(len(w)):
                mine = ref.mae(ev.y_input, ev.y_target, ev.x_input, w[r], d, pred)
                worst = max(worst, abs(mine - mae[di, r]) / abs(mae[di, r]))
        y_in, y_tg, kept = ref.dataset(track, L, offsets, pred, *speed)
        assert np.array_equal(y_in, ev.y_input) and np.array_equal(y_tg, ev.y_target), "harness dataset differs from the reference's"
        out.update({f"{tag}_timing": np.asarray(timing), f"{tag}_cycle_frame_num": np.asarray(L), f"{tag}_offsets_given": np.asarray(offsets),
                    f"{tag}_x_input": np.asarray(ev.x_input), f"{tag}_pred_time_offset": np.asarray(pred), f"{tag}_speed": np.asarray(speed),
                    f"{tag}_y_input": ev.y_input, f"{tag}_y_target": ev.y_target, f"{tag}_kept": np.asarray(kept), f"{tag}_weights": w, f"{tag}_mae": mae})
        print(tag, "L", L, "pred", pred, "series", ev.y_target.size, "candidate cycles", -(-N_FRAMES // L), "mae range", mae.min(), mae.max())
    out["restatement_dev"] = np.asarray(worst)
    print("restatement_dev", worst)
    path = os.path.join(HERE, "polyfit_opt.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
