#!/usr/bin/env python3
"""Generate tests/golden/replay_precise.npz by running the REAL reference's ErrorCalculator.calculate_precise (wtracker/eval/error_calculator.py:64-160)
on the replayed logs of four experiments of the first scenario of tests/harness/replay_precise_ref.py (scenario_main: 96 x 131 frames, 70 jittered
OPTIMAL experiments, R = 120 rows each).

Runs only where a checkout of the reference is available (make_eval_golden.REF; it never travels with the tests).  Nothing of the reference's source
is copied: the outputs are numeric data only.  The placeholder modules and the worm-view reader are make_eval_golden.py's.

replay_precise.npz
  the scenario as the tests rebuild it from its seed (track, frames, background, a, valid: they are compared, so a numpy whose generator drew other
  numbers fails loudly instead of testing another scenario; the frames are three grey levels, a dark ellipse and 40 speckles each, so the file
  compresses to a few dozen KB), experiments = the four experiment ids, and per experiment e: worm_e / mic_e, the wrm / mic columns of its replayed
  log (replay_ref.rows, pinned to the reference's Simulator by tests/test_replay_ref.py), and ref_e = calculate_precise's return value in its own
  layout (the legal rows' errors first) at diff_thresh = 20, DataAnalyzer.calc_precise_error's default.

Usage: python tests/golden/make_replay_precise_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_eval_golden import _register_placeholders, _WormViews  # noqa: E402

EXPERIMENTS = (0, 63, 64, 69)
DIFF_THRESH = 20


def main():
    _register_placeholders()
    from harness import replay_precise_ref as pr
    from harness import replay_ref as rr
    from wtracker.eval.error_calculator import ErrorCalculator
    from wtracker.utils.bbox_utils import BoxFormat, BoxUtils

    def disc(b, bounds):
        return BoxUtils.discretize(b, bounds=bounds, box_format=BoxFormat.XYWH)

    sc = pr.scenario_main()
    g, R = sc["g"], sc["g"].n_log * sc["g"].L
    pos, move = pr.scan_of(sc)
    out = dict(track=sc["track"], frames=sc["frames"], background=sc["bg"], a=sc["a"], valid=sc["valid"], experiments=np.array(EXPERIMENTS, dtype=np.int64),
               diff_thresh=np.float64(DIFF_THRESH))
    frame_nums = np.arange(R, dtype=np.int64)
    for e in EXPERIMENTS:
        rows = rr.rows(g, sc["track"], pos, move, e, summaries=False)["rows"]
        worm, mic = rows[:, 10:14].copy(), rows[:, 6:10].copy()
        views = _WormViews(sc["frames"], worm, disc)
        views.frame_nums = frame_nums
        ref = ErrorCalculator.calculate_precise(background=sc["bg"], worm_bboxes=worm.copy(), mic_bboxes=mic.copy(), frame_nums=frame_nums.copy(),
                                                worm_reader=views, diff_thresh=DIFF_THRESH)
        assert views.k == len(views.views)
        out[f"worm_{e}"], out[f"mic_{e}"], out[f"ref_{e}"] = worm, mic, np.asarray(ref, dtype=np.float64)
    path = os.path.join(HERE, "replay_precise.npz")
    np.savez_compressed(path, **out)
    print("replay_precise.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
