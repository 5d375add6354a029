#!/usr/bin/env python3
"""sha256 digests of what the polynomial-fit kernels and the two weight searches return on tests/golden/replay_hard.npz (100 ms imaging: L = 5, 80 cycles),
as one JSON object.  Run it with two builds of the library (WTK_HIP_LIB names another one) and compare the lines: a refactor of csrc/polyfit_solve.h or of
polyfit_opt.swarm_search must leave every digest as it was.
Usage: [WTK_HIP_LIB=other.so] python tools/polyfit_bits.py"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(0, [0]), (2, [-8, -6, -4, -2, 0, 1]), (3, list(range(-6, 2))), (7, list(range(-14, 2)))]  # (degree, sample times)
TIMES, POP, SEARCH = SHAPES[1][1], 70, dict(pop_size=70, max_epoch=12, seed=3)


def sha(*arrays) -> str:
    h = hashlib.sha256()
    for a in arrays:
        a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def search_sha(r) -> str:
    return sha(r.weights, np.float64(r.mae), r.history, np.int64(r.epochs))


def main():
    import torch

    from wtracker_amd import hip
    from wtracker_amd.polyfit_opt import WeightEvaluator
    from wtracker_amd.replay import Replay
    from wtracker_amd.sim import ExperimentConfig, TimingConfig

    if hip.device_count() < 1:
        raise SystemExit("polyfit_bits: no HIP device visible")
    z = np.load(os.path.join(ROOT, "tests", "golden", "replay_hard.npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    ec = ExperimentConfig("hard", meta["num_frames"], meta["frames_per_sec"], tuple(meta["orig_resolution"]), meta["px_per_mm"], tuple(meta["init_position"]))
    tc = TimingConfig(ec, 100, 40, 50, meta["camera_size_mm"], meta["micro_size_mm"])
    rp = Replay(z["track"], tc, ec)
    assert (rp.L, rp.n_cycles) == (5, 80)
    t_eval, C, dev = rp.L + rp.I // 2, rp.n_cycles, rp._dev
    out = {}  # nothing that names the build: two runs are compared byte for byte
    rng = np.random.default_rng(7)
    for degree, times in SHAPES:
        N = len(times)
        w = rng.uniform(0.05, 1.0, size=N)
        sparse = np.zeros(N)
        sparse[-2:] = w[-2:]  # all but two weights zero: rank deficient from degree 2 on
        for name, track in (("f64", rp.track), ("f32", rp.track.to(torch.float32).contiguous())):
            for wname, wv in (("dense", w), ("sparse", sparse)):
                pred, ok = torch.zeros((C, 2), dtype=torch.float64, device=dev), torch.zeros((C,), dtype=torch.int32, device=dev)
                hip.track_polyfit(track, rp.n_track, rp._cycles, C, rp.L, times, wv, degree, t_eval, pred, ok, stream=rp._stream())
                out[f"track_polyfit d{degree} n{N} {name} {wname}"] = sha(pred, ok)
        weights = rng.uniform(0.05, 1.0, size=(POP, N))
        weights[1] = sparse
        tg = rp.polyfit_population(weights, degree, times)
        out[f"polyfit_population d{degree} n{N}"] = sha(tg.a, tg.valid)
    ev16 = WeightEvaluator.from_tracks([z["track"]], tc, SHAPES[3][1], t_eval)
    w16 = rng.uniform(0.05, 1.0, size=(POP, 16))
    for degree in (0, 2, 7):
        out[f"eval_many d{degree} n16 series{ev16.n_series}"] = sha(ev16.eval_many(w16, degree))
    ev = WeightEvaluator.from_tracks([z["track"]], tc, TIMES, t_eval)
    out["WeightEvaluator.optimize"] = search_sha(ev.optimize(2, **SEARCH))
    out["Replay.optimize_polyfit"] = search_sha(rp.optimize_polyfit(2, TIMES, **SEARCH))
    out["Replay.optimize_polyfit lb=0.05"] = search_sha(rp.optimize_polyfit(2, TIMES, lb=0.05, **SEARCH))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
