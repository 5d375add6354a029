#!/usr/bin/env python3
"""bench.py — frames/s of the YOLOv8s + ResMLP sim-loop hot path on MI355X (BASELINE.json metric).

One "step" = one super-batch: every rank runs the detector (63 conv layers in ~50 launches: fused front, fused C2f tail,
implicit-GEMM and window-kernel convs with fused Detect tails, SPPF pool, head select) on its `--batch` synthetic 640x640
frames that are already resident in HBM, the [B,4] track slices are all-gathered (N > 1 only), and the ResMLP movement
vectors of the cycles that became computable are produced (wtracker_amd/pipeline.py).  Prints ONE JSON line on rank 0.

  python bench.py --gpus 1 --steps 20 --warmup 3                      # plain run: the headline alone
  python bench.py --gpus 1 --steps 20 --warmup 3 --full               # + every other figure and check below
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
      --master-port P bench.py --gpus N --steps K --warmup W

A plain run sets up, warms up, times EXACTLY `--steps` steps of the headline mode (one window; `--repeats R` asks for R windows),
writes that mode's outputs of its last timed step with `--dump-outputs DIR` (DIR/xywh.npy, conf.npy, anchor.npy, moves.npy,
move_valid.npy: float32, same seeded inputs in every run) and prints the line.  Everything marked [full] below is measured
only with `--full`.

What the line carries (everything measured inside this one command):
  value / ms_per_step   the HEADLINE mode (`dtype`): a plain run with the default `--dtype auto` times the reference-precision mode
                        "f16x3"; with `--full` it is the fastest reference-precision mode ("f16x3", else "fp32") whose survivor
                        indices equal the fp32 CPU restatement's on EVERY parity frame of this run; the choice is made from the
                        `parity` object measured in this very command (N = 1).
                        The reference computes in fp32 and keeps the arg-max anchor (yolo/yolo_train_config.yaml:51,
                        yolo_controller.py:76): a mode that picks another survivor on some frames is not the headline.
                        `--repeats` timed windows of EXACTLY `--steps` steps each, every window bracketed by barrier + device
                        synchronisation, MAX over ranks per window; value = frames of one window / MEDIAN window
  headline_exactness_verified, headline_check
                        [full] the parity gate and the device-side check of the headline mode (null in a plain run)
  roofline              [full] dominant kernel of the headline mode, algorithmic FLOPs / live HIP-event launch time
  value_fp16 / value_hybrid / value_f16x3 / value_fp32, parity_index_match_<mode>, hybrid_overflow, hybrid_second_look_share
                        flat copies of the per-mode numbers (a plain run: the headline mode's value only; the others [full], N = 1 only)
  fp16_throughput       [full] the plain fp16 mode: labelled, NOT the headline (survivor index differs on ~2 % of the frames)  (N = 1 only)
  hybrid / f16x3 / fp32 per-mode objects: value / windows / roofline; hybrid and fp32 [full]                              (N = 1 only)
  parity                [full] survivor-index match rate and IoU distribution of ALL modes against the fp32 CPU restatement on
                        the CPU leg's frames, computed outside the timed regions                               (N = 1 only)
  cpu_baseline          [full] oracle/ (kind "port") timed on the host cores at B = 64, 15 and 1               (N = 1 only)
  closed_loop, latency  [full] the reference's operating point and its small-batch calls                       (N = 1 only)
  dist                  N > 1: world size and backend as torch.distributed reports them + a checksum of the gathered track
Fields that cannot be measured from inside the process (HBM bytes and MFMA-busy share come from rocprofv3 PMC passes) are
read from profiles/*.json ONLY when that file was collected on exactly these kernel sources (`src_sha`), and then carry a
`provenance` entry; otherwise they are null.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# One hardware queue per stream: the HIP runtime multiplexes streams onto GPU_MAX_HW_QUEUES (default 4) hardware queues.  This process keeps five
# streams busy (two lanes, the shared pair of side streams, torch's default stream); with four queues two of them share one and serialise:
# 26.2 k frames/s against 27.1 k with 5, 6 or 8 queues (profiles/r02_notes.md §8).  Read by the runtime when it initialises: set before torch loads.
# (wtracker_amd.hip.request_hw_queues() is the same request for other users of the library; hip.load() itself leaves the environment alone.)
# N > 1 with RCCL (`--backend nccl`): one process per GPU, so the eight queues are per DEVICE exactly as at N = 1; RCCL adds its own
# stream(s) for the one 1-KiB all-gather per step, which is why the value is 8 and not 5.  The one-GPU rehearsal of the multi-rank path
# (`--backend gloo`, every rank on cuda:0) keeps the runtime default: there the processes share a device and their queues add up (19.5 k -> 4.9 k).
_pre = argparse.ArgumentParser(add_help=False)
_pre.add_argument("--backend", default="nccl")
_pre.add_argument("--legs-child", action="store_true")  # (the small-batch legs' child process keeps the runtime default: a controller user's environment)
if _pre.parse_known_args()[0].backend == "nccl" and not _pre.parse_known_args()[0].legs_child:
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

import numpy as np  # noqa: E402
import torch  # noqa: E402

# dense MFMA peaks, /opt/skills/guides/MI355X_MICROARCH.md.  f16x3 (split-fp16 operands): a product is three fp16 MFMAs, so the
# ALGORITHMIC flop rate (2 per multiply-accumulate of the model) is bounded by a third of the fp16 peak.
PEAK_TFLOPS = {"fp16": 2500.0, "fp32": 157.3, "f16x3": 2500.0 / 3.0, "hybrid": 2500.0}  # hybrid: the profiled handle is its fp16 one
PEAK_BASIS = {"fp16": "fp16 dense MFMA 2.5 PFLOP/s", "hybrid": "fp16 dense MFMA 2.5 PFLOP/s (the profiled handle is the fp16 one)",
              "fp32": "fp32 matrix (v_mfma_f32_16x16x4_f32) 157.3 TFLOP/s",
              "f16x3": "fp16 dense MFMA 2.5 PFLOP/s / 3 MFMAs per product (split-fp16 operands): 833.3 TFLOP/s algorithmic"}
HBM_PEAK_GBPS = 8000.0
# the hybrid sub-object: decisions with a margin below 0.04 get a second, full-precision look (at most 24 per 64 frames).  Every survivor mismatch of the
# fp16 mode measured so far (30 in 1 792 frames, tools/margin_study.py) has a margin below 0.019; 16.5 % of the frames are below 0.04, at most 16 per batch.
# The second look's cost follows the NUMBER of weak frames (device-side dynamic batch, wtk_yolo_set_dynamic_batch), so K is only a ceiling.
# Ceiling = the whole batch (K = B): NO weak row can be cut off, by construction (ADVICE r02 / VERDICT r02 item 4); the overflow counter of
# wtk_recheck_select_counted is reported anyway and must read 0.
# The margin is CALIBRATED on this model inside the run (HybridDetector.calibrate on HYBRID_CAL_FRAMES frames the timed region and the parity leg never
# see: max(6 sigma of the fp16 decision margin's noise against f16x3, 2 x the largest margin of any outright disagreement, 0.02)): the fp16 logit noise is
# a property of the weights — sigma 0.012 for the seed-0 draw used here, 0.055 for other draws (tests/test_gpu_hybrid_validation.py validates the
# procedure out of sample on four draws) — so a fixed number would be a guess: round 2's 0.04 is ~3.3 sigma here, i.e. about one wrong survivor in 1e5 frames.
HYBRID_MARGIN_FALLBACK = 0.04
HYBRID_CAL_FRAMES, HYBRID_CAL_SEED = 512, 40000
# Deferred second look: the weak rows of HYBRID_DEFER consecutive batches of a lane share one f16x3 pass (its fixed cost of ~1.2 ms is paid once per
# HYBRID_DEFER batches); queue of HYBRID_QUEUE rows per lane = 40 % of the frames it can receive — a fuller queue is COUNTED (overflow) and demotes the mode.
HYBRID_DEFER, HYBRID_QUEUE_PER_64 = 5, 128
HYBRID_EXACT_MEM_GB = 48.0  # f16x3 workspace of one lane's second-look handle
PROFILE_ROUND = "r06"
# The headline is a REFERENCE-PRECISION mode (the reference computes in fp32: yolo/yolo_train_config.yaml:51 `half: False`): the fastest of these whose
# survivor index equals the fp32 restatement's on every parity frame of the run AND whose boxes pass BASELINE.md section 4's gate (matched IoU >= 0.999).
# fp16 (throughput) and hybrid (fp16 rows + a full-precision second look at weak decisions: index-exact by a calibrated margin, boxes of the
# unchecked rows are fp16 rows — matched IoU >= 0.98, 1 px) are labelled sub-objects, never the headline of `--dtype auto`.
HEADLINE_CANDIDATES = ("f16x3", "fp32")
HEADLINE_IOU_MIN = 0.999
PMC_SUFFIX = {"fp16": "", "hybrid": "", "f16x3": "_f16x3"}  # committed profiles/<round>_conv_traffic<suffix>.json / _pmc_mfma_util<suffix>.json


def cpu_baseline(weights, dims, size: int, folded_path: str, frames64: np.ndarray, conf: float) -> tuple:
    """The CPU restatement (oracle/, kind 'port') on a bounded sample of the same workload, at the three batch sizes of
    BASELINE.md §4: 64 (the benched super-batch), 15 (the reference's real cycle batch, yolo_controller.py:108-109) and 1
    (provide_movement_vector, yolo_controller.py:96-98).  Thread count: the torch-CPU conv stack peaks near 32 threads on the
    GPU box's host (8: 14.8, 16: 18.3, 32: 19.2, 64: 11.4, 128: 5.9 frames/s measured with tools/cpu_threads_probe.py), so
    min(cores, 32) is used.  Returns (json object, oracle outputs on `frames64` = the checker for the parity object)."""
    from oracle import resmlp_oracle
    from oracle import yolo_oracle as yo

    cores = min(os.cpu_count() or 1, 32)
    torch.set_num_threads(cores)
    model = yo.YoloOracle(weights, dims)
    st = resmlp_oracle.load_state(folded_path)

    def timed(frames, batch, warm_batches):
        for i in range(warm_batches):
            yo.predict(model, list(frames[:batch]), imgsz=size, conf=conf)
        outs = []
        t0 = time.perf_counter()
        for i in range(0, len(frames), batch):
            outs.append(yo.predict(model, list(frames[i : i + batch]), imgsz=size, conf=conf))
        resmlp_oracle.forward(st, np.zeros((max(len(frames) // 9, 1), 28), dtype=np.float32))  # one ResMLP sample per 9-frame cycle
        dt = time.perf_counter() - t0
        return dt, outs

    dt64, outs = timed(frames64, 64, 1)
    checker = tuple(np.concatenate([o[k] for o in outs]) for k in range(3))
    dt15, _ = timed(frames64[:60], 15, 1)
    dt1, _ = timed(frames64[:24], 1, 2)
    by_batch = {"64": {"value": len(frames64) / dt64, "frames": len(frames64), "seconds": dt64},
                "15": {"value": 60 / dt15, "frames": 60, "seconds": dt15},
                "1": {"value": 24 / dt1, "frames": 24, "seconds": dt1}}
    obj = {"value": by_batch["64"]["value"], "unit": "frames/s", "cores": cores, "kind": "port", "by_batch": by_batch,
           "sample": f"{len(frames64)} synthetic {size}x{size} frames in batches of 64 (value), 60 in batches of 15, 24 one at a time; torch-CPU fp32 "
                     f"restatement (oracle/yolo_oracle.py) + numpy ResMLP, {cores} threads, {dt64 + dt15 + dt1:.1f} s"}
    return obj, checker


def closed_loop(weights, scale: str, nc: int, device: int, conf: float) -> dict:
    """The reference's REAL operating point, outside the headline: a closed-loop experiment driven through the controller API —
    per cycle ONE `_cycle_predict_all` over the cycle's camera views and ONE single-frame `provide_movement_vector` call (yolo_controller.py:95-109) —
    at the reference's shapes: 360 x 360 camera views (4 mm at 90 px/mm) of larger frames, letterboxed to imgsz 384 (initialize_experiment.ipynb
    cell 9), 200 / 40 / 50 ms timing at 60 fps = 15-frame cycles.  `HipYoloController(device_frames=...)`: frames resident in HBM, views cut and
    letterboxed on the device; its calls return numpy rows, so every figure is host-inclusive (launches, the 12-byte-per-view upload, the D2H of the
    rows, the host sync).  Next to it the CPU restatement's controller (oracle/controllers_oracle.py: OracleYoloController) on the host cores, same
    frames, same driver (tests/harness: the stand-in for the reference's Simulator, pinned by the reference's logs)."""
    import tempfile

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from harness.sim_harness import ArrayReader, Simulator
    from oracle import yolo_oracle as yo
    from oracle.controllers_oracle import OracleYoloController
    from wtracker_amd import frames as fr
    from wtracker_amd import yolo_spec as ys
    from wtracker_amd.controllers import HipYoloController, YoloConfig
    from wtracker_amd.sim import ExperimentConfig, TimingConfig, TrackLogger

    size, cycles = 1024, 30
    ec = ExperimentConfig("closed_loop", cycles * 15 + 1, 60, (size, size), 90, (size // 2, size // 2))
    frames_np, _ = fr.synthetic_frames(ec.num_frames, size, seed=77)
    dev_frames = torch.from_numpy(frames_np).to(torch.device("cuda", device))
    tmp = tempfile.NamedTemporaryFile(suffix=".wtk", delete=False)
    tmp.close()
    ys.save_weights(tmp.name, weights, scale, nc)

    def drive(make, deferred=False):
        tc = TimingConfig(ec, 200, 40, 50, (4, 4), (0.32, 0.32))
        assert (tc.imaging_frame_num, tc.pred_frame_num, tc.moving_frame_num, tc.cycle_frame_num, tc.camera_size_px) == (12, 3, 3, 15, (360, 360))
        ctrl = make(tc)
        moves, calls = [], {1: [], 15: []}
        for name in ("predict_views", "predict"):  # time every detector call of the controller by its batch size
            if hasattr(ctrl, name):
                inner = getattr(ctrl, name)

                def timed(frames_or_entries, _inner=inner):
                    t0 = time.perf_counter()
                    r = _inner(frames_or_entries)
                    calls.setdefault(len(frames_or_entries), []).append(time.perf_counter() - t0)
                    return r

                setattr(ctrl, name, timed)
        pmv = ctrl.provide_movement_vector

        def wrapped(sim):
            m = pmv(sim)
            moves.append((int(m[0]), int(m[1])))
            return m

        ctrl.provide_movement_vector = wrapped
        ends = []  # wall clock at every cycle end: the steady state is the MEDIAN cycle (a run of 30 cycles holds the controller's first calls — new
        oce = ctrl.on_cycle_end  # buffers, captures — and the odd host hiccup of tens of milliseconds, which a real run of thousands of cycles does not see)

        def cycle_end(sim):
            oce(sim)
            ends.append(time.perf_counter())

        ctrl.on_cycle_end = cycle_end
        log = TrackLogger(ctrl, deferred=deferred)
        t0 = time.perf_counter()
        Simulator(tc, ec, log, reader=ArrayReader(frames_np)).run()
        dt = time.perf_counter() - t0
        med = lambda v: float(np.median(v) * 1e3) if len(v) else None
        cyc = np.diff(np.array(ends)) if len(ends) > 2 else np.array([dt / cycles])
        return {"seconds": dt, "frames_per_s": 15.0 / float(np.median(cyc)), "ms_per_cycle": float(np.median(cyc)) * 1e3, "ms_per_cycle_p90": float(np.quantile(cyc, 0.9)) * 1e3,
                "frames_per_s_whole_run": ec.num_frames / dt, "ms_cycle_batch_call_B15": med(calls[15][1:] or calls[15]),
                "ms_single_frame_call_B1": med(calls[1][1:] or calls[1]), "calls_B15": len(calls[15]), "calls_B1": len(calls[1])}, moves, log.rows

    out = {"what": "closed loop through the controller API at the reference's operating point; host-inclusive wall time under tests/harness' Simulator.run; frames_per_s = 15 / the median cycle",
           "frames": f"{ec.num_frames} synthetic {size}x{size} uint8 gray frames resident in HBM, camera view 360x360 -> imgsz 384, conf {conf}",
           "timing_ms": [200, 40, 50], "cycle_frames": 15, "cycles": cycles, "calls_per_cycle": "one B=15 _cycle_predict_all + one B=1 provide_movement_vector"}
    ref_moves = None
    rows_of = {}
    for dtype, plan, deferred in (("f16x3", "auto", False), ("fp32", "auto", False), ("f16x3", "latency", False), ("f16x3", "throughput", False), ("f16x3", "auto", True),
                                  ("fp32", "auto", True)):
        cfg = YoloConfig(model_path=tmp.name, device=f"cuda:{device}", pred_kwargs={"imgsz": 384, "conf": conf}, dtype=dtype, scale=scale, max_batch=16, plan=plan)
        drive(lambda tc: HipYoloController(tc, cfg, device_frames=dev_frames), deferred)  # warm-up pass: handle creation, captures
        res, moves, rows = drive(lambda tc: HipYoloController(tc, cfg, device_frames=dev_frames), deferred)
        for det in cfg.model._dets.values():
            det.close()
        cfg.model = None
        res["moves"] = len(moves)
        if ref_moves is None:
            ref_moves = moves
        res["moves_equal_first_mode"] = moves == ref_moves
        if deferred:
            res["rows_equal_immediate_log"] = rows == rows_of[(dtype, plan)]
        else:
            rows_of[(dtype, plan)] = rows
        out[f"{dtype}_{plan}" + ("_deferred_log" if deferred else "")] = res
    out["deferred_log"] = ("*_deferred_log = the same loop under TrackLogger(deferred=True): the cycle batch — which feeds nothing back into the loop — is enqueued at the "
                           "cycle's end on the controller's second lane and its rows are written one cycle later, so it runs on the GPU beside the next cycle's single-frame "
                           "call (a handle each under plan 'auto'); same moves, same rows, the last batch collected inside the timed run")
    out["plans"] = ("*_auto = YoloConfig.plan 'auto' (the default): the single-frame call on a latency-plan handle (split-K convs grouped per dependency level, conv_sk.hip; eager launches on one stream), the "
                    "15-frame call on a throughput-plan handle — each call on the plan that is faster for it; f16x3_latency = both calls on ONE latency-plan handle (a frame's "
                    "result is bit-identical whichever call sees it); f16x3_throughput = both calls on the large-batch kernels (what every call ran on before round 5)")
    # the CPU restatement's controller on the host cores, same frames and driver
    cores = min(os.cpu_count() or 1, 32)
    torch.set_num_threads(cores)
    depth, width, maxch = ys.SCALES[scale]
    oracle = yo.YoloOracle(weights, ys.model_dims(width, depth, maxch, nc))
    res, moves_o, _ = drive(lambda tc: OracleYoloController(tc, oracle, imgsz=384, conf=conf))
    res.update({"cores": cores, "kind": "port", "moves_equal_device": moves_o == ref_moves})
    out["cpu_oracle_controller"] = res
    out["moves_equal_oracle"] = moves_o == ref_moves
    os.unlink(tmp.name)
    return out


LINE_LIMIT = 4096  # the driver keeps the tail of stdout: the final line must be short enough to survive whole (BENCH_r04: a 25 KB line did not parse)
DETAIL_FILE = "bench_detail.json"


def _r(v, digits=5):
    """Floats of the compact line at `digits` significant digits (None stays None)."""
    if isinstance(v, float):
        return float(f"{v:.{digits}g}")
    return v


def _finite(o):
    """NaN / inf -> None all the way down (the line is strict JSON: allow_nan=False)."""
    if isinstance(o, float):
        return o if np.isfinite(o) else None
    if isinstance(o, dict):
        return {k: _finite(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [_finite(v) for v in o]
    if isinstance(o, np.generic):
        return _finite(o.item())
    return o


def compact_line(detail: dict) -> dict:
    """The ONE final stdout line (<= LINE_LIMIT bytes) from the full result object: the contract's keys, the headline mode's window statistics,
    its roofline (with the peak's basis) and end-to-end fraction, the CPU baseline, the parity of every mode in two scalars each, the four per-mode
    values and the latency path's scalars.  Everything else (per-mode objects, kernels[], calibration, closed_loop, latency tables) is in DETAIL_FILE."""
    keep = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data")
    line = {k: _r(detail[k], 7) for k in keep}
    cfg = detail["config"]
    line["config"] = {k: cfg[k] for k in ("workload", "batch_per_gpu", "lanes_per_gpu", "global_batch", "headline_mode", "parallelism") if k in cfg}
    w = detail.get("windows") or {}
    line["windows"] = {k: _r(w.get(k)) for k in ("n", "steps_each", "median_ms", "min_ms", "max_ms")}
    rf = detail.get("roofline")
    if rf:
        keys = ("kernel", "bound", "achieved", "peak", "peak_basis", "unit", "frac", "frac_of_fp16_peak", "traffic", "hbm_gbps", "hbm_frac", "mfma_util_pmc",
                "avg_launch_ms", "flop_per_launch_avg", "launches_per_step", "end_to_end_frac")
        line["roofline"] = {k: _r(rf.get(k)) for k in keys}
        prov = rf.get("provenance") or {}
        line["roofline"]["provenance"] = sorted({f"{p['file']}@{p['src_sha']}" for p in prov.values()}) or None
    else:
        line["roofline"] = None
    cb = detail.get("cpu_baseline")
    if cb:
        line["cpu_baseline"] = {"value": _r(cb["value"]), "unit": cb["unit"], "cores": cb["cores"], "kind": cb["kind"], "sample": cb["sample"][:160]}
    par = detail.get("parity")
    if par:
        line["parity"] = {dt: {"index_match_rate": _r(par[dt]["index_match_rate"]), "iou_matched_min": _r((par[dt].get("iou_matched") or {}).get("min"), 7)}
                          for dt in ("f16x3", "fp32", "hybrid", "fp16") if dt in par}
    line["headline_exactness_verified"] = detail.get("headline_exactness_verified")
    hc = detail.get("headline_check")
    if hc:
        line["headline_check"] = {k: _r(hc[k]) for k in ("frames", "index_mismatches", "box_abs_diff_max_px", "verified")}
    for k, v in detail.items():
        if k.startswith("value_") or k.startswith("latency_") or k in ("closed_loop_f16x3_frames_per_s", "closed_loop_f16x3_deferred_log_frames_per_s"):
            line[k] = _r(v)
    if "dist" in detail:
        d = detail["dist"]
        line["dist"] = {k: d[k] for k in ("world_size", "backend", "track_rows", "checksum_equal_on_all_ranks") if k in d}
    line["detail"] = DETAIL_FILE
    return line


def emit(detail: dict) -> str:
    """Writes the full object to DETAIL_FILE (next to this script, and under gpurun_out/ when that directory exists, so that it is carried back from a
    GPU box) and returns the compact final line; never larger than LINE_LIMIT (optional parts are dropped in a fixed order before that could happen)."""
    blob = json.dumps(detail, allow_nan=False)
    for d in (ROOT, os.path.join(ROOT, "gpurun_out")):
        if os.path.isdir(d):
            try:
                with open(os.path.join(d, DETAIL_FILE), "w") as f:
                    f.write(blob + "\n")
            except OSError:
                pass
    line = compact_line(detail)
    s = json.dumps(line, allow_nan=False)
    for k in ("headline_check", "dist", "parity", "windows"):
        if len(s) < LINE_LIMIT:
            break
        line.pop(k, None)
        s = json.dumps(line, allow_nan=False)
    assert len(s) < LINE_LIMIT, len(s)
    return s


def latency_leg(weights, scale: str, nc: int, device: int, conf: float) -> dict:
    """The reference's two detector calls per cycle — one batch of cycle_frame_num = 15 frames and ONE frame (yolo_controller.py:96-98,108-109), imgsz 384
    (initialize_experiment.ipynb cell 9) — and BASELINE config 2 (640 x 640, B = 1), on handles of max_batch 16 of three kinds: latency plan
    (wtk_yolo_create_planned: every conv on the split-K kernel), throughput plan (such a small handle runs its maps of <= 4 096 pixels — the 12 x 12 maps — on the
    split-K kernel and the under-filled window layers on 64-cout tiles) and the large-batch kernels alone (what every call ran on before round 5).  Per shape:
      device_ms  HIP events on the call's stream around 40 back-to-back calls / 40 (frames resident in HBM: what the device needs per call)
      host_ms    median wall time of one call + stream synchronisation seen from the host (launch / replay cost included, no PCIe traffic)
      pcie_ms    median of wtk_yolo_predict_host: upload of the frames, the call, download of the rows (what a host-frame controller call costs)."""
    from wtracker_amd import frames as fr
    from wtracker_amd import hip
    from wtracker_amd import yolo_spec as ys

    depth, width, maxch = ys.SCALES[scale]
    dev = torch.device("cuda", device)
    st = torch.cuda.Stream(device=dev)
    rows = []
    for dtype in ("f16x3", "fp32"):
        # "large_batch_kernels" = the throughput plan WITHOUT the rules of small handles (WTK_NO_SK_MIXED=1, WTK_SMALL_NARROW=0): what every call ran on before round 5
        for plan in ("latency", "throughput", "large_batch_kernels"):
            for size, B in ((384, 1), (384, 15), (640, 1)):
                prev = os.environ.get("WTK_NO_SK_MIXED")
                if plan == "large_batch_kernels":
                    os.environ["WTK_NO_SK_MIXED"] = "1"
                    os.environ["WTK_SMALL_NARROW"] = "0"
                # handle sizes as the controller makes them (controllers._YoloModel.detector): the latency-plan handle of plan "auto" holds 4 frames, the others 16
                det = hip.HipYolo(weights, (size, size), 4 if plan == "latency" and B <= 4 else 16, dtype=dtype, nc=nc, width=width, depth=depth, max_channels=maxch,
                                  device=device, plan="throughput" if plan == "large_batch_kernels" else plan)
                if plan == "large_batch_kernels":
                    os.environ.pop("WTK_NO_SK_MIXED") if prev is None else os.environ.__setitem__("WTK_NO_SK_MIXED", prev)
                    os.environ.pop("WTK_SMALL_NARROW", None)
                f_np = fr.diverse_frames(16, size, seed=4242)[:B]
                f = torch.from_numpy(f_np).to(dev)
                x = torch.empty((B, 4), dtype=torch.float32, device=dev)
                c = torch.empty((B,), dtype=torch.float32, device=dev)
                a = torch.empty((B,), dtype=torch.int32, device=dev)
                call = lambda: det.predict(f, B, size, size, 1, x, c, a, conf=conf, stream=st.cuda_stream)
                for _ in range(5):  # warm-up (eager launches since round 6; with WTK_GRAPH=1: eager, capture, replays)
                    call()
                st.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                n = 40
                e0.record(st)
                for _ in range(n):
                    call()
                e1.record(st)
                st.synchronize()
                device_ms = e0.elapsed_time(e1) / n
                host = []
                for _ in range(30):
                    t0 = time.perf_counter()
                    call()
                    st.synchronize()
                    host.append(time.perf_counter() - t0)
                pcie = []
                for _ in range(15):
                    t0 = time.perf_counter()
                    det.predict_host(f_np, conf=conf)
                    pcie.append(time.perf_counter() - t0)
                gflop = 2.0 * det.macs_per_frame * B / 1e9
                rows.append({"dtype": dtype, "plan": plan, "size": size, "batch": B, "device_ms": device_ms, "host_ms": float(np.median(host)) * 1e3,
                             "pcie_ms": float(np.median(pcie[3:])) * 1e3, "gflop": gflop, "achieved_tflops": gflop / device_ms, "frac_of_peak": gflop / device_ms / PEAK_TFLOPS[dtype]})
                det.close()
    return {"what": latency_leg.__doc__.split("Per shape:")[0].strip().replace("\n", " "), "rows": rows}


def step_outputs(pipe, s: int) -> dict:
    """What step s of the timed path handed its caller, as float32 host arrays (call after a fence: every row is final).  `xywh`: the track rows
    of the step's super-batch (NaN = no detection); `conf` / `anchor`: this rank's survivor confidence and anchor index (-1 = none); `moves` /
    `move_valid`: the raw ResMLP (dx, dy) and validity of the cycles whose prediction frame lies in the super-batch."""
    lanes = len(pipe.dets)
    lane = s % lanes
    k = (s // lanes) % max(int(getattr(pipe.dets[lane], "defer", 1)), 1)  # the lane's ring slot of step s (TrackPipeline._step_on_current_stream)
    f0, f1 = pipe.plan.super_range(s)
    lo, hi = pipe.plan.cycles(s)
    arrays = {"xywh": pipe.track[f0:f1], "conf": pipe.local_conf[lane][k], "anchor": pipe.local_anchor[lane][k], "moves": pipe.moves[lo:hi], "move_valid": pipe.valid[lo:hi]}
    return {name: a.float().cpu().numpy() for name, a in arrays.items()}


class Workload:
    """One precision mode of the benched workload on this rank: `lanes` detector handles, the ResMLP, the pipeline."""

    def __init__(self, args, dtype, lanes, weights, dims3, folded, local_rank, rank, world, group, dev, n_steps, streams=None):
        from wtracker_amd import hip
        from wtracker_amd.pipeline import TrackPipeline

        width, depth, maxch = dims3

        def handle(dt, max_batch):
            return hip.HipYolo(weights, (args.size, args.size), max_batch, dtype=dt, nc=1, width=width, depth=depth, max_channels=maxch, device=local_rank)

        if dtype == "hybrid":  # fp16 on every frame + the K weakest decisions of each batch again in f16x3, merged on the device
            from wtracker_amd.hybrid import HybridDetector

            q = args.hybrid_queue
            self.dets = [HybridDetector(handle("fp16", args.batch), handle("f16x3", q), margin=args.hybrid_margin, k=q, defer=args.defer) for _ in range(lanes)]
        else:
            self.dets = [handle(dtype, args.batch) for _ in range(lanes)]
        self.mlp = hip.HipMLP(folded.layers, folded.n_blocks, folded.layers_per_block, device=local_rank)
        # 60 fps, 100/40/50 ms timing (BASELINE config 3): imaging 6, pred 3, moving 3 frames
        self.pipe = TrackPipeline(self.dets, self.mlp, folded, args.batch, n_steps * args.batch * world, imaging_frame_num=6,
                                  pred_frame_num=3, cycle_frame_num=9, conf=args.conf, rank=rank, world=world, group=group, device=dev, streams=streams)
        self.dtype, self.lanes = dtype, lanes

    def close(self):
        for d in self.dets:
            d.close()
        self.mlp.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=1, help="timed windows of --steps steps each (median reported); the default 1 times exactly --steps steps")
    ap.add_argument("--full", action="store_true", help="also measure and check everything besides the headline: the other precision modes, the hybrid "
                    "calibration, the per-kernel roofline, headline_check, the CPU baseline with the parity of every mode, the closed-loop and latency legs")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the headline mode's last timed step computed to DIR/<name>.npy (float32)")
    ap.add_argument("--batch", type=int, default=64, help="frames per GPU per step (BASELINE config 3: 64)")
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--dtype", default="auto", choices=["auto", "fp16", "fp32", "f16x3", "hybrid"],
                    help="precision mode of the headline value; auto = the fastest reference-precision mode (f16x3, else fp32) whose survivors equal the fp32 "
                         "restatement's on every parity frame of this run and whose matched IoU is >= 0.999")
    ap.add_argument("--pool", type=int, default=128, help="distinct synthetic frames kept in HBM per rank")
    ap.add_argument("--cpu-frames", type=int, default=128, help="frames of the CPU-baseline / parity sample (0 = skip both)")
    ap.add_argument("--no-profile", action="store_true", help="skip the per-kernel HIP-event timing (no roofline object)")
    ap.add_argument("--no-fp32", action="store_true", help="measure the headline mode only (no per-mode sub-objects)")
    ap.add_argument("--no-hybrid", action="store_true", help="skip the hybrid sub-object (and its calibration pass)")
    ap.add_argument("--no-check", action="store_true", help="skip headline_check (profiling passes: nothing but the timed workload's kernels in the trace)")
    ap.add_argument("--legs-child", action="store_true", help=argparse.SUPPRESS)  # internal: run closed_loop / latency_leg and print them as one JSON line
    ap.add_argument("--no-latency", action="store_true", help="skip the latency sub-object (B = 1 / 15 at 384^2, B = 1 at 640^2: the reference's calls and BASELINE config 2)")
    ap.add_argument("--legs-subprocess", action="store_true", help="run the small-batch legs (closed_loop, latency) in a child process without GPU_MAX_HW_QUEUES (round 5's arrangement, kept for A/B: since round 6 the legs give the same device times in this process)")
    ap.add_argument("--no-closed-loop", action="store_true", help="skip the closed_loop sub-object (the reference's real operating point: 360 -> 384 views, 15-frame cycles)")
    ap.add_argument("--conf", type=float, default=0.1)
    ap.add_argument("--defer", type=int, default=HYBRID_DEFER, help="hybrid: batches of a lane whose weak rows share one full-precision pass (1 = second look inside every step)")
    ap.add_argument("--hybrid-queue", type=int, default=0, help="hybrid, deferred: rows of a lane's queue (0 = from the calibration: twice the measured weak share, at most defer x batch)")
    ap.add_argument("--hybrid-margin", type=float, default=0.0, help="hybrid: decision-margin threshold; 0 = calibrate it on this model inside the run")
    ap.add_argument("--lanes", type=int, default=2, help="forward passes in flight per GPU (each lane = own workspace + HIP stream)")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend for N>1 (nccl = RCCL; gloo only to rehearse the "
                    "multi-rank path on a one-GPU box, where every rank then shares cuda:0)")
    args = ap.parse_args()

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("bench.py --gpus N>1 must be launched with torch.distributed.run (one rank per GPU)")
        raise SystemExit(f"WORLD_SIZE={world} != --gpus {args.gpus}")

    from wtracker_amd import _build, hip, metrics, resmlp
    from wtracker_amd import frames as fr
    from wtracker_amd import yolo_spec as ys

    if args.legs_child:
        if not os.environ.get("WTK_HIP_LIB"):
            _build.ensure_built(verbose=False)
        w = ys.synthetic_weights("s", 1, seed=0)
        legs = {}
        if not args.no_closed_loop:
            legs["closed_loop"] = closed_loop(w, "s", 1, local_rank, args.conf)
        if not args.no_latency:
            legs["latency"] = latency_leg(w, "s", 1, local_rank, args.conf)
        print(json.dumps(_finite(legs), allow_nan=False), flush=True)
        return

    # The library is (re)built BEFORE any rendezvous, serialised over the ranks of the node by a file lock (_build.ensure_built): a
    # stale or missing .so is compiled by the first rank through the lock, a compiler error makes every rank exit non-zero, and
    # no rank can sit in a barrier waiting for a build that failed.  WTK_HIP_LIB (another build on purpose) skips the check.
    if not os.environ.get("WTK_HIP_LIB"):
        _build.ensure_built(verbose=False)
    if args.backend != "nccl" and torch.cuda.device_count() <= local_rank:
        local_rank = 0  # rehearsal: ranks share the one visible GPU
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(args.backend, rank=rank, world_size=world)
    if hip.device_count() <= local_rank:
        raise SystemExit("no HIP device visible: the product path has no CPU fallback")

    scale, nc = "s", 1
    weights = ys.synthetic_weights(scale, nc, seed=0)
    depth, width, maxch = ys.SCALES[scale]
    golden = os.path.join(ROOT, "tests", "golden", "resmlp_100ms.npz")
    folded = resmlp.load_npz(golden)  # ResMLP(imaging-100ms_pred-40ms_moving-50ms): the reference's shipped weights

    # synthetic frames, resident in HBM before the timed region; every rank draws its own seed
    pool = max(args.pool // args.batch, 1) * args.batch
    # frames of many seeded tracks (4 consecutive frames each): consecutive frames of ONE track are near-duplicates, which would give every frame of a batch
    # the same decision margin and make the hybrid mode's data-dependent second look meaningless; every other mode's work is independent of the pixel values
    frames_np = fr.diverse_frames(pool, args.size, seed=3000 + 1000 * rank)
    frames = torch.from_numpy(frames_np).to(dev)
    n_pool_batches = pool // args.batch

    lane_streams: dict = {}  # the same lane streams for every mode measured in this process

    def fence(pipe):
        pipe.synchronize()
        torch.cuda.synchronize(dev)
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize(dev)

    def measure(dtype: str, lanes: int, repeats: int, profile: bool) -> dict:
        """Warm-up, `repeats` timed windows of args.steps steps, then (optionally) the per-kernel profile pass."""
        prof_steps = max(min(args.steps, 10), 1) if profile else 0
        n_steps = args.warmup + repeats * args.steps + 2 * prof_steps + lanes
        wl = Workload(args, dtype, lanes, weights, (width, depth, maxch), folded, local_rank, rank, world, None, dev, n_steps,
                      streams=lane_streams.setdefault(lanes, [torch.cuda.Stream(device=dev) for _ in range(lanes)]) if lanes > 1 else None)
        pipe = wl.pipe

        def run(s: int):
            b = s % n_pool_batches
            pipe.step(s, frames[b * args.batch : (b + 1) * args.batch])

        s = 0
        for _ in range(args.warmup):
            run(s)
            s += 1
        fence(pipe)
        win = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            for _ in range(args.steps):
                run(s)
                s += 1
            fence(pipe)
            win.append(time.perf_counter() - t0)
        outputs = step_outputs(pipe, s - 1) if args.dump_outputs and rank == 0 else None  # before the profile pass below reuses the buffers
        if world > 1:
            t = torch.tensor(win, dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)  # a window ends when the slowest rank is done
            win = [float(v) for v in t.cpu()]
        med = float(np.median(win))
        frames_per_window = args.steps * args.batch * world
        gflop_frame = 2.0 * wl.dets[0].macs_per_frame / 1e9  # conv MACs only (28.432 GFLOP at 640x640)
        res = {"dtype": dtype, "value": frames_per_window / med, "unit": "frames/s", "ms_per_step": med / args.steps * 1e3,
               # whole-job arithmetic rate of the timed windows against the mode's matrix peak (per GPU): what `value` is made of
               "end_to_end": {"gflop_per_frame": gflop_frame, "achieved_tflops_per_gpu": frames_per_window / world * gflop_frame / med / 1e3,
                              "peak": PEAK_TFLOPS[dtype], "frac": frames_per_window / world * gflop_frame / med / 1e3 / PEAK_TFLOPS[dtype]},
               "windows": {"n": repeats, "steps_each": args.steps, "median_ms": med * 1e3, "min_ms": min(win) * 1e3, "max_ms": max(win) * 1e3,
                           "first_ms": win[0] * 1e3, "value_best": frames_per_window / min(win), "value_worst": frames_per_window / max(win)}}
        if outputs is not None:
            res["outputs"] = outputs
        if profile:
            # per-kernel device time with HIP events on the launch stream: one stream, one event pair around every run of launches
            # of the same kernel (wtk_yolo_get_kernel_profile); lane 0's handle is the profiled one
            det = wl.dets[0]
            s = (s + lanes - 1) // lanes * lanes
            det.set_profiling(True)
            for i in range(prof_steps):
                run(s + i * lanes)  # steps congruent to 0 mod lanes run on lane 0
            fence(pipe)
            res["roofline"] = roofline_object(det.get_profile(), det.get_kernel_profile(), prof_steps, dtype)
            res["roofline"]["end_to_end_frac"] = res["end_to_end"]["frac"]
            det.set_profiling(False)
        if dtype == "hybrid":  # how many rows the second look replaced (device counters, read after the last window)
            n_rep = sum(int(d.replaced.item()) for d in wl.dets)
            res["second_look"] = {"rows_replaced": n_rep, "of_frames": s * args.batch, "share": n_rep / max(s * args.batch, 1),
                                  "ceiling_per_batch": wl.dets[0].k, "margin": wl.dets[0].margin,
                                  "overflow_rows": sum(d.overflow_count() for d in wl.dets)}  # weak rows WITHOUT a second look: 0 by construction at K = B
        if world > 1:  # evidence that the collective saw N ranks: a checksum of the gathered track, equal on every rank
            tr = torch.nan_to_num(pipe.track[: s * args.batch * world].double(), nan=-1.0)
            cs = torch.stack([tr.sum(), (tr * torch.arange(1, tr.shape[0] + 1, device=dev, dtype=torch.float64)[:, None]).sum()])
            lo, hi = cs.clone(), cs.clone()
            dist.all_reduce(lo, op=dist.ReduceOp.MIN)
            dist.all_reduce(hi, op=dist.ReduceOp.MAX)
            res["dist"] = {"world_size": dist.get_world_size(), "backend": dist.get_backend(), "track_rows": int(tr.shape[0]),
                           "track_checksum": [float(v) for v in cs.cpu()], "checksum_equal_on_all_ranks": bool(torch.equal(lo, hi))}
        wl.close()
        return res

    def committed(name: str):
        """profiles/<round>_<name>.json if it was collected on exactly the kernel sources of this build, else None."""
        path = os.path.join(ROOT, "profiles", f"{PROFILE_ROUND}_{name}.json")
        if not os.path.exists(path) or args.size != 640 or args.batch != 64:
            return None, None
        j = json.load(open(path))
        if j.get("src_sha") != _build.source_sha():
            return None, None
        return j, {"file": os.path.relpath(path, ROOT), "src_sha": j["src_sha"], "collected": j.get("collected", "rocprofv3 --pmc, separate passes"),
                   "note": "not measured in this run; valid for these kernel sources only"}

    def roofline_object(prof: dict, kprof: dict, prof_steps: int, dtype: str) -> dict:
        peak = PEAK_TFLOPS[dtype]
        # (hybrid: the profiled handle is its fp16 one — the same kernels on the same shapes as the plain fp16 mode; fp32: no PMC pass committed)
        sfx = PMC_SUFFIX.get(dtype)
        tj, tprov = committed("conv_traffic" + sfx) if sfx is not None else (None, None)
        uj, uprov = committed("pmc_mfma_util" + sfx) if sfx is not None else (None, None)

        def kernel_line(name, k):
            avg_ms = k["total_ms"] / max(k["launches"], 1)
            flop_per_launch = k["flops"] / max(k["launches"], 1)
            ach = flop_per_launch / (avg_ms * 1e-3) / 1e12 if avg_ms > 0 else 0.0
            tr = tj["per_kernel"][name]["hbm_bytes_per_launch_avg"] if tj and name in tj.get("per_kernel", {}) else None
            e = {"kernel": name, "achieved": ach, "frac": ach / peak, "traffic": tr, "launches_per_step": k["launches"] / prof_steps,
                 "avg_launch_ms": avg_ms, "flop_per_launch_avg": flop_per_launch, "ms_per_step": k["total_ms"] / prof_steps}
            if tr is not None and avg_ms > 0:  # HBM side of the same kernel: PMC bytes per launch / live launch duration
                e["hbm_gbps"] = tr / (avg_ms * 1e-3) / 1e9
                e["hbm_frac"] = e["hbm_gbps"] / HBM_PEAK_GBPS
            if uj and name in uj["per_kernel"]:  # MFMA-busy share (executed MFMAs, 2.4 GHz nominal)
                e["mfma_util_pmc"] = uj["per_kernel"][name]["mfma_util"]
            return e

        conv_kernels = {n: k for n, k in kprof.items() if k["flops"] > 0 and k["launches"] > 0}
        lines = sorted((kernel_line(n, k) for n, k in conv_kernels.items()), key=lambda e: -e["ms_per_step"])
        dom = lines[0]  # the kernel the forward pass spends most of its device time in
        fam_ms = sum(k["total_ms"] for k in conv_kernels.values())
        fam_launches = sum(k["launches"] for k in conv_kernels.values())
        fam_flops = sum(k["flops"] for k in conv_kernels.values())
        fam_ach = fam_flops / (fam_ms * 1e-3) / 1e12
        prov = {}
        if tprov:
            prov["traffic, hbm_gbps, hbm_frac"] = tprov
        if uprov:
            prov["mfma_util_pmc"] = uprov
        return {"kernel": dom["kernel"], "bound": "mfma", "achieved": dom["achieved"], "peak": peak, "peak_basis": PEAK_BASIS[dtype], "unit": "TFLOP/s", "frac": dom["frac"],
                # the same algorithmic rate against the hardware's dense fp16 peak (fp32 mode: against its own matrix peak, there is no fp16 in it)
                "frac_of_fp16_peak": dom["achieved"] / PEAK_TFLOPS["fp16"] if dtype != "fp32" else None,
                "traffic": dom["traffic"], "hbm_gbps": dom.get("hbm_gbps"), "hbm_frac": dom.get("hbm_frac"), "mfma_util_pmc": dom.get("mfma_util_pmc"),
                "launches_per_step": dom["launches_per_step"], "avg_launch_ms": dom["avg_launch_ms"], "flop_per_launch_avg": dom["flop_per_launch_avg"],
                "share_of_forward": dom["ms_per_step"] / sum(v["total_ms"] / prof_steps for v in prof.values()),
                "timing": f"HIP events on the launch stream, {prof_steps} single-stream forwards of this run",
                # every MFMA kernel of the forward pass together (what `value` is made of)
                "conv_family": {"achieved": fam_ach, "frac": fam_ach / peak, "launches_per_step": fam_launches / prof_steps,
                                "avg_launch_ms": fam_ms / fam_launches, "flop_per_launch_avg": fam_flops / fam_launches,
                                "traffic": tj["hbm_bytes_per_launch_avg"] if tj else None},
                "kernels": lines, "class_ms_per_step": {k: v["total_ms"] / prof_steps for k, v in prof.items()},
                "provenance": prov or None}

    # A plain run measures the headline mode and nothing else; --full adds every other figure and check of the line
    profile = args.full and not args.no_profile
    modes: dict = {}
    calibration = None
    want_hybrid = args.dtype == "hybrid" or (args.full and args.dtype == "auto" and world == 1 and not args.no_fp32 and not args.no_hybrid)
    if args.hybrid_margin <= 0.0:
        if want_hybrid:
            from wtracker_amd.hybrid import HybridDetector

            mkc = lambda dt: hip.HipYolo(weights, (args.size, args.size), 64, dtype=dt, nc=nc, width=width, depth=depth, max_channels=maxch, device=local_rank)
            cal = HybridDetector(mkc("fp16"), mkc("f16x3"), margin=HYBRID_MARGIN_FALLBACK, k=64)
            cal_frames = torch.from_numpy(fr.diverse_frames(HYBRID_CAL_FRAMES, args.size, seed=HYBRID_CAL_SEED + 1000 * rank)).to(dev)
            calibration = cal.calibrate((cal_frames[i : i + 64] for i in range(0, len(cal_frames), 64)), args.size, args.size, 1, conf=args.conf)
            calibration["frames_seed"] = HYBRID_CAL_SEED + 1000 * rank
            args.hybrid_margin = calibration["margin"]
            cal.close()
            del cal_frames
            if world > 1:  # every rank uses the widest margin any rank measured
                t = torch.tensor([args.hybrid_margin], dtype=torch.float64, device=dev)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                args.hybrid_margin = float(t.item())
        else:
            args.hybrid_margin = HYBRID_MARGIN_FALLBACK
    if args.hybrid_queue <= 0:
        # a lane's queue receives the weak rows of `defer` batches: twice the share measured on the calibration frames (+ 10 %), never more than all of them —
        # and never more frames than HYBRID_EXACT_MEM_GB of f16x3 workspace hold (107 MB of activations per 640x640 frame, per lane): at 1280x1280 / B = 256 that
        # is ~110 rows, so the number of batches that share a pass shrinks with it (down to the immediate form, ceiling = what fits; overflow is counted)
        share = calibration["share_below_margin"] if calibration is not None else HYBRID_QUEUE_PER_64 / (64.0 * HYBRID_DEFER)
        per_batch = args.batch * min(1.0, 2.0 * share + 0.1)
        fits = max(int(HYBRID_EXACT_MEM_GB * 1e9 / (107e6 * (args.size / 640.0) ** 2)), 1)
        if args.defer > 1 and fits < 2 * per_batch:
            args.defer = 1
        if args.defer > 1:
            args.defer = int(max(2, min(args.defer, fits // max(per_batch, 1))))
            args.hybrid_queue = int(min(args.defer * args.batch, fits, max(args.batch // 2, np.ceil(args.defer * per_batch))))
        else:
            args.hybrid_queue = int(min(args.batch, fits))
    # the mode measured first, with all windows: the requested one, else the first reference-precision candidate (the SAME mode at every N)
    first_dtype = args.dtype if args.dtype != "auto" else HEADLINE_CANDIDATES[0]
    modes[first_dtype] = measure(first_dtype, args.lanes, args.repeats, profile)
    if args.full and world == 1 and not args.no_fp32:
        # every other mode of the same workload, in the same command (fewer windows where a window is long)
        for dt, rep in (("f16x3", max(min(args.repeats, 5), 1)), ("fp16", args.repeats), ("hybrid", max(min(args.repeats, 5), 1)), ("fp32", max(min(args.repeats, 3), 1))):
            if dt not in modes and (dt != "hybrid" or want_hybrid):
                modes[dt] = measure(dt, args.lanes, rep, profile)

    mk = lambda dt, mb: hip.HipYolo(weights, (args.size, args.size), mb, dtype=dt, nc=nc, width=width, depth=depth, max_channels=maxch, device=local_rank)

    def device_check(dt: str) -> dict:
        """Evidence for the headline mode that needs no CPU: its rows against the fp32 mode's (exact-fp32 MFMA: the reference's literal arithmetic) on the
        frames of the TIMED pool of this rank; index mismatches are summed over the ranks, the largest box difference is the maximum over them."""
        m = (len(frames) // 64) * 64
        rows = {}
        for d in (dt, "fp32"):
            if d == "hybrid":  # the look-twice object on the run's margin (immediate form: rows are final when the call returns)
                from wtracker_amd.hybrid import HybridDetector

                det = HybridDetector(mk("fp16", 64), mk("f16x3", 64), margin=args.hybrid_margin, k=64)
            else:
                det = mk(d, 64)
            x, c, a = (torch.empty((m, 4), dtype=torch.float32, device=dev), torch.empty((m,), dtype=torch.float32, device=dev),
                       torch.empty((m,), dtype=torch.int32, device=dev))
            for i in range(0, m, 64):
                det.predict(frames[i : i + 64], 64, args.size, args.size, 1, x[i : i + 64], c[i : i + 64], a[i : i + 64], conf=args.conf)
            torch.cuda.synchronize(dev)
            det.close()
            rows[d] = (x, a)
        same = rows[dt][1] == rows["fp32"][1]
        both = same & (rows["fp32"][1] >= 0)
        dbox = (rows[dt][0][both] - rows["fp32"][0][both]).abs().max() if bool(both.any()) else torch.zeros((), device=dev)
        t = torch.stack([(~same).sum().double(), torch.tensor(float(m), device=dev, dtype=torch.float64)])
        dmax = dbox.double().reshape(1)
        if world > 1:
            dist.all_reduce(t, op=dist.ReduceOp.SUM)
            dist.all_reduce(dmax, op=dist.ReduceOp.MAX)
        return {"against": "fp32 mode on the device (v_mfma_f32_16x16x4_f32: the reference's arithmetic, yolo_train_config.yaml:51), frames of the timed pool, every rank",
                "frames": int(t[1].item()), "index_mismatches": int(t[0].item()), "box_abs_diff_max_px": float(dmax.item()),
                "verified": bool(t[0].item() == 0 and dmax.item() <= 2e-2)}

    par = None
    cpu_obj = None
    if args.full and world == 1 and args.cpu_frames > 0:
        # ---- CPU baseline (oracle, kind 'port') + parity of every mode against it on the same frames, outside any timed region
        n = max(args.cpu_frames // 64, 1) * 64
        sample = fr.diverse_frames(n, args.size, seed=2000)
        cpu_obj, (xo, co, ao) = cpu_baseline(weights, ys.model_dims(width, depth, maxch, nc), args.size, golden, sample, args.conf)
        par = {"checker": "oracle/yolo_oracle.py (fp32 torch-CPU restatement; parity unpinned: no ultralytics, no trained weights)",
               "frames": f"{n} synthetic {args.size}x{args.size} frames from {n // 4} seeded tracks, conf {args.conf}",
               "headline_gate": f"index_match_rate == 1.0 and iou_matched.min >= {HEADLINE_IOU_MIN} (BASELINE.md section 4)",
               "floors_asserted_in_tests": "tests/test_gpu_configs.py: fp32 / f16x3 index match == 1 and boxes within 2e-2 px; fp16 index match >= 0.96, matched IoU min >= 0.99 (256 frames); "
                                           "hybrid index match == 1, boxes within 1 px; tests/test_gpu_hybrid_validation.py: hybrid == f16x3 survivors on 2 048 out-of-sample frames x 3 weight seeds, overflow 0"}
        for dtype in ("fp16", "fp32", "f16x3"):
            det = mk(dtype, 64)
            res = [det.predict_host(sample[i : i + 64], conf=args.conf) for i in range(0, n, 64)]
            det.close()
            xg, cg, ag = (np.concatenate([r[k] for r in res]) for k in range(3))
            par[dtype] = metrics.accuracy_report(xg, ag, xo, ao, cg, co)
        if want_hybrid:
            from wtracker_amd.hybrid import HybridDetector

            kq = min(64, args.hybrid_queue if args.defer <= 1 else 64)
            hyb = HybridDetector(mk("fp16", 64), mk("f16x3", kq), margin=args.hybrid_margin, k=kq)
            sdev = torch.from_numpy(sample).to(dev)
            ox, oc, oa = (torch.empty((n, 4), dtype=torch.float32, device=dev), torch.empty((n,), dtype=torch.float32, device=dev),
                          torch.empty((n,), dtype=torch.int32, device=dev))
            for i in range(0, n, 64):
                hyb.predict(sdev[i : i + 64], 64, args.size, args.size, 1, ox[i : i + 64], oc[i : i + 64], oa[i : i + 64], conf=args.conf)
            torch.cuda.synchronize(dev)
            par["hybrid"] = metrics.accuracy_report(ox.cpu().numpy(), oa.cpu().numpy(), xo, ao, oc.cpu().numpy(), co)
            par["hybrid"]["rows_replaced"] = int(hyb.replaced.item())
            par["hybrid"]["overflow_rows"] = hyb.overflow_count()
            # more out-of-sample evidence inside the run (device only, no CPU restatement needed): the hybrid against the f16x3 mode on the frames of the
            # TIMED pool, which neither the calibration nor the CPU leg has seen — every survivor must be f16x3's
            det3 = mk("f16x3", 64)
            m_pool = (len(frames) // 64) * 64
            px, pc, pa = (torch.empty((m_pool, 4), dtype=torch.float32, device=dev), torch.empty((m_pool,), dtype=torch.float32, device=dev),
                          torch.empty((m_pool,), dtype=torch.int32, device=dev))
            hx, hc, ha = torch.empty_like(px), torch.empty_like(pc), torch.empty_like(pa)
            for i in range(0, m_pool, 64):
                det3.predict(frames[i : i + 64], 64, args.size, args.size, 1, px[i : i + 64], pc[i : i + 64], pa[i : i + 64], conf=args.conf)
                hyb.predict(frames[i : i + 64], 64, args.size, args.size, 1, hx[i : i + 64], hc[i : i + 64], ha[i : i + 64], conf=args.conf)
            torch.cuda.synchronize(dev)
            par["hybrid"]["vs_f16x3_on_timed_pool"] = {"frames": int(m_pool), "index_match": int((pa == ha).sum().item()),
                                                      "index_match_rate": float((pa == ha).float().mean().item()), "overflow_rows": hyb.overflow_count()}
            det3.close()
            hyb.close()

    def exact(dt: str) -> bool:
        """The mode returned the fp32 restatement's survivor on EVERY parity frame of this run and its boxes pass the stated gate."""
        if par is None or dt not in par or par[dt]["index_match_rate"] != 1.0:
            return False
        iou = par[dt].get("iou_matched")
        return iou is None or iou["min"] >= HEADLINE_IOU_MIN  # (None: no frame with a detection on both sides)

    if args.dtype != "auto":
        head_dtype, head_reason = args.dtype, "requested with --dtype"
    else:
        head_dtype = next((dt for dt in HEADLINE_CANDIDATES if dt in modes and exact(dt)), None)
        head_reason = f"fastest reference-precision mode with parity.index_match_rate == 1.0 and iou_matched.min >= {HEADLINE_IOU_MIN} on this run's parity frames"
        if head_dtype is None:  # no CPU parity leg in this run (N > 1, --cpu-frames 0) or no candidate passed it: the first candidate, and say what was verified
            head_dtype = first_dtype
            if not args.full:
                head_reason = "plain run: the reference-precision mode f16x3, whose exactness a --full run checks (parity, headline_check)"
            elif par is None:
                head_reason = "no CPU parity leg in this run (N > 1 or --cpu-frames 0): the reference-precision mode f16x3; see headline_check for the device-side evidence"
            else:
                head_reason = "NO candidate passed the parity gate of this run: f16x3 reported, exactness NOT established"
    head = modes[head_dtype]
    head_check = device_check(head_dtype) if args.full and head_dtype in ("f16x3", "hybrid", "fp16") and not args.no_check else None
    if par is not None and head_dtype in par:
        verified = exact(head_dtype) and (head_check is None or head_check["verified"])
    elif not args.full and head_dtype != "fp32":  # plain run: nothing was checked (null, not false)
        verified = None
    else:  # no CPU leg: the device-side check alone (fp32 IS the reference's arithmetic; --no-check: nothing was verified)
        verified = bool(head_check and head_check["verified"]) if head_dtype != "fp32" else True
    if head.get("outputs") is not None:
        os.makedirs(args.dump_outputs, exist_ok=True)
        for name, a in head["outputs"].items():
            np.save(os.path.join(args.dump_outputs, f"{name}.npy"), a)

    # The two small-batch legs run in THIS process since round 6 (round 5 needed a child process: its replayed captures forked into side streams and ran 2-4 x slower
    # here, where eight hardware queues are requested and a dozen handles have come and gone).  Handles of <= 16 frames now run on the caller's stream alone, eagerly:
    # same device times in either process (0.512 / 0.510 ms single frame, 1.132 / 1.134 ms cycle batch; profiles/r06_notes.md section 4); --legs-subprocess is the A/B.
    closed = lat = None
    want_closed = args.full and world == 1 and not args.no_closed_loop and not args.no_fp32
    want_lat = args.full and world == 1 and not args.no_latency and not args.no_fp32 and args.size == 640
    if (want_closed or want_lat) and not args.legs_subprocess:
        if want_closed:
            closed = closed_loop(weights, "s", 1, local_rank, args.conf)
        if want_lat:
            lat = latency_leg(weights, "s", 1, local_rank, args.conf)
    elif want_closed or want_lat:
        import subprocess

        env = {k: v for k, v in os.environ.items() if k != "GPU_MAX_HW_QUEUES"}
        cmd = [sys.executable, os.path.abspath(__file__), "--legs-child", "--conf", str(args.conf)] + ([] if want_closed else ["--no-closed-loop"]) + ([] if want_lat else ["--no-latency"])
        try:
            r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
            legs = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]) if r.returncode == 0 else {"error": r.stderr[-800:]}
        except Exception as e:  # the headline must not depend on a side leg
            legs = {"error": repr(e)}
        closed, lat = legs.get("closed_loop"), legs.get("latency")
        if "error" in legs:
            closed = {"error": legs["error"]}

    out = {
        "metric": f"frames/sec YOLOv8s+ResMLP sim loop @{args.size}x{args.size}",
        "value": head["value"],
        "unit": "frames/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": head["ms_per_step"],
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": head_dtype,
        "data": "synthetic",
        "config": {"workload": ("BASELINE configs[2]" if args.size == 640 else f"BASELINE configs[4] per-GPU shape ({args.size}x{args.size})")
                               + ": full sim loop, YOLOv8s (nc=1, seeded synthetic weights) + ResMLP(imaging-100ms_pred-40ms_moving-50ms, reference weights)",
                   "frame": f"{args.size}x{args.size} uint8 gray, resident in HBM", "batch_per_gpu": args.batch, "lanes_per_gpu": args.lanes,
                   "global_batch": args.batch * world, "timing_ms": [100, 40, 50], "conf": args.conf,
                   "headline_mode": head_dtype, "headline_reason": head_reason,
                   "parallelism": f"frame-sharded x{world}, one RCCL all-gather of [B,4] tracks per step" if world > 1 else "single GPU"},
        "windows": head["windows"],
        "roofline": head.get("roofline"),
    }
    if "dist" in head:
        out["dist"] = head["dist"]
    # Was the exactness of the headline mode established IN THIS RUN?  N = 1: the CPU parity leg (index match == 1 and the IoU gate) and the device-side check;
    # N > 1 (no CPU leg): the device-side check alone — f16x3 rows against the fp32 mode's on every rank's timed pool
    out["headline_exactness_verified"] = verified
    out["headline_check"] = head_check
    out["end_to_end"] = head["end_to_end"]
    if closed is not None:
        out["closed_loop"] = closed
        if "f16x3_auto" in closed:
            out["closed_loop_f16x3_frames_per_s"] = closed["f16x3_auto"]["frames_per_s"]
        if "f16x3_auto_deferred_log" in closed:
            out["closed_loop_f16x3_deferred_log_frames_per_s"] = closed["f16x3_auto_deferred_log"]["frames_per_s"]
    if lat is not None:
        out["latency"] = lat
        # two scalars per reference-precision mode in the main line: the reference's two calls, each on the plan the controller's default ("auto":
        # controllers._YoloModel.detector) gives it — the single frame on a latency-plan handle, the cycle batch on a small throughput-plan handle
        for r in lat["rows"]:
            if r["plan"] == ("latency" if r["batch"] <= 4 else "throughput"):  # 384: the reference's imgsz; 640, B = 1: BASELINE configs[1]
                out[f"latency_b{r['batch']}_{r['size']}_{r['dtype']}_ms"] = r["device_ms"]
        lat["main_line"] = ("latency_b1_* = the latency-plan row, latency_b15_* = the throughput-plan row (the plan YoloConfig.plan = 'auto' picks per call); "
                            "latency_b1_640_* = BASELINE configs[1] (YoloController, 640 x 640, batch 1)")
    # flat per-mode keys (a record that keeps only top-level scalars still carries every mode and its exactness)
    for dt, m in modes.items():
        out[f"value_{dt}"] = m["value"]
        out[f"ms_per_step_{dt}"] = m["ms_per_step"]
        out[f"end_to_end_frac_{dt}"] = m["end_to_end"]["frac"]
        if m.get("roofline"):
            out[f"roofline_frac_{dt}"] = m["roofline"]["frac"]
    if par is not None:
        for dt in ("fp16", "hybrid", "f16x3", "fp32"):
            if dt in par:
                out[f"parity_index_match_{dt}"] = par[dt]["index_match_rate"]
                if par[dt].get("iou_matched"):
                    out[f"parity_iou_matched_min_{dt}"] = par[dt]["iou_matched"]["min"]
    if "hybrid" in modes:
        out["hybrid_overflow"] = modes["hybrid"]["second_look"]["overflow_rows"] + (par["hybrid"]["overflow_rows"] if par and "hybrid" in par else 0)
        out["hybrid_second_look_share"] = modes["hybrid"]["second_look"]["share"]
        if par and "hybrid" in par and "vs_f16x3_on_timed_pool" in par["hybrid"]:
            out["hybrid_vs_f16x3_pool_index_match"] = par["hybrid"]["vs_f16x3_on_timed_pool"]["index_match_rate"]
        out["hybrid_margin"] = args.hybrid_margin
        out["hybrid_defer"] = args.defer  # movement vectors of a held step come up to defer x lanes super-batches after its frames (TrackPipeline.step)
        out["hybrid_queue"] = args.hybrid_queue
        if calibration is not None:
            out["hybrid_calibration"] = calibration
    notes = {
        "fp16": "plain fp16 mode (throughput only): its survivor differs from the fp32 restatement's on ~2 % of the frames, so it is not the headline",
        "hybrid": ("NOT a headline mode: rows that take no second look are fp16 rows (tolerance: survivor index equal by a margin calibrated to 6 sigma — a statistical guarantee —, "
                   "matched IoU >= 0.98, boxes within 1 px; tests/test_gpu_hybrid_validation.py).  "
                   f"wtracker_amd.hybrid.HybridDetector: fp16 on every frame, then EVERY frame whose decision margin is below {args.hybrid_margin:.4f} (calibrated on this model in this "
                   f"run) again through an f16x3 handle — the weak rows of {args.defer} batches of a lane share one pass (device-side queue, dynamic batch: the cost follows the "
                   "number of weak frames), rows written back on the device; fixed launch sequence, no host round trip; overflow of the queue is counted and must be 0"),
        "f16x3": ("split-fp16 storage and three v_mfma_f32_16x16x32_f16 per product: every conv tensor within 4e-6 of the exact-fp32 "
                  "mode's (tests/test_gpu_f16x3.py), survivor indices equal the fp32 restatement's; roofline peak = fp16 peak / 3"),
        "fp32": "reference precision (ultralytics half: False): exact-fp32 v_mfma_f32_16x16x4_f32 through the same kernels",
    }
    for dt, m in modes.items():
        key = "fp16_throughput" if dt == "fp16" else dt
        out[key] = {k: m[k] for k in ("dtype", "value", "unit", "ms_per_step", "windows", "second_look", "end_to_end", "roofline") if k in m}
        out[key]["note"] = notes[dt]
    if cpu_obj is not None:
        out["cpu_baseline"] = cpu_obj
        out["parity"] = par
    if rank == 0:
        print(emit(_finite(out)), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
