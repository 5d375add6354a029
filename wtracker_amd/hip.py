"""ctypes binding of libwtk_hip.so — the C ABI declared in include/wtk_hip.h.

There is NO CPU fallback: if the shared library is missing or a GPU is not visible the calls
raise.  (The oracle under oracle/ is test infrastructure and is never imported from here.)
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

# WTK_HIP_LIB: load another build of the same library instead (A/B timing of two builds in one GPU session)
_LIB_PATH = os.environ.get("WTK_HIP_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libwtk_hip.so")
_lib: Optional[C.CDLL] = None

WTK_F32 = 0
WTK_F16 = 1
WTK_F16X3 = 2
DTYPES = {"fp32": WTK_F32, "f32": WTK_F32, "float32": WTK_F32, "fp16": WTK_F16, "f16": WTK_F16, "float16": WTK_F16, "f16x3": WTK_F16X3, "fp16x3": WTK_F16X3}


class WtkError(RuntimeError):
    pass


class _MlpLayer(C.Structure):
    _fields_ = [("in_dim", C.c_int32), ("out_dim", C.c_int32), ("relu", C.c_int32), ("reserved", C.c_int32),
                ("weight", C.POINTER(C.c_float)), ("bias", C.POINTER(C.c_float))]


class _MlpDesc(C.Structure):
    _fields_ = [("device", C.c_int32), ("n_layers", C.c_int32), ("n_blocks", C.c_int32), ("layers_per_block", C.c_int32),
                ("layers", C.POINTER(_MlpLayer))]


class _MlpTrainLayer(C.Structure):
    _fields_ = [("in_dim", C.c_int32), ("out_dim", C.c_int32), ("relu", C.c_int32), ("batch_norm", C.c_int32)]


class _MlpTrainerDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("device", "n_models", "n_layers", "n_blocks", "layers_per_block", "loss", "optimizer", "max_batch")] + [
        ("layers", C.POINTER(_MlpTrainLayer)), ("state", C.POINTER(C.c_float))]


class _ConvBlob(C.Structure):
    _fields_ = [("cout", C.c_int32), ("cin", C.c_int32), ("k", C.c_int32), ("stride", C.c_int32), ("act", C.c_int32),
                ("reserved", C.c_int32), ("weight", C.POINTER(C.c_float)), ("bias", C.POINTER(C.c_float))]


class _ReplayConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("num_frames", "imaging_frame_num", "moving_frame_num", "pred_frame_num", "cam_w", "cam_h", "mic_w", "mic_h",
                                         "frame_w", "frame_h", "init_x", "init_y")]


class _ReplaySetTrack(C.Structure):
    _fields_ = [("R", C.c_int64)] + [(n, C.c_int32) for n in ("cyc_off", "n_track", "num_frames", "n_cycles", "n_log", "x_max", "y_max", "init_x", "init_y",
                                                              "chunk0")]


class _ReplaySetFrames(C.Structure):
    _fields_ = [("frames", C.c_void_p), ("bg", C.c_void_p), ("diff_thresh", C.c_double), ("row0", C.c_int64), ("n_frames", C.c_int32), ("H", C.c_int32),
                ("W", C.c_int32), ("reserved", C.c_int32)]


class _ReplaySetGeometry(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("cam_w", "cam_h", "mic_w", "mic_h")] + [(n, C.c_double) for n in ("time_factor", "dist_factor", "speed_factor")]


class _AnalysisConfig(C.Structure):
    _fields_ = ([("bounds", C.c_double * 4)] + [(n, C.c_double) for n in ("time_factor", "dist_factor", "speed_factor", "min_speed", "min_bbox_error",
                                                                          "min_dist_error", "min_width", "min_height")]
                + [(n, C.c_int32) for n in ("period", "imaging_only", "use_bounds", "trim_cycles", "no_preds", "reserved")])


class _YoloDesc(C.Structure):
    _fields_ = [("device", C.c_int32), ("dtype", C.c_int32), ("imgsz_h", C.c_int32), ("imgsz_w", C.c_int32),
                ("max_batch", C.c_int32), ("nc", C.c_int32), ("width_mult", C.c_float), ("depth_mult", C.c_float),
                ("max_channels", C.c_int32), ("n_convs", C.c_int32), ("convs", C.POINTER(_ConvBlob))]


_vp, _i32, _i64, _f32, _f64, _size = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_double, C.c_size_t
_pvp, _pi32, _pi64, _pf32, _pf64, _pcfg = C.POINTER(_vp), C.POINTER(_i32), C.POINTER(_i64), C.POINTER(_f32), C.POINTER(_f64), C.POINTER(_ReplayConfig)
_pacfg = C.POINTER(_AnalysisConfig)
_ptrk = C.POINTER(_ReplaySetTrack)
_pfrm = C.POINTER(_ReplaySetFrames)
_pgeo = C.POINTER(_ReplaySetGeometry)

# The C ABI, one row per symbol of include/wtk_hip.h and in its order: name -> (restype, argtypes).  load() applies it and nothing else declares a
# signature; tests/test_abi.py compares every row with the header's prototype, kind by kind (pointer, int32, int64, size_t, float, double).
SIGNATURES = {
    "wtk_last_error": (C.c_char_p, []),
    "wtk_abi_version": (_i32, []),
    "wtk_device_count": (_i32, []),
    "wtk_mlp_create": (_i32, [_pvp, C.POINTER(_MlpDesc)]),
    "wtk_mlp_destroy": (None, [_vp]),
    "wtk_mlp_forward": (_i32, [_vp, _vp, _i32, _vp, _vp]),
    "wtk_mlp_forward_host": (_i32, [_vp, _vp, _i32, _vp]),
    "wtk_mlp_predict_track": (_i32, [_vp, _vp, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _vp]),
    "wtk_mlp_trainer_state_floats": (_i64, [C.POINTER(_MlpTrainerDesc), _pi64]),
    "wtk_mlp_trainer_create": (_i32, [_pvp, C.POINTER(_MlpTrainerDesc)]),
    "wtk_mlp_trainer_destroy": (None, [_vp]),
    "wtk_mlp_trainer_grad": (_i32, [_vp, _vp, _vp, _i32, _vp, _vp, _vp]),
    "wtk_mlp_trainer_step": (_i32, [_vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "wtk_mlp_trainer_train_epoch": (_i32, [_vp, _vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "wtk_mlp_trainer_eval_epoch": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "wtk_mlp_trainer_get_state": (_i32, [_vp, _i32, _vp, _vp, _vp]),
    "wtk_mlp_trainer_get_stopping": (_i32, [_vp, _vp, _vp, _vp, _vp]),
    "wtk_mlp_folded_floats": (_i64, [C.POINTER(_MlpTrainLayer), _i32, _i32, _i32]),
    "wtk_mlp_fold_state_host": (_i32, [C.POINTER(_MlpTrainLayer), _i32, _i32, _i32, _vp, _vp]),
    "wtk_mlp_trainer_fold": (_i32, [_vp, _i32, _vp, _vp]),
    "wtk_mlp_trainer_keep_scored": (_i32, [_vp, _vp, _vp, _vp]),
    "wtk_mlp_trainer_get_scores": (_i32, [_vp, _vp, _vp, _vp]),
    "wtk_yolo_conv_count": (_i32, [_f32, _f32, _i32, _i32]),
    "wtk_yolo_conv_info": (_i32, [_f32, _f32, _i32, _i32, _i32, _pi32, _pi32, _pi32, _pi32, _pi32, C.c_char_p, _size]),
    "wtk_yolo_create": (_i32, [_pvp, C.POINTER(_YoloDesc)]),
    "wtk_yolo_destroy": (None, [_vp]),
    "wtk_yolo_create_planned": (_i32, [_pvp, C.POINTER(_YoloDesc), _i32]),
    "wtk_yolo_plan": (_i32, [_vp]),
    "wtk_yolo_predict": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _f32, _f32, _i32, _vp, _vp, _vp, _vp]),
    "wtk_yolo_predict_host": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _f32, _f32, _i32, _vp, _vp, _vp]),
    "wtk_yolo_debug_head": (_i32, [_vp, _i32, _i32, _vp, _vp]),
    "wtk_yolo_debug_tensor": (_i32, [_vp, _i32, _i32, _vp, _size, _vp]),
    "wtk_yolo_decode_host": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _f32, _vp, _vp, _vp]),
    "wtk_yolo_status": (_i32, [_vp, _pi32, _i32]),
    "wtk_yolo_workload": (_i32, [_vp, _pf64, _pi32]),
    "wtk_yolo_set_profiling": (_i32, [_vp, _i32]),
    "wtk_yolo_get_profile": (_i32, [_vp, _i32, _pf64, _pi64]),
    "wtk_yolo_get_kernel_profile": (_i32, [_vp, _i32, _pf64, _pi64, _pf64]),
    "wtk_crop_views": (_i32, [_vp, _i32, _i32, _i32, _i32, _vp, _i32, _i32, _vp, _vp]),
    "wtk_yolo_margin_buffer": (_i32, [_vp, _pvp]),
    "wtk_yolo_last_margins_host": (_i32, [_vp, _i32, _vp]),
    "wtk_yolo_predict_nms": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _f32, _f32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "wtk_yolo_decode_nms_host": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _f32, _f32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "wtk_track_median_centers": (_i32, [_vp, _i32, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _vp]),
    "wtk_track_polyfit": (_i32, [_vp, _i32, _i32, _vp, _i32, _i32, _vp, _vp, _i32, _i32, _f64, _vp, _vp, _vp]),
    "wtk_track_training_pairs": (_i32, [_vp, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp]),
    "wtk_recheck_select": (_i32, [_vp, _i32, _i32, _f32, _vp, _vp, _vp]),
    "wtk_recheck_select_counted": (_i32, [_vp, _i32, _i32, _f32, _vp, _vp, _vp, _vp]),
    "wtk_yolo_set_dynamic_batch": (_i32, [_vp, _vp]),
    "wtk_yolo_set_side_streams": (_i32, [_vp, _i32]),
    "wtk_release_cached_memory": (_i32, []),
    "wtk_recheck_merge": (_i32, [_vp, _vp, _i32, _i32, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "wtk_recheck_enqueue": (_i32, [_vp, _i32, _f32, _vp, _i64, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "wtk_recheck_scatter": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "wtk_hybrid_create": (_i32, [_pvp, _vp, _vp, _f32, _i32, _i32]),
    "wtk_hybrid_destroy": (None, [_vp]),
    "wtk_hybrid_set_margin": (_i32, [_vp, _f32]),
    "wtk_hybrid_predict": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _f32, _vp, _vp, _vp, _vp]),
    "wtk_hybrid_predict_views": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _i32, _i32, _f32, _vp, _vp, _vp, _vp]),
    "wtk_hybrid_flush": (_i32, [_vp, _vp]),
    "wtk_hybrid_pending": (_i32, [_vp]),
    "wtk_hybrid_counters": (_i32, [_vp, _pi64, _pi64]),
    "wtk_hybrid_hold": (_i32, [_vp, _i32]),
    "wtk_hybrid_config": (_i32, [_vp, _pi32, _pi32, _pf32]),
    "wtk_yolo_predict_views": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _i32, _i32, _f32, _f32, _i32, _vp, _vp, _vp, _vp]),
    "wtk_comm_unique_id": (_i32, [_vp, _size]),
    "wtk_comm_create": (_i32, [_pvp, _i32, _i32, _i32, _vp]),
    "wtk_comm_destroy": (None, [_vp]),
    "wtk_allgather_tracks": (_i32, [_vp, _vp, _i32, _vp, _vp]),
    "wtk_background": (_i32, [_vp, _i32, _i64, _vp, _i32, _i32, _vp, _vp]),
    "wtk_precise_error": (_i32, [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _i32, _f64, _vp, _vp, _vp, _vp]),
    "wtk_polyfit_dataset": (_i32, [_vp, _i32, _i32, _i32, _vp, _i32, _i32, _f64, _f64, _vp, _vp, _i32, _vp, _vp]),
    "wtk_polyfit_mae_scratch_doubles": (_i64, [_i32, _i32]),
    "wtk_polyfit_weight_mae": (_i32, [_vp, _vp, _i64, _i32, _vp, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _i64, _vp, _vp]),
    "wtk_polyfit_swarm_step": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _f64, _f64, _f64, _f64, _f64, _f64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "wtk_replay_scan": (_i32, [_pcfg, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "wtk_replay_scratch_doubles": (_i64, [_i32, _i64]),
    "wtk_replay_rows": (_i32, [_pcfg, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "wtk_replay_polyfit_targets_scratch_doubles": (_i64, [_i32, _i32, _i32, _i32]),
    "wtk_replay_polyfit_targets": (_i32, [_vp, _i32, _i32, _i32, _vp, _i32, _vp, _i32, _i32, _f64, _vp, _vp, _i32, _vp, _vp, _vp, _i64, _vp, _vp]),
    "wtk_replay_objective": (_i32, [_pcfg, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp]),
    "wtk_replay_set_scan": (_i32, [_pcfg, _ptrk, _vp, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "wtk_replay_set_scratch_doubles": (_i64, [_ptrk, _i32, _i32, _i32]),
    "wtk_replay_set_rows": (_i32, [_pcfg, _ptrk, _vp, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp]),
    "wtk_replay_set_objective": (_i32, [_pcfg, _ptrk, _vp, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp,
                                        _vp, _vp]),
    "wtk_replay_set_precise_scratch_doubles": (_i64, [_ptrk, _i32, _i32, _i32]),
    "wtk_replay_set_precise": (_i32, [_pcfg, _ptrk, _vp, _pfrm, _vp, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp]),
    "wtk_replay_set_precise_objective": (_i32, [_pcfg, _ptrk, _vp, _pfrm, _vp, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _vp,
                                                _vp, _i64, _i32, _vp, _vp, _vp, _vp]),
    "wtk_replay_set_scan_geom": (_i32, [_pcfg, _ptrk, _vp, _pgeo, _vp, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "wtk_replay_set_rows_geom": (_i32, [_pcfg, _ptrk, _vp, _pgeo, _vp, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp]),
    "wtk_replay_set_objective_geom": (_i32, [_pcfg, _ptrk, _vp, _pgeo, _vp, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64,
                                             _i32, _vp, _vp, _vp, _vp]),
    "wtk_replay_set_precise_geom": (_i32, [_pcfg, _ptrk, _vp, _pgeo, _vp, _pfrm, _vp, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp,
                                           _i64, _vp, _vp]),
    "wtk_replay_set_precise_objective_geom": (_i32, [_pcfg, _ptrk, _vp, _pgeo, _vp, _pfrm, _vp, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp,
                                                     _i32, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp]),
    "wtk_replay_mlp_targets": (_i32, [C.POINTER(_MlpTrainLayer), _i32, _i32, _i32, _vp, _i32, _vp, _vp, _i32, _vp, _i32, _vp, _i32, _f32, _vp, _vp, _vp, _vp, _vp]),
    "wtk_replay_mlp_targets_waves": (_i32, [_i64]),
    "wtk_replay_mlp_targets_bounds": (_i32, [C.POINTER(_MlpTrainLayer), _i32, _i32, _i32, _vp, _i32, _vp, _vp, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp,
                                             _vp]),
    "wtk_replay_yolo_step": (_i32, [_pcfg, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "wtk_replay_yolo_positions": (_i32, [_pcfg, _i32, _vp, _vp, _vp, _vp, _vp]),
    "wtk_replay_yolo_track": (_i32, [_pcfg, _i32, _vp, _vp, _vp, _vp]),
    "wtk_boxes_scratch_bytes": (_i64, [_i32, _i32, _i32]),
    "wtk_boxes": (_i32, [_vp, _i32, _i32, _i32, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "wtk_replay_analysis_scratch_doubles": (_i64, [_i32, _i64, _i32, _i32]),
    "wtk_replay_analyze": (_i32, [_pcfg, _pacfg, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                  _vp, _i64, _vp]),
    "wtk_replay_set_analysis_scratch_doubles": (_i64, [_ptrk, _i32, _i32, _i32, _i32, _i32]),
    "wtk_replay_set_analyze": (_i32, [_pcfg, _pacfg, _ptrk, _vp, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _vp,
                                      _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "wtk_replay_set_analyze_geom": (_i32, [_pcfg, _pacfg, _ptrk, _vp, _pgeo, _vp, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _vp,
                                           _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "wtk_replay_precise_scratch_doubles": (_i64, [_i32, _i64]),
    "wtk_replay_precise": (_i32, [_pcfg, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _f64, _i32, _vp, _vp, _vp, _vp, _i64, _vp, _vp]),
    "wtk_replay_precise_objective": (_i32, [_pcfg, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _f64, _i32, _vp, _vp,
                                            _i64, _i32, _vp, _vp, _vp]),
}
SYMBOLS = list(SIGNATURES)  # every symbol include/wtk_hip.h declares


def lib_path() -> str:
    return _LIB_PATH


def _preload_torch_hip_runtime():
    """One HIP / HSA runtime per process.  PyTorch-ROCm ships its own libamdhip64.so / libhsa-runtime64.so (same sonames as
    /opt/rocm's).  Loaded AFTER `import torch`, libwtk_hip.so binds to torch's copies (soname match) and both share one runtime;
    loaded BEFORE it, /opt/rocm's copies come in first, torch later maps its own by path, and the second runtime to initialise
    finds no GPU ("No HIP GPUs are available").  So when torch is installed but not imported yet, its runtime libraries are
    mapped first (without importing torch)."""
    import importlib.util
    import sys

    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    libdir = os.path.join(os.path.dirname(spec.origin), "lib")
    for name in ("libhsa-runtime64.so", "libamdhip64.so"):
        path = os.path.join(libdir, name)
        if os.path.exists(path):
            try:
                C.CDLL(path, mode=C.RTLD_GLOBAL)
            except OSError:
                return  # fall back to the system runtime: nothing else to do here


def request_hw_queues(n: int = 8) -> bool:
    """Ask the HIP runtime for `n` hardware queues (GPU_MAX_HW_QUEUES; runtime default 4).  The detector keeps up to five streams busy per
    process (two lanes, the shared pair of side streams, the caller's default stream); the runtime multiplexes streams onto its hardware queues
    and streams that share one serialise (-3 %, and cliffs of -40 % for unlucky layouts: profiles/r02_notes.md §8).  The runtime reads the
    variable when it initialises, so call this before the first HIP call of the process (before `import torch` touches the GPU); an explicit
    value of the caller always wins.  OPT-IN on purpose: `load()` does not touch the environment, because children of the calling
    process inherit it — several processes sharing ONE device (e.g. the gloo rehearsal of the multi-rank path) must keep the runtime default
    (eight queues each: 19.5 k -> 4.9 k frames/s).  Returns True when the value was set by this call."""
    if "GPU_MAX_HW_QUEUES" in os.environ:
        return False
    os.environ["GPU_MAX_HW_QUEUES"] = str(int(n))
    return True


_warned_queues = False


def warn_if_streams_exceed_hw_queues(n_busy_streams: int) -> bool:
    """One warning per process when a caller is about to keep more streams busy than the HIP runtime has hardware queues by default (4) and
    GPU_MAX_HW_QUEUES was not set: streams that share a queue serialise (-3 % for the bench's five streams, up to -40 % for unlucky layouts,
    profiles/r02_notes.md section 8).  `request_hw_queues()` before the first HIP call is the fix; it is opt-in because child processes inherit the
    variable.  Returns True when the warning was issued."""
    global _warned_queues
    if _warned_queues or n_busy_streams <= 4 or "GPU_MAX_HW_QUEUES" in os.environ:
        return False
    import warnings

    _warned_queues = True
    warnings.warn(f"wtracker_amd: {n_busy_streams} HIP streams will be busy at once but GPU_MAX_HW_QUEUES is unset (runtime default: 4 hardware queues; streams that "
                  "share one serialise).  Call wtracker_amd.hip.request_hw_queues() before the first HIP call of the process, or export GPU_MAX_HW_QUEUES=8.",
                  RuntimeWarning, stacklevel=3)
    return True


def load() -> C.CDLL:
    """Load libwtk_hip.so (built in-tree by `python -m wtracker_amd._build` / __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise WtkError(f"{_LIB_PATH} not found: the HIP extension is not built (run __graft_entry__.build()); "
                       "there is no CPU fallback")
    _preload_torch_hip_runtime()
    lib = C.CDLL(_LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is None:
            if os.environ.get("WTK_HIP_LIB"):  # (an older build named for an A/B timing may lack the newer entry points)
                continue
            raise WtkError(f"{_LIB_PATH} does not export {name}: the library is older than this binding (rebuild it)")
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


def _check(rc: int, what: str):
    if rc != 0:
        raise WtkError(f"{what}: {load().wtk_last_error().decode(errors='replace')}")


def device_count() -> int:
    return int(load().wtk_device_count())


def _fptr(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _ptr(x) -> C.c_void_p:
    """Device pointer from a torch tensor / int, host pointer from a numpy array; None -> NULL."""
    if x is None:
        return C.c_void_p(0)
    if isinstance(x, np.ndarray):
        return C.c_void_p(x.ctypes.data)
    if isinstance(x, int):
        return C.c_void_p(x)
    if hasattr(x, "data_ptr"):
        return C.c_void_p(x.data_ptr())
    raise TypeError(f"cannot take a pointer of {type(x)}")


def crop_views(frames_dev, N: int, H: int, W: int, Cc: int, pos_xy_dev, view_w: int, view_h: int, views_dev, stream: int = 0):
    """Device-side ViewController.camera_view for a batch: views[n] = window of frames[n] centred on pos_xy[n]
    with replicate borders.  All arguments are device tensors / pointers."""
    _check(load().wtk_crop_views(_ptr(frames_dev), N, H, W, Cc, _ptr(pos_xy_dev), view_w, view_h, _ptr(views_dev),
                                 C.c_void_p(stream)), "wtk_crop_views")


def release_cached_memory():
    """Give the device memory of destroyed detector handles (kept for reuse) back to the driver."""
    _check(load().wtk_release_cached_memory(), "wtk_release_cached_memory")


def recheck_select(margins_dev, B: int, K: int, margin: float, slots_dev, n_weak_dev=None, stream: int = 0, n_overflow_dev=None):
    """slots[k] = batch row of the k-th smallest decision margin (device int32 [K]); n_weak = min(K, rows below `margin`);
    n_overflow += the weak rows beyond the ceiling K (they get no second look); asynchronous on `stream`."""
    _check(load().wtk_recheck_select_counted(_ptr(margins_dev), B, K, margin, _ptr(slots_dev), _ptr(n_weak_dev), _ptr(n_overflow_dev), C.c_void_p(stream)),
           "wtk_recheck_select_counted")


def recheck_enqueue(margins_dev, B: int, margin: float, frames_dev, frame_bytes: int, q_frames_dev, q_cap: int, q_len_dev, q_xywh_ptrs, q_conf_ptrs, q_anchor_ptrs,
                    dst_xywh, dst_conf, dst_anchor, pos_scratch_dev, n_overflow_dev=None, stream: int = 0):
    """Append the batch rows with margin < `margin` (frame copy + output addresses) to the device-side queue of the deferred second look."""
    _check(load().wtk_recheck_enqueue(_ptr(margins_dev), B, margin, _ptr(frames_dev), frame_bytes, _ptr(q_frames_dev), q_cap, _ptr(q_len_dev), _ptr(q_xywh_ptrs),
                                      _ptr(q_conf_ptrs), _ptr(q_anchor_ptrs), _ptr(dst_xywh), _ptr(dst_conf), _ptr(dst_anchor), _ptr(pos_scratch_dev),
                                      _ptr(n_overflow_dev), C.c_void_p(stream)), "wtk_recheck_enqueue")


def recheck_scatter(q_len_dev, q_cap: int, src_xywh, src_conf, src_anchor, q_xywh_ptrs, q_conf_ptrs, q_anchor_ptrs, n_replaced_dev=None, stream: int = 0):
    """Rows 0 .. *q_len - 1 of the full-precision pass go to the addresses queued by recheck_enqueue; the queue is empty afterwards."""
    _check(load().wtk_recheck_scatter(_ptr(q_len_dev), q_cap, _ptr(src_xywh), _ptr(src_conf), _ptr(src_anchor), _ptr(q_xywh_ptrs), _ptr(q_conf_ptrs),
                                      _ptr(q_anchor_ptrs), _ptr(n_replaced_dev), C.c_void_p(stream)), "wtk_recheck_scatter")


def recheck_merge(margins_dev, slots_dev, B: int, K: int, margin: float, src_xywh, src_conf, src_anchor, dst_xywh, dst_conf=None, dst_anchor=None,
                  n_replaced_dev=None, stream: int = 0):
    """Rows slots[k] of dst_* take row k of src_* where the fast pass's margin is below `margin`."""
    _check(load().wtk_recheck_merge(_ptr(margins_dev), _ptr(slots_dev), B, K, margin, _ptr(src_xywh), _ptr(src_conf), _ptr(src_anchor), _ptr(dst_xywh),
                                    _ptr(dst_conf), _ptr(dst_anchor), _ptr(n_replaced_dev), C.c_void_p(stream)), "wtk_recheck_merge")


COMM_ID_BYTES = 128


def comm_unique_id() -> bytes:
    """Rank 0: the RCCL rendezvous token (128 bytes) to hand to every other rank out of band."""
    buf = (C.c_uint8 * COMM_ID_BYTES)()
    _check(load().wtk_comm_unique_id(buf, COMM_ID_BYTES), "wtk_comm_unique_id")
    return bytes(buf)


class WtkComm:
    """The C ABI's own RCCL communicator (wtk_comm_*): one per rank, for callers that do not use torch.distributed."""

    def __init__(self, device: int, rank: int, world: int, unique_id: bytes):
        if len(unique_id) != COMM_ID_BYTES:
            raise WtkError("unique_id must be the 128 bytes of comm_unique_id()")
        self._h = C.c_void_p()
        buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(unique_id)
        _check(load().wtk_comm_create(C.byref(self._h), device, rank, world, buf), "wtk_comm_create")
        self.rank, self.world, self.device = rank, world, device

    def allgather_tracks(self, local_dev, n_local: int, all_dev, stream: int = 0):
        """all_dev[r * n_local : (r + 1) * n_local] = rank r's local_dev [n_local, 4] float32 (device tensors)."""
        _check(load().wtk_allgather_tracks(self._h, _ptr(local_dev), n_local, _ptr(all_dev), C.c_void_p(stream)), "wtk_allgather_tracks")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            load().wtk_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _track_is_f64(track_dev) -> int:
    dt = str(getattr(track_dev, "dtype", ""))
    if dt.endswith("float64"):
        return 1
    if dt.endswith("float32"):
        return 0
    raise WtkError("track must be a float32 or float64 device tensor [n_frames, 4]")


def track_median_centers(track_dev, n_frames: int, cycles_dev, n_samples: int, cycle_frame_num: int, imaging_frame_num: int, pred_dev, valid_dev,
                         stream: int = 0):
    """OptimalController's target for every cycle in `cycles_dev` (wtk_track_median_centers); pred_dev float64 [n,2]."""
    _check(load().wtk_track_median_centers(_ptr(track_dev), _track_is_f64(track_dev), n_frames, _ptr(cycles_dev), n_samples, cycle_frame_num,
                                           imaging_frame_num, _ptr(pred_dev), _ptr(valid_dev), C.c_void_p(stream)), "wtk_track_median_centers")


def track_polyfit(track_dev, n_frames: int, cycles_dev, n_samples: int, cycle_frame_num: int, sample_times: Sequence[int], weights: Sequence[float],
                  degree: int, t_eval: float, pred_dev, valid_dev, stream: int = 0):
    """PolyfitController's extrapolated head position for every cycle in `cycles_dev` (wtk_track_polyfit); pred_dev float64 [n,2]."""
    st = np.ascontiguousarray(sample_times, dtype=np.int32)
    w = np.ascontiguousarray(weights, dtype=np.float64)
    if len(st) != len(w):
        raise WtkError("sample_times and weights differ in length")
    _check(load().wtk_track_polyfit(_ptr(track_dev), _track_is_f64(track_dev), n_frames, _ptr(cycles_dev), n_samples, cycle_frame_num, _ptr(st), _ptr(w),
                                    len(st), degree, float(t_eval), _ptr(pred_dev), _ptr(valid_dev), C.c_void_p(stream)), "wtk_track_polyfit")


def track_training_pairs(track_dev, n_frames: int, row0: int, n_rows: int, input_frames: Sequence[int], pred_frames: Sequence[int], x_dev, y_dev,
                         keep_dev, stream: int = 0):
    """NumpyDataset.create_from_config's rows row0 .. row0+n_rows-1 (wtk_track_training_pairs); the caller drops keep == 0."""
    xi = np.ascontiguousarray(input_frames, dtype=np.int32)
    yi = np.ascontiguousarray(pred_frames, dtype=np.int32)
    _check(load().wtk_track_training_pairs(_ptr(track_dev), _track_is_f64(track_dev), n_frames, row0, n_rows, _ptr(xi), len(xi), _ptr(yi), len(yi),
                                           _ptr(x_dev), _ptr(y_dev), _ptr(keep_dev), C.c_void_p(stream)), "wtk_track_training_pairs")


BG_MEDIAN, BG_MEAN = 0, 1  # WTK_BG_MEDIAN / WTK_BG_MEAN
BG_MEDIAN_MAX_PROBES, BG_MEAN_MAX_PROBES = 65535, 1 << 24


def background(frames_dev, n_frames: int, frame_bytes: int, probe_idx_dev, n_probes: int, method: int, bg_dev, stream: int = 0):
    """bg_dev[frame_bytes] = per-byte median / mean of the probe frames (wtk_background); probe_idx_dev int32 [n_probes] or None (frames 0..n-1)."""
    _check(load().wtk_background(_ptr(frames_dev), n_frames, frame_bytes, _ptr(probe_idx_dev), n_probes, method, _ptr(bg_dev), C.c_void_p(stream)),
           "wtk_background")


def boxes_scratch_bytes(H: int, W: int, n_sel: int) -> int:
    """Bytes of scratch wtk_boxes needs for n_sel frames of H x W: 8 + 4 H ceil(W / 32) per frame (the winner key and the bit mask)."""
    n = int(load().wtk_boxes_scratch_bytes(H, W, n_sel))
    if n < 0:
        raise WtkError(f"wtk_boxes_scratch_bytes: H = {H}, W = {W}, n_sel = {n_sel} is not a shape wtk_boxes takes (all positive, H * W <= 2^30)")
    return n


def boxes(frames_dev, n_frames: int, H: int, W: int, bg_dev, frame_idx_dev, n_sel: int, diff_thresh: int, boxes_dev, area2_dev, mask_dev, fault_count_dev,
          scratch_dev, scratch_bytes: int, stream: int = 0):
    """boxes_dev int32 [n_sel, 4] = the box of the largest foreground contour of every selected frame (wtk_boxes); frame_idx_dev int32 [n_sel] or None
    (frames 0..n_sel-1), area2_dev int64 [n_sel] or None, mask_dev uint8 [n_sel, H, W] or None, fault_count_dev int32 [1] (added to), scratch_dev of
    boxes_scratch_bytes(H, W, n_sel) bytes.  boxes_dev None (with area2_dev None): the mask stage alone."""
    _check(load().wtk_boxes(_ptr(frames_dev), n_frames, H, W, _ptr(bg_dev), _ptr(frame_idx_dev), n_sel, int(diff_thresh), _ptr(boxes_dev), _ptr(area2_dev),
                            _ptr(mask_dev), _ptr(fault_count_dev), _ptr(scratch_dev), int(scratch_bytes), C.c_void_p(stream)), "wtk_boxes")


def precise_error(frames_dev, n_frames: int, H: int, W: int, bg_dev, worm_dev, mic_dev, frame_nums_dev, n_rows: int, diff_thresh: float, err_dev,
                  counts_dev=None, n_bad_frame_dev=None, stream: int = 0):
    """err_dev float64 [n_rows] = the precise error of every log row (wtk_precise_error); boxes float32 or float64 [n_rows, 4], both of one dtype."""
    f64 = _track_is_f64(worm_dev)
    if _track_is_f64(mic_dev) != f64:
        raise WtkError("worm and microscope boxes must share one dtype")
    _check(load().wtk_precise_error(_ptr(frames_dev), n_frames, H, W, _ptr(bg_dev), _ptr(worm_dev), _ptr(mic_dev), f64, _ptr(frame_nums_dev), n_rows,
                                    float(diff_thresh), _ptr(err_dev), _ptr(counts_dev), _ptr(n_bad_frame_dev), C.c_void_p(stream)), "wtk_precise_error")


def polyfit_dataset(track_dev, n_frames: int, cycle_frame_num: int, input_offsets: Sequence[int], pred_time_offset: int, min_speed: float, max_speed: float,
                    y_input_dev, y_target_dev, capacity: int, count_dev, stream: int = 0):
    """WeightEvaluator's dataset of one log appended behind the *count_dev cycles already in y_input_dev [N, 2 * capacity] / y_target_dev [2 * capacity]
    (wtk_polyfit_dataset); input_offsets sorted ascending."""
    off = np.ascontiguousarray(input_offsets, dtype=np.int32)
    _check(load().wtk_polyfit_dataset(_ptr(track_dev), _track_is_f64(track_dev), n_frames, cycle_frame_num, _ptr(off), len(off), int(pred_time_offset),
                                      float(min_speed), float(max_speed), _ptr(y_input_dev), _ptr(y_target_dev), capacity, _ptr(count_dev),
                                      C.c_void_p(stream)), "wtk_polyfit_dataset")


def polyfit_mae_scratch_doubles(P: int, M: int) -> int:
    return int(load().wtk_polyfit_mae_scratch_doubles(P, M))


def polyfit_weight_mae(y_input_dev, y_target_dev, ld: int, M: int, sample_times: Sequence[int], pred_time_offset: int, degree: int, weights_dev, P: int,
                       mae_dev, scratch_dev, scratch_doubles: int, stop_dev=None, stream: int = 0):
    """mae_dev[p] = WeightEvaluator.eval(weights_dev[p], degree) for P weight vectors (wtk_polyfit_weight_mae); all float64 device tensors."""
    st = np.ascontiguousarray(sample_times, dtype=np.int32)
    _check(load().wtk_polyfit_weight_mae(_ptr(y_input_dev), _ptr(y_target_dev), ld, M, _ptr(st), len(st), int(pred_time_offset), degree, _ptr(weights_dev), P,
                                         _ptr(mae_dev), _ptr(scratch_dev), scratch_doubles, _ptr(stop_dev), C.c_void_p(stream)), "wtk_polyfit_weight_mae")


def polyfit_swarm_step(mae_dev, rand_dev, P: int, N: int, epoch: int, max_early_stop: int, w: float, c1: float, c2: float, lb: float, ub: float, vmax: float,
                       pos_dev, vel_dev, pbest_pos_dev, pbest_val_dev, gbest_pos_dev, gbest_val_dev, ctrl_dev, history_dev, stream: int = 0):
    """One epoch of the weight swarm on device-resident state (wtk_polyfit_swarm_step); rand_dev: this epoch's [2, P, N] slice."""
    _check(load().wtk_polyfit_swarm_step(_ptr(mae_dev), _ptr(rand_dev), P, N, epoch, max_early_stop, float(w), float(c1), float(c2), float(lb), float(ub),
                                         float(vmax), _ptr(pos_dev), _ptr(vel_dev), _ptr(pbest_pos_dev), _ptr(pbest_val_dev), _ptr(gbest_pos_dev),
                                         _ptr(gbest_val_dev), _ptr(ctrl_dev), _ptr(history_dev), C.c_void_p(stream)), "wtk_polyfit_swarm_step")


REPLAY_CSV, REPLAY_OPTIMAL, REPLAY_POLYFIT, REPLAY_MLP = 0, 1, 2, 3  # WTK_REPLAY_*
REPLAY_ROW_DOUBLES, REPLAY_SUMMARY_DOUBLES = 16, 6


def replay_config(num_frames: int, imaging_frame_num: int, moving_frame_num: int, pred_frame_num: int, camera_size: Sequence[int],
                  micro_size: Sequence[int], frame_wh: Sequence[int], init_position: Sequence[int]) -> _ReplayConfig:
    """The wtk_replay_config of an experiment; sizes and positions are (x, y) pairs."""
    return _ReplayConfig(int(num_frames), int(imaging_frame_num), int(moving_frame_num), int(pred_frame_num), int(camera_size[0]), int(camera_size[1]),
                         int(micro_size[0]), int(micro_size[1]), int(frame_wh[0]), int(frame_wh[1]), int(init_position[0]), int(init_position[1]))


def replay_scan(cfg: _ReplayConfig, kind: int, E: int, n_cycles: int, track_dev, n_track: int, a_dev, b_dev, valid_dev, share_dev, pos_dev, move_dev,
                stream: int = 0):
    """Moves and cycle-start positions of E experiments (wtk_replay_scan); per-cycle arrays are [n_cycles, E, ...] device tensors."""
    _check(load().wtk_replay_scan(C.byref(cfg) if cfg is not None else None, kind, E, n_cycles, _ptr(track_dev), n_track, _ptr(a_dev), _ptr(b_dev),
                                  _ptr(valid_dev), _ptr(share_dev), _ptr(pos_dev), _ptr(move_dev), C.c_void_p(stream)), "wtk_replay_scan")


def replay_scratch_doubles(E: int, R: int) -> int:
    return int(load().wtk_replay_scratch_doubles(E, R))


def replay_rows(cfg: _ReplayConfig, E: int, n_cycles: int, track_dev, n_track: int, share_dev, pos_dev, move_dev, row_slot_dev, n_slots: int, rows_dev,
                bbox_err_dev, mse_err_dev, summary_dev, scratch_dev, scratch_doubles: int, stream: int = 0):
    """Log rows, per-row errors and per-experiment summaries from a scan's positions and moves (wtk_replay_rows)."""
    _check(load().wtk_replay_rows(C.byref(cfg) if cfg is not None else None, E, n_cycles, _ptr(track_dev), n_track, _ptr(share_dev), _ptr(pos_dev),
                                  _ptr(move_dev), _ptr(row_slot_dev), n_slots, _ptr(rows_dev), _ptr(bbox_err_dev), _ptr(mse_err_dev), _ptr(summary_dev),
                                  _ptr(scratch_dev), scratch_doubles, C.c_void_p(stream)), "wtk_replay_rows")


REPLAY_OBJECTIVES = {"trimmed_bbox_error": 0, "bbox_error": 1, "mse_error": 2, "non_perfect": 3}  # WTK_REPLAY_OBJ_*


def replay_polyfit_targets_scratch_doubles(n_classes: int, P: int, n_times: int, degree: int) -> int:
    return int(load().wtk_replay_polyfit_targets_scratch_doubles(n_classes, P, n_times, degree))


def replay_polyfit_targets(track_dev, n_track: int, n_cycles: int, cycle_frame_num: int, weights_dev, P: int, sample_times: Sequence[int], degree: int,
                           t_eval: float, cycle_class_dev, class_mask_dev, n_classes: int, a_dev, valid_dev, scratch_dev, scratch_doubles: int, stop_dev=None,
                           stream: int = 0):
    """Polyfit targets of P device-resident weight vectors in one call (wtk_replay_polyfit_targets): a_dev [n_cycles, P, 2], valid_dev [n_cycles, P]."""
    if _track_is_f64(track_dev) != 1:
        raise WtkError("wtk_replay_polyfit_targets takes a float64 track")
    st = np.ascontiguousarray(sample_times, dtype=np.int32)
    _check(load().wtk_replay_polyfit_targets(_ptr(track_dev), n_track, n_cycles, cycle_frame_num, _ptr(weights_dev), P, _ptr(st), len(st), degree, float(t_eval),
                                             _ptr(cycle_class_dev), _ptr(class_mask_dev), n_classes, _ptr(a_dev), _ptr(valid_dev), _ptr(scratch_dev),
                                             scratch_doubles, _ptr(stop_dev), C.c_void_p(stream)), "wtk_replay_polyfit_targets")


def replay_objective(cfg: _ReplayConfig, kind: int, E: int, n_cycles: int, track_dev, n_track: int, a_dev, b_dev, valid_dev, share_dev, pos_dev, move_dev,
                     summary_dev, scratch_dev, scratch_doubles: int, objective: int, objective_dev, stop_dev=None, stream: int = 0):
    """objective_dev[e] = the chosen closed-loop error of experiment e (wtk_replay_objective): scan, rows reduction and one division, no host round trip."""
    _check(load().wtk_replay_objective(C.byref(cfg) if cfg is not None else None, kind, E, n_cycles, _ptr(track_dev), n_track, _ptr(a_dev), _ptr(b_dev),
                                       _ptr(valid_dev), _ptr(share_dev), _ptr(pos_dev), _ptr(move_dev), _ptr(summary_dev), _ptr(scratch_dev), scratch_doubles,
                                       objective, _ptr(objective_dev), _ptr(stop_dev), C.c_void_p(stream)), "wtk_replay_objective")


ROW_CHUNK = 4096  # kRowChunk (csrc/replay_device.h): logged rows per block of a reducing kernel


class ReplaySetTable:
    """The track table of a set of tracks in one super-track (wtk_replay_set_track [T]): `host` the ctypes array the entry points check, `dev` the
    same bytes on the device (uploaded here, once).  `tracks`: per track a dict of cyc_off, n_track, num_frames, n_cycles, n_log, frame_wh, init_position
    (clamped here, as the scan clamps it); R and chunk0 are derived."""

    def __init__(self, tracks: Sequence[dict], cycle_frame_num: int, guard_cycles: int, n_super: int, device=None):
        self.T, self.L, self.guard_cycles, self.n_super = len(tracks), int(cycle_frame_num), int(guard_cycles), int(n_super)
        self.host = (_ReplaySetTrack * max(1, self.T))()
        chunk0 = 0
        for t, tr in enumerate(tracks):
            (W, H), R = tr["frame_wh"], int(tr["n_log"]) * self.L
            x, y = (int(min(max(int(v), 0), int(m) - 1)) for v, m in zip(tr["init_position"], (W, H)))
            self.host[t] = _ReplaySetTrack(R, int(tr["cyc_off"]), int(tr["n_track"]), int(tr["num_frames"]), int(tr["n_cycles"]), int(tr["n_log"]), int(W) - 1,
                                           int(H) - 1, x, y, chunk0)
            chunk0 += (R + ROW_CHUNK - 1) // ROW_CHUNK
        self.n_chunks = chunk0
        self.dev = None
        if device is not None:
            import torch

            raw = np.frombuffer(bytes(self.host), dtype=np.uint8).copy()
            self.dev = torch.from_numpy(raw).to(device)

    def _args(self):
        return self.host, _ptr(self.dev), self.T, self.guard_cycles


class ReplaySetGeometry:
    """The per-track geometry table of a set (wtk_replay_set_geometry [T]), beside its ReplaySetTable: `host` the ctypes array the entry points check,
    `dev` the same bytes on the device (uploaded here, once).  `entries`: per track a dict of cam (w, h), mic (w, h) in pixels and factors (time,
    distance, speed) of change_unit.  Passed as `geom=` to the replay_set_* calls; None there means the config's sizes for every track."""

    def __init__(self, entries: Sequence[dict], device=None):
        self.T = len(entries)
        self.host = (_ReplaySetGeometry * max(1, self.T))()
        for t, g in enumerate(entries):
            (cw, ch), (mw, mh), (tf, df, sf) = g["cam"], g["mic"], g["factors"]
            self.host[t] = _ReplaySetGeometry(int(cw), int(ch), int(mw), int(mh), float(tf), float(df), float(sf))
        self.dev = None
        if device is not None:
            import torch

            raw = np.frombuffer(bytes(self.host), dtype=np.uint8).copy()
            self.dev = torch.from_numpy(raw).to(device)


def _geom_args(table: ReplaySetTable, geom: Optional[ReplaySetGeometry]):
    """(tracks_host, tracks_dev, geom_host, geom_dev, T, guard_cycles) of a *_geom entry point."""
    if geom is not None and geom.T != table.T:
        raise WtkError(f"the geometry table needs one entry per track: {table.T} tracks, {geom.T} entries")
    host, dev, T, guard = table._args()
    return host, dev, (geom.host if geom is not None else None), (_ptr(geom.dev) if geom is not None else None), T, guard


def replay_set_scan(cfg: _ReplayConfig, table: ReplaySetTable, kind: int, E: int, track_dev, a_dev, b_dev, valid_dev, share_dev, pos_dev, move_dev, stop_dev=None,
                    stream: int = 0, geom: Optional[ReplaySetGeometry] = None):
    """wtk_replay_scan of every (track, experiment) of a set (wtk_replay_set_scan); per-cycle arrays are [n_super / L, E, ...] device tensors.
    `geom` (here and in the calls below): the set's ReplaySetGeometry, which selects the *_geom entry point of the same name."""
    fn, head = (load().wtk_replay_set_scan, table._args()) if geom is None else (load().wtk_replay_set_scan_geom, _geom_args(table, geom))
    _check(fn(C.byref(cfg) if cfg is not None else None, *head, kind, E, _ptr(track_dev), table.n_super, _ptr(a_dev),
                                      _ptr(b_dev), _ptr(valid_dev), _ptr(share_dev), _ptr(pos_dev), _ptr(move_dev), _ptr(stop_dev), C.c_void_p(stream)),
           "wtk_replay_set_scan")


def replay_set_scratch_doubles(table: ReplaySetTable, E: int) -> int:
    return int(load().wtk_replay_set_scratch_doubles(table.host, table.T, table.L, E))


def replay_set_rows(cfg: _ReplayConfig, table: ReplaySetTable, E: int, track_dev, share_dev, pos_dev, move_dev, track_summary_dev, summary_dev, scratch_dev,
                    scratch_doubles: int, stop_dev=None, stream: int = 0, geom: Optional[ReplaySetGeometry] = None):
    """Per-track summaries [T, E, 6] and the pooled summary [E, 6] from a set scan's positions and moves (wtk_replay_set_rows)."""
    fn, head = (load().wtk_replay_set_rows, table._args()) if geom is None else (load().wtk_replay_set_rows_geom, _geom_args(table, geom))
    _check(fn(C.byref(cfg) if cfg is not None else None, *head, E, _ptr(track_dev), table.n_super, _ptr(share_dev),
                                      _ptr(pos_dev), _ptr(move_dev), _ptr(track_summary_dev), _ptr(summary_dev), _ptr(scratch_dev), scratch_doubles,
                                      _ptr(stop_dev), C.c_void_p(stream)), "wtk_replay_set_rows")


def replay_set_objective(cfg: _ReplayConfig, table: ReplaySetTable, kind: int, E: int, track_dev, a_dev, b_dev, valid_dev, share_dev, pos_dev, move_dev,
                         track_summary_dev, summary_dev, scratch_dev, scratch_doubles: int, objective: int, objective_dev, track_objective_dev=None,
                         stop_dev=None, stream: int = 0, geom: Optional[ReplaySetGeometry] = None):
    """objective_dev[e] = the chosen closed-loop error of experiment e pooled over the set's tracks (wtk_replay_set_objective); track_objective_dev
    [T, E] (optional): the same of each track."""
    fn, head = (load().wtk_replay_set_objective, table._args()) if geom is None else (load().wtk_replay_set_objective_geom, _geom_args(table, geom))
    _check(fn(C.byref(cfg) if cfg is not None else None, *head, kind, E, _ptr(track_dev), table.n_super, _ptr(a_dev),
                                           _ptr(b_dev), _ptr(valid_dev), _ptr(share_dev), _ptr(pos_dev), _ptr(move_dev), _ptr(track_summary_dev),
                                           _ptr(summary_dev), _ptr(scratch_dev), scratch_doubles, objective, _ptr(objective_dev), _ptr(track_objective_dev),
                                           _ptr(stop_dev), C.c_void_p(stream)), "wtk_replay_set_objective")


REPLAY_PRECISE_SUMMARY_DOUBLES = 6
REPLAY_PRECISE_OBJECTIVES = {"trimmed_precise_error": 0, "precise_error": 1, "precise_non_perfect": 2}  # WTK_REPLAY_POBJ_*


class ReplaySetFrames:
    """The frames table of a set of tracks (wtk_replay_set_frames [T]), beside its ReplaySetTable: `host` the ctypes array the entry points check,
    `dev` the same bytes on the device (uploaded here, once).  `entries`: per track a dict of frames (device pointer), bg (device pointer), n_frames, H,
    W, diff_thresh; row0 is derived from the table's R.  The caller keeps the tensors behind the pointers alive."""

    def __init__(self, table: ReplaySetTable, entries: Sequence[dict], device=None):
        if len(entries) != table.T:
            raise WtkError(f"the frames table needs one entry per track: {table.T} tracks, {len(entries)} entries")
        self.T = table.T
        self.host = (_ReplaySetFrames * max(1, self.T))()
        row0 = 0
        for t, fr in enumerate(entries):
            self.host[t] = _ReplaySetFrames(int(fr["frames"]), int(fr["bg"]), float(fr["diff_thresh"]), row0, int(fr["n_frames"]), int(fr["H"]), int(fr["W"]), 0)
            row0 += int(table.host[t].R)
        self.n_rows = row0
        self.dev = None
        if device is not None:
            import torch

            raw = np.frombuffer(bytes(self.host), dtype=np.uint8).copy()
            self.dev = torch.from_numpy(raw).to(device)

    def _args(self):
        return self.host, _ptr(self.dev)


def replay_set_precise_scratch_doubles(table: ReplaySetTable, E: int) -> int:
    return int(load().wtk_replay_set_precise_scratch_doubles(table.host, table.T, table.L, E))


def replay_set_precise(cfg: _ReplayConfig, table: ReplaySetTable, frames: ReplaySetFrames, E: int, track_dev, share_dev, pos_dev, move_dev, max_crop_px: int,
                       err_dev, counts_dev, track_summary_dev, summary_dev, scratch_dev, scratch_doubles: int, stop_dev=None, stream: int = 0,
                       geom: Optional[ReplaySetGeometry] = None):
    """The precise error of every (track, experiment, logged frame) of a set scan (wtk_replay_set_precise): per-track summaries [T, E, 6], the pooled
    summary [E, 6]; err_dev float64 [E, sum R] and counts_dev int32 [E, sum R, 2] or None."""
    fn, (*head, T, guard) = (load().wtk_replay_set_precise, table._args()) if geom is None else (load().wtk_replay_set_precise_geom, _geom_args(table, geom))
    _check(fn(C.byref(cfg) if cfg is not None else None, *head, *frames._args(), T, guard, E, _ptr(track_dev), table.n_super,
                                         _ptr(share_dev), _ptr(pos_dev), _ptr(move_dev), int(max_crop_px), _ptr(err_dev), _ptr(counts_dev),
                                         _ptr(track_summary_dev), _ptr(summary_dev), _ptr(scratch_dev), scratch_doubles, _ptr(stop_dev), C.c_void_p(stream)),
           "wtk_replay_set_precise")


def replay_set_precise_objective(cfg: _ReplayConfig, table: ReplaySetTable, frames: ReplaySetFrames, kind: int, E: int, track_dev, a_dev, b_dev, valid_dev,
                                 share_dev, pos_dev, move_dev, max_crop_px: int, track_summary_dev, summary_dev, scratch_dev, scratch_doubles: int,
                                 objective: int, objective_dev, track_objective_dev=None, stop_dev=None, stream: int = 0,
                                 geom: Optional[ReplaySetGeometry] = None):
    """objective_dev[e] = the chosen precise-error figure of experiment e pooled over the set's tracks (wtk_replay_set_precise_objective);
    track_objective_dev [T, E] (optional): the same of each track."""
    fn, (*head, T, guard) = ((load().wtk_replay_set_precise_objective, table._args()) if geom is None
                             else (load().wtk_replay_set_precise_objective_geom, _geom_args(table, geom)))
    _check(fn(C.byref(cfg) if cfg is not None else None, *head, *frames._args(), T, guard, kind, E, _ptr(track_dev),
                                                   table.n_super, _ptr(a_dev), _ptr(b_dev), _ptr(valid_dev), _ptr(share_dev), _ptr(pos_dev), _ptr(move_dev),
                                                   int(max_crop_px), _ptr(track_summary_dev), _ptr(summary_dev), _ptr(scratch_dev), scratch_doubles, objective,
                                                   _ptr(objective_dev), _ptr(track_objective_dev), _ptr(stop_dev), C.c_void_p(stream)),
           "wtk_replay_set_precise_objective")


def replay_precise_scratch_doubles(E: int, R: int) -> int:
    return int(load().wtk_replay_precise_scratch_doubles(E, R))


def replay_precise(cfg: _ReplayConfig, E: int, n_cycles: int, track_dev, n_track: int, share_dev, pos_dev, move_dev, frames_dev, n_frames: int, H: int, W: int,
                   bg_dev, diff_thresh: float, max_crop_px: int, err_dev, counts_dev, summary_dev, scratch_dev, scratch_doubles: int, stop_dev=None,
                   stream: int = 0):
    """The precise error of every (experiment, logged frame) pair of a scan and its per-experiment summaries (wtk_replay_precise): frames_dev uint8
    [n_frames, H, W], bg_dev uint8 [H, W]; err_dev float64 [E, R] and counts_dev int32 [E, R, 2] or None."""
    _check(load().wtk_replay_precise(C.byref(cfg) if cfg is not None else None, E, n_cycles, _ptr(track_dev), n_track, _ptr(share_dev), _ptr(pos_dev),
                                     _ptr(move_dev), _ptr(frames_dev), n_frames, H, W, _ptr(bg_dev), float(diff_thresh), int(max_crop_px), _ptr(err_dev),
                                     _ptr(counts_dev), _ptr(summary_dev), _ptr(scratch_dev), scratch_doubles, _ptr(stop_dev), C.c_void_p(stream)),
           "wtk_replay_precise")


def replay_precise_objective(cfg: _ReplayConfig, kind: int, E: int, n_cycles: int, track_dev, n_track: int, a_dev, b_dev, valid_dev, share_dev, pos_dev,
                             move_dev, frames_dev, n_frames: int, H: int, W: int, bg_dev, diff_thresh: float, max_crop_px: int, summary_dev, scratch_dev,
                             scratch_doubles: int, objective: int, objective_dev, stop_dev=None, stream: int = 0):
    """objective_dev[e] = the chosen precise-error figure of experiment e (wtk_replay_precise_objective): scan, precise and one division."""
    _check(load().wtk_replay_precise_objective(C.byref(cfg) if cfg is not None else None, kind, E, n_cycles, _ptr(track_dev), n_track, _ptr(a_dev),
                                               _ptr(b_dev), _ptr(valid_dev), _ptr(share_dev), _ptr(pos_dev), _ptr(move_dev), _ptr(frames_dev), n_frames, H, W,
                                               _ptr(bg_dev), float(diff_thresh), int(max_crop_px), _ptr(summary_dev), _ptr(scratch_dev), scratch_doubles,
                                               objective, _ptr(objective_dev), _ptr(stop_dev), C.c_void_p(stream)), "wtk_replay_precise_objective")


# WTK_ANALYSIS_COL_*: the columns of DataAnalyzer's table, in the header's order
ANALYSIS_COLUMNS = ["frame", "cycle", "plt_x", "plt_y", "cam_x", "cam_y", "cam_w", "cam_h", "mic_x", "mic_y", "mic_w", "mic_h", "wrm_x", "wrm_y", "wrm_w", "wrm_h",
                    "time", "cycle_step", "wrm_center_x", "wrm_center_y", "mic_center_x", "mic_center_y", "wrm_speed_x", "wrm_speed_y", "wrm_speed",
                    "worm_deviation_x", "worm_deviation_y", "worm_deviation", "bbox_error", "precise_error"]
ANALYSIS_MAX_COLUMNS, ANALYSIS_MAX_PERCENTILES = 32, 16


def replay_analysis_config(period: int, imaging_only: bool, bounds, trim_cycles: bool, factors: Sequence[float], min_speed: float, min_bbox_error: float,
                           min_dist_error: float, min_width: float, min_height: float, no_preds: bool) -> _AnalysisConfig:
    """The wtk_replay_analysis_config of an analysis; `bounds` (x0, y0, x1, y1) or None, `factors` (time, distance, speed)."""
    b = (C.c_double * 4)(*(float(v) for v in (bounds if bounds is not None else (0, 0, 0, 0))))
    return _AnalysisConfig(b, float(factors[0]), float(factors[1]), float(factors[2]), float(min_speed), float(min_bbox_error), float(min_dist_error),
                           float(min_width), float(min_height), int(period), int(bool(imaging_only)), int(bounds is not None), int(bool(trim_cycles)),
                           int(bool(no_preds)), 0)


def replay_analysis_scratch_doubles(E: int, R: int, n_cols: int, Q: int) -> int:
    return int(load().wtk_replay_analysis_scratch_doubles(E, R, n_cols, Q))


def replay_analyze(cfg: _ReplayConfig, acfg: _AnalysisConfig, E: int, n_cycles: int, track_dev, n_track: int, share_dev, pos_dev, move_dev, precise_pair_dev,
                   columns: Sequence[int], percentiles: Sequence[float], max_lds_rows: int, describe_dev, cycle_max_dev, cycle_mean_dev, step_quantiles_dev,
                   step_count_dev, anomaly_counts_dev, anomaly_mask_dev, stats_dev, scratch_dev, scratch_doubles: int, stream: int = 0):
    """DataAnalyzer's statistics of every experiment of a scan (wtk_replay_analyze); `columns`: WTK_ANALYSIS_COL_* ids; every output is a device tensor
    or None: describe [E, n_cols, 5 + Q], cycle_max / cycle_mean [E, n_log, n_cols], step_quantiles [E, L, n_cols, Q] float64, step_count [E, L, n_cols]
    int32, anomaly_counts [E, 7] and stats [E, 4] int64, anomaly_mask [E, R] uint8."""
    cols, q = np.ascontiguousarray(columns, dtype=np.int32), np.ascontiguousarray(percentiles, dtype=np.float64)
    _check(load().wtk_replay_analyze(C.byref(cfg) if cfg is not None else None, C.byref(acfg) if acfg is not None else None, E, n_cycles, _ptr(track_dev),
                                     n_track, _ptr(share_dev), _ptr(pos_dev), _ptr(move_dev), _ptr(precise_pair_dev), _ptr(cols), len(cols), _ptr(q), len(q),
                                     int(max_lds_rows), _ptr(describe_dev), _ptr(cycle_max_dev), _ptr(cycle_mean_dev), _ptr(step_quantiles_dev),
                                     _ptr(step_count_dev), _ptr(anomaly_counts_dev), _ptr(anomaly_mask_dev), _ptr(stats_dev), _ptr(scratch_dev), scratch_doubles,
                                     C.c_void_p(stream)), "wtk_replay_analyze")


def replay_set_analysis_scratch_doubles(table: ReplaySetTable, E: int, n_cols: int, Q: int) -> int:
    return int(load().wtk_replay_set_analysis_scratch_doubles(table.host, table.T, table.L, E, n_cols, Q))


def replay_set_analyze(cfg: _ReplayConfig, acfg: _AnalysisConfig, table: ReplaySetTable, E: int, track_dev, share_dev, pos_dev, move_dev, precise_rows_dev,
                       columns: Sequence[int], percentiles: Sequence[float], max_lds_rows: int, track_outputs: Sequence, pooled_outputs: Sequence, scratch_dev,
                       scratch_doubles: int, stream: int = 0, geom: Optional[ReplaySetGeometry] = None):
    """DataAnalyzer's statistics of every (track, experiment) of a set scan and of every experiment over the concatenation of its logs
    (wtk_replay_set_analyze).  `track_outputs`: the eight per-track device tensors or None, in the header's order: describe [T, E, n_cols, 5 + Q],
    cycle_max / cycle_mean [E, sum n_log, n_cols], step_quantiles [T, E, L, n_cols, Q], step_count [T, E, L, n_cols] int32, anomaly_counts [T, E, 7]
    int64, anomaly_mask [E, sum R] uint8, stats [T, E, 4] int64.  `pooled_outputs`: the five pooled ones: describe [E, n_cols, 5 + Q], step_quantiles
    [E, L, n_cols, Q], step_count [E, L, n_cols] int32, anomaly_counts [E, 7], stats [E, 4] int64.  precise_rows_dev: float64 [E, sum R] or None."""
    if len(track_outputs) != 8 or len(pooled_outputs) != 5:
        raise WtkError("wtk_replay_set_analyze takes eight per-track and five pooled outputs (None where one is not wanted)")
    cols, q = np.ascontiguousarray(columns, dtype=np.int32), np.ascontiguousarray(percentiles, dtype=np.float64)
    fn, head = (load().wtk_replay_set_analyze, table._args()) if geom is None else (load().wtk_replay_set_analyze_geom, _geom_args(table, geom))
    _check(fn(C.byref(cfg) if cfg is not None else None, C.byref(acfg) if acfg is not None else None, *head, E,
                                         _ptr(track_dev), table.n_super, _ptr(share_dev), _ptr(pos_dev), _ptr(move_dev), _ptr(precise_rows_dev), _ptr(cols),
                                         len(cols), _ptr(q), len(q), int(max_lds_rows), *(_ptr(t) for t in track_outputs), *(_ptr(t) for t in pooled_outputs),
                                         _ptr(scratch_dev), scratch_doubles, C.c_void_p(stream)), "wtk_replay_set_analyze")


def replay_yolo_step(cfg: _ReplayConfig, n_cycles: int, c: int, xywh_dev, share_dev, pos_dev, move_dev, stream: int = 0):
    """The YOLO controller between two single-frame detector calls (wtk_replay_yolo_step): move_dev[c] from the float32 row xywh_dev, pos_dev[c + 1] after
    the cycle's motor steps.  pos_dev / move_dev: int32 [n_cycles, 1, 2] device tensors."""
    _check(load().wtk_replay_yolo_step(C.byref(cfg) if cfg is not None else None, n_cycles, c, _ptr(xywh_dev), _ptr(share_dev), _ptr(pos_dev), _ptr(move_dev),
                                       C.c_void_p(stream)), "wtk_replay_yolo_step")


def replay_yolo_positions(cfg: _ReplayConfig, n_cycles: int, share_dev, pos_dev, move_dev, frame_pos_dev, stream: int = 0):
    """frame_pos_dev int32 [R, 2]: the platform position at every logged frame's camera picture (wtk_replay_yolo_positions)."""
    _check(load().wtk_replay_yolo_positions(C.byref(cfg) if cfg is not None else None, n_cycles, _ptr(share_dev), _ptr(pos_dev), _ptr(move_dev),
                                            _ptr(frame_pos_dev), C.c_void_p(stream)), "wtk_replay_yolo_positions")


def replay_yolo_track(cfg: _ReplayConfig, n_cycles: int, xywh_dev, frame_pos_dev, track_dev, stream: int = 0):
    """View-pixel detections float32 [R, 4] -> the absolute float64 track [R, 4] wtk_replay_rows reads (wtk_replay_yolo_track)."""
    _check(load().wtk_replay_yolo_track(C.byref(cfg) if cfg is not None else None, n_cycles, _ptr(xywh_dev), _ptr(frame_pos_dev), _ptr(track_dev),
                                        C.c_void_p(stream)), "wtk_replay_yolo_track")


def mlp_structure(shapes_relu: Sequence[tuple]):
    """The wtk_mlp_train_layer array of a structure: [(in_dim, out_dim, relu)] in execution order (batch_norm is left 0: the blob does not depend on it)."""
    arr = (_MlpTrainLayer * len(shapes_relu))()
    for i, (k, n, relu) in enumerate(shapes_relu):
        arr[i] = _MlpTrainLayer(int(k), int(n), int(bool(relu)), 0)
    return arr


def mlp_folded_floats(layers, n_blocks: int, layers_per_block: int) -> int:
    """Floats of one model's inference blob (wtk_mlp_folded_floats; needs no device): -1 for a structure wtk_mlp_create refuses."""
    return int(load().wtk_mlp_folded_floats(layers, len(layers), int(n_blocks), int(layers_per_block)))


def mlp_fold_state_host(layers, n_blocks: int, layers_per_block: int, state: np.ndarray) -> np.ndarray:
    """The inference blob of one model's unfolded float32 state (wtk_mlp_fold_state_host; needs no device).  `layers`: a _MlpTrainLayer array
    with the batch_norm flags of the state."""
    F = mlp_folded_floats(layers, n_blocks, layers_per_block)
    if F < 0:
        raise WtkError("wtk_mlp_folded_floats: the structure has no inference blob")
    state = np.ascontiguousarray(state, dtype=np.float32)
    blob = np.empty(F, dtype=np.float32)
    _check(load().wtk_mlp_fold_state_host(layers, len(layers), int(n_blocks), int(layers_per_block), _ptr(state), _ptr(blob)), "wtk_mlp_fold_state_host")
    return blob


def replay_mlp_targets(layers, n_blocks: int, layers_per_block: int, blob_dev, E: int, track32_dev, track_dev, n_track: int, anchors_dev, n_cycles: int,
                       input_frames: Sequence[int], bound: float, a_dev, b_dev, valid_dev, stop_dev=None, stream: int = 0):
    """MLP targets of E device-resident folded models in one call (wtk_replay_mlp_targets): a_dev, b_dev [n_cycles, E, 2], valid_dev [n_cycles, E].
    `bound`: the clip bound of every cycle as a float, or a device float32 [n_cycles] tensor of per-cycle bounds (wtk_replay_mlp_targets_bounds)."""
    inf = np.ascontiguousarray(input_frames, dtype=np.int32)
    if hasattr(bound, "data_ptr"):
        _check(load().wtk_replay_mlp_targets_bounds(layers, len(layers), int(n_blocks), int(layers_per_block), _ptr(blob_dev), int(E), _ptr(track32_dev),
                                                    _ptr(track_dev), int(n_track), _ptr(anchors_dev), int(n_cycles), _ptr(inf), len(inf), _ptr(bound),
                                                    _ptr(a_dev), _ptr(b_dev), _ptr(valid_dev), _ptr(stop_dev), C.c_void_p(stream)),
               "wtk_replay_mlp_targets_bounds")
        return
    _check(load().wtk_replay_mlp_targets(layers, len(layers), int(n_blocks), int(layers_per_block), _ptr(blob_dev), int(E), _ptr(track32_dev), _ptr(track_dev),
                                         int(n_track), _ptr(anchors_dev), int(n_cycles), _ptr(inf), len(inf), C.c_float(bound), _ptr(a_dev), _ptr(b_dev),
                                         _ptr(valid_dev), _ptr(stop_dev), C.c_void_p(stream)), "wtk_replay_mlp_targets")


def replay_mlp_targets_waves(blob_floats: int) -> int:
    """Wavefronts per workgroup wtk_replay_mlp_targets runs next to a blob of that size (before the cap by the number of tiles)."""
    return int(load().wtk_replay_mlp_targets_waves(int(blob_floats)))


# -------------------------------------------------------------------------------------------------
class HipMLP:
    """Device ResMLP (wtk_mlp).  `layers` = list of (W[out,in] fp32, b[out] fp32, relu: bool), BN folded,
    in the order input, block0.l0.., ..., output."""

    def __init__(self, layers: Sequence[tuple], n_blocks: int, layers_per_block: int, device: int = 0):
        lib = load()
        self._keep = []
        arr = (_MlpLayer * len(layers))()
        for i, (w, b, relu) in enumerate(layers):
            w = np.ascontiguousarray(w, dtype=np.float32)
            b = np.ascontiguousarray(b, dtype=np.float32)
            assert w.ndim == 2 and b.shape == (w.shape[0],)
            self._keep += [w, b]
            arr[i] = _MlpLayer(w.shape[1], w.shape[0], int(bool(relu)), 0, _fptr(w), _fptr(b))
        desc = _MlpDesc(device, len(layers), n_blocks, layers_per_block, arr)
        self._h = C.c_void_p()
        _check(lib.wtk_mlp_create(C.byref(self._h), C.byref(desc)), "wtk_mlp_create")
        self.in_dim = int(layers[0][0].shape[1])
        self.out_dim = int(layers[-1][0].shape[0])
        self.device = device

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            load().wtk_mlp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:  # at interpreter shutdown the module globals (load, _lib) may already be gone
            self.close()
        except Exception:
            pass

    def forward_host(self, x: np.ndarray) -> np.ndarray:
        """x: [B, in_dim] float32 (host) -> [B, out_dim] float32 (host)."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        assert x.ndim == 2 and x.shape[1] == self.in_dim
        y = np.empty((x.shape[0], self.out_dim), dtype=np.float32)
        if x.shape[0] == 0:
            return y
        _check(load().wtk_mlp_forward_host(self._h, _ptr(x), x.shape[0], _ptr(y)), "wtk_mlp_forward_host")
        return y

    def forward(self, x_dev, y_dev, batch: int, stream: int = 0):
        """Device tensors (torch) / raw device pointers; asynchronous on `stream` (hipStream_t as int)."""
        _check(load().wtk_mlp_forward(self._h, _ptr(x_dev), batch, _ptr(y_dev), C.c_void_p(stream)), "wtk_mlp_forward")

    def predict_track(self, track_dev, n_frames: int, anchor_frames_dev, n_samples: int, input_frames: Sequence[int],
                      pred_dev, valid_dev=None, stream: int = 0):
        inf = np.ascontiguousarray(input_frames, dtype=np.int32)
        _check(load().wtk_mlp_predict_track(self._h, _ptr(track_dev), n_frames, _ptr(anchor_frames_dev), n_samples,
                                            _ptr(inf), len(inf), _ptr(pred_dev), _ptr(valid_dev), C.c_void_p(stream)),
               "wtk_mlp_predict_track")


# -------------------------------------------------------------------------------------------------
def yolo_conv_table(width: float, depth: float, max_channels: int, nc: int) -> list[dict]:
    """The library's own conv list (name, cout, cin, k, stride, act) — needs no GPU."""
    lib = load()
    n = lib.wtk_yolo_conv_count(width, depth, max_channels, nc)
    if n <= 0:
        raise WtkError("wtk_yolo_conv_count: bad model scale")
    out = []
    for i in range(n):
        co, ci, k, s, a = (C.c_int32() for _ in range(5))
        name = C.create_string_buffer(96)
        _check(lib.wtk_yolo_conv_info(width, depth, max_channels, nc, i, C.byref(co), C.byref(ci), C.byref(k), C.byref(s),
                                      C.byref(a), name, 96), "wtk_yolo_conv_info")
        out.append(dict(name=name.value.decode(), cout=co.value, cin=ci.value, k=k.value, stride=s.value, act=a.value))
    return out


STATUS_NONFINITE = 1
PLANS = {"auto": 0, "throughput": 1, "latency": 2}
PLAN_C2F_TAIL = 0x100  # WTK_PLAN_C2F_TAIL, a flag next to the plan


class HipYolo:
    """Device YOLOv8 detector (wtk_yolo) for one network input size.

    weights: dict name -> (W[cout,k,k,cin] fp32 O-H-W-I, b[cout] fp32) for every conv of
    wtracker_amd.yolo_spec.conv_table(scale, nc)."""

    def __init__(self, weights: dict, imgsz: tuple[int, int], max_batch: int, dtype: str = "fp16", nc: int = 1,
                 width: float = 0.5, depth: float = 0.33, max_channels: int = 1024, device: int = 0, plan: str = "auto"):
        """plan: "auto" (latency when max_batch <= 4 and the dtype is fp32 / f16x3, else throughput; WTK_LATENCY_PLAN=0/1 overrides), "throughput" or
        "latency" (include/wtk_hip.h: wtk_yolo_create_planned) — fixed for the handle's life, so a frame's result does not depend on the batch it is in."""
        lib = load()
        if plan not in PLANS:
            raise WtkError(f"plan must be one of {sorted(PLANS)}")
        table = yolo_conv_table(width, depth, max_channels, nc)
        arr = (_ConvBlob * len(table))()
        self._keep = []
        for i, t in enumerate(table):
            if t["name"] not in weights:
                raise WtkError(f"missing weights for conv {t['name']}")
            w, b = weights[t["name"]]
            w = np.ascontiguousarray(w, dtype=np.float32)
            b = np.ascontiguousarray(b, dtype=np.float32)
            if w.shape != (t["cout"], t["k"], t["k"], t["cin"]) or b.shape != (t["cout"],):
                raise WtkError(f"conv {t['name']}: expected weight {(t['cout'], t['k'], t['k'], t['cin'])}, got {w.shape}")
            self._keep += [w, b]
            arr[i] = _ConvBlob(t["cout"], t["cin"], t["k"], t["stride"], t["act"], 0, _fptr(w), _fptr(b))
        desc = _YoloDesc(device, DTYPES[dtype], int(imgsz[0]), int(imgsz[1]), int(max_batch), nc, width, depth, max_channels,
                         len(table), arr)
        self._h = C.c_void_p()
        # every handle made here asks for model.2.cv2 inside model.2.m.0.cv2's kernel (include/wtk_hip.h: WTK_PLAN_C2F_TAIL; handles it does not apply to ignore it)
        rc = lib.wtk_yolo_create_planned(C.byref(self._h), C.byref(desc), PLANS[plan] | PLAN_C2F_TAIL)
        _check(rc, "wtk_yolo_create_planned")
        self.plan = "latency" if lib.wtk_yolo_plan(self._h) == PLANS["latency"] else "throughput"
        self._keep = []  # the library copied everything to the device
        self.imgsz = (int(imgsz[0]), int(imgsz[1]))
        self.max_batch = int(max_batch)
        self.dtype = dtype
        self.nc = nc
        self.device = device
        macs, anchors = C.c_double(), C.c_int32()
        _check(lib.wtk_yolo_workload(self._h, C.byref(macs), C.byref(anchors)), "wtk_yolo_workload")
        self.macs_per_frame = macs.value
        self.anchors = anchors.value

    def close(self):
        for d in self.__dict__.pop("_dependents", []):  # native objects that borrow this handle (wtk_hybrid) go first
            d._release()
        if getattr(self, "_h", None) is not None and self._h:
            load().wtk_yolo_destroy(self._h)
            self._h = None

    def __del__(self):
        try:  # at interpreter shutdown the module globals (load, _lib) may already be gone
            self.close()
        except Exception:
            pass

    def predict_host(self, frames: np.ndarray, conf: float = 0.1, iou: float = 0.7, max_det: int = 1):
        """frames: uint8 [B,H,W] or [B,H,W,C] (host).  Returns (xywh [B,4] f32 with NaN rows, conf [B], anchor [B])."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        if frames.ndim == 3:
            frames = frames[..., None]
        B, H, W, Cc = frames.shape
        xywh = np.empty((B, 4), dtype=np.float32)
        cf = np.empty((B,), dtype=np.float32)
        an = np.empty((B,), dtype=np.int32)
        _check(load().wtk_yolo_predict_host(self._h, _ptr(frames), B, H, W, Cc, conf, iou, max_det, _ptr(xywh), _ptr(cf),
                                            _ptr(an)), "wtk_yolo_predict_host")
        return xywh, cf, an

    def predict(self, frames_dev, B: int, H: int, W: int, Cc: int, out_xywh, out_conf=None, out_anchor=None,
                conf: float = 0.1, iou: float = 0.7, max_det: int = 1, stream: int = 0):
        """Device pointers / torch CUDA tensors; asynchronous on `stream`."""
        _check(load().wtk_yolo_predict(self._h, _ptr(frames_dev), B, H, W, Cc, conf, iou, max_det, _ptr(out_xywh),
                                       _ptr(out_conf), _ptr(out_anchor), C.c_void_p(stream)), "wtk_yolo_predict")

    def status(self, clear: bool = False) -> int:
        """Range-guard flags (include/wtk_hip.h: WTK_STATUS_NONFINITE = 1, sticky, raised by the head kernels when a head logit is inf / NaN — an
        activation left the fp16 range somewhere in the network).  No device call: valid for the work the
        caller has synchronised with."""
        f = C.c_int32()
        _check(load().wtk_yolo_status(self._h, C.byref(f), int(clear)), "wtk_yolo_status")
        return f.value

    def set_dynamic_batch(self, n_dev):
        """`n_dev`: device int32 scalar (tensor / pointer) holding the number of batch rows that matter in the following calls, or None."""
        _check(load().wtk_yolo_set_dynamic_batch(self._h, _ptr(n_dev)), "wtk_yolo_set_dynamic_batch")

    def set_side_streams(self, n: int):
        """Streams the forward pass spreads over besides the caller's: 2 (default: P3 / P4 Detect towers on a side stream each), 1 or 0."""
        _check(load().wtk_yolo_set_side_streams(self._h, n), "wtk_yolo_set_side_streams")

    def last_margins(self, B: int) -> np.ndarray:
        """Decision margins (class-logit units) of the B frames of the last max_det = 1 call: min(best - second-best anchor logit,
        |best - logit(conf)|) — small values mark frames on which a perturbation of the logits could change the result."""
        out = np.empty((B,), dtype=np.float32)
        _check(load().wtk_yolo_last_margins_host(self._h, B, _ptr(out)), "wtk_yolo_last_margins_host")
        return out

    def margin_buffer(self) -> int:
        """Device address of the handle's [max_batch] float margin buffer (for device-resident pipelines)."""
        p = C.c_void_p()
        _check(load().wtk_yolo_margin_buffer(self._h, C.byref(p)), "wtk_yolo_margin_buffer")
        return int(p.value)

    def predict_nms(self, frames_dev, B: int, H: int, W: int, Cc: int, max_det: int, out_xywh, out_conf=None, out_cls=None, out_anchor=None,
                    out_count=None, conf: float = 0.1, iou: float = 0.7, stream: int = 0):
        """General greedy NMS, up to `max_det` boxes per frame (wtk_yolo_predict_nms); outputs [B,max_det,...] device tensors."""
        _check(load().wtk_yolo_predict_nms(self._h, _ptr(frames_dev), B, H, W, Cc, conf, iou, max_det, _ptr(out_xywh), _ptr(out_conf),
                                           _ptr(out_cls), _ptr(out_anchor), _ptr(out_count), C.c_void_p(stream)), "wtk_yolo_predict_nms")

    def decode_nms_host(self, box: np.ndarray, cls: np.ndarray, H: int, W: int, max_det: int, conf: float = 0.1, iou: float = 0.7):
        """NMS on given head logits -> (xywh [B,max_det,4], conf [B,max_det], cls [B,max_det], anchor [B,max_det], count [B])."""
        box = np.ascontiguousarray(box, dtype=np.float32)
        cls = np.ascontiguousarray(cls, dtype=np.float32)
        B = box.shape[0]
        assert box.shape == (B, self.anchors, 64) and cls.shape == (B, self.anchors, self.nc)
        xywh = np.empty((B, max_det, 4), dtype=np.float32)
        cf = np.empty((B, max_det), dtype=np.float32)
        kc = np.empty((B, max_det), dtype=np.int32)
        an = np.empty((B, max_det), dtype=np.int32)
        cnt = np.empty((B,), dtype=np.int32)
        _check(load().wtk_yolo_decode_nms_host(self._h, _ptr(box), _ptr(cls), B, H, W, conf, iou, max_det, _ptr(xywh), _ptr(cf), _ptr(kc), _ptr(an),
                                               _ptr(cnt)), "wtk_yolo_decode_nms_host")
        return xywh, cf, kc, an, cnt

    def predict_views(self, frames_dev, n_frames: int, H: int, W: int, Cc: int, frame_index_dev, pos_xy_dev, B: int, view_w: int,
                      view_h: int, out_xywh, out_conf=None, out_anchor=None, conf: float = 0.1, iou: float = 0.7, max_det: int = 1,
                      stream: int = 0):
        """Detector on the (view_w x view_h) camera views of device-resident full frames (crop + letterbox fused on the
        device; wtk_yolo_predict_views).  frame_index_dev [B] int32 or None, pos_xy_dev [B,2] int32; boxes in view pixels."""
        _check(load().wtk_yolo_predict_views(self._h, _ptr(frames_dev), n_frames, H, W, Cc, _ptr(frame_index_dev), _ptr(pos_xy_dev), B,
                                             view_w, view_h, conf, iou, max_det, _ptr(out_xywh), _ptr(out_conf), _ptr(out_anchor),
                                             C.c_void_p(stream)), "wtk_yolo_predict_views")

    def debug_head(self, B: int):
        """Raw head logits of the last forward: (box [B,A,64], cls [B,A,nc]) fp32, levels concatenated."""
        lib = load()
        boxes, clss = [], []
        S_h, S_w = self.imgsz
        for lvl, s in enumerate((8, 16, 32)):
            A = (S_h // s) * (S_w // s)
            bx = np.empty((B, A, 64), dtype=np.float32)
            cl = np.empty((B, A, self.nc), dtype=np.float32)
            _check(lib.wtk_yolo_debug_head(self._h, lvl, B, _ptr(bx), _ptr(cl)), "wtk_yolo_debug_head")
            boxes.append(bx)
            clss.append(cl)
        return np.concatenate(boxes, 1), np.concatenate(clss, 1)

    def debug_tensor(self, conv_index: int, B: int, raw: bool = False) -> np.ndarray:
        """Output of conv blob `conv_index` (yolo_conv_table order) of the last forward: fp32 [B,h,w,cout].  raw: as the pass left it — a Detect
        box-tower conv is not completed densely after a sparse pass (WTK_DEBUG_RAW), so only the tiles under the survivors hold that pass's values."""
        lib = load()
        if raw:
            conv_index = -2 - conv_index
        shp = (C.c_int32 * 3)()
        _check(lib.wtk_yolo_debug_tensor(self._h, conv_index, B, None, 0, shp), "wtk_yolo_debug_tensor")
        out = np.empty((B, shp[0], shp[1], shp[2]), dtype=np.float32)
        _check(lib.wtk_yolo_debug_tensor(self._h, conv_index, B, _ptr(out), out.size, shp), "wtk_yolo_debug_tensor")
        return out

    def sparse_counts(self):
        """(tiles listed for box.0, for box.1 + box.2, grid of the box.0 launch, of the box.1 + box.2 launch) of the last list-form sparse pass."""
        return tuple(int(v) for v in self.debug_tensor(-1, 1).ravel())  # WTK_DEBUG_SPARSE_COUNTS

    def decode_host(self, box: np.ndarray, cls: np.ndarray, H: int, W: int, conf: float = 0.1):
        box = np.ascontiguousarray(box, dtype=np.float32)
        cls = np.ascontiguousarray(cls, dtype=np.float32)
        B = box.shape[0]
        assert box.shape == (B, self.anchors, 64) and cls.shape == (B, self.anchors, self.nc)
        xywh = np.empty((B, 4), dtype=np.float32)
        cf = np.empty((B,), dtype=np.float32)
        an = np.empty((B,), dtype=np.int32)
        _check(load().wtk_yolo_decode_host(self._h, _ptr(box), _ptr(cls), B, H, W, conf, _ptr(xywh), _ptr(cf), _ptr(an)),
               "wtk_yolo_decode_host")
        return xywh, cf, an

    def set_profiling(self, enabled: bool):
        _check(load().wtk_yolo_set_profiling(self._h, int(enabled)), "wtk_yolo_set_profiling")

    def get_profile(self) -> dict:
        names = ["stem", "conv", "pool", "head"]
        out = {}
        for i, nme in enumerate(names):
            ms, n = C.c_double(), C.c_int64()
            _check(load().wtk_yolo_get_profile(self._h, i, C.byref(ms), C.byref(n)), "wtk_yolo_get_profile")
            out[nme] = dict(total_ms=ms.value, launches=n.value)
        return out

    KERNELS = ["stem_mfma_kernel", "conv_igemm_kernel+conv1x1_wide_kernel", "sppf_pool_kernel", "head", "conv3x3_halo_kernel",
               "front_fused_kernel+c2f32_fused_kernel", "conv3x3_c32_kernel", "conv3x3_halo_kernel(sparse box towers)"]

    def get_kernel_profile(self) -> dict:
        """Per-kernel device time, launches and algorithmic FLOPs of the profiled forwards (wtk_yolo_get_kernel_profile)."""
        out = {}
        for i, nme in enumerate(self.KERNELS):
            ms, n, fl = C.c_double(), C.c_int64(), C.c_double()
            _check(load().wtk_yolo_get_kernel_profile(self._h, i, C.byref(ms), C.byref(n), C.byref(fl)), "wtk_yolo_get_kernel_profile")
            out[nme] = dict(total_ms=ms.value, launches=n.value, flops=fl.value)
        return out
