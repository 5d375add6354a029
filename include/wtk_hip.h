/*
 * wtk_hip.h — C ABI of libwtk_hip.so, the MI355X (gfx950) implementation of WTracker's
 * per-frame detection + prediction hot path.
 *
 * The reference (giladfrid009/WTracker) is pure Python and has no FFI; the interfaces this
 * library stands in for are the Python methods cited at each entry point (paths relative to the
 * reference repository root).  INTEGRATION.md shows the ctypes binding a WTracker maintainer
 * would add to call these from the reference's own controllers.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on error; wtk_last_error() returns a
 *     thread-local, NUL-terminated description of the last failure on the calling thread;
 *   - plain pointers and sizes only; `stream` arguments are a hipStream_t passed as void*
 *     (NULL = the default stream);
 *   - a handle owns its weights and workspace (device memory); callers own all I/O buffers;
 *   - a handle is not re-entrant: use one handle per stream / thread;
 *   - "no detection" is not an error: the bbox row is 4 x NaN (yolo_controller.py:84-85).
 */
#ifndef WTK_HIP_H
#define WTK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WTK_ABI_VERSION 7 /* 7: + wtk_yolo_create_planned / wtk_yolo_plan, wtk_yolo_status (additive); 2: + wtk_yolo_predict_views / _nms, wtk_track_*, wtk_comm_*; 3: + WTK_F16X3, wtk_recheck_*; 4: + wtk_recheck_select_counted; 5: + wtk_recheck_enqueue / _scatter; 6: + wtk_hybrid_*; still 7: + wtk_background, wtk_precise_error (additive: every earlier entry point is unchanged); still 7: + wtk_polyfit_*; still 7: + wtk_replay_* (additive); still 7: + wtk_replay_polyfit_targets / _scratch_doubles, wtk_replay_objective (additive); still 7: + wtk_replay_yolo_step / _positions / _track (additive); still 7: + wtk_mlp_trainer_* (additive); still 7: + wtk_mlp_folded_floats / _fold_state_host, wtk_mlp_trainer_fold / _keep_scored / _get_scores, wtk_replay_mlp_targets / _waves (additive) */

typedef enum wtk_dtype {
    WTK_F32 = 0, /* fp32 storage, exact-fp32 MFMA (v_mfma_f32_16x16x4_f32): parity mode   */
    WTK_F16 = 1, /* fp16 storage, fp16 MFMA (v_mfma_f32_16x16x32_f16) with fp32 accumulate */
    WTK_F16X3 = 2 /* split-fp16 storage (hi + lo * 2^-11 pairs), three fp16 MFMAs per product: fp32-grade results (the error of a plain
                     fp32 dot product) from the fp16 matrix pipe.  Channel widths in multiples of 64 (YOLOv8 s / l).                     */
} wtk_dtype;

const char *wtk_last_error(void);
int wtk_abi_version(void);
/* Number of visible HIP devices (0 when there is none); never fails. */
int wtk_device_count(void);

/* ------------------------------------------------------------------------------------------
 * ResMLP trajectory predictor.
 * Replaces: WormPredictor.forward -> RMLP.forward   wtracker/neural/mlp.py:47-48,176-188
 *           (MLPLayer = Linear+BatchNorm1d(eval)+ReLU, mlp.py:67-71; MlpBlock, mlp.py:121-126)
 * ------------------------------------------------------------------------------------------ */
typedef struct wtk_mlp wtk_mlp;

/* One folded affine layer  y = act(W x + b).  BatchNorm1d running statistics are folded into
 * (W, b) by the caller (eval mode, mlp_controllers.py:29).  W is row-major [out_dim][in_dim]. */
typedef struct wtk_mlp_layer {
    int32_t in_dim;
    int32_t out_dim;
    int32_t relu;        /* 1: ReLU after the affine */
    int32_t reserved;
    const float *weight; /* host pointer, [out_dim][in_dim] */
    const float *bias;   /* host pointer, [out_dim]         */
} wtk_mlp_layer;

typedef struct wtk_mlp_desc {
    int32_t device;           /* HIP device ordinal */
    int32_t n_layers;         /* total: 1 (input) + n_blocks*layers_per_block + 1 (output) */
    int32_t n_blocks;         /* residual blocks: h <- h + block(h)   (mlp.py:185-187)      */
    int32_t layers_per_block; /* 4 in both shipped models                                    */
    const wtk_mlp_layer *layers; /* order: input, block0.l0..l3, block1..., output           */
} wtk_mlp_desc;

int wtk_mlp_create(wtk_mlp **out, const wtk_mlp_desc *desc);
void wtk_mlp_destroy(wtk_mlp *h);
/* y[B][out] = model(x[B][in]); x and y are DEVICE pointers, fp32 row-major. */
int wtk_mlp_forward(wtk_mlp *h, const float *x_dev, int32_t batch, float *y_dev, void *stream);
/* Same with HOST pointers (synchronous): what MLPController.provide_movement_vector needs for
 * its single [1,28] sample (mlp_controllers.py:59). */
int wtk_mlp_forward_host(wtk_mlp *h, const float *x_host, int32_t batch, float *y_host);

/* Batched open-loop form of MLPController.provide_movement_vector (mlp_controllers.py:36-68)
 * over a device-resident track: for every sample s with anchor frame t = anchor_frames[s]
 * gather the boxes track[t + input_frames[j]] (j < n_in; out-of-range or non-finite -> the
 * sample is flagged invalid, mlp_controllers.py:43-44), subtract box 0's x/y from every x/y
 * (mlp_controllers.py:50-56), run the model.  pred[s] = raw model output (dx, dy) before the
 * host-side clip/round; valid[s] = 1/0.  track is [n_frames][4] fp32 xywh (absolute coords). */
int wtk_mlp_predict_track(wtk_mlp *h, const float *track_dev, int32_t n_frames,
                          const int32_t *anchor_frames_dev, int32_t n_samples,
                          const int32_t *input_frames_host, int32_t n_in,
                          float *pred_dev /*[n_samples][2]*/, int32_t *valid_dev /*[n_samples]*/,
                          void *stream);

/* ------------------------------------------------------------------------------------------
 * Training a population of ResMLP predictors, one workgroup per model.
 * Replaces: MLPTrainer.train_batch / test_batch / fit   wtracker/neural/training.py:61-130,267-333
 *           over RMLP in train mode                      wtracker/neural/mlp.py:51-188
 *           with the optimizers of neural/config.py:28-33 (lr and weight_decay given, the rest torch's defaults).
 *
 * State of ONE model, `n_state` floats: for every layer in execution order W [out][in], b [out] and, with BatchNorm, gamma [out], beta [out]
 *     (the n_train trainable floats); behind them, for every BatchNorm layer in order, running_mean [out], running_var [out].
 *     num_batches_tracked is the handle's step counter (the caller adds it to the initial value).
 * Every call trains / evaluates all n_models models in ONE launch on `stream`; x / y are shared device arrays [n][in] / [n][out] fp32.
 *   grad        train-mode forward + backward of one batch (rows 0 .. batch - 1): grad_dev [n_models][n_train], loss_dev [n_models].  No step, no statistics update.
 *   train_epoch model e walks rows order_dev[e][0 .. n - 1] (null: 0 .. n - 1) in batches of batch_size (the last may be partial): forward, loss, backward,
 *               optimizer step with lr_dev[e] / weight_decay_dev[e].  An order entry outside [0, n) is clamped into it (no load leaves x / y): callers validate.  loss_dev / num_correct_dev [n_models][ceil(n / batch_size)]; num_correct = samples with
 *               ||pred - y||_2 < 1 (training.py:317).  Models with active_dev[e] == 0 are skipped (active_dev null: all run).
 *   step        train_epoch with n = batch and no order: the same bits.
 *   eval_epoch  eval-mode forward (running statistics) of rows 0 .. n - 1 in batches; pred_dev [n_models][n][out] (optional).  track_best != 0 keeps the early-stopping
 *               state of training.py:119-128 per model (2: forget the state of earlier calls first, as a new Trainer.fit starts from best_val_loss = None):
 *               curr = the batch losses added in fp32 in batch order, divided by their number; curr < best (strict) copies the state to the best slot and resets the
 *               counter, otherwise the counter grows and, with patience > 0 and counter >= patience, active_dev[e] is cleared.
 *   get_state   which = 0 state, 1 best state ([n_models][n_state]), 2 / 3 first / second optimizer moment ([n_models][n_train]); steps_host [n_models] (optional) =
 *               optimizer steps taken (which = 1: at the best state).  Synchronises `stream`.
 * Refused: widths above 128, more than 64 layers, an activation other than ReLU / none, a loss other than mse / l1, batch_size outside [1, max_batch <= 1024],
 *     and, for a model with BatchNorm, a batch of one sample (batch_size 1 or a last partial batch of 1): train-mode BatchNorm needs more than 1 value per channel.
 * ------------------------------------------------------------------------------------------ */
typedef struct wtk_mlp_trainer wtk_mlp_trainer;
typedef struct wtk_mlp_train_layer {
    int32_t in_dim;
    int32_t out_dim;
    int32_t relu;       /* 1: ReLU, 0: none */
    int32_t batch_norm; /* 1: BatchNorm1d between the Linear and the activation */
} wtk_mlp_train_layer;
#define WTK_LOSS_MSE 0
#define WTK_LOSS_L1 1
#define WTK_OPT_ADAM 0
#define WTK_OPT_ADAMW 1
#define WTK_OPT_SGD 2
#define WTK_OPT_RMSPROP 3
typedef struct wtk_mlp_trainer_desc {
    int32_t device;
    int32_t n_models;
    int32_t n_layers; /* 1 (input) + n_blocks * layers_per_block + 1 (output) */
    int32_t n_blocks;
    int32_t layers_per_block;
    int32_t loss;      /* WTK_LOSS_* */
    int32_t optimizer; /* WTK_OPT_*  */
    int32_t max_batch; /* largest batch_size of any later call */
    const wtk_mlp_train_layer *layers;
    const float *state; /* host, [n_models][n_state]: the initial state of every model */
} wtk_mlp_trainer_desc;
int64_t wtk_mlp_trainer_state_floats(const wtk_mlp_trainer_desc *desc, int64_t *n_train_out);
int wtk_mlp_trainer_create(wtk_mlp_trainer **out, const wtk_mlp_trainer_desc *desc);
void wtk_mlp_trainer_destroy(wtk_mlp_trainer *h);
int wtk_mlp_trainer_grad(wtk_mlp_trainer *h, const float *x_dev, const float *y_dev, int32_t batch, float *grad_dev, float *loss_dev, void *stream);
int wtk_mlp_trainer_step(wtk_mlp_trainer *h, const float *x_dev, const float *y_dev, int32_t batch, const double *lr_dev, const double *weight_decay_dev,
                         float *loss_dev, int32_t *num_correct_dev, void *stream);
int wtk_mlp_trainer_train_epoch(wtk_mlp_trainer *h, const float *x_dev, const float *y_dev, int32_t n, const int32_t *order_dev, int32_t batch_size,
                                const double *lr_dev, const double *weight_decay_dev, int32_t *active_dev, float *loss_dev, int32_t *num_correct_dev,
                                void *stream);
int wtk_mlp_trainer_eval_epoch(wtk_mlp_trainer *h, const float *x_dev, const float *y_dev, int32_t n, int32_t batch_size, int32_t patience,
                               int32_t track_best, int32_t *active_dev, float *loss_dev, int32_t *num_correct_dev, float *pred_dev, void *stream);
int wtk_mlp_trainer_get_state(wtk_mlp_trainer *h, int32_t which, float *state_host, int32_t *steps_host, void *stream);
int wtk_mlp_trainer_get_stopping(wtk_mlp_trainer *h, float *best_loss_host, int32_t *has_best_host, int32_t *no_improve_host, void *stream);

/* ------------------------------------------------------------------------------------------
 * A trained population as inference parameters, and the best state by a caller's score.
 * Blob of ONE model, wtk_mlp_folded_floats(...) floats: what wtk_mlp_create builds from folded layers — per layer W [out_pad][in_pad] (in_pad = in_dim
 *     rounded up to 4, out_pad = out_dim rounded up to 16, padding 0), then b [out_pad]; the whole rounded up to 4 floats.
 * The fold is resmlp._fold's, bit for bit: float64 arithmetic cast to float32 at the end, s = gamma / sqrt(running_var + 1e-5), W' = W s,
 *     b' = (b - running_mean) s + beta (product and sum rounded separately); layers without BatchNorm pass through unchanged.
 *   folded_floats    the blob size of a structure (batch_norm is not looked at), -1 for a structure wtk_mlp_create refuses.  Needs no device.
 *   fold_state_host  blob_host = the fold of one model's state_host (the layout above wtk_mlp_trainer_create).  Needs no device: the same function the
 *                    device runs, compiled for the host.
 *   trainer_fold     blob_dev [n_models][folded_floats] = the fold of every model's state, one launch on `stream`; which = 0 the current state, 1 the best
 *                    state by validation loss, 4 the best state by score (refused before the first keep_scored call).
 *   keep_scored      for every model with active_dev[e] != 0 (null: all): where score_dev[e] is finite and strictly below the stored score, or no score is
 *                    stored yet, the current state and step count are copied to a third slot and the score is stored.  NaN and +-inf never win; a tie keeps
 *                    the earlier state.  One launch on `stream`.  The slot (n_models x n_state floats) is allocated and filled with the initial state by the
 *                    FIRST call: that call allocates device memory and uploads; later calls only launch.
 *   get_state        which = 4 reads the slot (steps_host: the steps at the kept state); before any keep_scored call it is the initial state.
 *   get_scores       best_score_host [n_models] (NaN where has_score_host[e] == 0).  Synchronises `stream`.
 * ------------------------------------------------------------------------------------------ */
int64_t wtk_mlp_folded_floats(const wtk_mlp_train_layer *layers, int32_t n_layers, int32_t n_blocks, int32_t layers_per_block);
int wtk_mlp_fold_state_host(const wtk_mlp_train_layer *layers, int32_t n_layers, int32_t n_blocks, int32_t layers_per_block, const float *state_host,
                            float *blob_host);
int wtk_mlp_trainer_fold(wtk_mlp_trainer *h, int32_t which, float *blob_dev /*[n_models][folded_floats]*/, void *stream);
int wtk_mlp_trainer_keep_scored(wtk_mlp_trainer *h, const double *score_dev /*[n_models]*/, const int32_t *active_dev, void *stream);
int wtk_mlp_trainer_get_scores(wtk_mlp_trainer *h, double *best_score_host, int32_t *has_score_host, void *stream);

/* ------------------------------------------------------------------------------------------
 * YOLOv8 detector (single image size per handle).
 * Replaces: YoloController.predict          wtracker/sim/sim_controllers/yolo_controller.py:64-90
 *           i.e. ultralytics YOLO.predict(source=frames, max_det=1, imgsz=..., conf=...):
 *           letterbox + BGR->RGB + /255, DetectionModel forward, DFL decode,
 *           non_max_suppression, scale_boxes, xyxy -> xywh.
 * ------------------------------------------------------------------------------------------ */
typedef struct wtk_yolo wtk_yolo;

/* One fused conv (Conv2d + folded BatchNorm2d [+ SiLU]).  Weight layout is O-H-W-I:
 * [cout][kh][kw][cin] fp32 (cin fastest).  The conv list order is fixed; see
 * wtk_yolo_conv_count / wtk_yolo_conv_info. */
typedef struct wtk_conv_blob {
    int32_t cout, cin, k, stride;
    int32_t act; /* 1: SiLU, 0: linear (the Detect heads' last 1x1) */
    int32_t reserved;
    const float *weight; /* host pointer */
    const float *bias;   /* host pointer, [cout] */
} wtk_conv_blob;

typedef struct wtk_yolo_desc {
    int32_t device;
    int32_t dtype;      /* wtk_dtype */
    int32_t imgsz_h;    /* network input height (multiple of 32) */
    int32_t imgsz_w;    /* network input width  (multiple of 32) */
    int32_t max_batch;  /* frames per forward pass the workspace is sized for */
    int32_t nc;         /* number of classes, 1 .. 80 (1 for the worm detector, yolo_train_config.yaml:27; 80 = a stock YOLOv8 head) */
    float width_mult;   /* 0.50 for YOLOv8s.  Width rule: every channel width of the scale (64, 128, 256, 512, 1024, each capped at max_channels, times
                         * width_mult, rounded up to 8) a multiple of 16, and the stem (the first of them) at most 64: YOLOv8 n, s, m and l.  wtk_yolo_create
                         * refuses YOLOv8x (width 1.25: an 80-channel stem) with a message that names the stem width and the limit.  WTK_F16X3: multiples
                         * of 64 (stem: 32 or 64), i.e. s and l. */
    float depth_mult;   /* 0.33 for YOLOv8s */
    int32_t max_channels; /* 1024 for YOLOv8s */
    int32_t n_convs;    /* must equal wtk_yolo_conv_count(width, depth, maxch, nc) */
    const wtk_conv_blob *convs;
} wtk_yolo_desc;

/* Number / description of the fused convs a model of this scale has, in the order the blob
 * table must follow.  name_out receives e.g. "model.2.m.0.cv1" (ultralytics module path). */
int wtk_yolo_conv_count(float width_mult, float depth_mult, int32_t max_channels, int32_t nc);
int wtk_yolo_conv_info(float width_mult, float depth_mult, int32_t max_channels, int32_t nc,
                       int32_t index, int32_t *cout, int32_t *cin, int32_t *k, int32_t *stride,
                       int32_t *act, char *name_out, size_t name_cap);

int wtk_yolo_create(wtk_yolo **out, const wtk_yolo_desc *desc);
void wtk_yolo_destroy(wtk_yolo *h);
/* The same with the launch plan named by the caller.  A handle is planned ONCE, for one of two regimes:
 *   WTK_PLAN_THROUGHPUT  large batches (BASELINE configs 3-5): window / implicit-GEMM kernels with big tiles, fused Detect tails;
 *   WTK_PLAN_LATENCY     the reference's own operating point — one call of cycle_frame_num (9 / 15) frames and one single-frame
 *                        call per cycle at imgsz 384 (yolo_controller.py:96-98,108-109; initialize_experiment.ipynb: imgsz 384):
 *                        every conv is cut along K as well (split-K implicit GEMM + a slab-combining pass), so that a layer of a
 *                        few thousand pixels still runs on every CU, and the convs of one dependency level of the network (a Detect
 *                        tower's box and class convs, a PAN layer and the tower of the feature map before it) run as ONE launch on
 *                        the caller's stream: 48 dependent launches per YOLOv8s forward, no side streams.  WTK_F32 and WTK_F16X3
 *                        only (WTK_F16 handles stay on the throughput plan).
 *   WTK_PLAN_AUTO        (= wtk_yolo_create) latency when max_batch <= 4 and the dtype allows it, else throughput (measured on MI355X at imgsz 384:
 *                        B = 1 0.51 ms against 0.67-1.00 ms on the throughput plan, B = 15 1.5 ms against 1.1 ms — the cross-over lies near B = 6); the
 *                        environment variable WTK_LATENCY_PLAN=0 / 1 overrides AUTO only.
 * The first eager call of a latency-plan handle at a batch size also TIMES its launch choices (every grouped launch's tile / form candidates, inside the real
 * forward pass: ~0.1 s once; WTK_SK_AUTOTUNE=0 keeps the cost model's); the choice changes no result bit.
 * Launches are eager.
 * The plan never changes per call: within a handle a frame's logits do not depend on the batch it arrives in.  Both plans meet the
 * same tolerances against the fp32 restatement; they are not bit-identical to each other (K is summed in a different order).
 * WTK_PLAN_C2F_TAIL is a flag, or'ed into any of the three: on WTK_F16X3 throughput-plan handles of more than 16 frames the first C2f's closing 1x1
 * (model.2.cv2) runs inside the kernel of the 3x3 before it (model.2.m.0.cv2), whose output then never reaches memory — one launch and 0.64 GB of
 * traffic per 64 frames at 640 x 640 fewer, every result bit kept.  Other handles ignore it.  A flag and not the default because it changes what such a
 * handle launches; the Python binding always sets it.  WTK_NO_C2F_SPLIT_TAIL=1 in the environment overrides it (A/B). */
typedef enum wtk_plan { WTK_PLAN_AUTO = 0, WTK_PLAN_THROUGHPUT = 1, WTK_PLAN_LATENCY = 2, WTK_PLAN_C2F_TAIL = 0x100 } wtk_plan;
int wtk_yolo_create_planned(wtk_yolo **out, const wtk_yolo_desc *desc, int32_t plan);
/* The plan a handle runs on: WTK_PLAN_THROUGHPUT or WTK_PLAN_LATENCY (-1 on a null handle). */
int wtk_yolo_plan(wtk_yolo *h);

/* frames: DEVICE pointer, uint8, [B][H][W][C] with C = 1 (gray; replicated to 3 channels as
 * yolo_controller.py:68-69 does) or C = 3 (BGR).  H x W is letterboxed to imgsz_h x imgsz_w
 * (identity when equal): resized by r = min(imgsz_h / H, imgsz_w / W) and padded with 114 to exactly imgsz_h x imgsz_w, the image
 * centred (LetterBox(auto=False)).  One exception makes a handle created at the reference's own network shape for these frames
 * (LetterBox(auto=True) at imgsz S = max(imgsz_h, imgsz_w): wtracker_amd.yolo_spec.letterbox_shape) resize as the reference does:
 * where r' = min(S / H, S / W) gives a resized image that still fits the handle, r' is used.  The two differ only when the short
 * side's product rounds DOWN onto the handle's side (435 x 579 into 288 x 384: 288 x 384, not 288 x 383).  The boxes are mapped
 * back as scale_boxes does, from the two shapes alone.  Outputs (DEVICE pointers, may be NULL except out_xywh):
 *   out_xywh   [B][4] fp32: x_topleft, y_topleft, w, h in input-image pixels; 4 x NaN = none
 *   out_conf   [B]    fp32: score of the kept detection (0 when none)
 *   out_anchor [B]    int32: anchor index of the kept detection (-1 when none)
 * conf/iou/max_det follow non_max_suppression; max_det must be 1 (yolo_controller.py:76). */
int wtk_yolo_predict(wtk_yolo *h, const uint8_t *frames_dev, int32_t B, int32_t H, int32_t W,
                     int32_t C, float conf, float iou, int32_t max_det, float *out_xywh,
                     float *out_conf, int32_t *out_anchor, void *stream);
/* Same with HOST pointers for frames and outputs (synchronous; PCIe-inclusive). */
int wtk_yolo_predict_host(wtk_yolo *h, const uint8_t *frames_host, int32_t B, int32_t H,
                          int32_t W, int32_t C, float conf, float iou, int32_t max_det,
                          float *out_xywh, float *out_conf, int32_t *out_anchor);

/* Test / profiling hooks: raw head outputs of the last forward pass, copied to HOST as fp32.
 *   level 0..2 -> stride 8/16/32.  box: [B][h*w][64] DFL logits; cls: [B][h*w][nc] logits. */
int wtk_yolo_debug_head(wtk_yolo *h, int32_t level, int32_t B, float *box_host, float *cls_host);
/* Test hook: the output tensor of conv blob `conv_index` (wtk_yolo_conv_info order) after the last forward pass,
 * copied to HOST as fp32 [B][h][w][cout].  shape_hwc (optional) receives {h, w, cout}; pass out_host = NULL to
 * query the shape only.  Intermediates that a fused kernel keeps on chip (model.0 / model.1 when the fused
 * front is active) hold stale data. */
int wtk_yolo_debug_tensor(wtk_yolo *h, int32_t conv_index, int32_t B, float *out_host, size_t out_cap,
                          int32_t *shape_hwc);
/* ... and one index that names no conv: the live-tile counts of the last sparse forward pass (list form of the
 * sparse Detect box towers), shape {1, 1, 4}: tiles listed for box.0, tiles listed for box.1 + box.2, and the
 * grids of the two launches (the host's upper bounds of the counts).  Zeros where the handle never ran one. */
#define WTK_DEBUG_SPARSE_COUNTS (-1)
/* ... and conv_index = WTK_DEBUG_RAW(i): conv i as the last pass LEFT it.  Reading a Detect box-tower conv by its
 * plain index first completes what a sparse pass skipped (dense launches over every pixel); the raw read does not,
 * so after a sparse pass only the tiles under the survivors hold that pass's values.  (An involution: i <-> -2 - i.) */
#define WTK_DEBUG_RAW(i) (-2 - (i))
/* Run ONLY decode + selection on caller-provided head logits (HOST fp32, same layout as
 * wtk_yolo_debug_head, levels concatenated in anchor order) — isolates the NMS/argmax logic
 * from conv rounding for bit-exact index tests. */
int wtk_yolo_decode_host(wtk_yolo *h, const float *box_host /*[B][A][64]*/,
                         const float *cls_host /*[B][A][nc]*/, int32_t B, int32_t H, int32_t W,
                         float conf, float *out_xywh, float *out_conf, int32_t *out_anchor);
/* Range guard of the fp16-storage modes (WTK_F16, WTK_F16X3: activations and weights live as fp16 values / pairs, |x| < 65 504 in the library's
 * log2(e)-scaled activation domain).  The reference runs a trained, BatchNorm-folded checkpoint in fp32 (yolo_controller.py:42-45,
 * yolo/yolo_train_config.yaml:51) — weights this library has never seen — so both ends are checked:
 *   at wtk_yolo_create   a packed weight beyond the fp16 range is REFUSED (the message names the conv).  Small weights need no guard: below the fp16
 *                        normal range the hi half is a subnormal (spacing 2^-24) and the lo half carries the rest times 2^11, so the pair still
 *                        holds the weight to an ABSOLUTE error of ~2^-36 — far below the rounding of the products it takes part in;
 *   at run time          every max_det = 1 / NMS call reads every class logit: an activation that overflowed anywhere in the network reaches the
 *                        head as inf / NaN in its receptive field, and the head kernels then raise WTK_STATUS_NONFINITE (sticky).  They also
 *                        raise it for an inf / NaN among the box logits they decode: the survivor's (max_det = 1), every candidate's (NMS).
 * wtk_yolo_status: the flags as of the work the caller has synchronised with (no device call: the word lives in pinned host memory);
 * clear != 0 resets the sticky bits.  A WTK_F32 handle reports NONFINITE only for inf / NaN that fp32 itself produces. */
#define WTK_STATUS_NONFINITE 1
int wtk_yolo_status(wtk_yolo *h, int32_t *flags, int32_t clear);
/* Algorithmic work of one forward pass: conv MACs per frame and the number of anchors. */
int wtk_yolo_workload(wtk_yolo *h, double *macs_per_frame, int32_t *anchors);
/* Average device time (ms) per launch of each kernel class over the frames processed since
 * the last reset, measured with HIP events on the caller's stream when profiling is enabled.
 * kernel_class: 0 stem, 1 conv (implicit GEMM), 2 pool, 3 head (decode+select). */
int wtk_yolo_set_profiling(wtk_yolo *h, int32_t enabled);
int wtk_yolo_get_profile(wtk_yolo *h, int32_t kernel_class, double *total_ms, int64_t *launches);
/* The same measurement per kernel (source file) of the forward pass, with the algorithmic FLOPs (2 x MACs) its launches
 * executed: kernel_id 0 stem_mfma_kernel, 1 conv_igemm_kernel + conv1x1_wide_kernel, 2 sppf_pool_kernel, 3 head kernels, 4 conv3x3_halo_kernel
 * (including its fused 1x1 tails), 5 front_fused_kernel + c2f32_fused_kernel, 6 conv3x3_c32_kernel, 7 the conv3x3_halo_kernel launches
 * of sparse Detect box towers (0 FLOPs: the host does not know how many of their tiles were live; launches > 0 tells that the
 * handle's max_det = 1 calls run sparse).  Class 1 of wtk_yolo_get_profile is the sum of ids 1, 4, 5, 6 and 7.  (Build-side instrumentation for bench.py's roofline object; the
 * reference has no counterpart.) */
int wtk_yolo_get_kernel_profile(wtk_yolo *h, int32_t kernel_id, double *total_ms, int64_t *launches, double *flops);

/* ------------------------------------------------------------------------------------------
 * Camera / microscope view extraction for a batch of (frame, platform position) pairs.
 * Replaces: ViewController.camera_view / micro_view -> read() (cv.copyMakeBorder REPLICATE by
 *           camera_size//2) + _custom_view slice   wtracker/sim/view_controller.py:45-61,143-181
 * frames [N][H][W][C] uint8, pos_xy [N][2] int32 (x, y), views [N][view_w][view_h][C] — rows = w,
 * cols = h exactly as the reference slices (view_controller.py:171); all DEVICE pointers.
 * ------------------------------------------------------------------------------------------ */
int wtk_crop_views(const uint8_t *frames_dev, int32_t N, int32_t H, int32_t W, int32_t C,
                   const int32_t *pos_xy_dev, int32_t view_w, int32_t view_h, uint8_t *views_dev,
                   void *stream);

/* ------------------------------------------------------------------------------------------
 * Decision margin of every frame of the handle's last max_det = 1 call, in class-logit units:
 *   min( best anchor's logit - best logit among all other anchors ,  | best logit - logit(conf) | )
 * i.e. how far the result is from selecting another survivor or from flipping between a detection and a NaN row.  The fp16
 * mode's head logits differ from the fp32 reference's by ~0.01: a frame whose margin is well above that has the fp32
 * survivor; a caller that needs the reference's survivor on EVERY frame re-runs the few frames below its threshold on an fp32
 * handle (wtracker_amd.controllers.YoloConfig.recheck_margin does).  No counterpart in the reference.
 * wtk_yolo_margin_buffer: device pointer of the handle's [max_batch] float buffer (valid once the call's stream work is done);
 * wtk_yolo_last_margins_host: synchronises the device and copies B values.
 * ------------------------------------------------------------------------------------------ */
int wtk_yolo_margin_buffer(wtk_yolo *h, const float **margins_dev);
int wtk_yolo_last_margins_host(wtk_yolo *h, int32_t B, float *margins_host);

/* ------------------------------------------------------------------------------------------
 * Detector with the GENERAL greedy NMS (max_det >= 1 boxes per frame): the part of ultralytics'
 * non_max_suppression(conf, iou, agnostic=False, max_det) that the reference's call site never reaches because it
 * hard-wires max_det = 1 (yolo_controller.py:76; yolo/yolo_train_config.yaml:49-50,61 give iou 0.7, max_det 300, class-aware).
 * Candidates = anchors whose best class score > conf, visited in descending score (lowest anchor index on ties); a
 * candidate is dropped when its IoU with an already kept box of the same class exceeds `iou`.
 * Outputs per frame, rows in descending score: out_xywh [B][max_det][4] (x, y, w, h in input-image pixels, NaN rows past the
 * last box), out_conf [B][max_det], out_cls [B][max_det] (-1 past the last), out_anchor [B][max_det], out_count [B]; all but
 * out_xywh may be NULL.  With max_det = 1 the first row equals wtk_yolo_predict's result.
 * wtk_yolo_decode_nms_host: the same selection on caller-supplied head logits (test hook, as wtk_yolo_decode_host).
 * ------------------------------------------------------------------------------------------ */
int wtk_yolo_predict_nms(wtk_yolo *h, const uint8_t *frames_dev, int32_t B, int32_t H, int32_t W, int32_t C, float conf, float iou,
                         int32_t max_det, float *out_xywh, float *out_conf, int32_t *out_cls, int32_t *out_anchor,
                         int32_t *out_count, void *stream);
int wtk_yolo_decode_nms_host(wtk_yolo *h, const float *box_host, const float *cls_host, int32_t B, int32_t H, int32_t W,
                             float conf, float iou, int32_t max_det, float *out_xywh, float *out_conf, int32_t *out_cls,
                             int32_t *out_anchor, int32_t *out_count);

/* ------------------------------------------------------------------------------------------
 * The other predictors behind provide_movement_vector and the training-pair builder, batched over a
 * DEVICE-resident track [n_frames][4] xywh (float32: the detector's track; float64: a loaded bboxes.csv), NaN row =
 * missed detection.  One sample per cycle; the result is the predicted ABSOLUTE head position — the caller subtracts the
 * camera centre and rounds in float64 on the host exactly as the reference does (the prediction itself does not depend
 * on the platform position, so all cycles of a track are computed in one launch).
 *
 * wtk_track_median_centers  replaces OptimalController.provide_movement_vector  optimal_controller.py:16-32
 *     pred[i] = per-axis median of the finite box centres of frames [(cycles[i]+1)*cycle_frame_num, +imaging_frame_num)
 * wtk_track_polyfit         replaces PolyfitController.provide_movement_vector  polyfit_controller.py:54-84
 *     weighted least-squares polynomial (numpy.polynomial.polynomial.polyfit semantics: column-scaled, minimum norm)
 *     through the finite centres at frames cycles[i]*cycle_frame_num + sample_times, evaluated at t_eval
 *     (= cycle_frame_num + imaging_frame_num // 2); sample_times / weights as PolyfitConfig.__post_init__ leaves them
 * wtk_track_training_pairs  replaces NumpyDataset.create_from_config            neural/dataset.py:42-96
 *     rows row0 .. row0+n_rows-1: X = boxes at row + input_frames, Y = centres at row + pred_frames, float64 -> float32,
 *     then relative to the float32 corner of the first input box; keep[i] = 0 where the row holds a NaN (caller compacts)
 * valid[i] = 0: no usable frame (the reference returns (0, 0) for that cycle).  pred is float64.
 * ------------------------------------------------------------------------------------------ */
int wtk_track_median_centers(const void *track_dev, int32_t track_is_f64, int32_t n_frames, const int32_t *cycles_dev,
                             int32_t n_samples, int32_t cycle_frame_num, int32_t imaging_frame_num, double *pred_dev,
                             int32_t *valid_dev, void *stream);
int wtk_track_polyfit(const void *track_dev, int32_t track_is_f64, int32_t n_frames, const int32_t *cycles_dev,
                      int32_t n_samples, int32_t cycle_frame_num, const int32_t *sample_times_host,
                      const double *weights_host, int32_t n_times, int32_t degree, double t_eval, double *pred_dev,
                      int32_t *valid_dev, void *stream);
int wtk_track_training_pairs(const void *track_dev, int32_t track_is_f64, int32_t n_frames, int32_t row0, int32_t n_rows,
                             const int32_t *input_frames_host, int32_t n_in, const int32_t *pred_frames_host,
                             int32_t n_out, float *x_dev, float *y_dev, int32_t *keep_dev, void *stream);

/* ------------------------------------------------------------------------------------------
 * Second look at weak decisions, on the device (extension; host-side form: YoloConfig.recheck_margin).  The fp16 detector
 * reports a decision margin per frame (wtk_yolo_margin_buffer); the K frames of a batch with the smallest margins are
 * detected again by a full-precision handle (WTK_F16X3 / WTK_F32, e.g. through wtk_yolo_predict_views with
 * frame_index = slots) and replace the fast rows where margin < `margin`.  No host synchronisation: K is fixed.
 * One reading of "weak" holds in every entry point below: a row is weak iff margin < `margin` on the margin AS GIVEN, so a NaN row is
 * never weak (NaN < x is false for every x) and with `margin` = +inf every row but the NaN and +inf ones is.
 *   wtk_recheck_select  slots[k] = batch row of the k-th smallest margin (ties: lower row first; for the ORDER a NaN counts as +inf
 *                       and ties with a real +inf; -0.0 and +0.0 tie), k < K;
 *                       *n_weak (nullable) = min(K, rows with margin < `margin`): the leading slots that will be merged
 *   wtk_recheck_select_counted  the same, and *n_overflow (nullable) += max(rows with margin < `margin` - K, 0): the weak rows
 *                       the ceiling K cut off.  They keep their fast-pass result WITHOUT a second look, so a caller that
 *                       promises full-precision decisions must either use K = B (no row can be cut off; with the dynamic
 *                       batch below the cost still follows the number of weak rows) or check this counter.
 *   wtk_yolo_set_dynamic_batch  the handle reads the number of batch rows that matter from DEVICE memory at run time
 *                       (nullptr: off): kernels skip the tiles of images beyond it, rows beyond it hold scratch.  With
 *                       n_dev = n_weak the second look costs what the weak frames cost, with no host round trip.
 *   wtk_recheck_merge   row slots[k] of dst_* = row k of src_* where margins[slots[k]] < margin; *n_replaced += count
 * Replaces nothing in the reference (yolo_controller.py:62-90 computes every frame in fp32).
 * ------------------------------------------------------------------------------------------ */
int wtk_recheck_select(const float *margins_dev, int32_t B, int32_t K, float margin, int32_t *slots_dev,
                       int32_t *n_weak_dev, void *stream);
int wtk_recheck_select_counted(const float *margins_dev, int32_t B, int32_t K, float margin, int32_t *slots_dev,
                               int32_t *n_weak_dev, int32_t *n_overflow_dev, void *stream);
int wtk_yolo_set_dynamic_batch(wtk_yolo *h, const int32_t *n_dev);
/* Concurrency inside one forward pass: n = 2 (default) runs the P3 and the P4 Detect tower on a side stream each next to the PAN path,
 * 1 puts both on one side stream, 0 keeps every launch on the caller's stream.  A process that keeps several handles busy at once
 * (two lanes, a second-look handle) can have too many streams in flight; the side streams themselves are ONE pair per process and
 * device, shared by all handles. */
int wtk_yolo_set_side_streams(wtk_yolo *h, int32_t n);
/* ABI v3 symbol of the (removed) block cache of destroyed handles: nothing is cached any more, the call returns 0. */
int wtk_release_cached_memory(void);
int wtk_recheck_merge(const float *margins_dev, const int32_t *slots_dev, int32_t B, int32_t K, float margin,
                      const float *src_xywh, const float *src_conf, const int32_t *src_anchor, float *dst_xywh,
                      float *dst_conf, int32_t *dst_anchor, int32_t *n_replaced_dev, void *stream);
/* Deferred form of the same second look: the weak rows of SEVERAL fast passes share ONE full-precision pass, whose fixed cost
 * (a forward pass of ~60 launches costs ~1.2 ms however few frames are live) is then paid once per D batches.
 *   wtk_recheck_enqueue  every row of the batch with margin < `margin` is appended to a device-side queue: a copy of its frame
 *                        (frames_dev [B][frame_bytes] -> q_frames_dev [q_cap][frame_bytes]) and the addresses of its three
 *                        outputs (dst_xywh + 4 b, dst_conf + b, dst_anchor + b; the last two nullable).  *q_len += rows queued;
 *                        rows that find the queue full keep their fast result and are COUNTED in *n_overflow (nullable) — a
 *                        caller that flushes every D batches with q_cap >= D * B can never overflow.
 *   (the caller then runs a full-precision handle over q_frames_dev with wtk_yolo_set_dynamic_batch(h, q_len_dev))
 *   wtk_recheck_scatter  rows 0 .. *q_len - 1 of src_* go to the queued addresses; *n_replaced += count; *q_len = 0.
 * The output rows named at enqueue time must stay valid until the scatter.  pos_scratch_dev: int32 [B].
 * Replaces nothing in the reference (yolo_controller.py:62-90 computes every frame in fp32). */
int wtk_recheck_enqueue(const float *margins_dev, int32_t B, float margin, const uint8_t *frames_dev, int64_t frame_bytes,
                        uint8_t *q_frames_dev, int32_t q_cap, int32_t *q_len_dev, void **q_xywh_ptrs_dev,
                        void **q_conf_ptrs_dev, void **q_anchor_ptrs_dev, float *dst_xywh, float *dst_conf,
                        int32_t *dst_anchor, int32_t *pos_scratch_dev, int32_t *n_overflow_dev, void *stream);
int wtk_recheck_scatter(int32_t *q_len_dev, int32_t q_cap, const float *src_xywh, const float *src_conf,
                        const int32_t *src_anchor, void **q_xywh_ptrs_dev, void **q_conf_ptrs_dev,
                        void **q_anchor_ptrs_dev, int32_t *n_replaced_dev, void *stream);

/* ------------------------------------------------------------------------------------------
 * Hybrid detector: the two-handle "look twice where fp16 is unsure" scheme above as ONE object behind this boundary, so that a
 * C / C++ host gets the fast mode with full-precision decisions from a single call per batch — what YoloController.predict
 * (yolo_controller.py:62-90, every frame in fp32: yolo/yolo_train_config.yaml:51 `half: False`) returns, at the fp16 handle's
 * speed on the frames whose decision is clear.  `fast` and `exact` are wtk_yolo handles of the same model on the same device
 * (typically WTK_F16 and WTK_F16X3); the object borrows them (the caller destroys them AFTER wtk_hybrid_destroy) and owns the
 * exact handle's dynamic batch while it lives: a full-precision handle serves at most one hybrid object at a time (create refuses
 * a handle whose dynamic batch is already set).
 *   margin  rows whose fast-pass decision margin is below it are looked at again (choose it from measurements on the model:
 *           see wtracker_amd/hybrid.py calibrate(); a fixed number is not a guarantee).
 *   k       ceiling of rows per second look; 0 = the largest value that can never cut a weak row off (the whole batch; the
 *           exact handle's max_batch in deferred mode).  A smaller k COUNTS what it cuts off (wtk_hybrid_counters).
 *   defer   1: every call looks again before it returns its rows to the stream.  D > 1: the weak rows of D consecutive calls
 *           share one full-precision pass (device-side queue of k frame copies); the rows a call named are final only after
 *           the flush that follows — automatically on every D-th call, or wtk_hybrid_flush.  The output buffers named by a
 *           call must stay valid until then; every call must bring frames of the same shape.
 * Everything is enqueued on `stream`; no entry point but _counters synchronises.  One thread per object.
 * ------------------------------------------------------------------------------------------ */
typedef struct wtk_hybrid wtk_hybrid;
int wtk_hybrid_create(wtk_hybrid **out, wtk_yolo *fast, wtk_yolo *exact, float margin, int32_t k, int32_t defer);
void wtk_hybrid_destroy(wtk_hybrid *h);
int wtk_hybrid_set_margin(wtk_hybrid *h, float margin);
/* same arguments and results as wtk_yolo_predict with max_det = 1 */
int wtk_hybrid_predict(wtk_hybrid *h, const uint8_t *frames_dev, int32_t B, int32_t H, int32_t W, int32_t C, float conf,
                       float *out_xywh, float *out_conf, int32_t *out_anchor, void *stream);
/* same arguments and results as wtk_yolo_predict_views with max_det = 1; defer must be 1 */
int wtk_hybrid_predict_views(wtk_hybrid *h, const uint8_t *frames_dev, int32_t n_frames, int32_t H, int32_t W, int32_t C,
                             const int32_t *frame_index_dev, const int32_t *pos_xy_dev, int32_t B, int32_t view_w,
                             int32_t view_h, float conf, float *out_xywh, float *out_conf, int32_t *out_anchor,
                             void *stream);
int wtk_hybrid_flush(wtk_hybrid *h, void *stream);
/* calls whose weak rows still wait for their full-precision pass (0: every row handed out so far is final); -1 on a null handle */
int wtk_hybrid_pending(wtk_hybrid *h);
/* rows replaced so far / weak rows the ceiling cut off so far (must read 0 for the full-precision claim).  Synchronises the device. */
int wtk_hybrid_counters(wtk_hybrid *h, int64_t *rows_replaced, int64_t *rows_overflowed);
/* hold = 1: the full-precision handle gets its static batch back so that the caller can run it directly on whole batches (calibration of
 * the margin); hold = 0: the object takes it again.  Needs wtk_hybrid_pending() == 0; predict / flush are refused while held. */
int wtk_hybrid_hold(wtk_hybrid *h, int32_t hold);
/* the configuration in effect: ceiling k, defer, margin (each nullable) */
int wtk_hybrid_config(wtk_hybrid *h, int32_t *k, int32_t *defer, float *margin);

/* ------------------------------------------------------------------------------------------
 * Detector on camera views of device-resident full frames: view cropping fused with the letterbox in front of
 * the detector, so the per-frame host crop + upload of the reference's loop disappears.
 * Replaces: YoloController.on_camera_frame -> sim.camera_view()   yolo_controller.py:58-59
 *           ViewController.read (copyMakeBorder REPLICATE) + _custom_view   view_controller.py:45-61,143-172
 *           + the LetterBox resize inside YOLO.predict                    yolo_controller.py:72-78
 * frames [n_frames][H][W][C] uint8 (DEVICE); batch row n is the w x h view of frame frame_index[n] (NULL: frame n)
 * centred on platform position pos_xy[n] = (x, y) — rows = w, cols = h as the reference slices.  Outputs as
 * wtk_yolo_predict, boxes in VIEW pixel coordinates (what predict() on the cropped frames returns).
 * ------------------------------------------------------------------------------------------ */
int wtk_yolo_predict_views(wtk_yolo *h, const uint8_t *frames_dev, int32_t n_frames, int32_t H, int32_t W, int32_t C,
                           const int32_t *frame_index_dev, const int32_t *pos_xy_dev, int32_t B,
                           int32_t view_w, int32_t view_h, float conf, float iou, int32_t max_det,
                           float *out_xywh, float *out_conf, int32_t *out_anchor, void *stream);

/* ------------------------------------------------------------------------------------------
 * Multi-GPU: the path's ONLY collective, for callers that do not go through PyTorch.
 * The reference has no distributed code; this replaces nothing — it is what lets frames be sharded over the GPUs of a node:
 * every rank detects its n_local frames of a super-batch, one all-gather (RCCL over xGMI, 16 B per frame: latency-bound)
 * gives every rank the whole [world * n_local][4] block in rank order = frame order (wtracker_amd/pipeline.py shows the
 * sharding; it uses torch.distributed's RCCL communicator for the same ncclAllGather).
 * Rendezvous: rank 0 calls wtk_comm_unique_id and hands the 128 bytes to the other ranks out of band (file, socket, MPI);
 * every rank then calls wtk_comm_create.  librccl is loaded on the first wtk_comm_* call, not with libwtk_hip.so.
 * ------------------------------------------------------------------------------------------ */
#define WTK_COMM_ID_BYTES 128
typedef struct wtk_comm wtk_comm;
int wtk_comm_unique_id(uint8_t *id_out, size_t cap);
int wtk_comm_create(wtk_comm **out, int32_t device, int32_t rank, int32_t world, const uint8_t *id);
void wtk_comm_destroy(wtk_comm *c);
int wtk_allgather_tracks(wtk_comm *c, const float *local_dev, int32_t n_local, float *all_dev, void *stream);

/* ------------------------------------------------------------------------------------------
 * Experiment evaluation on the device: the background of an experiment and the precise tracking error of a log, bit-exact to the
 * reference's numpy code, from frames already resident in device memory (no per-frame host reads, no worm-view image files).
 * Both enqueue on `stream`; neither synchronises nor allocates.
 *
 * wtk_background  replaces BGExtractor.calc_background (its median / mean step)   dataset/bg_extractor.py:18-75
 *     bg[i] = per-byte median (WTK_BG_MEDIAN: np.median(...).astype(uint8), i.e. floor((a + b) / 2) of the two middle values for even
 *     n) or mean (WTK_BG_MEAN: floor(sum / n)) of byte i over the probe frames.  frames_dev [n_frames][frame_bytes] (gray or BGR, taken
 *     as flat bytes); probe_idx_dev [n_probes] frame ids in [0, n_frames) (the caller's to check), or NULL for frames 0 .. n_probes-1.
 *     n_probes: 1 .. 65535 for the median (uint16 counts), 1 .. 2^24 for the mean (uint32 sums); a larger n is an error, never a
 *     wrapped result.
 * wtk_precise_error  replaces ErrorCalculator.calculate_precise per row             eval/error_calculator.py:64-160
 *     row r: the worm box and the microscope box (xywh; float32, or float64 with boxes_are_f64) discretised as BoxUtils.discretize
 *     (bbox_utils.py:118-167: floor / ceil, clip to H x W, zero-area boxes illegal), total = pixels of the worm crop of frame
 *     frame_nums[r] with |frame - bg| > diff_thresh, inside = those in the worm / microscope intersection;
 *     err[r] = 1 - inside / total (float64), 0 where total = 0, NaN where the worm box is illegal or frame_nums[r] is outside
 *     [0, n_frames) (those rows are also added to *n_bad_frame_dev, nullable).  counts_dev [n_rows][2] = (total, inside), nullable.
 *     frames_dev [n_frames][H][W] gray, bg_dev [H][W].  err is PER ROW; the reference's own return value shifts the legal rows'
 *     errors to the front (see wtracker_amd/evaluation.py, layout="reference").
 * ------------------------------------------------------------------------------------------ */
#define WTK_BG_MEDIAN 0
#define WTK_BG_MEAN 1
int wtk_background(const uint8_t *frames_dev, int32_t n_frames, int64_t frame_bytes, const int32_t *probe_idx_dev, int32_t n_probes,
                   int32_t method, uint8_t *bg_dev, void *stream);
int wtk_precise_error(const uint8_t *frames_dev, int32_t n_frames, int32_t H, int32_t W, const uint8_t *bg_dev,
                      const void *worm_xywh_dev, const void *mic_xywh_dev, int32_t boxes_are_f64,
                      const int32_t *frame_nums_dev, int32_t n_rows, double diff_thresh, double *err_dev,
                      int32_t *counts_dev, int32_t *n_bad_frame_dev, void *stream);

/* ------------------------------------------------------------------------------------------
 * Weight search for the polynomial-fit controller (csrc/polyfit_opt.hip): the reference's WeightEvaluator and the particle swarm that
 * polyfit_optimizer.ipynb runs over it, on the device.  Everything enqueues on `stream`; nothing synchronises or allocates.
 *
 * wtk_polyfit_dataset  replaces WeightEvaluator._extract_positions                  sim_controllers/polyfit_controller.py:145-188
 *     One candidate cycle per cycle_start = 0, L, 2L, ... of the track ([n_frames][4] xywh, float32 or float64).  A cycle is kept when
 *     every input frame cycle_start + input_offsets[i] is >= 0, the target frame cycle_start + pred_time_offset is < n_frames, all
 *     2 n_times + 2 centre coordinates are finite and sqrt(dx^2 + dy^2) / (pred_time_offset - input_offsets[0]) of target against first
 *     input lies in [min_speed, max_speed].  input_offsets (host) must be SORTED ascending with input_offsets[n-1] <= pred_time_offset
 *     (beyond it the reference raises IndexError at the end of the log; here the call is refused) and input_offsets[0] < pred_time_offset.
 *     Kept cycles are appended IN CYCLE ORDER behind the *count_dev cycles the buffers already hold (several logs: call again with the same
 *     buffers): y_input_dev [n_times][2 * capacity] with x and y of cycle k in columns 2k, 2k + 1, y_target_dev [2 * capacity] likewise.
 *     *count_dev += kept; a count above `capacity` (cycles) after the call means the buffers were too small: nothing is written past them.
 * wtk_polyfit_weight_mae  replaces WeightEvaluator.eval for P weight vectors         polyfit_controller.py:207-221
 *     mae_dev[p] = mean_m |y_target[m] - polyval(t_pred, polyfit(sample_times, y_input[:, m], degree, w = weights_dev[p]))| over the M series
 *     (M = 2 x kept cycles; y_input_dev [n_times][ld], ld >= M), numpy's scaling and rcond = n_times * eps cut included.  NaN where the weights
 *     are not finite, where the solver did not converge, and for M = 0.  Fixed-order reduction: equal inputs give equal bits in every call,
 *     whatever P.  n_times <= 16, degree <= 7.  scratch_dev: wtk_polyfit_mae_scratch_doubles(P, M) doubles.  stop_dev (nullable): the call
 *     does nothing once *stop_dev != 0 on the device (the swarm's stop flag).
 * wtk_polyfit_swarm_step  one epoch of the inertia-weight particle swarm over weight vectors (no counterpart in the reference's code: it calls
 *     mealpy).  From mae_dev [P] of the current positions: personal bests (strictly lower only), global best (lowest particle among equals),
 *     history_dev[epoch] = best so far, ctrl_dev = {stop flag, epochs since the last improvement, epochs run, particle of the global best};
 *     the stop flag rises once max_early_stop epochs brought no improvement, and a raised flag makes this and later calls return at once.
 *     Otherwise v <- clamp(w v + c1 r1 (pbest - x) + c2 r2 (gbest - x), -vmax, vmax), x <- clip(x + v, lb, ub) with r1 = rand_dev[0][p][n],
 *     r2 = rand_dev[1][p][n] uniform in [0, 1) (the caller's: one [2][P][N] slice per epoch).  pos / vel / pbest_pos [P][N], pbest_val [P],
 *     gbest_pos [N], gbest_val [1]; the caller initialises them (pbest_val = gbest_val = +inf, ctrl = 0).
 * ------------------------------------------------------------------------------------------ */
int wtk_polyfit_dataset(const void *track_dev, int32_t track_is_f64, int32_t n_frames, int32_t cycle_frame_num,
                        const int32_t *input_offsets_host, int32_t n_times, int32_t pred_time_offset, double min_speed,
                        double max_speed, double *y_input_dev, double *y_target_dev, int32_t capacity, int32_t *count_dev,
                        void *stream);
int64_t wtk_polyfit_mae_scratch_doubles(int32_t P, int32_t M);
int wtk_polyfit_weight_mae(const double *y_input_dev, const double *y_target_dev, int64_t ld, int32_t M,
                           const int32_t *sample_times_host, int32_t n_times, int32_t pred_time_offset, int32_t degree,
                           const double *weights_dev, int32_t P, double *mae_dev, double *scratch_dev, int64_t scratch_doubles,
                           const int32_t *stop_dev, void *stream);
int wtk_polyfit_swarm_step(const double *mae_dev, const double *rand_dev, int32_t P, int32_t N, int32_t epoch,
                           int32_t max_early_stop, double w, double c1, double c2, double lb, double ub, double vmax,
                           double *pos_dev, double *vel_dev, double *pbest_pos_dev, double *pbest_val_dev, double *gbest_pos_dev,
                           double *gbest_val_dev, int32_t *ctrl_dev, double *history_dev, void *stream);

/* ------------------------------------------------------------------------------------------
 * Closed-loop replay of track-driven experiments (csrc/replay.hip): the reference's Simulator + SineMotorController + LoggingController
 * (sim/simulator.py:140-194, sim/motor_controllers.py:58-88, sim_controllers/logging_controller.py:145-185) for E experiments on one
 * track at once, with ErrorCalculator.calculate_bbox_error / calculate_mse_error (eval/error_calculator.py:164-212) of every logged row.
 * Everything enqueues on `stream`; nothing synchronises or allocates.  All device arrays of per-cycle values are CYCLE-major: [n_cycles][E].
 *
 * Geometry (wtk_replay_config): a cycle has L = imaging_frame_num + moving_frame_num frames; the move of cycle c is decided at frame
 * c L + imaging_frame_num and taken over the next moving_frame_num frames; the platform position is clamped to [0, frame_w - 1] x
 * [0, frame_h - 1]; the camera / microscope corner is position - size / 2 (integer division).  Logged are the cycles 0 .. n_log - 1 with
 * n_log = (num_frames - 1) / L, all L frames of each: R = n_log L rows per experiment, row r = frame r (the last cycle is never logged).
 * n_cycles: cycles to scan, n_log <= n_cycles, decision frame of the last one < num_frames.
 *
 * wtk_replay_scan   one lane per experiment, sequential over cycles.  Move of cycle c per axis, float64, rounded half to even, with
 *     cam = position - cam_size / 2 (integer) at the cycle's start:
 *       WTK_REPLAY_CSV      rint(((x - cam) + w / 2) - cam_size / 2)   (x, y, w, h) = track row c L + imaging - pred_frame_num
 *       WTK_REPLAY_OPTIMAL  rint(a - (cam + cam_size / 2))             a = a_dev[c][e]
 *       WTK_REPLAY_POLYFIT  rint((a - cam) - cam_size / 2)
 *       WTK_REPLAY_MLP      rint(a + (b - (cam + cam_size / 2)))       a = clipped model output, b = b_dev[c][e] corner of the first input box
 *     (0, 0) where valid_dev[c][e] == 0 (CSV: where the row is outside the track or not finite) or the expression is not finite; |move|
 *     saturates at 2^30.  Then moving_frame_num motor steps: want = share[k] move + carry, took = rint(want), carry = want - took,
 *     position = clamp(position + took).  share_dev [moving_frame_num] doubles is the caller's half-cosine table
 *     (cos(k pi / M) - cos((k + 1) pi / M)) / 2, computed on the host.  Out: pos_dev [n_cycles][E][2] position at the cycle's start,
 *     move_dev [n_cycles][E][2].  a_dev / b_dev [n_cycles][E][2] doubles, valid_dev [n_cycles][E]; CSV needs none of them, b_dev is MLP's.
 * wtk_replay_rows   one thread per (experiment, logged row) from the scan's pos_dev / move_dev.  Row: platform position, camera box,
 *     microscope box, logged worm box ((x - cam_x) + cam_x, (y - cam_y) + cam_y, w, h; a non-finite track row as 0, 0, 0, 0), its
 *     bbox error (0 where the worm box has no area) and MSE error.  bbox_err_dev / mse_err_dev [E][R] (nullable).  rows_dev
 *     [n_slots][R][WTK_REPLAY_ROW_DOUBLES] (nullable, with row_slot_dev [E]: the slot of experiment e or -1): plt_x, plt_y, cam_x, cam_y,
 *     cam_w, cam_h, mic_x, mic_y, mic_w, mic_h, wrm_x, wrm_y, wrm_w, wrm_h, cycle, phase (0 imaging, 1 moving).  summary_dev
 *     [E][WTK_REPLAY_SUMMARY_DOUBLES]: sum and count of the bbox error over all rows, the same over the imaging rows of the cycles
 *     1 .. n_log - 2 (DataAnalyzer.clean(trim_cycles=True, imaging_only=True)), the count of rows with bbox error > 1e-7, the sum of the
 *     MSE error.  Sums have a fixed order (per lane in index order, a binary tree per chunk of 4096 rows, chunks in index order): an
 *     experiment gives the same bits alone and in any population.  scratch_dev: wtk_replay_scratch_doubles(E, R) doubles.
 * Refused (error code, no memory touched): E < 1, moving_frame_num < 1, imaging_frame_num < 1, pred_frame_num > imaging_frame_num (or < 1
 * for CSV), a track shorter than R, a camera smaller than the microscope, n_cycles outside the range above, a required pointer that is null.
 * ------------------------------------------------------------------------------------------ */
#define WTK_REPLAY_CSV 0
#define WTK_REPLAY_OPTIMAL 1
#define WTK_REPLAY_POLYFIT 2
#define WTK_REPLAY_MLP 3
#define WTK_REPLAY_ROW_DOUBLES 16
#define WTK_REPLAY_SUMMARY_DOUBLES 6
typedef struct wtk_replay_config {
    int32_t num_frames;        /* frames of the experiment (ExperimentConfig.num_frames) */
    int32_t imaging_frame_num; /* TimingConfig */
    int32_t moving_frame_num;
    int32_t pred_frame_num;
    int32_t cam_w, cam_h;      /* camera_size_px */
    int32_t mic_w, mic_h;      /* micro_size_px */
    int32_t frame_w, frame_h;  /* the frame the position is clamped to (the reader's frame_shape[1], [0]) */
    int32_t init_x, init_y;    /* ExperimentConfig.init_position */
} wtk_replay_config;
int wtk_replay_scan(const wtk_replay_config *cfg, int32_t kind, int32_t E, int32_t n_cycles, const double *track_dev, int32_t n_track,
                    const double *a_dev, const double *b_dev, const int32_t *valid_dev, const double *share_dev, int32_t *pos_dev,
                    int32_t *move_dev, void *stream);
int64_t wtk_replay_scratch_doubles(int32_t E, int64_t R);
int wtk_replay_rows(const wtk_replay_config *cfg, int32_t E, int32_t n_cycles, const double *track_dev, int32_t n_track,
                    const double *share_dev, const int32_t *pos_dev, const int32_t *move_dev, const int32_t *row_slot_dev, int32_t n_slots,
                    double *rows_dev, double *bbox_err_dev, double *mse_err_dev, double *summary_dev, double *scratch_dev,
                    int64_t scratch_doubles, void *stream);

/* ------------------------------------------------------------------------------------------
 * The closed-loop error as the objective of the Polyfit weight search (csrc/replay_targets.hip, csrc/replay.hip).
 *
 * wtk_replay_polyfit_targets   the per-cycle Polyfit targets of P weight vectors in one call: a_dev [n_cycles][P][2], valid_dev
 *     [n_cycles][P], what wtk_replay_scan reads.  weights_dev [P][n_times] doubles on the device (the swarm's position buffer); one degree,
 *     one set of sample_times_host (frame offsets from the cycle's start, weight j belongs to time j) and one t_eval for all of them.  For
 *     every (cycle, particle) the result has the bits wtk_track_polyfit (float64 track) gives for that cycle with that particle's weights.
 *     The SVD of a fit depends on the weights and on which samples are finite only, so the caller groups the cycles: class_mask_dev
 *     [n_classes] (bit j set: sample j of the cycle lies inside the track and its centre x + w / 2, y + h / 2 is finite), cycle_class_dev
 *     [n_cycles] the class of each cycle.  One SVD per (class, particle), then one thread per (cycle, particle).  A cycle whose samples
 *     are not the ones its class names (or whose class index is out of range) gets valid = 0; so do a class without samples and a solve
 *     that did not converge.  scratch_dev: wtk_replay_polyfit_targets_scratch_doubles(n_classes, P, n_times, degree) doubles (-1: bad sizes).
 * wtk_replay_objective   wtk_replay_scan, then the reduction of wtk_replay_rows without row, per-row or slot output, then
 *     objective_dev[e] = one float64 division of experiment e's summary: WTK_REPLAY_OBJ_TRIMMED_BBOX summary[2] / summary[3] (the rows
 *     DataAnalyzer.clean(trim_cycles=True, imaging_only=True) keeps), _MEAN_BBOX [0] / [1], _MEAN_MSE [5] / [1], _NON_PERFECT [4] / [1];
 *     0 / 0 is NaN.  pos_dev / move_dev / summary_dev / scratch_dev are the work buffers of the two steps, sized as for them.
 * stop_dev (nullable): when *stop_dev != 0 at run time every launch of the call returns at once and no memory is touched (the ctrl
 *     word of wtk_polyfit_swarm_step: all epochs of a search are enqueued back to back).
 * Refused (error code, no memory touched): n_times outside 1..16, degree outside 0..7, P outside 1..65535, n_classes outside
 *     1..n_cycles, scratch too small, a required pointer that is null; wtk_replay_objective: what wtk_replay_scan / _rows refuse, an unknown
 *     objective, the trimmed objective with fewer than 3 logged cycles.
 * ------------------------------------------------------------------------------------------ */
#define WTK_REPLAY_OBJ_TRIMMED_BBOX 0
#define WTK_REPLAY_OBJ_MEAN_BBOX 1
#define WTK_REPLAY_OBJ_MEAN_MSE 2
#define WTK_REPLAY_OBJ_NON_PERFECT 3
int64_t wtk_replay_polyfit_targets_scratch_doubles(int32_t n_classes, int32_t P, int32_t n_times, int32_t degree);
int wtk_replay_polyfit_targets(const double *track_dev, int32_t n_track, int32_t n_cycles, int32_t cycle_frame_num, const double *weights_dev,
                               int32_t P, const int32_t *sample_times_host, int32_t n_times, int32_t degree, double t_eval,
                               const int32_t *cycle_class_dev, const int32_t *class_mask_dev, int32_t n_classes, double *a_dev,
                               int32_t *valid_dev, double *scratch_dev, int64_t scratch_doubles, const int32_t *stop_dev, void *stream);
int wtk_replay_objective(const wtk_replay_config *cfg, int32_t kind, int32_t E, int32_t n_cycles, const double *track_dev, int32_t n_track,
                         const double *a_dev, const double *b_dev, const int32_t *valid_dev, const double *share_dev, int32_t *pos_dev,
                         int32_t *move_dev, double *summary_dev, double *scratch_dev, int64_t scratch_doubles, int32_t objective,
                         double *objective_dev, const int32_t *stop_dev, void *stream);

/* ------------------------------------------------------------------------------------------
 * A population replayed on a SET of T tracks at once, with a pooled objective (csrc/replay_set.hip).
 *
 * All tracks share the timing, camera and microscope entries of `cfg` (its num_frames, frame_w, frame_h, init_x, init_y are not read: they
 * are each track's own, in the table; the *_geom entry points further down give every track its own camera and microscope too).  The tracks lie in ONE "super-track" track_dev [n_super][4], n_super a multiple of L: track t
 * starts at row cyc_off L, holds its n_track rows, then NaN rows up to the end of its slot of max(n_cycles, ceil(n_track / L)) cycles, then
 * guard_cycles further all-NaN cycles.  Every targets entry point treats a NaN row as it treats a row outside the track, so ONE call of
 * wtk_replay_polyfit_targets / wtk_replay_mlp_targets / wtk_track_polyfit / wtk_track_median_centers / wtk_mlp_predict_track over the
 * super-track, with n_cycles = n_super / L, gives every cycle of every track the bits the call on that track alone gives, as long as
 * no frame offset from a cycle's start reaches further than guard_cycles L frames.  All per-cycle arrays (a_dev, b_dev, valid_dev,
 * pos_dev, move_dev) are indexed by the super-track's cycle: [n_super / L][E]...; track t's cycles are the contiguous slice from cyc_off.
 * The NaN fill is the caller's: the entry points check the table, never the rows.
 *
 * wtk_replay_set_track   one table entry.  The caller fills every field; the derived ones (n_cycles' range, n_log = (num_frames - 1) / L,
 *     R = n_log L, chunk0 = the sum of ceil(R / 4096) over the tracks before) are checked against the others.  tracks_host [T] is read by
 *     the checks, tracks_dev [T] (the same bytes, uploaded once by the caller) by the kernels.
 * wtk_replay_set_scan   wtk_replay_scan of every (track, experiment): one lane each, sequential over the track's cycles from the track's own
 *     clamped init position, with the track's own clamp and (CSV) row count.  Out: pos_dev / move_dev [n_super / L][E][2]; cycles of no
 *     track are not written.
 * wtk_replay_set_rows   wtk_replay_rows' reduction (no row, per-row or slot output) of every (track, experiment): one block per
 *     (experiment, chunk of 4096 rows of one track), the same lane order and tree; the trimmed rows drop the first and the last logged
 *     cycle of EVERY track (DataAnalyzer.clean works per log).  One finish launch adds, per (experiment, slot), each track's chunk partials
 *     in index order into track_summary_dev [T][E][WTK_REPLAY_SUMMARY_DOUBLES] (bit-equal to wtk_replay_rows' summary of that track alone)
 *     and those, in track order from 0.0, into summary_dev [E][WTK_REPLAY_SUMMARY_DOUBLES].  No floating-point atomics: a (track,
 *     experiment) pair gives the same bits for any E, any T and any place in the set.  scratch_dev: wtk_replay_set_scratch_doubles(
 *     tracks_host, T, cycle_frame_num, E) doubles (-1: a bad table).
 * wtk_replay_set_objective   scan, rows, and in the finish launch objective_dev[e] = one float64 division of the POOLED slots (the ids of
 *     wtk_replay_objective: sums over all tracks / counts over all tracks, the mean over the rows of all logs); track_objective_dev
 *     [T][E] (nullable): the same division of each track's slots.  0 / 0 is NaN.  Three launches whatever T is.  T = 1 gives
 *     wtk_replay_objective's bits.
 * stop_dev (nullable): as for wtk_replay_objective.
 * Refused (error code, nothing launched): T < 1, for track t (named by index) what wtk_replay_scan / wtk_replay_rows refuse of an
 *     experiment, an entry whose derived fields contradict the others, an init position outside the frame, a slot that overlaps the slot
 *     and guard before it or ends beyond n_super, guard_cycles < 0, n_super not a multiple of L, (experiment, chunk) blocks >= 2^31,
 *     T > 65535, the trimmed objective where any track logs fewer than 3 cycles, an unknown objective, scratch too small,
 *     a required pointer that is null.
 * ------------------------------------------------------------------------------------------ */
typedef struct wtk_replay_set_track {
    int64_t R;          /* logged rows: n_log L */
    int32_t cyc_off;    /* first cycle of the track in the super-track; its first row is cyc_off L */
    int32_t n_track;    /* rows of the track itself */
    int32_t num_frames; /* ExperimentConfig.num_frames of this track */
    int32_t n_cycles;   /* cycles scanned: n_log <= n_cycles, decision frame of the last one < num_frames */
    int32_t n_log;      /* (num_frames - 1) / L */
    int32_t x_max, y_max;   /* frame_w - 1, frame_h - 1: the clamp of this track's platform position */
    int32_t init_x, init_y; /* ExperimentConfig.init_position, clamped to the frame */
    int32_t chunk0;     /* first chunk of the track: the sum of ceil(R / 4096) over the tracks before it */
} wtk_replay_set_track;
int wtk_replay_set_scan(const wtk_replay_config *cfg, const wtk_replay_set_track *tracks_host, const wtk_replay_set_track *tracks_dev, int32_t T,
                        int32_t guard_cycles, int32_t kind, int32_t E, const double *track_dev, int32_t n_super, const double *a_dev,
                        const double *b_dev, const int32_t *valid_dev, const double *share_dev, int32_t *pos_dev, int32_t *move_dev,
                        const int32_t *stop_dev, void *stream);
int64_t wtk_replay_set_scratch_doubles(const wtk_replay_set_track *tracks_host, int32_t T, int32_t cycle_frame_num, int32_t E);
int wtk_replay_set_rows(const wtk_replay_config *cfg, const wtk_replay_set_track *tracks_host, const wtk_replay_set_track *tracks_dev, int32_t T,
                        int32_t guard_cycles, int32_t E, const double *track_dev, int32_t n_super, const double *share_dev,
                        const int32_t *pos_dev, const int32_t *move_dev, double *track_summary_dev, double *summary_dev, double *scratch_dev,
                        int64_t scratch_doubles, const int32_t *stop_dev, void *stream);
int wtk_replay_set_objective(const wtk_replay_config *cfg, const wtk_replay_set_track *tracks_host, const wtk_replay_set_track *tracks_dev,
                             int32_t T, int32_t guard_cycles, int32_t kind, int32_t E, const double *track_dev, int32_t n_super,
                             const double *a_dev, const double *b_dev, const int32_t *valid_dev, const double *share_dev, int32_t *pos_dev,
                             int32_t *move_dev, double *track_summary_dev, double *summary_dev, double *scratch_dev, int64_t scratch_doubles,
                             int32_t objective, double *objective_dev, double *track_objective_dev, const int32_t *stop_dev, void *stream);

/* ------------------------------------------------------------------------------------------
 * The PRECISE error of a population on a set of tracks (csrc/replay_set.hip): wtk_replay_precise (below) of every
 * (track, experiment) of a set scan, each track with its own frames, background, frame shape and threshold, in a number of launches that
 * does not depend on T, and the objective pooled over the rows of all tracks.
 *
 * wtk_replay_set_frames   one entry per track, beside wtk_replay_set_track: frames [n_frames][H][W] gray uint8 on the device (row r of the
 *     track is frame r, n_frames >= R), bg [H][W], (H, W) = the track's (y_max + 1, x_max + 1), diff_thresh (a pixel is foreground where
 *     |frame - bg| > diff_thresh), row0 = the sum of R over the tracks before it.  frames_host [T] is read by the checks, frames_dev [T]
 *     (the same bytes, uploaded once by the caller) by the kernels.
 * wtk_replay_set_precise   from a set scan's pos_dev / move_dev: one workgroup per logged row of ALL tracks (global row rho = row0 + r),
 *     which finds its track by a search on row0 and runs wtk_replay_precise's per-frame statements on that track's view and frames; the
 *     walk launch likewise; the reduction one block per (experiment, chunk of 4096 rows of one track), the trimmed rows dropping the first
 *     and the last logged cycle of EVERY track; the set's finish launch.  Four launches whatever T is.  max_crop_px as for
 *     wtk_replay_precise: it never changes a bit.
 *   err_dev [E][sum R] float64 (nullable), counts_dev [E][sum R][2] int32 (nullable): track t's rows are the columns from row0.
 *   track_summary_dev [T][E][WTK_REPLAY_PRECISE_SUMMARY_DOUBLES]: bit-equal to wtk_replay_precise's summary of that track alone;
 *     summary_dev [E][...]: those added in track order from 0.0.  No floating-point atomics.
 *   scratch_dev: wtk_replay_set_precise_scratch_doubles(tracks_host, T, cycle_frame_num, E) doubles (-1: a bad table): E sum R pair
 *     errors ([sum R][E], track t's block from row0 E), E S 6 chunk partials (S = the chunks of all tracks), ceil(sum R / 2) doubles of
 *     int32 flags.
 * wtk_replay_set_precise_objective   wtk_replay_set_scan, the above without per-pair output, and in the finish launch objective_dev[e] =
 *     one float64 division of the POOLED slots for a WTK_REPLAY_POBJ_* id; track_objective_dev [T][E] (nullable): the same of each
 *     track's slots, wtk_replay_precise_objective's bits.  0 / 0 is NaN.  Five launches whatever T is.
 * stop_dev (nullable): as for wtk_replay_objective.
 * Refused (error code, nothing launched): everything wtk_replay_set_rows / wtk_replay_set_objective refuse of the track table; for track
 *     t (named by index) a null frames or background pointer, (H, W) other than the track's, H * W > 2^30, n_frames < R, a diff_thresh that
 *     is not finite, row0 that is not the prefix sum of R; max_crop_px < 0, sum R >= 2^31, S E >= 2^31, scratch too small, an unknown
 *     objective, the trimmed objective where any track logs fewer than 3 cycles, a required pointer that is null.
 * ------------------------------------------------------------------------------------------ */
typedef struct wtk_replay_set_frames {
    const uint8_t *frames; /* [n_frames][H][W] gray, on the device */
    const uint8_t *bg;     /* [H][W], on the device */
    double diff_thresh;
    int64_t row0;          /* first global logged row of the track: the sum of R over the tracks before it */
    int32_t n_frames, H, W;
    int32_t reserved;
} wtk_replay_set_frames;
int64_t wtk_replay_set_precise_scratch_doubles(const wtk_replay_set_track *tracks_host, int32_t T, int32_t cycle_frame_num, int32_t E);
int wtk_replay_set_precise(const wtk_replay_config *cfg, const wtk_replay_set_track *tracks_host, const wtk_replay_set_track *tracks_dev,
                           const wtk_replay_set_frames *frames_host, const wtk_replay_set_frames *frames_dev, int32_t T, int32_t guard_cycles,
                           int32_t E, const double *track_dev, int32_t n_super, const double *share_dev, const int32_t *pos_dev,
                           const int32_t *move_dev, int32_t max_crop_px, double *err_dev, int32_t *counts_dev, double *track_summary_dev,
                           double *summary_dev, double *scratch_dev, int64_t scratch_doubles, const int32_t *stop_dev, void *stream);
int wtk_replay_set_precise_objective(const wtk_replay_config *cfg, const wtk_replay_set_track *tracks_host,
                                     const wtk_replay_set_track *tracks_dev, const wtk_replay_set_frames *frames_host,
                                     const wtk_replay_set_frames *frames_dev, int32_t T, int32_t guard_cycles, int32_t kind, int32_t E,
                                     const double *track_dev, int32_t n_super, const double *a_dev, const double *b_dev,
                                     const int32_t *valid_dev, const double *share_dev, int32_t *pos_dev, int32_t *move_dev,
                                     int32_t max_crop_px, double *track_summary_dev, double *summary_dev, double *scratch_dev,
                                     int64_t scratch_doubles, int32_t objective, double *objective_dev, double *track_objective_dev,
                                     const int32_t *stop_dev, void *stream);

/* ------------------------------------------------------------------------------------------
 * A set whose recordings were taken at different scales: every track with its own camera size, microscope size and
 * unit factors, as the reference derives a TimingConfig's pixel sizes and DataAnalyzer.change_unit's factors from the recording's own
 * px_per_mm.  The cycle structure (imaging_frame_num, moving_frame_num, pred_frame_num) stays `cfg`'s for all tracks.
 *
 * wtk_replay_set_geometry   one entry per track, beside wtk_replay_set_track: the camera and microscope sizes in pixels that `cfg` holds for
 *     all tracks elsewhere, and change_unit's (time, distance, speed) factors that wtk_replay_analysis_config holds for all tracks
 *     elsewhere.  geom_host [T] is read by the checks, geom_dev [T] (the same bytes, uploaded once by the caller) by the kernels.
 * The *_geom entry points are the entry points of the same name without the suffix, with the table: every (track, experiment) pair has the
 *     bits of the single-track entry point called with the track's own sizes in its wtk_replay_config (and, for the analysis, the track's
 *     factors in its wtk_replay_analysis_config); pooled figures add the tracks as before.  The same launches: their number does not depend
 *     on T.  geom_host = geom_dev = NULL: `cfg`'s sizes and `acfg`'s factors for every track, which is what the entry points without the
 *     suffix pass.  The factors are read by wtk_replay_set_analyze_geom alone (there `acfg`'s three factors are not read when a table is given).
 * Refused (error code, nothing launched) beyond what the entry point without the suffix refuses: one of the two table pointers null and
 *     the other not; for track t (named by index) a camera smaller than the microscope or a negative microscope size; in the analysis a
 *     factor that is not finite.
 * ------------------------------------------------------------------------------------------ */
typedef struct wtk_replay_set_geometry {
    int32_t cam_w, cam_h, mic_w, mic_h;            /* TimingConfig.camera_size_px, micro_size_px of this track */
    double time_factor, dist_factor, speed_factor; /* change_unit of this track's log; 1, 1, 1 for unit "frame" */
} wtk_replay_set_geometry;
int wtk_replay_set_scan_geom(const wtk_replay_config *cfg, const wtk_replay_set_track *tracks_host, const wtk_replay_set_track *tracks_dev,
                             const wtk_replay_set_geometry *geom_host, const wtk_replay_set_geometry *geom_dev, int32_t T, int32_t guard_cycles,
                             int32_t kind, int32_t E, const double *track_dev, int32_t n_super, const double *a_dev, const double *b_dev,
                             const int32_t *valid_dev, const double *share_dev, int32_t *pos_dev, int32_t *move_dev, const int32_t *stop_dev,
                             void *stream);
int wtk_replay_set_rows_geom(const wtk_replay_config *cfg, const wtk_replay_set_track *tracks_host, const wtk_replay_set_track *tracks_dev,
                             const wtk_replay_set_geometry *geom_host, const wtk_replay_set_geometry *geom_dev, int32_t T, int32_t guard_cycles,
                             int32_t E, const double *track_dev, int32_t n_super, const double *share_dev, const int32_t *pos_dev,
                             const int32_t *move_dev, double *track_summary_dev, double *summary_dev, double *scratch_dev,
                             int64_t scratch_doubles, const int32_t *stop_dev, void *stream);
int wtk_replay_set_objective_geom(const wtk_replay_config *cfg, const wtk_replay_set_track *tracks_host, const wtk_replay_set_track *tracks_dev,
                                  const wtk_replay_set_geometry *geom_host, const wtk_replay_set_geometry *geom_dev, int32_t T,
                                  int32_t guard_cycles, int32_t kind, int32_t E, const double *track_dev, int32_t n_super, const double *a_dev,
                                  const double *b_dev, const int32_t *valid_dev, const double *share_dev, int32_t *pos_dev, int32_t *move_dev,
                                  double *track_summary_dev, double *summary_dev, double *scratch_dev, int64_t scratch_doubles,
                                  int32_t objective, double *objective_dev, double *track_objective_dev, const int32_t *stop_dev,
                                  void *stream);
int wtk_replay_set_precise_geom(const wtk_replay_config *cfg, const wtk_replay_set_track *tracks_host, const wtk_replay_set_track *tracks_dev,
                                const wtk_replay_set_geometry *geom_host, const wtk_replay_set_geometry *geom_dev,
                                const wtk_replay_set_frames *frames_host, const wtk_replay_set_frames *frames_dev, int32_t T,
                                int32_t guard_cycles, int32_t E, const double *track_dev, int32_t n_super, const double *share_dev,
                                const int32_t *pos_dev, const int32_t *move_dev, int32_t max_crop_px, double *err_dev, int32_t *counts_dev,
                                double *track_summary_dev, double *summary_dev, double *scratch_dev, int64_t scratch_doubles,
                                const int32_t *stop_dev, void *stream);
int wtk_replay_set_precise_objective_geom(const wtk_replay_config *cfg, const wtk_replay_set_track *tracks_host,
                                          const wtk_replay_set_track *tracks_dev, const wtk_replay_set_geometry *geom_host,
                                          const wtk_replay_set_geometry *geom_dev, const wtk_replay_set_frames *frames_host,
                                          const wtk_replay_set_frames *frames_dev, int32_t T, int32_t guard_cycles, int32_t kind, int32_t E,
                                          const double *track_dev, int32_t n_super, const double *a_dev, const double *b_dev,
                                          const int32_t *valid_dev, const double *share_dev, int32_t *pos_dev, int32_t *move_dev,
                                          int32_t max_crop_px, double *track_summary_dev, double *summary_dev, double *scratch_dev,
                                          int64_t scratch_doubles, int32_t objective, double *objective_dev, double *track_objective_dev,
                                          const int32_t *stop_dev, void *stream);

/* ------------------------------------------------------------------------------------------
 * The per-cycle ResMLP targets of a population of E models of one structure in one call: what Replay.mlp computes model by model
 * (wtk_mlp_predict_track, the float32 clip, the first box's corner), in the layout wtk_replay_scan reads for WTK_REPLAY_MLP, bit for bit.
 *   layers ...        the structure (in_dim, out_dim, relu of every layer; batch_norm is not looked at), as for wtk_mlp_folded_floats
 *   blob_dev          [E][wtk_mlp_folded_floats(...)] float32, 16-byte aligned: wtk_mlp_trainer_fold's output, or host-folded blobs uploaded
 *   track32_dev       [n_track][4] float32 xywh, 16-byte aligned (the gather's track);  track_dev: the float64 track (the corner b)
 *   anchors_dev       [n_cycles] anchor frames; the gather reads frames anchor + input_frames_host[j], j < n_in
 *   a_dev             [n_cycles][E][2] = (double)clamp(prediction, -bound, bound) in float32 with NaN kept; 0 where the sample is invalid
 *   b_dev             [n_cycles][E][2] = track_dev's (x, y) at clamp(anchor + input_frames_host[0], 0, n_track - 1)
 *   valid_dev         [n_cycles][E] = 0 where a gathered frame lies outside the track or a box is not finite
 * One launch on `stream`; nothing is allocated, nothing waited for.  stop_dev (nullable): when *stop_dev != 0 the launch writes nothing.
 * One workgroup per (model, run of 16-cycle tiles) stages the blob in LDS once; wtk_replay_mlp_targets_waves(blob floats) is the number of wavefronts
 * that fit next to it (at most 8; blobs above 32704 floats are read from global memory).
 * Refused (error code, nothing launched): out_dim != 2, n_in outside 1..16 or n_in * 4 != in_dim, E < 1, n_cycles < 1, n_track < 1, a structure
 *     wtk_mlp_create refuses, a required pointer that is null or misaligned.
 * ------------------------------------------------------------------------------------------ */
int wtk_replay_mlp_targets(const wtk_mlp_train_layer *layers, int32_t n_layers, int32_t n_blocks, int32_t layers_per_block, const float *blob_dev, int32_t E,
                           const float *track32_dev, const double *track_dev, int32_t n_track, const int32_t *anchors_dev, int32_t n_cycles,
                           const int32_t *input_frames_host, int32_t n_in, float bound, double *a_dev, double *b_dev, int32_t *valid_dev,
                           const int32_t *stop_dev, void *stream);
int32_t wtk_replay_mlp_targets_waves(int64_t blob_floats);
/* wtk_replay_mlp_targets with a clip bound per cycle: bounds_dev [n_cycles] float32 on the device, cycle c's prediction is clamped to
 * +-bounds_dev[c] (a set whose tracks were recorded at different px_per_mm: MLPController's bound max_speed px_per_mm / fps pred_frames[0]
 * is the track's own).  The same launch; a constant array gives wtk_replay_mlp_targets' bits.  Refused beyond what
 * wtk_replay_mlp_targets refuses: a null bounds_dev. */
int wtk_replay_mlp_targets_bounds(const wtk_mlp_train_layer *layers, int32_t n_layers, int32_t n_blocks, int32_t layers_per_block, const float *blob_dev,
                                  int32_t E, const float *track32_dev, const double *track_dev, int32_t n_track, const int32_t *anchors_dev,
                                  int32_t n_cycles, const int32_t *input_frames_host, int32_t n_in, const float *bounds_dev, double *a_dev,
                                  double *b_dev, int32_t *valid_dev, const int32_t *stop_dev, void *stream);

/* ------------------------------------------------------------------------------------------
 * The YOLO controller's closed loop from device-resident state (csrc/replay_yolo.hip): the one experiment kind whose
 * targets depend on the camera view.  E = 1; pos_dev / move_dev are the scan's [n_cycles][1][2] arrays, filled cycle by cycle.  The caller
 * writes pos_dev[0] (the clamped init position) and then enqueues, per cycle c on ONE stream: wtk_yolo_predict_views (B = 1,
 * pos_xy_dev = pos_dev + 2 c, the controller's decision view) and wtk_replay_yolo_step.  Nothing goes to the host in between.
 *
 * wtk_replay_yolo_step   HipYoloController.provide_movement_vector on xywh_dev (float32 [4], view pixels, NaN x 4 = no detection) as numpy 2
 *     evaluates it on a float32 row: (0, 0) unless all four are finite; else per axis mid = x + w / 2 and mid - cam_size / 2 in float32,
 *     rounded half to even.  Then the scan's moving_frame_num motor steps (the same device function).  Writes move_dev[c] and, where
 *     c + 1 < n_cycles, pos_dev[c + 1].  One thread, plain stores.
 * wtk_replay_yolo_positions   one thread per logged frame: frame_pos_dev [R][2], the platform position at that frame's camera picture
 *     (wtk_replay_rows' position of the row): what wtk_yolo_predict_views takes as pos_xy_dev for the log's detections.
 * wtk_replay_yolo_track   one thread per logged frame: xywh_dev [R][4] float32 view-pixel detections -> track_dev [R][4] float64 absolute
 *     boxes, what wtk_replay_rows reads.  TrackLogger._write_rows' dtype rule, per cycle: all L rows finite -> x + cam_x in float32, then
 *     widened; any row NaN -> the whole cycle in float64.  NaN rows stay NaN (wtk_replay_rows logs them as 0, 0, 0, 0).
 * Refused (error code, no memory touched): what wtk_replay_scan refuses of the geometry, c outside [0, n_cycles), a camera or frame side
 * above 8192, a null pointer.
 * ------------------------------------------------------------------------------------------ */
int wtk_replay_yolo_step(const wtk_replay_config *cfg, int32_t n_cycles, int32_t c, const float *xywh_dev, const double *share_dev,
                         int32_t *pos_dev, int32_t *move_dev, void *stream);
int wtk_replay_yolo_positions(const wtk_replay_config *cfg, int32_t n_cycles, const double *share_dev, const int32_t *pos_dev,
                              const int32_t *move_dev, int32_t *frame_pos_dev, void *stream);
int wtk_replay_yolo_track(const wtk_replay_config *cfg, int32_t n_cycles, const float *xywh_dev, const int32_t *frame_pos_dev, double *track_dev,
                          void *stream);

/* ------------------------------------------------------------------------------------------
 * Background-subtraction worm boxes (csrc/box_ops.hip): BoxCalculator._calc_bounding_box (dataset/box_calculator.py:75-101) for gray
 * frames, on frames resident in device memory.  Everything enqueues on `stream`; nothing synchronises or allocates.
 *
 * Per selected frame f (frame_idx_dev[i], or i where frame_idx_dev is NULL), in exact integer arithmetic:
 *   m0 = |f - bg| > diff_thresh;  erode 5 x 5 and dilate 15 x 15 (= the reference's 5 x 5 opening followed by its 11 x 11 dilation), both
 *   over the in-image pixels of the window only;  for every 8-connected component A2 = twice the area of the polygon through the pixel
 *   centres of its outer border (cv.contourArea of the RETR_EXTERNAL / CHAIN_APPROX_NONE contour);  the winner has the largest A2, among
 *   equal A2 the one whose raster-first pixel comes last;  boxes_dev[i] = (min x, min y, width, height) of the winner in pixels,
 *   (0, 0, 0, 0) where nothing is foreground.
 * area2_dev [n_sel] int64 (nullable): the winner's A2, 0 without foreground.  mask_dev [n_sel][H][W] uint8 (nullable): the mask after
 * the morphology, 0 / 255.  boxes_dev may be NULL when area2_dev is: only the mask stage runs (its bit-packed result stays in scratch).
 * Faults: a frame index outside [0, n_frames) reads nothing and gives box (-1, -1, -1, -1), area -1 and a zero mask; so does a frame
 * whose border trace exceeds its bound of 8 H W steps (a defect, never seen).  *fault_count_dev += the number of such frames.
 * scratch: wtk_boxes_scratch_bytes(H, W, n_sel) bytes, 8-byte aligned: [n_sel] uint64 winner keys, then [n_sel][H][ceil(W / 32)] uint32
 * mask words (bit b of word c of a row = pixel 32 c + b).  wtk_boxes_scratch_bytes returns -1 for sizes wtk_boxes refuses.
 * Refused (error code, nothing launched): a null pointer, n_frames / H / W / n_sel <= 0, H * W > 2^30, diff_thresh outside 1 .. 255,
 * scratch too small or misaligned, more than 2^31 - 1 blocks in one call (split the selection).
 * ------------------------------------------------------------------------------------------ */
int64_t wtk_boxes_scratch_bytes(int32_t H, int32_t W, int32_t n_sel);
int wtk_boxes(const uint8_t *frames_dev, int32_t n_frames, int32_t H, int32_t W, const uint8_t *bg_dev, const int32_t *frame_idx_dev,
              int32_t n_sel, int32_t diff_thresh, int32_t *boxes_dev, int64_t *area2_dev, uint8_t *mask_dev, int32_t *fault_count_dev,
              void *scratch, int64_t scratch_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * The reference's analysis of a replayed population (csrc/replay_analysis.hip): DataAnalyzer.initialize / clean /
 * change_unit / describe / calc_anomalies / print_stats (eval/data_analyzer.py:54-107, 121-159, 178-213, 326-416) and the Plotter's
 * per-cycle and per-cycle-step aggregates (eval/plotter.py:164-168, 203-213, 237-245) of every experiment of a scan, from the scan's
 * pos_dev / move_dev.  Nothing of size [E][R][columns] is stored: a row's columns are recomputed where they are consumed, with the device
 * functions wtk_replay_rows calls.  Everything enqueues on `stream`; nothing synchronises or allocates.
 *
 * Columns (WTK_ANALYSIS_COL_*) of logged row r of an experiment, float64 in the reference's order of operations: frame = time = r,
 * cycle, cycle_step = r mod L, the row's 14 values plt_x .. wrm_h, wrm_center = wrm + size / 2 and mic_center likewise, wrm_speed_x =
 * (wrm_center_x[r] - wrm_center_x[r - period]) / period (NaN for r < period; over the whole log, kept or not), wrm_speed = sqrt(sx sx +
 * sy sy), worm_deviation_x = wrm_center_x - mic_center_x, worm_deviation = sqrt(dx dx + dy dy), bbox_error as wtk_replay_rows computes
 * it.  Then every column is rounded as DataFrame.round(5) rounds: rint(v 1e5) / 1e5, half to even, non-finite values unchanged.
 * precise_error is precise_pair_dev[r][e] unrounded ([R][E]: the first R E doubles of wtk_replay_precise's scratch_dev; NaN = no value).
 * clean, on the rounded values and in this order: imaging_only keeps the rows of the imaging phase; use_bounds keeps a row where
 * (wrm_x .. wrm_h all finite and wrm_x >= bounds[0], wrm_x + wrm_w <= bounds[2], wrm_y >= bounds[1], wrm_y + wrm_h <= bounds[3]) or the
 * microscope box passes the same test (what the reference's in-place mask update makes of its has_pred rule); trim_cycles then drops
 * cycle 0 and the LARGEST cycle among the rows that survived the first two (per experiment).  change_unit: the kept, rounded values
 * times time_factor (time), dist_factor (positions, sizes, centres, deviations), speed_factor (speeds); errors, frame, cycle and
 * cycle_step unchanged.  The caller passes (1, 1, 1) for unit "frame" and (ms_per_frame / 1000, mm_per_px 1000, their quotient) for "sec".
 *
 * Outputs (all nullable), over the kept rows of experiment e and the n_cols columns named in columns_host:
 *   describe_dev [E][n_cols][5 + Q]   count of non-NaN values, mean, std (ddof 1, two passes about the computed mean), min, the Q
 *       percentiles of percentiles_host (numpy's `linear`: pos = q (n - 1), lo = floor(pos), t = pos - lo; a + (b - a) t for t < 0.5,
 *       else b - (b - a)(1 - t)), max.  Count 0: NaN but for the count; count 1: std NaN.
 *   cycle_max_dev, cycle_mean_dev [E][n_log][n_cols]   per logged cycle, NaN values skipped, NaN where the cycle keeps none.
 *   step_quantiles_dev [E][L][n_cols][Q], step_count_dev [E][L][n_cols] int32   the same percentiles and the count per cycle_step.
 *   anomaly_counts_dev [E][7] int64   calc_anomalies on the unit-changed values: rows with wrm_speed >= min_speed, bbox_error >=
 *       min_bbox_error, worm_deviation >= min_dist_error, wrm_w >= min_width, wrm_h >= min_height, (no_preds and a non-finite worm box),
 *       any of them.  Comparisons with NaN are false; +inf switches a threshold off.  anomaly_mask_dev [E][R] uint8: bit k = kind k, 0 on
 *       rows that are not kept.
 *   stats_dev [E][4] int64   print_stats: removed rows, kept rows with a NaN in the worm box, distinct cycles kept, kept rows with
 *       bbox_error > 1e-7.
 * Sums have a fixed order that depends on R alone (thread t of 512 adds the segment's rows t, t + 512, ... in order, then a binary
 * tree): an experiment gives the same bits alone and in any population.  Order statistics are exact: segments (the experiment, or one
 * cycle step of it) of up to max_lds_rows rows are sorted in LDS, longer ones go through a radix select over recomputed values; both
 * return the same bits.  max_lds_rows = 0: the default, 19960 (160 KiB of LDS); larger values mean the default.
 * scratch_dev: wtk_replay_analysis_scratch_doubles(E, R, n_cols, Q) doubles (-1: negative sizes).
 * Refused (error code, nothing launched): what wtk_replay_rows refuses of the geometry, a required pointer that is null, n_cols outside
 * 1..WTK_ANALYSIS_MAX_COLUMNS, Q outside 0..WTK_ANALYSIS_MAX_PERCENTILES, an unknown column, a percentile outside [0, 1], period < 1,
 * the precise_error column without precise_pair_dev, max_lds_rows < 0, scratch too small.
 * ------------------------------------------------------------------------------------------ */
#define WTK_ANALYSIS_COL_FRAME 0
#define WTK_ANALYSIS_COL_CYCLE 1
#define WTK_ANALYSIS_COL_PLT_X 2
#define WTK_ANALYSIS_COL_PLT_Y 3
#define WTK_ANALYSIS_COL_CAM_X 4
#define WTK_ANALYSIS_COL_CAM_Y 5
#define WTK_ANALYSIS_COL_CAM_W 6
#define WTK_ANALYSIS_COL_CAM_H 7
#define WTK_ANALYSIS_COL_MIC_X 8
#define WTK_ANALYSIS_COL_MIC_Y 9
#define WTK_ANALYSIS_COL_MIC_W 10
#define WTK_ANALYSIS_COL_MIC_H 11
#define WTK_ANALYSIS_COL_WRM_X 12
#define WTK_ANALYSIS_COL_WRM_Y 13
#define WTK_ANALYSIS_COL_WRM_W 14
#define WTK_ANALYSIS_COL_WRM_H 15
#define WTK_ANALYSIS_COL_TIME 16
#define WTK_ANALYSIS_COL_CYCLE_STEP 17
#define WTK_ANALYSIS_COL_WRM_CENTER_X 18
#define WTK_ANALYSIS_COL_WRM_CENTER_Y 19
#define WTK_ANALYSIS_COL_MIC_CENTER_X 20
#define WTK_ANALYSIS_COL_MIC_CENTER_Y 21
#define WTK_ANALYSIS_COL_WRM_SPEED_X 22
#define WTK_ANALYSIS_COL_WRM_SPEED_Y 23
#define WTK_ANALYSIS_COL_WRM_SPEED 24
#define WTK_ANALYSIS_COL_WORM_DEVIATION_X 25
#define WTK_ANALYSIS_COL_WORM_DEVIATION_Y 26
#define WTK_ANALYSIS_COL_WORM_DEVIATION 27
#define WTK_ANALYSIS_COL_BBOX_ERROR 28
#define WTK_ANALYSIS_COL_PRECISE_ERROR 29
#define WTK_ANALYSIS_N_COLUMNS 30
#define WTK_ANALYSIS_MAX_COLUMNS 32
#define WTK_ANALYSIS_MAX_PERCENTILES 16
typedef struct wtk_replay_analysis_config {
    double bounds[4];          /* x0, y0, x1, y1 (read where use_bounds != 0) */
    double time_factor, dist_factor, speed_factor; /* change_unit; 1, 1, 1 for unit "frame" */
    double min_speed, min_bbox_error, min_dist_error, min_width, min_height; /* calc_anomalies; +inf = off */
    int32_t period;            /* frames the speed looks back (initialize) */
    int32_t imaging_only, use_bounds, trim_cycles; /* clean */
    int32_t no_preds;          /* calc_anomalies */
    int32_t reserved;
} wtk_replay_analysis_config;
int64_t wtk_replay_analysis_scratch_doubles(int32_t E, int64_t R, int32_t n_cols, int32_t Q);
int wtk_replay_analyze(const wtk_replay_config *cfg, const wtk_replay_analysis_config *acfg, int32_t E, int32_t n_cycles,
                       const double *track_dev, int32_t n_track, const double *share_dev, const int32_t *pos_dev, const int32_t *move_dev,
                       const double *precise_pair_dev, const int32_t *columns_host, int32_t n_cols, const double *percentiles_host,
                       int32_t Q, int32_t max_lds_rows, double *describe_dev, double *cycle_max_dev, double *cycle_mean_dev,
                       double *step_quantiles_dev, int32_t *step_count_dev, int64_t *anomaly_counts_dev, uint8_t *anomaly_mask_dev,
                       int64_t *stats_dev, double *scratch_dev, int64_t scratch_doubles, void *stream);

/* ------------------------------------------------------------------------------------------
 * The analysis of a population replayed on a SET of tracks (csrc/replay_set_analysis.hip): what the reference's Plotter
 * computes from several logs at once (eval/plotter.py:37-40: every log through its own DataAnalyzer.initialize / clean / change_unit, the
 * cleaned frames concatenated with a log_num column), from a set scan's pos_dev / move_dev.  Log (t, e) is wtk_replay_analyze's experiment e
 * on track t alone: frame, time, cycle and cycle_step count from the track's own row 0, wrm_speed is NaN on the first `period` rows of every
 * track, and trim_cycles drops cycle 0 and that log's own largest surviving cycle.
 *
 * Per-track outputs (all nullable), each bit-equal to wtk_replay_analyze's output on that track alone, for any E, any T, any place of the track
 * in the set and any max_lds_rows.  With row0[t] = the sum of R and log0[t] = the sum of n_log over the tracks before t:
 *   track_describe_dev [T][E][n_cols][5 + Q], track_step_quantiles_dev [T][E][L][n_cols][Q], track_step_count_dev [T][E][L][n_cols] int32,
 *   track_anomaly_counts_dev [T][E][7] int64, track_stats_dev [T][E][4] int64:  track t's block is the t-th.
 *   cycle_max_dev, cycle_mean_dev [E][sum n_log][n_cols]:  track t's cycles are the rows log0[t] .. log0[t] + n_log - 1 of every experiment (all
 *       of it is groupby(["log_num", "cycle"]) of the concatenation).
 *   anomaly_mask_dev [E][sum R] uint8:  track t's rows are the columns from row0[t] (wtk_replay_set_precise's err_dev layout).
 * Pooled outputs (all nullable): the statistics over the concatenation of the T cleaned logs of experiment e, in track order.
 *   describe_dev [E][n_cols][5 + Q], step_quantiles_dev [E][L][n_cols][Q], step_count_dev [E][L][n_cols] int32.  Count, min, max and every
 *       percentile are exact: the order statistics of the union of the kept non-NaN values under numpy's `linear` rule.  Mean and std in a
 *       fixed order: sum_t = track t's sum with wtk_replay_analyze's bits; S = (...((sum_0 + sum_1) + sum_2)...) over the tracks that keep a
 *       value, starting from the first such track's own sum (not from 0.0); N = the sum of the counts; mean = S / N; ss_t = the sum of
 *       (v - mean)^2 about the POOLED mean in the per-track order, chained the same way; std = sqrt(SS / (N - 1)).  N = 0: NaN but for the
 *       count; N = 1: std NaN.  T = 1: the per-track bits.
 *   anomaly_counts_dev [E][7], stats_dev [E][4] int64: integer sums over the tracks (distinct cycles: distinct (log_num, cycle) pairs).
 * precise_rows_dev (nullable) [E][sum R]: the precise_error column, unrounded: wtk_replay_set_precise's err_dev.
 * No floating-point atomics: an experiment gives the same bits alone and in any population; the pooled bits depend on the order of the tracks
 * through the chain above only.  Segments are sorted in LDS or go through the radix select as for wtk_replay_analyze; the way is chosen per
 * launch from max_lds_rows (0 = 19960): by the longest track for the per-track launches, by the sum over the tracks for the pooled ones.
 * Nine launches with every output asked for, whatever T is (DESIGN.md section 28 lists them).  Everything enqueues on `stream`; nothing synchronises or allocates.
 * scratch_dev: wtk_replay_set_analysis_scratch_doubles(tracks_host, T, cycle_frame_num, E, n_cols, Q) doubles (-1: a bad table or negative
 *     sizes): the prefix sums row0 / log0, the per-(track, experiment) last cycles and integer counts.
 * Refused (error code, nothing launched), a track named by its index: everything wtk_replay_set_rows refuses of the track table; everything
 *     wtk_replay_analyze refuses of the spec (the precise_error column without precise_rows_dev); T E n_cols L or the cycle launch's blocks
 *     >= 2^31; sum R >= 2^31; scratch too small; a required pointer that is null.
 * ------------------------------------------------------------------------------------------ */
int64_t wtk_replay_set_analysis_scratch_doubles(const wtk_replay_set_track *tracks_host, int32_t T, int32_t cycle_frame_num, int32_t E,
                                                int32_t n_cols, int32_t Q);
int wtk_replay_set_analyze(const wtk_replay_config *cfg, const wtk_replay_analysis_config *acfg, const wtk_replay_set_track *tracks_host,
                           const wtk_replay_set_track *tracks_dev, int32_t T, int32_t guard_cycles, int32_t E, const double *track_dev,
                           int32_t n_super, const double *share_dev, const int32_t *pos_dev, const int32_t *move_dev,
                           const double *precise_rows_dev, const int32_t *columns_host, int32_t n_cols, const double *percentiles_host,
                           int32_t Q, int32_t max_lds_rows, double *track_describe_dev, double *cycle_max_dev, double *cycle_mean_dev,
                           double *track_step_quantiles_dev, int32_t *track_step_count_dev, int64_t *track_anomaly_counts_dev,
                           uint8_t *anomaly_mask_dev, int64_t *track_stats_dev, double *describe_dev, double *step_quantiles_dev,
                           int32_t *step_count_dev, int64_t *anomaly_counts_dev, int64_t *stats_dev, double *scratch_dev,
                           int64_t scratch_doubles, void *stream);
/* wtk_replay_set_analyze with the per-track geometry table (wtk_replay_set_geometry above): log (t, e) is
 * wtk_replay_analyze's experiment e on track t alone with the track's camera and microscope sizes and with the track's three factors in the
 * place of acfg's; the pooled statistics are taken over the values so converted, as the reference concatenates logs that each went through
 * their own change_unit.  acfg's bounds and thresholds stay one for all tracks.  NULL tables: wtk_replay_set_analyze. */
int wtk_replay_set_analyze_geom(const wtk_replay_config *cfg, const wtk_replay_analysis_config *acfg, const wtk_replay_set_track *tracks_host,
                                const wtk_replay_set_track *tracks_dev, const wtk_replay_set_geometry *geom_host,
                                const wtk_replay_set_geometry *geom_dev, int32_t T, int32_t guard_cycles, int32_t E, const double *track_dev,
                                int32_t n_super, const double *share_dev, const int32_t *pos_dev, const int32_t *move_dev,
                                const double *precise_rows_dev, const int32_t *columns_host, int32_t n_cols, const double *percentiles_host,
                                int32_t Q, int32_t max_lds_rows, double *track_describe_dev, double *cycle_max_dev, double *cycle_mean_dev,
                                double *track_step_quantiles_dev, int32_t *track_step_count_dev, int64_t *track_anomaly_counts_dev,
                                uint8_t *anomaly_mask_dev, int64_t *track_stats_dev, double *describe_dev, double *step_quantiles_dev,
                                int32_t *step_count_dev, int64_t *anomaly_counts_dev, int64_t *stats_dev, double *scratch_dev,
                                int64_t scratch_doubles, void *stream);

/* ------------------------------------------------------------------------------------------
 * The precise tracking error of a replayed population (csrc/replay_precise.hip): ErrorCalculator.calculate_precise
 * (eval/error_calculator.py:64-160) of every (experiment, logged frame) pair of a scan, with wtk_precise_error's counts and bits for the
 * row wtk_replay_rows logs.  frames_dev [n_frames][H][W] gray with n_frames >= R: row r is frame r.  bg_dev [H][W].  A pixel is
 * foreground where |frame - bg| > diff_thresh.
 *
 * wtk_replay_precise   one workgroup per logged frame.  The segmented mask of frame r depends on the frame, the background and the
 *     track's row r only: it is built once, as an exclusive summed-area table in LDS over the row's discretised box grown by one pixel
 *     (the logged box (x - cam) + cam moves an edge by at most one pixel), and every experiment is answered with two rectangle sums
 *     (the logged worm box; worm x microscope, 0 where the intersection is empty).  A pair whose logged box is not inside the table's
 *     region, and every pair of a frame whose table needs more than max_crop_px uint32 cells ((h + 3) x pitch, pitch = (w + 3) | 1 for a
 *     w x h box away from the frame's edge), is computed by the direct walk over the crop, as wtk_precise_error does (a second launch
 *     without LDS, which does nothing for frames that left no such pair): same counts, so max_crop_px never changes a bit.  max_crop_px = 0: the default, 160 KiB of LDS = 40960 cells; larger values mean the default.
 *   err_dev [E][R] float64 (nullable): 1 - inside / total, 0 where total = 0, NaN for an illegal logged worm box.  counts_dev
 *     [E][R][2] int32 (nullable): (total, inside), (0, 0) on NaN rows.
 *   summary_dev [E][WTK_REPLAY_PRECISE_SUMMARY_DOUBLES]: [0] sum of err over the rows with a value (not NaN), [1] their number, [2] [3]
 *     the same over the imaging rows of the cycles 1 .. n_log - 2 (DataAnalyzer.clean(trim_cycles=True, imaging_only=True)), [4] rows with
 *     err > 1e-7, [5] NaN rows.  NaN rows enter no sum (pandas' mean of the column).  Sums are taken in wtk_replay_rows' fixed order
 *     (chunks of 4096 rows, 256 lane-serial accumulators, a binary tree, chunk partials in index order): an experiment gives the same
 *     bits alone and in any population.  scratch_dev: wtk_replay_precise_scratch_doubles(E, R) doubles (-1: negative sizes): the
 *     E R pair errors, the chunk partials and R int32 flags.
 * wtk_replay_precise_objective   wtk_replay_scan, wtk_replay_precise without per-pair output, then objective_dev[e] = one float64
 *     division: WTK_REPLAY_POBJ_TRIMMED_PRECISE summary[2] / summary[3], _MEAN_PRECISE [0] / [1], _NON_PERFECT [4] / [1]; 0 / 0 is NaN.
 * stop_dev (nullable): as for wtk_replay_objective.
 * Refused (error code, nothing launched): what wtk_replay_rows refuses of the geometry, a required pointer that is null, n_frames < R,
 *     (H, W) other than the config's (frame_h, frame_w), H * W > 2^30, max_crop_px < 0, scratch too small; the objective: what
 *     wtk_replay_scan refuses, an unknown objective, the trimmed objective with fewer than 3 logged cycles.
 * ------------------------------------------------------------------------------------------ */
#define WTK_REPLAY_PRECISE_SUMMARY_DOUBLES 6
#define WTK_REPLAY_POBJ_TRIMMED_PRECISE 0
#define WTK_REPLAY_POBJ_MEAN_PRECISE 1
#define WTK_REPLAY_POBJ_NON_PERFECT 2
int64_t wtk_replay_precise_scratch_doubles(int32_t E, int64_t R);
int wtk_replay_precise(const wtk_replay_config *cfg, int32_t E, int32_t n_cycles, const double *track_dev, int32_t n_track,
                       const double *share_dev, const int32_t *pos_dev, const int32_t *move_dev, const uint8_t *frames_dev, int32_t n_frames,
                       int32_t H, int32_t W, const uint8_t *bg_dev, double diff_thresh, int32_t max_crop_px, double *err_dev,
                       int32_t *counts_dev, double *summary_dev, double *scratch_dev, int64_t scratch_doubles, const int32_t *stop_dev,
                       void *stream);
int wtk_replay_precise_objective(const wtk_replay_config *cfg, int32_t kind, int32_t E, int32_t n_cycles, const double *track_dev,
                                 int32_t n_track, const double *a_dev, const double *b_dev, const int32_t *valid_dev,
                                 const double *share_dev, int32_t *pos_dev, int32_t *move_dev, const uint8_t *frames_dev, int32_t n_frames,
                                 int32_t H, int32_t W, const uint8_t *bg_dev, double diff_thresh, int32_t max_crop_px, double *summary_dev,
                                 double *scratch_dev, int64_t scratch_doubles, int32_t objective, double *objective_dev,
                                 const int32_t *stop_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* WTK_HIP_H */
