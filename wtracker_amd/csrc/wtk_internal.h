// Internal declarations shared by the HOST-side translation units of libwtk_hip.so (round 6: csrc/wtk_api.hip was one file of 2 500 lines):
//   wtk_api.hip     errors, versions, ResMLP / track / recheck / crop entry points
//   wtk_plan.hip    the detector handle: model table, weight packing, graph planning (channel-slice views), launch schedule of the latency plan,
//                   stream pool, status page, create / destroy
//   wtk_run.hip     one forward pass: enqueue, the predict entry points, test hooks
//   wtk_hybrid.hip  the look-twice detector composed from the entry points above
// Kernel-side declarations live in wtk_kernels.h.
#pragma once
#include "../../include/wtk_hip.h"
#include "wtk_kernels.h"

#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

namespace wtk {
// thread-local error message of the C ABI (wtk_last_error); both return 1
int fail(const std::string &msg);
int fail_hip(const char *what, hipError_t e);
int ensure_attributes(int device); // kernel attributes, once per device
// the shapes the device's polynomial fit (polyfit_solve.h) admits, refused under the entry point's name
inline int check_fit_shape(const char *who, int32_t n_times, int32_t degree) {
    if (n_times <= 0 || n_times > kTrackMaxTimes) return fail(std::string(who) + ": 1..16 sample times");
    if (degree < 0 || degree + 1 > kTrackMaxCoef) return fail(std::string(who) + ": degree must be in [0, 7]");
    return 0;
}
}
#define HIP_TRY(expr)                                                                                                          \
    do {                                                                                                                       \
        hipError_t _e = (expr);                                                                                                \
        if (_e != hipSuccess) return wtk::fail_hip(#expr, _e);                                                                 \
    } while (0)

// Stream entry points launch on the handle's device whatever the caller's current device is, and leave the caller's
// current device as they found it (PyTorch tracks the same thread-local HIP state).
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int device) {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != device) {
            err = hipSetDevice(device);
            switched = err == hipSuccess;
        }
    }
    ~DeviceGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
};
#define DEVICE_GUARD(h)                                                                                                        \
    DeviceGuard _guard((h)->device);                                                                                           \
    if (_guard.err != hipSuccess) return wtk::fail_hip("selecting the handle's device", _guard.err)

inline uint16_t f32_to_f16_bits(float f) {
    _Float16 h = (_Float16)f; // round-to-nearest-even, host compiler builtin
    uint16_t b;
    std::memcpy(&b, &h, 2);
    return b;
}

inline float f16_bits_to_f32(uint16_t b) {
    _Float16 h;
    std::memcpy(&h, &b, 2);
    return (float)h;
}


// ---------------------------------------------------------------------------------------------
// the detector handle
// ---------------------------------------------------------------------------------------------
struct ConvSpec {
    std::string name;
    int cout, cin, k, stride, act;
};

struct ModelDims {
    int c[5];  // channel widths of P1..P5
    int n[4];  // C2f repeats of layers 2,4,6,8
    int hb, hc; // Detect hidden widths (box tower, cls tower)
    int nc;
};

struct Buf {
    size_t elems_per_image = 0; // h*w*C
    int h = 0, w = 0, C = 0;
    int f32 = 0; // 1: stored as fp32 whatever the handle's dtype (the Detect outputs: head logits are never rounded to fp16)
    void *ptr = nullptr;
};

enum OpKind { OP_STEM, OP_CONV, OP_POOL };

struct Op {
    OpKind kind;
    // conv
    int in_buf = -1, in_coff = 0, cin = 0;
    int out_buf = -1, out_coff = 0;
    int out2_buf = -1, out2_coff = 0;
    int res_buf = -1, res_coff = 0;
    int tail_op = -1; // index of a 1x1 op computed in this op's epilogue (the Detect towers' last 1x1 in conv3x3_halo, model.4.cv1 in conv_igemm, model.2.cv2 in conv3x3_c32's split form)
    int folded = 0;   // 1: this op runs inside another op's kernel
    int in2_buf = -1, in2_coff = 0, in2_split = 0; // half-resolution source of the first in2_split input channels (ConvArgs::in2)
    int cout = 0, cout_pad = 0, k = 1, stride = 1, act = 1;
    int cfg = 0;
    int K = 0, Kpad = 0;
    int tile_w = 0;
    int halo = 0; // 1: conv3x3_halo kernel, 2: conv3x3_c32 kernel
    int side = 0;        // 1: runs on the handle's side stream (Detect towers of P3 / P4)
    int wait_feat = -1;  // side ops: feature event (0: P3 ready, 1: P4 ready) to wait for before the first one
    int signal_feat = -1; // main ops: record this feature event after the op
    void *w = nullptr; // packed device weights
    float *bias = nullptr;
    double macs_per_image = 0;
    int spec = -1; // index of the (first) conv blob this op computes, for wtk_yolo_debug_tensor
    int sk = 0;                  // latency plan: this conv runs on conv_sk_kernel (split-K implicit GEMM, conv_sk.hip)
    int sk_atoms = 0;            // ... with this many K atoms (conv_sk_slices(nk), or conv_sk_plan_atoms on a small throughput-plan handle)
    float *sk_partial = nullptr; // ... and this is its slab scratch ([slices][max_batch * ho * wo][cout_pad] fp32; null: one slice)
    unsigned *sk_tickets = nullptr; // ... and the arrival counters of its tiles (zero between launches; null: one slice, or WTK_SK_FINISH=1)
};

// Kernel classes of the profile (wtk_yolo_get_kernel_profile; the values are ABI).  The public class 1 ("conv") of wtk_yolo_get_profile is the sum of
// PROF_IGEMM, PROF_HALO, PROF_FUSED and PROF_C32.
enum ProfClass {
    PROF_STEM = 0,
    PROF_IGEMM = 1, // conv_igemm, conv_sk, conv1x1_wide, the strided window kernel
    PROF_POOL = 2,
    PROF_HEAD = 3,
    PROF_HALO = 4,  // conv3x3_halo (+ fused tails), conv3x3_ws64
    PROF_FUSED = 5, // fused front / C2f tail
    PROF_C32 = 6,   // conv3x3_c32
    PROF_SPARSE = 7, // conv3x3_halo launches of the sparse Detect box towers: counted with 0 FLOPs (the host does not know how many tiles were live)
};

// What one conv op of a forward pass launches at a batch size (wtk_run.hip: resolve_conv decides, issue_conv enqueues): the launcher, the profile class
// and the filled arguments — `a` for the implicit-GEMM family and split-K, `g` (next to the `a` it was derived from) for the window kernels.
enum LaunchKind { L_IGEMM, L_IGEMM_SPLIT, L_WIDE_1X1, L_HALO, L_HALO_SPLIT, L_C32, L_C32_SPLIT, L_WS64, L_S2WIN, L_S2WIN_SPLIT, L_SK };
struct ConvLaunch {
    LaunchKind kind;
    ProfClass cls;
    int cfg; // L_IGEMM, L_IGEMM_SPLIT: the tile configuration (ConvCfg)
    wtk::ConvArgs a;
    wtk::HaloArgs g;
};

struct wtk_yolo {
    int device = 0;
    int is_f16 = 1;
    int esize = 2;
    // WTK_F16X3: split-fp16 storage (wtk_kernels.h, kSplitScale).  Planned like the fp32 mode (is_f16 = 0, esize = 4: a split tensor
    // takes the same 4 bytes per value), launched on the SPLIT instantiations of the fp16 kernels with pseudo-channel arguments.
    int split = 0;
    const int *n_dyn = nullptr; // wtk_yolo_set_dynamic_batch: device-side count of the batch rows that matter (<= B of the call)
    int S_h = 0, S_w = 0, max_batch = 0;
    ModelDims dims;
    std::vector<Buf> bufs;
    std::vector<Op> ops;
    std::vector<std::pair<void *, size_t>> dev_allocs; // (pointer, bytes) of every dev_alloc
    int box_buf[3] = {-1, -1, -1}, cls_buf[3] = {-1, -1, -1};
    int lh[3] = {0, 0, 0}, lw[3] = {0, 0, 0};
    int cls_ld = 32;
    double macs_per_frame = 0;
    int anchors = 0;
    // staging for the host entry points and for letterboxing
    uint8_t *frames_dev = nullptr;
    size_t frames_cap = 0;
    uint8_t *lb_dev = nullptr;
    size_t lb_cap = 0;
    void *zero_page = nullptr;
    float *o_xywh = nullptr, *o_conf = nullptr;
    float *o_margin = nullptr; // decision margin of every frame of the last max_det = 1 call (wtk_yolo_last_margins_host / wtk_yolo_margin_buffer)
    int *o_anchor = nullptr;
    // scratch of the general NMS (max_det > 1), allocated at its first use
    float *nms_score = nullptr, *nms_box = nullptr;
    int *nms_cls = nullptr;
    // profiling
    int use_halo = 1;
    int front_debug = 0; // WTK_FRONT_DEBUG=1: the fused front also writes the model.0 / model.1 tensors (test hook)
    int use_tail = 1; // WTK_NO_FUSED_TAIL=1: Detect box.2 as its own launch (A/B switch)
    int use_tail_cls_split = 1; // WTK_NO_SPLIT_CLS_TAIL=1: f16x3 handles launch the class towers' last 1x1 on its own (A/B switch; fp16 handles: WTK_NO_FUSED_TAIL)
    int halo_small_blocks = 1; // WTK_HALO_SMALL_BLOCKS=0: always 256-pixel blocks (A/B switch)
    int halo_persist = 1; // WTK_HALO_PERSIST=0: one tile per block (A/B switch)
    int halo_slabs = 3; // WTK_HALO_SLABS=2: two-slab / vmcnt(0) schedule of conv3x3_halo_kernel (A/B switch)
    int use_c32s = 1;  // WTK_NO_C32S=1: the 32 -> 32 channel 3x3 layers of a split (f16x3) handle through conv_igemm_kernel (A/B switch)
    int use_s2win = 1; // WTK_NO_S2WIN=1: strided 3x3 convs through conv_igemm_kernel instead of the parity-plane window kernel (A/B switch)
    int use_ws64 = 1;  // WTK_NO_WS64=1: 64 -> 64 channel 3x3 layers through conv3x3_halo_kernel instead of the weight-stationary kernel (A/B switch)
    int use_wide = 1;  // WTK_NO_WIDE_1X1=1: every 1x1 conv through conv_igemm_kernel (A/B switch)
    int use_c2f = 0;   // ops[3..5] (model.2.m.0.cv1, m.0.cv2, model.2.cv2) run as ONE fused kernel (c2f_fused.hip)
    int use_front = 0; // ops[0..2] (stem, model.1, model.2.cv1) run as ONE fused kernel (front_fused.hip)
    int c2f_tail_asked = 0; // the create call carried WTK_PLAN_C2F_TAIL
    int c2f_tail_op = -1; // f16x3: the op (model.2.m.0.cv2) whose kernel also runs model.2.cv2 and does not store its own output z (wtk_plan.hip: fuse_c2f_split_tail)
    // Sparse Detect box towers (wtk_run.hip: resolve_sparse; DESIGN.md "Sparse box towers").  det[i]: the ops of level i's towers that a sparse call treats
    // differently — op0 the shared first 3x3 of both towers (run as its class half in place, as its box half behind the head's selection), box1 / box2 the rest
    // of the box tower.  The live mask, sel_anchor and sel_score belong to the handle (two lanes run two handles concurrently); the mask lies behind the zero
    // page in the same allocation (HaloArgs::live_off).
    int use_sparse_box = 1; // WTK_NO_SPARSE_BOX=1: every call dense (A/B and test switch)
    struct DetLevel {
        int op0 = -1, box1 = -1, box2 = -1;
    } det[3];
    size_t live_bytes = 0; // 0: this handle never runs sparse
    // List form (the default; WTK_SPARSE_LIST=0: the masked form, one full-grid launch per level and stage behind a cleared mask): counters and the two stages'
    // tile lists of live_list_cap[] entries behind the mask's live_mask_bytes, sized like the mask for max_batch (the layout: SparseMask below).
    int use_sparse_list = 1;
    int sparse_min_tenths = 0; // threshold of sparse_box_pays (below) for this handle's calls, in tenths of a round
    size_t live_mask_bytes = 0;
    unsigned live_list_cap[2] = {0, 0};
    unsigned sparse_grid[2] = {0, 0}; // grids of the two list launches of the last list-form sparse pass (wtk_yolo_debug_tensor: WTK_DEBUG_SPARSE_COUNTS)
    int *sel_anchor = nullptr;
    float *sel_score = nullptr;
    int sparse_B = 0; // > 0: the last forward pass (of this batch size) left the box towers sparse; wtk_yolo_debug_head / _debug_tensor complete them first.
                      // Host-side state, set when a pass is enqueued: eager passes only (a pass under stream capture stays dense, wtk_run.hip)
    ConvLaunch sparse_done[6]; // ... by these launches: box.0 and box.1 + box.2 of the three levels as that pass resolved them, mask off
    int num_cus = 0;
    // Latency plan (small batches: the reference's own operating point, one B = cycle_frame_num call and one B = 1 call per cycle,
    // yolo_controller.py:96-98,108-109).  Chosen when the handle is created — max_batch <= 4 and a reference-precision dtype, WTK_LATENCY_PLAN=0/1, or the caller's word (wtk_yolo_create_planned) —
    // and NOT per call: every conv behind the fused front then runs on conv_sk_kernel whatever the batch of the call, so a frame's logits do not
    // depend on the batch it arrives in.  The Detect towers' 1x1 tails are launches of their own in this plan.
    int latency = 0;
    // latency plan, round 6: the convs of one dependency level run as ONE grouped split-K launch on the caller's stream (sk_schedule).
    int sk_group = 1;                      // WTK_SK_GROUP=0: one launch per conv, in op order (test hook: the grouped launches must give the same bits)
    int sk_force_tile = -1, sk_force_form = -1; // WTK_SK_TILE / WTK_SK_FORM, read when the handle is created (test hooks: every tile and form gives the same bits)
    std::map<long long, wtk::SkChoice> sk_choices; // (launch or op, batch) -> what the split-K cost model chose (it runs once per key, not per call)
    // autotune of the latency plan (wtk_run.hip: sk_autotune): the first eager call at a batch size times every (tile, forms) candidate of every launch inside the
    // real forward pass and keeps the fastest; neither enters the arithmetic.  WTK_SK_AUTOTUNE=0: the cost model's choice.
    int sk_autotune = 1;
    int tune_pass = -1;                                     // >= 0: a timing pass is being enqueued (candidate = pass % candidates of the launch)
    std::map<long long, std::vector<wtk::SkChoice>> sk_cands; // (launch, batch) -> candidates, [0] = the cost model's
    std::map<long long, std::vector<float>> tune_ms;         // ... and the best time seen of each
    std::vector<hipEvent_t> tune_ev;                        // two per launch of lat_sched
    std::vector<long long> tune_key;                        // key of the launch timed through tune_ev[2 i], [2 i + 1] in this pass (-1: none)
    std::vector<int> sk_tuned;                              // batch sizes that have been tuned
    std::vector<std::vector<int>> lat_sched; // launches behind ops[0..2] in order: one op, or up to kSkGroupMax split-K ops that do not depend on each other
    int small_narrow = 0; // a small handle (max_batch <= 16, f16x3) runs window / implicit-GEMM layers whose grid leaves most CUs idle on 64-cout tiles (WTK_SMALL_NARROW=0: off)
    int halo_deep = 0;    // f16x3: the 64-cout x 128-pixel window tiles on the six-slab ring (small handles; WTK_HALO_DEEP)
    int *status_host = nullptr; // pinned, device-visible: sticky run-time flags written by the head kernels (wtk_yolo_status); a slot of the process-wide page
    int *status_dev = nullptr;  // ... and the device's address of the same word
    int status_static = 0;      // flags fixed at create time (none today)
    int profiling = 0;
    static constexpr int kProfKernels = 8, kProfEvents = 96; // (one slot per ProfClass)
    hipEvent_t ev[kProfEvents];
    // concurrency: the P3 / P4 Detect towers run on a side stream next to the PAN path
    // Side streams of one forward pass (op.side = index, 0 = the caller's stream): 1 / 2 = P3 / P4 Detect towers (they only need t15 / t18).  The pair is
    // process-wide (ensure_side_streams); wtk_yolo_set_side_streams(1) folds both towers onto stream 1, (0) keeps everything on the caller's stream.
    static constexpr int kSideStreams = 3;
    hipStream_t side_stream[kSideStreams] = {};
    hipEvent_t feat_ev[2] = {nullptr, nullptr}, side_done[kSideStreams] = {};
    int use_side = 1;
    int side_streams = 2;
    hipStream_t host_stream = nullptr; // pooled stream of the *_host entry points (taken at the first host call)
    int ev_created = 0;
    double prof_ms[kProfKernels] = {};
    double prof_flops[kProfKernels] = {};
    long long prof_launches[kProfKernels] = {};
};

namespace wtk {
// Sparse box towers pay from a call size on.  The tail behind the head — select, box.0 of the three levels from the live-tile list, box.1 + box.2 likewise, decode
// — is four dependent launches on the caller's stream, each at least one tile's walk (box.0 of P5: 144 taps), where the dense box towers of P3 / P4 ran beside the
// PAN path; what it saves grows with the rounds of blocks the dense launches took.  Measured (profiles/r08_notes.md part 2, one caller, sparse against dense per
// call, "rounds" = 256-pixel blocks of the dense P3 box.1 launch over the CUs): -5.7 % at 6.4 rounds (640 x 640, B = 64), -3.0 % at 4.0, -3.5 % at 3.2 (B = 32),
// -2.1 % at 2.4 (B = 24), -0.1 % at 1.7 (B = 17), +1.0 % at 1.2 and +2.3 % at 0.55 (384 x 384, B = 32 / 15 on a 32-frame handle).  The smallest measured size
// at which sparse is at least 1 % faster is 2.4 rounds; tests/test_gpu_sparse_box.py pins a call of 2.65 rounds (640 x 512, B = 33) as dense, so the threshold
// is the next measured point, 3.2 rounds, in tenths of a round.
// h8 x w8: the P3 map; (h8 + 1) x (w8 + 1) per image is the stacked flat geometry of a one-strip map (halo_geometry_stacked), a few per cent under it for a
// map cut into strips.  No CU count (a device that reports none): never sparse.
constexpr int kSparseBlockPx = 256, kSparseMinTenths = 32;
// kSparseMaxDenseBatch is not measured but fixed: a handle of at most 16 frames (a controller's) stays dense and allocates nothing, whatever the threshold.
// min_tenths: the handle's threshold (kSparseMinTenths; WTK_SPARSE_MIN_TENTHS, a measurement switch read at create, moves it).
constexpr int kSparseMaxDenseBatch = 16;
inline bool sparse_box_pays(int B, int h8, int w8, int num_cus, int min_tenths = kSparseMinTenths) {
    return num_cus > 0 && 10ll * B * (h8 + 1) * (w8 + 1) >= (long long)min_tenths * kSparseBlockPx * num_cus;
}
// Upper bound of the 128-pixel units ONE survivor marks for box.0: its 3 x 3 neighbourhood is three runs of <= 3 flat outputs, 2 * pitch + 3 outputs from the
// first to the last, in one column strip or in two neighbours (a strip is >= 3 columns wide whenever there are two).  box.1 + box.2: one unit per survivor.
inline int sparse_units_per_frame(int pitch, int strips) { return ((2 * pitch + 2) / 128 + 2) * (strips > 1 ? 2 : 1); }
// The sparse region: what lies behind the zero page in the handle's zero_page allocation, and the only place that knows its layout.
//   [kZeroPageBytes of zeros][mask: per level live0 then live1][kSparseCounters counters (HeadSparseArgs::count)][tile list of stage 0][tile list of stage 1]
// A mask array (live0: box.0's units, live1: box.1 + box.2's) is strips x ld bytes, rounded up to 4; ld = the 128-pixel units of a strip's stacked rows, rounded
// up to an even count.  The mask depends on the batch: wtk_plan.hip sizes it, and the lists, for max_batch from halo_geometry_stacked; resolve_sparse
// (wtk_run.hip) lays a call's arrays out for its B from the resolved launch's geometry, inside that size.  Counters and lists sit behind the HANDLE's mask size.
constexpr unsigned kZeroPageBytes = 256, kSparseCounters = 4;
struct SparseMask {
    int ld[3] = {0, 0, 0};
    unsigned off0[3] = {0, 0, 0}, off1[3] = {0, 0, 0}; // byte offsets of live0 / live1 of a level from the start of the region
    unsigned bytes = 0;                                // of the levels added so far
    int units_per_frame = 0;                           // most tiles one frame lists for box.0 (box.1 + box.2: one)
};
// level l (lh rows; pitch, strips: the stacked flat geometry of its window launch) of a batch of B frames, behind the levels before it
inline void sparse_mask_add_level(SparseMask &m, int l, int B, int lh, int pitch, int strips) {
    m.ld[l] = 2 * (int)(((long long)B * (lh + 1) * pitch + 255) / 256);
    const unsigned bytes = ((unsigned)strips * (unsigned)m.ld[l] + 3u) & ~3u;
    m.off0[l] = m.bytes, m.off1[l] = m.bytes + bytes;
    m.bytes += 2 * bytes;
    const int units = sparse_units_per_frame(pitch, strips);
    if (units > m.units_per_frame) m.units_per_frame = units;
}
// entries of the tile list of a stage (0: box.0, 1: box.1 + box.2) that B frames can fill
inline unsigned sparse_list_cap(const SparseMask &m, int stage, int B) { return stage ? (unsigned)B : (unsigned)B * (unsigned)m.units_per_frame; }
// byte offsets from the start of the region, for a handle whose mask takes mask_bytes and whose lists hold cap[] entries
inline size_t sparse_count_off(size_t mask_bytes) { return mask_bytes; }
inline size_t sparse_list_off(size_t mask_bytes, const unsigned cap[2], int stage) { return mask_bytes + 4 * (size_t)kSparseCounters + (stage ? 4 * (size_t)cap[0] : 0); }
inline size_t sparse_region_bytes(size_t mask_bytes, const unsigned cap[2]) { return sparse_list_off(mask_bytes, cap, 1) + 4 * (size_t)cap[1]; }
// stream pool (wtk_plan.hip)
int pooled_stream(int device, hipStream_t *s);
void unpool_stream(int device, hipStream_t s);
}
