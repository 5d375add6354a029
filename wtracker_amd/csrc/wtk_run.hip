// The detector handle, part 2 (see wtk_internal.h): one forward pass — letterbox / view cut, the fused front, the conv ops (one grouped split-K launch per
// dependency level on latency-plan handles), pool, head —, the predict entry points and the test hooks.
#include "wtk_internal.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>

using namespace wtk;

#ifdef WTK_WS64_STAMPS // diagnostic builds: per-wave interval stamps of the kernel under study (tools/gpu_sessions/ws64_stamps.py)
static unsigned long long *g_dbg_stamps = nullptr;
constexpr size_t kDbgStampBytes = 1 << 20;
extern "C" int wtk_debug_stamps(unsigned long long *host, size_t n_words) {
    if (!g_dbg_stamps || n_words * 8 > kDbgStampBytes) return 1;
    if (hipDeviceSynchronize() != hipSuccess) return 1;
    return hipMemcpy(host, g_dbg_stamps, n_words * 8, hipMemcpyDeviceToHost) == hipSuccess ? 0 : 1;
}
#endif

// ultralytics LetterBox geometry + scale_boxes inverse: the ONE place the letterbox kernels and the head get their numbers from.
// Forward (LetterBox): the reference scales by r = min(imgsz / H, imgsz / W) and pads the resized image up to the next stride multiple (auto=True), so a
// handle created at that shape (yolo_spec.letterbox_shape) has imgsz = max(Sh, Sw), and the short side of the resized image may be a product that was
// rounded DOWN onto Sh (435 x 579 at 384: 288.50 -> 288 rows, 384 columns; r taken from the handle's short side, 288 / 435, would give 383 columns).
// So r comes from S = max(Sh, Sw) whenever the resized image fits the handle, and from r = min(Sh / H, Sw / W) (pad to exactly Sh x Sw, auto=False)
// otherwise.  The two rules differ only where the short side binds and H * r rounds onto Sh, i.e. only on a letterbox_shape handle.
// Inverse (scale_boxes) recomputes gain and padding from the two shapes alone, in doubles; only the results are rounded to float.
static void letterbox_geom(int H, int W, int Sh, int Sw, int &new_h, int &new_w, int &top, int &left, float &gain, float &pad_x, float &pad_y) {
    const int S = std::max(Sh, Sw);
    double r = std::min((double)S / H, (double)S / W);
    new_w = (int)std::nearbyint(W * r);
    new_h = (int)std::nearbyint(H * r);
    if (new_h > Sh || new_w > Sw) {
        r = std::min((double)Sh / H, (double)Sw / W);
        new_w = (int)std::nearbyint(W * r);
        new_h = (int)std::nearbyint(H * r);
    }
    const double dw = (Sw - new_w) / 2.0, dh = (Sh - new_h) / 2.0;
    top = (int)std::nearbyint(dh - 0.1);
    left = (int)std::nearbyint(dw - 0.1);
    const double g = std::min((double)Sh / H, (double)Sw / W);
    gain = (float)g;
    pad_x = (float)std::nearbyint((Sw - W * g) / 2.0 - 0.1);
    pad_y = (float)std::nearbyint((Sh - H * g) / 2.0 - 0.1);
}

// outputs of the general NMS path (max_det >= 1 rows per image)
struct NmsOut {
    float iou;
    int max_det;
    int *out_cls, *out_count;
};
// the batch rows are camera views of full frames (wtk_yolo_predict_views) — crop + letterbox in one kernel
struct ViewSrc {
    const int32_t *pos_xy, *frame_index;
    int view_w, view_h, n_frames;
};

// A forward pass while it is enqueued: what the caller asked for, its lanes and, in profiling mode, the event brackets and counters of the kernel classes.
// Two lanes: the caller's stream runs backbone + PAN + the P5 tower; the P3 / P4 Detect towers run on the side streams as soon as their feature map is
// complete and fill the tails of the small PAN kernels.  Profiling keeps everything on one stream so the per-class event brackets stay meaningful.
struct Pass {
    wtk_yolo *h;
    const uint8_t *net_in; // the caller's frames; the network-size frames once enqueue_input has run
    int B, C;
    hipStream_t main_st;    // the caller's stream
    int32_t H, W;           // the image scale_boxes maps back to: the frames, or (enqueue_input) the views cut from them
    float conf, *out_xywh, *out_conf;
    int32_t *out_anchor;
    const ViewSrc *vs = nullptr;
    const NmsOut *nms = nullptr;
    bool two_lanes = false;
    unsigned side_used = 0; // bit i: side_stream[i] carries work of this pass
    const struct SparseBox *sparse = nullptr; // this pass leaves the box towers to enqueue_sparse_tail
    int cur_class = -1, nev = 0;
    int ev_class[wtk_yolo::kProfEvents];
    long long launches[wtk_yolo::kProfKernels] = {};
    double flops[wtk_yolo::kProfKernels] = {};
    double op_flops(const Op &o) const { return 2.0 * B * o.macs_per_image; } // algorithmic: 2 x output pixels x cout x (cin x k x k)
    void count(ProfClass cls, double fl = 0.0) { ++launches[cls], flops[cls] += fl; }
};

static HeadArgs head_args(const Pass &p) {
    wtk_yolo *h = p.h;
    const float conf = p.conf;
    HeadArgs a;
    std::memset(&a, 0, sizeof(a));
    for (int i = 0; i < 3; ++i) {
        a.box[i] = h->bufs[h->box_buf[i]].ptr;
        a.cls[i] = h->bufs[h->cls_buf[i]].ptr;
        a.lh[i] = h->lh[i];
        a.lw[i] = h->lw[i];
    }
    a.cls_ld = h->cls_ld;
    a.nc = h->dims.nc;
    a.N = p.B;
    a.conf = conf;
    int nh, nw, top, left;
    letterbox_geom(p.H, p.W, h->S_h, h->S_w, nh, nw, top, left, a.gain, a.pad_x, a.pad_y);
    a.img_w = (float)p.W, a.img_h = (float)p.H;
    a.out_xywh = p.out_xywh, a.out_conf = p.out_conf, a.out_anchor = p.out_anchor;
    a.out_margin = h->o_margin;
    a.status = h->status_dev;
    a.conf_logit = conf > 0.f && conf < 1.f ? std::log(conf / (1.f - conf)) : (conf <= 0.f ? -INFINITY : INFINITY);
    return a;
}
static int run_head(const Pass &p) { // (the test hooks behind the decode entry points: a pass that is nothing else)
    const HeadArgs a = head_args(p);
    if (const NmsOut *nms = p.nms) {
        const wtk_yolo *h = p.h;
        NmsArgs q;
        std::memset(&q, 0, sizeof(q));
        q.h = a;
        q.iou = nms->iou, q.max_det = nms->max_det;
        q.scratch_score = h->nms_score, q.scratch_cls = h->nms_cls, q.scratch_box = h->nms_box;
        q.out_xywh = a.out_xywh, q.out_conf = a.out_conf, q.out_anchor = a.out_anchor, q.out_cls = nms->out_cls, q.out_count = nms->out_count;
        HIP_TRY(launch_head_nms(q, p.main_st));
        return 0;
    }
    HIP_TRY(launch_head(a, p.main_st));
    return 0;
}

static int ensure_nms_scratch(wtk_yolo *h, hipStream_t st) {
    if (h->nms_score) return 0;
    HIP_TRY(hipStreamSynchronize(st));
    const size_t n = (size_t)h->max_batch * h->anchors;
    HIP_TRY(hipMalloc(&h->nms_score, n * sizeof(float)));
    HIP_TRY(hipMalloc(&h->nms_cls, n * sizeof(int)));
    HIP_TRY(hipMalloc(&h->nms_box, n * 4 * sizeof(float)));
    return 0;
}

// The pair of side streams is shared by every handle of the process on a device (ensure_side_streams).  Two host threads (ctypes releases the GIL)
// that enqueue on it at the same time would interleave their feature-event waits and tower launches on the shared pair.  Every enqueue that touches
// the pair holds this lock; a single-threaded caller (the bench, the controllers) never contends on it.
static std::mutex g_side_mu;

// side streams and their events, taken at the first forward pass that uses them
static int ensure_side_streams(wtk_yolo *h) {
    // ONE pair of side streams per process and device, shared by every handle and never destroyed.  The HIP runtime multiplexes streams onto its
    // hardware queues (four by default); with two lanes (two caller streams) a pair per handle made six streams, and which of them shared a queue
    // depended on the order in which streams had been created in the process: the same workload ran at 24.5 .. 27 k frames/s (fp16) or 14.8 .. 17.7 k
    // (hybrid) depending on what had run before it (tools/gpu_sessions/order_probe.py).  Two callers + one shared pair = four streams: every stream
    // has a queue of its own, and the rate no longer depends on the history of the process.  The towers of different handles then run one after the
    // other on a side stream; lanes are out of phase, nothing is lost (26.8 k / 17.6 k).
    for (int i = 1; i <= 2; ++i) {
        if (!h->side_stream[i]) {
            static std::mutex mu;
            static std::vector<std::pair<int, hipStream_t>> g_shared[2]; // per slot: (device, stream)
            std::lock_guard<std::mutex> lk(mu);
            for (auto &e : g_shared[i - 1])
                if (e.first == h->device) h->side_stream[i] = e.second;
            if (!h->side_stream[i]) {
                HIP_TRY(hipStreamCreateWithFlags(&h->side_stream[i], hipStreamNonBlocking));
                g_shared[i - 1].emplace_back(h->device, h->side_stream[i]);
            }
        }
        if (!h->side_done[i]) HIP_TRY(hipEventCreateWithFlags(&h->side_done[i], hipEventDisableTiming));
    }
    for (int i = 0; i < 2; ++i)
        if (!h->feat_ev[i]) HIP_TRY(hipEventCreateWithFlags(&h->feat_ev[i], hipEventDisableTiming));
    return 0;
}

// ---- resolve: what a conv op launches at batch B (ConvLaunch, wtk_internal.h).  Nothing here touches a stream or changes the handle. ----

// the conv of `op` as the implicit-GEMM / split-K launchers take it (split handles: pseudo-channel arguments)
static ConvArgs conv_args(const wtk_yolo *h, const Op &op, int B) {
    const Buf &ib = h->bufs[op.in_buf], &ob = h->bufs[op.out_buf];
    ConvArgs a;
    std::memset(&a, 0, sizeof(a));
    a.in = ib.ptr, a.in_ld = ib.C, a.in_coff = op.in_coff;
    a.N = B, a.H = ib.h, a.W = ib.w, a.Cin = op.cin;
    a.Ho = ob.h, a.Wo = ob.w, a.Cout = op.cout, a.CoutPad = op.cout_pad;
    a.KH = a.KW = op.k, a.stride = op.stride, a.pad = op.k / 2;
    a.w = op.w, a.bias = op.bias, a.zeros = h->zero_page, a.n_dyn = h->n_dyn;
    a.out = ob.ptr, a.out_ld = ob.C, a.out_coff = op.out_coff, a.out_f32 = ob.f32;
    if (op.out2_buf >= 0) a.out2 = h->bufs[op.out2_buf].ptr, a.out2_ld = h->bufs[op.out2_buf].C, a.out2_coff = op.out2_coff;
    if (op.in2_buf >= 0) a.in2 = h->bufs[op.in2_buf].ptr, a.in2_ld = h->bufs[op.in2_buf].C, a.in2_coff = op.in2_coff, a.in2_split = op.in2_split;
    if (op.res_buf >= 0) a.res = h->bufs[op.res_buf].ptr, a.res_ld = h->bufs[op.res_buf].C, a.res_coff = op.res_coff;
    a.act = op.act, a.K = op.K, a.Kpad = op.Kpad;
    a.M = (long long)B * ob.h * ob.w;
    a.tile_w = op.tile_w;
    if (op.tile_w) {
        const int th = conv_cfg_bm(op.cfg) / op.tile_w;
        a.tiles_x = (ob.w + op.tile_w - 1) / op.tile_w, a.tiles_y = (ob.h + th - 1) / th;
    }
    if (h->split) {
        // pseudo-channels: every channel count / offset of a split tensor doubles (an fp32 output keeps its real layout)
        a.in_ld *= 2, a.in_coff *= 2, a.Cin *= 2, a.K *= 2, a.Kpad *= 2;
        a.in2_ld *= 2, a.in2_coff *= 2, a.in2_split *= 2;
        a.res_ld *= 2, a.res_coff *= 2, a.out2_ld *= 2, a.out2_coff *= 2;
        if (!a.out_f32) a.out_ld *= 2, a.out_coff *= 2;
    }
    return a;
}

// ... as conv_sk_kernel takes it (the plan marks only convs that fit: anything else is an internal error)
static int sk_args(const wtk_yolo *h, const Op &op, int B, ConvArgs &a) {
    a = conv_args(h, op, B);
    a.tile_w = 0;
    if (!conv_sk_eligible(a, h->split)) return fail("internal: conv " + std::to_string(&op - h->ops.data()) + " of the latency plan does not fit conv_sk_kernel");
    return 0;
}

// ... and as the window kernels take it on an H x W map, strip geometry apart.  Tensor views, Cin and Kpad come from `a`: a split handle's pseudo-channels
// are doubled in conv_args alone.  A fused 1x1 tail rides along.
static HaloArgs halo_args(const wtk_yolo *h, const Op &op, const ConvArgs &a, int H, int W) {
    HaloArgs g;
    std::memset(&g, 0, sizeof(g));
    g.in = a.in, g.in_ld = a.in_ld, g.in_coff = a.in_coff;
    g.N = a.N, g.H = H, g.W = W, g.Cin = a.Cin;
    g.Cout = op.cout, g.CoutPad = op.cout_pad;
    g.w = op.w, g.bias = op.bias;
    g.out = a.out, g.out_ld = a.out_ld, g.out_coff = a.out_coff;
    g.out2 = a.out2, g.out2_ld = a.out2_ld, g.out2_coff = a.out2_coff;
    g.res = a.res, g.res_ld = a.res_ld, g.res_coff = a.res_coff;
    g.act = op.act, g.Kpad = a.Kpad;
    g.n_dyn = h->n_dyn, g.zeros = h->zero_page;
    if (op.tail_op >= 0) {
        const Op &t = h->ops[op.tail_op];
        g.tail_w = t.w, g.tail_bias = t.bias, g.tail_kpad = t.Kpad;
        g.tail_out = h->bufs[t.out_buf].ptr, g.tail_ld = h->bufs[t.out_buf].C, g.tail_coff = t.out_coff;
        g.tail_cout = t.cout, g.tail_f32 = h->bufs[t.out_buf].f32;
        if (h->split) { // pseudo-channels for the split weights (and for a split output; the fp32 head logits keep their real layout)
            g.tail_kpad *= 2;
            if (!g.tail_f32) g.tail_ld *= 2, g.tail_coff *= 2;
        }
    }
    return g;
}

// strided 3x3: the parity-plane window kernel; the geometry lives on the OUTPUT map (stacked images, one strip)
static HaloArgs s2win_args(const wtk_yolo *h, const Op &op, const ConvArgs &a) {
    HaloArgs g = halo_args(h, op, a, a.Ho, a.Wo);
    g.S = a.Wo, g.pitch = a.Wo + 1, g.strips = 1, g.bm = 256;
    g.blocks_per_strip = (int)(((long long)a.N * (a.Ho + 1) * g.pitch + 255) / 256);
    if (2LL * g.blocks_per_strip * (op.cout_pad / 128) <= h->num_cus) { // small maps: half-size blocks fill the chip
        g.bm = 128;
        g.blocks_per_strip = (int)(((long long)a.N * (a.Ho + 1) * g.pitch + 127) / 128);
    }
    return g;
}

static int halo_mode(const wtk_yolo *h) { return h->split ? HALO_SPLIT : h->is_f16 ? HALO_F16 : HALO_F32; }
// stride-1 3x3 on an LDS-resident window (op.halo 1: conv3x3_halo.hip, 2: conv3x3_c32.hip): the kernel of the family, its strip geometry and tile-shape knobs
static void resolve_window(const wtk_yolo *h, const Op &op, ConvLaunch &r) {
    const int B = r.a.N, H = r.a.H, W = r.a.W;
    HaloArgs &g = r.g;
    g = halo_args(h, op, r.a, H, W);
    g.slabs = h->split ? 3 : h->halo_slabs, g.persist_cus = h->halo_persist ? h->num_cus : 0;
    if (op.halo == 1 && h->use_ws64 && h->halo_slabs == 3 &&
        ws64_eligible(op.k, op.stride, op.cin, op.cout, op.cout_pad, h->is_f16, op.out2_buf >= 0, op.tail_op >= 0)) {
        halo_geometry_stacked(B, H, W, ws64_rows_max(), &g.S, &g.pitch, &g.strips, &g.blocks_per_strip);
        // worth it when every group of a persistent block gets at least two tiles (weights are staged once per block)
        if ((long long)g.strips * g.blocks_per_strip >= 4LL * h->num_cus) {
            r.kind = L_WS64; // g.bm stays 0 (the weave schedules of round 3 lost: the round-2 schedule)
            return;
        }
    }
    const int rows_max = (op.halo == 2 && h->split) ? c32_split_rows_max() : (op.halo == 2 || h->split) ? kHaloRowsMax : halo_rows_max(op.cout, h->halo_slabs);
    if (op.halo == 2) {
        halo_geometry(H, W, rows_max, &g.S, &g.pitch, &g.strips, &g.blocks_per_strip);
        r.kind = h->split ? L_C32_SPLIT : L_C32;
        return;
    }
    r.kind = h->split ? L_HALO_SPLIT : L_HALO;
    halo_geometry_stacked(B, H, W, rows_max, &g.S, &g.pitch, &g.strips, &g.blocks_per_strip);
    // the tiles of the launch as `g` stands, on the cout tile halo_variant names for it (no instantiation: no rule applies, and the launcher refuses `g`)
    HaloVariant v{};
    auto tiles = [&]() { return halo_variant(g, halo_mode(h), &v) ? (long long)g.strips * g.blocks_per_strip * (op.cout_pad / v.bn) : 1LL << 40; };
    // small maps: halve the blocks when 256-pixel blocks leave at least half of the CUs without work
    if ((h->halo_slabs == 3 || h->split) && h->halo_small_blocks && 2 * tiles() <= h->num_cus) {
        g.bm = 128;
        halo_geometry_stacked(B, H, W, rows_max, &g.S, &g.pitch, &g.strips, &g.blocks_per_strip, 128);
        // still under half of the CUs with 128-pixel blocks (a small handle's cycle batch on the 24 x 24 maps): 64-cout tiles as well —
        // each block then walks the same taps over half the couts
        if (h->small_narrow && h->split && op.tail_op < 0 && 2 * tiles() <= h->num_cus && v.bn > 64) g.narrow = 1;
    }
    // fp32 handles: the exact-fp32 matrix instructions make these layers arithmetic bound, so a grid on under three quarters of the CUs (a small
    // handle's 48 x 48 maps: 141-150 blocks of 128 / 192 couts) is cut into 64-cout tiles (Detect P3 first convs 205 us, class tower 139 us before)
    if (h->small_narrow && !h->split && op.tail_op < 0 && op.cout_pad % 64 == 0 && 4 * tiles() <= 3LL * h->num_cus && v.bn > 64) g.narrow = 1;
    // Small f16x3 handles: the 64-cout window tiles on the six-slab ring with fragment prefetch (conv3x3_halo.hip; bit-identical to the
    // three-slab kernel).  A cycle batch's 24 x 24 layers 19.4 -> 15.9 us each; the 256-pixel tiles and the large handles measure the
    // same either way (profiles/r05_notes.md section 7), so those keep the three-slab kernel.  WTK_HALO_DEEP: 0 off, 1 small handles
    // (default), 2 every handle; read when the handle is created.
    if (h->halo_deep) g.deep = 1;
}

// The kernel of one conv op at batch B, its profile class and its arguments: every eligibility test and every occupancy rule that needs the handle, in the order
// they apply (the window family's rules set knobs of HaloArgs — bm, narrow, deep, slabs, persist_cus —, which halo_variant turns into an instantiation).
static int resolve_conv(const wtk_yolo *h, const Op &op, int B, ConvLaunch &r) {
    const Buf &ib = h->bufs[op.in_buf], &ob = h->bufs[op.out_buf];
    r.cls = op.sk ? PROF_IGEMM : (op.halo == 2 ? PROF_C32 : (op.halo ? PROF_HALO : PROF_IGEMM));
    r.cfg = op.cfg, r.kind = L_IGEMM;
    if (op.sk) {
        r.kind = L_SK;
        return sk_args(h, op, B, r.a);
    }
    ConvArgs &a = r.a;
    a = conv_args(h, op, B);
    const bool plain = op.res_buf < 0 && op.out2_buf < 0 && op.in2_buf < 0, halves = ib.h == 2 * ob.h && ib.w == 2 * ob.w;
    if (h->split && !op.halo && h->use_s2win && halves && split_s2win_eligible(op.k, op.stride, op.cin, op.cout, op.cout_pad, ob.w, plain && !ob.f32)) {
        r.kind = L_S2WIN_SPLIT; // split operands: the parity-plane window kernel on pseudo-channels
        r.g = s2win_args(h, op, a);
    } else if (h->split && !op.halo) {
        r.kind = L_IGEMM_SPLIT;
        // a small handle's 128 x 128-tile layer whose grid leaves a third of the CUs idle: 64-cout tiles, twice the blocks (same K order: same bits)
        if (h->small_narrow && r.cfg == CFG_128x128 && !a.in2 && !a.tile_w && 3 * ((a.M + 127) / 128) * (a.CoutPad / 128) <= 2LL * h->num_cus) r.cfg = CFG_128x64;
    } else if (op.halo) {
        resolve_window(h, op, r);
    } else if (h->use_s2win && op.tail_op < 0 && s2win_eligible(op.k, op.stride, op.cin, op.cout, op.cout_pad, h->is_f16, ob.w, plain) && halves) {
        r.kind = L_S2WIN;
        r.g = s2win_args(h, op, a);
    } else if (op.tail_op >= 0) { // implicit GEMM with the 1x1 behind it fused into its epilogue
        const Op &t = h->ops[op.tail_op];
        a.tail_w = t.w, a.tail_bias = t.bias, a.tail_kpad = t.Kpad, a.tail_act = t.act;
        a.tail_out = h->bufs[t.out_buf].ptr, a.tail_ld = h->bufs[t.out_buf].C, a.tail_coff = t.out_coff;
    } else if (h->use_wide && conv1x1_wide_eligible(a, h->is_f16) && a.CoutPad >= 256 && ((a.M + 255) / 256) * (a.CoutPad / 128) >= 384) {
        r.kind = L_WIDE_1X1;
    }
    return 0;
}

// ---- sparse Detect box towers (DESIGN.md "Sparse box towers") ----
// A max_det = 1 call reads the 64 box logits of ONE anchor per frame, so the box towers (model.22.cv2.*) only matter on the 5 x 5 patch under the survivor.
// What a sparse call launches in place of a level's tower ops: cls0 = the class half (couts hb .. hb + hc) of the shared first conv, in the tower's place on its
// lane; behind the head's selection box0 = its box half (couts 0 .. hb) and box1 = box.1 with box.2 in its epilogue, both with the live mask.  All three run on
// the packed weights, the geometry and the 64-cout tile of the dense launches, so every pixel they compute has the dense pass's bits.
struct SparseBox {
    ConvLaunch cls0[3], box0[3], box1[3];
    HeadSparseArgs hs; // geometry and mask layout for the head kernels (hs.h is filled per call)
    unsigned list_grid[2]; // list form: the host's bound of the live tiles of this call per stage = the grid of its launch
    int level_of_op0(const wtk_yolo *h, size_t oi) const {
        for (int l = 0; l < 3; ++l)
            if ((int)oi == h->det[l].op0) return l;
        return -1;
    }
    bool skips(const wtk_yolo *h, size_t oi) const {
        for (int l = 0; l < 3; ++l)
            if ((int)oi == h->det[l].box1 || (int)oi == h->det[l].box2) return true;
        return false;
    }
};

// The rule, in one place.  A call goes sparse iff it is a max_det = 1 call (the caller checks), the switch WTK_NO_SPARSE_BOX is not set, the call is large
// enough for the sparse tail to pay (sparse_box_pays, wtk_internal.h: 3.2 rounds of P3 blocks, from measurement), the handle is a
// throughput-plan f16x3 handle (wtk_plan.hip allocates the mask for those alone: fp16 / fp32 run the shared first conv as ONE 192-cout tile, whose halves would
// be other instantiations; latency-plan handles run the box-tower convs as members of grouped split-K launches shared with the PAN path, and five more
// dependent levels would cost a single frame more than the skipped tiles save), and EVERY box op of every level resolves, at this batch size, to the window
// kernel that takes the mask: the shared conv unfused on conv3x3_halo_kernel<split>, box.1 on it with box.2 as its fused tail.  Anything else (a small handle
// whose 12 x 12 maps run split-K, WTK_NO_FUSED_TAIL, WTK_NO_HALO) keeps the whole handle dense.
static bool resolve_sparse(const wtk_yolo *h, int B, SparseBox &sp) {
    if (!h->use_sparse_box || !h->split || h->latency || !h->live_bytes) return false;
    if (!sparse_box_pays(B, h->lh[0], h->lw[0], h->num_cus, h->sparse_min_tenths)) return false; // a call too small for the sparse tail to pay (wtk_internal.h)
    std::memset(&sp.hs, 0, sizeof(sp.hs));
    SparseMask m; // this call's mask arrays inside the region that wtk_plan.hip sized for max_batch (wtk_internal.h)
    for (int l = 0; l < 3; ++l) {
        const wtk_yolo::DetLevel &d = h->det[l];
        if (d.op0 < 0 || d.box1 < 0 || d.box2 < 0) return false;
        const Op &o0 = h->ops[d.op0], &b1 = h->ops[d.box1], &b2 = h->ops[d.box2];
        if (o0.folded || o0.tail_op >= 0 || o0.cout != h->dims.hb + h->dims.hc || h->dims.hb != 64 || h->dims.hc % 64 || b1.tail_op != d.box2 || !b2.folded) return false;
        ConvLaunch r0, r1;
        if (resolve_conv(h, o0, B, r0) || resolve_conv(h, b1, B, r1)) return false;
        if (r0.kind != L_HALO_SPLIT || r1.kind != L_HALO_SPLIT || r0.g.res || r0.g.out2 || r1.g.res || r1.g.out2) return false;
        HaloVariant v0, v1; // the dense launches must already run on the list kernel's cout tile, by their layers' own width (not cut into it for a thin grid)
        if (!halo_variant(r0.g, HALO_SPLIT, &v0) || !halo_variant(r1.g, HALO_SPLIT, &v1) || v0.bn != kHaloListVariant.bn || v1.bn != kHaloListVariant.bn || r0.g.narrow || r1.g.narrow) return false;
        if (r0.g.S != r1.g.S || r0.g.pitch != r1.g.pitch || r0.g.strips != r1.g.strips) return false;
        sparse_mask_add_level(m, l, B, h->lh[l], r0.g.pitch, r0.g.strips);
        if (m.bytes > h->live_mask_bytes) return false;
        sp.hs.S[l] = r0.g.S, sp.hs.pitch[l] = r0.g.pitch, sp.hs.ld[l] = m.ld[l];
        sp.hs.off0[l] = m.off0[l], sp.hs.off1[l] = m.off1[l];
        // the two halves of the shared conv: rows [0, hb) and [hb, hb + hc) of its packed weights and bias, the same slices of d1.  64-cout tiles either way
        // (narrow: the class half's 128 couts would otherwise pick the 128-cout tile)
        const int hb = h->dims.hb;
        sp.box0[l] = r0;
        sp.box0[l].g.Cout = sp.box0[l].g.CoutPad = hb;
        sp.box0[l].g.live_off = kZeroPageBytes + m.off0[l], sp.box0[l].g.live_ld = m.ld[l];
        sp.cls0[l] = r0;
        HaloArgs &c = sp.cls0[l].g;
        c.Cout = c.CoutPad = o0.cout - hb, c.narrow = 1;
        c.w = reinterpret_cast<const char *>(c.w) + (size_t)hb * c.Kpad * 2; // split rows: Kpad pseudo-channels of fp16
        c.bias = c.bias + hb;
        c.out_coff += 2 * hb; // pseudo-channels
        sp.box1[l] = r1;
        sp.box1[l].g.live_off = kZeroPageBytes + m.off1[l], sp.box1[l].g.live_ld = m.ld[l];
    }
    sp.hs.live = reinterpret_cast<unsigned char *>(h->zero_page) + kZeroPageBytes;
    sp.hs.sel_anchor = h->sel_anchor, sp.hs.sel_score = h->sel_score, sp.hs.n_dyn = h->n_dyn;
    sp.list_grid[0] = sp.list_grid[1] = 0;
    if (h->use_sparse_list) { // counters and lists behind the handle's mask; a call lists at most B * units_per_frame tiles for box.0 and B for box.1 + box.2
        for (int s = 0; s < 2; ++s) sp.list_grid[s] = sparse_list_cap(m, s, B);
        if (sp.list_grid[0] > h->live_list_cap[0] || sp.list_grid[1] > h->live_list_cap[1]) return false;
        sp.hs.count = reinterpret_cast<unsigned *>(sp.hs.live + sparse_count_off(h->live_mask_bytes));
        for (int s = 0; s < 2; ++s) sp.hs.list[s] = reinterpret_cast<unsigned *>(sp.hs.live + sparse_list_off(h->live_mask_bytes, h->live_list_cap, s));
        sp.hs.cap[0] = sp.list_grid[0], sp.hs.cap[1] = sp.list_grid[1];
    }
    return true;
}

// key of a launch's cached choice (sk_choices, sk_cands, tune_ms, tune_key): a dependency level of lat_sched, or kOpKeyBase + the index of an op launched alone
constexpr long long kOpKeyBase = 100000;
static long long choice_key(long long launch, int B) { return (launch << 24) | (long long)B; }

// ---- issue: the resolved launch on stream `st`.  Nothing is decided here. ----
static int issue_conv(wtk_yolo *h, const Op &op, const ConvLaunch &r, hipStream_t st) {
    switch (r.kind) {
    case L_IGEMM: HIP_TRY(launch_conv(r.a, r.cfg, h->is_f16, st)); break;
    case L_IGEMM_SPLIT: HIP_TRY(launch_conv_split(r.a, r.cfg, st)); break;
    case L_WIDE_1X1: HIP_TRY(launch_conv1x1_wide(r.a, st)); break;
    case L_HALO: HIP_TRY(launch_conv3x3_halo(r.g, h->is_f16, st)); break;
    case L_HALO_SPLIT: HIP_TRY(launch_conv3x3_halo_split(r.g, st)); break;
    case L_C32: HIP_TRY(launch_conv3x3_c32(r.g, st)); break;
    case L_C32_SPLIT: HIP_TRY(launch_conv3x3_c32_split(r.g, st)); break;
    case L_S2WIN: HIP_TRY(launch_conv3x3_s2(r.g, st)); break;
    case L_S2WIN_SPLIT: HIP_TRY(launch_conv3x3_s2_split(r.g, st)); break;
    case L_WS64:
#ifdef WTK_WS64_STAMPS
        if (std::getenv("WTK_WS64_STAMPS")) {
            if (!g_dbg_stamps) HIP_TRY(hipMalloc(&g_dbg_stamps, kDbgStampBytes));
            HaloArgs g = r.g;
            g.dbg_stamps = g_dbg_stamps;
            HIP_TRY(launch_conv3x3_ws64(g, h->num_cus, st));
            break;
        }
#endif
        HIP_TRY(launch_conv3x3_ws64(r.g, h->num_cus, st));
        break;
    case L_SK: {
        const SkMember one{r.a, op.sk_atoms, op.sk_partial, op.sk_tickets};
        HIP_TRY(launch_conv_sk_group(&one, 1, h->split, h->num_cus, h->sk_force_tile, h->sk_force_form, st, &h->sk_choices[choice_key(kOpKeyBase + (&op - h->ops.data()), r.a.N)]));
        break;
    }
    }
    return 0;
}

// profiling: the launches that follow belong to class `cls` (a new event bracket when the class changes)
static int mark(Pass &p, ProfClass cls) {
    if (!p.h->profiling || cls == p.cur_class || p.nev >= wtk_yolo::kProfEvents - 1) return 0;
    HIP_TRY(hipEventRecord(p.h->ev[p.nev], p.main_st));
    p.ev_class[p.nev++] = p.cur_class = cls;
    return 0;
}

// letterbox (or view crop + letterbox) into the staging image when the frames are not network-size already; H x W becomes the image scale_boxes maps back to
static int enqueue_input(Pass &p) {
    wtk_yolo *h = p.h;
    const ViewSrc *vs = p.vs;
    int32_t &H = p.H, &W = p.W;
    float g, px, py;
    if (vs) {
        ViewLetterboxArgs va;
        std::memset(&va, 0, sizeof(va));
        va.frames = p.net_in, va.frame_index = vs->frame_index, va.pos_xy = vs->pos_xy, va.dst = h->lb_dev;
        va.N = p.B, va.H = H, va.W = W, va.C = p.C, va.F = vs->n_frames;
        va.view_w = vs->view_w, va.view_h = vs->view_h, va.Sh = h->S_h, va.Sw = h->S_w;
        va.rows = vs->view_w, va.cols = vs->view_h; // frame[y : y + w, x : x + h], view_controller.py:171
        letterbox_geom(va.rows, va.cols, h->S_h, h->S_w, va.new_h, va.new_w, va.top, va.left, g, px, py);
        HIP_TRY(launch_view_letterbox(va, p.main_st));
        p.net_in = h->lb_dev;
        H = va.rows, W = va.cols; // from here on the "image" is the view: scale_boxes maps back to view pixels
    } else if (H != h->S_h || W != h->S_w) {
        LetterboxArgs la;
        std::memset(&la, 0, sizeof(la));
        la.src = p.net_in, la.dst = h->lb_dev;
        la.N = p.B, la.H = H, la.W = W, la.C = p.C, la.Sh = h->S_h, la.Sw = h->S_w;
        letterbox_geom(H, W, h->S_h, h->S_w, la.new_h, la.new_w, la.top, la.left, g, px, py);
        HIP_TRY(launch_letterbox(la, p.main_st));
        p.net_in = h->lb_dev;
    }
    return 0;
}

// ops[0..2] (stem, model.1, model.2.cv1) as ONE fused kernel
static int enqueue_front(Pass &p) {
    wtk_yolo *h = p.h;
    if (mark(p, PROF_FUSED)) return 1;
    const Op &o0 = h->ops[0], &o1 = h->ops[1], &o2 = h->ops[2];
    FrontArgs f;
    std::memset(&f, 0, sizeof(f));
    f.frames = p.net_in, f.N = p.B, f.H = h->S_h, f.W = h->S_w, f.C = p.C;
    f.w0 = o0.w, f.b0 = o0.bias;
    f.w1 = o1.w, f.b1 = o1.bias, f.Kpad1 = o1.Kpad;
    f.w2 = o2.w, f.b2 = o2.bias, f.Kpad2 = o2.Kpad;
    f.out = h->bufs[o2.out_buf].ptr, f.out_ld = h->bufs[o2.out_buf].C, f.out_coff = o2.out_coff;
    if (h->front_debug) f.dbg_t0 = h->bufs[o0.out_buf].ptr, f.dbg_t1 = h->bufs[o1.out_buf].ptr;
    if (h->split) { // pseudo-channels (see conv_args)
        f.Kpad1 *= 2, f.Kpad2 *= 2, f.out_ld *= 2, f.out_coff *= 2;
        f.n_dyn = h->n_dyn, f.stem_split = 1;
        HIP_TRY(launch_front_fused_split(f, h->num_cus, p.main_st));
    } else
        HIP_TRY(launch_front_fused(f, h->num_cus, p.main_st));
    p.count(PROF_FUSED, p.op_flops(o0) + p.op_flops(o1) + p.op_flops(o2));
    return 0;
}

// ops[3..5] (model.2.m.0.cv1, m.0.cv2, model.2.cv2) as ONE fused kernel, launched at op 5
static int enqueue_c2f(Pass &p, const Op &op) {
    wtk_yolo *h = p.h;
    if (mark(p, PROF_FUSED)) return 1;
    const Op &m1 = h->ops[3], &m2 = h->ops[4];
    const Buf &cb = h->bufs[op.in_buf];
    C2fArgs c;
    std::memset(&c, 0, sizeof(c));
    c.cat = cb.ptr, c.cat_ld = cb.C, c.a_coff = op.in_coff, c.b_coff = m1.in_coff;
    c.N = p.B, c.H = cb.h, c.W = cb.w, c.zeros = h->zero_page;
    c.w_m1 = m1.w, c.b_m1 = m1.bias, c.w_m2 = m2.w, c.b_m2 = m2.bias, c.Kpad_m = m1.Kpad;
    c.w_cv2 = op.w, c.b_cv2 = op.bias, c.Kpad_cv2 = op.Kpad;
    c.out = h->bufs[op.out_buf].ptr, c.out_ld = h->bufs[op.out_buf].C, c.out_coff = op.out_coff;
    HIP_TRY(launch_c2f_fused(c, h->num_cus, p.main_st));
    p.count(PROF_FUSED, p.op_flops(m1) + p.op_flops(m2) + p.op_flops(op));
    return 0;
}

// one op of the plan in its own launch, on its lane
static int enqueue_op(Pass &p, size_t oi) {
    wtk_yolo *h = p.h;
    const Op &op = h->ops[oi];
    if (h->use_c2f && (oi == 3 || oi == 4)) return 0; // folded into the fused C2f tail launched at op 5
    if (op.folded) return 0;                          // runs in the epilogue of the op that names it as tail_op
    if (h->use_c2f && oi == 5) return enqueue_c2f(p, op);
    if (p.sparse && p.sparse->skips(h, oi)) return 0; // box.1 / box.2 of a sparse pass: behind the head's selection
    hipStream_t st = p.main_st;
    if (p.two_lanes && op.side) { // a Detect tower: on its side stream, behind its feature map
        const int sidx = std::min(op.side, h->side_streams); // wtk_yolo_set_side_streams(1): both towers on side stream 1
        st = h->side_stream[sidx];
        if (op.wait_feat >= 0) HIP_TRY(hipStreamWaitEvent(st, h->feat_ev[op.wait_feat], 0));
        p.side_used |= 1u << sidx;
    }
    if (op.kind == OP_STEM) {
        if (mark(p, PROF_STEM)) return 1;
        StemArgs a;
        std::memset(&a, 0, sizeof(a));
        a.frames = p.net_in, a.N = p.B, a.H = h->S_h, a.W = h->S_w, a.C = p.C;
        a.w = op.w, a.bias = op.bias, a.out = h->bufs[op.out_buf].ptr;
        a.Cout = op.cout, a.Ho = h->S_h / 2, a.Wo = h->S_w / 2;
        a.out_split = a.in_split = h->split; // split store, split operands
        a.n_dyn = h->n_dyn;
        HIP_TRY(launch_stem(a, h->is_f16, st));
        p.count(PROF_STEM, p.op_flops(op));
        return 0;
    }
    if (op.kind == OP_POOL) {
        if (mark(p, PROF_POOL)) return 1;
        const Buf &b = h->bufs[op.in_buf];
        PoolArgs a;
        std::memset(&a, 0, sizeof(a));
        a.buf = b.ptr, a.N = p.B, a.H = b.h, a.W = b.w, a.c = op.cin, a.split = h->split;
        HIP_TRY(launch_sppf_pool(a, h->is_f16, st));
        p.count(PROF_POOL);
        return 0;
    }
    if (const int l = p.sparse ? p.sparse->level_of_op0(h, oi) : -1; l >= 0) { // the shared first conv of a tower pair: its class half, in its place
        const ConvLaunch &c = p.sparse->cls0[l];
        if (mark(p, c.cls) || issue_conv(h, op, c, st)) return 1;
        p.count(c.cls, p.op_flops(op) * h->dims.hc / (h->dims.hb + h->dims.hc));
        return 0;
    }
    ConvLaunch r;
    if (resolve_conv(h, op, p.B, r) || mark(p, r.cls) || issue_conv(h, op, r, st)) return 1;
    p.count(r.cls, p.op_flops(op) + (op.tail_op >= 0 ? p.op_flops(h->ops[op.tail_op]) : 0.0));
    if (p.two_lanes && op.signal_feat >= 0) HIP_TRY(hipEventRecord(h->feat_ev[op.signal_feat], p.main_st));
    return 0;
}

// Latency-plan handles (round 6): everything on the caller's stream, the independent convs of a dependency level (sk_schedule) grouped into ONE launch; ops[0 .. 2]
// (the front, when it did not run fused) first.  In a timing pass of sk_autotune (tune_pass >= 0) a grouped launch runs as its candidate number, between two events.
static int enqueue_levels(Pass &p, size_t first_op) {
    wtk_yolo *h = p.h;
    for (size_t oi = first_op; oi < 3 && oi < h->ops.size(); ++oi)
        if (enqueue_op(p, oi)) return 1;
    for (size_t li = 0; li < h->lat_sched.size(); ++li) {
        const std::vector<int> &L = h->lat_sched[li];
        if (!(h->ops[L[0]].kind == OP_CONV && h->ops[L[0]].sk)) { // (the pool, or a conv that does not fit the split-K kernel: one op, its own launch)
            if (enqueue_op(p, (size_t)L[0])) return 1;
            continue;
        }
        if (mark(p, PROF_IGEMM)) return 1;
        SkMember m[kSkGroupMax];
        const int n = (int)L.size();
        for (int k = 0; k < n; ++k) {
            const Op &op = h->ops[L[k]];
            m[k] = SkMember{ConvArgs(), op.sk_atoms, op.sk_partial, op.sk_tickets};
            if (sk_args(h, op, p.B, m[k].a)) return 1;
            p.flops[PROF_IGEMM] += p.op_flops(op);
        }
        const long long key = choice_key((long long)li, p.B);
        SkChoice *choice = &h->sk_choices[key], cand;
        hipEvent_t *ev = h->tune_pass >= 0 ? &h->tune_ev[2 * li] : nullptr;
        if (ev) {
            std::vector<SkChoice> &cands = h->sk_cands[key];
            if (cands.empty()) {
                cands.resize(kSkMaxCandidates);
                cands.resize((size_t)std::max(conv_sk_enumerate(m, n, h->split, h->num_cus, h->sk_force_tile, h->sk_force_form, cands.data(), kSkMaxCandidates), 0));
                if (cands.empty()) return fail("internal: no launch candidate for level " + std::to_string(li));
                h->tune_ms[key].assign(cands.size(), 1e30f);
            }
            cand = cands[(size_t)h->tune_pass % cands.size()];
            choice = &cand;
            HIP_TRY(hipEventRecord(ev[0], p.main_st));
        }
        HIP_TRY(launch_conv_sk_group(m, n, h->split, h->num_cus, h->sk_force_tile, h->sk_force_form, p.main_st, choice));
        if (ev) {
            HIP_TRY(hipEventRecord(ev[1], p.main_st));
            h->tune_key[li] = key;
        }
        p.count(PROF_IGEMM);
    }
    return 0;
}

// The end of a sparse pass, on the caller's stream behind the joined side streams: select (which marks the live units and lists their tiles), box.0 of the three
// levels in one launch from the list, box.1 + box.2 likewise, decode (which also leaves mask and counters zero for the next call): four dependent launches whose
// window grids are the host's bound of the live tiles.  The masked form (WTK_SPARSE_LIST=0) clears the mask, selects, and runs the six window launches of the
// levels as full grids whose blocks look their units up in the mask.  In profiling mode the window launches are a class of their own with 0 FLOPs (the host does
// not know the live tiles), so the roofline does not credit the window kernel with work it skipped.
static int enqueue_sparse_tail(Pass &p) {
    wtk_yolo *h = p.h;
    const SparseBox &sp = *p.sparse;
    hipStream_t st = p.main_st;
    HeadSparseArgs hs = sp.hs;
    hs.h = head_args(p);
    if (mark(p, PROF_HEAD)) return 1;
    if (!hs.list[0]) HIP_TRY(hipMemsetAsync(hs.live, 0, h->live_mask_bytes, st));
    HIP_TRY(launch_head_select_sparse(hs, st));
    p.count(PROF_HEAD);
    if (mark(p, PROF_SPARSE)) return 1;
    if (hs.list[0]) {
        for (int stage = 0; stage < 2; ++stage) {
            HaloListArgs g;
            for (int l = 0; l < 3; ++l) g.m[l] = (stage ? sp.box1 : sp.box0)[l].g;
            g.list = hs.list[stage], g.count = hs.count + stage;
            HIP_TRY(launch_conv3x3_halo_list(g, sp.list_grid[stage], st));
            for (int l = 0; l < 3; ++l) p.count(PROF_SPARSE); // the class counts box-tower convs run sparse, as the masked form's six launches do: one launch, three convs
        }
    } else {
        for (int l = 0; l < 3; ++l) {
            if (issue_conv(h, h->ops[h->det[l].op0], sp.box0[l], st)) return 1;
            p.count(PROF_SPARSE);
        }
        for (int l = 0; l < 3; ++l) {
            if (issue_conv(h, h->ops[h->det[l].box1], sp.box1[l], st)) return 1;
            p.count(PROF_SPARSE);
        }
    }
    if (mark(p, PROF_HEAD)) return 1;
    HIP_TRY(launch_head_decode(hs, st));
    p.count(PROF_HEAD);
    h->sparse_B = p.B;
    h->sparse_grid[0] = sp.list_grid[0], h->sparse_grid[1] = sp.list_grid[1];
    for (int l = 0; l < 3; ++l) { // what complete_box_towers launches: this pass's own box launches, without the mask
        h->sparse_done[l] = sp.box0[l], h->sparse_done[3 + l] = sp.box1[l];
        h->sparse_done[l].g.live_off = h->sparse_done[3 + l].g.live_off = 0;
        h->sparse_done[l].g.live_ld = h->sparse_done[3 + l].g.live_ld = 0;
    }
    return 0;
}

// Dense on demand: the test hooks that read box-tower tensors (wtk_yolo_debug_head, wtk_yolo_debug_tensor) first run what the last sparse pass skipped — the
// box ops of its batch size without a mask.  Their inputs (the neck maps, d1's class half) are buffers of their own and still hold that pass's values, and the
// dense launches compute every pixel with the bits the sparse ones gave the survivors'.  The device is idle when this is called.
static int complete_box_towers(wtk_yolo *h) {
    if (!h->sparse_B) return 0;
    for (int l = 0; l < 3; ++l)
        if (issue_conv(h, h->ops[h->det[l].op0], h->sparse_done[l], nullptr)) return 1;
    for (int l = 0; l < 3; ++l)
        if (issue_conv(h, h->ops[h->det[l].box1], h->sparse_done[3 + l], nullptr)) return 1;
    HIP_TRY(hipDeviceSynchronize());
    h->sparse_B = 0;
    return 0;
}

// The same for the first C2f's bottleneck output z on a handle that runs model.2.cv2 inside model.2.m.0.cv2's kernel (wtk_plan.hip: fuse_c2f_split_tail):
// the forward pass never stores z, so the test hook that reads it first runs the unfused launch at its batch size.  Its inputs (m.0.cv1's output, y1 in
// the concat buffer) still hold the last pass's values, and the plain kernel forms z with the fused kernel's arithmetic.  The device is idle when this is called.
static int complete_c2f_z(wtk_yolo *h, int B) {
    Op m2 = h->ops[h->c2f_tail_op];
    m2.tail_op = -1;
    ConvLaunch r;
    if (resolve_conv(h, m2, B, r) || issue_conv(h, m2, r, nullptr)) return 1;
    HIP_TRY(hipDeviceSynchronize());
    return 0;
}

// Enqueue one forward pass on `st`: input (letterbox / view) -> front -> ops or dependency levels -> join the side streams -> head -> profile read-out.
// No allocation, no synchronisation (profiling mode excepted): safe inside a caller's stream capture.  A pass that is being CAPTURED stays dense: the handle
// remembers on the host whether its last pass left the box towers sparse (sparse_B, for the debug entry points), and a captured pass runs when its graph is
// replayed, not when it is enqueued — the host could not know which kind of pass ran last.
static int yolo_enqueue_pass(Pass p) { // a fresh pass (the caller's frames, batch, stream and request), by value: this function's to fill
    wtk_yolo *h = p.h;
    hipStream_t st = p.main_st;
    SparseBox sp;
    if (!p.nms && resolve_sparse(h, p.B, sp)) { // max_det = 1: the box towers only where the survivors need them
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone) p.sparse = &sp;
    }
    if (enqueue_input(p)) return 1;
    const bool grouped = h->latency && h->sk_group && !h->lat_sched.empty();
    if (!grouped && h->use_side && h->side_streams > 0 && !h->profiling && ensure_side_streams(h)) return 1;
    p.two_lanes = !grouped && h->use_side && h->side_streams > 0 && h->side_stream[1] && !h->profiling;
    std::unique_lock<std::mutex> side_lock;
    if (p.two_lanes) side_lock = std::unique_lock<std::mutex>(g_side_mu);
    const bool front = h->use_front && reinterpret_cast<uintptr_t>(p.net_in) % 4 == 0;
    if (front && enqueue_front(p)) return 1;
    const size_t first_op = front ? 3 : 0;
    if (grouped && enqueue_levels(p, first_op)) return 1;
    for (size_t oi = first_op; !grouped && oi < h->ops.size(); ++oi)
        if (enqueue_op(p, oi)) return 1;
    for (int i = 1; i < wtk_yolo::kSideStreams; ++i)
        if (p.side_used & (1u << i)) {
            HIP_TRY(hipEventRecord(h->side_done[i], h->side_stream[i]));
            HIP_TRY(hipStreamWaitEvent(st, h->side_done[i], 0));
        }
    if (p.sparse) {
        if (enqueue_sparse_tail(p)) return 1;
    } else {
        h->sparse_B = 0; // a dense pass computes every box logit
        if (mark(p, PROF_HEAD)) return 1;
        if (run_head(p)) return 1;
        p.count(PROF_HEAD);
    }
    if (!h->profiling) return 0;
    if (p.nev < wtk_yolo::kProfEvents) { // close the last bracket
        HIP_TRY(hipEventRecord(h->ev[p.nev], st));
        p.ev_class[p.nev++] = -1;
    }
    HIP_TRY(hipEventSynchronize(h->ev[p.nev - 1]));
    for (int i = 0; i + 1 < p.nev; ++i) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, h->ev[i], h->ev[i + 1]));
        h->prof_ms[p.ev_class[i]] += ms;
    }
    for (int i = 0; i < wtk_yolo::kProfKernels; ++i) h->prof_launches[i] += p.launches[i], h->prof_flops[i] += p.flops[i];
    return 0;
}

// Autotune of a latency-plan handle: the first EAGER forward pass at a batch size is preceded by timing passes — the same forward pass (real frames, real
// activations), every grouped launch between two events, launch i running its candidate number (pass mod candidates_i) — and every launch keeps the
// (tile, forms) that took the least time.  The cost model that otherwise decides is calibrated on a few layers of one network at one size; the choice
// enters no arithmetic (tests/test_gpu_latency.py: every tile and form gives the same bits), so timing noise can cost microseconds, never results.
static int sk_autotune(const Pass &p) {
    wtk_yolo *h = p.h;
    hipStream_t st = p.main_st;
    const size_t n = h->lat_sched.size();
    while (h->tune_ev.size() < 2 * n) {
        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e));
        h->tune_ev.push_back(e);
    }
    h->tune_key.assign(n, -1);
    constexpr int kReps = 3;
    size_t most = 1;
    int rc = 0;
    for (size_t pass = 0; pass < most * kReps && !rc; ++pass) {
        h->tune_pass = (int)pass;
        rc = yolo_enqueue_pass(p);
        h->tune_pass = -1;
        if (rc) break;
        if (hipStreamSynchronize(st) != hipSuccess) {
            rc = fail("sk_autotune: hipStreamSynchronize failed");
            break;
        }
        for (size_t li = 0; li < n; ++li) {
            const long long key = h->tune_key[li];
            if (key < 0) continue;
            const std::vector<SkChoice> &cands = h->sk_cands[key];
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, h->tune_ev[2 * li], h->tune_ev[2 * li + 1]) != hipSuccess) continue;
            float &best = h->tune_ms[key][pass % cands.size()];
            best = std::min(best, ms);
            most = std::max(most, cands.size());
        }
    }
    if (rc) return rc;
    for (size_t li = 0; li < n; ++li) {
        const long long key = h->tune_key[li];
        if (key < 0) continue;
        const std::vector<SkChoice> &cands = h->sk_cands[key];
        const std::vector<float> &ms = h->tune_ms[key];
        size_t b = 0;
        for (size_t i = 1; i < cands.size(); ++i)
            if (ms[i] < ms[b] * 0.97f) b = i; // (the model's choice unless another is clearly faster)
        h->sk_choices[key] = cands[b];
    }
    h->sk_tuned.push_back(p.B);
    return 0;
}

static int yolo_enqueue(const Pass &p) {
    wtk_yolo *h = p.h;
    if (h->latency && h->sk_group && h->sk_autotune && !h->lat_sched.empty() && !h->profiling && h->tune_pass < 0 &&
        std::find(h->sk_tuned.begin(), h->sk_tuned.end(), p.B) == h->sk_tuned.end()) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(p.main_st, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone) { // (a capture cannot be timed: it keeps the cost model's choices)
            if (sk_autotune(p)) return 1;
        }
    }
    return yolo_enqueue_pass(p);
}

// staging image of the network input (letterbox / view), allocated once
static int ensure_staging(wtk_yolo *h, hipStream_t st) {
    if (h->lb_cap) return 0;
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipMalloc(&h->lb_dev, (size_t)h->max_batch * h->S_h * h->S_w * 3));
    h->lb_cap = (size_t)h->max_batch * h->S_h * h->S_w * 3;
    return 0;
}

extern "C" int wtk_yolo_predict(wtk_yolo *h, const uint8_t *frames_dev, int32_t B, int32_t H, int32_t W, int32_t C, float conf, float iou,
                                int32_t max_det, float *out_xywh, float *out_conf, int32_t *out_anchor, void *stream) {
    (void)iou; // with max_det == 1 the IoU threshold cannot change the survivor
    if (!h || !frames_dev || !out_xywh) return fail("wtk_yolo_predict: null argument");
    if (B <= 0) return fail("wtk_yolo_predict: empty batch (the reference asserts len(frames) > 0, yolo_controller.py:65)");
    if (B > h->max_batch) return fail("wtk_yolo_predict: batch exceeds max_batch");
    if (C != 1 && C != 3) return fail("wtk_yolo_predict: frames must have 1 (gray) or 3 (BGR) channels");
    if (max_det != 1) return fail("wtk_yolo_predict: max_det must be 1 (yolo_controller.py:76 hard-wires it); wtk_yolo_predict_nms takes max_det > 1");
    if (H <= 0 || W <= 0) return fail("wtk_yolo_predict: bad frame size");
    DEVICE_GUARD(h);
    hipStream_t st = (hipStream_t)stream;
    if ((H != h->S_h || W != h->S_w) && ensure_staging(h, st)) return 1;
    return yolo_enqueue(Pass{h, frames_dev, B, C, st, H, W, conf, out_xywh, out_conf, out_anchor});
}

extern "C" int wtk_yolo_predict_nms(wtk_yolo *h, const uint8_t *frames_dev, int32_t B, int32_t H, int32_t W, int32_t C, float conf, float iou,
                                    int32_t max_det, float *out_xywh, float *out_conf, int32_t *out_cls, int32_t *out_anchor, int32_t *out_count,
                                    void *stream) {
    if (!h || !frames_dev || !out_xywh) return fail("wtk_yolo_predict_nms: null argument");
    if (B <= 0) return fail("wtk_yolo_predict_nms: empty batch (the reference asserts len(frames) > 0, yolo_controller.py:65)");
    if (B > h->max_batch) return fail("wtk_yolo_predict_nms: batch exceeds max_batch");
    if (C != 1 && C != 3) return fail("wtk_yolo_predict_nms: frames must have 1 (gray) or 3 (BGR) channels");
    if (max_det < 1 || max_det > 30000) return fail("wtk_yolo_predict_nms: max_det must be in [1, 30000]");
    if (!(iou >= 0.f && iou <= 1.f)) return fail("wtk_yolo_predict_nms: iou must be in [0, 1]");
    if (H <= 0 || W <= 0) return fail("wtk_yolo_predict_nms: bad frame size");
    DEVICE_GUARD(h);
    hipStream_t st = (hipStream_t)stream;
    if ((H != h->S_h || W != h->S_w) && ensure_staging(h, st)) return 1;
    if (ensure_nms_scratch(h, st)) return 1;
    const NmsOut nms{iou, max_det, out_cls, out_count};
    return yolo_enqueue(Pass{h, frames_dev, B, C, st, H, W, conf, out_xywh, out_conf, out_anchor, nullptr, &nms});
}

extern "C" int wtk_yolo_predict_views(wtk_yolo *h, const uint8_t *frames_dev, int32_t n_frames, int32_t H, int32_t W, int32_t C,
                                      const int32_t *frame_index_dev, const int32_t *pos_xy_dev, int32_t B, int32_t view_w, int32_t view_h, float conf,
                                      float iou, int32_t max_det, float *out_xywh, float *out_conf, int32_t *out_anchor, void *stream) {
    (void)iou;
    if (!h || !frames_dev || !pos_xy_dev || !out_xywh) return fail("wtk_yolo_predict_views: null argument");
    if (B <= 0) return fail("wtk_yolo_predict_views: empty batch (the reference asserts len(frames) > 0, yolo_controller.py:65)");
    if (B > h->max_batch) return fail("wtk_yolo_predict_views: batch exceeds max_batch");
    if (C != 1 && C != 3) return fail("wtk_yolo_predict_views: frames must have 1 (gray) or 3 (BGR) channels");
    if (max_det != 1) return fail("wtk_yolo_predict_views: max_det must be 1 (yolo_controller.py:76 hard-wires it)");
    if (H <= 0 || W <= 0 || view_w <= 0 || view_h <= 0 || n_frames <= 0) return fail("wtk_yolo_predict_views: bad frame / view size");
    if (!frame_index_dev && B > n_frames) return fail("wtk_yolo_predict_views: without frame_index the batch rows are frames 0..B-1");
    DEVICE_GUARD(h);
    hipStream_t st = (hipStream_t)stream;
    if (ensure_staging(h, st)) return 1;
    const ViewSrc vs{pos_xy_dev, frame_index_dev, view_w, view_h, n_frames};
    return yolo_enqueue(Pass{h, frames_dev, B, C, st, H, W, conf, out_xywh, out_conf, out_anchor, &vs});
}

extern "C" int wtk_yolo_predict_host(wtk_yolo *h, const uint8_t *frames_host, int32_t B, int32_t H, int32_t W, int32_t C, float conf,
                                     float iou, int32_t max_det, float *out_xywh, float *out_conf, int32_t *out_anchor) {
    if (!h || !frames_host || !out_xywh) return fail("wtk_yolo_predict_host: null argument");
    if (B <= 0) return fail("wtk_yolo_predict_host: empty batch (the reference asserts len(frames) > 0, yolo_controller.py:65)");
    if (B > h->max_batch) return fail("wtk_yolo_predict_host: batch exceeds max_batch");
    if (H <= 0 || W <= 0 || (C != 1 && C != 3)) return fail("wtk_yolo_predict_host: bad frame shape");
    DEVICE_GUARD(h);
    const size_t need = (size_t)B * H * W * C;
    if (need > h->frames_cap) {
        (void)hipFree(h->frames_dev);
        h->frames_dev = nullptr;
        h->frames_cap = 0;
        const size_t cap = std::max(need, (size_t)h->max_batch * H * W * C);
        HIP_TRY(hipMalloc(&h->frames_dev, cap));
        h->frames_cap = cap;
    }
    if (!h->host_stream && pooled_stream(h->device, &h->host_stream)) return 1;
    hipStream_t st = h->host_stream;
    HIP_TRY(hipMemcpyAsync(h->frames_dev, frames_host, need, hipMemcpyHostToDevice, st));
    if (wtk_yolo_predict(h, h->frames_dev, B, H, W, C, conf, iou, max_det, h->o_xywh, h->o_conf, h->o_anchor, st)) return 1;
    HIP_TRY(hipMemcpyAsync(out_xywh, h->o_xywh, sizeof(float) * 4 * B, hipMemcpyDeviceToHost, st));
    if (out_conf) HIP_TRY(hipMemcpyAsync(out_conf, h->o_conf, sizeof(float) * B, hipMemcpyDeviceToHost, st));
    if (out_anchor) HIP_TRY(hipMemcpyAsync(out_anchor, h->o_anchor, sizeof(int) * B, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

extern "C" int wtk_yolo_set_side_streams(wtk_yolo *h, int32_t n) {
    if (!h || n < 0 || n > 2) return fail("wtk_yolo_set_side_streams: n must be 0, 1 or 2");
    h->side_streams = n;
    h->use_side = n > 0;
    return 0;
}

extern "C" int wtk_yolo_set_dynamic_batch(wtk_yolo *h, const int32_t *n_dev) {
    if (!h) return fail("wtk_yolo_set_dynamic_batch: null handle");
    h->n_dyn = n_dev;
    return 0;
}

extern "C" int wtk_yolo_margin_buffer(wtk_yolo *h, const float **margins_dev) {
    if (!h || !margins_dev) return fail("wtk_yolo_margin_buffer: null argument");
    *margins_dev = h->o_margin;
    return 0;
}

extern "C" int wtk_yolo_last_margins_host(wtk_yolo *h, int32_t B, float *margins_host) {
    if (!h || !margins_host || B <= 0 || B > h->max_batch) return fail("wtk_yolo_last_margins_host: bad argument");
    DEVICE_GUARD(h);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(margins_host, h->o_margin, sizeof(float) * B, hipMemcpyDeviceToHost));
    return 0;
}

static void to_f32(const void *src, float *dst, size_t n, int is_f16) {
    if (!is_f16) {
        std::memcpy(dst, src, n * 4);
        return;
    }
    const _Float16 *s = reinterpret_cast<const _Float16 *>(src);
    for (size_t i = 0; i < n; ++i) dst[i] = (float)s[i];
}

extern "C" int wtk_yolo_debug_head(wtk_yolo *h, int32_t level, int32_t B, float *box_host, float *cls_host) {
    if (!h || level < 0 || level > 2 || B <= 0 || B > h->max_batch) return fail("wtk_yolo_debug_head: bad argument");
    DEVICE_GUARD(h);
    HIP_TRY(hipDeviceSynchronize());
    if (box_host && complete_box_towers(h)) return 1; // (a sparse pass computed the survivors' box logits only)
    const size_t A = (size_t)h->lh[level] * h->lw[level];
    if (box_host) {
        const size_t n = (size_t)B * A * 64;
        HIP_TRY(hipMemcpy(box_host, h->bufs[h->box_buf[level]].ptr, n * 4, hipMemcpyDeviceToHost)); // fp32 in both modes
    }
    if (cls_host) {
        const size_t n = (size_t)B * A * h->cls_ld;
        std::vector<float> full(n);
        HIP_TRY(hipMemcpy(full.data(), h->bufs[h->cls_buf[level]].ptr, n * 4, hipMemcpyDeviceToHost)); // fp32 in both modes
        for (size_t i = 0; i < (size_t)B * A; ++i)
            for (int k = 0; k < h->dims.nc; ++k) cls_host[i * h->dims.nc + k] = full[i * h->cls_ld + k];
    }
    return 0;
}

extern "C" int wtk_yolo_debug_tensor(wtk_yolo *h, int32_t conv_index, int32_t B, float *out_host, size_t out_cap, int32_t *shape_hwc) {
    if (!h || B <= 0 || B > h->max_batch) return fail("wtk_yolo_debug_tensor: bad argument");
    if (conv_index == WTK_DEBUG_SPARSE_COUNTS) { // no conv: [1][1][4] = tiles the last list-form sparse pass listed for box.0 and box.1 + box.2, and the grids it launched
        if (shape_hwc) shape_hwc[0] = 1, shape_hwc[1] = 1, shape_hwc[2] = 4;
        if (!out_host) return 0;
        if (out_cap < 4) return fail("wtk_yolo_debug_tensor: output buffer too small");
        unsigned cnt[2] = {0, 0};
        if (h->live_list_cap[0]) {
            DEVICE_GUARD(h);
            HIP_TRY(hipDeviceSynchronize());
            // count[2], count[3]: where head_decode_kernel leaves the two stages' counts (HeadSparseArgs)
            HIP_TRY(hipMemcpy(cnt, reinterpret_cast<const char *>(h->zero_page) + kZeroPageBytes + sparse_count_off(h->live_mask_bytes) + 2 * sizeof(unsigned), sizeof(cnt), hipMemcpyDeviceToHost));
        }
        out_host[0] = (float)cnt[0], out_host[1] = (float)cnt[1], out_host[2] = (float)h->sparse_grid[0], out_host[3] = (float)h->sparse_grid[1];
        return 0;
    }
    const bool raw = conv_index <= WTK_DEBUG_RAW(0); // the tensor as the last pass left it: no dense completion of a sparse pass
    if (raw) conv_index = WTK_DEBUG_RAW(conv_index);
    const Op *op = nullptr;
    for (const Op &o : h->ops)
        if (o.spec == conv_index && o.out_buf >= 0) op = &o;
    if (!op) return fail("wtk_yolo_debug_tensor: no op computes conv " + std::to_string(conv_index));
    const Buf &b = h->bufs[op->out_buf];
    if (shape_hwc) shape_hwc[0] = b.h, shape_hwc[1] = b.w, shape_hwc[2] = op->cout;
    if (!out_host) return 0;
    const size_t px = (size_t)B * b.h * b.w;
    if (out_cap < px * op->cout) return fail("wtk_yolo_debug_tensor: output buffer too small");
    DEVICE_GUARD(h);
    HIP_TRY(hipDeviceSynchronize());
    for (int l = 0; l < 3; ++l) { // a box-tower conv: a sparse pass computed it on the survivors' tiles only
        const int oi = (int)(op - h->ops.data());
        if (!raw && (oi == h->det[l].op0 || oi == h->det[l].box1 || oi == h->det[l].box2) && complete_box_towers(h)) return 1;
    }
    if (!raw && h->c2f_tail_op >= 0 && op == &h->ops[h->c2f_tail_op] && complete_c2f_z(h, B)) return 1; // z, which the fused launch does not store
    std::vector<char> tmp(px * b.C * (b.f32 ? 4 : h->esize));
    HIP_TRY(hipMemcpy(tmp.data(), b.ptr, tmp.size(), hipMemcpyDeviceToHost));
    std::vector<float> full(px * b.C);
    if (h->split && !b.f32) {
        const _Float16 *sp = reinterpret_cast<const _Float16 *>(tmp.data());
        for (size_t i = 0; i < px; ++i)
            for (int c = 0; c < b.C; ++c) {
                const size_t o = i * 2 * b.C + 64 * (c >> 5) + (c & 31);
                full[i * b.C + c] = (float)sp[o] + (float)sp[o + 32] * kSplitInv;
            }
    } else {
        to_f32(tmp.data(), full.data(), full.size(), b.f32 ? 0 : h->is_f16);
    }
    const float unscale = op->act ? 1.0f / kActScale : 1.0f; // SiLU outputs are stored log2(e)-scaled
    for (size_t i = 0; i < px; ++i)
        for (int k = 0; k < op->cout; ++k) out_host[i * op->cout + k] = full[i * b.C + op->out_coff + k] * unscale;
    return 0;
}

static int upload_head_logits(wtk_yolo *h, const float *box_host, const float *cls_host, int32_t B);

extern "C" int wtk_yolo_decode_nms_host(wtk_yolo *h, const float *box_host, const float *cls_host, int32_t B, int32_t H, int32_t W, float conf, float iou,
                                        int32_t max_det, float *out_xywh, float *out_conf, int32_t *out_cls, int32_t *out_anchor, int32_t *out_count) {
    if (!h || !box_host || !cls_host || !out_xywh || B <= 0 || B > h->max_batch || max_det < 1) return fail("wtk_yolo_decode_nms_host: bad argument");
    DEVICE_GUARD(h);
    HIP_TRY(hipDeviceSynchronize());
    if (upload_head_logits(h, box_host, cls_host, B)) return 1;
    if (ensure_nms_scratch(h, nullptr)) return 1;
    const size_t rows = (size_t)B * max_det;
    float *d_xywh = nullptr, *d_conf = nullptr;
    int *d_cls = nullptr, *d_anchor = nullptr, *d_count = nullptr;
    hipError_t e = hipSuccess;
    if ((e = hipMalloc(&d_xywh, rows * 16)) != hipSuccess || (e = hipMalloc(&d_conf, rows * 4)) != hipSuccess || (e = hipMalloc(&d_cls, rows * 4)) != hipSuccess ||
        (e = hipMalloc(&d_anchor, rows * 4)) != hipSuccess || (e = hipMalloc(&d_count, (size_t)B * 4)) != hipSuccess) {
        (void)hipFree(d_xywh), (void)hipFree(d_conf), (void)hipFree(d_cls), (void)hipFree(d_anchor), (void)hipFree(d_count);
        return fail_hip("wtk_yolo_decode_nms_host: hipMalloc", e);
    }
    const NmsOut nms{iou, max_det, d_cls, d_count};
    int rc = run_head(Pass{h, nullptr, B, 0, nullptr, H, W, conf, d_xywh, d_conf, d_anchor, nullptr, &nms});
    if (!rc) {
        if ((e = hipMemcpy(out_xywh, d_xywh, rows * 16, hipMemcpyDeviceToHost)) != hipSuccess) rc = fail_hip("wtk_yolo_decode_nms_host: copy", e);
        if (!rc && out_conf && (e = hipMemcpy(out_conf, d_conf, rows * 4, hipMemcpyDeviceToHost)) != hipSuccess) rc = fail_hip("copy", e);
        if (!rc && out_cls && (e = hipMemcpy(out_cls, d_cls, rows * 4, hipMemcpyDeviceToHost)) != hipSuccess) rc = fail_hip("copy", e);
        if (!rc && out_anchor && (e = hipMemcpy(out_anchor, d_anchor, rows * 4, hipMemcpyDeviceToHost)) != hipSuccess) rc = fail_hip("copy", e);
        if (!rc && out_count && (e = hipMemcpy(out_count, d_count, (size_t)B * 4, hipMemcpyDeviceToHost)) != hipSuccess) rc = fail_hip("copy", e);
    }
    (void)hipFree(d_xywh), (void)hipFree(d_conf), (void)hipFree(d_cls), (void)hipFree(d_anchor), (void)hipFree(d_count);
    return rc;
}

extern "C" int wtk_yolo_decode_host(wtk_yolo *h, const float *box_host, const float *cls_host, int32_t B, int32_t H, int32_t W, float conf,
                                    float *out_xywh, float *out_conf, int32_t *out_anchor) {
    if (!h || !box_host || !cls_host || !out_xywh || B <= 0 || B > h->max_batch) return fail("wtk_yolo_decode_host: bad argument");
    DEVICE_GUARD(h);
    HIP_TRY(hipDeviceSynchronize());
    if (upload_head_logits(h, box_host, cls_host, B)) return 1;
    if (run_head(Pass{h, nullptr, B, 0, nullptr, H, W, conf, h->o_xywh, h->o_conf, h->o_anchor})) return 1;
    HIP_TRY(hipMemcpy(out_xywh, h->o_xywh, sizeof(float) * 4 * B, hipMemcpyDeviceToHost));
    if (out_conf) HIP_TRY(hipMemcpy(out_conf, h->o_conf, sizeof(float) * B, hipMemcpyDeviceToHost));
    if (out_anchor) HIP_TRY(hipMemcpy(out_anchor, h->o_anchor, sizeof(int) * B, hipMemcpyDeviceToHost));
    return 0;
}

// scatter concatenated [B][A][.] fp32 logits into the per-level head buffers (storage dtype): the test hook behind the two
// decode entry points
static int upload_head_logits(wtk_yolo *h, const float *box_host, const float *cls_host, int32_t B) {
    const int A = h->anchors;
    size_t a0 = 0;
    for (int l = 0; l < 3; ++l) {
        const size_t Al = (size_t)h->lh[l] * h->lw[l];
        std::vector<float> bx((size_t)B * Al * 64), cl((size_t)B * Al * h->cls_ld, 0.f);
        for (int n = 0; n < B; ++n)
            for (size_t j = 0; j < Al; ++j) {
                std::memcpy(&bx[((size_t)n * Al + j) * 64], &box_host[((size_t)n * A + a0 + j) * 64], 64 * sizeof(float));
                for (int k = 0; k < h->dims.nc; ++k) cl[((size_t)n * Al + j) * h->cls_ld + k] = cls_host[((size_t)n * A + a0 + j) * h->dims.nc + k];
            }
        HIP_TRY(hipMemcpy(h->bufs[h->box_buf[l]].ptr, bx.data(), bx.size() * 4, hipMemcpyHostToDevice)); // fp32 in both modes
        HIP_TRY(hipMemcpy(h->bufs[h->cls_buf[l]].ptr, cl.data(), cl.size() * 4, hipMemcpyHostToDevice));
        a0 += Al;
    }
    h->sparse_B = 0; // the head buffers now hold the caller's logits, all of them
    return 0;
}

