// TEST INFRASTRUCTURE (included by hip_stub.cpp): per-launch checks of the library's own kernels.  The launch layer runs no kernel; what it CAN do is
// what a careful host would do before every launch of a hand-written kernel: look at the argument struct the kernel is about to read and check that every
// pointer is a live device allocation and that the extent the kernel's indexing implies (pixels x leading dimension + channel offset + channels, in the
// element size of the instantiation) fits inside that allocation.  A planner / launcher inconsistency that would make a kernel read or write out of bounds
// on the GPU shows up here as a violation, in the build container.
#include "../../wtracker_amd/csrc/wtk_kernels.h"

namespace stubchk {

struct TArgs { // template arguments of an instantiation, parsed from the mangled name
    bool f16 = false, f32 = false;
    std::vector<long long> ints; // Li..E and Lb..E in order
};
static TArgs parse_targs(const std::string &mangled, const char *kernel) {
    TArgs t;
    size_t p = mangled.find(kernel);
    if (p == std::string::npos) return t;
    p += std::strlen(kernel);
    if (p >= mangled.size() || mangled[p] != 'I') return t;
    ++p;
    while (p < mangled.size() && mangled[p] != 'E') {
        if (mangled.compare(p, 5, "DF16_") == 0) {
            t.f16 = true, p += 5;
        } else if (mangled[p] == 'f') {
            t.f32 = true, ++p;
        } else if (mangled[p] == 'L' && p + 1 < mangled.size() && (mangled[p + 1] == 'i' || mangled[p + 1] == 'b' || mangled[p + 1] == 'j')) {
            p += 2;
            bool neg = false;
            if (p < mangled.size() && mangled[p] == 'n') neg = true, ++p;
            long long v = 0;
            while (p < mangled.size() && mangled[p] >= '0' && mangled[p] <= '9') v = v * 10 + (mangled[p++] - '0');
            t.ints.push_back(neg ? -v : v);
            if (p < mangled.size() && mangled[p] == 'E') ++p;
        } else
            break; // something this parser does not know: keep what it has
    }
    return t;
}

// bytes a channel-slice view needs: (pixels - 1) * ld + coff + channels elements
static size_t view_bytes(long long pixels, long long ld, long long coff, long long channels, int es) {
    if (pixels <= 0) return 0;
    return (size_t)(((pixels - 1) * ld + coff + channels) * es);
}

static void check_conv_args(const char *kn, const wtk::ConvArgs &a, int es, bool split) {
    const long long px_in = (long long)a.N * a.H * a.W, px_out = (long long)a.N * a.Ho * a.Wo;
    if (a.M != px_out) fail(kn, "ConvArgs.M != N * Ho * Wo");
    if (a.in_coff + a.Cin > a.in_ld) fail(kn, "input slice [in_coff, in_coff + Cin) leaves the pixel (in_ld)");
    dev_ptr_ok(a.in, view_bytes(px_in, a.in_ld, a.in_coff, a.Cin, es), kn, "in");
    dev_ptr_ok(a.w, (size_t)a.CoutPad * a.Kpad * es, kn, "w");
    dev_ptr_ok(a.bias, (size_t)a.CoutPad * 4, kn, "bias");
    dev_ptr_ok(a.zeros, 16, kn, "zeros");
    const int stored = a.Cout * ((split && !a.out_f32) ? 2 : 1), es_out = a.out_f32 ? 4 : es;
    if (!a.tail_w) {
        if (a.out_coff + stored > a.out_ld) fail(kn, "output slice leaves the pixel (out_ld)");
        dev_ptr_ok(a.out, view_bytes(px_out, a.out_ld, a.out_coff, stored, es_out), kn, "out");
    } else {
        dev_ptr_ok(a.tail_w, (size_t)128 * a.tail_kpad * es, kn, "tail_w");
        dev_ptr_ok(a.tail_bias, 128 * 4, kn, "tail_bias");
        dev_ptr_ok(a.tail_out, view_bytes(px_out, a.tail_ld, a.tail_coff, 128, es), kn, "tail_out");
    }
    if (a.out2) dev_ptr_ok(a.out2, view_bytes(4 * px_out, a.out2_ld, a.out2_coff, a.Cout * (split ? 2 : 1), es), kn, "out2");
    if (a.res) dev_ptr_ok(a.res, view_bytes(px_out, a.res_ld, a.res_coff, a.Cout * (split ? 2 : 1), es), kn, "res");
    if (a.in2) {
        if ((a.H & 1) || (a.W & 1)) fail(kn, "two-source conv on an odd map");
        dev_ptr_ok(a.in2, view_bytes((long long)a.N * (a.H / 2) * (a.W / 2), a.in2_ld, a.in2_coff, a.in2_split, es), kn, "in2");
    }
    const int pad_out_h = (a.H + 2 * a.pad - a.KH) / a.stride + 1, pad_out_w = (a.W + 2 * a.pad - a.KW) / a.stride + 1;
    if (pad_out_h != a.Ho || pad_out_w != a.Wo) fail(kn, "Ho / Wo do not follow from H / W / k / stride / pad");
    if (a.CoutPad < a.Cout) fail(kn, "CoutPad < Cout");
}

// HaloArgs kernels: stride-1 window kernels (H x W = input = output map) and the strided parity-plane kernel (H x W = OUTPUT map, input 2H x 2W)
static void check_halo_args(const char *kn, const wtk::HaloArgs &a, int es, bool split, bool strided) {
    const long long px_out = (long long)a.N * a.H * a.W, px_in = strided ? 4 * px_out : px_out;
    if (a.in_coff + a.Cin > a.in_ld) fail(kn, "input slice leaves the pixel (in_ld)");
    dev_ptr_ok(a.in, view_bytes(px_in, a.in_ld, a.in_coff, a.Cin, es), kn, "in");
    dev_ptr_ok(a.w, (size_t)a.CoutPad * a.Kpad * es, kn, "w");
    dev_ptr_ok(a.bias, (size_t)a.CoutPad * 4, kn, "bias");
    dev_ptr_ok(a.zeros, 16, kn, "zeros");
    const int stored = a.Cout * (split ? 2 : 1);
    if (!a.tail_w) {
        if (a.out_coff + stored > a.out_ld) fail(kn, "output slice leaves the pixel (out_ld)");
        dev_ptr_ok(a.out, view_bytes(px_out, a.out_ld, a.out_coff, stored, es), kn, "out");
    } else {
        const int tstored = a.tail_cout * ((split && !a.tail_f32) ? 2 : 1);
        dev_ptr_ok(a.tail_w, (size_t)a.tail_cout * a.tail_kpad * es, kn, "tail_w"); // (at least the stored rows)
        dev_ptr_ok(a.tail_bias, (size_t)a.tail_cout * 4, kn, "tail_bias");
        dev_ptr_ok(a.tail_out, view_bytes(px_out, a.tail_ld, a.tail_coff, tstored, a.tail_f32 ? 4 : es), kn, "tail_out");
    }
    if (a.out2) dev_ptr_ok(a.out2, view_bytes(4 * px_out, a.out2_ld, a.out2_coff, stored, es), kn, "out2");
    if (a.res) dev_ptr_ok(a.res, view_bytes(px_out, a.res_ld, a.res_coff, stored, es), kn, "res");
    if (a.S <= 0 || a.pitch <= 0 || a.strips <= 0 || a.blocks_per_strip <= 0) fail(kn, "strip geometry not filled in (S / pitch / strips / blocks_per_strip)");
    if (a.CoutPad < a.Cout) fail(kn, "CoutPad < Cout");
}

// The window family: the instantiation a launch names (the template integers of its symbol: conv3x3_halo_kernel<T, BN, NHALO, MINW, NWB, HROWS, BMT, TAIL,
// SPLIT>, conv3x3_halo_pkernel<T, BN, HROWS>) must be the one wtk::halo_variant derives from the launch's own argument struct
static void check_halo_variant(const char *kn, const TArgs &t, bool persistent, const wtk::HaloArgs &a) {
    const std::vector<long long> &i = t.ints;
    if (i.size() != (persistent ? 2u : 8u) || t.f16 == t.f32) return fail(kn, "template arguments of the symbol not understood");
    const wtk::HaloVariant named = persistent ? wtk::HaloVariant{t.f16, (int)i[0], 2, 2, 3, (int)i[1], 256, 0, 0, 1}
                                              : wtk::HaloVariant{t.f16, (int)i[0], (int)i[1], (int)i[2], (int)i[3], (int)i[4], (int)i[5], (int)i[6], (int)i[7], 0};
    wtk::HaloVariant v;
    if (!wtk::halo_variant(a, named.split ? wtk::HALO_SPLIT : t.f16 ? wtk::HALO_F16 : wtk::HALO_F32, &v))
        fail(kn, "halo_variant has no instantiation for the arguments of this launch");
    else if (!(v == named))
        fail(kn, "the launched instantiation is not the one halo_variant names for its arguments");
}

// returns the size of the kernel's argument struct (args[0]) for the launch trace, 0 for a kernel that is not listed here
static size_t check_launch(const std::string &name, dim3 grid, dim3 block, void **args) {
    (void)grid, (void)block;
    if (!args || !args[0]) return 0;
    size_t bytes = 0;
    auto has = [&](const char *s) { return name.find(s) != std::string::npos; };
    if (has("conv_igemm_kernel")) {
        bytes = sizeof(wtk::ConvArgs);
        const TArgs t = parse_targs(name, "conv_igemm_kernel");
        const auto &a = *reinterpret_cast<const wtk::ConvArgs *>(args[0]);
        // <T, BM, BN, WAVES_P, WAVES_C, bools..., SPLIT>: SPLIT is the last bool when there are 9 value arguments
        const bool split = t.ints.size() >= 9 && t.ints.back() == 1;
        check_conv_args("conv_igemm_kernel", a, t.f16 ? 2 : 4, split);
    } else if (has("conv_sk_kernel")) {
        bytes = sizeof(wtk::SkGroupArgs);
        const TArgs t = parse_targs(name, "conv_sk_kernel"); // <SPLIT, BM, BN, WAVES_P, WAVES_C, NS>
        const bool split = !t.ints.empty() && t.ints[0] == 1;
        const int bm = t.ints.size() > 1 ? (int)t.ints[1] : 64, bn = t.ints.size() > 2 ? (int)t.ints[2] : 32;
        const auto &g = *reinterpret_cast<const wtk::SkGroupArgs *>(args[0]);
        unsigned long long blocks = 0;
        for (int i = 0; i < wtk::kSkGroupMax; ++i) {
            if (g.first[i] == 0xffffffffu) continue;
            const wtk::SkArgs &a = g.p[i];
            const char *kn = "conv_sk_kernel";
            if (g.first[i] != blocks) fail(kn, "member grids are not concatenated in order");
            if (a.ptiles != (int)((a.M + bm - 1) / bm) || a.nct * bn != a.CoutPad) fail(kn, "tile counts do not match the instantiation");
            blocks += (unsigned long long)a.ptiles * a.nct * a.S;
            const long long px_in = (long long)a.N * a.H * a.W, px_out = (long long)a.N * a.Ho * a.Wo;
            if (a.M != px_out) fail(kn, "M != N * Ho * Wo");
            if (a.S != 1 && a.S != a.NA) fail(kn, "S is neither 1 nor the atom count");
            if (a.NA < 1 || a.NA > 8 || a.NA > a.nk) fail(kn, "atom count out of range");
            const int cpb_real = a.cpb - a.in2_blocks;
            dev_ptr_ok(a.in, (size_t)((px_in - 1) * a.in_ldb + a.in_offb + (size_t)a.cpb * 128), kn, "in"); // (a two-source conv addresses `in` by the block index of the concat)
            (void)cpb_real;
            if (a.in2) dev_ptr_ok(a.in2, (size_t)(((long long)a.N * (a.H / 2) * (a.W / 2) - 1) * a.in2_ldb + a.in2_offb + (size_t)a.in2_blocks * 128), kn, "in2");
            dev_ptr_ok(a.w, (size_t)a.CoutPad * a.w_rowb, kn, "w");
            dev_ptr_ok(a.bias, (size_t)a.CoutPad * 4, kn, "bias");
            const int es_out = (!split || a.out_f32) ? 4 : 2, stored = a.Cout * ((split && !a.out_f32) ? 2 : 1);
            dev_ptr_ok(a.out, view_bytes(px_out, a.out_ld, a.out_coff, stored, es_out), kn, "out");
            if (a.res) dev_ptr_ok(a.res, view_bytes(px_out, a.res_ld, a.res_coff, a.Cout * (split ? 2 : 1), split ? 2 : 4), kn, "res");
            if (a.S > 1) {
                dev_ptr_ok(a.partial, (size_t)a.S * a.M * a.CoutPad * 4, kn, "partial");
                if (a.tickets) dev_ptr_ok(a.tickets, (size_t)a.ptiles * a.nct * 4, kn, "tickets");
            }
            if (a.n_dyn) dev_ptr_ok(a.n_dyn, 4, kn, "n_dyn");
        }
        if (blocks != grid.x) fail("conv_sk_kernel", "grid does not equal the sum of the members' grids");
    } else if (has("sk_finish_kernel")) {
        bytes = sizeof(wtk::SkArgs);
        const auto &a = *reinterpret_cast<const wtk::SkArgs *>(args[0]);
        dev_ptr_ok(a.partial, (size_t)a.S * a.M * a.CoutPad * 4, "sk_finish_kernel", "partial");
    } else if (has("conv1x1_wide_kernel")) {
        bytes = sizeof(wtk::ConvArgs);
        check_conv_args("conv1x1_wide_kernel", *reinterpret_cast<const wtk::ConvArgs *>(args[0]), 2, false);
    } else if (has("conv3x3_halo_kernel") || has("conv3x3_halo_pkernel")) {
        bytes = sizeof(wtk::HaloArgs);
        const bool persistent = has("conv3x3_halo_pkernel");
        const TArgs t = parse_targs(name, persistent ? "conv3x3_halo_pkernel" : "conv3x3_halo_kernel");
        // conv3x3_halo_kernel<T, BN, NHALO, MINW, NWB, HROWS, BMT, TAIL, SPLIT>
        const bool split = !persistent && t.ints.size() >= 8 && t.ints.back() == 1;
        check_halo_args(persistent ? "conv3x3_halo_pkernel" : "conv3x3_halo_kernel", *reinterpret_cast<const wtk::HaloArgs *>(args[0]), t.f16 ? 2 : 4, split, false);
        check_halo_variant(persistent ? "conv3x3_halo_pkernel" : "conv3x3_halo_kernel", t, persistent, *reinterpret_cast<const wtk::HaloArgs *>(args[0]));
    } else if (has("halo_list_kernel")) {
        // halo_list_kernel<TAIL>: every member, on the block size of the list and without the knobs the list kernel does not read, must come out as the list
        // kernel's fixed tile.  (bytes stays 0: the recorded traces hash no argument struct for this kernel.)
        const TArgs t = parse_targs(name, "halo_list_kernel");
        wtk::HaloVariant want = wtk::kHaloListVariant, v;
        want.tail = !t.ints.empty() && t.ints[0] == 1;
        for (wtk::HaloArgs m : reinterpret_cast<const wtk::HaloListArgs *>(args[0])->m) {
            m.bm = want.bmt, m.deep = 0;
            if (!wtk::halo_variant(m, wtk::HALO_SPLIT, &v) || !(v == want)) fail("halo_list_kernel", "a member does not come out as kHaloListVariant");
        }
    } else if (has("conv3x3_ws64_kernel")) {
        bytes = sizeof(wtk::HaloArgs);
        check_halo_args("conv3x3_ws64_kernel", *reinterpret_cast<const wtk::HaloArgs *>(args[0]), 2, false, false);
    } else if (has("conv3x3_s2_kernel")) {
        bytes = sizeof(wtk::HaloArgs);
        const TArgs t = parse_targs(name, "conv3x3_s2_kernel"); // <BMT, SPLIT>
        check_halo_args("conv3x3_s2_kernel", *reinterpret_cast<const wtk::HaloArgs *>(args[0]), 2, t.ints.size() >= 2 && t.ints[1] == 1, true);
    } else if (has("conv3x3_c32_split_kernel")) {
        bytes = sizeof(wtk::HaloArgs);
        check_halo_args("conv3x3_c32_split_kernel", *reinterpret_cast<const wtk::HaloArgs *>(args[0]), 2, true, false);
    } else if (has("conv3x3_c32_kernel")) {
        bytes = sizeof(wtk::HaloArgs);
        check_halo_args("conv3x3_c32_kernel", *reinterpret_cast<const wtk::HaloArgs *>(args[0]), 2, false, false);
    } else if (has("front_fused_split_kernel") || has("front_fused_kernel")) {
        bytes = sizeof(wtk::FrontArgs);
        const bool split = has("front_fused_split_kernel");
        const char *kn = split ? "front_fused_split_kernel" : "front_fused_kernel";
        const auto &a = *reinterpret_cast<const wtk::FrontArgs *>(args[0]);
        dev_ptr_ok(a.frames, (size_t)a.N * a.H * a.W * a.C, kn, "frames");
        dev_ptr_ok(a.w0, 32, kn, "w0"), dev_ptr_ok(a.b0, 32 * 4, kn, "b0");
        dev_ptr_ok(a.w1, (size_t)64 * a.Kpad1 * 2, kn, "w1"), dev_ptr_ok(a.b1, 64 * 4, kn, "b1");
        dev_ptr_ok(a.w2, (size_t)64 * a.Kpad2 * 2, kn, "w2"), dev_ptr_ok(a.b2, 64 * 4, kn, "b2");
        dev_ptr_ok(a.out, view_bytes((long long)a.N * (a.H / 4) * (a.W / 4), a.out_ld, a.out_coff, split ? 128 : 64, 2), kn, "out");
        if ((a.H % 4) || (a.W % 4)) fail(kn, "frame size not a multiple of 4");
    } else if (has("c2f32_fused_kernel")) {
        bytes = sizeof(wtk::C2fArgs);
        const auto &a = *reinterpret_cast<const wtk::C2fArgs *>(args[0]);
        const long long px = (long long)a.N * a.H * a.W;
        dev_ptr_ok(a.cat, view_bytes(px, a.cat_ld, std::max(a.a_coff, a.b_coff), 32, 2), "c2f32_fused_kernel", "cat");
        dev_ptr_ok(a.out, view_bytes(px, a.out_ld, a.out_coff, 64, 2), "c2f32_fused_kernel", "out");
        dev_ptr_ok(a.w_m1, (size_t)32 * a.Kpad_m * 2, "c2f32_fused_kernel", "w_m1"), dev_ptr_ok(a.w_m2, (size_t)32 * a.Kpad_m * 2, "c2f32_fused_kernel", "w_m2");
        dev_ptr_ok(a.w_cv2, (size_t)64 * a.Kpad_cv2 * 2, "c2f32_fused_kernel", "w_cv2");
        dev_ptr_ok(a.zeros, 16, "c2f32_fused_kernel", "zeros");
    } else if (has("stem_mfma_kernel")) {
        bytes = sizeof(wtk::StemArgs);
        const TArgs t = parse_targs(name, "stem_mfma_kernel");
        const auto &a = *reinterpret_cast<const wtk::StemArgs *>(args[0]);
        dev_ptr_ok(a.frames, (size_t)a.N * a.H * a.W * a.C, "stem_mfma_kernel", "frames");
        const int es = t.f16 || a.out_split ? 2 : 4;
        dev_ptr_ok(a.out, (size_t)a.N * a.Ho * a.Wo * a.Cout * (a.out_split ? 2 : 1) * es, "stem_mfma_kernel", "out");
        dev_ptr_ok(a.bias, (size_t)a.Cout * 4, "stem_mfma_kernel", "bias");
        if (a.Ho * 2 != a.H || a.Wo * 2 != a.W) fail("stem_mfma_kernel", "Ho / Wo are not H / 2, W / 2");
    } else if (has("sppf_pool_kernel")) {
        bytes = sizeof(wtk::PoolArgs);
        const TArgs t = parse_targs(name, "sppf_pool_kernel");
        const auto &a = *reinterpret_cast<const wtk::PoolArgs *>(args[0]);
        dev_ptr_ok(a.buf, (size_t)a.N * a.H * a.W * 4 * a.c * (t.f16 || a.split ? 2 : 4) * (a.split ? 2 : 1), "sppf_pool_kernel", "buf");
    } else if (has("head_select_kernel") || has("head_nms_kernel")) {
        const bool nms = has("head_nms_kernel");
        bytes = nms ? sizeof(wtk::NmsArgs) : sizeof(wtk::HeadArgs);
        const char *kn = nms ? "head_nms_kernel" : "head_select_kernel";
        const wtk::HeadArgs &a = nms ? reinterpret_cast<const wtk::NmsArgs *>(args[0])->h : *reinterpret_cast<const wtk::HeadArgs *>(args[0]);
        long long A = 0;
        for (int l = 0; l < 3; ++l) {
            const long long px = (long long)a.N * a.lh[l] * a.lw[l];
            A += (long long)a.lh[l] * a.lw[l];
            dev_ptr_ok(a.box[l], (size_t)px * 64 * 4, kn, "box[l]");
            dev_ptr_ok(a.cls[l], (size_t)px * a.cls_ld * 4, kn, "cls[l]");
        }
        if (a.nc > a.cls_ld) fail(kn, "nc > cls_ld");
        if (a.status) dev_ptr_ok(a.status, 4, kn, "status");
        if (a.out_margin) dev_ptr_ok(a.out_margin, (size_t)a.N * 4, kn, "out_margin");
        if (nms) {
            const auto &q = *reinterpret_cast<const wtk::NmsArgs *>(args[0]);
            dev_ptr_ok(q.scratch_score, (size_t)a.N * A * 4, kn, "scratch_score");
            dev_ptr_ok(q.scratch_cls, (size_t)a.N * A * 4, kn, "scratch_cls");
            dev_ptr_ok(q.scratch_box, (size_t)a.N * A * 16, kn, "scratch_box");
            dev_ptr_ok(q.out_xywh, (size_t)a.N * q.max_det * 16, kn, "out_xywh");
            if (q.out_conf) dev_ptr_ok(q.out_conf, (size_t)a.N * q.max_det * 4, kn, "out_conf");
            if (q.out_cls) dev_ptr_ok(q.out_cls, (size_t)a.N * q.max_det * 4, kn, "out_cls");
            if (q.out_anchor) dev_ptr_ok(q.out_anchor, (size_t)a.N * q.max_det * 4, kn, "out_anchor");
            if (q.out_count) dev_ptr_ok(q.out_count, (size_t)a.N * 4, kn, "out_count");
        } else {
            dev_ptr_ok(a.out_xywh, (size_t)a.N * 16, kn, "out_xywh");
            if (a.out_conf) dev_ptr_ok(a.out_conf, (size_t)a.N * 4, kn, "out_conf");
            if (a.out_anchor) dev_ptr_ok(a.out_anchor, (size_t)a.N * 4, kn, "out_anchor");
        }
    } else if (has("view_letterbox_kernel")) {
        bytes = sizeof(wtk::ViewLetterboxArgs);
        const auto &a = *reinterpret_cast<const wtk::ViewLetterboxArgs *>(args[0]);
        dev_ptr_ok(a.frames, (size_t)a.F * a.H * a.W * a.C, "view_letterbox_kernel", "frames");
        dev_ptr_ok(a.pos_xy, (size_t)a.N * 8, "view_letterbox_kernel", "pos_xy");
        if (a.frame_index) dev_ptr_ok(a.frame_index, (size_t)a.N * 4, "view_letterbox_kernel", "frame_index");
        dev_ptr_ok(a.dst, (size_t)a.N * a.Sh * a.Sw * a.C, "view_letterbox_kernel", "dst");
    } else if (has("letterbox_kernel")) {
        bytes = sizeof(wtk::LetterboxArgs);
        const auto &a = *reinterpret_cast<const wtk::LetterboxArgs *>(args[0]);
        dev_ptr_ok(a.src, (size_t)a.N * a.H * a.W * a.C, "letterbox_kernel", "src");
        dev_ptr_ok(a.dst, (size_t)a.N * a.Sh * a.Sw * a.C, "letterbox_kernel", "dst");
    } else if (has("mlp_kernel")) {
        bytes = sizeof(wtk::MlpArgs);
        const auto &a = *reinterpret_cast<const wtk::MlpArgs *>(args[0]);
        dev_ptr_ok(a.params, (size_t)a.n_params * 4, "mlp_kernel", "params");
        dev_ptr_ok(a.layers, (size_t)a.n_layers * sizeof(wtk::MlpLayerDev), "mlp_kernel", "layers");
        if (a.x) dev_ptr_ok(a.x, (size_t)a.B * a.in_dim * 4, "mlp_kernel", "x");
        dev_ptr_ok(a.y, (size_t)a.B * a.out_dim * 4, "mlp_kernel", "y");
    }
    return bytes;
}

} // namespace stubchk

// selftest hook (driver.cpp): the variant check on a launch of conv3x3_halo_kernel<fp16, bn, 2, 2, 3, 432, 256, false, false> whose arguments — 64 -> 128
// channels, three slabs, 256-pixel blocks — ask for the 128-cout tile of that shape
extern "C" void stub_selftest_window_variant(int bn) {
    wtk::HaloArgs a{};
    a.Cin = 64, a.Cout = a.CoutPad = 128, a.strips = a.blocks_per_strip = 1, a.slabs = 3;
    const std::string name = "conv3x3_halo_kernelIDF16_Li" + std::to_string(bn) + "ELi2ELi2ELi3ELi432ELi256ELb0ELb0EE";
    stubchk::check_halo_variant("conv3x3_halo_kernel", stubchk::parse_targs(name, "conv3x3_halo_kernel"), false, a);
}
