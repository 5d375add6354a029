// 3x3 / stride-1 convolution for thin layers (fp16, Cin = 32, Cout <= 96) — YOLOv8s' first C2f
// bottleneck (model.2.m.0.cv1/cv2: 32 -> 32 channels on the 160x160 map, 64 frames = 1.6 M pixels).
//
// These layers are HBM / latency bound (K = 288, N = 32: 18 MFMA-cycles per pixel row), so the design
// removes every per-tap synchronisation instead of chasing MFMA rate:
//   * same flat-strip window as conv3x3_halo.hip, but a window row is 64 bytes (32 fp16 channels) and
//     ALL nine taps' weights ([9][Cout][64 B] <= 55 KB) are staged once next to it -> one barrier per
//     block, then 9 x (ds_read_b128 + MFMA) with no further waits;
//   * 46-83 KB of LDS and 256 threads per block -> 2-3 blocks per CU hide the staging latency;
//   * 64-byte rows need their own XOR swizzles (bank = (addr/4) % 64 covers FOUR rows): pixel rows use
//     key = (row >> 1) & 3, weight rows key = (((row / NV) & 1) << 1) | ((row >> 1) & 1); both were
//     checked conflict-free for every ds_read_b128 lane group and every tap offset by enumeration.
#include "wtk_device.h"

#include <algorithm>

namespace wtk {

namespace {

constexpr int kBM = 256;
constexpr int kRowsMax = kHaloRowsMax; // same strip geometry as the 128-byte-row kernel

template <int BN> // BN = CoutPad: 32, 64 or 96; 4 waves, each 64 px x BN cout
__global__ __launch_bounds__(256) void conv3x3_c32_kernel(const HaloArgs a) {
    constexpr int TC = BN / 16, TP = 4, NV = 4 * TC;
    constexpr int WROWS = 9 * BN; // weight rows (tap, cout), 64 B each
    __shared__ __attribute__((aligned(16))) char win[kRowsMax * 64];
    __shared__ __attribute__((aligned(16))) char wts[WROWS * 64];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 15, lg = lane >> 4;

    unsigned t = blockIdx.x;
    unsigned q = fdiv(t, a.d_bps);
    const int o0 = (int)(t - q * (unsigned)a.blocks_per_strip) * kBM;
    t = q;
    q = fdiv(t, a.d_strips);
    const int xs = (int)(t - q * (unsigned)a.strips) * a.S;
    const int n = (int)q;
    const int pitch = a.pitch;
    const int halo_rows = kBM + 2 * pitch + 2;
    const int halo_pieces = (halo_rows + 15) >> 4; // 16 rows of 64 B per 1-KiB LDS-DMA piece

    const _Float16 *in = reinterpret_cast<const _Float16 *>(a.in) + (long long)n * a.H * a.W * a.in_ld + a.in_coff;
    const _Float16 *wgt = reinterpret_cast<const _Float16 *>(a.w);
    const char *zero_page = reinterpret_cast<const char *>(a.zeros);

    // ---- stage the window: lane -> (row = piece*16 + lane/4, physical chunk = lane%4)
    for (int piece = wave; piece < halo_pieces; piece += 4) {
        const int hr = piece * 16 + (lane >> 2);
        const int lc = (lane & 3) ^ ((hr >> 1) & 3); // typed out: see wtk_device.h, operand-tile layout
        const unsigned flat = (unsigned)(o0 + hr);
        const unsigned r = fdiv(flat, a.d_pitch);
        const int cc = (int)(flat - r * (unsigned)pitch);
        const int iy = (int)r - 1, ix = xs + cc - 1;
        const bool ok = hr < halo_rows && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
        const char *src = ok ? reinterpret_cast<const char *>(in + ((long long)iy * a.W + ix) * a.in_ld + lc * 8) : zero_page;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                         (__attribute__((address_space(3))) void *)(win + piece * 1024), 16, 0, 0);
    }
    // ---- stage all nine weight slabs: LDS row = tap*BN + cout
    for (int piece = wave; piece < (WROWS + 15) / 16; piece += 4) {
        const int row = piece * 16 + (lane >> 2);
        const int tap = row / BN, co = row - tap * BN;
        static_assert(layout_check::is_weight_key<NV, 64>([](int co) { return (((co / NV) & 1) << 1) | ((co >> 1) & 1); }), "typed-out key differs from tile_weight_key");
        const int key = (((co / NV) & 1) << 1) | ((co >> 1) & 1); // typed out: see wtk_device.h, operand-tile layout
        const int lc = (lane & 3) ^ key;
        const char *src = row < WROWS ? reinterpret_cast<const char *>(wgt + (long long)co * a.Kpad + tap * 32 + lc * 8) : zero_page;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                         (__attribute__((address_space(3))) void *)(wts + piece * 1024), 16, 0, 0);
    }

    // accumulators start at the bias of this lane's couts (rows exist up to CoutPad), fetched while the window is in flight
    const int cb = lg * NV;
    floatx4 acc[TC][TP];
#pragma unroll
    for (int i = 0; i < TC; ++i) {
        const floatx4 b4 = (floatx4){a.bias[cb + i * 4 + 0], a.bias[cb + i * 4 + 1], a.bias[cb + i * 4 + 2], a.bias[cb + i * 4 + 3]};
#pragma unroll
        for (int j = 0; j < TP; ++j) acc[i][j] = b4;
    }

    const int wrow_l = (lr >> 2) * NV + (lr & 3); // + 4*i per cout tile, + tap*BN
    static_assert(layout_check::is_weight_key<NV, 64>([](int wrow_l) { return (((wrow_l / NV) & 1) << 1) | ((wrow_l >> 1) & 1); }), "typed-out key differs from tile_weight_key");
    const int wkey_l = (((wrow_l / NV) & 1) << 1) | ((wrow_l >> 1) & 1); // typed out: see wtk_device.h, operand-tile layout
    const unsigned wfrag0 = wrow_l * 64 + ((lg ^ wkey_l) << 4);
    const int prow0 = wave * 64 + lr;

    __syncthreads(); // the only barrier: window + weights have landed

#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        const int base = prow0 + (tap / 3) * pitch + (tap % 3);
        const unsigned pa = base * 64 + ((lg ^ ((base >> 1) & 3)) << 4); // tiles j: + j*1024 (key unchanged); typed out: see wtk_device.h, operand-tile layout
        half8 pf[TP], wf[TC];
#pragma unroll
        for (int j = 0; j < TP; ++j) pf[j] = *reinterpret_cast<const half8 *>(win + pa + j * 1024);
#pragma unroll
        for (int i = 0; i < TC; ++i) wf[i] = *reinterpret_cast<const half8 *>(wts + tap * (BN * 64) + wfrag0 + i * 256);
#pragma unroll
        for (int i = 0; i < TC; ++i)
#pragma unroll
            for (int j = 0; j < TP; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[i], pf[j], acc[i][j], 0, 0, 0);
    }

    // ---- epilogue: lane (pixel lr of tile j, group lg) owns couts lg*NV .. lg*NV+NV-1
    if (cb + NV > a.Cout) return;
    _Float16 *out = reinterpret_cast<_Float16 *>(a.out);
    const _Float16 *res = reinterpret_cast<const _Float16 *>(a.res);
#pragma unroll
    for (int j = 0; j < TP; ++j) {
        const unsigned o = (unsigned)(o0 + wave * 64 + j * 16 + lr);
        const unsigned y = fdiv(o, a.d_pitch);
        const int x = (int)(o - y * (unsigned)pitch);
        if ((int)y >= a.H || x >= a.S || xs + x >= a.W) continue;
        float v[NV];
#pragma unroll
        for (int i = 0; i < TC; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) v[i * 4 + r] = acc[i][j][r];
        if (a.act) {
#pragma unroll
            for (int i = 0; i < NV; ++i) v[i] = wtk_silu_scaled(v[i]);
        }
        const long long pix = ((long long)n * a.H + (int)y) * a.W + xs + x;
        if (res) {
#pragma unroll
            for (int i = 0; i < NV; i += 8) {
                const half8 rv = *reinterpret_cast<const half8 *>(res + pix * a.res_ld + a.res_coff + cb + i);
#pragma unroll
                for (int e = 0; e < 8; ++e) v[i + e] += (float)rv[e];
            }
        }
#pragma unroll
        for (int i = 0; i < NV; i += 8) {
            half8 h;
#pragma unroll
            for (int e = 0; e < 8; ++e) h[e] = (_Float16)v[i + e];
            *reinterpret_cast<half8 *>(out + pix * a.out_ld + a.out_coff + cb + i) = h;
        }
    }
}


// ---------------------------------------------------------------------------------------------------------------
// Split-fp16 form ("f16x3" handles, wtk_kernels.h kSplitScale): 32 -> 32 channels, a pixel is ONE 128-byte row [hi32 | lo32] and
// so is a (tap, cout) weight row.  Persistent: a block stages all nine weight slabs (36 KB) once and walks 256-pixel tiles; per
// tile the window (<= 352 rows, 44 KB) is requested in one go, then 9 taps x (12 ds_read_b128 + 24 MFMAs) per wave with no further
// waits: hi.hi in `acc`, the two 2^-11 cross terms in `acc1` (the accumulation order of conv3x3_halo_kernel's split form).
// The layer is HBM / latency bound (split rows double the bytes: 420 MB per 64 frames at 160 x 160), so the schedule is about
// keeping requests in flight: the NEXT tile's window (and its residual rows, into registers) is requested right after the
// barrier that ends the multiply phase, i.e. before this tile's SiLU + stores, and the second block of the CU (80 KB of LDS each)
// multiplies meanwhile.  Every XCD owns one contiguous run of tiles (vertical neighbours share window rows in its L2).
// Rows and swizzles are conv3x3_halo_kernel's: pixel rows key = row & 7; weight rows key = ((row >> 1) & 1) | (((row / 8) & 3) << 1)
// with the lane -> row map (lr >> 2) * 8 + (lr & 3) + 4 i, the same slot function of (lr, lg) as that kernel's 64-cout tile.
constexpr int kSplitRows = kHaloRowsSmall;        // 352 rows: 256 + 2 * pitch + 2 -> strips of <= 45 columns
constexpr int kSplitPiecesPerWave = kSplitRows / 8 / 4; // 11 LDS-DMA pieces (8 rows) per wave: a fixed count, rows behind the window read the zero page

__global__ __launch_bounds__(256, 2) void conv3x3_c32_split_kernel(const HaloArgs a) {
    constexpr int TC = 2, TP = 4, NV = 8;
    __shared__ __attribute__((aligned(16))) char win[kSplitRows * 128];
    __shared__ __attribute__((aligned(16))) char wts[9 * 32 * 128];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 15, lg = lane >> 4;

    // ---- this block's tiles: XCD x owns tiles [start, start + count), its blocks take them round-robin
    int ntiles = a.N * a.strips * a.blocks_per_strip;
    if (a.n_dyn) ntiles = min(max(*a.n_dyn, 0), a.N) * a.strips * a.blocks_per_strip; // dynamic batch: the tiles of the first *n_dyn images
    const int per = a.grid >> 3; // blocks per XCD (the launcher makes the grid a multiple of 8)
    const XcdRange xr = xcd_range(blockIdx.x, a.grid, ntiles);
    const int start = xr.first, count = xr.count;
    int t = blockIdx.x >> 3;
    if (t >= count) return; // block-uniform

    const int pitch = a.pitch;
    const int halo_rows = kBM + 2 * pitch + 2;
    const _Float16 *wgt = reinterpret_cast<const _Float16 *>(a.w);
    const char *zero_page = reinterpret_cast<const char *>(a.zeros);
    _Float16 *out = reinterpret_cast<_Float16 *>(a.out);
    const _Float16 *res = reinterpret_cast<const _Float16 *>(a.res);
    const int cb = lg * NV; // this lane's eight couts

    struct Tile {
        int n, xs, o0;
    };
    auto geometry = [&](int tile) {
        unsigned v = (unsigned)tile;
        unsigned q = fdiv(v, a.d_bps);
        Tile g;
        g.o0 = (int)(v - q * (unsigned)a.blocks_per_strip) * kBM;
        v = q;
        q = fdiv(v, a.d_strips);
        g.xs = (int)(v - q * (unsigned)a.strips) * a.S;
        g.n = (int)q;
        return g;
    };
    // NHWC pixel index of this lane's pixel in tile j of the wave's 64 outputs, -1 for the junk positions of the flat strip
    auto pixel = [&](const Tile &g, int j) -> long long {
        const unsigned o = (unsigned)(g.o0 + wave * 64 + j * 16 + lr);
        const unsigned y = fdiv(o, a.d_pitch);
        const int x = (int)(o - y * (unsigned)pitch);
        if ((int)y >= a.H || x >= a.S || g.xs + x >= a.W) return -1;
        return ((long long)g.n * a.H + (int)y) * a.W + g.xs + x;
    };
    // the window: lane -> (row = piece*8 + lane/8, physical chunk = lane%8)
    auto request_window = [&](const Tile &g) {
        const _Float16 *in = reinterpret_cast<const _Float16 *>(a.in) + (long long)g.n * a.H * a.W * a.in_ld + a.in_coff;
#pragma unroll
        for (int k = 0; k < kSplitPiecesPerWave; ++k) {
            const int piece = wave + 4 * k;
            const int hr = piece * 8 + (lane >> 3);
            const int lc = (lane & 7) ^ (hr & 7); // typed out: see wtk_device.h, operand-tile layout
            const unsigned flat = (unsigned)(g.o0 + hr);
            const unsigned r = fdiv(flat, a.d_pitch);
            const int cc = (int)(flat - r * (unsigned)pitch);
            const int iy = (int)r - 1, ix = g.xs + cc - 1;
            const bool ok = hr < halo_rows && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
            const char *src = ok ? reinterpret_cast<const char *>(in + ((long long)iy * a.W + ix) * a.in_ld + lc * 8) : zero_page;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                             (__attribute__((address_space(3))) void *)(win + piece * 1024), 16, 0, 0);
        }
    };
    // the residual rows of a tile, raw (junk positions read pixel 0): [j][0] = eight hi halves, [j][1] = their lo halves
    auto request_residual = [&](const Tile &g, half8 (&rr)[TP][2]) {
#pragma unroll
        for (int j = 0; j < TP; ++j) {
            const long long pix = pixel(g, j);
            const _Float16 *p = res + (pix < 0 ? 0 : pix) * a.res_ld + a.res_coff + cb;
            rr[j][0] = *reinterpret_cast<const half8 *>(p);
            rr[j][1] = *reinterpret_cast<const half8 *>(p + 32);
        }
    };

    // ---- all nine weight slabs, once: LDS row = tap*32 + cout (36 pieces, nine per wave)
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int piece = wave + 4 * k;
        const int row = piece * 8 + (lane >> 3);
        const int tap = row >> 5, co = row & 31;
        static_assert(layout_check::is_weight_key<NV>([](int co) { return ((co >> 1) & 1) | (((co >> 3) & 3) << 1); }), "typed-out key differs from tile_weight_key");
        const int key = ((co >> 1) & 1) | (((co >> 3) & 3) << 1); // typed out: see wtk_device.h, operand-tile layout
        const int lc = (lane & 7) ^ key;
        const char *src = reinterpret_cast<const char *>(wgt + (long long)co * a.Kpad + tap * 64 + lc * 8);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                         (__attribute__((address_space(3))) void *)(wts + piece * 1024), 16, 0, 0);
    }
    Tile cur = geometry(start + t);
    half8 rcur[TP][2];
#pragma unroll
    for (int j = 0; j < TP; ++j) rcur[j][0] = rcur[j][1] = (half8){0, 0, 0, 0, 0, 0, 0, 0};
    if (res) request_residual(cur, rcur);
    request_window(cur);

    floatx4 bias4[TC];
#pragma unroll
    for (int i = 0; i < TC; ++i) bias4[i] = (floatx4){a.bias[cb + i * 4 + 0], a.bias[cb + i * 4 + 1], a.bias[cb + i * 4 + 2], a.bias[cb + i * 4 + 3]};

    const int wrow_l = (lr >> 2) * NV + (lr & 3); // + 4*i per cout tile, + tap*32
    static_assert(layout_check::is_weight_key<NV>([](int wrow_l) { return ((wrow_l >> 1) & 1) | (((wrow_l >> 3) & 3) << 1); }), "typed-out key differs from tile_weight_key");
    const int wkey_l = ((wrow_l >> 1) & 1) | (((wrow_l >> 3) & 3) << 1); // typed out: see wtk_device.h, operand-tile layout
    const unsigned wfrag0 = wrow_l * 128 + ((lg ^ wkey_l) << 4);
    const int prow0 = wave * 64 + lr;

    for (;;) {
        floatx4 acc[TC][TP], acc1[TC][TP];
#pragma unroll
        for (int i = 0; i < TC; ++i)
#pragma unroll
            for (int j = 0; j < TP; ++j) acc[i][j] = bias4[i], acc1[i][j] = (floatx4){0.f, 0.f, 0.f, 0.f};

        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads(); // this tile's window (and, first time round, the weights) have landed

#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int base = prow0 + (tap / 3) * pitch + (tap % 3);
            const unsigned pa = tile_pixel_off(base, lg); // tiles j: + j*2048 (key unchanged); lo halves: ^ 64
            half8 ph[TP], pl[TP], wh[TC], wl[TC];
#pragma unroll
            for (int j = 0; j < TP; ++j) ph[j] = *reinterpret_cast<const half8 *>(win + pa + j * 2048);
#pragma unroll
            for (int i = 0; i < TC; ++i) wh[i] = *reinterpret_cast<const half8 *>(wts + tap * 4096 + wfrag0 + i * 512);
#pragma unroll
            for (int i = 0; i < TC; ++i) wl[i] = *reinterpret_cast<const half8 *>(wts + tap * 4096 + tile_khalf1(wfrag0) + i * 512);
#pragma unroll
            for (int j = 0; j < TP; ++j) pl[j] = *reinterpret_cast<const half8 *>(win + tile_khalf1(pa) + j * 2048);
#pragma unroll
            for (int i = 0; i < TC; ++i)
#pragma unroll
                for (int j = 0; j < TP; ++j) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[i], ph[j], acc[i][j], 0, 0, 0);
                    acc1[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[i], ph[j], acc1[i][j], 0, 0, 0);
                }
#pragma unroll
            for (int i = 0; i < TC; ++i)
#pragma unroll
                for (int j = 0; j < TP; ++j) acc1[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[i], pl[j], acc1[i][j], 0, 0, 0);
        }

        __syncthreads(); // every wave is done reading the window: the next tile's requests go out before this tile's epilogue
        t += per;
        const bool more = t < count; // block-uniform
        Tile nxt = cur;
        half8 rnext[TP][2];
#pragma unroll
        for (int j = 0; j < TP; ++j) rnext[j][0] = rcur[j][0], rnext[j][1] = rcur[j][1];
        if (more) {
            nxt = geometry(start + t);
            if (res) request_residual(nxt, rnext);
            request_window(nxt);
        }

        // ---- epilogue: lane (pixel lr of tile j, group lg) owns couts 8 lg .. 8 lg + 7 -> one 16-byte hi run and one 16-byte lo run
#pragma unroll
        for (int j = 0; j < TP; ++j) {
            const long long pix = pixel(cur, j);
            if (pix < 0) continue;
            float v[NV];
#pragma unroll
            for (int i = 0; i < TC; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) v[i * 4 + r] = wtk_split_value(acc[i][j][r], acc1[i][j][r]);
            if (a.act) wtk_silu_scaled_run<NV>(v);
            if (res) {
#pragma unroll
                for (int e = 0; e < NV; ++e) v[e] += wtk_split_value((float)rcur[j][0][e], (float)rcur[j][1][e]);
            }
            wtk_split_store<NV>(out + pix * a.out_ld + a.out_coff, cb, v);
        }
        if (!more) break;
        cur = nxt;
#pragma unroll
        for (int j = 0; j < TP; ++j) rcur[j][0] = rnext[j][0], rcur[j][1] = rnext[j][1];
    }
}

// ---------------------------------------------------------------------------------------------------------------
// The split kernel above with the C2f block's closing 1x1 (model.2.cv2: 96 -> 64 channels, SiLU) in its epilogue: the bottleneck output
// z = SiLU(conv) + y1 never reaches HBM, and y1 is fetched once.  After the epilogue's arithmetic lane (lr, lg) holds channels 8 lg .. 8 lg + 7
// of pixel lr of tile j — the B fragment of v_mfma_f32_16x16x32_f16 for a 32-channel K block — and so do the residual registers (y1) and a
// second pair of 16-byte loads 32 channels lower (y0): the 1x1's three K blocks [y0 | y1 | z] are in registers in fragment form, no pixel
// goes through LDS and no wave needs another wave's data.  Arithmetic and K order are conv_igemm_kernel's split form (per block hi.hi into
// c2, lo_w.hi then hi_w.lo into c2l, accumulators from the bias), so the result has the bits of the two launches this replaces.
// LDS: the 1x1's weights are 3 blocks x 64 couts x 128-byte rows = 24 KB, which two 80 KB blocks per CU cannot both add.  One 512-thread
// block per CU instead: two four-wave halves, each with the plain kernel's tile loop on its own 44 KB window buffer and its own tiles, and
// ONE copy of the weights (36 + 24 KB): 148 KB.  A barrier now spans both halves; every wave executes the same number of them (a half
// without a tile in the last round only keeps the count).  The halves run in lock step: with half 1 one barrier behind half 0 (one half
// multiplying while the other is in its epilogue) the pass measured the same (profiles/r23_notes.md), so the simpler form stays.
// Weight rows of the 1x1: LDS row = block * 64 + cout, key and lane -> row map of a 16-cout-per-lane tile (tile_weight_key<16>): lane (lr, lg)
// ends up with couts 16 lg .. 16 lg + 15 of its pixel.
__global__ __launch_bounds__(512) void conv3x3_c32_split_kernel_cv2(const HaloArgs a) {
    constexpr int TC = 2, TP = 4, NV = 8, TC2 = 4, NV2 = 16;
    __shared__ __attribute__((aligned(16))) char win2[2][kSplitRows * 128];
    __shared__ __attribute__((aligned(16))) char wts[9 * 32 * 128];
    __shared__ __attribute__((aligned(16))) char wts2[3 * 64 * 128];
    __shared__ __attribute__((aligned(16))) float bias2s[64];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave8 = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = wave8 >> 2, wave = wave8 & 3; // the half of the block, the wave inside it (= pixel quarter of the half's tile)
    const int lr = lane & 15, lg = lane >> 4;
    char *win = win2[half];

    // ---- this half's tiles: XCD x owns tiles [start, start + count), the halves of its blocks take them round-robin
    int ntiles = a.N * a.strips * a.blocks_per_strip;
    if (a.n_dyn) ntiles = min(max(*a.n_dyn, 0), a.N) * a.strips * a.blocks_per_strip;
    const int per = 2 * (a.grid >> 3); // halves per XCD
    const XcdRange xr = xcd_range(blockIdx.x, a.grid, ntiles);
    const int start = xr.first, count = xr.count;
    const int t0 = 2 * (int)(blockIdx.x >> 3);
    if (t0 >= count) return; // block-uniform
    const int rounds = (count - t0 + per - 1) / per; // tiles of half 0 = barrier rounds of the block (half 1 has as many or one fewer)
    int t = t0 + half;

    const int pitch = a.pitch;
    const int halo_rows = kBM + 2 * pitch + 2;
    const _Float16 *wgt = reinterpret_cast<const _Float16 *>(a.w);
    const _Float16 *wgt2 = reinterpret_cast<const _Float16 *>(a.tail_w);
    _Float16 *tout = reinterpret_cast<_Float16 *>(a.tail_out);
    const _Float16 *res = reinterpret_cast<const _Float16 *>(a.res);
    const int cb = lg * NV, cb2 = lg * NV2; // this lane's eight channels of the 3x3, its sixteen couts of the 1x1

    struct Tile {
        int n, xs, o0;
    };
    auto geometry = [&](int tile) {
        unsigned v = (unsigned)tile;
        unsigned q = fdiv(v, a.d_bps);
        Tile g;
        g.o0 = (int)(v - q * (unsigned)a.blocks_per_strip) * kBM;
        v = q;
        q = fdiv(v, a.d_strips);
        g.xs = (int)(v - q * (unsigned)a.strips) * a.S;
        g.n = (int)q;
        return g;
    };
    auto pixel = [&](const Tile &g, int j) -> long long {
        const unsigned o = (unsigned)(g.o0 + wave * 64 + j * 16 + lr);
        const unsigned y = fdiv(o, a.d_pitch);
        const int x = (int)(o - y * (unsigned)pitch);
        if ((int)y >= a.H || x >= a.S || g.xs + x >= a.W) return -1;
        return ((long long)g.n * a.H + (int)y) * a.W + g.xs + x;
    };
    // The window, in buffer form (lds_dma_buf: the resource spans the tile's image, rows outside it take the out-of-range offset and land
    // zeros).  hipcc does not see these requests, which is the point: the epilogue that follows them reads registers and the 1x1's weights
    // in LDS, and must not be made to wait for the next window.  The barrier that publishes a window is preceded by s_waitcnt vmcnt(0).
    auto request_window = [&](const Tile &g) {
        const rsrc_t rs = make_rsrc(reinterpret_cast<const _Float16 *>(a.in) + (long long)g.n * a.H * a.W * a.in_ld + a.in_coff);
#pragma unroll
        for (int k = 0; k < kSplitPiecesPerWave; ++k) {
            const int piece = wave + 4 * k;
            const int hr = piece * 8 + (lane >> 3);
            const int lc = tile_src_chunk(lane & 7, tile_pixel_key(hr));
            const unsigned flat = (unsigned)(g.o0 + hr);
            const unsigned r = fdiv(flat, a.d_pitch);
            const int cc = (int)(flat - r * (unsigned)pitch);
            const int iy = (int)r - 1, ix = g.xs + cc - 1;
            const bool ok = hr < halo_rows && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
            lds_dma_buf(rs, ok ? (unsigned)(((iy * a.W + ix) * a.in_ld + lc * 8) * 2) : 0xffffffffu, 0u, win + piece * 1024);
        }
    };
    // y0 and y1 of a tile's pixels, raw (junk positions read pixel 0): [j][0] = eight hi halves, [j][1] = their lo halves; y0 lies one
    // 32-channel block (64 pseudo-channels) below the residual y1
    auto request_y = [&](const Tile &g, half8 (&y0)[TP][2], half8 (&y1)[TP][2]) {
#pragma unroll
        for (int j = 0; j < TP; ++j) {
            const long long pix = pixel(g, j);
            const _Float16 *p = res + (pix < 0 ? 0 : pix) * a.res_ld + a.res_coff + cb;
            y0[j][0] = *reinterpret_cast<const half8 *>(p - 64);
            y0[j][1] = *reinterpret_cast<const half8 *>(p - 32);
            y1[j][0] = *reinterpret_cast<const half8 *>(p);
            y1[j][1] = *reinterpret_cast<const half8 *>(p + 32);
        }
    };

    // ---- both weight sets, once, by all eight waves: the nine 3x3 slabs (LDS row = tap*32 + cout, 36 pieces), the 1x1's three K blocks (24 pieces)
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const int piece = wave8 + 8 * k;
        if (piece < 36) {
            const int row = piece * 8 + (lane >> 3);
            const int tap = row >> 5, co = row & 31;
            const int lc = tile_src_chunk(lane & 7, tile_weight_key<NV>(co));
            lds_dma16(reinterpret_cast<const char *>(wgt + (long long)co * a.Kpad + tap * 64 + lc * 8), wts + piece * 1024);
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int piece = wave8 + 8 * k;
        const int row = piece * 8 + (lane >> 3);
        const int blk = row >> 6, co = row & 63;
        const int lc = tile_src_chunk(lane & 7, tile_weight_key<NV2>(co));
        lds_dma16(reinterpret_cast<const char *>(wgt2 + (long long)co * a.tail_kpad + blk * 64 + lc * 8), wts2 + piece * 1024);
    }
    Tile cur = geometry(start + min(t, count - 1));
    if (t < count) request_window(cur);
    if (tid < 64) bias2s[tid] = a.tail_bias[tid];

    floatx4 bias4[TC];
#pragma unroll
    for (int i = 0; i < TC; ++i) bias4[i] = (floatx4){a.bias[cb + i * 4 + 0], a.bias[cb + i * 4 + 1], a.bias[cb + i * 4 + 2], a.bias[cb + i * 4 + 3]};

    const int wrow_l = (lr >> 2) * NV + (lr & 3); // + 4*i per cout tile, + tap*32
    const unsigned wfrag0 = tile_chunk_off(wrow_l, lg, tile_weight_key<NV>(wrow_l));
    const int wrow2_l = (lr >> 2) * NV2 + (lr & 3); // + 4*i per cout tile, + block*64
    const unsigned wfrag2 = tile_chunk_off(wrow2_l, lg, tile_weight_key<NV2>(wrow2_l));
    const int prow0 = wave * 64 + lr;

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads(); // both weight sets, the 1x1's bias and both halves' first windows have landed

    for (int round = 0; round < rounds; ++round) {
        const bool active = t < count; // half-uniform; false only for half 1 in the last round
        floatx4 acc[TC][TP], acc1[TC][TP];
        half8 y0[TP][2], y1[TP][2];
        if (active) {
            request_y(cur, y0, y1); // in flight during the multiply phase
#pragma unroll
            for (int i = 0; i < TC; ++i)
#pragma unroll
                for (int j = 0; j < TP; ++j) acc[i][j] = bias4[i], acc1[i][j] = (floatx4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int base = prow0 + (tap / 3) * pitch + (tap % 3);
                const unsigned pa = tile_pixel_off(base, lg); // tiles j: + j*2048 (key unchanged); lo halves: ^ 64
                half8 ph[TP], pl[TP], wh[TC], wl[TC];
#pragma unroll
                for (int j = 0; j < TP; ++j) ph[j] = *reinterpret_cast<const half8 *>(win + pa + j * 2048);
#pragma unroll
                for (int i = 0; i < TC; ++i) wh[i] = *reinterpret_cast<const half8 *>(wts + tap * 4096 + wfrag0 + i * 512);
#pragma unroll
                for (int i = 0; i < TC; ++i) wl[i] = *reinterpret_cast<const half8 *>(wts + tap * 4096 + tile_khalf1(wfrag0) + i * 512);
#pragma unroll
                for (int j = 0; j < TP; ++j) pl[j] = *reinterpret_cast<const half8 *>(win + tile_khalf1(pa) + j * 2048);
#pragma unroll
                for (int i = 0; i < TC; ++i)
#pragma unroll
                    for (int j = 0; j < TP; ++j) {
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[i], ph[j], acc[i][j], 0, 0, 0);
                        acc1[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[i], ph[j], acc1[i][j], 0, 0, 0);
                    }
#pragma unroll
                for (int i = 0; i < TC; ++i)
#pragma unroll
                    for (int j = 0; j < TP; ++j) acc1[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[i], pl[j], acc1[i][j], 0, 0, 0);
            }
            // y0 / y1 are taken here, behind the multiply phase that hid their latency: from now on they are values in registers to hipcc, and no
            // wait for them can land behind the window requests below
#pragma unroll
            for (int j = 0; j < TP; ++j) asm volatile("" : "+v"(y0[j][0]), "+v"(y0[j][1]), "+v"(y1[j][0]), "+v"(y1[j][1]));
        }

        __syncthreads(); // this half is done reading its window: the next tile's requests go out before this tile's epilogue
        if (active) {
            t += per;
            Tile nxt = cur;
            if (t < count) { // half-uniform
                nxt = geometry(start + t);
                request_window(nxt);
            }

            // ---- epilogue, one pixel tile at a time: z in registers, then the 1x1 over [y0 | y1 | z] for the lane's 16 couts
#pragma unroll
            for (int j = 0; j < TP; ++j) {
                half8 zh, zl;
                {
                    float v[NV];
#pragma unroll
                    for (int i = 0; i < TC; ++i)
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[i * 4 + r] = wtk_split_value(acc[i][j][r], acc1[i][j][r]);
                    wtk_silu_scaled_run<NV>(v);
#pragma unroll
                    for (int e = 0; e < NV; ++e) v[e] += wtk_split_value((float)y1[j][0][e], (float)y1[j][1][e]);
                    split_pack8(v, zh, zl); // what wtk_split_store would have written and the 1x1 read back
                }
                floatx4 c2[TC2], c2l[TC2];
#pragma unroll
                for (int i = 0; i < TC2; ++i) c2[i] = *reinterpret_cast<const floatx4 *>(bias2s + cb2 + i * 4), c2l[i] = (floatx4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int blk = 0; blk < 3; ++blk) { // K order of the concat: y0, y1, z
                    const half8 ph = blk == 0 ? y0[j][0] : blk == 1 ? y1[j][0] : zh;
                    const half8 pl = blk == 0 ? y0[j][1] : blk == 1 ? y1[j][1] : zl;
#pragma unroll
                    for (int i = 0; i < TC2; ++i) {
                        const half8 wh = *reinterpret_cast<const half8 *>(wts2 + blk * 8192 + wfrag2 + i * 512);
                        const half8 wl = *reinterpret_cast<const half8 *>(wts2 + blk * 8192 + tile_khalf1(wfrag2) + i * 512);
                        c2[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, ph, c2[i], 0, 0, 0);
                        c2l[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl, ph, c2l[i], 0, 0, 0);
                        c2l[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, pl, c2l[i], 0, 0, 0);
                    }
                }
                const long long pix = pixel(cur, j);
                if (pix >= 0) {
                    float v2[NV2];
#pragma unroll
                    for (int i = 0; i < TC2; ++i)
#pragma unroll
                        for (int r = 0; r < 4; ++r) v2[i * 4 + r] = wtk_split_value(c2[i][r], c2l[i][r]);
                    wtk_silu_scaled_run<NV2>(v2);
                    wtk_split_store<NV2>(tout + pix * a.tail_ld + a.tail_coff, cb2, v2);
                }
            }
            cur = nxt;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads(); // the next tile's window has landed
    }
}

} // namespace

bool c32_eligible(int k, int stride, int cin, int cout_stored, int is_f16, bool has_out2) {
    return is_f16 && k == 3 && stride == 1 && cin == 32 && cout_stored % 8 == 0 && cout_stored <= 96 && !has_out2;
}

hipError_t launch_conv3x3_c32(HaloArgs a, hipStream_t stream) {
    if (a.Cin != 32 || a.Cout % 8 != 0 || a.Cout > a.CoutPad || a.CoutPad % 32 != 0 || a.CoutPad > 96 || a.out2) return hipErrorInvalidValue;
    if (a.in_ld % 8 || a.in_coff % 8 || a.out_ld % 8 || a.out_coff % 8 || a.Kpad < 9 * 32) return hipErrorInvalidValue;
    if (a.pitch != a.S + 2 || kBM + 2 * a.pitch + 2 > kRowsMax || a.strips * a.S < a.W) return hipErrorInvalidValue;
    if (a.blocks_per_strip * kBM < a.H * a.pitch) return hipErrorInvalidValue;
    if (a.res && (a.res_ld % 8 || a.res_coff % 8)) return hipErrorInvalidValue;
    const long long blocks = (long long)a.N * a.strips * a.blocks_per_strip;
    if (blocks <= 0 || blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    a.d_bps = make_fastdiv((unsigned)a.blocks_per_strip);
    a.d_strips = make_fastdiv((unsigned)a.strips);
    a.d_pitch = make_fastdiv((unsigned)a.pitch);
    switch (a.CoutPad) {
    case 32: hipLaunchKernelGGL((conv3x3_c32_kernel<32>), dim3((unsigned)blocks), dim3(256), 0, stream, a); break;
    case 64: hipLaunchKernelGGL((conv3x3_c32_kernel<64>), dim3((unsigned)blocks), dim3(256), 0, stream, a); break;
    default: hipLaunchKernelGGL((conv3x3_c32_kernel<96>), dim3((unsigned)blocks), dim3(256), 0, stream, a); break;
    }
    return hipGetLastError();
}

// split-fp16 operands: real channel counts here (the arguments of launch_conv3x3_c32_split are in pseudo-channels but Cout / CoutPad)
bool c32_split_eligible(int k, int stride, int cin, int cout, bool plain_out) { return k == 3 && stride == 1 && cin == 32 && cout == 32 && plain_out; }
int c32_split_rows_max() { return kSplitRows; }

hipError_t launch_conv3x3_c32_split(HaloArgs a, hipStream_t stream) {
    if (a.Cin != 64 || a.Cout != 32 || a.CoutPad != 32 || a.out2 || a.Kpad != 9 * 64) return hipErrorInvalidValue;
    if (a.in_ld % 64 || a.in_coff % 64 || a.out_ld % 64 || a.out_coff % 64) return hipErrorInvalidValue;
    // fused 1x1 (conv3x3_c32_split_kernel_cv2): 96 -> 64 channels with SiLU over [y0 | y1 | z], y1 = the residual, y0 the 32 channels below it, split output
    if (a.tail_w && 2LL * a.H * a.W * a.in_ld >= 0x7fffffffLL) return hipErrorInvalidValue; // that kernel addresses an image's window rows by 32-bit byte offsets
    if (a.tail_w && (!a.res || a.res_coff < 64 || !a.act || a.tail_kpad != 3 * 64 || a.tail_cout != 64 || a.tail_f32 || a.tail_ld % 64 || a.tail_coff % 64)) return hipErrorInvalidValue;
    if (a.res && (a.res_ld % 64 || a.res_coff % 64)) return hipErrorInvalidValue;
    if (a.pitch != a.S + 2 || kBM + 2 * a.pitch + 2 > kSplitRows || a.strips * a.S < a.W) return hipErrorInvalidValue;
    if (a.blocks_per_strip * kBM < a.H * a.pitch) return hipErrorInvalidValue;
    const long long tiles = (long long)a.N * a.strips * a.blocks_per_strip;
    if (tiles <= 0 || tiles > 0x7fffffffLL) return hipErrorInvalidValue;
    a.d_bps = make_fastdiv((unsigned)a.blocks_per_strip);
    a.d_strips = make_fastdiv((unsigned)a.strips);
    a.d_pitch = make_fastdiv((unsigned)a.pitch);
    // two persistent blocks per CU (80 KB of LDS each), a multiple of 8 so that every XCD gets the same number of them
    const long long cus = a.persist_cus > 0 ? a.persist_cus : 256;
    if (a.tail_w) { // one 512-thread block per CU (148 KB of LDS), each half of a block a tile walker
        const long long blocks2 = std::max(8LL, std::min(cus, ((tiles + 1) / 2 + 7) / 8 * 8) / 8 * 8);
        a.grid = (int)blocks2;
        hipLaunchKernelGGL(conv3x3_c32_split_kernel_cv2, dim3((unsigned)blocks2), dim3(512), 0, stream, a);
        return hipGetLastError();
    }
    long long blocks = std::min(2 * cus, (tiles + 7) / 8 * 8);
    blocks = std::max(8LL, blocks / 8 * 8);
    a.grid = (int)blocks;
    hipLaunchKernelGGL(conv3x3_c32_split_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, a);
    return hipGetLastError();
}

} // namespace wtk
