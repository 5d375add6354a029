// Stacked flat window geometry shared by the 3x3 window kernels (conv3x3_halo.hip, conv3x3_ws64.hip, conv3x3_s2.hip): the header
// comment of conv3x3_halo.hip describes it.
#pragma once
#include "wtk_device.h"

namespace wtk {

constexpr int kBM = 256; // flat output pixels of a full-size block

// Stacked geometry (header comment).  Window row `flat` (relative to the strip) -> input pixel: stacked row rho = flat / pitch
// holds image n = rho / (H+1), input row iy = rho % (H+1) - 1 (-1: the shared zero row); column ix = xs + flat % pitch - 1.
__device__ __forceinline__ bool halo_in_coords(const HaloArgs &a, int flat, int xs, int &n, int &iy, int &ix) {
    const int rho = (int)fdiv((unsigned)flat, a.d_pitch);
    const int cc = flat - rho * a.pitch;
    n = (int)fdiv((unsigned)rho, a.d_h1);
    iy = rho - n * (a.H + 1) - 1;
    ix = xs + cc - 1;
    return n < a.N && iy >= 0 && (unsigned)ix < (unsigned)a.W;
}
// Flat output index -> (image, row, column inside the strip); false for the junk row / junk columns / past the last image
__device__ __forceinline__ bool halo_out_coords(const HaloArgs &a, int o, int xs, int &n, int &y, int &x) {
    const int q = (int)fdiv((unsigned)o, a.d_pitch);
    x = o - q * a.pitch;
    n = (int)fdiv((unsigned)q, a.d_h1);
    y = q - n * (a.H + 1);
    return n < a.N && y < a.H && x < a.S && xs + x < a.W;
}

// Per-lane byte offsets of a wave's window pieces (wave w stages pieces w, w+8, ...: 8 rows x 8 chunks of 16 B each).  The 8 x KMAX
// rows of a wave are evaluated ONCE — lane L works out row L&7 of piece L>>3 — and handed to the lanes that need them with
// ds_bpermute, instead of every lane redoing the divisions for each of its pieces: the ~250 VALU instructions this took per
// block sat in front of the block's first LDS-DMA request (stamped: 0.5 us of a 10-18 us block).
template <typename T, int KMAX>
__device__ __forceinline__ void halo_piece_offsets(const HaloArgs &a, int o0, int xs, int n_base, int halo_rows, int wave, int lane, unsigned (&hoff)[KMAX],
                                                   unsigned &hvalid) {
    static_assert(KMAX <= 8, "one lane per (piece, row)");
    constexpr int CE = Elem<T>::CE;
    const int hr_e = (wave + 8 * (lane >> 3)) * 8 + (lane & 7);
    int pn, iy, ix;
    const bool ok_e = halo_in_coords(a, o0 + hr_e, xs, pn, iy, ix) && hr_e < halo_rows;
    const unsigned row_e = ok_e ? (unsigned)(((((long long)(pn - n_base) * a.H + iy) * a.W + ix) * a.in_ld) * (long long)sizeof(T)) : 0xffffffffu;
    const unsigned lc_term = (unsigned)((((lane & 7) ^ ((lane >> 3) & 7)) * CE) * (int)sizeof(T)); // logical chunk landing on this lane's slot
    hvalid = 0;
#pragma unroll
    for (int q = 0; q < KMAX; ++q) {
        const unsigned v = (unsigned)__builtin_amdgcn_ds_bpermute((q * 8 + (lane >> 3)) * 4, (int)row_e);
        const bool ok = v != 0xffffffffu;
        hoff[q] = ok ? v + lc_term : 0u;
        hvalid |= ok ? (1u << q) : 0u;
    }
}
// Output pixel of a wave's flat outputs o_first + L (L < 64), evaluated once per lane: pixel index (n*H + y)*W + xs + x, or -1 for
// junk rows / columns; `col` = xs + x.  The lanes of pixel tile j fetch theirs with ds_bpermute from lane j*16 + (lane & 15).
__device__ __forceinline__ void halo_out_pixel(const HaloArgs &a, int o_first, int xs, int lane, int &pix_e, int &col_e) {
    int n, y, x;
    const bool ok = halo_out_coords(a, o_first + lane, xs, n, y, x);
    col_e = xs + x;
    pix_e = ok ? (n * a.H + y) * a.W + col_e : -1;
}
__device__ __forceinline__ int lane_fetch(int src_lane, int v) { return __builtin_amdgcn_ds_bpermute(src_lane * 4, v); }

} // namespace wtk
