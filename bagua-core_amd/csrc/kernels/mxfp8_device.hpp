// mxfp8_device.hpp — the format-specific steps of the MXFP8 kernels (mxfp8.hip).  The
// format-independent ones (mx_load_tile, mx_block_amax, the host checks, mx_grid) are
// mxfp4_device.hpp's, as they stand.
//   device  mx8_decode          payload bytes -> values as T stores them, either conversion
//           mx8_quant_lane / mx8_encode_lane   a lane's part of a cooperative block encode
//           mx8_store_lane / mx8_store_block / mx8_zero_slack   a block's result into its segment
//           mx8_encode_whole    a whole block held by one lane
//           mx8_reduce_block    decode and tree-sum of one block of p received segments
//   host    mx8_hw, mx8_holds
// Arithmetic of one block: mxfp8_common.hpp.
#pragma once

#include <cstdint>

#include "mxfp4_device.hpp"
#include "mxfp8_common.hpp"

namespace bagua {

typedef short mx8_s16x2 __attribute__((ext_vector_type(2)));
typedef float mx8_f32x2 __attribute__((ext_vector_type(2)));

// true if one of the four bytes of w has magnitude 0x7F: 0x7F + 1 carries into bit 7, no
// smaller magnitude does, and no carry leaves its byte
__device__ __forceinline__ bool mx8_has_nan_code(uint32_t w) {
    return (((w & 0x7f7f7f7fu) + 0x01010101u) & 0x80808080u) != 0u;
}

// NB payload bytes (NB / 4 words, low byte first) of a block with scale byte sb -> NB values
// as T stores them (bits; 16-bit patterns zero-extended)
template <typename T, bool HW, int NB>
__device__ __forceinline__ void mx8_decode(const uint32_t (&w)[NB / 4], uint32_t sb, uint32_t (&u)[NB]) {
    if (sb == kMxNanScale) {
#pragma unroll
        for (int e = 0; e < NB; ++e) u[e] = mx_nan_bits<T>();
        return;
    }
    const float maxf = T::init_max();
    if constexpr (HW) {
        const float scale = __uint_as_float(sb << 23);  // the conversion reads its exponent: 2^(sb - 127)
#pragma unroll
        for (int k = 0; k < NB / 4; ++k) {
            const mx8_f32x2 lo = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w[k], scale, false);
            const mx8_f32x2 hi = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w[k], scale, true);
            u[4 * k] = stored_bits<T>(mx_clamp(lo.x, maxf));
            u[4 * k + 1] = stored_bits<T>(mx_clamp(lo.y, maxf));
            u[4 * k + 2] = stored_bits<T>(mx_clamp(hi.x, maxf));
            u[4 * k + 3] = stored_bits<T>(mx_clamp(hi.y, maxf));
        }
    } else {
        const float sc = mx8_scale(sb);
#pragma unroll
        for (int e = 0; e < NB; ++e) u[e] = stored_bits<T>(mx8_dequant((w[e / 4] >> (8 * (e % 4))) & 0xffu, sc, maxf));
    }
    // magnitude 0x7F (no encoder writes it): the canonical NaN for that element
#pragma unroll
    for (int k = 0; k < NB / 4; ++k)
        if (__builtin_expect(mx8_has_nan_code(w[k]), 0)) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (((w[k] >> (8 * e)) & 0x7fu) == kMx8NanCode) u[4 * k + e] = mx_nan_bits<T>();
        }
}

// ------------------------------------------------------------------------
// encode
// ------------------------------------------------------------------------
// the N (a multiple of 4) payload bytes of N values (f32, not yet clamped) of a block without
// NaN under the block's scale byte, element e in byte e % 4 of word e / 4.  HW: gfx950's
// v_cvt_scalef32_pk_fp8_f32, two elements into one half of the word per instruction.
template <int N, bool HW>
__device__ __forceinline__ void mx8_quant_lane(const float* f, uint32_t byte, float maxf, uint32_t (&w)[N / 4]) {
    if constexpr (HW) {
        const float scale = __uint_as_float(byte << 23);
#pragma unroll
        for (int k = 0; k < N / 4; ++k) {
            mx8_s16x2 v = {0, 0};
            v = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(v, mx_clamp(f[4 * k], maxf), mx_clamp(f[4 * k + 1], maxf), scale,
                                                         false);
            v = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(v, mx_clamp(f[4 * k + 2], maxf), mx_clamp(f[4 * k + 3], maxf),
                                                         scale, true);
            w[k] = __builtin_bit_cast(uint32_t, v);
        }
    } else {
        const float inv = mx8_inv_scale(byte);
#pragma unroll
        for (int k = 0; k < N / 4; ++k) {
            w[k] = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) w[k] |= mx8_quant(mx_clamp(f[4 * k + e], maxf), inv) << (8 * e);
        }
    }
}

// The lane's part of a cooperative block encode after mx_block_amax: from the block's amax its
// scale byte and the lane's payload words; a NaN block: 0xFF and zero words.
template <int N, bool HW>
__device__ __forceinline__ void mx8_encode_lane(const float (&f)[N], uint32_t am, float maxf, uint32_t& byte,
                                                uint32_t (&w)[N / 4]) {
    byte = kMxNanScale;
#pragma unroll
    for (int k = 0; k < N / 4; ++k) w[k] = 0;
    if (am <= 0x7f800000u) {
        byte = mx8_scale_byte(min(am, __float_as_uint(maxf)));
        mx8_quant_lane<N, HW>(f, byte, maxf, w);
    }
}

// scale byte and payload words of one whole block held by one lane (x: f32, invalid elements +0)
template <bool HW>
__device__ __forceinline__ void mx8_encode_whole(const float (&x)[kMxBlock], float maxf, uint32_t& byte,
                                                 uint32_t (&w)[8]) {
    if constexpr (!HW) {
        mx8_encode_block(x, maxf, byte, w);
    } else {
        uint32_t am = 0;
#pragma unroll
        for (int e = 0; e < kMxBlock; ++e) am = max(am, __float_as_uint(x[e]) & 0x7fffffffu);
        mx8_encode_lane<kMxBlock, true>(x, am, maxf, byte, w);
    }
}

// The slack of a segment's scale bytes (the payload has none: 32 bytes per block), zeroed by
// whoever writes block nb - 1 of a range that ends its chunk (last).  seg points at the scale
// byte of block bb of the chunk, b and nb count from there; sbytes is the whole region's.
__device__ __forceinline__ void mx8_zero_slack(uint8_t* seg, int64_t b, int64_t nb, int64_t bb, bool last,
                                               int64_t sbytes) {
    if (last && b == nb - 1)
        for (int64_t q = nb; q < sbytes - bb; ++q) seg[q] = 0;
}

// Block b's result of a cooperative encode: the lane's N bytes at its place `sub` in the
// block as one 4-B / 8-B store (a wave row writes 256 / 512 contiguous bytes), and from
// sub-lane 0 the scale byte and the slack.  Plain stores, as MXFP4's.
template <int N>
__device__ __forceinline__ void mx8_store_lane(uint8_t* seg, uint8_t* pay, int64_t b, int sub, uint32_t byte,
                                               const uint32_t (&w)[N / 4], int64_t nb, int64_t bb, bool last,
                                               int64_t sbytes) {
    if constexpr (N == 4) reinterpret_cast<uint32_t*>(pay + b * kMx8BlockBytes)[sub] = w[0];
    else reinterpret_cast<uint2*>(pay + b * kMx8BlockBytes)[sub] = make_uint2(w[0], w[1]);
    if (sub == 0) {
        seg[b] = (uint8_t)byte;
        mx8_zero_slack(seg, b, nb, bb, last, sbytes);
    }
}

// its whole-block sibling (one lane encoded block b of a whole chunk's nb)
__device__ __forceinline__ void mx8_store_block(uint8_t* seg, uint8_t* pay, int64_t b, uint32_t byte,
                                                const uint32_t (&w)[8], int64_t nb, int64_t sbytes) {
    seg[b] = (uint8_t)byte;
    uint4* q = reinterpret_cast<uint4*>(pay + b * kMx8BlockBytes);
    q[0] = make_uint4(w[0], w[1], w[2], w[3]);
    q[1] = make_uint4(w[4], w[5], w[6], w[7]);
    mx8_zero_slack(seg, b, nb, 0, true, sbytes);
}

// ------------------------------------------------------------------------
// Block b of the p segments at `in` (segb bytes apart, sbytes of them scale bytes) decoded,
// summed as bagua_reduce_chunks does (s[y] = 0 + c[y] + c[y + BY], folded s[y] += s[y + h]),
// divided by pf = p if average, and rounded to T: x, as f32; padding past cs stays +0, as
// the encoder sees it.  p <= 2 * BY.  W elements of every segment at a time: sixteen (one 16-B
// payload load) for BY = 2 and 4, eight (one 8-B load) for BY = 8, whose W * BY partial sums would
// otherwise fill the register file and leave one wave per SIMD.
// ------------------------------------------------------------------------
template <typename T, int BY, bool HW>
__device__ __forceinline__ void mx8_reduce_block(const uint8_t* in, int64_t segb, int64_t sbytes, int64_t b, int p,
                                                 int average, float pf, int64_t cs, float (&x)[kMxBlock]) {
    constexpr int W = BY <= 4 ? 16 : 8;
#pragma unroll
    for (int q = 0; q < kMxBlock / W; ++q) {
        float s[W][BY];
#pragma unroll
        for (int e = 0; e < W; ++e)
#pragma unroll
            for (int y = 0; y < BY; ++y) s[e][y] = 0.0f;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            uint32_t w[BY][W / 4], sb[BY];
#pragma unroll
            for (int y = 0; y < BY; ++y) {
                const int cc = r * BY + y < p ? r * BY + y : p - 1;
                const uint8_t* seg = in + (int64_t)cc * segb;
                sb[y] = seg[b];
                if constexpr (W == 16) {
                    const uint4 v = reinterpret_cast<const uint4*>(seg + sbytes + b * kMx8BlockBytes)[q];
                    w[y][0] = v.x, w[y][1] = v.y, w[y][2] = v.z, w[y][3] = v.w;
                } else {
                    const uint2 v = reinterpret_cast<const uint2*>(seg + sbytes + b * kMx8BlockBytes)[q];
                    w[y][0] = v.x, w[y][1] = v.y;
                }
            }
#pragma unroll
            for (int y = 0; y < BY; ++y) {
                if (r * BY + y >= p) break;
                uint32_t u[W];
                mx8_decode<T, HW, W>(w[y], sb[y], u);
#pragma unroll
                for (int e = 0; e < W; ++e) s[e][y] = s[e][y] + from_stored_bits<T>(u[e]);
            }
        }
#pragma unroll
        for (int e = 0; e < W; ++e) {
            tree_finish<BY>(s[e]);
            const int64_t j = b * kMxBlock + q * W + e;
            x[q * W + e] = j < cs ? as_stored<T>(average ? s[e][0] / pf : s[e][0]) : 0.0f;
        }
    }
}

// ------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------
// a buffer that holds p segments of chunks of cs elements
static inline bool mx8_holds(size_t bytes, int cs, int p) { return bytes >= (size_t)p * (size_t)mx8_segment_bytes(cs); }

// BAGUA_MXFP8_HWCVT=1 (the default) / 0: the hardware conversions or the arithmetic (A/B; same bytes)
inline bool mx8_hw() { return tune_int("BAGUA_MXFP8_HWCVT", 1) != 0; }

}  // namespace bagua
