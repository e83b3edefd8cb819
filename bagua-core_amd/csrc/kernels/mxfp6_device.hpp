// mxfp6_device.hpp — the format-specific steps of the MXFP6 kernels (mxfp6.hip).  The
// format-independent ones (mx_load_tile, mx_block_amax, the host checks, mx_grid) are
// mxfp4_device.hpp's, as they stand.
//   device  mx6_quad            a value from another lane of the lane's group of four (DPP)
//           mx6_decode          packed codes -> values as T stores them
//           mx6_encode_lane     a lane's part of a cooperative block encode: its 24 / 48 code bits
//           mx6_store_lane      those bits of four lanes as three aligned words, the scale byte
//           mx6_field           a lane's 24 / 48 code bits out of the aligned words that cover them
//           mx6_store_block / mx6_zero_slack   a whole block's result, a segment's slack
//           mx6_reduce_block    decode and tree-sum of one block of p received segments
//   host    mx6_holds
// A block's 32 six-bit codes are 24 bytes, so a lane's share (3 or 6 bytes) is no aligned
// word; four neighbouring lanes' shares (12 or 24 bytes) are three.  Arithmetic of one block:
// mxfp6_common.hpp.
#pragma once

#include <cstdint>

#include "mxfp4_device.hpp"
#include "mxfp6_common.hpp"

namespace bagua {

// the aligned word of the cooperative kernels: N = 4 elements per lane (f32) pack into 24 bits,
// three 4-B words per four lanes; N = 8 (16-bit T) into 48 bits, three 8-B words
template <int N>
struct Mx6Word {
    using type = uint32_t;
};
template <>
struct Mx6Word<8> {
    using type = uint64_t;
};

// v of lane 4 * (lane / 4) + ((CTRL >> 2 * (lane % 4)) & 3): one v_mov_b32 with a quad_perm per
// 32 bits, no LDS.  All four lanes of the group must be active.
template <int CTRL>
__device__ __forceinline__ uint32_t mx6_quad(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, false);
}
template <int CTRL>
__device__ __forceinline__ uint64_t mx6_quad(uint64_t v) {
    return (uint64_t)mx6_quad<CTRL>((uint32_t)v) | ((uint64_t)mx6_quad<CTRL>((uint32_t)(v >> 32)) << 32);
}
constexpr int kMx6QuadNext = 0xF9;  // [1, 2, 3, 3]: the right neighbour's value

// NE codes from bit `bit0` of the words w of a block with scale byte sb -> NE values as T
// stores them (bits; 16-bit patterns zero-extended)
template <typename T, int NE, int NW>
__device__ __forceinline__ void mx6_decode(const uint32_t (&w)[NW], int bit0, uint32_t sb, uint32_t (&u)[NE]) {
    if (sb == kMxNanScale) {
#pragma unroll
        for (int e = 0; e < NE; ++e) u[e] = mx_nan_bits<T>();
        return;
    }
    const float maxf = T::init_max(), sc = mx6_scale(sb);
#pragma unroll
    for (int e = 0; e < NE; ++e) u[e] = stored_bits<T>(mx6_dequant(mx6_code_at(w, bit0 + 6 * e), sc, maxf));
}

// ------------------------------------------------------------------------
// encode
// ------------------------------------------------------------------------
// The lane's part of a cooperative block encode after mx_block_amax: from the block's amax its
// scale byte and the lane's N codes, code e in bits [6 e, 6 e + 6) of c; a NaN block: 0xFF and
// zero codes.
template <int N>
__device__ __forceinline__ void mx6_encode_lane(const float (&f)[N], uint32_t am, float maxf, uint32_t& byte,
                                                uint32_t (&c)[N / 4]) {
    byte = kMxNanScale;
#pragma unroll
    for (int k = 0; k < N / 4; ++k) c[k] = 0;
    if (am <= 0x7f800000u) {
        byte = mx6_scale_byte(min(am, __float_as_uint(maxf)));
        const float inv = mx6_inv_scale(byte);
#pragma unroll
        for (int e = 0; e < N; ++e) mx6_put_code(c, 6 * e, mx6_quant(mx_clamp(f[e], maxf), inv));
    }
}

// The slack of both regions of a segment, zeroed by whoever writes block nb - 1 of a range
// that ends its chunk (last): the scale bytes past the last block and the 0, 8, 16 or 24
// payload bytes past 24 nb, as 8-B words.  seg and pay point at the scale byte and the payload
// of block bb of the chunk, b and nb count from there; sbytes / pbytes are the whole regions'.
__device__ __forceinline__ void mx6_zero_slack(uint8_t* seg, uint8_t* pay, int64_t b, int64_t nb, int64_t bb, bool last,
                                               int64_t sbytes, int64_t pbytes) {
    if (last && b == nb - 1) {
        for (int64_t q = nb; q < sbytes - bb; ++q) seg[q] = 0;
        for (int64_t q = nb * kMx6BlockBytes; q < pbytes - bb * kMx6BlockBytes; q += 8)
            *reinterpret_cast<uint2*>(pay + q) = make_uint2(0u, 0u);
    }
}

// Block b's result of a cooperative encode.  Lane s of a group of four holds the field c_s of
// F = 24 / 48 bits; the group's 4 F bits are three words of 4 F / 3 = 32 / 64 bits, word s =
// c_s >> (F / 3) s | c_(s + 1) << (F - (F / 3) s).  Lane s < 3 takes c_(s + 1) by one quad move,
// assembles word s and stores it: a wave row writes 192 / 384 contiguous bytes, no byte twice.
// Sub-lane 0 adds the scale byte and the slack.  Plain stores, as MXFP4's.  The lanes of a
// block are whole groups, so callers that drop blocks past the range keep groups whole.
template <int N>
__device__ __forceinline__ void mx6_store_lane(uint8_t* seg, uint8_t* pay, int64_t b, int sub, uint32_t byte,
                                               const uint32_t (&c)[N / 4], int64_t nb, int64_t bb, bool last,
                                               int64_t sbytes, int64_t pbytes) {
    using W = typename Mx6Word<N>::type;
    constexpr int BW = 8 * (int)sizeof(W);
    W mine = c[0];
    if constexpr (N == 8) mine |= (W)c[1] << 32;
    const W next = mx6_quad<kMx6QuadNext>(mine);
    const int s = sub & 3;
    const W w = (mine >> (s * (BW / 4))) | (next << ((3 - s) * (BW / 4)));
    if (s < 3) reinterpret_cast<W*>(pay + b * kMx6BlockBytes)[(sub >> 2) * 3 + s] = w;
    if (sub == 0) {
        seg[b] = (uint8_t)byte;
        mx6_zero_slack(seg, pay, b, nb, bb, last, sbytes, pbytes);
    }
}

// its whole-block sibling (one lane encoded block b of a whole chunk's nb): 24 B as three 8-B words
__device__ __forceinline__ void mx6_store_block(uint8_t* seg, uint8_t* pay, int64_t b, uint32_t byte,
                                                const uint32_t (&w)[kMx6BlockWords], int64_t nb, int64_t sbytes,
                                                int64_t pbytes) {
    seg[b] = (uint8_t)byte;
    uint2* q = reinterpret_cast<uint2*>(pay + b * kMx6BlockBytes);
    q[0] = make_uint2(w[0], w[1]);
    q[1] = make_uint2(w[2], w[3]);
    q[2] = make_uint2(w[4], w[5]);
    mx6_zero_slack(seg, pay, b, nb, 0, true, sbytes, pbytes);
}

// ------------------------------------------------------------------------
// decode
// ------------------------------------------------------------------------
// The field of lane s of a group of four out of the group's three words: it starts in word
// lo = 3 s / 4 at bit (3 BW / 4) s mod BW and, for s = 1 and 2, ends in word hi = lo + 1 (for s = 0
// and 3 hi is shifted past the field's bits or out, whatever it holds).
template <typename W>
__device__ __forceinline__ W mx6_field(W lo, W hi, int s) {
    constexpr int BW = 8 * (int)sizeof(W);
    const int sh = (s * 3 * (BW / 4)) % BW;
    return (lo >> sh) | ((hi << 1) << (BW - 1 - sh));
}

// ------------------------------------------------------------------------
// Block b of the p segments at `in` (segb bytes apart, sbytes of them scale bytes) decoded,
// summed as bagua_reduce_chunks does (s[y] = 0 + c[y] + c[y + BY], folded s[y] += s[y + h]),
// divided by pf = p if average, and rounded to T: x, as f32; padding past cs stays +0, as
// the encoder sees it.  p <= 2 * BY.  W elements of every segment at a time, from the aligned
// 4-B words that cover their 6 W bits: sixteen (96 bits, three words, none read twice) for
// BY = 2 and 4; eight (48 bits in two words, the words at bytes 4 and 16 read by two groups)
// for BY = 8, whose W * BY partial sums would otherwise leave one wave per SIMD (as MXFP8's).
// ------------------------------------------------------------------------
template <typename T, int BY>
__device__ __forceinline__ void mx6_reduce_block(const uint8_t* in, int64_t segb, int64_t sbytes, int64_t b, int p,
                                                 int average, float pf, int64_t cs, float (&x)[kMxBlock]) {
    constexpr int W = BY <= 4 ? 16 : 8;
    constexpr int NW = W == 16 ? 3 : 2;
#pragma unroll
    for (int q = 0; q < kMxBlock / W; ++q) {
        const int word0 = q * W * 6 / 32, bit0 = q * W * 6 % 32;
        float s[W][BY];
#pragma unroll
        for (int e = 0; e < W; ++e)
#pragma unroll
            for (int y = 0; y < BY; ++y) s[e][y] = 0.0f;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            uint32_t w[BY][NW], sb[BY];
#pragma unroll
            for (int y = 0; y < BY; ++y) {
                const int cc = r * BY + y < p ? r * BY + y : p - 1;
                const uint8_t* seg = in + (int64_t)cc * segb;
                sb[y] = seg[b];
                const uint32_t* pw = reinterpret_cast<const uint32_t*>(seg + sbytes + b * kMx6BlockBytes) + word0;
#pragma unroll
                for (int h = 0; h < NW; ++h) w[y][h] = pw[h];
            }
#pragma unroll
            for (int y = 0; y < BY; ++y) {
                if (r * BY + y >= p) break;
                uint32_t u[W];
                mx6_decode<T, W>(w[y], bit0, sb[y], u);
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
static inline bool mx6_holds(size_t bytes, int cs, int p) { return bytes >= (size_t)p * (size_t)mx6_segment_bytes(cs); }

}  // namespace bagua
