// mxfp4_device.hpp — the steps the MXFP4 kernel files (mxfp4.hip, mxfp4_ring.hip) are composed
// of, each stated once, and what their launchers share.
//   device  mx_decode          payload bytes -> values as T stores them, either conversion
//           mx_block_amax, mx_encode_lane   a lane's part of a cooperative block encode
//           mx_store_lane / mx_store_block / mx_zero_slack   a block's result into its segment
//           mx_load_tile / mx_store_row                       a wave tile of one tensor, f32 state back
//           mx_reduce_block    decode and tree-sum of one block of p received segments
//           mx_add_residual    a whole block's f32 residual onto its values
//   host    the argument checks of the entries; the two launch knobs (run-time value ->
//           template argument: with_dtype / with_bool / with_by, codec_common.hpp)
// Arithmetic of one block: mxfp4_common.hpp.
#pragma once

#include <climits>
#include <cstdint>
#include <type_traits>

#include "codec_common.hpp"
#include "launch_util.hpp"
#include "mxfp4_common.hpp"

namespace bagua {

template <typename T>
__device__ __forceinline__ uint32_t mx_nan_bits() {  // canonical quiet NaN of T
    if constexpr (sizeof(typename T::storage) == 4) return 0x7fc00000u;
    else if constexpr (T::kDtype == BAGUA_DTYPE_F16) return 0x7e00u;
    else return 0x7fc0u;
}

// NB payload bytes (word w, low byte first) of a block with scale byte sb -> 2 * NB values
// as T stores them (bits; 16-bit patterns zero-extended)
template <typename T, bool HW, int NB>
__device__ __forceinline__ void mx_decode(uint32_t w, uint32_t sb, uint32_t (&u)[2 * NB]) {
    if (sb == kMxNanScale) {
#pragma unroll
        for (int e = 0; e < 2 * NB; ++e) u[e] = mx_nan_bits<T>();
        return;
    }
    const float maxf = T::init_max();
    if constexpr (HW) {
        typedef float f32x2v __attribute__((ext_vector_type(2)));
        const float scale = __uint_as_float(sb << 23);
        f32x2v r[NB];
        r[0] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, scale, 0);
        if constexpr (NB > 1) r[1] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, scale, 1);
        if constexpr (NB > 2) r[2] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, scale, 2);
        if constexpr (NB > 3) r[3] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, scale, 3);
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            u[2 * k] = stored_bits<T>(mx_clamp(r[k].x, maxf));
            u[2 * k + 1] = stored_bits<T>(mx_clamp(r[k].y, maxf));
        }
    } else {
        const float hs = mx_half_scale(sb);
#pragma unroll
        for (int e = 0; e < 2 * NB; ++e) u[e] = stored_bits<T>(mx_dequant((w >> (4 * e)) & 15u, hs, maxf));
    }
}

// ------------------------------------------------------------------------
// encode
// ------------------------------------------------------------------------
// the rounding of an element to E2M1: mx_quant, gfx950's v_cvt_scalef32_pk_fp4_f32, or mx_quant_sr
enum MxRound { kMxArith, kMxHw, kMxSr };
constexpr MxRound mx_round(bool hw, bool sr = false) { return sr ? kMxSr : hw ? kMxHw : kMxArith; }

// the N (4 or 8) payload nibbles of N values (f32, not yet clamped) of a block without NaN
// under the block's scale byte, element e in bits 4e .. 4e + 3.  kMxSr: j0 is the index of
// f[0] in the whole tensor, k0 / k1 the halves of the key (unused otherwise).
template <int N, MxRound RND>
__device__ __forceinline__ uint32_t mx_quant_lane(const float* f, uint32_t byte, float maxf, uint32_t j0 = 0,
                                                  uint32_t k0 = 0, uint32_t k1 = 0) {
    uint32_t w = 0;
    if constexpr (RND == kMxHw) {
        const float scale = __uint_as_float(byte << 23);  // the conversion reads its exponent: 2^(byte - 127)
        w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, mx_clamp(f[0], maxf), mx_clamp(f[1], maxf), scale, 0);
        w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, mx_clamp(f[2], maxf), mx_clamp(f[3], maxf), scale, 1);
        if constexpr (N == 8) {
            w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, mx_clamp(f[4], maxf), mx_clamp(f[5], maxf), scale, 2);
            w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, mx_clamp(f[6], maxf), mx_clamp(f[7], maxf), scale, 3);
        }
    } else if constexpr (RND == kMxSr) {
        // one hash per pair of the vector (MXFP4.md, "Stochastic rounding")
        const float inv = mx_inv_scale(byte);
        uint32_t r[N];
        mx_sr_bits<N>(j0, k0, k1, r);
#pragma unroll
        for (int e = 0; e < N; ++e) w |= mx_quant_sr(mx_clamp(f[e], maxf), inv, r[e]) << (4 * e);
    } else {
        const float inv = mx_inv_scale(byte);
#pragma unroll
        for (int e = 0; e < N; ++e) w |= mx_quant(mx_clamp(f[e], maxf), inv) << (4 * e);
    }
    return w;
}

// The lane's part of a cooperative block encode, in two steps.  A lane holds N values f
// (invalid elements +0) of a block whose kMxBlock / N lanes are neighbours.
// mx_block_amax: the bits of the block's largest |x| through xor shuffles.  Every lane of the
// wave must get here, so callers drop the lanes past the last block after it, not before.
template <int N>
__device__ __forceinline__ uint32_t mx_block_amax(const float (&f)[N]) {
    constexpr int G = kMxBlock / N;
    uint32_t am = 0;
#pragma unroll
    for (int e = 0; e < N; ++e) am = max(am, __float_as_uint(f[e]) & 0x7fffffffu);
#pragma unroll
    for (int o = 1; o < G; o <<= 1) am = max(am, (uint32_t)__shfl_xor((int)am, o, kWave));
    return am;
}

// mx_encode_lane: from that amax the block's scale byte and the lane's payload word; a NaN
// block: 0xFF and a zero word.  j0, k0, k1: as mx_quant_lane's.
template <int N, MxRound RND>
__device__ __forceinline__ void mx_encode_lane(const float (&f)[N], uint32_t am, float maxf, uint32_t& byte,
                                               uint32_t& w, uint32_t j0 = 0, uint32_t k0 = 0, uint32_t k1 = 0) {
    byte = kMxNanScale;
    w = 0;
    if (am <= 0x7f800000u) {
        byte = mx_scale_byte(min(am, __float_as_uint(maxf)));
        w = mx_quant_lane<N, RND>(f, byte, maxf, j0, k0, k1);
    }
}

// The slack of both regions of a segment, zeroed by whoever writes block nb - 1 of a range
// that ends its chunk (last).  seg and pay point at the scale byte and the payload of block
// bb of the chunk, b and nb count from there; sbytes / pbytes are the whole regions'.
// Whole-chunk callers pass bb = 0, last = true.
__device__ __forceinline__ void mx_zero_slack(uint8_t* seg, uint8_t* pay, int64_t b, int64_t nb, int64_t bb, bool last,
                                              int64_t sbytes, int64_t pbytes) {
    if (last && b == nb - 1) {
        for (int64_t q = nb; q < sbytes - bb; ++q) seg[q] = 0;
        if ((bb + nb) * kMxBlockBytes < pbytes)
            *reinterpret_cast<uint4*>(pay + nb * kMxBlockBytes) = make_uint4(0u, 0u, 0u, 0u);
    }
}

// Block b's result of a cooperative encode: the lane's N nibbles at its place `sub` in the
// block, and from sub-lane 0 the scale byte and the slack.  Plain stores: the payload stays
// in L2 / the Infinity Cache for its reader.
template <int N>
__device__ __forceinline__ void mx_store_lane(uint8_t* seg, uint8_t* pay, int64_t b, int sub, uint32_t byte,
                                              uint32_t w, int64_t nb, int64_t bb, bool last, int64_t sbytes,
                                              int64_t pbytes) {
    if constexpr (N == 4) reinterpret_cast<uint16_t*>(pay + b * kMxBlockBytes)[sub] = (uint16_t)w;
    else reinterpret_cast<uint32_t*>(pay + b * kMxBlockBytes)[sub] = w;
    if (sub == 0) {
        seg[b] = (uint8_t)byte;
        mx_zero_slack(seg, pay, b, nb, bb, last, sbytes, pbytes);
    }
}

// its whole-block sibling (one lane encoded block b of a whole chunk's nb)
__device__ __forceinline__ void mx_store_block(uint8_t* seg, uint8_t* pay, int64_t b, uint32_t byte,
                                               const uint32_t (&w)[4], int64_t nb, int64_t sbytes, int64_t pbytes) {
    seg[b] = (uint8_t)byte;
    *reinterpret_cast<uint4*>(pay + b * kMxBlockBytes) = make_uint4(w[0], w[1], w[2], w[3]);
    mx_zero_slack(seg, pay, b, nb, 0, true, sbytes, pbytes);
}

// ------------------------------------------------------------------------
// The lane's part of a wave tile of one tensor of X (a dtype; F32 for residual state), as
// f32: N consecutive elements of each of R rows, row k being blocks b0 + k * BW ..
// + BW - 1 of src (BW = 64 * N / 32 blocks per wave-wide row), the lane's elements starting
// at (b0 + k * BW) * 32 + lane * N.  vec: the tile is whole and src 16-B aligned, so 16-B
// loads (NT: non-temporal), all issued before any is unpacked; otherwise guarded element
// loads, elements at or past n count as +0 and are not read.
// ------------------------------------------------------------------------
template <typename X, bool NT, int R, int N>
__device__ __forceinline__ void mx_load_tile(const typename X::storage* src, int64_t b0, int lane, int64_t n, bool vec,
                                             float (&f)[R][N]) {
    constexpr int VN = Vec<X>::N, V = N / VN, BW = kWave / (kMxBlock / N);
    if (__builtin_expect(vec, 1)) {  // the vector path laid out as the fall-through

        uint4 raw[R][V];
#pragma unroll
        for (int k = 0; k < R; ++k)
#pragma unroll
            for (int h = 0; h < V; ++h) {
                const typename X::storage* q = src + (b0 + k * BW) * kMxBlock + lane * N + h * VN;
                raw[k][h] = NT ? nt_load16(q) : *reinterpret_cast<const uint4*>(q);
            }
#pragma unroll
        for (int k = 0; k < R; ++k)
#pragma unroll
            for (int h = 0; h < V; ++h) unpack16<X>(raw[k][h], reinterpret_cast<float(&)[VN]>(f[k][h * VN]));
    } else {
#pragma unroll
        for (int k = 0; k < R; ++k)
#pragma unroll
            for (int e = 0; e < N; ++e) {
                const int64_t j = (b0 + k * BW) * kMxBlock + lane * N + e;
                f[k][e] = j < n ? X::to_f(src[j]) : 0.0f;
            }
    }
}

// one row of f32 state back where mx_load_tile<F32> read it: N floats from dst + j0 on, as
// 16-B stores where vec, otherwise those below n one by one
template <bool NT, int N>
__device__ __forceinline__ void mx_store_row(float* dst, int64_t j0, int64_t n, bool vec, const float (&f)[N]) {
    if (vec) {
#pragma unroll
        for (int h = 0; h < N / 4; ++h) {
            const uint4 u = make_uint4(__float_as_uint(f[4 * h]), __float_as_uint(f[4 * h + 1]),
                                       __float_as_uint(f[4 * h + 2]), __float_as_uint(f[4 * h + 3]));
            if constexpr (NT) nt_store16(u, dst + j0 + 4 * h);
            else *reinterpret_cast<uint4*>(dst + j0 + 4 * h) = u;
        }
    } else {
#pragma unroll
        for (int e = 0; e < N; ++e)
            if (j0 + e < n) dst[j0 + e] = f[e];
    }
}

// x += the residual of block b (error feedback's compensated value, mx_ef_sum): a tile of
// one row that is the whole block; mx_store_row<false>(res, b * 32, ...) writes the new one back
__device__ __forceinline__ void mx_add_residual(float (&x)[kMxBlock], const float* res, int64_t b, int64_t n,
                                                bool vec) {
    float e[1][kMxBlock];
    mx_load_tile<F32, false>(res, b, 0, n, vec, e);
#pragma unroll
    for (int i = 0; i < kMxBlock; ++i) x[i] = mx_ef_sum(x[i], e[0][i]);
}

// ------------------------------------------------------------------------
// Block b of the p segments at `in` (segb bytes apart, sbytes of them scale bytes) decoded,
// summed as bagua_reduce_chunks does (s[y] = 0 + c[y] + c[y + BY], folded s[y] += s[y + h]),
// divided by pf = p if average, and rounded to T: x, as f32; padding past cs stays +0, as
// the encoder sees it.  p <= 2 * BY.
// ------------------------------------------------------------------------
template <typename T, int BY, bool HW>
__device__ __forceinline__ void mx_reduce_block(const uint8_t* in, int64_t segb, int64_t sbytes, int64_t b, int p,
                                                int average, float pf, int64_t cs, float (&x)[kMxBlock]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {  // eight elements (one payload word) of every segment at a time
        float s[8][BY];
#pragma unroll
        for (int e = 0; e < 8; ++e)
#pragma unroll
            for (int y = 0; y < BY; ++y) s[e][y] = 0.0f;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            uint32_t w[BY], sb[BY];
#pragma unroll
            for (int y = 0; y < BY; ++y) {
                const int cc = r * BY + y < p ? r * BY + y : p - 1;
                const uint8_t* seg = in + (int64_t)cc * segb;
                sb[y] = seg[b];
                w[y] = reinterpret_cast<const uint32_t*>(seg + sbytes + b * kMxBlockBytes)[q];
            }
#pragma unroll
            for (int y = 0; y < BY; ++y) {
                if (r * BY + y >= p) break;
                uint32_t u[8];
                mx_decode<T, HW, 4>(w[y], sb[y], u);
#pragma unroll
                for (int e = 0; e < 8; ++e) s[e][y] = s[e][y] + from_stored_bits<T>(u[e]);
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            tree_finish<BY>(s[e]);
            const int64_t j = b * kMxBlock + q * 8 + e;
            x[q * 8 + e] = j < cs ? as_stored<T>(average ? s[e][0] / pf : s[e][0]) : 0.0f;
        }
    }
}

// ------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------
// run-time value -> template argument: with_dtype / with_bool / with_by, codec_common.hpp

// the argument checks the entries share: p chunks of cs elements (the encode and the decode
// put chunks on grid.y: max_p = kMxGridChunks), ...
constexpr int kMxGridChunks = 65535;
static inline bool mx_counts_ok(int p, int cs, int max_p = INT_MAX) { return p > 0 && p <= max_p && cs >= 0; }
// ... a buffer that holds their p segments ...
static inline bool mx_holds(size_t bytes, int cs, int p) { return bytes >= (size_t)p * (size_t)mx_segment_bytes(cs); }
// ... aligned for its accesses: 4 where payload is read as 2- and 4-B words, 16 where payload
// words and the 16-B slack store are written ...
static inline bool mx_aligned(const void* p, int a) { return (uintptr_t)p % a == 0; }
// ... and f32 residual state
static inline bool mx_residual_ok(const float* r) { return r && mx_aligned(r, 4); }

// BAGUA_MXFP4_HWCVT=1 (the default) / 0: the hardware conversions or the arithmetic (A/B; same bytes)
inline bool mx_hw() { return tune_int("BAGUA_MXFP4_HWCVT", 1) != 0; }

inline int mx_grid(int64_t items, int64_t per_block, int nact, const char* knob) {
    int64_t b = (items + per_block - 1) / per_block;
    const int64_t cap = (tune_int(knob, 2 * kTargetBlocks) + nact - 1) / nact;
    if (b > cap) b = cap;
    return (int)(b < 1 ? 1 : b);
}

}  // namespace bagua
