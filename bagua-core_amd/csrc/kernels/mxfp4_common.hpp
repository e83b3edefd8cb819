// mxfp4_common.hpp — the arithmetic of the MXFP4 codec (MXFP4.md), one block of 32
// elements at a time.  Plain integer / IEEE binary32 expressions that give the same bits
// on the host and on the device, so the rules can be exercised without a GPU
// (tools/mxfp4_host_check.cpp) and the kernels in mxfp4.hip only add the data movement.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MX_HD __host__ __device__ __forceinline__
#else
#define MX_HD inline
#endif

namespace bagua {

constexpr int kMxBlock = 32;        // elements sharing one scale byte
constexpr int kMxBlockBytes = 16;   // their payload
constexpr uint32_t kMxNanScale = 0xffu;

MX_HD uint32_t mx_bits(float f) { return __builtin_bit_cast(uint32_t, f); }
MX_HD float mx_float(uint32_t u) { return __builtin_bit_cast(float, u); }

MX_HD int64_t mx_align32(int64_t v) { return (v + 31) / 32 * 32; }
MX_HD int64_t mx_blocks(int64_t cs) { return (cs + kMxBlock - 1) / kMxBlock; }
MX_HD int64_t mx_scale_bytes(int64_t cs) { return mx_align32(mx_blocks(cs)); }
MX_HD int64_t mx_payload_bytes(int64_t cs) { return mx_align32(kMxBlockBytes * mx_blocks(cs)); }
MX_HD int64_t mx_segment_bytes(int64_t cs) { return mx_scale_bytes(cs) + mx_payload_bytes(cs); }

// Scale byte e + 127 of a block whose largest |x| has the bits `amax` (finite): with
// amax = 1.f * 2^(E-127) = m * 2^k, m = 1.f / 2 in [0.5, 1), k = E - 126, the rule
// e = k - 3 (m <= 0.75) or k - 2 is E - 129 + (fraction > 0.5), and adding 0x3fffff
// carries into the exponent exactly when the fraction field exceeds 0x400000.
// Denormal and zero amax (E = 0) clamp to e = -127.
MX_HD uint32_t mx_scale_byte(uint32_t amax) {
    const int32_t b = (int32_t)((amax + 0x3fffffu) >> 23) - 2;
    return b > 0 ? (uint32_t)b : 0u;
}

// 2^-e for scale byte e + 127 in [0, 253]: biased exponent 254 - byte, always normal
MX_HD float mx_inv_scale(uint32_t byte) { return mx_float((254u - byte) << 23); }

// 2^(e-1): the factor of the doubled grid 0,1,2,3,4,6,8,12 (2^-128 and 2^-127 are denormal)
MX_HD float mx_half_scale(uint32_t byte) {
    return mx_float(byte >= 2u ? (byte - 1u) << 23 : 0x00200000u << byte);
}

// +-inf -> +-largest finite T, finite values and the sign of zero unchanged (x is no NaN)
MX_HD float mx_clamp(float x, float maxf) { return __builtin_fminf(__builtin_fmaxf(x, -maxf), maxf); }

// sign << 3 | code of x * 2^-e, |x * 2^-e| <= 6, rounded to the E2M1 grid, ties to the
// even code.  The grid's step is 0.5 below 2, 1 below 4, 2 below 8: adding M = 2^22 times
// the step rounds |y| to that step in the add itself (RNE), leaving n = |y| / step in the
// low bits of the sum and the exponent E' = max(E, 127) + 22 above them, and
// code = n + 2 * (max(E, 127) - 127).
MX_HD uint32_t mx_quant(float x, float inv) {
    const float y = x * inv;
    const uint32_t yb = mx_bits(y), ya = yb & 0x7fffffffu;
    const uint32_t mx = ya > 0x3f800000u ? ya : 0x3f800000u;
    const float m = mx_float((mx & 0x7f800000u) + 0x0b000000u);
    const uint32_t tb = mx_bits(mx_float(ya) + m);
    return ((tb & 7u) + (tb >> 22) - 298u) | ((yb >> 28) & 8u);
}

// twice the grid value of a code
MX_HD uint32_t mx_grid2(uint32_t code) { return (uint32_t)(0x0C08060403020100ull >> (8u * code)) & 0xffu; }

// the f32 value of a nibble under half scale hs, magnitude clamped to maxf (the product is
// exact: a 2-bit significand times a power of two, denormals included; past the f32 range
// it is inf and clamps)
MX_HD float mx_dequant(uint32_t nib, float hs, float maxf) {
    const float v = __builtin_fminf((float)mx_grid2(nib & 7u) * hs, maxf);
    return mx_float(mx_bits(v) | ((nib & 8u) << 28));
}

// One block: x[32] as f32 (invalid elements already +0) -> scale byte and 16 payload
// bytes as 4 little-endian words.
MX_HD void mx_encode_block(const float (&x)[kMxBlock], float maxf, uint32_t& byte, uint32_t (&w)[4]) {
    uint32_t am = 0;
#pragma unroll
    for (int e = 0; e < kMxBlock; ++e) {
        const uint32_t a = mx_bits(x[e]) & 0x7fffffffu;
        am = a > am ? a : am;
    }
    w[0] = w[1] = w[2] = w[3] = 0u;
    if (am > 0x7f800000u) {  // a NaN in the block
        byte = kMxNanScale;
        return;
    }
    const uint32_t mb = mx_bits(maxf);
    byte = mx_scale_byte(am < mb ? am : mb);
    const float inv = mx_inv_scale(byte);
#pragma unroll
    for (int e = 0; e < kMxBlock; ++e) w[e / 8] |= mx_quant(mx_clamp(x[e], maxf), inv) << (4 * (e % 8));
}

// ---- stochastic rounding (MXFP4.md, "Stochastic rounding") ---------------------------
// The plain block encode with one change: an element goes to the grid value above it with
// probability equal to its fractional position between the two neighbours, decided by 16
// bits r of a counter-based hash of (key, element index in the tensor).  Scale byte, NaN
// blocks, clamps and invalid elements are the plain rule's.

// splitmix64's finaliser; the key of one (seed, step, rank, stage) is host-only arithmetic
inline uint64_t mx_sm64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
inline uint64_t mx_sr_key(uint64_t seed, uint64_t step, uint32_t rank, uint32_t stage) {
    return mx_sm64(mx_sm64(mx_sm64(seed) ^ step) ^ (2ull * rank + stage));
}

// the word of element pair `pair` = j >> 1: its low half serves the even j, its high half the odd
MX_HD uint32_t mx_fmix32(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    return h ^ (h >> 16);
}
MX_HD uint32_t mx_sr_word(uint32_t k0, uint32_t k1, uint32_t pair) { return mx_fmix32(pair + k0) ^ k1; }

// r of the N elements j0 .. j0 + N - 1 (N even): N / 2 hashes when j0 is even, one more when
// a pair straddles each end
template <int N>
MX_HD void mx_sr_bits(uint32_t j0, uint32_t k0, uint32_t k1, uint32_t (&r)[N]) {
    const uint32_t p0 = j0 >> 1;
    if ((j0 & 1u) == 0u) {
#pragma unroll
        for (int h = 0; h < N / 2; ++h) {
            const uint32_t w = mx_sr_word(k0, k1, p0 + h);
            r[2 * h] = w & 0xffffu;
            r[2 * h + 1] = w >> 16;
        }
    } else {
        r[0] = mx_sr_word(k0, k1, p0) >> 16;
#pragma unroll
        for (int h = 1; h < N / 2; ++h) {
            const uint32_t w = mx_sr_word(k0, k1, p0 + h);
            r[2 * h - 1] = w & 0xffffu;
            r[2 * h] = w >> 16;
        }
        r[N - 1] = mx_sr_word(k0, k1, p0 + N / 2) & 0xffffu;
    }
}

// mx_quant with the stochastic rule: y = |x * 2^-e| <= 6 lies on the grid of step s = 0.5
// below 2, 1 below 4, 2 from 4, s = 2^(max(E, 127) - 128).  Q = floor(y / s * 2^16) (the
// product with 2^16 / s is exact, at most 3 * 2^16, and the conversion truncates) holds
// n = floor(y / s) above its 16 fraction bits F, so (Q + r) >> 16 = n + ((F + r) >> 16),
// and the code of (n + up) * s is n + up + 2 * (max(E, 127) - 127) as in mx_quant.
MX_HD uint32_t mx_quant_sr(float x, float inv, uint32_t r) {
    const float y = x * inv;
    const uint32_t yb = mx_bits(y), ya = yb & 0x7fffffffu;
    const uint32_t me = (ya > 0x3f800000u ? ya : 0x3f800000u) & 0x7f800000u;
    const uint32_t q = (uint32_t)(mx_float(ya) * mx_float(0x87800000u - me));
    return (((q + r) >> 16) + (me >> 22) - 254u) | ((yb >> 28) & 8u);
}

// mx_encode_block under the stochastic rule; j0: the index of x[0] in the whole tensor
MX_HD void mx_encode_block_sr(const float (&x)[kMxBlock], float maxf, uint32_t j0, uint32_t k0, uint32_t k1,
                              uint32_t& byte, uint32_t (&w)[4]) {
    uint32_t am = 0;
#pragma unroll
    for (int e = 0; e < kMxBlock; ++e) {
        const uint32_t a = mx_bits(x[e]) & 0x7fffffffu;
        am = a > am ? a : am;
    }
    w[0] = w[1] = w[2] = w[3] = 0u;
    if (am > 0x7f800000u) {  // a NaN in the block
        byte = kMxNanScale;
        return;
    }
    const uint32_t mb = mx_bits(maxf);
    byte = mx_scale_byte(am < mb ? am : mb);
    const float inv = mx_inv_scale(byte);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t r[8];
        mx_sr_bits<8>(j0 + 8u * k, k0, k1, r);
#pragma unroll
        for (int e = 0; e < 8; ++e) w[k] |= mx_quant_sr(mx_clamp(x[8 * k + e], maxf), inv, r[e]) << (4 * e);
    }
}

// ---- error feedback (MXFP4.md, "Error feedback") -----------------------------------
// K: 0 f32, 1 f16, 2 bf16 (the BAGUA_DTYPE_* codes).

// A decoded value d (finite, |d| <= the largest finite T) as it reads back after a store
// to T, round to nearest even.  bf16 is the upper half of the f32 bits, denormals included.
// A decode in f16's normal range is exact (a 2-bit significand); below 2^-14 f16's step is
// 2^-24, and adding 0.5, whose unit in the last place is 2^-24, rounds |d| to it in the add.
template <int K>
MX_HD float mx_as_stored(float d) {
    if constexpr (K == 2) {
        const uint32_t u = mx_bits(d);
        return mx_float((u + 0x7fffu + ((u >> 16) & 1u)) & 0xffff0000u);
    } else if constexpr (K == 1) {
        const uint32_t u = mx_bits(d), a = u & 0x7fffffffu;
        if (a >= 0x38800000u) return d;  // |d| >= 2^-14
        const float r = (mx_float(a) + 0.5f) - 0.5f;
        return mx_float(mx_bits(r) | (u & 0x80000000u));
    } else {
        return d;
    }
}

// the compensated value of the rule: x + e, one binary32 add (a NaN stays a NaN)
MX_HD float mx_ef_sum(float x, float e) { return x + e; }

// the new residual of one element of a block that holds no NaN: vc = the clamped
// compensated value, d = the decode of its nibble (mx_dequant: clamped f32)
template <int K>
MX_HD float mx_ef_residual(float vc, float d) { return vc - mx_as_stored<K>(d); }

// One block of the rule: x[32] as f32 and the residual e[32] -> scale byte, payload words
// and the new residual (all +0 for a NaN block: the state is reset, not poisoned).
template <int K>
MX_HD void mx_encode_block_ef(const float (&x)[kMxBlock], float (&e)[kMxBlock], float maxf, uint32_t& byte,
                              uint32_t (&w)[4]) {
    float v[kMxBlock];
#pragma unroll
    for (int i = 0; i < kMxBlock; ++i) v[i] = mx_ef_sum(x[i], e[i]);
    mx_encode_block(v, maxf, byte, w);
    if (byte == kMxNanScale) {
#pragma unroll
        for (int i = 0; i < kMxBlock; ++i) e[i] = 0.0f;
        return;
    }
    const float hs = mx_half_scale(byte);
#pragma unroll
    for (int i = 0; i < kMxBlock; ++i)
        e[i] = mx_ef_residual<K>(mx_clamp(v[i], maxf), mx_dequant((w[i / 8] >> (4 * (i % 8))) & 15u, hs, maxf));
}

// ---- the decentralized ring op (MXFP4.md, "Ring op") ---------------------------------
// Per element, with the block's scale byte between the second and the third line:
//   m = mix<T>(t, l, r, w, 1/3, -5/3)                      ring_mix.hpp
//   (byte, nibble) = the plain block encode of the 32 m    mx_encode_block
//   d = mx_dq<T>(nibble, byte)                             the decode as stored in T
//   L = stored(L + d_left); R = stored(R + d_right); t = stored(d_mine + W); W = t
// T is a dtype as in ring_mix.hpp: the kernels pass F32 / F16 / BF16 (codec_common.hpp),
// the host check MxT<K> below.

// any f32 value as f16 / bf16 bits, round to nearest even, and back: what the device's
// conversions give (a NaN comes out quiet), in integer and exact binary32 steps
MX_HD uint32_t mx_f16_bits(float f) {
    const uint32_t u = mx_bits(f), s = (u >> 16) & 0x8000u, a = u & 0x7fffffffu;
    if (a > 0x7f800000u) return s | 0x7e00u | ((a >> 13) & 0x3ffu);
    if (a >= 0x477ff000u) return s | 0x7c00u;  // 65520 and above round to inf
    if (a >= 0x38800000u) return s | (((a + 0xfffu + ((a >> 13) & 1u)) >> 13) - (112u << 10));
    return s | (mx_bits(mx_float(a) + 0.5f) - 0x3f000000u);  // units of 2^-24, rounded in the add
}
MX_HD float mx_f16_value(uint32_t h) {
    const uint32_t s = (h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu;
    if (e == 31u) return mx_float(s | 0x7f800000u | (m << 13));
    if (e == 0u) return mx_float(s | mx_bits((float)m * mx_float(0x33800000u)));  // m * 2^-24, exact
    return mx_float(s | ((e + 112u) << 23) | (m << 13));
}
MX_HD uint32_t mx_bf16_bits(float f) {
    const uint32_t u = mx_bits(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u >> 16) | 0x40u;
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}

template <int K>
struct MxT {  // K: 0 f32, 1 f16, 2 bf16
    using storage = uint16_t;
    static MX_HD float to_f(storage v) { return K == 1 ? mx_f16_value(v) : mx_float((uint32_t)v << 16); }
    static MX_HD storage from_f(float f) { return (storage)(K == 1 ? mx_f16_bits(f) : mx_bf16_bits(f)); }
    static MX_HD float stored(float f) { return to_f(from_f(f)); }
};
template <>
struct MxT<0> {
    using storage = float;
    static MX_HD float to_f(storage v) { return v; }
    static MX_HD storage from_f(float f) { return f; }
    static MX_HD float stored(float f) { return f; }
};

// the mix factors: f64 literals cast to f32, then to T by the 16-bit kernels (K:600)
inline float mx_ring_factor(int dtype, double f) {
    const float v = (float)f;
    return dtype == 1 ? MxT<1>::stored(v) : dtype == 2 ? MxT<2>::stored(v) : v;
}

// a nibble of a block with scale byte `byte` as the decode stores it in T: the canonical
// NaN under 0xFF, otherwise the grid value, magnitude clamped to maxf, rounded to T
template <typename T>
MX_HD float mx_dq(uint32_t nib, uint32_t byte, float maxf) {
    if (byte == kMxNanScale) return mx_float(0x7fc00000u);
    return T::stored(mx_dequant(nib, mx_half_scale(byte), maxf));
}

// :126-151 with the three decoded values of one element
template <typename T>
MX_HD void mx_ring_apply(float d_mine, float d_left, float d_right, float& t, float& w, float& l, float& r) {
    l = T::stored(l + d_left);   // L += dq(from_left)
    r = T::stored(r + d_right);  // R += dq(from_right)
    t = T::stored(d_mine + w);   // t = dq(mine) + W
    w = t;                       // W = t (clone)
}

}  // namespace bagua
