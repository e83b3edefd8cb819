// mxfp6_common.hpp — the arithmetic of the MXFP6 codec (MXFP6.md), one block of 32 E2M3
// elements at a time.  As mxfp8_common.hpp: plain integer / IEEE binary32 expressions that
// give the same bits on the host and on the device, so the rules can be exercised without a
// GPU (tools/mxfp6_host_check.cpp) and the kernels in mxfp6.hip only add the data movement.
// mx_bits, mx_float, mx_clamp, MxT, the block size and the NaN scale byte are
// mxfp4_common.hpp's.
#pragma once

#include <stdint.h>

#include "mxfp4_common.hpp"

namespace bagua {

constexpr int kMx6BlockBytes = 24;  // payload of one block: 32 six-bit codes
constexpr int kMx6BlockWords = 6;   // ... as little-endian 32-bit words

MX_HD int64_t mx6_payload_bytes(int64_t cs) { return mx_align32(kMx6BlockBytes * mx_blocks(cs)); }
MX_HD int64_t mx6_segment_bytes(int64_t cs) { return mx_scale_bytes(cs) + mx6_payload_bytes(cs); }

// Scale byte e + 127 of a block whose largest |x| has the bits `amax` (finite): with
// amax = 1.f * 2^(E-127) = m * 2^k, m = 1.f / 2 in [0.5, 1), k = E - 126, the rule
// e = k - 3 (m <= 0.9375) or k - 2 is E - 129 + (fraction > 0.875), and adding 0x0fffff
// carries into the exponent exactly when the fraction field exceeds 0x700000.  Zero and
// denormal amax clamp to e = -127.  The largest scaled magnitude lies in (3.75, 7.5].
MX_HD uint32_t mx6_scale_byte(uint32_t amax) {
    const int32_t b = (int32_t)((amax + 0x0fffffu) >> 23) - 2;
    return b > 0 ? (uint32_t)b : 0u;
}

// 2^-e for scale byte e + 127 in [0, 253]: biased exponent 254 - byte, always normal
MX_HD float mx6_inv_scale(uint32_t byte) { return mx_float((254u - byte) << 23); }

// 2^e: the decode's factor (2^-127 is denormal; 0xFF never gets here)
MX_HD float mx6_scale(uint32_t byte) { return mx_float(byte ? byte << 23 : 0x00400000u); }

// sign << 5 | E << 3 | M of x * 2^-e, |x * 2^-e| <= 7.5, rounded to the nearest E2M3 value,
// ties to the even mantissa.  With Ey = max(floor(log2 |y|), 0) the grid's step is
// 2^(Ey - 3) (the subnormals share the step of the first binade): adding 2^23 times the
// step rounds |y| to it in the add itself (RNE), leaving n = |y| / step in [0, 16] in the low
// bits of the sum, and the code is n + 8 * Ey; n = 16 carries into the next exponent.
MX_HD uint32_t mx6_quant(float x, float inv) {
    const float y = x * inv;
    const uint32_t yb = mx_bits(y), ya = yb & 0x7fffffffu;
    const uint32_t me = (ya > 0x3f800000u ? ya : 0x3f800000u) & 0x7f800000u;
    const uint32_t tb = mx_bits(mx_float(ya) + mx_float(me + 0x0a000000u));
    return ((tb & 31u) + (me >> 20) - 1016u) | ((yb >> 26) & 0x20u);
}

// the f32 value of a code under the scale factor sc = 2^e, magnitude clamped to maxf.  M or
// 8 + M times 2^(max(E, 1) - 4) is exact, and so is its product with sc: a 4-bit significand
// at 2^-130 or above, denormals included; past the f32 range it is inf and clamps.
MX_HD float mx6_dequant(uint32_t code, float sc, float maxf) {
    const uint32_t e = (code >> 3) & 3u, m = code & 7u;
    const float g = (float)(e ? 8u + m : m) * mx_float((123u + (e ? e : 1u)) << 23);
    const float v = __builtin_fminf(g * sc, maxf);
    return mx_float(mx_bits(v) | ((code & 0x20u) << 26));
}

// a code of a block with scale byte `byte` as f32 before the rounding to T: the canonical NaN
// under 0xFF (no code is a NaN of its own)
MX_HD float mx6_decode(uint32_t code, uint32_t byte, float maxf) {
    if (byte == kMxNanScale) return mx_float(0x7fc00000u);
    return mx6_dequant(code, mx6_scale(byte), maxf);
}

// code j of a run of codes packed six bits apart from bit `bit0` of the little-endian words w
// (bit0 + 6 j + 6 <= 32 NW); with constant arguments the shifts fold
template <int NW>
MX_HD uint32_t mx6_code_at(const uint32_t (&w)[NW], int bit) {
    const int k = bit / 32, s = bit % 32;
    uint32_t c = w[k] >> s;
    if (s > 26) c |= w[k + 1] << (32 - s);
    return c & 63u;
}

// ... and its inverse: code c (six bits) or'ed into its place
template <int NW>
MX_HD void mx6_put_code(uint32_t (&w)[NW], int bit, uint32_t c) {
    const int k = bit / 32, s = bit % 32;
    w[k] |= c << s;
    if (s > 26) w[k + 1] |= c >> (32 - s);
}

// One block: x[32] as f32 (invalid elements already +0) -> scale byte and 24 payload bytes
// as 6 little-endian words, element j in bits [6 j, 6 j + 6) of the 192.
MX_HD void mx6_encode_block(const float (&x)[kMxBlock], float maxf, uint32_t& byte, uint32_t (&w)[kMx6BlockWords]) {
    uint32_t am = 0;
#pragma unroll
    for (int e = 0; e < kMxBlock; ++e) {
        const uint32_t a = mx_bits(x[e]) & 0x7fffffffu;
        am = a > am ? a : am;
    }
#pragma unroll
    for (int k = 0; k < kMx6BlockWords; ++k) w[k] = 0u;
    if (am > 0x7f800000u) {  // a NaN in the block
        byte = kMxNanScale;
        return;
    }
    const uint32_t mb = mx_bits(maxf);
    byte = mx6_scale_byte(am < mb ? am : mb);
    const float inv = mx6_inv_scale(byte);
#pragma unroll
    for (int e = 0; e < kMxBlock; ++e) mx6_put_code(w, 6 * e, mx6_quant(mx_clamp(x[e], maxf), inv));
}

// ---- error feedback (MXFP6.md, "Error feedback") -----------------------------------
// MXFP4's rule (mx_encode_block_ef) with the E2M3 block encode and decode: the compensated
// value mx_ef_sum and the residual against the decode as T stores it, mx_ef_residual<K>, are
// mxfp4_common.hpp's.  A decode in T's normal range is exact in T (a 4-bit significand), so
// mx_as_stored rounds only among the denormals of f16 and bf16.
// K: 0 f32, 1 f16, 2 bf16.  x[32] as f32 and the residual e[32] -> scale byte, payload words and the new residual
// (all +0 for a NaN block: the state is reset, not poisoned).
template <int K>
MX_HD void mx6_encode_block_ef(const float (&x)[kMxBlock], float (&e)[kMxBlock], float maxf, uint32_t& byte,
                               uint32_t (&w)[kMx6BlockWords]) {
    float v[kMxBlock];
#pragma unroll
    for (int i = 0; i < kMxBlock; ++i) v[i] = mx_ef_sum(x[i], e[i]);
    mx6_encode_block(v, maxf, byte, w);
    if (byte == kMxNanScale) {
#pragma unroll
        for (int i = 0; i < kMxBlock; ++i) e[i] = 0.0f;
        return;
    }
    const float sc = mx6_scale(byte);
#pragma unroll
    for (int i = 0; i < kMxBlock; ++i)
        e[i] = mx_ef_residual<K>(mx_clamp(v[i], maxf), mx6_dequant(mx6_code_at(w, 6 * i), sc, maxf));
}

}  // namespace bagua
