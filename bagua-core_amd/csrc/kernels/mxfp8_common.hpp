// mxfp8_common.hpp — the arithmetic of the MXFP8 codec (MXFP8.md), one block of 32 E4M3
// elements at a time.  As mxfp4_common.hpp: plain integer / IEEE binary32 expressions that
// give the same bits on the host and on the device, so the rules can be exercised without a
// GPU (tools/mxfp8_host_check.cpp) and the kernels in mxfp8.hip only add the data movement.
// mx_bits, mx_float, mx_clamp, mx_as_stored, MxT, the block size and the NaN scale byte are
// mxfp4_common.hpp's.
#pragma once

#include <stdint.h>

#include "mxfp4_common.hpp"

namespace bagua {

constexpr int kMx8BlockBytes = 32;     // payload of one block: a byte per element
constexpr uint32_t kMx8NanCode = 0x7fu;  // the one magnitude the encoder never writes

MX_HD int64_t mx8_payload_bytes(int64_t cs) { return kMx8BlockBytes * mx_blocks(cs); }
MX_HD int64_t mx8_segment_bytes(int64_t cs) { return mx_scale_bytes(cs) + mx8_payload_bytes(cs); }

// Scale byte e + 127 of a block whose largest |x| has the bits `amax` (finite): with
// amax = 1.f * 2^(E-127) = m * 2^k, m = 1.f / 2 in [0.5, 1), k = E - 126, the rule
// e = k - 9 (m <= 0.875) or k - 8 is E - 135 + (fraction > 0.75), and adding 0x1fffff
// carries into the exponent exactly when the fraction field exceeds 0x600000.  Small, zero
// and denormal amax clamp to e = -127.  The largest scaled magnitude lies in (224, 448].
MX_HD uint32_t mx8_scale_byte(uint32_t amax) {
    const int32_t b = (int32_t)((amax + 0x1fffffu) >> 23) - 8;
    return b > 0 ? (uint32_t)b : 0u;
}

// 2^-e for scale byte e + 127 in [0, 247]: biased exponent 254 - byte, always normal
MX_HD float mx8_inv_scale(uint32_t byte) { return mx_float((254u - byte) << 23); }

// 2^e: the decode's factor (2^-127 is denormal; 0xFF never gets here)
MX_HD float mx8_scale(uint32_t byte) { return mx_float(byte ? byte << 23 : 0x00400000u); }

// sign << 7 | E << 3 | M of x * 2^-e, |x * 2^-e| <= 448, rounded to the nearest E4M3 value,
// ties to the even mantissa.  With Ey = max(floor(log2 |y|), -6) the grid's step is
// 2^(Ey - 3) (the subnormals share the step of the first binade): adding 2^23 times the
// step rounds |y| to it in the add itself (RNE), leaving n = |y| / step in [0, 16] in the low
// bits of the sum, and the code is n + 8 * (Ey + 6); n = 16 carries into the next exponent.
MX_HD uint32_t mx8_quant(float x, float inv) {
    const float y = x * inv;
    const uint32_t yb = mx_bits(y), ya = yb & 0x7fffffffu;
    const uint32_t me = (ya > 0x3c800000u ? ya : 0x3c800000u) & 0x7f800000u;
    const uint32_t tb = mx_bits(mx_float(ya) + mx_float(me + 0x0a000000u));
    return ((tb & 31u) + (me >> 20) - 968u) | ((yb >> 24) & 0x80u);
}

// the f32 value of an element byte (magnitude below 0x7F) under the scale factor sc = 2^e,
// magnitude clamped to maxf.  M or 8 + M times 2^(max(E, 1) - 10) is exact, and so is its
// product with sc: a 4-bit significand at 2^-136 or above, denormals included; past the f32
// range it is inf and clamps.
MX_HD float mx8_dequant(uint32_t code, float sc, float maxf) {
    const uint32_t e = (code >> 3) & 15u, m = code & 7u;
    const float g = (float)(e ? 8u + m : m) * mx_float((117u + (e ? e : 1u)) << 23);
    const float v = __builtin_fminf(g * sc, maxf);
    return mx_float(mx_bits(v) | ((code & 0x80u) << 24));
}

// an element byte of a block with scale byte `byte` as f32 before the rounding to T: the
// canonical NaN under 0xFF or for magnitude 0x7F
MX_HD float mx8_decode(uint32_t code, uint32_t byte, float maxf) {
    if (byte == kMxNanScale || (code & 0x7fu) == kMx8NanCode) return mx_float(0x7fc00000u);
    return mx8_dequant(code, mx8_scale(byte), maxf);
}

// One block: x[32] as f32 (invalid elements already +0) -> scale byte and 32 payload
// bytes as 8 little-endian words.
MX_HD void mx8_encode_block(const float (&x)[kMxBlock], float maxf, uint32_t& byte, uint32_t (&w)[8]) {
    uint32_t am = 0;
#pragma unroll
    for (int e = 0; e < kMxBlock; ++e) {
        const uint32_t a = mx_bits(x[e]) & 0x7fffffffu;
        am = a > am ? a : am;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k] = 0u;
    if (am > 0x7f800000u) {  // a NaN in the block
        byte = kMxNanScale;
        return;
    }
    const uint32_t mb = mx_bits(maxf);
    byte = mx8_scale_byte(am < mb ? am : mb);
    const float inv = mx8_inv_scale(byte);
#pragma unroll
    for (int e = 0; e < kMxBlock; ++e) w[e / 4] |= mx8_quant(mx_clamp(x[e], maxf), inv) << (8 * (e % 4));
}

}  // namespace bagua
