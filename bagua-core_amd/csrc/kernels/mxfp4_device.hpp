// mxfp4_device.hpp — what the MXFP4 kernel files (mxfp4.hip, mxfp4_ring.hip) share on the
// device and in their launchers: the decode of payload bytes as T stores them, with either
// conversion, and the two launch knobs.
#pragma once

#include <cstdint>

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

// the N payload nibbles a lane contributes to a block without NaN: its N values (f32, not yet
// clamped) under the block's scale byte, element e in bits 4e .. 4e + 3
template <int N, bool HW>
__device__ __forceinline__ uint32_t mx_quant_lane(const float (&f)[N], uint32_t byte, float maxf) {
    uint32_t w = 0;
    if constexpr (HW) {
        const float scale = __uint_as_float(byte << 23);  // the conversion reads its exponent: 2^(byte - 127)
        w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, mx_clamp(f[0], maxf), mx_clamp(f[1], maxf), scale, 0);
        w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, mx_clamp(f[2], maxf), mx_clamp(f[3], maxf), scale, 1);
        if constexpr (N == 8) {
            w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, mx_clamp(f[4], maxf), mx_clamp(f[5], maxf), scale, 2);
            w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, mx_clamp(f[6], maxf), mx_clamp(f[7], maxf), scale, 3);
        }
    } else {
        const float inv = mx_inv_scale(byte);
#pragma unroll
        for (int e = 0; e < N; ++e) w |= mx_quant(mx_clamp(f[e], maxf), inv) << (4 * e);
    }
    return w;
}

// BAGUA_MXFP4_HWCVT=1 (the default) / 0: the hardware conversions or the arithmetic (A/B; same bytes)
inline bool mx_hw() { return tune_int("BAGUA_MXFP4_HWCVT", 1) != 0; }

inline int mx_grid(int64_t items, int64_t per_block, int nact, const char* knob) {
    int64_t b = (items + per_block - 1) / per_block;
    const int64_t cap = (tune_int(knob, 2 * kTargetBlocks) + nact - 1) / nact;
    if (b > cap) b = cap;
    return (int)(b < 1 ? 1 : b);
}

}  // namespace bagua
