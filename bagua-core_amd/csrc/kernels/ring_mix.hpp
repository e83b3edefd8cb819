// ring_mix.hpp — the mix step of the decentralized ring op
// (decentralized_low_precision_synchronous.rs:45-60), t += L/3; t += R/3; t += W * (-5/3),
// three rounded addmuls, stated once for the MinMax kernels (decentralized.hip), the MXFP4
// kernels (mxfp4_ring.hip) and the host check (tools/mxfp4_host_check.cpp).
//
// T is a dtype: `storage` and `stored(f)`, f as it reads back after a store to T.  On the
// device that is F32 / F16 / BF16 of codec_common.hpp, on the host MxT<K> of mxfp4_common.hpp.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RING_HD __host__ __device__ __forceinline__
#else
#define RING_HD inline
#endif

namespace bagua {

// K:236-244 addmul as the elementwise kernels compute it (elementwise.hip)
template <typename T>
RING_HD float addmul(float x, float y, float f) {
    if constexpr (sizeof(typename T::storage) == 4) return __builtin_fmaf(y, f, x);
    else return T::stored(x + T::stored(y * f));
}

// addmul<T> already returns a value rounded to T (the 16-bit path ends in
// stored; f32 is stored as computed), and rounding is idempotent, so no
// further rounding is applied between the steps
template <typename T>
RING_HD float mix(float t, float l, float r, float w, float f13, float f53) {
    t = addmul<T>(t, l, f13);
    t = addmul<T>(t, r, f13);
    return addmul<T>(t, w, f53);
}

}  // namespace bagua
