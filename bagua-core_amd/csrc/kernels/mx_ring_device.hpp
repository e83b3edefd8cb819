// mx_ring_device.hpp — what the fused ring kernels of the two block codecs (mxfp4_ring.hip,
// mxfp8_ring.hip) share besides the arithmetic (ring_mix.hpp, mxfp4_common.hpp): the tile
// geometry, the interleaved four-tensor load, the store policy and the launchers' checks.
#pragma once

#include <cstdint>

#include "codec_common.hpp"
#include "launch_util.hpp"
#include "mxfp4_common.hpp"
#include "mxfp4_device.hpp"

namespace bagua {

constexpr int kMxRingRows = 2;       // blocks of each tensor a lane of the mix has in flight per iteration
constexpr int kMxRingApplyVecs = 2;  // 16-B vector positions per lane per apply iteration

template <bool NT>
__device__ __forceinline__ void mxr_store16(const uint4& v, void* p) {
    if constexpr (NT) nt_store16(v, p);
    else *reinterpret_cast<uint4*>(p) = v;
}

// The lane's vectors of rows k = 0 .. R - 1 of the wave tile that starts at block b0, of all
// four tensors, as f32: row k is blocks b0 + k * BW .. + BW - 1, the lane's vector starts at
// element (b0 + k * BW) * 32 + lane * N.  A whole tile takes non-temporal 16-B loads, all
// issued before any is consumed; otherwise guarded element loads, elements at or past n
// count as +0 and are not read (and +0 mixes to +0: +0 + (+0 * 1/3) twice, then
// +0 + (+0 * -5/3) = +0 + -0).
template <typename T, int R>
__device__ __forceinline__ void mxr_load_rows(const typename T::storage* __restrict__ t,
                                              const typename T::storage* __restrict__ w,
                                              const typename T::storage* __restrict__ l,
                                              const typename T::storage* __restrict__ r, int64_t b0, int lane,
                                              int64_t n, bool whole, float (&ft)[R][Vec<T>::N],
                                              float (&fw)[R][Vec<T>::N], float (&fl)[R][Vec<T>::N],
                                              float (&fr)[R][Vec<T>::N]) {
    constexpr int N = Vec<T>::N;
    constexpr int BW = kWave / (kMxBlock / N);
    if (whole) {
        uint4 qt[R], qw[R], ql[R], qr[R];
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int64_t j = (b0 + k * BW) * kMxBlock + lane * N;
            qt[k] = nt_load16(t + j);
            ql[k] = nt_load16(l + j);
            qr[k] = nt_load16(r + j);
            qw[k] = nt_load16(w + j);
        }
#pragma unroll
        for (int k = 0; k < R; ++k) {
            unpack16<T>(qt[k], ft[k]);
            unpack16<T>(ql[k], fl[k]);
            unpack16<T>(qr[k], fr[k]);
            unpack16<T>(qw[k], fw[k]);
        }
    } else {
#pragma unroll
        for (int k = 0; k < R; ++k)
#pragma unroll
            for (int e = 0; e < N; ++e) {
                const int64_t j = (b0 + k * BW) * kMxBlock + lane * N + e;
                const bool in = j < n;
                ft[k][e] = in ? T::to_f(t[j]) : 0.0f;
                fl[k][e] = in ? T::to_f(l[j]) : 0.0f;
                fr[k][e] = in ? T::to_f(r[j]) : 0.0f;
                fw[k][e] = in ? T::to_f(w[j]) : 0.0f;
            }
    }
}

// ------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------
// the four tensors take 16-B vector accesses
static bool mxr_aligned16(const void* a, const void* b, const void* c, const void* d) {
    return mx_aligned(a, 16) && mx_aligned(b, 16) && mx_aligned(c, 16) && mx_aligned(d, 16);
}

// Store policy of the apply and the one-rank kernel by what they write, four tensors: past
// the 256 MiB Infinity Cache the dirty lines cannot stay on chip and the stores are
// non-temporal, as the decode's (mxfp4.hip); BAGUA_MX_RING_NT=0 / 1 forces either (A/B)
template <typename T>
static bool mxr_nt_stores(int n) {
    const int env = tune_int("BAGUA_MX_RING_NT", -1);
    return env >= 0 ? env != 0 : 4 * (int64_t)n * (int64_t)sizeof(typename T::storage) > ((int64_t)256 << 20);
}

// workgroups of the mix geometry: a wave tile is kMxRingRows KiB of each tensor
template <typename T>
static int mxr_tile_grid(int n, const char* knob) {
    constexpr int64_t kTileElems = (int64_t)kMxRingRows * kWave * Vec<T>::N;
    return mx_grid(((int64_t)n + kTileElems - 1) / kTileElems, kWavesPerBlock, 1, knob);
}

}  // namespace bagua
