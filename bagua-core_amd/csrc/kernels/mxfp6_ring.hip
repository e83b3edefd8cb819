// mxfp6_ring.hip — the decentralized low-precision ring op
// (decentralized_low_precision_synchronous.rs:42-152) with the MXFP6 codec, fused into two
// streaming kernels around the exchange, and into one at one rank.  MXFP6.md, "Ring op".
//
// The reference sequence, its eleven launches and the reasoning are mxfp4_ring.hip's, and
// mxfp8_ring.hip's header says why the mixed t is never stored.  What differs is the payload:
// a lane's 4 / 8 codes are 3 / 6 bytes and no aligned word, so it leaves and arrives through
// groups of four lanes, whose 12 / 24 bytes are three aligned 4-B / 8-B words (mxfp6_device.hpp):
//   mix       mxfp8_ring_mix_kernel's geometry: one 16-B vector of t, L, R and W of each of
//             kMxRingRows blocks per lane, eight non-temporal loads issued together; the 8 / 4
//             lanes of a block share the amax of the mixed values by xor shuffles; lane s < 3
//             of a group of four takes its right neighbour's code bits by one quad move (two
//             for 48 bits) and stores word s, so a wave row writes 192 / 384 contiguous bytes
//             and no byte twice.  The quad move needs whole groups: a block's lanes are whole
//             groups and only whole blocks are dropped, on the ragged path too, where guarded
//             element loads replace the vector loads and the store stays.  Only the segment
//             is written.
//   apply     mxfp6_decode_kernel's geometry: a lane owns kMxRingApplyVecs 16-B vector
//             positions per iteration, vector v lane v % 4 of group v / 4; of each of the three
//             segments it reads the scale byte and the one or two aligned words that cover its
//             field (overlapping loads: lanes 1 and 2 read two words, lanes 0 and 3 one and
//             nothing outside their group's three) and writes L, R, t and W.
//   one rank  the mix kernel's geometry; after the shuffle a lane holds its block's scale byte
//             and its own codes and decodes them itself: d = dq(q(mixed)); L += d; R += d;
//             t = d + W; W = t.  No quad move, no payload written or read.
// Every intermediate is rounded to T exactly where the reference stores it, so the segment
// and all four tensors equal the composed sequence byte for byte.  The steps are the shared
// ones: mix<T> (ring_mix.hpp), mx_ring_apply (mxfp4_common.hpp), mx_block_amax
// (mxfp4_device.hpp), the E2M3 encode, store, field and decode of mxfp6_device.hpp, and the
// tile load, store policy and launch checks of mx_ring_device.hpp.  There is no
// hardware-conversion arm.  No LDS, no workspace; the compiler's register counts are in
// MXFP6.md and no instantiation uses scratch.
//
// Compiled without the packed f32 VALU instructions, as mxfp6.hip and mxfp8_ring.hip (whose
// header gives the reason): the contract is byte equality with the composed sequence.
#include <cstdint>

#include "codec_common.hpp"
#include "launch_util.hpp"
#include "mx_ring_device.hpp"
#include "mxfp6_common.hpp"
#include "mxfp6_device.hpp"
#include "ring_mix.hpp"

namespace bagua {

// (a target attribute that only the device pass sees)
#if defined(__HIP_DEVICE_COMPILE__)
#define MX6R_KERNEL __global__ __attribute__((target("no-packed-fp32-ops"))) __launch_bounds__(kBlock)
#else
#define MX6R_KERNEL __global__ __launch_bounds__(kBlock)
#endif

// the four results of N elements from element j0 on, as mx8r_store: 16-B stores where the
// vector is whole, otherwise the elements below n one by one
template <typename T, bool NTS>
__device__ __forceinline__ void mx6r_store(typename T::storage* t, typename T::storage* w, typename T::storage* l,
                                           typename T::storage* r, int64_t j0, int64_t n, bool vec,
                                           const float (&ft)[Vec<T>::N], const float (&fl)[Vec<T>::N],
                                           const float (&fr)[Vec<T>::N]) {
    if (vec) {
        const uint4 ot = pack16<T>(ft);
        mxr_store16<NTS>(pack16<T>(fl), l + j0);
        mxr_store16<NTS>(pack16<T>(fr), r + j0);
        mxr_store16<NTS>(ot, t + j0);
        mxr_store16<NTS>(ot, w + j0);  // W = t (clone)
    } else {
#pragma unroll
        for (int e = 0; e < Vec<T>::N; ++e)
            if (j0 + e < n) {
                l[j0 + e] = T::from_f(fl[e]);
                r[j0 + e] = T::from_f(fr[e]);
                t[j0 + e] = T::from_f(ft[e]);
                w[j0 + e] = T::from_f(ft[e]);
            }
    }
}

// The one or two aligned words that cover the field of lane s of group g in the payload `pay`
// of a segment: lo always, hi only where the field crosses into it (s = 1 and 2), so a lane
// never touches a word its group does not own.  The payload covers whole blocks, which are
// whole groups, so a group with one vector below the end has all three words.
template <typename W>
__device__ __forceinline__ void mx6r_words(const uint8_t* pay, int64_t g, int s, W& lo, W& hi) {
    const W* q = reinterpret_cast<const W*>(pay) + g * 3 + ((3 * s) >> 2);
    lo = q[0];
    hi = 0;
    if (s == 1 || s == 2) hi = q[1];
}

// N values as T stores them from the lane's words of a block with scale byte sb
template <typename T, int N>
__device__ __forceinline__ void mx6r_decode(typename Mx6Word<N>::type lo, typename Mx6Word<N>::type hi, int s,
                                            uint32_t sb, uint32_t (&u)[N]) {
    const typename Mx6Word<N>::type field = mx6_field(lo, hi, s);
    uint32_t c[N / 4];
    c[0] = (uint32_t)field;
    if constexpr (N == 8) c[1] = (uint32_t)(field >> 32);
    mx6_decode<T, N>(c, 0, sb, u);
}

// ------------------------------------------------------------------------
// mix + encode: t is read, never written
// ------------------------------------------------------------------------
template <typename T>
MX6R_KERNEL void mxfp6_ring_mix_kernel(const typename T::storage* __restrict__ t,
                                       const typename T::storage* __restrict__ l,
                                       const typename T::storage* __restrict__ r,
                                       const typename T::storage* __restrict__ w, int64_t n, float f13,
                                       float f53, uint8_t* __restrict__ out) {
    constexpr int N = Vec<T>::N;     // elements per 16-B vector: 4 / 8
    constexpr int G = kMxBlock / N;  // lanes per block: 8 / 4, whole groups of four
    constexpr int BW = kWave / G;    // blocks per wave-wide load: 8 / 16
    constexpr int R = kMxRingRows;
    constexpr int TB = R * BW;       // blocks per wave tile: 16 / 32 (512 / 1024 elements)
    const int64_t nb = mx_blocks(n), sbytes = mx_scale_bytes(n), pbytes = mx6_payload_bytes(n);
    uint8_t* pay = out + sbytes;
    const int lane = lane_id(), sub = lane % G, lb = lane / G;
    const int64_t tiles = (nb + TB - 1) / TB;
    const int64_t wave = (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
    const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
    const float maxf = T::init_max();
    for (int64_t tile = wave; tile < tiles; tile += nwaves) {
        const int64_t b0 = tile * TB;
        float ft[R][N], fw[R][N], fl[R][N], fr[R][N];
        mxr_load_rows<T, R>(t, w, l, r, b0, lane, n, (b0 + TB) * kMxBlock <= n, ft, fw, fl, fr);
#pragma unroll
        for (int k = 0; k < R; ++k) {
            float m[N];
#pragma unroll
            for (int e = 0; e < N; ++e) m[e] = mix<T>(ft[k][e], fl[k][e], fr[k][e], fw[k][e], f13, f53);
            const uint32_t am = mx_block_amax<N>(m);  // every lane of the wave shuffles
            const int64_t b = b0 + k * BW + lb;
            if (b >= nb) continue;  // whole blocks, so whole groups of four lanes
            uint32_t byte, c[N / 4];  // the plain block encode of the mixed values
            mx6_encode_lane<N>(m, am, maxf, byte, c);
            mx6_store_lane<N>(out, pay, b, sub, byte, c, nb, 0, true, sbytes, pbytes);
        }
    }
}

// ------------------------------------------------------------------------
// one rank: mix, encode, decode and apply in one pass
// ------------------------------------------------------------------------
template <typename T, bool NTS>
MX6R_KERNEL void mxfp6_ring_one_rank_kernel(typename T::storage* __restrict__ t,
                                            typename T::storage* __restrict__ w,
                                            typename T::storage* __restrict__ l,
                                            typename T::storage* __restrict__ r, int64_t n, float f13,
                                            float f53) {
    constexpr int N = Vec<T>::N;
    constexpr int G = kMxBlock / N;
    constexpr int BW = kWave / G;
    constexpr int R = kMxRingRows;
    constexpr int TB = R * BW;
    const int64_t nb = mx_blocks(n);
    const int lane = lane_id(), lb = lane / G;
    const int64_t tiles = (nb + TB - 1) / TB;
    const int64_t wave = (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
    const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
    const float maxf = T::init_max();
    for (int64_t tile = wave; tile < tiles; tile += nwaves) {
        const int64_t b0 = tile * TB;
        const bool whole = (b0 + TB) * kMxBlock <= n;
        float ft[R][N], fw[R][N], fl[R][N], fr[R][N];
        mxr_load_rows<T, R>(t, w, l, r, b0, lane, n, whole, ft, fw, fl, fr);
#pragma unroll
        for (int k = 0; k < R; ++k) {
            float m[N];
#pragma unroll
            for (int e = 0; e < N; ++e) m[e] = mix<T>(ft[k][e], fl[k][e], fr[k][e], fw[k][e], f13, f53);
            const uint32_t am = mx_block_amax<N>(m);
            if (b0 + k * BW + lb >= nb) continue;
            uint32_t byte, c[N / 4], u[N];
            mx6_encode_lane<N>(m, am, maxf, byte, c);
            mx6_decode<T, N>(c, 0, byte, u);  // the lane's own elements as every peer would decode them
#pragma unroll
            for (int e = 0; e < N; ++e) {
                const float d = from_stored_bits<T>(u[e]);
                mx_ring_apply<T>(d, d, d, ft[k][e], fw[k][e], fl[k][e], fr[k][e]);
            }
            mx6r_store<T, NTS>(t, w, l, r, (b0 + k * BW) * kMxBlock + lane * N, n, whole, ft[k], fl[k], fr[k]);
        }
    }
}

// ------------------------------------------------------------------------
// apply: decode three segments (they may be one and the same) and write the four tensors
// ------------------------------------------------------------------------
template <typename T, bool NTS>
MX6R_KERNEL void mxfp6_ring_apply_kernel(const uint8_t* mine, const uint8_t* from_left, const uint8_t* from_right,
                                         int64_t n, typename T::storage* __restrict__ t,
                                         typename T::storage* __restrict__ w,
                                         typename T::storage* __restrict__ l,
                                         typename T::storage* __restrict__ r) {
    constexpr int N = Vec<T>::N;
    constexpr int KV = kMxRingApplyVecs;
    using W = typename Mx6Word<N>::type;
    const int64_t sbytes = mx_scale_bytes(n);
    const int64_t nvec = (n + N - 1) / N;
    const int s = (int)(threadIdx.x & 3);  // v % 4 of every vector of the lane: all strides are multiples of four
    for (int64_t v0 = (int64_t)blockIdx.x * (kBlock * KV) + threadIdx.x; v0 < nvec;
         v0 += (int64_t)gridDim.x * (kBlock * KV)) {
        W lm[KV], hm[KV], ll[KV], hl[KV], lr[KV], hr[KV];
        uint32_t sm[KV], sl[KV], sr[KV];
        uint4 ql[KV], qr[KV], qw[KV];
#pragma unroll
        for (int k = 0; k < KV; ++k) {
            const int64_t v = v0 + k * kBlock, j = v * N;
            sm[k] = sl[k] = sr[k] = 0;
            lm[k] = hm[k] = ll[k] = hl[k] = lr[k] = hr[k] = 0;
            ql[k] = qr[k] = qw[k] = make_uint4(0u, 0u, 0u, 0u);
            if (v < nvec) {
                sm[k] = mine[j / kMxBlock];
                sl[k] = from_left[j / kMxBlock];
                sr[k] = from_right[j / kMxBlock];
                mx6r_words(mine + sbytes, v >> 2, s, lm[k], hm[k]);
                mx6r_words(from_left + sbytes, v >> 2, s, ll[k], hl[k]);
                mx6r_words(from_right + sbytes, v >> 2, s, lr[k], hr[k]);
                if (j + N <= n) {
                    ql[k] = nt_load16(l + j);
                    qr[k] = nt_load16(r + j);
                    qw[k] = nt_load16(w + j);
                }
            }
        }
#pragma unroll
        for (int k = 0; k < KV; ++k) {
            const int64_t j = (v0 + k * kBlock) * N;
            if (v0 + k * kBlock >= nvec) break;
            const bool vec = j + N <= n;
            uint32_t um[N], ul[N], ur[N];
            mx6r_decode<T, N>(lm[k], hm[k], s, sm[k], um);
            mx6r_decode<T, N>(ll[k], hl[k], s, sl[k], ul);
            mx6r_decode<T, N>(lr[k], hr[k], s, sr[k], ur);
            float ft[N], fw[N], fl[N], fr[N];
            if (vec) {
                unpack16<T>(ql[k], fl);
                unpack16<T>(qr[k], fr);
                unpack16<T>(qw[k], fw);
            } else {  // the last, partial vector: nothing at or past n is read or written
#pragma unroll
                for (int e = 0; e < N; ++e) {
                    const bool in = j + e < n;
                    fl[e] = in ? T::to_f(l[j + e]) : 0.0f;
                    fr[e] = in ? T::to_f(r[j + e]) : 0.0f;
                    fw[e] = in ? T::to_f(w[j + e]) : 0.0f;
                }
            }
#pragma unroll
            for (int e = 0; e < N; ++e)
                mx_ring_apply<T>(from_stored_bits<T>(um[e]), from_stored_bits<T>(ul[e]), from_stored_bits<T>(ur[e]),
                                 ft[e], fw[e], fl[e], fr[e]);
            mx6r_store<T, NTS>(t, w, l, r, j, n, vec, ft, fl, fr);
        }
    }
}

// ------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------
template <typename T>
static int mx6r_mix_impl(const void* t, const void* l, const void* r, const void* w, int n, uint8_t* out,
                         size_t out_bytes, hipStream_t s) {
    using S = typename T::storage;
    if (!t || !l || !r || !w || !out || n <= 0) return BAGUA_ERR_INVALID_ARG;
    if (!mx6_holds(out_bytes, n, 1) || !mx_aligned(out, 16)) return BAGUA_ERR_INVALID_ARG;  // 8-B payload words
    if (!mxr_aligned16(t, l, r, w)) return BAGUA_ERR_UNSUPPORTED;
    const float f13 = mx_ring_factor(T::kDtype, 1.0 / 3.0), f53 = mx_ring_factor(T::kDtype, -5.0 / 3.0);
    const dim3 grid(mxr_tile_grid<T>(n, "BAGUA_TUNE_MX6_RING_MIX_BLOCKS"));
    launch(mxfp6_ring_mix_kernel<T>, grid, dim3(kBlock), 0, s, static_cast<const S*>(t), static_cast<const S*>(l),
           static_cast<const S*>(r), static_cast<const S*>(w), (int64_t)n, f13, f53, out);
    return check_launch();
}

template <typename T>
static int mx6r_one_rank_impl(void* t, void* w, void* l, void* r, int n, hipStream_t s) {
    using S = typename T::storage;
    if (!t || !w || !l || !r || n <= 0) return BAGUA_ERR_INVALID_ARG;
    if (!mxr_aligned16(t, w, l, r)) return BAGUA_ERR_UNSUPPORTED;
    const float f13 = mx_ring_factor(T::kDtype, 1.0 / 3.0), f53 = mx_ring_factor(T::kDtype, -5.0 / 3.0);
    const dim3 grid(mxr_tile_grid<T>(n, "BAGUA_TUNE_MX6_RING_ONE_RANK_BLOCKS"));
    with_bool(mxr_nt_stores<T>(n), [&](auto nts) {
        launch(mxfp6_ring_one_rank_kernel<T, decltype(nts)::value>, grid, dim3(kBlock), 0, s, static_cast<S*>(t),
               static_cast<S*>(w), static_cast<S*>(l), static_cast<S*>(r), (int64_t)n, f13, f53);
    });
    return check_launch();
}

template <typename T>
static int mx6r_apply_impl(const uint8_t* mine, const uint8_t* from_left, const uint8_t* from_right, size_t comp_bytes,
                           int n, void* t, void* w, void* l, void* r, hipStream_t s) {
    using S = typename T::storage;
    if (!mine || !from_left || !from_right || !t || !w || !l || !r || n <= 0) return BAGUA_ERR_INVALID_ARG;
    if (!mx6_holds(comp_bytes, n, 1)) return BAGUA_ERR_INVALID_ARG;
    // payload read as 4-B (f32) / 8-B words: the decode's rule, 8 B for every dtype
    if (!mx_aligned(mine, 8) || !mx_aligned(from_left, 8) || !mx_aligned(from_right, 8)) return BAGUA_ERR_INVALID_ARG;
    if (!mxr_aligned16(t, w, l, r)) return BAGUA_ERR_UNSUPPORTED;
    const int64_t nvec = ((int64_t)n + Vec<T>::N - 1) / Vec<T>::N;
    const dim3 grid(mx_grid(nvec, kBlock * kMxRingApplyVecs, 1, "BAGUA_TUNE_MX6_RING_APPLY_BLOCKS"));
    with_bool(mxr_nt_stores<T>(n), [&](auto nts) {
        launch(mxfp6_ring_apply_kernel<T, decltype(nts)::value>, grid, dim3(kBlock), 0, s, mine, from_left, from_right,
               (int64_t)n, static_cast<S*>(t), static_cast<S*>(w), static_cast<S*>(l), static_cast<S*>(r));
    });
    return check_launch();
}

}  // namespace bagua

using namespace bagua;

extern "C" {

int bagua_ring_mix_mxfp6(int dtype, const void* tensor, const void* left, const void* right, const void* weight,
                         int num_elem, uint8_t* output, size_t output_bytes, bagua_stream_t stream) {
    return with_dtype(dtype, [&](auto t) {
        return mx6r_mix_impl<decltype(t)>(tensor, left, right, weight, num_elem, output, output_bytes,
                                          static_cast<hipStream_t>(stream));
    });
}

int bagua_ring_apply_mxfp6(int dtype, const uint8_t* mine, const uint8_t* from_left, const uint8_t* from_right,
                           size_t compressed_bytes, int num_elem, void* tensor, void* weight, void* left, void* right,
                           bagua_stream_t stream) {
    return with_dtype(dtype, [&](auto t) {
        return mx6r_apply_impl<decltype(t)>(mine, from_left, from_right, compressed_bytes, num_elem, tensor, weight,
                                            left, right, static_cast<hipStream_t>(stream));
    });
}

int bagua_ring_one_rank_mxfp6(int dtype, void* tensor, void* weight, void* left, void* right, int num_elem,
                              bagua_stream_t stream) {
    return with_dtype(dtype, [&](auto t) {
        return mx6r_one_rank_impl<decltype(t)>(tensor, weight, left, right, num_elem, static_cast<hipStream_t>(stream));
    });
}

}  // extern "C"
