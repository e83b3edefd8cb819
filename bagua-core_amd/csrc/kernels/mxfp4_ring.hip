// mxfp4_ring.hip — the decentralized low-precision ring op
// (decentralized_low_precision_synchronous.rs:42-152) with the MXFP4 codec, fused into two
// streaming kernels around the exchange, and into one at one rank.  MXFP4.md, "Ring op".
//
// Reference sequence on one bucket (n elements of T), eleven launches:
//   t += L*(1/3); t += R*(1/3); t += W*(-5/3)          :45-60  3 x addmul
//   compress(t, n_chunks = 1)                           :61-64  mxfp4_encode_kernel
//   ... ring exchange of the compressed bytes ...
//   t = dq(from_left);  L += t                          :126-133
//   t = dq(from_right); R += t                          :134-141
//   t = dq(mine);       t += W;  W = t                  :142-151
// A block of 32 elements is self-contained, so the mix and the encode are one pass with no
// min/max pass in front, no workspace and no LDS; and every path overwrites t (with dq(mine)
// + W) before anything reads it, so the mixed t is never stored:
//   mix       the three addmuls in registers (ring_mix.hpp) and the plain block encode of the
//             result, in mxfp4_encode_kernel's cooperative geometry: a lane owns one 16-B
//             vector of each of kMxRingRows blocks, of all four tensors, and the 8 / 4 lanes
//             of a block share its amax by xor shuffles.  Only the segment is written.
//   apply     mxfp4_decode_kernel's geometry: a lane owns a 16-B vector position, decodes its
//             2 / 4 payload bytes of the three segments and writes L, R, t and W.
//   one rank  its own left and right peer: the mix kernel's geometry, and each lane decodes
//             the nibbles and the scale byte it holds after the shuffle, d = dq(q(mixed));
//             L += d; R += d; t = d + W; W = t.  No payload is written or read.
// Every intermediate is rounded to T exactly where the reference stores it, so the segment
// and all four tensors equal the composed sequence byte for byte.
// The block encode, the store of its result with the slack rule and the decode are the
// steps of mxfp4_device.hpp (mx_block_amax, mx_encode_lane, mx_store_lane, mx_decode), shared with mxfp4.hip;
// the four-tensor load keeps its own interleaved issue order (mxr_load_rows).
//
// kMxRingRows = 2: with four tensors the plain encode's eight vectors in flight would be 32
// loads and 128 VGPRs of raw data.  Two rows are 8 loads and 128 B in flight per lane, what
// the plain encode has, and keep the mix at 62 VGPRs for f32 and 95-108 for 16-bit T, 8 and
// 4-5 waves per SIMD, where the 16-bit error-feedback encode, at 159-166, has 3 (the
// compiler's resource-usage remarks; MXFP4.md has the table).  Four rows would double the
// bytes in flight per lane for half the waves at best: no more bytes in flight per CU.  One
// row was not tried; neither count has been timed against the other.
#include <cstdint>

#include "codec_common.hpp"
#include "launch_util.hpp"
#include "mxfp4_common.hpp"
#include "mxfp4_device.hpp"
#include "ring_mix.hpp"

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
// mix + encode: t is read, never written
// ------------------------------------------------------------------------
template <typename T, bool HW>
__global__ __launch_bounds__(kBlock) void mxfp4_ring_mix_kernel(const typename T::storage* __restrict__ t,
                                                               const typename T::storage* __restrict__ l,
                                                               const typename T::storage* __restrict__ r,
                                                               const typename T::storage* __restrict__ w, int64_t n,
                                                               float f13, float f53, uint8_t* __restrict__ out) {
    constexpr int N = Vec<T>::N;        // elements per 16-B vector: 4 / 8
    constexpr int G = kMxBlock / N;     // lanes per block: 8 / 4
    constexpr int BW = kWave / G;       // blocks per wave-wide load: 8 / 16
    constexpr int R = kMxRingRows;
    constexpr int TB = R * BW;          // blocks per wave tile: 16 / 32 (512 / 1024 elements)
    const int64_t nb = mx_blocks(n), sbytes = mx_scale_bytes(n), pbytes = mx_payload_bytes(n);
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
            uint32_t byte, wd;  // the plain block encode of the mixed values
            mx_encode_lane<N, mx_round(HW)>(m, mx_block_amax<N>(m), maxf, byte, wd);
            const int64_t b = b0 + k * BW + lb;
            if (b >= nb) continue;
            mx_store_lane<N>(out, pay, b, sub, byte, wd, nb, 0, true, sbytes, pbytes);
        }
    }
}

// ------------------------------------------------------------------------
// one rank: mix, encode, decode and apply in one pass
// ------------------------------------------------------------------------
template <typename T, bool HW, bool NTS>
__global__ __launch_bounds__(kBlock) void mxfp4_ring_one_rank_kernel(typename T::storage* __restrict__ t,
                                                                    typename T::storage* __restrict__ w,
                                                                    typename T::storage* __restrict__ l,
                                                                    typename T::storage* __restrict__ r, int64_t n,
                                                                    float f13, float f53) {
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
            uint32_t byte, wd;  // the plain block encode of the mixed values
            mx_encode_lane<N, mx_round(HW)>(m, mx_block_amax<N>(m), maxf, byte, wd);
            if (b0 + k * BW + lb >= nb) continue;
            uint32_t u[N];  // the lane's own elements as every peer would decode them
            mx_decode<T, HW, N / 2>(wd, byte, u);
#pragma unroll
            for (int e = 0; e < N; ++e) {
                const float d = from_stored_bits<T>(u[e]);
                mx_ring_apply<T>(d, d, d, ft[k][e], fw[k][e], fl[k][e], fr[k][e]);
            }
            const int64_t j0 = (b0 + k * BW) * kMxBlock + lane * N;
            if (whole) {
                const uint4 ot = pack16<T>(ft[k]);
                mxr_store16<NTS>(pack16<T>(fl[k]), l + j0);
                mxr_store16<NTS>(pack16<T>(fr[k]), r + j0);
                mxr_store16<NTS>(ot, t + j0);
                mxr_store16<NTS>(ot, w + j0);
            } else {
#pragma unroll
                for (int e = 0; e < N; ++e)
                    if (j0 + e < n) {
                        l[j0 + e] = T::from_f(fl[k][e]);
                        r[j0 + e] = T::from_f(fr[k][e]);
                        t[j0 + e] = T::from_f(ft[k][e]);
                        w[j0 + e] = T::from_f(ft[k][e]);
                    }
            }
        }
    }
}

// ------------------------------------------------------------------------
// apply: decode three segments (they may be one and the same) and write the four tensors
// ------------------------------------------------------------------------
template <typename T, bool HW, bool NTS>
__global__ __launch_bounds__(kBlock) void mxfp4_ring_apply_kernel(const uint8_t* mine, const uint8_t* from_left,
                                                                 const uint8_t* from_right, int64_t n,
                                                                 typename T::storage* __restrict__ t,
                                                                 typename T::storage* __restrict__ w,
                                                                 typename T::storage* __restrict__ l,
                                                                 typename T::storage* __restrict__ r) {
    constexpr int N = Vec<T>::N;
    constexpr int KV = kMxRingApplyVecs;
    const int64_t sbytes = mx_scale_bytes(n);
    const int64_t nvec = (n + N - 1) / N;
    auto payload = [&](const uint8_t* seg, int64_t j) -> uint32_t {  // the N nibbles of the vector at element j
        if constexpr (N == 4) return *reinterpret_cast<const uint16_t*>(seg + sbytes + j / 2);
        else return *reinterpret_cast<const uint32_t*>(seg + sbytes + j / 2);
    };
    for (int64_t v0 = (int64_t)blockIdx.x * (kBlock * KV) + threadIdx.x; v0 < nvec;
         v0 += (int64_t)gridDim.x * (kBlock * KV)) {
        uint32_t pm[KV], pl[KV], pr[KV], sm[KV], sl[KV], sr[KV];
        uint4 ql[KV], qr[KV], qw[KV];
#pragma unroll
        for (int k = 0; k < KV; ++k) {
            const int64_t j = (v0 + k * kBlock) * N;
            pm[k] = pl[k] = pr[k] = sm[k] = sl[k] = sr[k] = 0;
            ql[k] = qr[k] = qw[k] = make_uint4(0u, 0u, 0u, 0u);
            if (v0 + k * kBlock < nvec) {
                sm[k] = mine[j / kMxBlock];
                sl[k] = from_left[j / kMxBlock];
                sr[k] = from_right[j / kMxBlock];
                pm[k] = payload(mine, j);
                pl[k] = payload(from_left, j);
                pr[k] = payload(from_right, j);
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
            uint32_t um[N], ul[N], ur[N];
            mx_decode<T, HW, N / 2>(pm[k], sm[k], um);
            mx_decode<T, HW, N / 2>(pl[k], sl[k], ul);
            mx_decode<T, HW, N / 2>(pr[k], sr[k], ur);
            if (j + N <= n) {
                float ft[N], fw[N], fl[N], fr[N];
                unpack16<T>(ql[k], fl);
                unpack16<T>(qr[k], fr);
                unpack16<T>(qw[k], fw);
#pragma unroll
                for (int e = 0; e < N; ++e)
                    mx_ring_apply<T>(from_stored_bits<T>(um[e]), from_stored_bits<T>(ul[e]),
                                     from_stored_bits<T>(ur[e]), ft[e], fw[e], fl[e], fr[e]);
                const uint4 ot = pack16<T>(ft);
                mxr_store16<NTS>(pack16<T>(fl), l + j);
                mxr_store16<NTS>(pack16<T>(fr), r + j);
                mxr_store16<NTS>(ot, t + j);
                mxr_store16<NTS>(ot, w + j);
            } else {  // the last, partial vector: nothing at or past n is read or written
#pragma unroll
                for (int e = 0; e < N; ++e)
                    if (j + e < n) {
                        float ft, fw = T::to_f(w[j + e]), fl = T::to_f(l[j + e]), fr = T::to_f(r[j + e]);
                        mx_ring_apply<T>(from_stored_bits<T>(um[e]), from_stored_bits<T>(ul[e]),
                                         from_stored_bits<T>(ur[e]), ft, fw, fl, fr);
                        l[j + e] = T::from_f(fl);
                        r[j + e] = T::from_f(fr);
                        t[j + e] = T::from_f(ft);
                        w[j + e] = T::from_f(ft);
                    }
            }
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

template <typename T>
static int mxr_mix_impl(const void* t, const void* l, const void* r, const void* w, int n, uint8_t* out,
                        size_t out_bytes, hipStream_t s) {
    using S = typename T::storage;
    if (!t || !l || !r || !w || !out || n <= 0) return BAGUA_ERR_INVALID_ARG;
    if (!mx_holds(out_bytes, n, 1) || !mx_aligned(out, 16)) return BAGUA_ERR_INVALID_ARG;
    if (!mxr_aligned16(t, l, r, w)) return BAGUA_ERR_UNSUPPORTED;
    const float f13 = mx_ring_factor(T::kDtype, 1.0 / 3.0), f53 = mx_ring_factor(T::kDtype, -5.0 / 3.0);
    const dim3 grid(mxr_tile_grid<T>(n, "BAGUA_TUNE_MX_RING_MIX_BLOCKS"));
    with_bool(mx_hw(), [&](auto hw) {
        launch(mxfp4_ring_mix_kernel<T, decltype(hw)::value>, grid, dim3(kBlock), 0, s, static_cast<const S*>(t),
               static_cast<const S*>(l), static_cast<const S*>(r), static_cast<const S*>(w), (int64_t)n, f13, f53, out);
    });
    return check_launch();
}

template <typename T>
static int mxr_one_rank_impl(void* t, void* w, void* l, void* r, int n, hipStream_t s) {
    using S = typename T::storage;
    if (!t || !w || !l || !r || n <= 0) return BAGUA_ERR_INVALID_ARG;
    if (!mxr_aligned16(t, w, l, r)) return BAGUA_ERR_UNSUPPORTED;
    const float f13 = mx_ring_factor(T::kDtype, 1.0 / 3.0), f53 = mx_ring_factor(T::kDtype, -5.0 / 3.0);
    const dim3 grid(mxr_tile_grid<T>(n, "BAGUA_TUNE_MX_RING_ONE_RANK_BLOCKS"));
    with_bool(mx_hw(), [&](auto hw) {
        with_bool(mxr_nt_stores<T>(n), [&](auto nts) {
            launch(mxfp4_ring_one_rank_kernel<T, decltype(hw)::value, decltype(nts)::value>, grid, dim3(kBlock), 0, s,
                   static_cast<S*>(t), static_cast<S*>(w), static_cast<S*>(l), static_cast<S*>(r), (int64_t)n, f13, f53);
        });
    });
    return check_launch();
}

template <typename T>
static int mxr_apply_impl(const uint8_t* mine, const uint8_t* from_left, const uint8_t* from_right, size_t comp_bytes,
                          int n, void* t, void* w, void* l, void* r, hipStream_t s) {
    using S = typename T::storage;
    if (!mine || !from_left || !from_right || !t || !w || !l || !r || n <= 0) return BAGUA_ERR_INVALID_ARG;
    if (!mx_holds(comp_bytes, n, 1)) return BAGUA_ERR_INVALID_ARG;
    if (!mx_aligned(mine, 4) || !mx_aligned(from_left, 4) || !mx_aligned(from_right, 4)) return BAGUA_ERR_INVALID_ARG;
    if (!mxr_aligned16(t, w, l, r)) return BAGUA_ERR_UNSUPPORTED;
    const int64_t nvec = ((int64_t)n + Vec<T>::N - 1) / Vec<T>::N;
    const dim3 grid(mx_grid(nvec, kBlock * kMxRingApplyVecs, 1, "BAGUA_TUNE_MX_RING_APPLY_BLOCKS"));
    with_bool(mx_hw(), [&](auto hw) {
        with_bool(mxr_nt_stores<T>(n), [&](auto nts) {
            launch(mxfp4_ring_apply_kernel<T, decltype(hw)::value, decltype(nts)::value>, grid, dim3(kBlock), 0, s, mine,
                   from_left, from_right, (int64_t)n, static_cast<S*>(t), static_cast<S*>(w), static_cast<S*>(l),
                   static_cast<S*>(r));
        });
    });
    return check_launch();
}

}  // namespace bagua

using namespace bagua;

extern "C" {

int bagua_ring_mix_mxfp4(int dtype, const void* tensor, const void* left, const void* right, const void* weight,
                         int num_elem, uint8_t* output, size_t output_bytes, bagua_stream_t stream) {
    return with_dtype(dtype, [&](auto t) {
        return mxr_mix_impl<decltype(t)>(tensor, left, right, weight, num_elem, output, output_bytes,
                                         static_cast<hipStream_t>(stream));
    });
}

int bagua_ring_apply_mxfp4(int dtype, const uint8_t* mine, const uint8_t* from_left, const uint8_t* from_right,
                           size_t compressed_bytes, int num_elem, void* tensor, void* weight, void* left, void* right,
                           bagua_stream_t stream) {
    return with_dtype(dtype, [&](auto t) {
        return mxr_apply_impl<decltype(t)>(mine, from_left, from_right, compressed_bytes, num_elem, tensor, weight,
                                           left, right, static_cast<hipStream_t>(stream));
    });
}

int bagua_ring_one_rank_mxfp4(int dtype, void* tensor, void* weight, void* left, void* right, int num_elem,
                              bagua_stream_t stream) {
    return with_dtype(dtype, [&](auto t) {
        return mxr_one_rank_impl<decltype(t)>(tensor, weight, left, right, num_elem, static_cast<hipStream_t>(stream));
    });
}

}  // extern "C"
