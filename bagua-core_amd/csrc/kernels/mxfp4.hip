// mxfp4.hip — block-scaled 4-bit gradient codec (OCP MXFP4: 32 E2M1 elements under one
// power-of-two scale byte) for gfx950.  Format and rules: MXFP4.md; the arithmetic of
// one block: mxfp4_common.hpp.
//
// Every block is self-contained, so all three kernels are single streaming passes with
// no workspace and no LDS:
//   encode   a lane owns one 16-B input vector (4 f32 / 8 16-bit elements) of each of eight
//            blocks, loaded together, so a wave's loads are contiguous; the 8 / 4 lanes of
//            a block share its amax by xor shuffles; 2 / 4 payload bytes per lane
//   decode   a lane owns one 16-B output vector (4 f32 / 8 16-bit elements: 2 / 4 payload
//            bytes), four vectors per iteration, so a wave's stores are contiguous
//   middle   (centralized op) a lane owns one block of the own chunk: it decodes the p
//            received versions eight elements at a time, sums them in the reference's
//            tree order (reduce.hip), rounds to T and encodes the 32 results
// and the two error-feedback kernels, the encode and the middle step with an f32 residual
// read and rewritten in the same pass (further down).  SR = true on the encode and the middle
// step rounds stochastically (MXFP4.md, "Stochastic rounding"): same data movement, mx_quant_sr.
//
// HW = true takes gfx950's conversions (v_cvt_scalef32_pk_fp4_f32 / _pk_f32_fp4) for the
// rounding to and from E2M1; the scale byte, NaN blocks, the inf and largest-finite
// clamps and the rounding to T stay in the arithmetic of mxfp4_common.hpp.
#include <algorithm>
#include <cstdint>

#include "codec_common.hpp"
#include "launch_util.hpp"
#include "mxfp4_common.hpp"
#include "mxfp4_device.hpp"

namespace bagua {

constexpr int kMxItemBytes = 128;  // input bytes a lane of the encode has in flight per iteration
constexpr int kMxDecodeVecs = 4;   // 16-B output vectors per lane per decode iteration
// blocks between two piece boundaries: one wave tile of the 16-bit encode, two of the f32
// encode; 128 scale bytes, 2 KiB of payload, 4096 elements
constexpr int kMxGranule = 128;

__device__ __forceinline__ int64_t mx_valid(int64_t in_num_elem, int64_t cs, int c) {
    const int64_t r = in_num_elem - (int64_t)c * cs;
    return r < 0 ? 0 : (r < cs ? r : cs);
}

// scale byte and payload words of one block (x: f32 values, invalid elements +0)
template <bool HW>
__device__ __forceinline__ void mx_encode(const float (&x)[kMxBlock], float maxf, uint32_t& byte, uint32_t (&w)[4]) {
    if constexpr (!HW) {
        mx_encode_block(x, maxf, byte, w);
    } else {
        uint32_t am = 0;
#pragma unroll
        for (int e = 0; e < kMxBlock; ++e) am = max(am, __float_as_uint(x[e]) & 0x7fffffffu);
        w[0] = w[1] = w[2] = w[3] = 0u;
        if (am > 0x7f800000u) {
            byte = kMxNanScale;
            return;
        }
        byte = mx_scale_byte(min(am, __float_as_uint(maxf)));
        const float scale = __uint_as_float(byte << 23);  // the conversion reads its exponent: 2^(byte - 127)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            w[k] = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w[k], mx_clamp(x[8 * k], maxf), mx_clamp(x[8 * k + 1], maxf), scale, 0);
            w[k] = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w[k], mx_clamp(x[8 * k + 2], maxf), mx_clamp(x[8 * k + 3], maxf), scale, 1);
            w[k] = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w[k], mx_clamp(x[8 * k + 4], maxf), mx_clamp(x[8 * k + 5], maxf), scale, 2);
            w[k] = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w[k], mx_clamp(x[8 * k + 6], maxf), mx_clamp(x[8 * k + 7], maxf), scale, 3);
        }
    }
}

// ------------------------------------------------------------------------
// encode: one wave owns a tile of 8 KiB of input as eight wave-wide loads of 1 KiB, issued
// together (nt: read once); the G = 32 / N neighbouring lanes that hold the N-element
// vectors of one block share its amax through log2(G) xor shuffles.  A lane holding a
// whole block instead (eight 16-B loads at a 128-B lane stride) took 116 us for 256 MiB of
// f32 with nt loads against 49 us here, and 49 us with default-policy loads, which then
// cost the decode behind it 15 us (profiles/r08_mxfp4_encode_variants.json).
//
// All three plain kernels work on blocks [bb, be) of their chunks (the whole chunk is
// [0, nb)): bb is a multiple of kMxGranule, be another or nb, so a range starts on a wave
// tile of every kernel and only the range that ends at nb has a ragged tile and the slack.
// ------------------------------------------------------------------------
//
// SR (MXFP4.md, "Stochastic rounding"): the same kernel with mx_quant_sr for the element
// rounding; a lane hashes once per pair of its vector, the word's index being the pair's
// index in the whole tensor (chunk * cs + index in chunk), so the bytes do not depend on
// chunking, range or grid.  k0 / k1: the halves of the 64-bit key, unused otherwise.
template <typename T, bool HW, bool SR>
__global__ __launch_bounds__(kBlock) void mxfp4_encode_kernel(const typename T::storage* __restrict__ in,
                                                             int64_t in_num_elem, int64_t cs, int target,
                                                             uint8_t* __restrict__ out, int64_t bb, int64_t be,
                                                             uint32_t k0, uint32_t k1) {
    using S = typename T::storage;
    constexpr int N = Vec<T>::N;        // elements per 16-B vector: 4 / 8
    constexpr int G = kMxBlock / N;     // lanes per block: 8 / 4
    constexpr int BW = kWave / G;       // blocks per wave-wide load: 8 / 16
    constexpr int R = kMxItemBytes / 16;  // loads in flight per lane
    constexpr int TB = R * BW;          // blocks per wave tile (8 KiB of input)
    const int c = target < 0 ? (int)blockIdx.y : target;
    const int64_t sbytes = mx_scale_bytes(cs), pbytes = mx_payload_bytes(cs);
    // everything below is relative to block bb of the chunk: the range's nb blocks, its n
    // valid elements, their source, scale bytes and payload
    const int64_t nb = be - bb, n = max(mx_valid(in_num_elem, cs, c) - bb * kMxBlock, (int64_t)0);
    const S* src = in + (int64_t)c * cs + bb * kMxBlock;
    const bool vec = ((uintptr_t)src % 16) == 0;
    uint8_t* seg = out + (int64_t)c * (sbytes + pbytes) + bb;
    uint8_t* pay = seg + (sbytes - bb) + bb * kMxBlockBytes;
    const bool last = be == mx_blocks(cs);  // this range ends the chunk: it writes the slack
    const int lane = lane_id(), sub = lane % G, lb = lane / G;
    const int64_t tiles = (nb + TB - 1) / TB;
    const int64_t wave = (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
    const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
    const float maxf = T::init_max();
    for (int64_t t = wave; t < tiles; t += nwaves) {
        const int64_t b0 = t * TB;
        float f[R][N];
        if (vec && (b0 + TB) * kMxBlock <= n) {
            uint4 raw[R];
#pragma unroll
            for (int k = 0; k < R; ++k) {
                const S* p = src + (b0 + k * BW) * kMxBlock + lane * N;
                raw[k] = nt_load16(p);
            }
#pragma unroll
            for (int k = 0; k < R; ++k) unpack16<T>(raw[k], f[k]);
        } else {
#pragma unroll
            for (int k = 0; k < R; ++k)
#pragma unroll
                for (int e = 0; e < N; ++e) {
                    const int64_t j = (b0 + k * BW) * kMxBlock + lane * N + e;
                    f[k][e] = j < n ? T::to_f(src[j]) : 0.0f;
                }
        }
#pragma unroll
        for (int k = 0; k < R; ++k) {
            uint32_t am = 0;
#pragma unroll
            for (int e = 0; e < N; ++e) am = max(am, __float_as_uint(f[k][e]) & 0x7fffffffu);
#pragma unroll
            for (int o = 1; o < G; o <<= 1) am = max(am, (uint32_t)__shfl_xor((int)am, o, kWave));
            const int64_t b = b0 + k * BW + lb;
            if (b >= nb) continue;
            uint32_t byte = kMxNanScale, w = 0;
            if (am <= 0x7f800000u) {
                byte = mx_scale_byte(min(am, __float_as_uint(maxf)));
                if constexpr (SR) {
                    const float inv = mx_inv_scale(byte);
                    uint32_t r[N];
                    mx_sr_bits<N>((uint32_t)((int64_t)c * cs + (bb + b0 + k * BW) * kMxBlock + lane * N), k0, k1, r);
#pragma unroll
                    for (int e = 0; e < N; ++e) w |= mx_quant_sr(mx_clamp(f[k][e], maxf), inv, r[e]) << (4 * e);
                } else if constexpr (HW) {
                    const float scale = __uint_as_float(byte << 23);
                    w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, mx_clamp(f[k][0], maxf), mx_clamp(f[k][1], maxf), scale, 0);
                    w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, mx_clamp(f[k][2], maxf), mx_clamp(f[k][3], maxf), scale, 1);
                    if constexpr (N == 8) {
                        w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, mx_clamp(f[k][4], maxf), mx_clamp(f[k][5], maxf), scale, 2);
                        w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, mx_clamp(f[k][6], maxf), mx_clamp(f[k][7], maxf), scale, 3);
                    }
                } else {
                    const float inv = mx_inv_scale(byte);
#pragma unroll
                    for (int e = 0; e < N; ++e) w |= mx_quant(mx_clamp(f[k][e], maxf), inv) << (4 * e);
                }
            }
            // plain stores: the payload stays in L2 / the Infinity Cache for its reader
            if constexpr (N == 4) reinterpret_cast<uint16_t*>(pay + b * kMxBlockBytes)[sub] = (uint16_t)w;
            else reinterpret_cast<uint32_t*>(pay + b * kMxBlockBytes)[sub] = w;
            if (sub == 0) {
                seg[b] = (uint8_t)byte;
                if (last && b == nb - 1) {  // slack of both regions, zero
                    for (int64_t q = nb; q < sbytes - bb; ++q) seg[q] = 0;
                    if ((bb + nb) * kMxBlockBytes < pbytes)
                        *reinterpret_cast<uint4*>(pay + nb * kMxBlockBytes) = make_uint4(0u, 0u, 0u, 0u);
                }
            }
        }
    }
}

// ------------------------------------------------------------------------
// decode
// ------------------------------------------------------------------------
template <typename T, bool HW, bool NTS>
__global__ __launch_bounds__(kBlock) void mxfp4_decode_kernel(const uint8_t* __restrict__ in, int64_t cs,
                                                             typename T::storage* __restrict__ out, int64_t bb,
                                                             int64_t be) {
    using S = typename T::storage;
    constexpr int N = Vec<T>::N;
    constexpr int KV = kMxDecodeVecs;
    const int c = blockIdx.y;
    const int64_t sbytes = mx_scale_bytes(cs);
    // relative to block bb of the chunk: scale bytes, payload, output and the range's n elements
    const uint8_t* seg = in + (int64_t)c * (sbytes + mx_payload_bytes(cs)) + bb;
    const uint8_t* pay = seg + (sbytes - bb) + bb * kMxBlockBytes;
    S* dst = out + (int64_t)c * cs + bb * kMxBlock;
    const bool vec = ((uintptr_t)dst % 16) == 0;
    const int64_t n = min(cs, be * kMxBlock) - bb * kMxBlock;
    const int64_t nvec = (n + N - 1) / N;
    for (int64_t v0 = (int64_t)blockIdx.x * (kBlock * KV) + threadIdx.x; v0 < nvec;
         v0 += (int64_t)gridDim.x * (kBlock * KV)) {
        uint32_t w[KV], sb[KV];
#pragma unroll
        for (int k = 0; k < KV; ++k) {
            const int64_t j = (v0 + k * kBlock) * N;
            w[k] = 0;
            sb[k] = 0;
            if (v0 + k * kBlock < nvec) {
                sb[k] = seg[j / kMxBlock];
                if constexpr (N == 4) w[k] = *reinterpret_cast<const uint16_t*>(pay + j / 2);
                else w[k] = *reinterpret_cast<const uint32_t*>(pay + j / 2);
            }
        }
#pragma unroll
        for (int k = 0; k < KV; ++k) {
            const int64_t j = (v0 + k * kBlock) * N;
            if (v0 + k * kBlock >= nvec) break;
            uint32_t u[N];
            mx_decode<T, HW, N / 2>(w[k], sb[k], u);
            if (vec && j + N <= n) {
                const uint4 q = pack_stored<T>(u);
                if constexpr (NTS) nt_store16(q, dst + j);
                else *reinterpret_cast<uint4*>(dst + j) = q;
            } else {
#pragma unroll
                for (int e = 0; e < N; ++e)
                    if (j + e < n) dst[j + e] = storage_from_bits<T>(u[e]);
            }
        }
    }
}

// ------------------------------------------------------------------------
// fused middle step of the centralized op: decode the p received segments of the own
// chunk, reduce them as bagua_reduce_chunks does (s[y] = 0 + c[y] + c[y + BY], folded
// s[y] += s[y + h]; the mean is s / p; rounded to T) and encode the result into the own
// segment.  Equal, byte for byte, to decompress + bagua_reduce_chunks + compress(target).
// ------------------------------------------------------------------------
//
// SR (never storing): the re-encode rounds stochastically, hashing with the index of the own
// chunk's elements in the whole tensor, j = target * cs + index, as compress_sr(target) does.
template <typename T, int BY, bool HW, bool STORE, bool SR>
__global__ __launch_bounds__(kBlock) void mxfp4_reduce_encode_kernel(const uint8_t* __restrict__ in, int64_t cs, int p,
                                                                    int average,
                                                                    typename T::storage* __restrict__ chunk,
                                                                    uint8_t* __restrict__ out_seg, int64_t bb,
                                                                    int64_t be, uint32_t j_chunk, uint32_t k0,
                                                                    uint32_t k1) {
    static_assert(!(SR && STORE), "the stochastic middle step does not store the reduced chunk");
    constexpr int N = Vec<T>::N;
    const int64_t nb = mx_blocks(cs), sbytes = mx_scale_bytes(cs), pbytes = mx_payload_bytes(cs);
    const int64_t segb = sbytes + pbytes;
    uint8_t* pay_out = out_seg + sbytes;
    const bool vec = STORE && ((uintptr_t)chunk % 16) == 0;
    const float pf = (float)p, maxf = T::init_max();
    for (int64_t b = bb + (int64_t)blockIdx.x * kBlock + threadIdx.x; b < be; b += (int64_t)gridDim.x * kBlock) {
        float x[kMxBlock];
#pragma unroll
        for (int q = 0; q < 4; ++q) {  // eight elements (one payload word) of every segment at a time
            float s[8][BY];
#pragma unroll
            for (int e = 0; e < 8; ++e)
#pragma unroll
                for (int y = 0; y < BY; ++y) s[e][y] = 0.0f;
#pragma unroll
            for (int r = 0; r < 2; ++r) {  // p <= 2 * BY
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
                // the reduced value as stored in T; padding past cs stays +0, as the encoder sees it
                x[q * 8 + e] = j < cs ? as_stored<T>(average ? s[e][0] / pf : s[e][0]) : 0.0f;
            }
        }
        if constexpr (STORE) {
            if (vec && (b + 1) * kMxBlock <= cs) {
#pragma unroll
                for (int k = 0; k < kMxBlock / N; ++k) {
                    float f[N];
#pragma unroll
                    for (int e = 0; e < N; ++e) f[e] = x[k * N + e];
                    *reinterpret_cast<uint4*>(chunk + b * kMxBlock + k * N) = pack16<T>(f);
                }
            } else {
#pragma unroll
                for (int e = 0; e < kMxBlock; ++e)
                    if (b * kMxBlock + e < cs) chunk[b * kMxBlock + e] = T::from_f(x[e]);
            }
        }
        uint32_t byte, w[4];
        if constexpr (SR) mx_encode_block_sr(x, maxf, j_chunk + (uint32_t)b * kMxBlock, k0, k1, byte, w);
        else mx_encode<HW>(x, maxf, byte, w);
        out_seg[b] = (uint8_t)byte;
        *reinterpret_cast<uint4*>(pay_out + b * kMxBlockBytes) = make_uint4(w[0], w[1], w[2], w[3]);
        if (b == nb - 1) {
            for (int64_t k = nb; k < sbytes; ++k) out_seg[k] = 0;
            if (nb * kMxBlockBytes < pbytes)
                *reinterpret_cast<uint4*>(pay_out + nb * kMxBlockBytes) = make_uint4(0u, 0u, 0u, 0u);
        }
    }
}

// ------------------------------------------------------------------------
// error feedback (MXFP4.md, "Error feedback"): the encode of v = x + e with the f32 residual
// e read and rewritten in the same pass, e' = clamp(v) - decode(nibble) as T stores it.  A
// block's decode is known where it is encoded, so the state is the residual alone.
// ------------------------------------------------------------------------
// NE values (one or two payload words' worth, NE / 8 words in w) of a block without NaN:
// v -> the new residual, in place
template <typename T, bool HW, int NE>
__device__ __forceinline__ void mx_residual(float (&v)[NE], const uint32_t* w, uint32_t byte, float maxf) {
    constexpr int K = T::kDtype;
    if constexpr (HW) {
        typedef float f32x2v __attribute__((ext_vector_type(2)));
        const float scale = __uint_as_float(byte << 23);
#pragma unroll
        for (int e = 0; e < NE; e += 8) {
            f32x2v r[4];
            r[0] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w[e / 8], scale, 0);
            r[1] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w[e / 8], scale, 1);
            if constexpr (NE >= 8) {
                r[2] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w[e / 8], scale, 2);
                r[3] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w[e / 8], scale, 3);
            }
#pragma unroll
            for (int q = 0; q < (NE < 8 ? NE : 8) / 2; ++q) {
                v[e + 2 * q] = mx_ef_residual<K>(mx_clamp(v[e + 2 * q], maxf), mx_clamp(r[q].x, maxf));
                v[e + 2 * q + 1] = mx_ef_residual<K>(mx_clamp(v[e + 2 * q + 1], maxf), mx_clamp(r[q].y, maxf));
            }
        }
    } else {
        const float hs = mx_half_scale(byte);
#pragma unroll
        for (int e = 0; e < NE; ++e)
            v[e] = mx_ef_residual<K>(mx_clamp(v[e], maxf), mx_dequant((w[e / 8] >> (4 * (e % 8))) & 15u, hs, maxf));
    }
}

// Worker step: mxfp4_encode_kernel's cooperative layout (a lane owns one 16-B vector of T of
// each of eight blocks) plus the matching residual, N / 4 16-B f32 vectors per lane-vector.
// Every chunk is fully valid.  Gradient loads are non-temporal as the plain encode's; the
// residual's loads and stores are non-temporal when NT (the host picks by the state's size).
// Chunks whose gradient or residual is not 16-B aligned, and ragged tiles, take guarded
// element accesses.
template <typename T, bool HW, bool NT>
__global__ __launch_bounds__(kBlock) void mxfp4_encode_ef_kernel(const typename T::storage* __restrict__ in,
                                                                int64_t cs, float* __restrict__ res,
                                                                uint8_t* __restrict__ out) {
    using S = typename T::storage;
    constexpr int N = Vec<T>::N;
    constexpr int G = kMxBlock / N;
    constexpr int BW = kWave / G;
    constexpr int R = kMxItemBytes / 16;
    constexpr int TB = R * BW;
    const int c = (int)blockIdx.y;
    const S* src = in + (int64_t)c * cs;
    float* rsd = res + (int64_t)c * cs;
    const bool vecx = ((uintptr_t)src % 16) == 0, vecr = ((uintptr_t)rsd % 16) == 0;
    const int64_t nb = mx_blocks(cs), sbytes = mx_scale_bytes(cs), pbytes = mx_payload_bytes(cs);
    uint8_t* seg = out + (int64_t)c * (sbytes + pbytes);
    uint8_t* pay = seg + sbytes;
    const int lane = lane_id(), sub = lane % G, lb = lane / G;
    const int64_t tiles = (nb + TB - 1) / TB;
    const int64_t wave = (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
    const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
    const float maxf = T::init_max();
    for (int64_t t = wave; t < tiles; t += nwaves) {
        const int64_t b0 = t * TB;
        const bool full = (b0 + TB) * kMxBlock <= cs;
        float f[R][N], r[R][N];
        if (vecx && full) {
            uint4 raw[R];
#pragma unroll
            for (int k = 0; k < R; ++k) raw[k] = nt_load16(src + (b0 + k * BW) * kMxBlock + lane * N);
#pragma unroll
            for (int k = 0; k < R; ++k) unpack16<T>(raw[k], f[k]);
        } else {
#pragma unroll
            for (int k = 0; k < R; ++k)
#pragma unroll
                for (int e = 0; e < N; ++e) {
                    const int64_t j = (b0 + k * BW) * kMxBlock + lane * N + e;
                    f[k][e] = j < cs ? T::to_f(src[j]) : 0.0f;
                }
        }
        if (vecr && full) {
#pragma unroll
            for (int k = 0; k < R; ++k)
#pragma unroll
                for (int h = 0; h < N / 4; ++h) {
                    const float* q = rsd + (b0 + k * BW) * kMxBlock + lane * N + 4 * h;
                    const uint4 u = NT ? nt_load16(q) : *reinterpret_cast<const uint4*>(q);
                    r[k][4 * h] = __uint_as_float(u.x);
                    r[k][4 * h + 1] = __uint_as_float(u.y);
                    r[k][4 * h + 2] = __uint_as_float(u.z);
                    r[k][4 * h + 3] = __uint_as_float(u.w);
                }
        } else {
#pragma unroll
            for (int k = 0; k < R; ++k)
#pragma unroll
                for (int e = 0; e < N; ++e) {
                    const int64_t j = (b0 + k * BW) * kMxBlock + lane * N + e;
                    r[k][e] = j < cs ? rsd[j] : 0.0f;
                }
        }
#pragma unroll
        for (int k = 0; k < R; ++k) {
            uint32_t am = 0;
#pragma unroll
            for (int e = 0; e < N; ++e) {
                r[k][e] = mx_ef_sum(f[k][e], r[k][e]);  // v, and below the new residual
                am = max(am, __float_as_uint(r[k][e]) & 0x7fffffffu);
            }
#pragma unroll
            for (int o = 1; o < G; o <<= 1) am = max(am, (uint32_t)__shfl_xor((int)am, o, kWave));
            const int64_t b = b0 + k * BW + lb;
            if (b >= nb) continue;
            uint32_t byte = kMxNanScale, w = 0;
            if (am <= 0x7f800000u) {
                byte = mx_scale_byte(min(am, __float_as_uint(maxf)));
                if constexpr (HW) {
                    const float scale = __uint_as_float(byte << 23);
                    w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, mx_clamp(r[k][0], maxf), mx_clamp(r[k][1], maxf), scale, 0);
                    w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, mx_clamp(r[k][2], maxf), mx_clamp(r[k][3], maxf), scale, 1);
                    if constexpr (N == 8) {
                        w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, mx_clamp(r[k][4], maxf), mx_clamp(r[k][5], maxf), scale, 2);
                        w = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(w, mx_clamp(r[k][6], maxf), mx_clamp(r[k][7], maxf), scale, 3);
                    }
                } else {
                    const float inv = mx_inv_scale(byte);
#pragma unroll
                    for (int e = 0; e < N; ++e) w |= mx_quant(mx_clamp(r[k][e], maxf), inv) << (4 * e);
                }
                mx_residual<T, HW, N>(r[k], &w, byte, maxf);
            } else {  // a NaN block: the state is reset
#pragma unroll
                for (int e = 0; e < N; ++e) r[k][e] = 0.0f;
            }
            if constexpr (N == 4) reinterpret_cast<uint16_t*>(pay + b * kMxBlockBytes)[sub] = (uint16_t)w;
            else reinterpret_cast<uint32_t*>(pay + b * kMxBlockBytes)[sub] = w;
            if (sub == 0) {
                seg[b] = (uint8_t)byte;
                if (b == nb - 1) {  // slack of both regions, zero
                    for (int64_t q = nb; q < sbytes; ++q) seg[q] = 0;
                    if (nb * kMxBlockBytes < pbytes)
                        *reinterpret_cast<uint4*>(pay + nb * kMxBlockBytes) = make_uint4(0u, 0u, 0u, 0u);
                }
            }
            const int64_t j0 = (b0 + k * BW) * kMxBlock + lane * N;
            if (vecr && full) {
#pragma unroll
                for (int h = 0; h < N / 4; ++h) {
                    const uint4 u = make_uint4(__float_as_uint(r[k][4 * h]), __float_as_uint(r[k][4 * h + 1]),
                                               __float_as_uint(r[k][4 * h + 2]), __float_as_uint(r[k][4 * h + 3]));
                    if constexpr (NT) nt_store16(u, rsd + j0 + 4 * h);
                    else *reinterpret_cast<uint4*>(rsd + j0 + 4 * h) = u;
                }
            } else {
#pragma unroll
                for (int e = 0; e < N; ++e)
                    if (j0 + e < cs) rsd[j0 + e] = r[k][e];
            }
        }
    }
}

// Server step: mxfp4_reduce_encode_kernel (never storing the reduced chunk) with the server
// residual of the lane's block, 32 f32 read and written as eight 16-B vectors; a residual
// that is only 4-B aligned and the ragged last block take element accesses.
template <typename T, int BY, bool HW>
__global__ __launch_bounds__(kBlock) void mxfp4_reduce_encode_ef_kernel(const uint8_t* __restrict__ in, int64_t cs,
                                                                       int p, int average, float* __restrict__ res,
                                                                       uint8_t* __restrict__ out_seg) {
    const int64_t nb = mx_blocks(cs), sbytes = mx_scale_bytes(cs), pbytes = mx_payload_bytes(cs);
    const int64_t segb = sbytes + pbytes;
    uint8_t* pay_out = out_seg + sbytes;
    const bool vec = ((uintptr_t)res % 16) == 0;
    const float pf = (float)p, maxf = T::init_max();
    for (int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x; b < nb; b += (int64_t)gridDim.x * kBlock) {
        float x[kMxBlock];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float s[8][BY];
#pragma unroll
            for (int e = 0; e < 8; ++e)
#pragma unroll
                for (int y = 0; y < BY; ++y) s[e][y] = 0.0f;
#pragma unroll
            for (int r = 0; r < 2; ++r) {  // p <= 2 * BY
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
        const bool whole = vec && (b + 1) * kMxBlock <= cs;
        float* rb = res + b * kMxBlock;
        if (whole) {
#pragma unroll
            for (int k = 0; k < kMxBlock / 4; ++k) {
                const uint4 u = *reinterpret_cast<const uint4*>(rb + 4 * k);
                x[4 * k] = mx_ef_sum(x[4 * k], __uint_as_float(u.x));
                x[4 * k + 1] = mx_ef_sum(x[4 * k + 1], __uint_as_float(u.y));
                x[4 * k + 2] = mx_ef_sum(x[4 * k + 2], __uint_as_float(u.z));
                x[4 * k + 3] = mx_ef_sum(x[4 * k + 3], __uint_as_float(u.w));
            }
        } else {
#pragma unroll
            for (int e = 0; e < kMxBlock; ++e)
                x[e] = mx_ef_sum(x[e], b * kMxBlock + e < cs ? rb[e] : 0.0f);
        }
        uint32_t byte, w[4];
        mx_encode<HW>(x, maxf, byte, w);
        out_seg[b] = (uint8_t)byte;
        *reinterpret_cast<uint4*>(pay_out + b * kMxBlockBytes) = make_uint4(w[0], w[1], w[2], w[3]);
        if (b == nb - 1) {
            for (int64_t k = nb; k < sbytes; ++k) out_seg[k] = 0;
            if (nb * kMxBlockBytes < pbytes)
                *reinterpret_cast<uint4*>(pay_out + nb * kMxBlockBytes) = make_uint4(0u, 0u, 0u, 0u);
        }
        if (byte != kMxNanScale) {
            mx_residual<T, HW, kMxBlock>(x, w, byte, maxf);
        } else {
#pragma unroll
            for (int e = 0; e < kMxBlock; ++e) x[e] = 0.0f;
        }
        if (whole) {
#pragma unroll
            for (int k = 0; k < kMxBlock / 4; ++k)
                *reinterpret_cast<uint4*>(rb + 4 * k) =
                    make_uint4(__float_as_uint(x[4 * k]), __float_as_uint(x[4 * k + 1]), __float_as_uint(x[4 * k + 2]),
                               __float_as_uint(x[4 * k + 3]));
        } else {
#pragma unroll
            for (int e = 0; e < kMxBlock; ++e)
                if (b * kMxBlock + e < cs) rb[e] = x[e];
        }
    }
}

// ------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------
// mx_hw() and mx_grid(): mxfp4_device.hpp

// A block range [bb, be) of a chunk of cs elements as the range entries take it: bb a
// multiple of the granule in [0, nb], be in [bb, nb] and either nb or a multiple of it.
// The whole-chunk entries pass kMxWhole for [0, nb).
constexpr int kMxWhole = -1;
static bool mx_range(int cs, int& bb, int& be) {
    const int nb = (int)mx_blocks(cs);
    if (bb == kMxWhole && be == kMxWhole) {
        bb = 0;
        be = nb;
        return true;
    }
    return bb >= 0 && bb <= nb && bb % kMxGranule == 0 && be >= bb && be <= nb && (be == nb || be % kMxGranule == 0);
}

template <typename T>
static int mx_compress_impl(const void* input, int in_num_elem, int cs, int p, uint8_t* out, size_t out_bytes,
                            int target, int bb, int be, const uint64_t* key, hipStream_t s) {
    using S = typename T::storage;
    if (p <= 0 || p > 65535 || cs < 0 || in_num_elem < 0 || target < -1 || target >= p || !out || !input)
        return BAGUA_ERR_INVALID_ARG;
    if (out_bytes < (size_t)p * (size_t)mx_segment_bytes(cs)) return BAGUA_ERR_INVALID_ARG;
    if ((uintptr_t)out % 16) return BAGUA_ERR_INVALID_ARG;  // payload words and the 16-B slack store are aligned stores
    if (!mx_range(cs, bb, be)) return BAGUA_ERR_INVALID_ARG;
    if (bb == be) return BAGUA_OK;
    // a wave tile is 8 KiB of input, a workgroup four of them; the grid covers the range
    constexpr int64_t kTileBlocks = kMxItemBytes * kWave / (int64_t)sizeof(S) / kMxBlock;
    const int nact = target < 0 ? p : 1;
    const dim3 grid(mx_grid(((int64_t)(be - bb) + kTileBlocks - 1) / kTileBlocks, kWavesPerBlock, nact,
                            "BAGUA_TUNE_MX_ENCODE_BLOCKS"),
                    nact);
    if (key)  // stochastic rounding: the arithmetic alone (MXFP4.md, "The hardware conversion")
        launch(mxfp4_encode_kernel<T, false, true>, grid, dim3(kBlock), 0, s, static_cast<const S*>(input),
               (int64_t)in_num_elem, (int64_t)cs, target, out, (int64_t)bb, (int64_t)be, (uint32_t)*key,
               (uint32_t)(*key >> 32));
    else if (mx_hw())
        launch(mxfp4_encode_kernel<T, true, false>, grid, dim3(kBlock), 0, s, static_cast<const S*>(input),
               (int64_t)in_num_elem, (int64_t)cs, target, out, (int64_t)bb, (int64_t)be, 0u, 0u);
    else
        launch(mxfp4_encode_kernel<T, false, false>, grid, dim3(kBlock), 0, s, static_cast<const S*>(input),
               (int64_t)in_num_elem, (int64_t)cs, target, out, (int64_t)bb, (int64_t)be, 0u, 0u);
    return check_launch();
}

template <typename T, bool HW>
static void mx_launch_decode(const dim3& grid, bool nt, const uint8_t* in, int64_t cs, typename T::storage* out,
                             int64_t bb, int64_t be, hipStream_t s) {
    if (nt) launch(mxfp4_decode_kernel<T, HW, true>, grid, dim3(kBlock), 0, s, in, cs, out, bb, be);
    else launch(mxfp4_decode_kernel<T, HW, false>, grid, dim3(kBlock), 0, s, in, cs, out, bb, be);
}

template <typename T>
static int mx_decompress_impl(const uint8_t* in, size_t in_bytes, int cs, int p, void* out, int bb, int be,
                              hipStream_t s) {
    using S = typename T::storage;
    if (p <= 0 || p > 65535 || cs < 0 || !in || !out) return BAGUA_ERR_INVALID_ARG;
    if (in_bytes < (size_t)p * (size_t)mx_segment_bytes(cs)) return BAGUA_ERR_INVALID_ARG;
    if ((uintptr_t)in % 4) return BAGUA_ERR_INVALID_ARG;  // payload read as 2- and 4-B words
    if (!mx_range(cs, bb, be)) return BAGUA_ERR_INVALID_ARG;
    if (bb == be) return BAGUA_OK;
    // store policy by the bucket's size (not the range's), as the 1-bit decode's (onebit.hip): past the
    // 256 MiB Infinity Cache the dirty lines cannot stay on chip; BAGUA_MX_DECODE_NT=0 / 1 forces either
    const int env = tune_int("BAGUA_MX_DECODE_NT", -1);
    const bool nt = env >= 0 ? env != 0 : (int64_t)cs * p * (int64_t)sizeof(S) > ((int64_t)256 << 20);
    constexpr int N = Vec<T>::N;
    const int64_t last = std::min(((int64_t)cs + N - 1) / N, (int64_t)be * (kMxBlock / N));
    const int64_t nvec = last - (int64_t)bb * (kMxBlock / N);  // the range's 16-B output vectors
    const dim3 grid(mx_grid(nvec, kBlock * kMxDecodeVecs, p, "BAGUA_TUNE_MX_DECODE_BLOCKS"), p);
    if (mx_hw()) mx_launch_decode<T, true>(grid, nt, in, (int64_t)cs, static_cast<S*>(out), bb, be, s);
    else mx_launch_decode<T, false>(grid, nt, in, (int64_t)cs, static_cast<S*>(out), bb, be, s);
    return check_launch();
}

template <typename T, int BY, bool HW>
static void mx_launch_reduce(int blocks, const uint8_t* in, int64_t cs, int p, int average,
                             typename T::storage* chunk, uint8_t* seg, int64_t bb, int64_t be, uint32_t j_chunk,
                             const uint64_t* key, hipStream_t s) {
    if (key)  // stochastic re-encode (never storing); the decode of the received segments is the plain one
        launch(mxfp4_reduce_encode_kernel<T, BY, HW, false, true>, dim3(blocks), dim3(kBlock), 0, s, in, cs, p,
               average, chunk, seg, bb, be, j_chunk, (uint32_t)*key, (uint32_t)(*key >> 32));
    else if (chunk)
        launch(mxfp4_reduce_encode_kernel<T, BY, HW, true, false>, dim3(blocks), dim3(kBlock), 0, s, in, cs, p,
               average, chunk, seg, bb, be, 0u, 0u, 0u);
    else
        launch(mxfp4_reduce_encode_kernel<T, BY, HW, false, false>, dim3(blocks), dim3(kBlock), 0, s, in, cs, p,
               average, chunk, seg, bb, be, 0u, 0u, 0u);
}

template <typename T, bool HW>
static void mx_dispatch_reduce(int blocks, const uint8_t* in, int64_t cs, int p, int average,
                               typename T::storage* chunk, uint8_t* seg, int64_t bb, int64_t be, uint32_t j_chunk,
                               const uint64_t* key, hipStream_t s) {
    switch (reduce_by(p)) {
        case 2: mx_launch_reduce<T, 2, HW>(blocks, in, cs, p, average, chunk, seg, bb, be, j_chunk, key, s); break;
        case 4: mx_launch_reduce<T, 4, HW>(blocks, in, cs, p, average, chunk, seg, bb, be, j_chunk, key, s); break;
        default: mx_launch_reduce<T, 8, HW>(blocks, in, cs, p, average, chunk, seg, bb, be, j_chunk, key, s); break;
    }
}

template <typename T>
static int mx_reduce_requantize_impl(const uint8_t* recv, size_t recv_bytes, int cs, int p, void* tensor, int average,
                                     uint8_t* out, size_t out_bytes, int target, int bb, int be, const uint64_t* key,
                                     hipStream_t s) {
    using S = typename T::storage;
    if (p <= 0 || cs < 0 || target < 0 || target >= p || !recv || !out) return BAGUA_ERR_INVALID_ARG;
    if (p > kMaxFusedChunks) return BAGUA_ERR_UNSUPPORTED;  // caller runs decompress + reduce + compress
    const size_t segb = (size_t)mx_segment_bytes(cs);
    if (recv_bytes < (size_t)p * segb || out_bytes < (size_t)p * segb) return BAGUA_ERR_INVALID_ARG;
    if ((uintptr_t)recv % 4 || (uintptr_t)out % 16) return BAGUA_ERR_INVALID_ARG;
    if (!mx_range(cs, bb, be)) return BAGUA_ERR_INVALID_ARG;
    if (bb == be) return BAGUA_OK;
    S* chunk = tensor ? static_cast<S*>(tensor) + (int64_t)target * cs : nullptr;  // nullptr: not stored
    uint8_t* seg = out + (size_t)target * segb;
    const int blocks = mx_grid(be - bb, kBlock, 1, "BAGUA_TUNE_MX_MIDDLE_BLOCKS");
    const uint32_t jc = (uint32_t)((int64_t)target * cs);  // index of the own chunk's first element
    if (mx_hw()) mx_dispatch_reduce<T, true>(blocks, recv, (int64_t)cs, p, average, chunk, seg, bb, be, jc, key, s);
    else mx_dispatch_reduce<T, false>(blocks, recv, (int64_t)cs, p, average, chunk, seg, bb, be, jc, key, s);
    return check_launch();
}

// ---- error feedback ----
template <typename T, bool HW>
static void mx_launch_encode_ef(const dim3& grid, bool nt, const typename T::storage* in, int64_t cs, float* res,
                                uint8_t* out, hipStream_t s) {
    if (nt) launch(mxfp4_encode_ef_kernel<T, HW, true>, grid, dim3(kBlock), 0, s, in, cs, res, out);
    else launch(mxfp4_encode_ef_kernel<T, HW, false>, grid, dim3(kBlock), 0, s, in, cs, res, out);
}

template <typename T>
static int mx_compress_ef_impl(const void* input, int in_num_elem, int cs, int p, uint8_t* out, size_t out_bytes,
                               int target, float* residual, hipStream_t s) {
    using S = typename T::storage;
    if (p <= 0 || p > 65535 || cs < 0 || target != -1 || !out || !input) return BAGUA_ERR_INVALID_ARG;
    if ((int64_t)in_num_elem != (int64_t)cs * p) return BAGUA_ERR_INVALID_ARG;  // every chunk fully valid
    if (!residual || (uintptr_t)residual % 4) return BAGUA_ERR_INVALID_ARG;
    if (out_bytes < (size_t)p * (size_t)mx_segment_bytes(cs)) return BAGUA_ERR_INVALID_ARG;
    if ((uintptr_t)out % 16) return BAGUA_ERR_INVALID_ARG;
    if (cs == 0) return BAGUA_OK;
    constexpr int64_t kTileElems = kMxItemBytes * kWave / (int64_t)sizeof(S);
    const dim3 grid(mx_grid(((int64_t)cs + kTileElems - 1) / kTileElems, kWavesPerBlock, p, "BAGUA_TUNE_MX_ENCODE_BLOCKS"),
                    p);
    // Residual policy by what the step streams, gradient plus residual: up to the 256 MiB
    // Infinity Cache default-policy accesses (the next step's encode may find the residual
    // there; not measured), past it non-temporal ones.  For 256 MiB of f32 non-temporal took
    // 143 against 146 us and the decode behind it 47 against 63 us; for 2^27 bf16 276 against
    // 252 us and the decode 56 against 62 us, so there the default policy was ahead in sum
    // (profiles/r09_mxfp4_ef.json; MXFP4.md).
    // BAGUA_MX_EF_RESIDUAL_NT=1 / 0 forces either (A/B).
    const int env = tune_int("BAGUA_MX_EF_RESIDUAL_NT", -1);
    const bool nt = env >= 0 ? env != 0 : (int64_t)cs * p * (4 + (int64_t)sizeof(S)) > ((int64_t)256 << 20);
    if (mx_hw()) mx_launch_encode_ef<T, true>(grid, nt, static_cast<const S*>(input), (int64_t)cs, residual, out, s);
    else mx_launch_encode_ef<T, false>(grid, nt, static_cast<const S*>(input), (int64_t)cs, residual, out, s);
    return check_launch();
}

template <typename T, bool HW>
static void mx_dispatch_reduce_ef(int blocks, const uint8_t* in, int64_t cs, int p, int average, float* res,
                                  uint8_t* seg, hipStream_t s) {
    switch (reduce_by(p)) {
        case 2:
            launch(mxfp4_reduce_encode_ef_kernel<T, 2, HW>, dim3(blocks), dim3(kBlock), 0, s, in, cs, p, average, res, seg);
            break;
        case 4:
            launch(mxfp4_reduce_encode_ef_kernel<T, 4, HW>, dim3(blocks), dim3(kBlock), 0, s, in, cs, p, average, res, seg);
            break;
        default:
            launch(mxfp4_reduce_encode_ef_kernel<T, 8, HW>, dim3(blocks), dim3(kBlock), 0, s, in, cs, p, average, res, seg);
            break;
    }
}

template <typename T>
static int mx_reduce_requantize_ef_impl(const uint8_t* recv, size_t recv_bytes, int cs, int p, int average,
                                        uint8_t* out, size_t out_bytes, int target, float* residual, hipStream_t s) {
    if (p <= 0 || cs < 0 || target < 0 || target >= p || !recv || !out) return BAGUA_ERR_INVALID_ARG;
    if (!residual || (uintptr_t)residual % 4) return BAGUA_ERR_INVALID_ARG;
    if (p > kMaxFusedChunks) return BAGUA_ERR_UNSUPPORTED;  // caller runs decompress + reduce + compress_ef
    const size_t segb = (size_t)mx_segment_bytes(cs);
    if (recv_bytes < (size_t)p * segb || out_bytes < (size_t)p * segb) return BAGUA_ERR_INVALID_ARG;
    if ((uintptr_t)recv % 4 || (uintptr_t)out % 16) return BAGUA_ERR_INVALID_ARG;
    if (cs == 0) return BAGUA_OK;
    uint8_t* seg = out + (size_t)target * segb;
    const int blocks = mx_grid(mx_blocks(cs), kBlock, 1, "BAGUA_TUNE_MX_MIDDLE_BLOCKS");
    if (mx_hw()) mx_dispatch_reduce_ef<T, true>(blocks, recv, (int64_t)cs, p, average, residual, seg, s);
    else mx_dispatch_reduce_ef<T, false>(blocks, recv, (int64_t)cs, p, average, residual, seg, s);
    return check_launch();
}

}  // namespace bagua

using namespace bagua;

extern "C" {

int bagua_mxfp4_ef_state_bytes(int chunk_size, int num_chunks, size_t* worker_bytes, size_t* server_bytes) {
    if (chunk_size < 0 || num_chunks <= 0 || !worker_bytes || !server_bytes) return BAGUA_ERR_INVALID_ARG;
    *worker_bytes = (size_t)chunk_size * (size_t)num_chunks * sizeof(float);
    *server_bytes = (size_t)chunk_size * sizeof(float);
    return BAGUA_OK;
}

int bagua_mxfp4_compress_ef(int dtype, const void* input, int input_num_element, int chunk_size, int num_chunks,
                            uint8_t* output, size_t output_bytes, int target_chunk, float* residual,
                            bagua_stream_t stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (dtype) {
        case BAGUA_DTYPE_F32:
            return mx_compress_ef_impl<F32>(input, input_num_element, chunk_size, num_chunks, output, output_bytes,
                                            target_chunk, residual, s);
        case BAGUA_DTYPE_F16:
            return mx_compress_ef_impl<F16>(input, input_num_element, chunk_size, num_chunks, output, output_bytes,
                                            target_chunk, residual, s);
        case BAGUA_DTYPE_BF16:
            return mx_compress_ef_impl<BF16>(input, input_num_element, chunk_size, num_chunks, output, output_bytes,
                                             target_chunk, residual, s);
    }
    return BAGUA_ERR_UNSUPPORTED;
}

int bagua_mxfp4_reduce_requantize_ef(int dtype, const uint8_t* input, size_t input_bytes, int chunk_size,
                                     int num_chunks, int average, uint8_t* output, size_t output_bytes,
                                     int target_chunk, float* residual, bagua_stream_t stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (dtype) {
        case BAGUA_DTYPE_F32:
            return mx_reduce_requantize_ef_impl<F32>(input, input_bytes, chunk_size, num_chunks, average, output,
                                                     output_bytes, target_chunk, residual, s);
        case BAGUA_DTYPE_F16:
            return mx_reduce_requantize_ef_impl<F16>(input, input_bytes, chunk_size, num_chunks, average, output,
                                                     output_bytes, target_chunk, residual, s);
        case BAGUA_DTYPE_BF16:
            return mx_reduce_requantize_ef_impl<BF16>(input, input_bytes, chunk_size, num_chunks, average, output,
                                                      output_bytes, target_chunk, residual, s);
    }
    return BAGUA_ERR_UNSUPPORTED;
}

size_t bagua_mxfp4_compressed_bytes(int chunk_size, int num_chunks) {
    if (chunk_size < 0 || num_chunks < 0) return 0;
    return (size_t)num_chunks * (size_t)mx_segment_bytes(chunk_size);
}

// the whole-chunk entries are the range [0, nb) (kMxWhole) of the range entries' code
static int mx_compress(int dtype, const void* input, int input_num_element, int chunk_size, int num_chunks,
                       uint8_t* output, size_t output_bytes, int target_chunk, int bb, int be, const uint64_t* key,
                       hipStream_t s) {
    switch (dtype) {
        case BAGUA_DTYPE_F32:
            return mx_compress_impl<F32>(input, input_num_element, chunk_size, num_chunks, output, output_bytes,
                                         target_chunk, bb, be, key, s);
        case BAGUA_DTYPE_F16:
            return mx_compress_impl<F16>(input, input_num_element, chunk_size, num_chunks, output, output_bytes,
                                         target_chunk, bb, be, key, s);
        case BAGUA_DTYPE_BF16:
            return mx_compress_impl<BF16>(input, input_num_element, chunk_size, num_chunks, output, output_bytes,
                                          target_chunk, bb, be, key, s);
    }
    return BAGUA_ERR_UNSUPPORTED;
}

static int mx_decompress(int dtype, const uint8_t* input, size_t input_bytes, int chunk_size, int num_chunks,
                         void* output, int bb, int be, hipStream_t s) {
    switch (dtype) {
        case BAGUA_DTYPE_F32:
            return mx_decompress_impl<F32>(input, input_bytes, chunk_size, num_chunks, output, bb, be, s);
        case BAGUA_DTYPE_F16:
            return mx_decompress_impl<F16>(input, input_bytes, chunk_size, num_chunks, output, bb, be, s);
        case BAGUA_DTYPE_BF16:
            return mx_decompress_impl<BF16>(input, input_bytes, chunk_size, num_chunks, output, bb, be, s);
    }
    return BAGUA_ERR_UNSUPPORTED;
}

static int mx_reduce_requantize(int dtype, const uint8_t* input, size_t input_bytes, int chunk_size, int num_chunks,
                                void* tensor, int average, uint8_t* output, size_t output_bytes, int target_chunk,
                                int bb, int be, const uint64_t* key, hipStream_t s) {
    switch (dtype) {
        case BAGUA_DTYPE_F32:
            return mx_reduce_requantize_impl<F32>(input, input_bytes, chunk_size, num_chunks, tensor, average, output,
                                                  output_bytes, target_chunk, bb, be, key, s);
        case BAGUA_DTYPE_F16:
            return mx_reduce_requantize_impl<F16>(input, input_bytes, chunk_size, num_chunks, tensor, average, output,
                                                  output_bytes, target_chunk, bb, be, key, s);
        case BAGUA_DTYPE_BF16:
            return mx_reduce_requantize_impl<BF16>(input, input_bytes, chunk_size, num_chunks, tensor, average,
                                                   output, output_bytes, target_chunk, bb, be, key, s);
    }
    return BAGUA_ERR_UNSUPPORTED;
}

int bagua_mxfp4_compress(int dtype, const void* input, int input_num_element, int chunk_size, int num_chunks,
                         uint8_t* output, size_t output_bytes, int target_chunk, bagua_stream_t stream) {
    return mx_compress(dtype, input, input_num_element, chunk_size, num_chunks, output, output_bytes, target_chunk,
                       kMxWhole, kMxWhole, nullptr, static_cast<hipStream_t>(stream));
}

int bagua_mxfp4_decompress(int dtype, const uint8_t* input, size_t input_bytes, int chunk_size, int num_chunks,
                           void* output, bagua_stream_t stream) {
    return mx_decompress(dtype, input, input_bytes, chunk_size, num_chunks, output, kMxWhole, kMxWhole,
                         static_cast<hipStream_t>(stream));
}

int bagua_mxfp4_reduce_requantize(int dtype, const uint8_t* input, size_t input_bytes, int chunk_size, int num_chunks,
                                  void* tensor, int average, uint8_t* output, size_t output_bytes, int target_chunk,
                                  bagua_stream_t stream) {
    return mx_reduce_requantize(dtype, input, input_bytes, chunk_size, num_chunks, tensor, average, output,
                                output_bytes, target_chunk, kMxWhole, kMxWhole, nullptr,
                                static_cast<hipStream_t>(stream));
}

// ---- pieces (MXFP4.md, "Pipelined op") ----
// Piece `piece` of schedule `pieces` as a block range: bagua_minmax_u8_piece_range's rule
// on nb blocks with edges rounded up to the granule.  Tapered from 3 pieces on: edge
// weights 0, 1, 3, ..., 2(k - 1), so the first and the last piece are half size.
int bagua_mxfp4_piece_range(int chunk_size, int pieces, int piece, int* block_begin, int* block_end) {
    const int count = pieces & BAGUA_PIECES_COUNT_MASK;
    if (chunk_size < 0 || count < 1 || piece < 0 || piece >= count || !block_begin || !block_end ||
        (pieces & ~(BAGUA_PIECES_COUNT_MASK | BAGUA_PIECES_TAPERED | BAGUA_PIECES_MULTIPATH | BAGUA_PIECES_FOLDED |
                    BAGUA_PIECES_TABLES)))
        return BAGUA_ERR_INVALID_ARG;
    const int64_t nb = mx_blocks(chunk_size);
    auto clip = [&](int64_t blocks) -> int {
        const int64_t x = (blocks + kMxGranule - 1) / kMxGranule * kMxGranule;
        return (int)(x < nb ? x : nb);
    };
    if (count >= 3 && (pieces & BAGUA_PIECES_TAPERED)) {
        const int64_t W = 2 * (int64_t)(count - 1);
        // edge j at weight 2j - 1 of W, rounded up, and at least a granule past edge j - 1: a
        // chunk of fewer than W granules then fills its first pieces and leaves its last ones
        // empty (with W granules or more the rounded edges are a granule apart by themselves)
        int64_t e = 0;
        for (int j = 1; j <= piece + 1; ++j) {
            if (j == piece + 1) *block_begin = (int)e;
            e = j >= count ? nb : clip(std::max((nb * (2 * (int64_t)j - 1) + W - 1) / W, e + kMxGranule));
        }
        *block_end = (int)e;
    } else {
        const int64_t L = clip((nb + count - 1) / count);  // nb < L only when one piece holds everything
        *block_begin = (int)std::min((int64_t)piece * L, nb);
        *block_end = (int)std::min(((int64_t)piece + 1) * L, nb);
    }
    return BAGUA_OK;
}

int bagua_mxfp4_compress_range(int dtype, const void* input, int input_num_element, int chunk_size, int num_chunks,
                               uint8_t* output, size_t output_bytes, int block_begin, int block_end,
                               bagua_stream_t stream) {
    if (block_begin < 0) return BAGUA_ERR_INVALID_ARG;
    return mx_compress(dtype, input, input_num_element, chunk_size, num_chunks, output, output_bytes, -1,
                       block_begin, block_end, nullptr, static_cast<hipStream_t>(stream));
}

int bagua_mxfp4_decompress_range(int dtype, const uint8_t* input, size_t input_bytes, int chunk_size, int num_chunks,
                                 void* output, int block_begin, int block_end, bagua_stream_t stream) {
    if (block_begin < 0) return BAGUA_ERR_INVALID_ARG;
    return mx_decompress(dtype, input, input_bytes, chunk_size, num_chunks, output, block_begin, block_end,
                         static_cast<hipStream_t>(stream));
}

int bagua_mxfp4_reduce_requantize_range(int dtype, const uint8_t* input, size_t input_bytes, int chunk_size,
                                        int num_chunks, int average, uint8_t* output, size_t output_bytes,
                                        int target_chunk, int block_begin, int block_end, bagua_stream_t stream) {
    if (block_begin < 0) return BAGUA_ERR_INVALID_ARG;
    return mx_reduce_requantize(dtype, input, input_bytes, chunk_size, num_chunks, nullptr, average, output,
                                output_bytes, target_chunk, block_begin, block_end, nullptr,
                                static_cast<hipStream_t>(stream));
}

// ---- stochastic rounding (MXFP4.md, "Stochastic rounding") ----
uint64_t bagua_mxfp4_sr_key(uint64_t seed, uint64_t step, int rank, int stage) {
    return mx_sr_key(seed, step, (uint32_t)rank, (uint32_t)stage);
}

uint32_t bagua_mxfp4_sr_word(uint64_t key, uint32_t pair_index) {
    return mx_sr_word((uint32_t)key, (uint32_t)(key >> 32), pair_index);
}

int bagua_mxfp4_compress_sr(int dtype, const void* input, int input_num_element, int chunk_size, int num_chunks,
                            uint8_t* output, size_t output_bytes, int target_chunk, uint64_t key,
                            bagua_stream_t stream) {
    return mx_compress(dtype, input, input_num_element, chunk_size, num_chunks, output, output_bytes, target_chunk,
                       kMxWhole, kMxWhole, &key, static_cast<hipStream_t>(stream));
}

int bagua_mxfp4_compress_sr_range(int dtype, const void* input, int input_num_element, int chunk_size, int num_chunks,
                                  uint8_t* output, size_t output_bytes, int block_begin, int block_end, uint64_t key,
                                  bagua_stream_t stream) {
    if (block_begin < 0) return BAGUA_ERR_INVALID_ARG;
    return mx_compress(dtype, input, input_num_element, chunk_size, num_chunks, output, output_bytes, -1,
                       block_begin, block_end, &key, static_cast<hipStream_t>(stream));
}

int bagua_mxfp4_reduce_requantize_sr(int dtype, const uint8_t* input, size_t input_bytes, int chunk_size,
                                     int num_chunks, int average, uint8_t* output, size_t output_bytes,
                                     int target_chunk, uint64_t key, bagua_stream_t stream) {
    return mx_reduce_requantize(dtype, input, input_bytes, chunk_size, num_chunks, nullptr, average, output,
                                output_bytes, target_chunk, kMxWhole, kMxWhole, &key,
                                static_cast<hipStream_t>(stream));
}

int bagua_mxfp4_reduce_requantize_sr_range(int dtype, const uint8_t* input, size_t input_bytes, int chunk_size,
                                           int num_chunks, int average, uint8_t* output, size_t output_bytes,
                                           int target_chunk, int block_begin, int block_end, uint64_t key,
                                           bagua_stream_t stream) {
    if (block_begin < 0) return BAGUA_ERR_INVALID_ARG;
    return mx_reduce_requantize(dtype, input, input_bytes, chunk_size, num_chunks, nullptr, average, output,
                                output_bytes, target_chunk, block_begin, block_end, &key,
                                static_cast<hipStream_t>(stream));
}

}  // extern "C"
