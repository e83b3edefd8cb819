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
//
// The kernels here are compositions of the steps in mxfp4_device.hpp, which mxfp4_ring.hip
// shares: the tile load of one tensor, the lane's part of a cooperative block encode, the
// store of a block's result with the slack rule, the decode-and-tree-sum of one block of the
// received segments, the residual of a block.  What is left in this file is each kernel's
// geometry, its order of steps, the error-feedback residual rule and the launchers.
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
#pragma unroll
        for (int k = 0; k < 4; ++k) w[k] = mx_quant_lane<8, kMxHw>(x + 8 * k, byte, maxf);
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
        mx_load_tile<T, true>(src, b0, lane, n, vec && (b0 + TB) * kMxBlock <= n, f);
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const uint32_t am = mx_block_amax<N>(f[k]);
            const int64_t b = b0 + k * BW + lb;
            if (b >= nb) continue;
            uint32_t byte, w;
            mx_encode_lane<N, mx_round(HW, SR)>(f[k], am, maxf, byte, w,
                                                (uint32_t)((int64_t)c * cs + (bb + b0 + k * BW) * kMxBlock + lane * N), k0, k1);
            mx_store_lane<N>(seg, pay, b, sub, byte, w, nb, bb, last, sbytes, pbytes);
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
        mx_reduce_block<T, BY, HW>(in, segb, sbytes, b, p, average, pf, cs, x);
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
        mx_store_block(out_seg, pay_out, b, byte, w, nb, sbytes, pbytes);
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
        mx_load_tile<T, true>(src, b0, lane, cs, vecx && full, f);
        mx_load_tile<F32, NT>(rsd, b0, lane, cs, vecr && full, r);
#pragma unroll
        for (int k = 0; k < R; ++k) {
#pragma unroll
            for (int e = 0; e < N; ++e) r[k][e] = mx_ef_sum(f[k][e], r[k][e]);  // v, and below the new residual
            const uint32_t am = mx_block_amax<N>(r[k]);
            const int64_t b = b0 + k * BW + lb;
            if (b >= nb) continue;
            uint32_t byte, w;
            mx_encode_lane<N, mx_round(HW)>(r[k], am, maxf, byte, w);
            if (byte != kMxNanScale) {
                mx_residual<T, HW, N>(r[k], &w, byte, maxf);
            } else {  // a NaN block: the state is reset
#pragma unroll
                for (int e = 0; e < N; ++e) r[k][e] = 0.0f;
            }
            mx_store_lane<N>(seg, pay, b, sub, byte, w, nb, 0, true, sbytes, pbytes);
            mx_store_row<NT>(rsd, (b0 + k * BW) * kMxBlock + lane * N, cs, vecr && full, r[k]);
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
        mx_reduce_block<T, BY, HW>(in, segb, sbytes, b, p, average, pf, cs, x);
        const bool whole = vec && (b + 1) * kMxBlock <= cs;
        mx_add_residual(x, res, b, cs, whole);
        uint32_t byte, w[4];
        mx_encode<HW>(x, maxf, byte, w);
        mx_store_block(out_seg, pay_out, b, byte, w, nb, sbytes, pbytes);
        if (byte != kMxNanScale) {
            mx_residual<T, HW, kMxBlock>(x, w, byte, maxf);
        } else {
#pragma unroll
            for (int e = 0; e < kMxBlock; ++e) x[e] = 0.0f;
        }
        mx_store_row<false>(res, b * kMxBlock, cs, whole, x);
    }
}

// ------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------
// mx_hw(), mx_grid() and the shared argument checks: mxfp4_device.hpp; the dispatch
// helpers (with_dtype / _bool / _by): codec_common.hpp

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
    if (!mx_counts_ok(p, cs, kMxGridChunks) || in_num_elem < 0 || target < -1 || target >= p || !out || !input)
        return BAGUA_ERR_INVALID_ARG;
    if (!mx_holds(out_bytes, cs, p) || !mx_aligned(out, 16)) return BAGUA_ERR_INVALID_ARG;
    if (!mx_range(cs, bb, be)) return BAGUA_ERR_INVALID_ARG;
    if (bb == be) return BAGUA_OK;
    // a wave tile is 8 KiB of input, a workgroup four of them; the grid covers the range
    constexpr int64_t kTileBlocks = kMxItemBytes * kWave / (int64_t)sizeof(S) / kMxBlock;
    const int nact = target < 0 ? p : 1;
    const dim3 grid(mx_grid(((int64_t)(be - bb) + kTileBlocks - 1) / kTileBlocks, kWavesPerBlock, nact,
                            "BAGUA_TUNE_MX_ENCODE_BLOCKS"),
                    nact);
    auto go = [&](auto kern) {
        launch(kern, grid, dim3(kBlock), 0, s, static_cast<const S*>(input), (int64_t)in_num_elem, (int64_t)cs, target,
               out, (int64_t)bb, (int64_t)be, key ? (uint32_t)*key : 0u, key ? (uint32_t)(*key >> 32) : 0u);
    };
    if (key) go(mxfp4_encode_kernel<T, false, true>);  // stochastic: the arithmetic alone (MXFP4.md, "The hardware conversion")
    else if (mx_hw()) go(mxfp4_encode_kernel<T, true, false>);
    else go(mxfp4_encode_kernel<T, false, false>);
    return check_launch();
}

template <typename T>
static int mx_decompress_impl(const uint8_t* in, size_t in_bytes, int cs, int p, void* out, int bb, int be,
                              hipStream_t s) {
    using S = typename T::storage;
    if (!mx_counts_ok(p, cs, kMxGridChunks) || !in || !out) return BAGUA_ERR_INVALID_ARG;
    if (!mx_holds(in_bytes, cs, p) || !mx_aligned(in, 4)) return BAGUA_ERR_INVALID_ARG;
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
    with_bool(mx_hw(), [&](auto hw) {
        with_bool(nt, [&](auto nts) {
            launch(mxfp4_decode_kernel<T, decltype(hw)::value, decltype(nts)::value>, grid, dim3(kBlock), 0, s, in,
                   (int64_t)cs, static_cast<S*>(out), (int64_t)bb, (int64_t)be);
        });
    });
    return check_launch();
}

// What the two middle steps check alike, in their order of precedence; the error-feedback one
// checks its residual first, which gives the code of the first line here.
static int mx_check_middle(const uint8_t* recv, size_t recv_bytes, int cs, int p, const uint8_t* out, size_t out_bytes,
                           int target) {
    if (!mx_counts_ok(p, cs) || target < 0 || target >= p || !recv || !out) return BAGUA_ERR_INVALID_ARG;
    if (p > kMaxFusedChunks) return BAGUA_ERR_UNSUPPORTED;  // caller runs decompress + reduce + compress
    if (!mx_holds(recv_bytes, cs, p) || !mx_holds(out_bytes, cs, p)) return BAGUA_ERR_INVALID_ARG;
    if (!mx_aligned(recv, 4) || !mx_aligned(out, 16)) return BAGUA_ERR_INVALID_ARG;
    return BAGUA_OK;
}

template <typename T>
static int mx_reduce_requantize_impl(const uint8_t* recv, size_t recv_bytes, int cs, int p, void* tensor, int average,
                                     uint8_t* out, size_t out_bytes, int target, int bb, int be, const uint64_t* key,
                                     hipStream_t s) {
    using S = typename T::storage;
    if (const int e = mx_check_middle(recv, recv_bytes, cs, p, out, out_bytes, target)) return e;
    if (!mx_range(cs, bb, be)) return BAGUA_ERR_INVALID_ARG;
    if (bb == be) return BAGUA_OK;
    S* chunk = tensor ? static_cast<S*>(tensor) + (int64_t)target * cs : nullptr;  // nullptr: not stored
    uint8_t* seg = out + (size_t)target * (size_t)mx_segment_bytes(cs);
    const int blocks = mx_grid(be - bb, kBlock, 1, "BAGUA_TUNE_MX_MIDDLE_BLOCKS");
    const uint32_t jc = key ? (uint32_t)((int64_t)target * cs) : 0u;  // index of the own chunk's first element
    with_by(p, [&](auto by) {
        with_bool(mx_hw(), [&](auto hw) {
            constexpr int BY = decltype(by)::value;
            constexpr bool HW = decltype(hw)::value;
            auto go = [&](auto kern) {
                launch(kern, dim3(blocks), dim3(kBlock), 0, s, recv, (int64_t)cs, p, average, chunk, seg, (int64_t)bb,
                       (int64_t)be, jc, key ? (uint32_t)*key : 0u, key ? (uint32_t)(*key >> 32) : 0u);
            };
            // stochastic re-encode (never storing); the decode of the received segments is the plain one
            if (key) go(mxfp4_reduce_encode_kernel<T, BY, HW, false, true>);
            else if (chunk) go(mxfp4_reduce_encode_kernel<T, BY, HW, true, false>);
            else go(mxfp4_reduce_encode_kernel<T, BY, HW, false, false>);
        });
    });
    return check_launch();
}

// ---- error feedback ----
template <typename T>
static int mx_compress_ef_impl(const void* input, int in_num_elem, int cs, int p, uint8_t* out, size_t out_bytes,
                               int target, float* residual, hipStream_t s) {
    using S = typename T::storage;
    if (!mx_counts_ok(p, cs, kMxGridChunks) || target != -1 || !out || !input) return BAGUA_ERR_INVALID_ARG;
    if ((int64_t)in_num_elem != (int64_t)cs * p) return BAGUA_ERR_INVALID_ARG;  // every chunk fully valid
    if (!mx_residual_ok(residual)) return BAGUA_ERR_INVALID_ARG;
    if (!mx_holds(out_bytes, cs, p) || !mx_aligned(out, 16)) return BAGUA_ERR_INVALID_ARG;
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
    with_bool(mx_hw(), [&](auto hw) {
        with_bool(nt, [&](auto ntr) {
            launch(mxfp4_encode_ef_kernel<T, decltype(hw)::value, decltype(ntr)::value>, grid, dim3(kBlock), 0, s,
                   static_cast<const S*>(input), (int64_t)cs, residual, out);
        });
    });
    return check_launch();
}

template <typename T>
static int mx_reduce_requantize_ef_impl(const uint8_t* recv, size_t recv_bytes, int cs, int p, int average,
                                        uint8_t* out, size_t out_bytes, int target, float* residual, hipStream_t s) {
    if (!mx_residual_ok(residual)) return BAGUA_ERR_INVALID_ARG;
    if (const int e = mx_check_middle(recv, recv_bytes, cs, p, out, out_bytes, target)) return e;
    if (cs == 0) return BAGUA_OK;
    uint8_t* seg = out + (size_t)target * (size_t)mx_segment_bytes(cs);
    const int blocks = mx_grid(mx_blocks(cs), kBlock, 1, "BAGUA_TUNE_MX_MIDDLE_BLOCKS");
    with_by(p, [&](auto by) {
        with_bool(mx_hw(), [&](auto hw) {
            launch(mxfp4_reduce_encode_ef_kernel<T, decltype(by)::value, decltype(hw)::value>, dim3(blocks),
                   dim3(kBlock), 0, s, recv, (int64_t)cs, p, average, residual, seg);
        });
    });
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
    return with_dtype(dtype, [&](auto t) {
        return mx_compress_ef_impl<decltype(t)>(input, input_num_element, chunk_size, num_chunks, output, output_bytes,
                                                target_chunk, residual, static_cast<hipStream_t>(stream));
    });
}

int bagua_mxfp4_reduce_requantize_ef(int dtype, const uint8_t* input, size_t input_bytes, int chunk_size,
                                     int num_chunks, int average, uint8_t* output, size_t output_bytes,
                                     int target_chunk, float* residual, bagua_stream_t stream) {
    return with_dtype(dtype, [&](auto t) {
        return mx_reduce_requantize_ef_impl<decltype(t)>(input, input_bytes, chunk_size, num_chunks, average, output,
                                                         output_bytes, target_chunk, residual,
                                                         static_cast<hipStream_t>(stream));
    });
}

size_t bagua_mxfp4_compressed_bytes(int chunk_size, int num_chunks) {
    if (chunk_size < 0 || num_chunks < 0) return 0;
    return (size_t)num_chunks * (size_t)mx_segment_bytes(chunk_size);
}

// the whole-chunk entries are the range [0, nb) (kMxWhole) of the range entries' code
static int mx_compress(int dtype, const void* input, int input_num_element, int chunk_size, int num_chunks,
                       uint8_t* output, size_t output_bytes, int target_chunk, int bb, int be, const uint64_t* key,
                       hipStream_t s) {
    return with_dtype(dtype, [&](auto t) {
        return mx_compress_impl<decltype(t)>(input, input_num_element, chunk_size, num_chunks, output, output_bytes,
                                             target_chunk, bb, be, key, s);
    });
}

static int mx_decompress(int dtype, const uint8_t* input, size_t input_bytes, int chunk_size, int num_chunks,
                         void* output, int bb, int be, hipStream_t s) {
    return with_dtype(dtype, [&](auto t) {
        return mx_decompress_impl<decltype(t)>(input, input_bytes, chunk_size, num_chunks, output, bb, be, s);
    });
}

static int mx_reduce_requantize(int dtype, const uint8_t* input, size_t input_bytes, int chunk_size, int num_chunks,
                                void* tensor, int average, uint8_t* output, size_t output_bytes, int target_chunk,
                                int bb, int be, const uint64_t* key, hipStream_t s) {
    return with_dtype(dtype, [&](auto t) {
        return mx_reduce_requantize_impl<decltype(t)>(input, input_bytes, chunk_size, num_chunks, tensor, average,
                                                      output, output_bytes, target_chunk, bb, be, key, s);
    });
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
