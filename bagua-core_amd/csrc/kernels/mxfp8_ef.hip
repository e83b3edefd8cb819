// mxfp8_ef.hip — error feedback for the MXFP8 codec (MXFP8.md, "Error feedback") on gfx950:
// the two encodes of the centralized op with an f32 residual read and rewritten in the same
// pass.  The rule of one block: mx8_encode_block_ef (mxfp8_common.hpp).
//
//   v = x + e;  vc = clamp(v);  (byte, codes) = the plain block encode of vc;
//   e' = vc - decode(codes, byte) as T stores it, or +0 for every element of a NaN block
//
// A block's decode is known where it is encoded, so the state is the residual alone and each
// encode stays one streaming kernel with no workspace, no LDS and no exchange between
// workgroups:
//   worker   mxfp8_encode_kernel's cooperative layout: a lane owns one 16-B gradient vector of
//            each of R blocks and the matching 16 B / 32 B of f32 residual; all loads of a tile
//            are issued before any is used; the 8 / 4 lanes of a block share the amax of v by
//            xor shuffles; the lane's 4 / 8 payload bytes leave as one word and are decoded
//            again from that word, in registers, for the residual, which goes back in place
//   server   mxfp8_reduce_encode_kernel's layout (never storing the reduced chunk): a lane owns
//            one block of the own chunk, reduces its p received versions in the reference's
//            tree order, adds the block's 32 residuals (eight 16-B vectors), encodes, stores
//            the block and writes the new residual back
// HW = true rounds to E4M3 with v_cvt_scalef32_pk_fp8_f32 and decodes the lane's own words with
// v_cvt_scalef32_pk_f32_fp8; HW = false is the arithmetic of mxfp8_common.hpp.  Same bytes and
// the same residual bits either way.
//
// Rows per wave tile of the worker step: 8 for f32, 4 for f16 / bf16 (MXFP8.md has the
// timings of 4 and 8 for each).  A 16-bit lane-vector carries twice the residual of an f32
// one, so both shapes have 192 B of loads per lane in flight.
//
// The kernels are compiled without the packed f32 VALU instructions (v_pk_add_f32,
// v_pk_mul_f32, v_pk_fma_f32), as mxfp8_ring.hip's and for its reason: the contract is bit
// equality of payload and residuals, and the residual is f32 adds and subtracts on
// neighbouring registers, which is what the compiler packs.
//
// Composed from the format-independent steps of mxfp4_device.hpp (tile load, block amax, row
// store, the residual add, grid) and the E4M3 steps of mxfp8_device.hpp, as they are.
#include <cstdint>

#include "codec_common.hpp"
#include "launch_util.hpp"
#include "mxfp4_device.hpp"
#include "mxfp8_common.hpp"
#include "mxfp8_device.hpp"

namespace bagua {

#if defined(__HIP_DEVICE_COMPILE__)
#define MX8EF_KERNEL __global__ __attribute__((target("no-packed-fp32-ops"))) __launch_bounds__(kBlock)
#else
#define MX8EF_KERNEL __global__ __launch_bounds__(kBlock)
#endif

// rows (16-B gradient loads in flight per lane) of the worker step's wave tile; the macros are
// for timing another value in a second build of the library (tools/mxfp8_ef_probe.py), not a switch
#ifndef BAGUA_MX8_EF_ROWS_F32
#define BAGUA_MX8_EF_ROWS_F32 8
#endif
#ifndef BAGUA_MX8_EF_ROWS_16
#define BAGUA_MX8_EF_ROWS_16 4
#endif
template <typename T>
constexpr int kMx8EfRows = sizeof(typename T::storage) == 4 ? BAGUA_MX8_EF_ROWS_F32 : BAGUA_MX8_EF_ROWS_16;

// NE compensated values v of a block without NaN and their just-encoded payload words w
// (element e in byte e % 4 of word e / 4) under the block's scale byte -> the new residual, in
// place.  d is the plain decode as T stores it, read back as f32: mx8_decode already rounds it
// to T, so what mx_ef_residual<K> has left to do is its subtraction (K = f32: d as it is).
template <typename T, bool HW, int NE>
__device__ __forceinline__ void mx8_residual(float (&v)[NE], const uint32_t (&w)[NE / 4], uint32_t byte, float maxf) {
    uint32_t u[NE];
    mx8_decode<T, HW, NE>(w, byte, u);
#pragma unroll
    for (int e = 0; e < NE; ++e)
        v[e] = mx_ef_residual<BAGUA_DTYPE_F32>(mx_clamp(v[e], maxf), from_stored_bits<T>(u[e]));
}

// ------------------------------------------------------------------------
// Worker step.  Every chunk is fully valid.  Gradient loads are non-temporal as the plain
// encode's; the residual's loads and stores are non-temporal when NT (the host picks by what
// the step streams).  Chunks whose gradient or residual is not 16-B aligned, and ragged
// tiles, take guarded element accesses.
// ------------------------------------------------------------------------
template <typename T, bool HW, bool NT>
MX8EF_KERNEL void mxfp8_encode_ef_kernel(const typename T::storage* __restrict__ in, int64_t cs,
                                         float* __restrict__ res, uint8_t* __restrict__ out) {
    using S = typename T::storage;
    constexpr int N = Vec<T>::N;      // elements per 16-B gradient vector: 4 / 8
    constexpr int G = kMxBlock / N;   // lanes per block: 8 / 4
    constexpr int BW = kWave / G;     // blocks per wave-wide load: 8 / 16
    constexpr int R = kMx8EfRows<T>;  // rows per tile
    constexpr int TB = R * BW;        // blocks per wave tile
    const int c = (int)blockIdx.y;
    const S* src = in + (int64_t)c * cs;
    float* rsd = res + (int64_t)c * cs;
    const bool vecx = ((uintptr_t)src % 16) == 0, vecr = ((uintptr_t)rsd % 16) == 0;
    const int64_t nb = mx_blocks(cs), sbytes = mx_scale_bytes(cs);
    uint8_t* seg = out + (int64_t)c * mx8_segment_bytes(cs);
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
            const uint32_t am = mx_block_amax<N>(r[k]);  // every lane of the wave shuffles
            const int64_t b = b0 + k * BW + lb;
            if (b >= nb) continue;
            uint32_t byte, w[N / 4];
            mx8_encode_lane<N, HW>(r[k], am, maxf, byte, w);
            if (byte != kMxNanScale) {
                mx8_residual<T, HW, N>(r[k], w, byte, maxf);
            } else {  // a NaN block: the state is reset
#pragma unroll
                for (int e = 0; e < N; ++e) r[k][e] = 0.0f;
            }
            mx8_store_lane<N>(seg, pay, b, sub, byte, w, nb, 0, true, sbytes);
            mx_store_row<NT>(rsd, (b0 + k * BW) * kMxBlock + lane * N, cs, vecr && full, r[k]);
        }
    }
}

// ------------------------------------------------------------------------
// Server step: the own chunk's block reduced as mxfp8_reduce_encode_kernel does (mx8_reduce_block:
// 16 elements of every segment at a time for BY = 2 and 4, 8 for BY = 8), compensated with the
// server residual and encoded; a residual that is only 4-B aligned and the ragged last block
// take element accesses.
// ------------------------------------------------------------------------
template <typename T, int BY, bool HW>
MX8EF_KERNEL void mxfp8_reduce_encode_ef_kernel(const uint8_t* __restrict__ in, int64_t cs, int p, int average,
                                                float* __restrict__ res, uint8_t* __restrict__ out_seg) {
    const int64_t nb = mx_blocks(cs), sbytes = mx_scale_bytes(cs);
    const int64_t segb = mx8_segment_bytes(cs);
    uint8_t* pay_out = out_seg + sbytes;
    const bool vec = ((uintptr_t)res % 16) == 0;
    const float pf = (float)p, maxf = T::init_max();
    for (int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x; b < nb; b += (int64_t)gridDim.x * kBlock) {
        float x[kMxBlock];
        mx8_reduce_block<T, BY, HW>(in, segb, sbytes, b, p, average, pf, cs, x);
        const bool whole = vec && (b + 1) * kMxBlock <= cs;
        mx_add_residual(x, res, b, cs, whole);
        uint32_t byte, w[8];
        mx8_encode_whole<HW>(x, maxf, byte, w);
        mx8_store_block(out_seg, pay_out, b, byte, w, nb, sbytes);
        if (byte != kMxNanScale) {
            mx8_residual<T, HW, kMxBlock>(x, w, byte, maxf);
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
template <typename T>
static int mx8_compress_ef_impl(const void* input, int in_num_elem, int cs, int p, uint8_t* out, size_t out_bytes,
                                int target, float* residual, hipStream_t s) {
    using S = typename T::storage;
    if (!mx_counts_ok(p, cs, kMxGridChunks) || target != -1 || !out || !input) return BAGUA_ERR_INVALID_ARG;
    if ((int64_t)in_num_elem != (int64_t)cs * p) return BAGUA_ERR_INVALID_ARG;  // every chunk fully valid
    if (!mx_residual_ok(residual)) return BAGUA_ERR_INVALID_ARG;
    if (!mx8_holds(out_bytes, cs, p) || !mx_aligned(out, 16)) return BAGUA_ERR_INVALID_ARG;
    if (cs == 0) return BAGUA_OK;
    // a wave tile is R wave-wide rows of 1 KiB of gradient, a workgroup four of them
    constexpr int64_t kTileElems = (int64_t)kMx8EfRows<T> * 16 * kWave / (int64_t)sizeof(S);
    const dim3 grid(mx_grid(((int64_t)cs + kTileElems - 1) / kTileElems, kWavesPerBlock, p, "BAGUA_TUNE_MX8_ENCODE_BLOCKS"),
                    p);
    // Residual policy: MXFP4's rule (mxfp4.hip) and its A/B switch, by what the step streams,
    // gradient plus residual: up to the 256 MiB Infinity Cache default-policy accesses, past it
    // non-temporal ones.  Both policies are timed in profiles/r15_mxfp8_ef.json (MXFP8.md).
    const int env = tune_int("BAGUA_MX_EF_RESIDUAL_NT", -1);
    const bool nt = env >= 0 ? env != 0 : (int64_t)cs * p * (4 + (int64_t)sizeof(S)) > ((int64_t)256 << 20);
    with_bool(mx8_hw(), [&](auto hw) {
        with_bool(nt, [&](auto ntr) {
            launch(mxfp8_encode_ef_kernel<T, decltype(hw)::value, decltype(ntr)::value>, grid, dim3(kBlock), 0, s,
                   static_cast<const S*>(input), (int64_t)cs, residual, out);
        });
    });
    return check_launch();
}

template <typename T>
static int mx8_reduce_requantize_ef_impl(const uint8_t* recv, size_t recv_bytes, int cs, int p, int average,
                                         uint8_t* out, size_t out_bytes, int target, float* residual, hipStream_t s) {
    // the residual first, then the plain middle step's checks in its order
    if (!mx_residual_ok(residual)) return BAGUA_ERR_INVALID_ARG;
    if (!mx_counts_ok(p, cs) || target < 0 || target >= p || !recv || !out) return BAGUA_ERR_INVALID_ARG;
    if (p > kMaxFusedChunks) return BAGUA_ERR_UNSUPPORTED;  // caller runs decompress + reduce + compress_ef
    if (!mx8_holds(recv_bytes, cs, p) || !mx8_holds(out_bytes, cs, p)) return BAGUA_ERR_INVALID_ARG;
    if (!mx_aligned(recv, 16) || !mx_aligned(out, 16)) return BAGUA_ERR_INVALID_ARG;  // 16-B payload loads and stores
    if (cs == 0) return BAGUA_OK;
    uint8_t* seg = out + (size_t)target * (size_t)mx8_segment_bytes(cs);
    const int blocks = mx_grid(mx_blocks(cs), kBlock, 1, "BAGUA_TUNE_MX8_MIDDLE_BLOCKS");
    with_by(p, [&](auto by) {
        with_bool(mx8_hw(), [&](auto hw) {
            launch(mxfp8_reduce_encode_ef_kernel<T, decltype(by)::value, decltype(hw)::value>, dim3(blocks),
                   dim3(kBlock), 0, s, recv, (int64_t)cs, p, average, residual, seg);
        });
    });
    return check_launch();
}

}  // namespace bagua

using namespace bagua;

extern "C" {

int bagua_mxfp8_ef_state_bytes(int chunk_size, int num_chunks, size_t* worker_bytes, size_t* server_bytes) {
    if (chunk_size < 0 || num_chunks <= 0 || !worker_bytes || !server_bytes) return BAGUA_ERR_INVALID_ARG;
    *worker_bytes = (size_t)chunk_size * (size_t)num_chunks * sizeof(float);
    *server_bytes = (size_t)chunk_size * sizeof(float);
    return BAGUA_OK;
}

int bagua_mxfp8_compress_ef(int dtype, const void* input, int input_num_element, int chunk_size, int num_chunks,
                            uint8_t* output, size_t output_bytes, int target_chunk, float* residual,
                            bagua_stream_t stream) {
    return with_dtype(dtype, [&](auto t) {
        return mx8_compress_ef_impl<decltype(t)>(input, input_num_element, chunk_size, num_chunks, output,
                                                 output_bytes, target_chunk, residual,
                                                 static_cast<hipStream_t>(stream));
    });
}

int bagua_mxfp8_reduce_requantize_ef(int dtype, const uint8_t* input, size_t input_bytes, int chunk_size,
                                     int num_chunks, int average, uint8_t* output, size_t output_bytes,
                                     int target_chunk, float* residual, bagua_stream_t stream) {
    return with_dtype(dtype, [&](auto t) {
        return mx8_reduce_requantize_ef_impl<decltype(t)>(input, input_bytes, chunk_size, num_chunks, average, output,
                                                          output_bytes, target_chunk, residual,
                                                          static_cast<hipStream_t>(stream));
    });
}

}  // extern "C"
