// mxfp6_ef.hip — error feedback for the MXFP6 codec (MXFP6.md, "Error feedback") on gfx950:
// the two encodes of the centralized op with an f32 residual read and rewritten in the same
// pass.  The rule of one block: mx6_encode_block_ef (mxfp6_common.hpp).
//
//   v = x + e;  vc = clamp(v);  (byte, codes) = the plain block encode of vc;
//   e' = vc - decode(codes, byte) as T stores it, or +0 for every element of a NaN block
//
// A block's decode is known where it is encoded, so the state is the residual alone and each
// encode stays one streaming kernel with no workspace, no LDS and no exchange between
// workgroups.  What the 6-bit packing changes against mxfp8_ef.hip: a lane's 24 / 48 code bits
// are no aligned word and leave only after a quad move into the group's three words
// (mx6_store_lane), so the residual is taken before that move, from the lane's own field:
//   worker   mxfp6_encode_kernel's cooperative layout: a lane owns one 16-B gradient vector of
//            each of R blocks and the matching 16 B / 32 B of f32 residual; all loads of a tile
//            are issued before any is used; the 8 / 4 lanes of a block share the amax of v by
//            xor shuffles; the lane's codes are decoded again at bit 0 of its own field, in
//            registers, for the residual; then the quad move, three of four lanes store an
//            aligned word, and the residual goes back in place
//   server   mxfp6_reduce_encode_kernel's layout (never storing the reduced chunk): a lane owns
//            one block of the own chunk, reduces its p received versions in the reference's
//            tree order, adds the block's 32 residuals (eight 16-B vectors), encodes to six
//            words, stores them as three 8-B words, decodes the six words for the residual and
//            writes it back
//
// Rows per wave tile of the worker step: 8 for f32, 4 for f16 / bf16, MXFP8's.  A 16-bit
// lane-vector carries twice the residual of an f32 one, so both shapes have 192 B of loads per
// lane in flight.
//
// The kernels are compiled without the packed f32 VALU instructions (v_pk_add_f32,
// v_pk_mul_f32, v_pk_fma_f32), as mxfp8_ef.hip's and for its reason: the contract is bit
// equality of payload and residuals, and the residual is f32 adds and subtracts on
// neighbouring registers, which is what the compiler packs.
//
// Composed from the format-independent steps of mxfp4_device.hpp (tile load, block amax, row
// store, the residual add, grid) and the E2M3 steps of mxfp6_device.hpp, as they are.
#include <cstdint>

#include "codec_common.hpp"
#include "launch_util.hpp"
#include "mxfp4_device.hpp"
#include "mxfp6_common.hpp"
#include "mxfp6_device.hpp"

namespace bagua {

#if defined(__HIP_DEVICE_COMPILE__)
#define MX6EF_KERNEL __global__ __attribute__((target("no-packed-fp32-ops"))) __launch_bounds__(kBlock)
#else
#define MX6EF_KERNEL __global__ __launch_bounds__(kBlock)
#endif

// rows (16-B gradient loads in flight per lane) of the worker step's wave tile
template <typename T>
constexpr int kMx6EfRows = sizeof(typename T::storage) == 4 ? 8 : 4;

// NE compensated values v of a block without NaN and their just-encoded codes, code e in bits
// [6 e, 6 e + 6) of the words w (a lane's own field or a whole block's six words), under the
// block's scale byte -> the new residual, in place.  d is the plain decode as T stores it, read
// back as f32: mx6_decode already rounds it to T, so what mx_ef_residual<K> has left to do is
// its subtraction (K = f32: d as it is).
template <typename T, int NE, int NW>
__device__ __forceinline__ void mx6_residual(float (&v)[NE], const uint32_t (&w)[NW], uint32_t byte, float maxf) {
    uint32_t u[NE];
    mx6_decode<T, NE>(w, 0, byte, u);
#pragma unroll
    for (int e = 0; e < NE; ++e)
        v[e] = mx_ef_residual<BAGUA_DTYPE_F32>(mx_clamp(v[e], maxf), from_stored_bits<T>(u[e]));
}

// ------------------------------------------------------------------------
// Worker step.  Every chunk is fully valid.  Gradient loads are non-temporal as the plain
// encode's; the residual's loads and stores are non-temporal when NT (the host picks by what
// the step streams).  Chunks whose gradient or residual is not 16-B aligned, and ragged
// tiles, take guarded element accesses; the segment stores are the same either way.  Only
// whole blocks are dropped past the chunk's end, so whole groups of four lanes reach the
// quad move of mx6_store_lane.
// ------------------------------------------------------------------------
template <typename T, bool NT>
MX6EF_KERNEL void mxfp6_encode_ef_kernel(const typename T::storage* __restrict__ in, int64_t cs,
                                         float* __restrict__ res, uint8_t* __restrict__ out) {
    using S = typename T::storage;
    constexpr int N = Vec<T>::N;      // elements per 16-B gradient vector: 4 / 8
    constexpr int G = kMxBlock / N;   // lanes per block: 8 / 4, whole groups of four
    constexpr int BW = kWave / G;     // blocks per wave-wide load: 8 / 16
    constexpr int R = kMx6EfRows<T>;  // rows per tile
    constexpr int TB = R * BW;        // blocks per wave tile
    const int c = (int)blockIdx.y;
    const S* src = in + (int64_t)c * cs;
    float* rsd = res + (int64_t)c * cs;
    const bool vecx = ((uintptr_t)src % 16) == 0, vecr = ((uintptr_t)rsd % 16) == 0;
    const int64_t nb = mx_blocks(cs), sbytes = mx_scale_bytes(cs), pbytes = mx6_payload_bytes(cs);
    uint8_t* seg = out + (int64_t)c * mx6_segment_bytes(cs);
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
            if (b >= nb) continue;  // whole blocks, so whole groups of four lanes
            uint32_t byte, code[N / 4];
            mx6_encode_lane<N>(r[k], am, maxf, byte, code);
            if (byte != kMxNanScale) {  // the same for every lane of the block
                mx6_residual<T, N>(r[k], code, byte, maxf);
            } else {  // a NaN block: the state is reset
#pragma unroll
                for (int e = 0; e < N; ++e) r[k][e] = 0.0f;
            }
            mx6_store_lane<N>(seg, pay, b, sub, byte, code, nb, 0, true, sbytes, pbytes);
            mx_store_row<NT>(rsd, (b0 + k * BW) * kMxBlock + lane * N, cs, vecr && full, r[k]);
        }
    }
}

// ------------------------------------------------------------------------
// Server step: the own chunk's block reduced as mxfp6_reduce_encode_kernel does
// (mx6_reduce_block: 16 elements of every segment at a time for BY = 2 and 4, 8 for BY = 8),
// compensated with the server residual and encoded; a residual that is only 4-B aligned and
// the ragged last block take element accesses.  The six payload words leave before they are
// decoded again, so x, the words and the decode are what is live in the residual pass.
// ------------------------------------------------------------------------
template <typename T, int BY>
MX6EF_KERNEL void mxfp6_reduce_encode_ef_kernel(const uint8_t* __restrict__ in, int64_t cs, int p, int average,
                                                float* __restrict__ res, uint8_t* __restrict__ out_seg) {
    const int64_t nb = mx_blocks(cs), sbytes = mx_scale_bytes(cs), pbytes = mx6_payload_bytes(cs);
    const int64_t segb = mx6_segment_bytes(cs);
    uint8_t* pay_out = out_seg + sbytes;
    const bool vec = ((uintptr_t)res % 16) == 0;
    const float pf = (float)p, maxf = T::init_max();
    for (int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x; b < nb; b += (int64_t)gridDim.x * kBlock) {
        float x[kMxBlock];
        mx6_reduce_block<T, BY>(in, segb, sbytes, b, p, average, pf, cs, x);
        const bool whole = vec && (b + 1) * kMxBlock <= cs;
        mx_add_residual(x, res, b, cs, whole);
        uint32_t byte, w[kMx6BlockWords];
        mx6_encode_block(x, maxf, byte, w);
        mx6_store_block(out_seg, pay_out, b, byte, w, nb, sbytes, pbytes);
        if (byte != kMxNanScale) {
            mx6_residual<T, kMxBlock>(x, w, byte, maxf);
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
static int mx6_compress_ef_impl(const void* input, int in_num_elem, int cs, int p, uint8_t* out, size_t out_bytes,
                                int target, float* residual, hipStream_t s) {
    using S = typename T::storage;
    if (!mx_counts_ok(p, cs, kMxGridChunks) || target != -1 || !out || !input) return BAGUA_ERR_INVALID_ARG;
    if ((int64_t)in_num_elem != (int64_t)cs * p) return BAGUA_ERR_INVALID_ARG;  // every chunk fully valid
    if (!mx_residual_ok(residual)) return BAGUA_ERR_INVALID_ARG;
    if (!mx6_holds(out_bytes, cs, p) || !mx_aligned(out, 16)) return BAGUA_ERR_INVALID_ARG;  // 8-B payload words
    if (cs == 0) return BAGUA_OK;
    // a wave tile is R wave-wide rows of 1 KiB of gradient, a workgroup four of them
    constexpr int64_t kTileElems = (int64_t)kMx6EfRows<T> * 16 * kWave / (int64_t)sizeof(S);
    const dim3 grid(mx_grid(((int64_t)cs + kTileElems - 1) / kTileElems, kWavesPerBlock, p, "BAGUA_TUNE_MX6_ENCODE_BLOCKS"),
                    p);
    // Residual policy: MXFP4's rule (mxfp4.hip) and its A/B switch, by what the step streams,
    // gradient plus residual: up to the 256 MiB Infinity Cache default-policy accesses, past it
    // non-temporal ones.
    const int env = tune_int("BAGUA_MX_EF_RESIDUAL_NT", -1);
    const bool nt = env >= 0 ? env != 0 : (int64_t)cs * p * (4 + (int64_t)sizeof(S)) > ((int64_t)256 << 20);
    with_bool(nt, [&](auto ntr) {
        launch(mxfp6_encode_ef_kernel<T, decltype(ntr)::value>, grid, dim3(kBlock), 0, s, static_cast<const S*>(input),
               (int64_t)cs, residual, out);
    });
    return check_launch();
}

template <typename T>
static int mx6_reduce_requantize_ef_impl(const uint8_t* recv, size_t recv_bytes, int cs, int p, int average,
                                         uint8_t* out, size_t out_bytes, int target, float* residual, hipStream_t s) {
    // the residual first, then the plain middle step's checks in its order
    if (!mx_residual_ok(residual)) return BAGUA_ERR_INVALID_ARG;
    if (!mx_counts_ok(p, cs) || target < 0 || target >= p || !recv || !out) return BAGUA_ERR_INVALID_ARG;
    if (p > kMaxFusedChunks) return BAGUA_ERR_UNSUPPORTED;  // caller runs decompress + reduce + compress_ef
    if (!mx6_holds(recv_bytes, cs, p) || !mx6_holds(out_bytes, cs, p)) return BAGUA_ERR_INVALID_ARG;
    if (!mx_aligned(recv, 16) || !mx_aligned(out, 16)) return BAGUA_ERR_INVALID_ARG;  // 4-B payload loads, 8-B stores
    if (cs == 0) return BAGUA_OK;
    uint8_t* seg = out + (size_t)target * (size_t)mx6_segment_bytes(cs);
    const int blocks = mx_grid(mx_blocks(cs), kBlock, 1, "BAGUA_TUNE_MX6_MIDDLE_BLOCKS");
    with_by(p, [&](auto by) {
        launch(mxfp6_reduce_encode_ef_kernel<T, decltype(by)::value>, dim3(blocks), dim3(kBlock), 0, s, recv,
               (int64_t)cs, p, average, residual, seg);
    });
    return check_launch();
}

}  // namespace bagua

using namespace bagua;

extern "C" {

int bagua_mxfp6_ef_state_bytes(int chunk_size, int num_chunks, size_t* worker_bytes, size_t* server_bytes) {
    if (chunk_size < 0 || num_chunks <= 0 || !worker_bytes || !server_bytes) return BAGUA_ERR_INVALID_ARG;
    *worker_bytes = (size_t)chunk_size * (size_t)num_chunks * sizeof(float);
    *server_bytes = (size_t)chunk_size * sizeof(float);
    return BAGUA_OK;
}

int bagua_mxfp6_compress_ef(int dtype, const void* input, int input_num_element, int chunk_size, int num_chunks,
                            uint8_t* output, size_t output_bytes, int target_chunk, float* residual,
                            bagua_stream_t stream) {
    return with_dtype(dtype, [&](auto t) {
        return mx6_compress_ef_impl<decltype(t)>(input, input_num_element, chunk_size, num_chunks, output,
                                                 output_bytes, target_chunk, residual,
                                                 static_cast<hipStream_t>(stream));
    });
}

int bagua_mxfp6_reduce_requantize_ef(int dtype, const uint8_t* input, size_t input_bytes, int chunk_size,
                                     int num_chunks, int average, uint8_t* output, size_t output_bytes,
                                     int target_chunk, float* residual, bagua_stream_t stream) {
    return with_dtype(dtype, [&](auto t) {
        return mx6_reduce_requantize_ef_impl<decltype(t)>(input, input_bytes, chunk_size, num_chunks, average, output,
                                                          output_bytes, target_chunk, residual,
                                                          static_cast<hipStream_t>(stream));
    });
}

}  // extern "C"
