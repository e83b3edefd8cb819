// mxfp8.hip — block-scaled 8-bit gradient codec (OCP MXFP8: 32 E4M3 elements under one
// power-of-two scale byte) for gfx950.  Format and rules: MXFP8.md; the arithmetic of one
// block: mxfp8_common.hpp.
//
// Every block is self-contained, so all three kernels are single streaming passes with no
// workspace, no LDS and no exchange between workgroups:
//   encode   a lane owns one 16-B input vector (4 f32 / 8 16-bit elements) of each of eight
//            blocks, loaded together, so a wave's loads are contiguous; the 8 / 4 lanes of a
//            block share its amax by xor shuffles; 4 / 8 payload bytes per lane, one store
//   decode   a lane owns one 16-B output vector (4 / 8 payload bytes in), four vectors per
//            iteration, so a wave's stores are contiguous
//   middle   (centralized op) a lane owns one block of the own chunk: it decodes the p
//            received versions sixteen elements (one 16-B load) at a time, sums them in the
//            reference's tree order (reduce.hip), rounds to T and encodes the 32 results
//
// HW = true takes gfx950's conversions (v_cvt_scalef32_pk_fp8_f32 / _pk_f32_fp8) for the
// rounding to and from E4M3; the scale byte, NaN blocks, magnitude 0x7F, the inf and
// largest-finite clamps and the rounding to T stay in the arithmetic of mxfp8_common.hpp.
//
// The kernels are compositions of the format-independent steps of mxfp4_device.hpp (tile
// load, block amax, grid and argument checks) and the E4M3 steps of mxfp8_device.hpp.
#include <algorithm>
#include <cstdint>

#include "codec_common.hpp"
#include "launch_util.hpp"
#include "mxfp4_device.hpp"
#include "mxfp8_common.hpp"
#include "mxfp8_device.hpp"

namespace bagua {

constexpr int kMx8ItemBytes = 128;  // input bytes a lane of the encode has in flight per iteration
constexpr int kMx8DecodeVecs = 4;   // 16-B output vectors per lane per decode iteration
// blocks between two piece boundaries, as MXFP4's: one wave tile of the 16-bit encode, two
// of the f32 encode; 128 scale bytes, 4 KiB of payload, 4096 elements
constexpr int kMx8Granule = 128;

__device__ __forceinline__ int64_t mx8_valid(int64_t in_num_elem, int64_t cs, int c) {
    const int64_t r = in_num_elem - (int64_t)c * cs;
    return r < 0 ? 0 : (r < cs ? r : cs);
}

// ------------------------------------------------------------------------
// encode: one wave owns a tile of 8 KiB of input as eight wave-wide loads of 1 KiB, issued
// together (nt: read once), the layout the 4-bit encode settled on (MXFP4.md, "Kernels").
// All three kernels work on blocks [bb, be) of their chunks (the whole chunk is [0, nb)):
// bb is a multiple of kMx8Granule, be another or nb, so a range starts on a wave tile of
// every kernel and only the range that ends at nb has a ragged tile and the slack.
// ------------------------------------------------------------------------
template <typename T, bool HW>
__global__ __launch_bounds__(kBlock) void mxfp8_encode_kernel(const typename T::storage* __restrict__ in,
                                                             int64_t in_num_elem, int64_t cs, int target,
                                                             uint8_t* __restrict__ out, int64_t bb, int64_t be) {
    using S = typename T::storage;
    constexpr int N = Vec<T>::N;           // elements per 16-B vector: 4 / 8
    constexpr int G = kMxBlock / N;        // lanes per block: 8 / 4
    constexpr int BW = kWave / G;          // blocks per wave-wide load: 8 / 16
    constexpr int R = kMx8ItemBytes / 16;  // loads in flight per lane
    constexpr int TB = R * BW;             // blocks per wave tile (8 KiB of input)
    const int c = target < 0 ? (int)blockIdx.y : target;
    const int64_t sbytes = mx_scale_bytes(cs);
    // everything below is relative to block bb of the chunk: the range's nb blocks, its n
    // valid elements, their source, scale bytes and payload
    const int64_t nb = be - bb, n = max(mx8_valid(in_num_elem, cs, c) - bb * kMxBlock, (int64_t)0);
    const S* src = in + (int64_t)c * cs + bb * kMxBlock;
    const bool vec = ((uintptr_t)src % 16) == 0;
    uint8_t* seg = out + (int64_t)c * mx8_segment_bytes(cs) + bb;
    uint8_t* pay = seg + (sbytes - bb) + bb * kMx8BlockBytes;
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
            uint32_t byte, w[N / 4];
            mx8_encode_lane<N, HW>(f[k], am, maxf, byte, w);
            mx8_store_lane<N>(seg, pay, b, sub, byte, w, nb, bb, last, sbytes);
        }
    }
}

// ------------------------------------------------------------------------
// decode
// ------------------------------------------------------------------------
template <typename T, bool HW, bool NTS>
__global__ __launch_bounds__(kBlock) void mxfp8_decode_kernel(const uint8_t* __restrict__ in, int64_t cs,
                                                             typename T::storage* __restrict__ out, int64_t bb,
                                                             int64_t be) {
    using S = typename T::storage;
    constexpr int N = Vec<T>::N;
    constexpr int KV = kMx8DecodeVecs;
    const int c = blockIdx.y;
    const int64_t sbytes = mx_scale_bytes(cs);
    // relative to block bb of the chunk: scale bytes, payload, output and the range's n elements
    const uint8_t* seg = in + (int64_t)c * mx8_segment_bytes(cs) + bb;
    const uint8_t* pay = seg + (sbytes - bb) + bb * kMx8BlockBytes;
    S* dst = out + (int64_t)c * cs + bb * kMxBlock;
    const bool vec = ((uintptr_t)dst % 16) == 0;
    const int64_t n = min(cs, be * kMxBlock) - bb * kMxBlock;
    const int64_t nvec = (n + N - 1) / N;
    for (int64_t v0 = (int64_t)blockIdx.x * (kBlock * KV) + threadIdx.x; v0 < nvec;
         v0 += (int64_t)gridDim.x * (kBlock * KV)) {
        uint32_t w[KV][N / 4], sb[KV];
#pragma unroll
        for (int k = 0; k < KV; ++k) {
            const int64_t j = (v0 + k * kBlock) * N;
            sb[k] = 0;
#pragma unroll
            for (int h = 0; h < N / 4; ++h) w[k][h] = 0;
            if (v0 + k * kBlock < nvec) {  // the payload covers whole blocks, so the whole word is there
                sb[k] = seg[j / kMxBlock];
                if constexpr (N == 4) {
                    w[k][0] = *reinterpret_cast<const uint32_t*>(pay + j);
                } else {
                    const uint2 q = *reinterpret_cast<const uint2*>(pay + j);
                    w[k][0] = q.x;
                    w[k][1] = q.y;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < KV; ++k) {
            const int64_t j = (v0 + k * kBlock) * N;
            if (v0 + k * kBlock >= nvec) break;
            uint32_t u[N];
            mx8_decode<T, HW, N>(w[k], sb[k], u);
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
// fused middle step of the centralized op: decode the p received segments of the own chunk,
// reduce them as bagua_reduce_chunks does, round to T and encode the result into the own
// segment.  Equal, byte for byte, to decompress + bagua_reduce_chunks + compress(target).
// ------------------------------------------------------------------------
template <typename T, int BY, bool HW, bool STORE>
__global__ __launch_bounds__(kBlock) void mxfp8_reduce_encode_kernel(const uint8_t* __restrict__ in, int64_t cs, int p,
                                                                    int average,
                                                                    typename T::storage* __restrict__ chunk,
                                                                    uint8_t* __restrict__ out_seg, int64_t bb,
                                                                    int64_t be) {
    constexpr int N = Vec<T>::N;
    const int64_t nb = mx_blocks(cs), sbytes = mx_scale_bytes(cs);
    const int64_t segb = mx8_segment_bytes(cs);
    uint8_t* pay_out = out_seg + sbytes;
    const bool vec = STORE && ((uintptr_t)chunk % 16) == 0;
    const float pf = (float)p, maxf = T::init_max();
    for (int64_t b = bb + (int64_t)blockIdx.x * kBlock + threadIdx.x; b < be; b += (int64_t)gridDim.x * kBlock) {
        float x[kMxBlock];
        mx8_reduce_block<T, BY, HW>(in, segb, sbytes, b, p, average, pf, cs, x);
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
        uint32_t byte, w[8];
        mx8_encode_whole<HW>(x, maxf, byte, w);
        mx8_store_block(out_seg, pay_out, b, byte, w, nb, sbytes);
    }
}

// ------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------
// A block range [bb, be) of a chunk of cs elements as the range entries take it: bb a
// multiple of the granule in [0, nb], be in [bb, nb] and either nb or a multiple of it.
// The whole-chunk entries pass kMx8Whole for [0, nb).
constexpr int kMx8Whole = -1;
static bool mx8_range(int cs, int& bb, int& be) {
    const int nb = (int)mx_blocks(cs);
    if (bb == kMx8Whole && be == kMx8Whole) {
        bb = 0;
        be = nb;
        return true;
    }
    return bb >= 0 && bb <= nb && bb % kMx8Granule == 0 && be >= bb && be <= nb && (be == nb || be % kMx8Granule == 0);
}

template <typename T>
static int mx8_compress_impl(const void* input, int in_num_elem, int cs, int p, uint8_t* out, size_t out_bytes,
                             int target, int bb, int be, hipStream_t s) {
    using S = typename T::storage;
    if (!mx_counts_ok(p, cs, kMxGridChunks) || in_num_elem < 0 || target < -1 || target >= p || !out || !input)
        return BAGUA_ERR_INVALID_ARG;
    if (!mx8_holds(out_bytes, cs, p) || !mx_aligned(out, 16)) return BAGUA_ERR_INVALID_ARG;
    if (!mx8_range(cs, bb, be)) return BAGUA_ERR_INVALID_ARG;
    if (bb == be) return BAGUA_OK;
    // a wave tile is 8 KiB of input, a workgroup four of them; the grid covers the range
    constexpr int64_t kTileBlocks = kMx8ItemBytes * kWave / (int64_t)sizeof(S) / kMxBlock;
    const int nact = target < 0 ? p : 1;
    const dim3 grid(mx_grid(((int64_t)(be - bb) + kTileBlocks - 1) / kTileBlocks, kWavesPerBlock, nact,
                            "BAGUA_TUNE_MX8_ENCODE_BLOCKS"),
                    nact);
    with_bool(mx8_hw(), [&](auto hw) {
        launch(mxfp8_encode_kernel<T, decltype(hw)::value>, grid, dim3(kBlock), 0, s, static_cast<const S*>(input),
               (int64_t)in_num_elem, (int64_t)cs, target, out, (int64_t)bb, (int64_t)be);
    });
    return check_launch();
}

template <typename T>
static int mx8_decompress_impl(const uint8_t* in, size_t in_bytes, int cs, int p, void* out, int bb, int be,
                               hipStream_t s) {
    using S = typename T::storage;
    if (!mx_counts_ok(p, cs, kMxGridChunks) || !in || !out) return BAGUA_ERR_INVALID_ARG;
    if (!mx8_holds(in_bytes, cs, p) || !mx_aligned(in, 8)) return BAGUA_ERR_INVALID_ARG;  // payload read as 8-B words
    if (!mx8_range(cs, bb, be)) return BAGUA_ERR_INVALID_ARG;
    if (bb == be) return BAGUA_OK;
    // store policy by the bucket's size (not the range's), as the other decodes': past the 256 MiB
    // Infinity Cache the dirty lines cannot stay on chip
    const bool nt = (int64_t)cs * p * (int64_t)sizeof(S) > ((int64_t)256 << 20);
    constexpr int N = Vec<T>::N;
    const int64_t last = std::min(((int64_t)cs + N - 1) / N, (int64_t)be * (kMxBlock / N));
    const int64_t nvec = last - (int64_t)bb * (kMxBlock / N);  // the range's 16-B output vectors
    const dim3 grid(mx_grid(nvec, kBlock * kMx8DecodeVecs, p, "BAGUA_TUNE_MX8_DECODE_BLOCKS"), p);
    with_bool(mx8_hw(), [&](auto hw) {
        with_bool(nt, [&](auto nts) {
            launch(mxfp8_decode_kernel<T, decltype(hw)::value, decltype(nts)::value>, grid, dim3(kBlock), 0, s, in,
                   (int64_t)cs, static_cast<S*>(out), (int64_t)bb, (int64_t)be);
        });
    });
    return check_launch();
}

template <typename T>
static int mx8_reduce_requantize_impl(const uint8_t* recv, size_t recv_bytes, int cs, int p, void* tensor, int average,
                                      uint8_t* out, size_t out_bytes, int target, int bb, int be, hipStream_t s) {
    using S = typename T::storage;
    if (!mx_counts_ok(p, cs) || target < 0 || target >= p || !recv || !out) return BAGUA_ERR_INVALID_ARG;
    if (p > kMaxFusedChunks) return BAGUA_ERR_UNSUPPORTED;  // caller runs decompress + reduce + compress
    if (!mx8_holds(recv_bytes, cs, p) || !mx8_holds(out_bytes, cs, p)) return BAGUA_ERR_INVALID_ARG;
    if (!mx_aligned(recv, 16) || !mx_aligned(out, 16)) return BAGUA_ERR_INVALID_ARG;  // 16-B payload loads and stores
    if (!mx8_range(cs, bb, be)) return BAGUA_ERR_INVALID_ARG;
    if (bb == be) return BAGUA_OK;
    S* chunk = tensor ? static_cast<S*>(tensor) + (int64_t)target * cs : nullptr;  // nullptr: not stored
    uint8_t* seg = out + (size_t)target * (size_t)mx8_segment_bytes(cs);
    const int blocks = mx_grid(be - bb, kBlock, 1, "BAGUA_TUNE_MX8_MIDDLE_BLOCKS");
    with_by(p, [&](auto by) {
        with_bool(mx8_hw(), [&](auto hw) {
            with_bool(chunk != nullptr, [&](auto st) {
                launch(mxfp8_reduce_encode_kernel<T, decltype(by)::value, decltype(hw)::value, decltype(st)::value>,
                       dim3(blocks), dim3(kBlock), 0, s, recv, (int64_t)cs, p, average, chunk, seg, (int64_t)bb,
                       (int64_t)be);
            });
        });
    });
    return check_launch();
}

}  // namespace bagua

using namespace bagua;

extern "C" {

size_t bagua_mxfp8_compressed_bytes(int chunk_size, int num_chunks) {
    if (chunk_size < 0 || num_chunks < 0) return 0;
    return (size_t)num_chunks * (size_t)mx8_segment_bytes(chunk_size);
}

// the whole-chunk entries are the range [0, nb) (kMx8Whole) of the range entries' code
static int mx8_compress(int dtype, const void* input, int input_num_element, int chunk_size, int num_chunks,
                        uint8_t* output, size_t output_bytes, int target_chunk, int bb, int be, hipStream_t s) {
    return with_dtype(dtype, [&](auto t) {
        return mx8_compress_impl<decltype(t)>(input, input_num_element, chunk_size, num_chunks, output, output_bytes,
                                              target_chunk, bb, be, s);
    });
}

static int mx8_decompress(int dtype, const uint8_t* input, size_t input_bytes, int chunk_size, int num_chunks,
                          void* output, int bb, int be, hipStream_t s) {
    return with_dtype(dtype, [&](auto t) {
        return mx8_decompress_impl<decltype(t)>(input, input_bytes, chunk_size, num_chunks, output, bb, be, s);
    });
}

static int mx8_reduce_requantize(int dtype, const uint8_t* input, size_t input_bytes, int chunk_size, int num_chunks,
                                 void* tensor, int average, uint8_t* output, size_t output_bytes, int target_chunk,
                                 int bb, int be, hipStream_t s) {
    return with_dtype(dtype, [&](auto t) {
        return mx8_reduce_requantize_impl<decltype(t)>(input, input_bytes, chunk_size, num_chunks, tensor, average,
                                                       output, output_bytes, target_chunk, bb, be, s);
    });
}

int bagua_mxfp8_compress(int dtype, const void* input, int input_num_element, int chunk_size, int num_chunks,
                         uint8_t* output, size_t output_bytes, int target_chunk, bagua_stream_t stream) {
    return mx8_compress(dtype, input, input_num_element, chunk_size, num_chunks, output, output_bytes, target_chunk,
                        kMx8Whole, kMx8Whole, static_cast<hipStream_t>(stream));
}

int bagua_mxfp8_decompress(int dtype, const uint8_t* input, size_t input_bytes, int chunk_size, int num_chunks,
                           void* output, bagua_stream_t stream) {
    return mx8_decompress(dtype, input, input_bytes, chunk_size, num_chunks, output, kMx8Whole, kMx8Whole,
                          static_cast<hipStream_t>(stream));
}

int bagua_mxfp8_reduce_requantize(int dtype, const uint8_t* input, size_t input_bytes, int chunk_size, int num_chunks,
                                  void* tensor, int average, uint8_t* output, size_t output_bytes, int target_chunk,
                                  bagua_stream_t stream) {
    return mx8_reduce_requantize(dtype, input, input_bytes, chunk_size, num_chunks, tensor, average, output,
                                 output_bytes, target_chunk, kMx8Whole, kMx8Whole, static_cast<hipStream_t>(stream));
}

// ---- pieces (MXFP8.md, "Pipelined op") ----
// the same rule on the same blocks and granule as the 4-bit codec's
int bagua_mxfp8_piece_range(int chunk_size, int pieces, int piece, int* block_begin, int* block_end) {
    return bagua_mxfp4_piece_range(chunk_size, pieces, piece, block_begin, block_end);
}

int bagua_mxfp8_compress_range(int dtype, const void* input, int input_num_element, int chunk_size, int num_chunks,
                               uint8_t* output, size_t output_bytes, int block_begin, int block_end,
                               bagua_stream_t stream) {
    if (block_begin < 0) return BAGUA_ERR_INVALID_ARG;
    return mx8_compress(dtype, input, input_num_element, chunk_size, num_chunks, output, output_bytes, -1,
                        block_begin, block_end, static_cast<hipStream_t>(stream));
}

int bagua_mxfp8_decompress_range(int dtype, const uint8_t* input, size_t input_bytes, int chunk_size, int num_chunks,
                                 void* output, int block_begin, int block_end, bagua_stream_t stream) {
    if (block_begin < 0) return BAGUA_ERR_INVALID_ARG;
    return mx8_decompress(dtype, input, input_bytes, chunk_size, num_chunks, output, block_begin, block_end,
                          static_cast<hipStream_t>(stream));
}

int bagua_mxfp8_reduce_requantize_range(int dtype, const uint8_t* input, size_t input_bytes, int chunk_size,
                                        int num_chunks, int average, uint8_t* output, size_t output_bytes,
                                        int target_chunk, int block_begin, int block_end, bagua_stream_t stream) {
    if (block_begin < 0) return BAGUA_ERR_INVALID_ARG;
    return mx8_reduce_requantize(dtype, input, input_bytes, chunk_size, num_chunks, nullptr, average, output,
                                 output_bytes, target_chunk, block_begin, block_end, static_cast<hipStream_t>(stream));
}

}  // extern "C"
