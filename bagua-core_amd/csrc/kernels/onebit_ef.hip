// onebit_ef.hip — error feedback for the 1-bit sign + scale codec (DESIGN.md §4,
// "error feedback").  The wire format is onebit.hip's, unchanged; what is new is
// caller-owned f32 state that carries each step's quantisation error into the next:
//
//   worker: carry[N] and scale[p] (one per chunk);  server: carry2[cs] and scale2[1]
//
// The carry is LAZY: it holds the compensated value v of the previous step, not the
// residual.  The residual is rebuilt from the carry and the previous scale,
//
//   d = as_stored<T>(k < 0 ? -s : +s)   what the receiver decoded for this element
//   r = k - d                           the previous step's residual
//   v = x + r                           compensated value; carry = v, in place
//   bit = v < 0;  |v| enters the scale tree where |x| does in the plain encode
//
// so the encode stays one pass (the scale of this step is known only after its
// tree; a materialised residual would need a second sweep, 8N more bytes).  The
// segment is byte-identical to the plain encode of v as an f32 array, and with
// zero state v = x: the plain encode's bytes.
#include <cstdint>
#include <type_traits>

#include "onebit_common.hpp"

namespace bagua {

// grid cap of the worker encode: one tile per wave up to 1 GiB of f32, as the plain encode
constexpr int kObEfEncodeBlocks = 65536;

// the lazy-carry rule for one element (dpos / dneg: +-scale as stored in T)
__device__ __forceinline__ float ef_compensate(float x, float k, float dpos, float dneg) {
    const float d = k < 0.0f ? dneg : dpos;
    const float r = k - d;
    return x + r;
}

// ------------------------------------------------------------------------
// worker encode: onebit_encode_kernel's tile layout (one wave per 1024-element
// tile, the lane's 16 sign bits in registers, odd_neighbour pairing, the DPP
// tree) on v = x + (carry - decoded), with the carry rewritten in place.
// Every chunk is fully valid (the op refuses partly valid tensors).
//
// Tiles per iteration: ONE for every T.  The carry is 16 B per lane per sub-tile
// whatever T is, so a tile already has 128 B (f32) / 96 B (16-bit) of loads in
// flight per lane -- more than the plain encode's 64 -- and one tile compiles to
// 70 VGPRs (f32, 7 waves per SIMD) / 62 (16-bit, 8 waves); two 16-bit tiles would
// hold 48 VGPRs of raw loads plus 32 of compensated values, past the 64-VGPR step
// and on towards the 96 one.
//
// scale[c] is read here while onebit_finalize_ef_kernel writes it: both run on
// the op's main stream, every piece's encode before the one finalize of the
// step, so an encode always sees the previous step's scale.
// ------------------------------------------------------------------------
template <typename T, bool NT>
__global__ __launch_bounds__(kBlock) void onebit_encode_ef_kernel(
    const typename T::storage* __restrict__ in, int64_t cs, float* __restrict__ carry,
    const float* __restrict__ scales, uint8_t* __restrict__ out, int64_t chunk_offset, float* __restrict__ partials,
    int64_t tiles_per_chunk, int64_t t_begin, int64_t t_end) {
    using S = typename T::storage;
    const int c = (int)blockIdx.y;
    const S* src = in + (int64_t)c * cs;
    float* kc = carry + (int64_t)c * cs;
    const bool vec = ((uintptr_t)src % (4 * sizeof(S))) == 0 && ((uintptr_t)kc % 16) == 0;
    uint8_t* bits = out + (int64_t)c * chunk_offset + 32;
    float* part = partials + (int64_t)c * tiles_per_chunk;
    // the previous step's scale of this chunk, uniform over the wave, and the two
    // values the receiver decoded with it
    const float s = scales[c];
    const float dpos = as_stored<T>(s), dneg = as_stored<T>(-s);
    const int lane = lane_id();
    const int64_t wave = grid_wave();
    const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
    for (int64_t t = t_begin + wave; t < t_end; t += nwaves) {
        float v[4][4];
        if (vec && (t + 1) * kObTile <= cs) {
            // full tiles: every load of the iteration issued before any is used
            using L = std::conditional_t<sizeof(S) == 4, uint4, uint2>;
            L raw[4];
            uint4 kraw[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const S* p = src + t * kObTile + k * 256 + lane * 4;
                if constexpr (sizeof(S) == 4) raw[k] = nt_load16(p);
                else raw[k] = nt_load8(p);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float* q = kc + t * kObTile + k * 256 + lane * 4;
                kraw[k] = NT ? nt_load16(q) : *reinterpret_cast<const uint4*>(q);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float x[4], kk[4];
                unpack4<T>(raw[k], x);
                unpack4<F32>(kraw[k], kk);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[k][e] = ef_compensate(x[e], kk[e], dpos, dneg);
                const uint4 w = make_uint4(__float_as_uint(v[k][0]), __float_as_uint(v[k][1]), __float_as_uint(v[k][2]),
                                           __float_as_uint(v[k][3]));
                float* q = kc + t * kObTile + k * 256 + lane * 4;
                if constexpr (NT) nt_store16(w, q);
                else *reinterpret_cast<uint4*>(q) = w;
            }
        } else {
            // ragged last tile of the chunk, or a chunk that does not start on 16 B:
            // guarded; padding past cs contributes 0 and touches no state
            const bool xvec = ((uintptr_t)src % (4 * sizeof(S))) == 0, kvec = ((uintptr_t)kc % 16) == 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t j = t * kObTile + k * 256 + lane * 4;
                float x[4], kk[4];
                load4<T>(src, j, cs, xvec, x);
                load4<F32>(kc, j, cs, kvec, kk);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[k][e] = j + e < cs ? ef_compensate(x[e], kk[e], dpos, dneg) : 0.0f;
                store4<F32, false>(kc, j, cs, kvec, v[k]);
            }
        }
        ob_emit_tile(v, bits, part, t, lane);
    }
}

// ------------------------------------------------------------------------
// finalize with the scale store: onebit_finalize_kernel's header and slack, and
// the chunk's new scale into the state (scale_out[c]; one slot when one chunk is
// targeted) for the next step's encode
// ------------------------------------------------------------------------
__global__ __launch_bounds__(kObFinalizeThreads) void onebit_finalize_ef_kernel(
    const float* __restrict__ partials, int64_t tiles_per_chunk, int64_t in_num_elem, int64_t cs, int target,
    uint8_t* __restrict__ out, int64_t chunk_offset, int64_t out_bytes, int num_chunks, float* __restrict__ scale_out) {
    __shared__ float lvl[2][2048];
    const float scale = ob_finalize(partials, tiles_per_chunk, in_num_elem, cs, target, out, chunk_offset, out_bytes,
                                    num_chunks, lvl);
    if (threadIdx.x == 0) scale_out[target < 0 ? blockIdx.x : 0] = scale;
}

// ------------------------------------------------------------------------
// server middle step: onebit_reduce_encode_kernel (decode the p received
// segments of the own chunk, reduce in the reference's tree order, round to T)
// with the carry rule applied to the reduced value before it is re-encoded.
// The reduced chunk is never stored (the op's final decode rewrites it).
// Padding past cs contributes 0 and touches no state.
// ------------------------------------------------------------------------
template <typename T, int BY, bool AVG>
__global__ __launch_bounds__(kBlock) void onebit_reduce_encode_ef_kernel(
    const uint8_t* __restrict__ in, int64_t chunk_offset, int64_t cs, int p, float* __restrict__ carry2,
    const float* __restrict__ scale2, uint8_t* __restrict__ out_seg, float* __restrict__ part) {
    __shared__ float pos[kMaxFusedChunks], neg[kMaxFusedChunks];
    ob_scale_tables<T>(in, chunk_offset, p, pos, neg);
    __syncthreads();
    const float s2 = scale2[0];
    const float dpos = as_stored<T>(s2), dneg = as_stored<T>(-s2);
    const int lane = lane_id();
    const int64_t tiles = (cs + kObTile - 1) / kObTile;
    const int64_t wave = grid_wave();
    const int64_t nwaves = (int64_t)gridDim.x * kWavesPerBlock;
    const float pf = (float)p;
    uint8_t* bits = out_seg + 32;
    for (int64_t t = wave; t < tiles; t += nwaves) {
        // the carry of the tile first: its latency hides under the reduce below
        // (carry2 is 16-B aligned, so a lane's four elements are one load)
        float kk[4][4];
#pragma unroll
        for (int k = 0; k < 4; ++k) load4<F32>(carry2, t * kObTile + k * 256 + lane * 4, cs, true, kk[k]);
        // the BY-wide accumulation of onebit_reduce_encode_kernel, written out in both: as a
        // shared step it cost several instantiations an occupancy step
        float s[16][BY];
#pragma unroll
        for (int b = 0; b < 16; ++b)
#pragma unroll
            for (int y = 0; y < BY; ++y) s[b][y] = 0.0f;
        for (int r = 0; r * BY < p; ++r) {
            uint32_t f[BY];
#pragma unroll
            for (int y = 0; y < BY; ++y) {  // each lane's 16-bit field of every segment
                const int c = r * BY + y < p ? r * BY + y : p - 1;
                f[y] = reinterpret_cast<const uint16_t*>(in + (int64_t)c * chunk_offset + 32 + t * kObTileBytes)[lane];
            }
#pragma unroll
            for (int y = 0; y < BY; ++y) {
                const int c = r * BY + y;
                if (c >= p) break;
#pragma unroll
                for (int b = 0; b < 16; ++b) s[b][y] = s[b][y] + (((f[y] >> b) & 1u) ? neg[c] : pos[c]);
            }
        }
        float v[4][4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int b = k * 4 + e;
                tree_finish<BY>(s[b]);
                const int64_t j = t * kObTile + k * 256 + lane * 4 + e;
                // the reduced value as stored in T is this step's x
                const float x = as_stored<T>(AVG ? s[b][0] / pf : s[b][0]);
                v[k][e] = j < cs ? ef_compensate(x, kk[k][e], dpos, dneg) : 0.0f;
            }
            store4<F32, false>(carry2, t * kObTile + k * 256 + lane * 4, cs, true, v[k]);
        }
        ob_emit_tile(v, bits, part, t, lane);
    }
}

// ------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------
// stage 0: encode every tile + finalize; 1: encode tiles [t_begin, t_end) only;
// 2: finalize only (headers, slack and the new scales from the partials)
template <typename T>
static int ob_compress_ef_impl(const void* input, int in_num_elem, int cs, int p, uint8_t* out, size_t out_bytes,
                               void* ws, size_t ws_bytes, float* carry, float* scales, hipStream_t s, int stage = 0,
                               int64_t t_begin = 0, int64_t t_end = INT64_MAX) {
    using S = typename T::storage;
    if (p <= 0 || p > 65535 || cs < 0 || !out || (!input && stage != 2) || t_begin < 0 || t_end < t_begin)
        return BAGUA_ERR_INVALID_ARG;
    if ((int64_t)in_num_elem != (int64_t)cs * p) return BAGUA_ERR_INVALID_ARG;  // every chunk fully valid
    if (!ob_ef_state_ok(carry, scales)) return BAGUA_ERR_INVALID_ARG;
    const int64_t co = (int64_t)(out_bytes / (size_t)p);
    const int64_t tiles = ob_tiles(cs);
    if (const int e = ob_check_encode(out, co, tiles, ws, ws_bytes, p)) return e;
    float* partials = static_cast<float*>(ws);
    const int64_t tb = stage == 2 ? 0 : t_begin, te = stage == 2 ? tiles : (t_end < tiles ? t_end : tiles);
    if (stage != 2 && te > tb) {
        const dim3 grid(ob_blocks(te - tb, p, tune_int("BAGUA_TUNE_OB_EF_ENCODE_BLOCKS", kObEfEncodeBlocks)), p);
        // Carry policy by the state's size, as the plain decode's stores (ob_nt_by_size):
        // the next step's encode finds a carry of up to 256 MiB in the Infinity Cache
        with_bool(ob_nt_by_size((int64_t)cs * p * 4, "BAGUA_OB_EF_CARRY_NT"), [&](auto nt) {
            launch(onebit_encode_ef_kernel<T, decltype(nt)::value>, grid, dim3(kBlock), 0, s,
                   static_cast<const S*>(input), (int64_t)cs, carry, static_cast<const float*>(scales), out, co,
                   partials, tiles, tb, te);
        });
    }
    if (stage != 1)
        launch(onebit_finalize_ef_kernel, dim3(p), dim3(kObFinalizeThreads), 0, s, partials, tiles, (int64_t)in_num_elem,
               (int64_t)cs, -1, out, co, (int64_t)out_bytes, p, scales);
    return check_launch();
}

template <typename T>
static int ob_reduce_requantize_ef_impl(const uint8_t* recv, size_t recv_bytes, int cs, int p, int average,
                                        uint8_t* out, size_t out_bytes, int target, void* ws, size_t ws_bytes,
                                        float* carry2, float* scale2, hipStream_t s) {
    if (!ob_ef_state_ok(carry2, scale2)) return BAGUA_ERR_INVALID_ARG;
    // UNSUPPORTED: the caller runs decompress + reduce + the worker encode on the own chunk
    if (const int e = ob_check_middle(recv, recv_bytes, cs, p, out, out_bytes, target, ws, ws_bytes)) return e;
    const int64_t co_in = (int64_t)(recv_bytes / (size_t)p), co = (int64_t)(out_bytes / (size_t)p);
    const int64_t tiles = ob_tiles(cs);
    float* part = static_cast<float*>(ws);
    uint8_t* seg = out + (int64_t)target * co;
    if (tiles > 0) {
        const int blocks = ob_blocks(tiles, 1);
        with_by(p, [&](auto by) {
            with_bool(average != 0, [&](auto avg) {
                launch(onebit_reduce_encode_ef_kernel<T, decltype(by)::value, decltype(avg)::value>, dim3(blocks),
                       dim3(kBlock), 0, s, recv, co_in, (int64_t)cs, p, carry2, static_cast<const float*>(scale2), seg,
                       part);
            });
        });
    }
    // header + slack of the own segment and the new server scale
    launch(onebit_finalize_ef_kernel, dim3(1), dim3(kObFinalizeThreads), 0, s, part, tiles, (int64_t)p * cs, (int64_t)cs,
           target, out, co, (int64_t)out_bytes, p, scale2);
    return check_launch();
}

}  // namespace bagua

using namespace bagua;

extern "C" {

int bagua_onebit_ef_state_bytes(int chunk_size, int num_chunks, size_t* carry_bytes, size_t* scale_bytes) {
    if (chunk_size < 0 || num_chunks <= 0 || !carry_bytes || !scale_bytes) return BAGUA_ERR_INVALID_ARG;
    *carry_bytes = (size_t)chunk_size * (size_t)num_chunks * sizeof(float);
    *scale_bytes = (size_t)num_chunks * sizeof(float);
    return BAGUA_OK;
}

// the error-feedback entries answer INVALID_ARG for U8, I64, U64 and unknown dtype codes;
// the whole-chunk entry is stage 0 / every tile of the range entry's code
static int ob_compress_ef(int dtype, const void* input, int input_num_element, int chunk_size, int num_chunks,
                          uint8_t* output, size_t output_bytes, void* workspace, size_t workspace_bytes, float* carry,
                          float* scales, bagua_stream_t stream, int stage, int64_t tile_begin, int64_t tile_end) {
    return with_dtype(
        dtype,
        [&](auto t) {
            return ob_compress_ef_impl<decltype(t)>(input, input_num_element, chunk_size, num_chunks, output,
                                                    output_bytes, workspace, workspace_bytes, carry, scales,
                                                    static_cast<hipStream_t>(stream), stage, tile_begin, tile_end);
        },
        BAGUA_ERR_INVALID_ARG);
}

int bagua_onebit_compress_ef(int dtype, const void* input, int input_num_element, int chunk_size, int num_chunks,
                             uint8_t* output, size_t output_bytes, void* workspace, size_t workspace_bytes,
                             int target_chunk, float* carry, float* scales, bagua_stream_t stream) {
    if (target_chunk != -1) return BAGUA_ERR_INVALID_ARG;
    return ob_compress_ef(dtype, input, input_num_element, chunk_size, num_chunks, output, output_bytes, workspace,
                          workspace_bytes, carry, scales, stream, 0, 0, INT64_MAX);
}

int bagua_onebit_encode_range_ef(int dtype, const void* input, int input_num_element, int chunk_size, int num_chunks,
                                 uint8_t* output, size_t output_bytes, void* workspace, size_t workspace_bytes,
                                 int tile_begin, int tile_end, float* carry, const float* scales,
                                 bagua_stream_t stream) {
    return ob_compress_ef(dtype, input, input_num_element, chunk_size, num_chunks, output, output_bytes, workspace,
                          workspace_bytes, carry, const_cast<float*>(scales), stream, 1, tile_begin, tile_end);
}

int bagua_onebit_finalize_ef(const void* workspace, size_t workspace_bytes, int input_num_element, int chunk_size,
                             int num_chunks, uint8_t* output, size_t output_bytes, float* scales,
                             bagua_stream_t stream) {
    // the header math is dtype-independent (partials are f32); the carry is not touched
    // (`scales` stands in for it in the pointer check)
    return ob_compress_ef_impl<F32>(nullptr, input_num_element, chunk_size, num_chunks, output, output_bytes,
                                    const_cast<void*>(workspace), workspace_bytes, scales, scales,
                                    static_cast<hipStream_t>(stream), 2);
}

int bagua_onebit_reduce_requantize_ef(int dtype, const uint8_t* input, size_t input_bytes, int chunk_size,
                                      int num_chunks, int average, uint8_t* output, size_t output_bytes,
                                      int target_chunk, void* workspace, size_t workspace_bytes, float* carry,
                                      float* scale, bagua_stream_t stream) {
    return with_dtype(
        dtype,
        [&](auto t) {
            return ob_reduce_requantize_ef_impl<decltype(t)>(input, input_bytes, chunk_size, num_chunks, average,
                                                             output, output_bytes, target_chunk, workspace,
                                                             workspace_bytes, carry, scale,
                                                             static_cast<hipStream_t>(stream));
        },
        BAGUA_ERR_INVALID_ARG);
}

}  // extern "C"
