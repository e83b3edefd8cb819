// onebit_common.hpp — device and launch helpers shared by the 1-bit codec kernels
// (onebit.hip, onebit_ef.hip): the lane-native tile layout, the fixed summation
// tree and its wave-level pieces.  Format: DESIGN.md §4.
#pragma once

#include <cstdint>
#include <type_traits>

#include "codec_common.hpp"
#include "launch_util.hpp"

namespace bagua {

constexpr int kObTile = 1024;
constexpr int kObTileBytes = 128;
constexpr int kObFinalizeThreads = 1024;
// encode / decode grid caps: 64 B of loads in flight per lane (one tile per
// iteration for 32-bit types, two for 16-bit ones).  Round 1 picked 1024 encode
// workgroups over 2048 (profiles/r01_onebit_shape_sweep.jsonl); round 3 found
// one tile per wave better still (16384 workgroups for 2^26 f32 elements):
// encode 45.8 -> 43.8 us, decode 42.7 -> 42.0 us per 256 MiB
// (tools/grid_sweep.py, profiles/r03_grid_sweep.jsonl); round 4 kept one tile per
// wave up to 1 GiB buckets (65536 workgroups): 1 GiB encode 186 -> 176 us, decode
// 193 -> 190 us, 256 MiB unchanged (profiles/r04_onebit_shape_sweep.jsonl)
constexpr int kObEncodeBlocks = 65536;
constexpr int kObDecodeBlocks = 65536;

__device__ __forceinline__ int64_t ob_valid(int64_t in_num_elem, int64_t cs, int c) {
    int64_t r = in_num_elem - (int64_t)c * cs;
    return r < 0 ? 0 : (r < cs ? r : cs);
}

// 4 consecutive elements of T starting at p (vector load when 4*sizeof(T)-aligned)
template <typename T>
__device__ __forceinline__ void load4(const typename T::storage* p, int64_t j, int64_t n, bool vec, float (&f)[4]) {
    using S = typename T::storage;
    if (vec && j + 4 <= n) {
        if constexpr (sizeof(S) == 4) {
            const uint4 v = nt_load16(p + j);
            f[0] = __uint_as_float(v.x); f[1] = __uint_as_float(v.y);
            f[2] = __uint_as_float(v.z); f[3] = __uint_as_float(v.w);
        } else {
            const uint2 v = nt_load8(p + j);
            f[0] = T::to_f((uint16_t)(v.x & 0xffff)); f[1] = T::to_f((uint16_t)(v.x >> 16));
            f[2] = T::to_f((uint16_t)(v.y & 0xffff)); f[3] = T::to_f((uint16_t)(v.y >> 16));
        }
        return;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) f[e] = (j + e < n) ? T::load(p, j + e) : 0.0f;
}

// 4 elements from one 16-B (f32) / 8-B (16-bit) load
template <typename T>
__device__ __forceinline__ void unpack4(const uint4& v, float (&f)[4]) {
    f[0] = __uint_as_float(v.x); f[1] = __uint_as_float(v.y);
    f[2] = __uint_as_float(v.z); f[3] = __uint_as_float(v.w);
}
template <typename T>
__device__ __forceinline__ void unpack4(const uint2& v, float (&f)[4]) {
    f[0] = T::to_f((uint16_t)(v.x & 0xffff)); f[1] = T::to_f((uint16_t)(v.x >> 16));
    f[2] = T::to_f((uint16_t)(v.y & 0xffff)); f[3] = T::to_f((uint16_t)(v.y >> 16));
}

template <typename T, bool NTS = true>
__device__ __forceinline__ void store4(typename T::storage* p, int64_t j, int64_t n, bool vec, const float (&f)[4]) {
    using S = typename T::storage;
    if (vec && j + 4 <= n) {
        if constexpr (sizeof(S) == 4) {
            const uint4 v = make_uint4(__float_as_uint(f[0]), __float_as_uint(f[1]), __float_as_uint(f[2]), __float_as_uint(f[3]));
            if constexpr (NTS) nt_store16(v, p + j);
            else *reinterpret_cast<uint4*>(p + j) = v;
        } else {
            uint2 v;
            v.x = (uint32_t)T::from_f(f[0]) | ((uint32_t)T::from_f(f[1]) << 16);
            v.y = (uint32_t)T::from_f(f[2]) | ((uint32_t)T::from_f(f[3]) << 16);
            if constexpr (NTS) nt_store8(v, p + j);
            else *reinterpret_cast<uint2*>(p + j) = v;
        }
        return;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (j + e < n) p[j + e] = T::from_f(f[e]);
}

// this wave's index in the grid, through readfirstlane so the compiler knows it (and every
// tile index and bound derived from it) is wave-uniform: scalar loop control and SGPR-based
// addresses instead of 64-bit VALU arithmetic and exec-mask branches per tile
__device__ __forceinline__ int64_t grid_wave() {
    return (int64_t)blockIdx.x * kWavesPerBlock + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
}

// the 64-lane tree of the tile sum: s[l] += s[l^h], h = 32..1 (== s[l] + s[l+h])
__device__ __forceinline__ float wave_tree_sum(float s) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s = s + __shfl_xor(s, o, kWave);
    return s;
}

// The same tree with its result in lane 0 only (the streaming kernels store lane 0's):
// s[l] += s[l+h] for h = 32, 16 by swapping halves across lanes (gfx950's permlane swaps),
// h = 8..1 by DPP row shifts -- no LDS round trip per level, and 8 instructions where the
// shuffles above take ~36 plus six ds_bpermute waits.  Every lane of the wave must be active
__device__ __forceinline__ float wave_tree_sum_lane0(float s) {
    s = s + __uint_as_float(__builtin_amdgcn_permlane32_swap(__float_as_uint(s), __float_as_uint(s), false, false)[1]);
    s = s + __uint_as_float(__builtin_amdgcn_permlane16_swap(__float_as_uint(s), __float_as_uint(s), false, false)[1]);
    s = s + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(s), 0x108, 0xf, 0xf, false));  // row_shl:8
    s = s + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(s), 0x104, 0xf, 0xf, false));  // row_shl:4
    s = s + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(s), 0x102, 0xf, 0xf, false));  // row_shl:2
    s = s + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(s), 0x101, 0xf, 0xf, false));  // row_shl:1
    return s;
}

// lane l + 1's value in even lanes l (an even lane and its odd neighbour share a DPP row)
__device__ __forceinline__ uint32_t odd_neighbour(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x101, 0xf, 0xf, false);  // row_shl:1
}

// lane-local part of the tile tree for values a[sub][e]
__device__ __forceinline__ float lane_tree(const float (&a)[4][4]) {
    float q[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = (a[k][0] + a[k][1]) + (a[k][2] + a[k][3]);
    return (q[0] + q[1]) + (q[2] + q[3]);
}

__device__ __forceinline__ float tile_from(const float* v, int64_t base, int64_t count, int lane) {
    float a[4][4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int64_t r = base + k * 256 + lane * 4 + e;
            const float x = v[r < count ? r : count - 1];  // clamped: no load waits behind a branch
            a[k][e] = r < count ? x : 0.0f;
        }
    return wave_tree_sum(lane_tree(a));
}

// Levels >= 2 of the chunk tree: lvl[0][0, ceil(m1 / 1024)) holds the level-1 group
// sums (published by a barrier); returns the root to every thread.
__device__ __forceinline__ float upper_tree(int64_t m1, float (&lvl)[2][2048]) {
    const int lane = lane_id(), wave = threadIdx.x / kWave, nw = kObFinalizeThreads / kWave;
    int cur = 0;
    bool done = m1 <= kObTile;
    int64_t m = (m1 + kObTile - 1) / kObTile;
    while (!done) {
        const int64_t g = (m + kObTile - 1) / kObTile;
        for (int64_t i = wave; i < g; i += nw) {
            const float s = tile_from(lvl[cur], i * kObTile, m, lane);
            if (lane == 0) lvl[cur ^ 1][i] = s;
        }
        __syncthreads();
        done = m <= kObTile;
        cur ^= 1;
        m = g;
    }
    return lvl[cur][0];
}

// The fixed 1024-tree over a chunk's m1 tile partials get(r), by one
// kObFinalizeThreads workgroup: level 1 -> 2 straight from `get` (each wave takes
// kFinBatch groups at once and issues all their loads before any tree, so the pass
// costs one memory latency instead of one per group),
// the higher levels in LDS.  Every thread returns the total (0 when m1 = 0).
template <typename Get>
__device__ __forceinline__ float chunk_tree(const Get& get, int64_t m1, float (&lvl)[2][2048]) {
    // the wave index through readfirstlane: the compiler then knows the group branches below
    // are wave-uniform (scalar branches, not exec masks)
    const int lane = lane_id(), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));
    const int nw = kObFinalizeThreads / kWave;
    if (m1 <= 0) return 0.0f;
    int64_t m = m1;
    const int64_t g1 = (m + kObTile - 1) / kObTile;
    constexpr int kFinBatch = 4;
    for (int64_t g0 = wave; g0 < g1; g0 += (int64_t)nw * kFinBatch) {
        float a[kFinBatch][4][4];
        if ((g0 + (int64_t)(kFinBatch - 1) * nw + 1) * kObTile <= m) {
            // every group of the batch is full: one base per group, immediate offsets
#pragma unroll
            for (int j = 0; j < kFinBatch; ++j) {
                const int64_t bj = (g0 + (int64_t)j * nw) * kObTile + lane * 4;
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int e = 0; e < 4; ++e) a[j][k][e] = get(bj + k * 256 + e);
            }
        } else {
        // otherwise per group, a wave-uniform branch: a full group's loads unconditional,
        // only the chunk's last, ragged group read element by element (guarded).  Guarded
        // loads for the whole batch are serialised by the compiler under this workgroup's
        // 128-VGPR budget: the finalize of 32 groups (one ragged batch) took 10.7 us, this
        // way 4.6; of 64 (one full batch) 5.3
#pragma unroll
        for (int j = 0; j < kFinBatch; ++j) {
            const int64_t g = g0 + (int64_t)j * nw;
            const int64_t bj = g * kObTile + lane * 4;
            if ((g + 1) * kObTile <= m) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int e = 0; e < 4; ++e) a[j][k][e] = get(bj + k * 256 + e);
            } else if (g * kObTile < m) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int64_t r = bj + k * 256 + e;
                        a[j][k][e] = r < m ? get(r) : 0.0f;
                    }
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int e = 0; e < 4; ++e) a[j][k][e] = 0.0f;
            }
        }
        }
#pragma unroll
        for (int j = 0; j < kFinBatch; ++j) {
            const int64_t g = g0 + (int64_t)j * nw;
            const float s = wave_tree_sum(lane_tree(a[j]));
            if (lane == 0 && g < g1) lvl[0][g] = s;
        }
    }
    __syncthreads();
    return upper_tree(m1, lvl);
}

// ------------------------------------------------------------------------
// The steps the 1-bit kernels are composed of, each stated once.  All of them are
// inlined into the tile loops and take their arrays by reference (the loops are
// tuned to a VGPR step: onebit_ef.hip's worker encode).
// ------------------------------------------------------------------------
// The two stores of a tile: even lanes store their 16-bit sign field and the odd neighbour's
// as one dword; lane 0 stores the tile's |v| partial.  wave_tree_sum_lane0 needs every lane
// of the wave active, so these stay outside any per-lane guard: padding past cs is zeroed
// values, never masked lanes
__device__ __forceinline__ void ob_store_field(uint32_t field, uint8_t* bits, int64_t t, int lane) {
    const uint32_t next = odd_neighbour(field);
    if ((lane & 1) == 0) reinterpret_cast<uint32_t*>(bits + t * kObTileBytes)[lane >> 1] = field | (next << 16);
}
__device__ __forceinline__ void ob_store_partial(float lane_sum, float* part, int64_t t, int lane) {
    const float s = wave_tree_sum_lane0(lane_sum);
    if (lane == 0) part[t] = s;
}
// tail of a tile for a lane that has its field and its part of the |v| tree already (the
// table kernel's fast paths)
__device__ __forceinline__ void ob_emit_field(uint32_t field, float lane_sum, uint8_t* bits, float* part, int64_t t,
                                              int lane) {
    ob_store_field(field, bits, t, lane);
    ob_store_partial(lane_sum, part, t, lane);
}

// the lane's 16 sign bits form its own 16-bit field (bit sub*4+e)
__device__ __forceinline__ uint32_t ob_sign_field(const float (&v)[4][4]) {
    uint32_t field = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) field |= (v[k][e] < 0.0f ? 1u : 0u) << (k * 4 + e);
    return field;
}
// bits and |v| partial of tile t from the lane's 16 values; with `field` for the kernels
// that have it before they store the values (the fused middle steps)
__device__ __forceinline__ void ob_emit_tile(const float (&v)[4][4], uint32_t field, uint8_t* bits, float* part,
                                             int64_t t, int lane) {
    ob_store_field(field, bits, t, lane);
    float ab[4][4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int e = 0; e < 4; ++e) ab[k][e] = __builtin_fabsf(v[k][e]);
    ob_store_partial(lane_tree(ab), part, t, lane);
}
__device__ __forceinline__ void ob_emit_tile(const float (&v)[4][4], uint8_t* bits, float* part, int64_t t, int lane) {
    ob_emit_tile(v, ob_sign_field(v), bits, part, t, lane);
}

// prologue of the fused middle steps: segment c of the p received ones decodes to
// +-scale_c as stored in T (pos[c] / neg[c], in LDS; the caller's barrier publishes them)
template <typename T>
__device__ __forceinline__ void ob_scale_tables(const uint8_t* in, int64_t chunk_offset, int p, float* pos, float* neg) {
    if (threadIdx.x < (unsigned)p) {
        float sc;
        __builtin_memcpy(&sc, in + (int64_t)threadIdx.x * chunk_offset, 4);
        pos[threadIdx.x] = as_stored<T>(sc);
        neg[threadIdx.x] = as_stored<T>(-sc);
    }
}

// decode of the lane's field of tile t: bit ? -scale : +scale, as a sign-bit flip of the
// scale's bits
template <typename T, bool NTS>
__device__ __forceinline__ void ob_decode_field(uint32_t field, uint32_t sbits, typename T::storage* dst, int64_t t,
                                                int64_t cs, bool vec, int lane) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float f[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) f[e] = __uint_as_float(sbits ^ ((field << (31 - (k * 4 + e))) & 0x80000000u));
        store4<T, NTS>(dst, t * kObTile + k * 256 + lane * 4, cs, vec, f);
    }
}

// Body of the finalize kernels, one kObFinalizeThreads workgroup per chunk: scale =
// F(partials) / n, the header, the slack; returns the scale to every thread
__device__ __forceinline__ float ob_finalize(const float* partials, int64_t tiles_per_chunk, int64_t in_num_elem,
                                             int64_t cs, int target, uint8_t* out, int64_t chunk_offset,
                                             int64_t out_bytes, int num_chunks, float (&lvl)[2][2048]) {
    const int c = target < 0 ? (int)blockIdx.x : target;
    const int64_t n = ob_valid(in_num_elem, cs, c);
    const float* part = partials + (int64_t)blockIdx.x * tiles_per_chunk;
    const int64_t m1 = (n + kObTile - 1) / kObTile;  // tiles holding valid elements
    const float total = chunk_tree([part](int64_t r) { return part[r]; }, m1, lvl);
    uint8_t* seg = out + (int64_t)c * chunk_offset;
    const float scale = n > 0 ? total / (float)n : 0.0f;
    if (threadIdx.x < 32) {
        const uint32_t sb = __float_as_uint(scale), nb = (uint32_t)n;
        const int t = threadIdx.x;
        uint32_t b = 0;
        if (t < 4) b = (sb >> (8 * t)) & 0xff;
        else if (t < 8) b = (nb >> (8 * (t - 4))) & 0xff;
        seg[t] = (uint8_t)b;
    }
    const int64_t tiles = (cs + kObTile - 1) / kObTile;
    for (int64_t j = 32 + tiles * kObTileBytes + threadIdx.x; j < chunk_offset; j += kObFinalizeThreads) seg[j] = 0;
    if (target < 0 && c == num_chunks - 1)
        for (int64_t j = (int64_t)num_chunks * chunk_offset + threadIdx.x; j < out_bytes; j += kObFinalizeThreads)
            out[j] = 0;
    return scale;
}

// ------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------
static int64_t ob_tiles(int64_t cs) { return (cs + kObTile - 1) / kObTile; }

static int ob_blocks(int64_t tiles, int nact, int target_blocks = kTargetBlocks) {
    int64_t b = (tiles + kWavesPerBlock - 1) / kWavesPerBlock;
    const int64_t cap = (target_blocks + nact - 1) / nact;
    if (b > cap) b = cap;
    return (int)(b < 1 ? 1 : b);
}

// the argument checks the entries share: a segment of co bytes holds its header and tiles ...
static inline bool ob_holds(int64_t co, int64_t tiles) { return co >= 32 + tiles * kObTileBytes; }
// ... every segment's bit tiles are dword-aligned (they are written as dwords) ...
static inline bool ob_aligned(const void* segs, int64_t co) { return ((uintptr_t)segs + 32) % 4 == 0 && co % 4 == 0; }
// ... the workspace holds the tile partials of the nact chunks encoded ...
static inline bool ob_ws_ok(const void* ws, size_t ws_bytes, int nact, int64_t tiles) {
    return ws && ws_bytes >= (size_t)nact * (size_t)(tiles > 0 ? tiles : 1) * sizeof(float);
}
// ... and the error-feedback state (the carry is read and written as 16-B vectors)
static inline bool ob_ef_state_ok(const float* carry, const float* scales) {
    return carry && scales && (uintptr_t)carry % 16 == 0 && (uintptr_t)scales % 16 == 0;
}

// What the two encodes check alike after their own arguments, in their order of precedence:
// p segments of co bytes each at `out`, nact of them encoded
static inline int ob_check_encode(const uint8_t* out, int64_t co, int64_t tiles, const void* ws, size_t ws_bytes, int nact) {
    if (!ob_holds(co, tiles)) return BAGUA_ERR_INVALID_ARG;
    if (!ob_ws_ok(ws, ws_bytes, nact, tiles)) return BAGUA_ERR_WORKSPACE;
    if (!ob_aligned(out, co)) return BAGUA_ERR_INVALID_ARG;
    return BAGUA_OK;
}

// What the two fused middle steps check alike, in their order of precedence (the
// error-feedback one checks its state first).  UNSUPPORTED: the op falls back on that code
// to decompress + reduce + compress
static inline int ob_check_middle(const uint8_t* recv, size_t recv_bytes, int cs, int p, const uint8_t* out, size_t out_bytes,
                           int target, const void* ws, size_t ws_bytes) {
    if (p <= 0 || p > kMaxFusedChunks || cs < 0 || target < 0 || target >= p || !recv || !out)
        return BAGUA_ERR_UNSUPPORTED;
    const int64_t co_in = (int64_t)(recv_bytes / (size_t)p), co = (int64_t)(out_bytes / (size_t)p);
    const int64_t tiles = ob_tiles(cs);
    if (!ob_holds(co_in, tiles) || !ob_holds(co, tiles)) return BAGUA_ERR_INVALID_ARG;
    if (!ob_aligned(recv, co_in) || !ob_aligned(out, co)) return BAGUA_ERR_INVALID_ARG;
    if (!ob_ws_ok(ws, ws_bytes, 1, tiles)) return BAGUA_ERR_WORKSPACE;
    return BAGUA_OK;
}

// Non-temporal accesses for a stream of `bytes` that the next kernel reads again?  Up to
// the 256 MiB Infinity Cache default-policy ones (the lines stay on chip for the reader);
// past it the cache cannot keep the dirty lines, which the next kernel then writes back.
// `knob` = 1 / 0 forces either (A/B)
static inline bool ob_nt_by_size(int64_t bytes, const char* knob) {
    const int env = tune_int(knob, -1);
    return (env >= 0 ? env : (bytes > ((int64_t)256 << 20) ? 1 : 0)) == 1;
}

}  // namespace bagua
