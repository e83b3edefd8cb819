// minmax_resident.hip — one-launch MinMax-UInt8 encode that keeps part of
// every chunk on chip across the chunk-wide min/max exchange.
//
// The reference encode (bagua_kernels.cu:533-571) reads each chunk three
// times (cub Min, cub Max, compress_float_to_uint8, K:268-371 + K:455-479);
// the two-kernel path in minmax_u8.hip reads it twice.  No payload byte can
// be emitted before the chunk's min/max is known, so the second read is
// intrinsic to any encoder that streams the chunk from HBM twice — but not to
// one that keeps what it read.  This kernel runs ONE workgroup per CU (the
// grid is the CU count), each owning one contiguous slice of a chunk:
//
//   pass 1: stream the slice once (default-policy loads): the first
//           R vectors per lane stay in VGPRs, the next H per lane are parked
//           in LDS (up to ~156 KiB per CU), the rest are only folded into the
//           min/max; publish the workgroup's {min, max} as two 8-byte
//           {tag, value} granules (the data is the flag: one atomic store
//           each, no fence, MI355X guide Guideline 16 R2)
//   exchange: two waves poll the chunk's granules, a batch of loads per lane in
//           flight at once (one memory round trip per round, not one per
//           granule), until each carries this launch's tag; a granule is kept
//           once it does; then they are folded (order-free keys, codec_common.hpp)
//   pass 2: quantise the streamed part first, in reverse (the lines pass 1
//           read last are the ones the 256 MiB Infinity Cache still holds),
//           then the LDS part, then the VGPR part, and write header / slack.
//
// minmax_resident_encode_kernel_stack (the f16 default) runs the passes in
// stack order instead -- pass 1: streamed, parked, held; pass 2: held, parked,
// streamed -- so the held vectors reuse the streaming buffers' registers and more
// of the chunk stays on chip without scratch (see the comment above that kernel).
// minmax_resident_encode_kernel_window (the f32 and bf16 default) keeps the order above
// and loads a last few held rows into the streaming buffers' registers once pass 1 has
// streamed, so as much stays on chip and the re-read follows the read closely.
//
// Layout of this file: the launch arguments and slice geometry; the per-vector and
// per-chunk pieces (fold_vec, write_extras, sweep_chunk, fold_missing_slices); the shared
// phases, each written once as a forced-inline template over the caller's register arrays
// (draw_ticket, park_tag, load_rows, fold_rows, fold_and_park, fold_stream_ascending, publish_partials,
// exchange_minmax, quant_rows, quant_parked, quant_top_tile, quant_stream_descending /
// _ascending, finish); the three kernels, each a sequence of those phases in its own order
// with its own scheduling barriers and trace stamps; then the host side: slots, kResCfg,
// one table of kernel pointers per dtype built from kResCfg, the launch plan and the C ABI.
//
// Per-launch state lives in a library-owned slot (one per stream; the
// hipStreamPerThread sentinel gets one per host thread) that is never reset:
// launch k on a slot draws tickets [kG, (k+1)G) from monotonic counters, so
// its tag is k+1 (no memset node, graph-replay safe).  The tickets (and the
// drain count below) are spread over kResLanes counters on separate 128-B lines,
// workgroup g on counter g % kResLanes (its XCD under round-robin placement):
// 256 returning atomics on ONE word serialise at the memory side (≈ 88 per µs,
// MI355X guide "dequeue"), which held the last workgroup's start ~3 µs back.  Thread 0 draws the
// ticket at kernel entry.  In the stack order nothing waits for it there: it is in flight with the
// first loads of pass 1, turned into the tag in LDS behind them, and read by every thread at the
// publish, where a barrier already stands.  In the window and stream-last orders thread 0's wave
// still waits for it (and divides) before its first load, because deferring it lost time there
// (see those kernels); no order has an LDS broadcast or a barrier ahead of its first loads, and
// idle workgroups never wait for the value.  Every workgroup bumps a
// second counter once it is done with the slot (after the exchange), so the
// host can tell when every launch it issued on a slot has let go of it; a
// slot changes owner (release, or LRU reclaim when all 64 are taken) only then.
// (An event recorded behind every launch cost 3-5 us per step, even without a
// system-scope fence: profiles/r02_slot_event_ab.jsonl.)
//
// Residency: the exchange needs every workgroup of a chunk resident at once.
// The grid equals the CU count and the kernel admits one workgroup per CU,
// but another stream's kernels can occupy CUs, so the wait is BOUNDED: a
// workgroup that times out folds every slice whose partials are still
// missing straight from memory (min/max is order-free and idempotent, so any
// mix of published partials and re-read slices is the chunk's exact min/max)
// and quantises its own slice.  The late workgroup, once it runs, finds the
// partials of all the others published and finishes normally.  No second
// kernel, no spin without a deadline; the bytes are the same either way.
//
// Bit-identity: the same per-element expressions as minmax_quantize_kernel;
// the min/max is order-free, so slicing cannot change it.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include <chrono>
#include <map>
#include <mutex>
#include <set>
#include <thread>
#include <utility>

#include "codec_common.hpp"
#include "launch_util.hpp"

namespace bagua {

constexpr int kResMaxGrid = 1024;
constexpr int kResSlots = 64;
constexpr int kResLanes = 8;  // ticket / drain counters per slot (one per XCD)

struct ResidentSlot {
    uint64_t ticket[kResLanes][16];   // monotonic ticket counters, one 128-B line each (workgroup g: lane g % 8)
    uint64_t drained[kResLanes][16];  // workgroups done with the slot, per lane (once each, at its end)
    uint64_t gave_up;                 // workgroups that timed out in the exchange (bagua_minmax_u8_resident_give_ups)
    uint64_t pad0[15];
    uint64_t gran[2 * kResMaxGrid];   // {tag << 32 | min key}, {tag << 32 | max key} per workgroup
};
static_assert(sizeof(ResidentSlot) % 64 == 0, "slot alignment");

struct ResidentArgs {
    const void* in;
    int64_t cs;            // chunk size (elements)
    int target;            // -1: all chunks
    int nact;              // active chunks
    int bpc;               // workgroups per active chunk
    int grid;              // launched workgroups (the CU count; idle ones >= nact * bpc)
    uint8_t* out;
    int64_t chunk_offset;  // bytes per segment
    int64_t out_bytes;
    int num_chunks;
    ResidentSlot* slot;
    uint64_t timeout_ticks;  // wall_clock64 ticks a workgroup waits for its chunk's partials
    uint64_t* trace;         // measurement hook: 8 wall_clock64 slots per workgroup, or nullptr
};

__device__ __forceinline__ void trace_stamp(const ResidentArgs& a, int g, int k) {
    if (a.trace != nullptr && threadIdx.x == 0) a.trace[8 * g + k] = wall_clock64();
}

// every launch on a slot has the same grid, so counter c receives the same number
// of tickets per launch: the workgroups g < grid with g % kResLanes == c
// (the result is never 0, the zeroed state).  The tag is resolved on the publish path, so a
// counter's first 2^32 tickets divide in 32 bits: the same value as the 64-bit expression
// below, without its ~100 instructions.
__device__ __forceinline__ uint32_t tag_of_ticket(uint64_t ticket, int grid, int lane) {
    const uint32_t per_launch = (uint32_t)((grid - lane + kResLanes - 1) / kResLanes);
    if ((ticket >> 32) == 0) {
        const uint32_t k = (uint32_t)ticket / per_launch;
        return (k == 0xffffffffu ? 0u : k) + 1u;
    }
    return (uint32_t)((ticket / (uint64_t)per_launch) % 0xffffffffull) + 1u;
}

template <typename T, int BLOCK>
struct SliceGeom {
    using S = typename T::storage;
    int c;               // chunk index in the tensor
    int cl;              // active-chunk index
    int b;               // slice index within the chunk
    const S* src;        // chunk start
    uint8_t* seg;        // chunk's segment
    uint8_t* payload;    // seg + 32
    int64_t j0;          // elements before the vector body (scalar head)
    int64_t nvec;        // body vectors
    int64_t v0, v1;      // this slice's vectors [v0, v1)
    bool last;           // last slice of the chunk: owns head, tail and slack

    __device__ __forceinline__ SliceGeom(const ResidentArgs& a, int g) {
        constexpr int N = Vec<T>::N;
        cl = g / a.bpc;
        b = g - cl * a.bpc;
        c = a.target < 0 ? cl : a.target;
        src = static_cast<const S*>(a.in) + (int64_t)c * a.cs;
        seg = a.out + (int64_t)c * a.chunk_offset;
        payload = seg + 32;
        const int al = common_alignment<T>((uintptr_t)src, (uintptr_t)payload);  // host checked >= 0
        j0 = al < a.cs ? al : a.cs;
        nvec = (a.cs - j0) / N;
        const int64_t per = ((nvec + a.bpc - 1) / a.bpc + BLOCK - 1) / BLOCK * BLOCK;
        v0 = (int64_t)b * per;
        v0 = v0 < nvec ? v0 : nvec;
        v1 = v0 + per < nvec ? v0 + per : nvec;
        last = (b == a.bpc - 1);
    }
};

template <typename T>
__device__ __forceinline__ void fold_vec(const uint4& r, uint32_t& lo, uint32_t& hi) {
    float f[Vec<T>::N];
    unpack16<T>(r, f);
#pragma unroll
    for (int i = 0; i < Vec<T>::N; ++i) {
        const int32_t k = f2key(f[i]);
        lo = min(lo, min_space_key(k));
        hi = min(hi, max_space_key(k));
    }
}

// the scalar head and tail elements of a chunk (owned by its last slice)
template <typename T, int BLOCK>
__device__ __forceinline__ void fold_scalars(const ResidentArgs& a, const SliceGeom<T, BLOCK>& s, uint32_t& lo,
                                             uint32_t& hi) {
    constexpr int N = Vec<T>::N;
    const int t = (int)threadIdx.x;
    for (int64_t j = t; j < s.j0; j += BLOCK) {
        const int32_t k = f2key(T::to_f(s.src[j]));
        lo = min(lo, min_space_key(k));
        hi = min(hi, max_space_key(k));
    }
    for (int64_t j = s.j0 + s.nvec * N + t; j < a.cs; j += BLOCK) {
        const int32_t k = f2key(T::to_f(s.src[j]));
        lo = min(lo, min_space_key(k));
        hi = min(hi, max_space_key(k));
    }
}

template <int SB, int BLOCK, bool NT = false>
__device__ __forceinline__ void load_tile(const uint4* __restrict__ v, int64_t base, int t, uint4 (&r)[SB]) {
#pragma unroll
    for (int j = 0; j < SB; ++j) r[j] = NT ? nt_load16(&v[base + j * BLOCK + t]) : v[base + j * BLOCK + t];
}

template <typename T>
__device__ __forceinline__ void quant_store(const uint4& r, const QParams& q, uint8_t* dst) {
    float f[Vec<T>::N];
    unpack16<T>(r, f);
    quant_store_vec<T>(f, q, dst);
}

// header of chunk c (slice 0), slack after the payload and the buffer tail
// (last slice), scalar head and tail elements (last slice) -- the same bytes
// minmax_quantize_kernel writes
template <typename T, int BLOCK>
__device__ void write_extras(const ResidentArgs& a, const SliceGeom<T, BLOCK>& s, float mn, float mx,
                             const QParams& q) {
    using S = typename T::storage;
    constexpr int N = Vec<T>::N;
    const int t = (int)threadIdx.x;
    if (s.b == 0 && t < 32) {
        const uint32_t bmn = sizeof(S) == 4 ? __float_as_uint(mn) : (uint32_t)T::from_f(mn);
        const uint32_t bmx = sizeof(S) == 4 ? __float_as_uint(mx) : (uint32_t)T::from_f(mx);
        uint32_t hb = 0;
        if (t < (int)sizeof(S)) hb = (bmn >> (8 * t)) & 0xff;
        else if (t < 2 * (int)sizeof(S)) hb = (bmx >> (8 * (t - (int)sizeof(S)))) & 0xff;
        s.seg[t] = (uint8_t)hb;
    }
    if (!s.last) return;
    for (int64_t j = 32 + a.cs + t; j < a.chunk_offset; j += BLOCK) s.seg[j] = 0;
    if (a.target < 0 && s.c == a.num_chunks - 1)
        for (int64_t j = (int64_t)a.num_chunks * a.chunk_offset + t; j < a.out_bytes; j += BLOCK) a.out[j] = 0;
    for (int64_t j = t; j < s.j0; j += BLOCK) s.payload[j] = (uint8_t)quant(T::to_f(s.src[j]), q);
    for (int64_t j = s.j0 + s.nvec * N + t; j < a.cs; j += BLOCK)
        s.payload[j] = (uint8_t)quant(T::to_f(s.src[j]), q);
}

// Waves 0 and 1 fold the granules of active chunk `cl`, wave w those with index w * 64 + l + 128 j
// (l the lane); false once `deadline` passes.  A batch of kSweepBatch granules per lane is
// requested back to back and waited for once, so a round costs one memory round trip per 512
// granules (one for a grid of up to 256 workgroups) instead of one per granule.  Two waves,
// because eight granules in flight per lane made the f32 R = 52 stack rows (24 is pinned by
// test_default_rows_use_no_scratch) spill.  (The f16 and bf16 R = 52 stack rows, not defaults, which
// spilled before, spill a few VGPRs more: 41 -> 48 and 33 -> 40 for f16, 0 -> 2-4 for bf16.)
// The outer loop over batches runs more than once only for more than 256 workgroups per chunk:
// kResMaxGrid allows it, no 256-CU part reaches it, and it is untested.
// A granule that carries this launch's tag is final, since a workgroup publishes once per launch:
// it is folded into the lane's key once and not read again, so the polling thins out as
// workgroups publish.
constexpr int kSweepWaves = 2;
constexpr int kSweepBatch = 4;
__device__ __forceinline__ bool sweep_chunk(const ResidentArgs& a, int cl, uint32_t tag, int w, uint64_t deadline,
                                            uint32_t& lo, uint32_t& hi, bool bounded) {
    const int lane = lane_id();
    const uint64_t* g = a.slot->gran + 2 * (int64_t)cl * a.bpc;  // uniform: the lane's part is a 32-bit offset
    const int n = 2 * a.bpc;
    const int first = w * kWave + lane;
    // even granules are minima and odd ones maxima, and the lane's are odd when the lane is: one key
    uint32_t key = 0xffffffffu;
    for (int base = first; base - first < n; base += kSweepBatch * kSweepWaves * kWave) {
        uint32_t missing = 0;  // bit j: granule base + 128 j is still to come
#pragma unroll
        for (int j = 0; j < kSweepBatch; ++j)
            if (base + j * kSweepWaves * kWave < n) missing |= 1u << j;
        for (;;) {
            uint64_t x[kSweepBatch];
#pragma unroll
            for (int j = 0; j < kSweepBatch; ++j) {
                x[j] = 0;  // tag 0: never this launch's
                if ((missing >> j) & 1u)
                    x[j] = __hip_atomic_load(g + (uint32_t)(base + j * kSweepWaves * kWave), __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT);
            }
#pragma unroll
            for (int j = 0; j < kSweepBatch; ++j) {
                if ((uint32_t)(x[j] >> 32) == tag) {
                    key = min(key, (uint32_t)x[j]);
                    missing &= ~(1u << j);
                }
            }
            if (__all(missing == 0)) break;
            if (bounded && (uint64_t)wall_clock64() > deadline) return false;
            __builtin_amdgcn_s_sleep(2);
        }
    }
    lo = wave_umin((lane & 1) ? 0xffffffffu : key);
    hi = wave_umin((lane & 1) ? key : 0xffffffffu);
    return true;
}

// after a give-up: the calling thread's share of the chunk's min/max, taking a
// slice's published partials when both carry this launch's tag and re-reading
// the slice otherwise.  Threads may disagree about a granule that lands
// meanwhile; every slice is then still covered whole (by the granule some
// thread took, or by all threads' strided re-reads), so the union is exact.
// LEAN: the re-read loop is not unrolled (a caller with no registers to spare on this
// rare path)
template <typename T, int BLOCK, bool LEAN = false>
__device__ void fold_missing_slices(const ResidentArgs& a, int cl, uint32_t tag, uint32_t& lo, uint32_t& hi) {
    const int t = (int)threadIdx.x;
    for (int b = 0; b < a.bpc; ++b) {
        const int gg = cl * a.bpc + b;
        const uint64_t* gr = a.slot->gran + 2 * (int64_t)gg;
        const uint64_t x0 = __hip_atomic_load(gr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint64_t x1 = __hip_atomic_load(gr + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((uint32_t)(x0 >> 32) == tag && (uint32_t)(x1 >> 32) == tag) {
            lo = min(lo, (uint32_t)x0);
            hi = min(hi, (uint32_t)x1);
            continue;
        }
        const SliceGeom<T, BLOCK> sg(a, gg);
        const uint4* __restrict__ v = reinterpret_cast<const uint4*>(sg.src + sg.j0);
        if constexpr (LEAN) {
#pragma unroll 1
            for (int64_t i = sg.v0 + t; i < sg.v1; i += BLOCK) fold_vec<T>(v[i], lo, hi);
        } else {
            for (int64_t i = sg.v0 + t; i < sg.v1; i += BLOCK) fold_vec<T>(v[i], lo, hi);
        }
        if (sg.last) fold_scalars<T, BLOCK>(a, sg, lo, hi);
    }
}

// ------------------------------------------------------------------------
// shared phases
// ------------------------------------------------------------------------
// Each phase of the encode is written once here; the three kernels below are sequences of
// these calls in their own order.  Every phase is forced inline and works on the caller's
// register arrays (uint4 (&)[M]), so a kernel decides which registers a phase uses and when
// they die; no phase knows which kernel calls it.  A row is BLOCK vectors, one per lane.
//
// The words after the parked rows in LDS (`scratch`, W = BLOCK / kWave): [0, W) per-wave min
// keys, [W, 2W) per-wave max keys, 2W the launch's tag, 2W + 1 whether the exchange completed,
// 2W + 2 + 2i and 2W + 3 + 2i the min and max keys sweeping wave i found (after a give-up: the
// chunk's), then two words for the traced kernel-entry time.
constexpr int res_scratch_words(int block) { return 2 * (block / kWave) + 2 + 2 * kSweepWaves + 2; }

// Trace stamp 0, kernel entry.  An active workgroup keeps it in LDS until stamp 1, so that no
// store to memory is pending when the counted waits of pass 1's first loads begin (stores and
// loads share vmcnt but need not return in order, so the compiler may then wait for everything).
template <int BLOCK>
__device__ __forceinline__ void trace_entry(const ResidentArgs& a, int t, uint32_t* scratch) {
    constexpr int W = BLOCK / kWave;
    if (a.trace != nullptr && t == 0) {
        const uint64_t now = wall_clock64();
        scratch[2 * W + 2 + 2 * kSweepWaves] = (uint32_t)now;
        scratch[2 * W + 3 + 2 * kSweepWaves] = (uint32_t)(now >> 32);
    }
}

// stamp 0 from LDS (thread 0 wrote it and reads it)
template <int BLOCK>
__device__ __forceinline__ void trace_entry_flush(const ResidentArgs& a, int g, int t,
                                                  const uint32_t* scratch) {
    constexpr int W = BLOCK / kWave;
    if (a.trace != nullptr && t == 0)
        a.trace[8 * g] = ((uint64_t)scratch[2 * W + 3 + 2 * kSweepWaves] << 32) | scratch[2 * W + 2 + 2 * kSweepWaves];
}

// The workgroup's ticket on counter `lane_c` of its slot, drawn by thread 0 at kernel entry.
// Nothing waits for it in here; the caller decides where the value is first used (park_tag): the
// stack order behind its first loads, the window and stream-last orders at once.
__device__ __forceinline__ uint64_t draw_ticket(const ResidentArgs& a, int lane_c, int t) {
    uint64_t ticket = 0;
    if (t == 0) {
        // The offset is 0, but opaque to the compiler: with an address it knows to be uniform it
        // rewrites the atomic as a wave-wide one whose result goes through v_readfirstlane, and
        // that is a full wait (vmcnt(0)) right here (seen with ROCm 7.2's clang 22.0.0git; without
        // that rewrite the offset costs one v_mov and changes nothing).
        int zero = 0;
        asm volatile("" : "+v"(zero));
        ticket = __hip_atomic_fetch_add(&a.slot->ticket[lane_c][zero], (uint64_t)1, __ATOMIC_RELAXED,
                                        __HIP_MEMORY_SCOPE_AGENT);
    }
    return ticket;
}

// Once the first loads of pass 1 are issued, thread 0 turns the ticket into the launch's tag and
// leaves it in LDS (word 2W; word 2W + 1: the exchange counts as complete until a sweeping wave
// says otherwise).  The wait for the ticket is a counted one that leaves those loads in flight --
// memory answers in order, so they could not be used earlier anyway -- and the division runs
// under their latency; the ticket holds no registers across pass 1.  Every thread reads the tag
// behind the publish's barrier (publish_partials).
template <int BLOCK>
__device__ __forceinline__ void park_tag(const ResidentArgs& a, uint64_t ticket, int lane_c, int t,
                                         uint32_t* scratch) {
    constexpr int W = BLOCK / kWave;
    if (t == 0) {
        scratch[2 * W] = tag_of_ticket(ticket, a.grid, lane_c);
        scratch[2 * W + 1] = 1u;
    }
}

// the workgroup is done with the slot (once per workgroup, idle ones included)
__device__ __forceinline__ void let_go_of_slot(const ResidentArgs& a, int lane_c, int t) {
    if (t == 0)
        __hip_atomic_fetch_add(&a.slot->drained[lane_c][0], (uint64_t)1, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
}

// end of an active workgroup: stamp 3 when traced, then the workgroup lets go of the slot (its
// granule reads ended at the exchange's barriers); counted last, so no later load waits
// behind this atomic (on gfx9 a non-returning atomic still holds vmcnt: mid-kernel it cost
// ~1.3 us, profiles/r03_resident_versions_ab.jsonl)
__device__ __forceinline__ void finish(const ResidentArgs& a, int g, int lane_c, int t) {
    if (a.trace != nullptr) {
        __syncthreads();
        trace_stamp(a, g, 3);
    }
    let_go_of_slot(a, lane_c, t);
}

// Rows [ROW0, ROW0 + K) counted from vector `base`, their indices clamped to `vl` (the
// slice's last vector): a short slice or a ragged tile loads like a whole one, all K loads in
// flight together and the wait counts static; a duplicate of a slice element never changes
// the min/max, and pass 2 stores only what is in range.  The row offset is a template
// argument so that the address folds to (base + t) + constant, as the other rows' do.
template <int K, int ROW0, int BLOCK, bool NT, int M>
__device__ __forceinline__ void load_rows(const uint4* v, int64_t base, int64_t vl, int t,
                                          uint4 (&r)[M]) {
    static_assert(K <= M, "more rows than registers");
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int64_t i = base + (int64_t)(ROW0 + k) * BLOCK + t;
        r[k] = NT ? nt_load16(&v[i < vl ? i : vl]) : v[i < vl ? i : vl];
    }
}

// FENCE4: four rows' keys at a time (a scheduling barrier after every fourth row), for a
// caller whose register budget has no room for every row's expanded keys at once
template <typename T, int K, bool FENCE4, int M>
__device__ __forceinline__ void fold_rows(const uint4 (&r)[M], uint32_t& lo, uint32_t& hi) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
        fold_vec<T>(r[k], lo, hi);
        if (FENCE4 && k % 4 == 3) __builtin_amdgcn_sched_barrier(0);
    }
}

// The parked rows, rows [ROW0, ROW0 + H) of the slice at vector `v0`, software-pipelined in
// batches of SB: the next batch is in flight while the current one is folded and parked, so
// memory never waits on VALU.  The caller requests the first batch into `cur`
// (load_rows<min(H, SB), ROW0>) together with whatever else it wants in flight, and folds
// that before it calls this.
template <typename T, int BLOCK, int H, int SB, int ROW0, bool NT>
__device__ __forceinline__ void fold_and_park(const uint4* v, int64_t v0, int64_t vl, int t,
                                              uint4 (&cur)[SB], uint4* park, uint32_t& lo, uint32_t& hi) {
    uint4 nxt[SB];
#pragma unroll
    for (int kb = 0; kb < H; kb += SB) {
#pragma unroll
        for (int j = 0; j < SB; ++j) {
            if (kb + SB + j < H) {
                const int64_t i = v0 + (int64_t)(ROW0 + kb + SB + j) * BLOCK + t;
                nxt[j] = NT ? nt_load16(&v[i < vl ? i : vl]) : v[i < vl ? i : vl];
            }
        }
#pragma unroll
        for (int j = 0; j < SB; ++j) {
            if (kb + j < H) {
                fold_vec<T>(cur[j], lo, hi);
                park[(kb + j) * BLOCK + t] = cur[j];
            }
        }
#pragma unroll
        for (int j = 0; j < SB; ++j) cur[j] = nxt[j];
    }
}

// The nfull > 0 full streamed tiles, ascending and double-buffered (2 x SB loads in flight
// per lane: with one wave per SIMD nothing else hides the latency).  `ra` holds tile 0,
// requested by the caller.  `last` is nfull - 1, computed by the caller next to nfull: written
// as nfull - 1 in here, the clamp is turned into a 64-bit min before the kernel's knowledge of
// nfull reaches it, which costs the loop six VALU instructions and three waits.
template <typename T, int BLOCK, int SB>
__device__ __forceinline__ void fold_stream_ascending(const uint4* v, int64_t stream0, int64_t nfull, int64_t last, int t,
                                                      uint4 (&ra)[SB], uint4 (&rb)[SB], uint32_t& lo,
                                                      uint32_t& hi) {
    constexpr int64_t tile = (int64_t)SB * BLOCK;
    for (int64_t i = 0; i < nfull; i += 2) {
        // unconditional (clamped) prefetches keep the wait counts static
        load_tile<SB, BLOCK>(v, stream0 + (i + 1 < nfull ? i + 1 : last) * tile, t, rb);
        fold_rows<T, SB, false>(ra, lo, hi);
        load_tile<SB, BLOCK>(v, stream0 + (i + 2 < nfull ? i + 2 : last) * tile, t, ra);
        if (i + 1 < nfull) fold_rows<T, SB, false>(rb, lo, hi);
    }
}

// every thread's keys in; the workgroup's minima out, in thread 0 only.  `w` is the thread's
// wave, t / kWave, computed once by the kernel: a second, separately simplified copy of the
// division keeps one more mask in SGPRs across the exchange, which spills at R = 52.
template <int BLOCK>
__device__ __forceinline__ void workgroup_umin(uint32_t& lo, uint32_t& hi, int t, int w, uint32_t* scratch) {
    constexpr int W = BLOCK / kWave;
    lo = wave_umin(lo);
    hi = wave_umin(hi);
    if (lane_id() == 0) { scratch[w] = lo; scratch[W + w] = hi; }
    __syncthreads();
    if (t == 0) {
#pragma unroll
        for (int i = 1; i < W; ++i) { lo = min(lo, scratch[i]); hi = min(hi, scratch[W + i]); }
    }
}

// end of pass 1: the launch's tag, read here from LDS (park_tag wrote it; the barrier is
// workgroup_umin's) and returned in every thread, and the workgroup's {min, max} as two 8-byte {tag, value} granules
template <int BLOCK>
__device__ __forceinline__ uint32_t publish_partials(const ResidentArgs& a, int g, uint32_t lo, uint32_t hi,
                                                     int t, int w, uint32_t* scratch) {
    constexpr int W = BLOCK / kWave;
    workgroup_umin<BLOCK>(lo, hi, t, w, scratch);
    const uint32_t tag = scratch[2 * W];
    if (t == 0) {
        uint64_t* mine = a.slot->gran + 2 * (int64_t)g;
        __hip_atomic_store(mine, ((uint64_t)tag << 32) | lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(mine + 1, ((uint64_t)tag << 32) | hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return tag;
}

struct MinMax {
    float mn, mx;
};

// The exchange: waves 0 and 1 sweep the granules of active chunk `cl` until every tag is this
// launch's or the deadline passes; on a give-up the whole workgroup folds the missing slices
// itself (fold_missing_slices; LEAN as there).  The chunk's min/max, the same in every thread.
template <typename T, int BLOCK, bool LEAN>
__device__ __forceinline__ MinMax exchange_minmax(const ResidentArgs& a, int cl, uint32_t tag, int t, int w,
                                                  uint32_t* scratch) {
    constexpr int W = BLOCK / kWave;
    if (w < kSweepWaves) {
        const uint64_t deadline = wall_clock64() + a.timeout_ticks;
        uint32_t l = 0, h = 0;
        const bool ok = sweep_chunk(a, cl, tag, w, deadline, l, h, true);
        if (lane_id() == 0) {
            if (!ok) scratch[2 * W + 1] = 0u;
            scratch[2 * W + 2 + 2 * w] = l;
            scratch[2 * W + 3 + 2 * w] = h;
        }
    }
    __syncthreads();
    if (scratch[2 * W + 1] == 0u) {
        if (t == 0) __hip_atomic_fetch_add(&a.slot->gave_up, (uint64_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        uint32_t l = 0xffffffffu, h = 0xffffffffu;
        fold_missing_slices<T, BLOCK, LEAN>(a, cl, tag, l, h);
        workgroup_umin<BLOCK>(l, h, t, w, scratch);
        if (t == 0) {
#pragma unroll
            for (int i = 0; i < kSweepWaves; ++i) {
                scratch[2 * W + 2 + 2 * i] = l;
                scratch[2 * W + 3 + 2 * i] = h;
            }
        }
        __syncthreads();
    }
    uint32_t cmin = scratch[2 * W + 2], cmax = scratch[2 * W + 3];
#pragma unroll
    for (int i = 1; i < kSweepWaves; ++i) {
        cmin = min(cmin, scratch[2 * W + 2 + 2 * i]);
        cmax = min(cmax, scratch[2 * W + 3 + 2 * i]);
    }
    return MinMax{from_min_space(cmin), from_max_space(cmax)};
}

// the part of [v0, v1) that lies in the ON_CHIP vectors a slice keeps on chip: a short slice's
// guard, compared with a lane's offset in 32 bits
template <int ON_CHIP>
__device__ __forceinline__ int on_chip_count(int64_t v0, int64_t v1) {
    return (int)(v1 - v0 < (int64_t)ON_CHIP ? (v1 > v0 ? v1 - v0 : 0) : (int64_t)ON_CHIP);
}

// Rows [ROW0, ROW0 + K) of a slice from registers; `vd` is the lane's first payload byte of
// the slice.  For a slice that holds its whole on-chip part (every slice of a bucket this
// path takes): no per-vector guards.  FENCE4: four rows' temporaries at a time.
template <typename T, int BLOCK, int K, int ROW0, bool FENCE4, int M>
__device__ __forceinline__ void quant_rows(const uint4 (&r)[M], const QParams& q, uint8_t* vd) {
    constexpr int N = Vec<T>::N;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        quant_store<T>(r[k], q, vd + (int64_t)(ROW0 + k) * BLOCK * N);
        if (FENCE4 && k % 4 == 3) __builtin_amdgcn_sched_barrier(0);
    }
}

// the same for a short slice: only the vectors below `nloc` (on_chip_count)
template <typename T, int BLOCK, int K, int ROW0, int M>
__device__ __forceinline__ void quant_rows_guarded(const uint4 (&r)[M], int nloc, int t, const QParams& q,
                                                   uint8_t* vd) {
    constexpr int N = Vec<T>::N;
#pragma unroll
    for (int k = 0; k < K; ++k)
        if ((ROW0 + k) * BLOCK + t < nloc) quant_store<T>(r[k], q, vd + (int64_t)(ROW0 + k) * BLOCK * N);
}

// The H parked rows, rows [ROW0, ROW0 + H) of a slice that holds its whole on-chip part, in
// batches of SB: without per-vector guards the LDS reads of a batch issue back to back and
// the quantise+stores pipeline (a guarded vector was its own exec-masked block that waited
// on its own ds_read: 11 us for 36 % of the payload)
template <typename T, int BLOCK, int H, int SB, int ROW0>
__device__ __forceinline__ void quant_parked(const uint4* park, int t, const QParams& q, uint8_t* vd) {
    constexpr int N = Vec<T>::N;
#pragma unroll
    for (int kb = 0; kb < H; kb += SB) {
        uint4 r[SB];
#pragma unroll
        for (int j = 0; j < SB; ++j)
            if (kb + j < H) r[j] = park[(kb + j) * BLOCK + t];
#pragma unroll
        for (int j = 0; j < SB; ++j)
            if (kb + j < H) quant_store<T>(r[j], q, vd + (int64_t)(ROW0 + kb + j) * BLOCK * N);
    }
}

template <typename T, int BLOCK, int H, int ROW0>
__device__ __forceinline__ void quant_parked_guarded(const uint4* park, int nloc, int t, const QParams& q,
                                                     uint8_t* vd) {
    constexpr int N = Vec<T>::N;
#pragma unroll
    for (int k = 0; k < H; ++k)
        if ((ROW0 + k) * BLOCK + t < nloc)
            quant_store<T>(park[k * BLOCK + t], q, vd + (int64_t)(ROW0 + k) * BLOCK * N);
}

// the ragged top tile [top, v1) from a clamped tile (load_rows<SB>): only what is in range
template <typename T, int BLOCK, int SB>
__device__ __forceinline__ void quant_top_tile(const uint4 (&r)[SB], int64_t top, int64_t v1, int t,
                                               const QParams& q, uint8_t* vdst) {
    constexpr int N = Vec<T>::N;
#pragma unroll
    for (int j = 0; j < SB; ++j) {
        const int64_t i = top + j * BLOCK + t;
        if (i < v1) quant_store<T>(r[j], q, vdst + i * N);
    }
}

// The nfull > 0 full streamed tiles, double-buffered from the top down (what pass 1 read
// last of the streamed part is re-read first).  `qa` holds the top tile, requested by the
// caller.
template <typename T, int BLOCK, int SB, bool NT>
__device__ __forceinline__ void quant_stream_descending(const uint4* v, int64_t stream0, int64_t nfull, int t,
                                                        const QParams& q, uint8_t* vdst, uint4 (&qa)[SB],
                                                        uint4 (&qb)[SB]) {
    constexpr int N = Vec<T>::N;
    constexpr int64_t tile = (int64_t)SB * BLOCK;
    for (int64_t i = nfull - 1; i >= 0; i -= 2) {
        load_tile<SB, BLOCK, NT>(v, stream0 + (i >= 1 ? i - 1 : 0) * tile, t, qb);
        const int64_t ba = stream0 + i * tile;
#pragma unroll
        for (int j = 0; j < SB; ++j) quant_store<T>(qa[j], q, vdst + (ba + j * BLOCK + t) * N);
        load_tile<SB, BLOCK, NT>(v, stream0 + (i >= 2 ? i - 2 : 0) * tile, t, qa);
        if (i >= 1) {
            const int64_t bb = ba - tile;
#pragma unroll
            for (int j = 0; j < SB; ++j) quant_store<T>(qb[j], q, vdst + (bb + j * BLOCK + t) * N);
        }
    }
}

// The same in pass 1's order: the tiles that have waited longest in the Infinity Cache are
// re-read before the payload stores push them out.  `qa` holds tile 0.
template <typename T, int BLOCK, int SB, bool NT>
__device__ __forceinline__ void quant_stream_ascending(const uint4* v, int64_t stream0, int64_t nfull, int t,
                                                       const QParams& q, uint8_t* vdst, uint4 (&qa)[SB],
                                                       uint4 (&qb)[SB]) {
    constexpr int N = Vec<T>::N;
    constexpr int64_t tile = (int64_t)SB * BLOCK;
    for (int64_t i = 0; i < nfull; i += 2) {
        load_tile<SB, BLOCK, NT>(v, stream0 + (i + 1 < nfull ? i + 1 : nfull - 1) * tile, t, qb);
        const int64_t ba = stream0 + i * tile;
#pragma unroll
        for (int j = 0; j < SB; ++j) quant_store<T>(qa[j], q, vdst + (ba + j * BLOCK + t) * N);
        load_tile<SB, BLOCK, NT>(v, stream0 + (i + 2 < nfull ? i + 2 : nfull - 1) * tile, t, qa);
        if (i + 1 < nfull) {
            const int64_t bb = ba + tile;
#pragma unroll
            for (int j = 0; j < SB; ++j) quant_store<T>(qb[j], q, vdst + (bb + j * BLOCK + t) * N);
        }
    }
}

// ------------------------------------------------------------------------
// the kernels: one per order of the phases
// ------------------------------------------------------------------------
// Stream-last order.  A slice is rows [0, R) held in VGPRs, rows [R, R + H) parked in LDS,
// the rest streamed:
//
//   pass 1: held, parked, streamed (ascending), a guarded ragged tail
//   pass 2: the streamed part first, in reverse (the ragged tail, then the full tiles from
//           the top down, the two top ones requested before the exchange), then the parked
//           rows, then the held rows
//
// Every buffer is live where the source says it is: no scheduling barriers.
// NTM: non-temporal load mask -- bit 0: pass 2's re-reads of the streamed part;
// bit 1: pass 1's loads of the part kept on chip (held in VGPRs / parked in LDS), which
// nothing re-reads, so they need not take Infinity-Cache lines from the streamed part
// Trace stamps: 0 entry, 1 pass 1 end, 2 exchange end, 4 streamed rows stored, 5 parked
// rows stored, 3 end.
template <typename T, int BLOCK, int R, int H, int SB, int NTM>
__global__ __launch_bounds__(BLOCK, 1) void minmax_resident_encode_kernel(ResidentArgs a) {
    constexpr int N = Vec<T>::N;
    constexpr bool NT = (NTM & 1) != 0;
    constexpr bool NT1 = (NTM & 2) != 0;
    // dynamic LDS only (guide Guideline 17): [H * BLOCK parked vectors][scratch]
    extern __shared__ __attribute__((aligned(16))) uint4 smem[];
    uint4* park = smem;
    uint32_t* scratch = reinterpret_cast<uint32_t*>(smem + H * BLOCK);  // res_scratch_words(BLOCK)
    const int t = (int)threadIdx.x;
    const int g = (int)blockIdx.x;
    const int lane_c = g % kResLanes;  // the workgroup's ticket and drain counter

    trace_entry<BLOCK>(a, t, scratch);
    const uint64_t ticket = draw_ticket(a, lane_c, t);
    if (g >= a.nact * a.bpc) {  // idle: the grid is the CU count on every launch of the slot
        trace_entry_flush<BLOCK>(a, g, t, scratch);
        let_go_of_slot(a, lane_c, t);  // (the ticket's value is not waited for)
        return;
    }
    // Unlike the stack order, thread 0's wave WAITS for the ticket here, before its first load.
    // This order starts pass 1 with R + SB loads per lane (44 at the f32 default); with the ticket
    // in flight ahead of them and the tag made behind them, as the stack order has it, the
    // default rows' encode was 0.6 us (f32) and 0.8-1.0 us (bf16) slower with either exchange
    // (profiles/resident_exchange_ab.jsonl: b_only against parent, ab_all against a_only).  What is left of the
    // deferral here: the other seven waves start loading at once, with no LDS broadcast and no
    // barrier, and the division takes its 32-bit path.
    park_tag<BLOCK>(a, ticket, lane_c, t, scratch);

    const SliceGeom<T, BLOCK> s(a, g);
    const uint4* __restrict__ v = reinterpret_cast<const uint4*>(s.src + s.j0);
    const int64_t v0 = s.v0, v1 = s.v1;
    const int64_t stream0 = v0 + (int64_t)(R + H) * BLOCK;  // first streamed vector

    // ---- pass 1 ------------------------------------------------------------
    uint32_t lo = min_space(T::init_max());
    uint32_t hi = max_space(-T::init_max());
    uint4 held[R > 0 ? R : 1];
    if (v1 > v0) {
        const int64_t vl = v1 - 1;
        load_rows<R, 0, BLOCK, NT1>(v, v0, vl, t, held);
        // the first batch of parked rows is in flight while the held rows are folded
        uint4 cur[SB];
        load_rows<(H < SB ? H : SB), R, BLOCK, NT1>(v, v0, vl, t, cur);
        fold_rows<T, R, false>(held, lo, hi);
        fold_and_park<T, BLOCK, H, SB, R, NT1>(v, v0, vl, t, cur, park, lo, hi);
        // streamed part: the full tiles, then the ragged tail tile
        const int64_t tile = (int64_t)SB * BLOCK;
        const int64_t nfull = v1 > stream0 ? (v1 - stream0) / tile : 0;
        if (nfull > 0) {
            uint4 ra[SB], rb[SB];
            load_tile<SB, BLOCK>(v, stream0, t, ra);
            fold_stream_ascending<T, BLOCK, SB>(v, stream0, nfull, nfull - 1, t, ra, rb, lo, hi);
        }
        for (int j = 0; j < SB; ++j) {
            const int64_t i = stream0 + nfull * tile + j * BLOCK + t;
            if (i < v1) fold_vec<T>(v[i], lo, hi);
        }
    }
    if (s.last) fold_scalars<T, BLOCK>(a, s, lo, hi);
    const int w = t / kWave;
    const uint32_t tag = publish_partials<BLOCK>(a, g, lo, hi, t, w, scratch);

    // the first tile pass 2 re-reads (the top full tile: reverse order) is loaded
    // now, so its latency overlaps the exchange wait instead of following it
    const int64_t tile2 = (int64_t)SB * BLOCK;
    const int64_t nfull2 = v1 > stream0 ? (v1 - stream0) / tile2 : 0;
    uint4 pre[SB], pre2[SB];
    if (nfull2 > 0) load_tile<SB, BLOCK, NT>(v, stream0 + (nfull2 - 1) * tile2, t, pre);
    if (nfull2 > 1) load_tile<SB, BLOCK, NT>(v, stream0 + (nfull2 - 2) * tile2, t, pre2);

    trace_entry_flush<BLOCK>(a, g, t, scratch);
    trace_stamp(a, g, 1);
    const MinMax m = exchange_minmax<T, BLOCK, false>(a, s.cl, tag, t, w, scratch);
    const QParams q = make_qparams(m.mn, m.mx);
    trace_stamp(a, g, 2);

    // ---- pass 2 ------------------------------------------------------------
    write_extras<T, BLOCK>(a, s, m.mn, m.mx, q);
    uint8_t* vdst = s.payload + s.j0;
    if (v1 > stream0) {
        // reverse order (what pass 1 read last is re-read first): the ragged
        // top tile, then the full tiles double-buffered from the top down
        const int64_t tile = (int64_t)SB * BLOCK;
        const int64_t nfull = (v1 - stream0) / tile;
        for (int j = 0; j < SB; ++j) {
            const int64_t i = stream0 + nfull * tile + j * BLOCK + t;
            if (i < v1) quant_store<T>(v[i], q, vdst + i * N);
        }
        if (nfull > 0) {
            // as quant_stream_descending, but the first two tiles are already here
            uint4 ra[SB], rb[SB];
#pragma unroll
            for (int j = 0; j < SB; ++j) { ra[j] = pre[j]; rb[j] = pre2[j]; }  // loaded before the exchange
            for (int64_t i = nfull - 1; i >= 0; i -= 2) {
                if (i != nfull - 1 || nfull < 2) load_tile<SB, BLOCK, NT>(v, stream0 + (i >= 1 ? i - 1 : 0) * tile, t, rb);
                const int64_t ba = stream0 + i * tile;
#pragma unroll
                for (int j = 0; j < SB; ++j) quant_store<T>(ra[j], q, vdst + (ba + j * BLOCK + t) * N);
                load_tile<SB, BLOCK, NT>(v, stream0 + (i >= 2 ? i - 2 : 0) * tile, t, ra);
                if (i >= 1) {
                    const int64_t bb = ba - tile;
#pragma unroll
                    for (int j = 0; j < SB; ++j) quant_store<T>(rb[j], q, vdst + (bb + j * BLOCK + t) * N);
                }
            }
        }
    }
    trace_stamp(a, g, 4);
    if (v0 + (int64_t)(R + H) * BLOCK <= v1) {
        uint8_t* vd = vdst + (v0 + t) * N;
        quant_parked<T, BLOCK, H, SB, R>(park, t, q, vd);
        trace_stamp(a, g, 5);
        quant_rows<T, BLOCK, R, 0, false>(held, q, vd);
    } else {
        // a short slice, guarded per vector against v1 itself
#pragma unroll
        for (int k = 0; k < H; ++k) {
            const int64_t i = v0 + (int64_t)(R + k) * BLOCK + t;
            if (i < v1) quant_store<T>(park[k * BLOCK + t], q, vdst + i * N);
        }
        trace_stamp(a, g, 5);
#pragma unroll
        for (int k = 0; k < R; ++k) {
            const int64_t i = v0 + (int64_t)k * BLOCK + t;
            if (i < v1) quant_store<T>(held[k], q, vdst + i * N);
        }
    }
    finish(a, g, lane_c, t);
}

// Stack order: the same slice layout as minmax_resident_encode_kernel, with the passes
// turned round so that the held rows are never live together with the streaming buffers:
//
//   pass 1: the streamed rows first (ascending, double-buffered), then the parked
//           rows, then the held rows, loaded last into the registers the streaming
//           buffers no longer need
//   pass 2: the held rows first, then the parked rows, then the streamed rows from
//           the top down.  The two top streamed tiles are requested once the held
//           rows are stored (their registers are free by then), so their latency
//           runs under the parked rows' quantisation.
//
// The register budget is max(4R, streaming buffers) + temporaries instead of their
// sum, which is what lets R grow past 28 at BLOCK = 512 without scratch.
// EARLY: the first streamed tile is requested before the ticket is drawn (kept for its rows:
// since this kernel no longer waits for the ticket at its start, it only swaps the first two
// requests; rows 23 and 24 now measure within 0.15 us of each other, profiles/resident_exchange_ab.jsonl).
// ASC: pass 2 re-reads the full streamed tiles in pass 1's order.
// Trace stamps: 0 entry, 1 pass 1 end, 2 exchange end, 6 held rows stored,
// 7 parked rows stored, 3 end.
template <typename T, int BLOCK, int R, int H, int SB, int NTM, bool EARLY, bool ASC>
__global__ __launch_bounds__(BLOCK, 1) void minmax_resident_encode_kernel_stack(ResidentArgs a) {
    constexpr int N = Vec<T>::N;
    constexpr bool NT = (NTM & 1) != 0;
    constexpr bool NT1 = (NTM & 2) != 0;
    static_assert(R > 0 && H > 0, "the stack order keeps rows in VGPRs and in LDS");
    extern __shared__ __attribute__((aligned(16))) uint4 smem[];
    uint4* park = smem;
    uint32_t* scratch = reinterpret_cast<uint32_t*>(smem + H * BLOCK);  // res_scratch_words(BLOCK)
    const int t = (int)threadIdx.x;
    const int g = (int)blockIdx.x;
    const int lane_c = g % kResLanes;  // the workgroup's ticket and drain counter
    const bool idle = g >= a.nact * a.bpc;  // the grid is the CU count on every launch of the slot

    const SliceGeom<T, BLOCK> s(a, idle ? 0 : g);
    const uint4* __restrict__ v = reinterpret_cast<const uint4*>(s.src + s.j0);
    const int64_t v0 = s.v0, v1 = s.v1;
    const int64_t vl = v1 - 1;                              // clamp target (used only when v1 > v0)
    const int64_t stream0 = v0 + (int64_t)(R + H) * BLOCK;  // first streamed vector
    const int64_t tile = (int64_t)SB * BLOCK;
    const int64_t nfull = v1 > stream0 ? (v1 - stream0) / tile : 0;
    const int64_t top = stream0 + nfull * tile;  // the ragged top tile [top, v1), possibly empty

    uint4 ra[SB];
    trace_entry<BLOCK>(a, t, scratch);
    if (EARLY && !idle && nfull > 0) load_tile<SB, BLOCK>(v, stream0, t, ra);
    const uint64_t ticket = draw_ticket(a, lane_c, t);
    if (idle) {
        trace_entry_flush<BLOCK>(a, g, t, scratch);
        let_go_of_slot(a, lane_c, t);
        return;
    }

    // ---- pass 1 ------------------------------------------------------------
    uint32_t lo = min_space(T::init_max());
    uint32_t hi = max_space(-T::init_max());
    uint4 held[R];
    if (v1 > v0) {
        uint4 rb[SB];
        if (!EARLY && nfull > 0) load_tile<SB, BLOCK>(v, stream0, t, ra);
        park_tag<BLOCK>(a, ticket, lane_c, t, scratch);
        if (nfull > 0) fold_stream_ascending<T, BLOCK, SB>(v, stream0, nfull, nfull - 1, t, ra, rb, lo, hi);
        // the ragged top tile and the first batch of parked rows are requested together
        uint4 cur[SB];
        if (v1 > top) load_rows<SB, 0, BLOCK, false>(v, top, vl, t, rb);
        load_rows<(H < SB ? H : SB), R, BLOCK, NT1>(v, v0, vl, t, cur);
        if (v1 > top) fold_rows<T, SB, false>(rb, lo, hi);
        fold_and_park<T, BLOCK, H, SB, R, NT1>(v, v0, vl, t, cur, park, lo, hi);
        // the held rows, last: every streaming buffer above is dead.  The scheduling
        // barriers keep it so: without them the scheduler lifts these loads over the
        // parked rows and expands every row's keys at once, which spills.
        __builtin_amdgcn_sched_barrier(0);
        load_rows<R, 0, BLOCK, NT1>(v, v0, vl, t, held);
        __builtin_amdgcn_sched_barrier(0);
        fold_rows<T, R, true>(held, lo, hi);
    } else {
        park_tag<BLOCK>(a, ticket, lane_c, t, scratch);  // an empty slice
    }
    if (s.last) fold_scalars<T, BLOCK>(a, s, lo, hi);
    const int w = t / kWave;
    const uint32_t tag = publish_partials<BLOCK>(a, g, lo, hi, t, w, scratch);
    trace_entry_flush<BLOCK>(a, g, t, scratch);
    trace_stamp(a, g, 1);

    // The exchange, written out: exchange_minmax<T, BLOCK, true> is this text, but called as a
    // helper it costs this kernel two more SGPRs across the give-up path, and the f32 rows with
    // R = 52 (17, 19, 24, 25), which sit at 256 VGPRs, then spill them to scratch
    // (test_default_rows_use_no_scratch checks row 24).  A change to one is a change to both:
    // tests/test_resident_source.py compares the text between the two marks with the helper's.
    constexpr int W = BLOCK / kWave;
    // exchange_minmax: begin
    if (w < kSweepWaves) {
        const uint64_t deadline = wall_clock64() + a.timeout_ticks;
        uint32_t l = 0, h = 0;
        const bool ok = sweep_chunk(a, s.cl, tag, w, deadline, l, h, true);
        if (lane_id() == 0) {
            if (!ok) scratch[2 * W + 1] = 0u;
            scratch[2 * W + 2 + 2 * w] = l;
            scratch[2 * W + 3 + 2 * w] = h;
        }
    }
    __syncthreads();
    if (scratch[2 * W + 1] == 0u) {
        if (t == 0) __hip_atomic_fetch_add(&a.slot->gave_up, (uint64_t)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        uint32_t l = 0xffffffffu, h = 0xffffffffu;
        fold_missing_slices<T, BLOCK, true>(a, s.cl, tag, l, h);
        workgroup_umin<BLOCK>(l, h, t, w, scratch);
        if (t == 0) {
#pragma unroll
            for (int i = 0; i < kSweepWaves; ++i) {
                scratch[2 * W + 2 + 2 * i] = l;
                scratch[2 * W + 3 + 2 * i] = h;
            }
        }
        __syncthreads();
    }
    uint32_t cmin = scratch[2 * W + 2], cmax = scratch[2 * W + 3];
#pragma unroll
    for (int i = 1; i < kSweepWaves; ++i) {
        cmin = min(cmin, scratch[2 * W + 2 + 2 * i]);
        cmax = min(cmax, scratch[2 * W + 3 + 2 * i]);
    }
    const MinMax m{from_min_space(cmin), from_max_space(cmax)};
    // exchange_minmax: end
    const QParams q = make_qparams(m.mn, m.mx);
    trace_stamp(a, g, 2);

    // ---- pass 2 ------------------------------------------------------------
    write_extras<T, BLOCK>(a, s, m.mn, m.mx, q);
    uint8_t* vdst = s.payload + s.j0;
    const bool whole = stream0 <= v1;  // the whole on-chip part is inside the slice: no per-vector guards
    uint8_t* vd = vdst + (v0 + t) * N;
    const int nloc = on_chip_count<(R + H) * BLOCK>(v0, v1);
    if (whole) quant_rows<T, BLOCK, R, 0, true>(held, q, vd);
    else quant_rows_guarded<T, BLOCK, R, 0>(held, nloc, t, q, vd);
    __builtin_amdgcn_sched_barrier(0);  // no streamed tile is requested while held rows are live
    trace_stamp(a, g, 6);
    // the two top streamed tiles (the ragged one, then the top full one), in flight
    // while the parked rows are quantised
    // (buffers of their own: pass 1's would count as live across the exchange)
    uint4 qa[SB], qb[SB];
    if (v1 > top) load_rows<SB, 0, BLOCK, NT>(v, top, vl, t, qb);
    if (nfull > 0) load_tile<SB, BLOCK, NT>(v, stream0 + (ASC ? 0 : nfull - 1) * tile, t, qa);
    if (whole) quant_parked<T, BLOCK, H, SB, R>(park, t, q, vd);
    else quant_parked_guarded<T, BLOCK, H, R>(park, nloc, t, q, vd);
    trace_stamp(a, g, 7);
    if (v1 > top) quant_top_tile<T, BLOCK, SB>(qb, top, v1, t, q, vdst);
    if (ASC && nfull > 0) quant_stream_ascending<T, BLOCK, SB, NT>(v, stream0, nfull, t, q, vdst, qa, qb);
    else if (nfull > 0) quant_stream_descending<T, BLOCK, SB, NT>(v, stream0, nfull, t, q, vdst, qa, qb);
    finish(a, g, lane_c, t);
}

// Window order: the stream-last order of minmax_resident_encode_kernel, with the stack
// trick applied to the streaming buffers' registers only.  A slice is rows [0, RE) held
// early in VGPRs, rows [RE, RE + H) parked in LDS, rows [RE + H, RE + H + RL) held late,
// the rest streamed:
//
//   pass 1: the early rows, the parked rows, the streamed rows (ascending,
//           double-buffered), then the late rows, loaded into the registers the
//           streaming buffers no longer need
//   pass 2: the late rows first (their registers become pass 2's tile buffers), then
//           the streamed rows from the top down, requested as soon as the late rows are
//           stored, then the parked rows, then the early rows.
//
// Between a streamed row's read and its re-read only the late rows' loads and stores go
// by (the stack order puts the whole on-chip part there), so the re-read finds more of
// its lines in the Infinity Cache; the register budget is
// 4 RE + max(streaming buffers, 4 RL) + temporaries.
// Trace stamps: 0 entry, 1 pass 1 end, 2 exchange end, 6 late rows stored, 4 streamed
// rows stored, 5 parked rows stored, 3 end.
template <typename T, int BLOCK, int RE, int H, int RL, int SB, int NTM>
__global__ __launch_bounds__(BLOCK, 1) void minmax_resident_encode_kernel_window(ResidentArgs a) {
    constexpr int N = Vec<T>::N;
    constexpr bool NT = (NTM & 1) != 0;
    constexpr bool NT1 = (NTM & 2) != 0;
    static_assert(RE > 0 && H > 0 && RL > 0, "the window order keeps rows in VGPRs (early and late) and in LDS");
    extern __shared__ __attribute__((aligned(16))) uint4 smem[];
    uint4* park = smem;
    uint32_t* scratch = reinterpret_cast<uint32_t*>(smem + H * BLOCK);  // res_scratch_words(BLOCK)
    const int t = (int)threadIdx.x;
    const int g = (int)blockIdx.x;
    const int lane_c = g % kResLanes;  // the workgroup's ticket and drain counter

    trace_entry<BLOCK>(a, t, scratch);
    const uint64_t ticket = draw_ticket(a, lane_c, t);
    if (g >= a.nact * a.bpc) {  // idle: the grid is the CU count on every launch of the slot
        trace_entry_flush<BLOCK>(a, g, t, scratch);
        let_go_of_slot(a, lane_c, t);  // (the ticket's value is not waited for)
        return;
    }
    // Unlike the stack order, thread 0's wave WAITS for the ticket here, before its first load.
    // This order starts pass 1 with R + SB loads per lane (44 at the f32 default); with the ticket
    // in flight ahead of them and the tag made behind them, as the stack order has it, the
    // default rows' encode was 0.6 us (f32) and 0.8-1.0 us (bf16) slower with either exchange
    // (profiles/resident_exchange_ab.jsonl: b_only against parent, ab_all against a_only).  What is left of the
    // deferral here: the other seven waves start loading at once, with no LDS broadcast and no
    // barrier, and the division takes its 32-bit path.
    park_tag<BLOCK>(a, ticket, lane_c, t, scratch);

    const SliceGeom<T, BLOCK> s(a, g);
    const uint4* __restrict__ v = reinterpret_cast<const uint4*>(s.src + s.j0);
    const int64_t v0 = s.v0, v1 = s.v1;
    const int64_t vl = v1 - 1;                                   // clamp target (used only when v1 > v0)
    const int64_t stream0 = v0 + (int64_t)(RE + H + RL) * BLOCK;  // first streamed vector
    const int64_t tile = (int64_t)SB * BLOCK;
    const int64_t nfull = v1 > stream0 ? (v1 - stream0) / tile : 0;
    const int64_t top = stream0 + nfull * tile;  // the ragged top tile [top, v1), possibly empty

    // ---- pass 1 ------------------------------------------------------------
    uint32_t lo = min_space(T::init_max());
    uint32_t hi = max_space(-T::init_max());
    uint4 held[RE], late[RL];
    if (v1 > v0) {
        load_rows<RE, 0, BLOCK, NT1>(v, v0, vl, t, held);
        // the first batch of parked rows is in flight while the early rows are folded
        uint4 cur[SB];
        load_rows<(H < SB ? H : SB), RE, BLOCK, NT1>(v, v0, vl, t, cur);
        fold_rows<T, RE, true>(held, lo, hi);
        fold_and_park<T, BLOCK, H, SB, RE, NT1>(v, v0, vl, t, cur, park, lo, hi);
        // streamed rows: the full tiles, then the ragged top tile (clamped)
        uint4 ra[SB], rb[SB];
        if (nfull > 0) {
            load_tile<SB, BLOCK>(v, stream0, t, ra);
            fold_stream_ascending<T, BLOCK, SB>(v, stream0, nfull, nfull - 1, t, ra, rb, lo, hi);
        }
        if (v1 > top) {
            load_rows<SB, 0, BLOCK, false>(v, top, vl, t, rb);
            fold_rows<T, SB, false>(rb, lo, hi);
        }
        // the late rows, last: every streaming buffer above is dead.  The scheduling
        // barriers keep it so (see minmax_resident_encode_kernel_stack).
        __builtin_amdgcn_sched_barrier(0);
        load_rows<RL, RE + H, BLOCK, NT1>(v, v0, vl, t, late);
        __builtin_amdgcn_sched_barrier(0);
        fold_rows<T, RL, true>(late, lo, hi);
    }
    if (s.last) fold_scalars<T, BLOCK>(a, s, lo, hi);
    const int w = t / kWave;
    const uint32_t tag = publish_partials<BLOCK>(a, g, lo, hi, t, w, scratch);
    trace_entry_flush<BLOCK>(a, g, t, scratch);
    trace_stamp(a, g, 1);

    const MinMax m = exchange_minmax<T, BLOCK, true>(a, s.cl, tag, t, w, scratch);
    const QParams q = make_qparams(m.mn, m.mx);
    trace_stamp(a, g, 2);

    // ---- pass 2 ------------------------------------------------------------
    write_extras<T, BLOCK>(a, s, m.mn, m.mx, q);
    uint8_t* vdst = s.payload + s.j0;
    const bool whole = stream0 <= v1;  // the whole on-chip part is inside the slice: no per-vector guards
    uint8_t* vd = vdst + (v0 + t) * N;
    const int nloc = on_chip_count<(RE + H + RL) * BLOCK>(v0, v1);
    if (whole) quant_rows<T, BLOCK, RL, RE + H, true>(late, q, vd);
    else quant_rows_guarded<T, BLOCK, RL, RE + H>(late, nloc, t, q, vd);
    __builtin_amdgcn_sched_barrier(0);  // no streamed tile is requested while late rows are live
    trace_stamp(a, g, 6);
    // the two top streamed tiles (the ragged one, then the top full one) are requested now
    // (buffers of their own: pass 1's would count as live across the exchange)
    {
        uint4 qa[SB], qb[SB];
        if (v1 > top) load_rows<SB, 0, BLOCK, NT>(v, top, vl, t, qb);
        if (nfull > 0) load_tile<SB, BLOCK, NT>(v, stream0 + (nfull - 1) * tile, t, qa);
        if (v1 > top) quant_top_tile<T, BLOCK, SB>(qb, top, v1, t, q, vdst);
        if (nfull > 0) quant_stream_descending<T, BLOCK, SB, NT>(v, stream0, nfull, t, q, vdst, qa, qb);
    }
    __builtin_amdgcn_sched_barrier(0);
    trace_stamp(a, g, 4);
    if (whole) {
        quant_parked<T, BLOCK, H, SB, RE>(park, t, q, vd);
        trace_stamp(a, g, 5);
        quant_rows<T, BLOCK, RE, 0, true>(held, q, vd);
    } else {
        quant_parked_guarded<T, BLOCK, H, RE>(park, nloc, t, q, vd);
        trace_stamp(a, g, 5);
        quant_rows_guarded<T, BLOCK, RE, 0>(held, nloc, t, q, vd);
    }
    finish(a, g, lane_c, t);
}

// ------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------
// Slot keys. hipStreamPerThread is a sentinel that names a DIFFERENT real
// stream on every host thread, so two threads launching on it must not share a
// slot (their tickets and granules would interleave): the sentinel is keyed
// together with the calling thread.  Every other handle is one stream.
struct StreamKey {
    hipStream_t s = nullptr;
    std::thread::id tid{};
    bool operator<(const StreamKey& o) const { return s != o.s ? s < o.s : tid < o.tid; }
    bool operator==(const StreamKey& o) const { return s == o.s && tid == o.tid; }
};
static StreamKey stream_key(hipStream_t s) {
    StreamKey k;
    k.s = s;
    if (s == hipStreamPerThread) k.tid = std::this_thread::get_id();
    return k;
}

struct SlotState {
    bool used = false;
    bool captured = false;  // a graph holds a launch on this slot: never reused (see below)
    StreamKey owner;
    uint64_t last_use = 0;  // LRU clock
    uint64_t launched = 0;  // workgroups launched on the slot since it was zeroed
};

struct ResidentDevice {
    bool init = false, ok = false;
    int grid = 0;
    int clock_khz = 0;
    ResidentSlot* slots = nullptr;
    uint64_t* probe_host = nullptr;  // pinned landing buffer for reading `drained` (kResLanes lines)
    SlotState state[kResSlots];
    std::map<StreamKey, int> stream_slot;
    uint64_t clock = 0;
    bool warned_full = false;
};
static std::mutex g_res_mu;
// streams whose compress calls never take the one-launch encode: streams that run
// codec work concurrently with another codec stream (the scheduler's lanes), where two
// encodes each needing every CU resident would wait on each other (bounded, but slow);
// guarded by g_res_mu
static std::set<hipStream_t>& resident_off_streams() {
    static auto* s = new std::set<hipStream_t>();
    return *s;
}
static uint64_t* g_res_trace = nullptr;  // bagua_minmax_u8_resident_trace
static ResidentDevice g_res_dev[64];

// kernel configurations: {BLOCK, R vectors per lane in VGPRs, H per lane in LDS, SB stream batch}
struct ResidentCfg {
    int block, r, h, sb;
    int ntm;    // non-temporal loads: bit 0 pass-2 re-reads, bit 1 pass-1 loads of the on-chip part
    int stack;  // bit 0: minmax_resident_encode_kernel_stack (stack-order passes); bit 1: its first tile
                // requested before the ticket; bit 2: pass 2 re-reads the streamed tiles bottom-up
    int rl;     // > 0: minmax_resident_encode_kernel_window (window order) with r rows held early and
                // rl rows held late
};
static constexpr ResidentCfg kResCfg[] = {
    {256, 32, 39, 8, 0},   // 0
    {256, 48, 39, 8, 0},   // 1
    {512, 24, 19, 8, 0},   // 2
    {256, 0, 0, 8, 0},     // 3: no retention (Infinity Cache only)
    {256, 32, 0, 8, 0},    // 4: VGPRs only
    {256, 16, 39, 16, 0},  // 5
    {256, 64, 39, 8, 0},   // 6
    {256, 80, 39, 8, 0},   // 7
    {256, 72, 39, 8, 0},   // 8
    {512, 28, 19, 8, 0},   // 9
    {256, 80, 39, 8, 1},    // 10
    {512, 28, 19, 8, 1},       // 11
    // 12: 11 with the on-chip part of pass 1 also loaded non-temporally (the default before the
    // stack and window orders).  The one-bucket loop is unchanged (1,894-1,898 vs 1,892-1,916
    // GiB/s), and alternating buckets -- a bucket last touched a whole other bucket ago, as in
    // training -- gain 1,900-1,928 vs 1,849-1,886 GiB/s (profiles/r04_resident_ntm_ab.jsonl; 13,
    // the on-chip part non-temporal with default re-reads, shortens the encode to 78-80 us but
    // slows the decode after it by as much)
    {512, 28, 19, 8, 3},       // 12
    {512, 28, 19, 8, 2},       // 13: only the on-chip part non-temporal
    // stack-order passes (minmax_resident_encode_kernel_stack): held rows and streaming
    // buffers share registers, so R grows without scratch; non-temporal as in 12
    {512, 40, 19, 8, 3, 1},  // 14
    {512, 44, 19, 8, 3, 1},  // 15
    {512, 48, 19, 8, 3, 1},  // 16
    {512, 52, 19, 4, 3, 1},  // 17 (R = 52 with SB = 8 needs scratch: not built)
    {512, 48, 19, 4, 3, 1},  // 18
    {512, 52, 19, 4, 3, 3},  // 19: 17 with the first streamed tile requested before the ticket
    {512, 28, 19, 8, 3, 1},  // 20: the order alone, at 12's R
    {512, 48, 19, 8, 3, 3},  // 21: 16 with the first streamed tile requested before the ticket
    {512, 44, 19, 8, 3, 3},  // 22: 15, likewise
    {512, 52, 19, 4, 3, 5},  // 23: 17 with pass 2's re-read bottom-up
    {512, 52, 19, 4, 3, 7},  // 24: 19, likewise
    {512, 52, 19, 4, 1, 1},  // 25: 17 with the on-chip part loaded with the default policy
    {512, 52, 19, 4, 1, 5},  // 26: 23, likewise
    {512, 48, 19, 4, 3, 5},  // 27: 18 bottom-up
    {512, 44, 19, 4, 3, 5},  // 28
    {512, 44, 19, 4, 3, 1},  // 29
    {512, 44, 19, 4, 3, 0},  // 30: stream-last (as 12) at R = 44, SB = 4: the window rows' control
    // window order (minmax_resident_encode_kernel_window): r rows held early, rl rows held late in
    // the streaming buffers' registers; non-temporal as in 12
    {512, 44, 19, 4, 3, 0, 8},   // 31: 52 rows in VGPRs (f32 and f16 spill: not candidates there)
    {512, 40, 19, 4, 3, 0, 12},  // 32: 52 rows in VGPRs without scratch for f32 and bf16
};
constexpr int kResNumCfg = (int)(sizeof(kResCfg) / sizeof(kResCfg[0]));
static_assert(kResCfg[29].rl == 0 && kResCfg[31].rl == 8 && kResCfg[32].rl == 12, "row numbers are named by BAGUA_RESIDENT_CFG and the tests");
// The default row per dtype, from the stack-order and window-order sweeps
// (profiles/resident_stack_ab.jsonl, profiles/resident_window_*.json*): f32 takes 32
// (window order, 40 rows held early + 12 late: 55 % of the bucket on chip as in 24, 256 VGPRs, no
// scratch, and a fresher re-read), bf16 takes 31 (44 + 8, likewise) and f16 stays on 29 (stack
// order, R = 44: the f16 kernels need more temporaries; its only window row without scratch,
// 36 + 8, lost to 29).  No default may use scratch (bagua_minmax_u8_resident_cfg_info,
// test_default_rows_use_no_scratch).
template <typename T>
constexpr int resident_default_cfg();
template <>
constexpr int resident_default_cfg<F32>() {
    return 32;
}
template <>
constexpr int resident_default_cfg<BF16>() {
    return 31;
}
template <>
constexpr int resident_default_cfg<F16>() {
    return 29;
}

static size_t resident_lds_bytes(const ResidentCfg& c) {
    return (size_t)c.h * c.block * 16 + 16 * ((size_t)(res_scratch_words(c.block) + 3) / 4);
}

using ResidentKernel = void (*)(ResidentArgs);

// the kernel of row CFG: its order's entry point with the row's parameters
template <typename T, int CFG>
static ResidentKernel resident_kernel_ptr() {
    constexpr ResidentCfg c = kResCfg[CFG];
    if constexpr (c.rl != 0)
        return &minmax_resident_encode_kernel_window<T, c.block, c.r, c.h, c.rl, c.sb, c.ntm>;
    else if constexpr (c.stack != 0)
        return &minmax_resident_encode_kernel_stack<T, c.block, c.r, c.h, c.sb, c.ntm, (c.stack & 2) != 0,
                                                    (c.stack & 4) != 0>;
    else
        return &minmax_resident_encode_kernel<T, c.block, c.r, c.h, c.sb, c.ntm>;
}

// One table per dtype, built from kResCfg: a new row there needs no other edit.
template <typename T, size_t... I>
static ResidentKernel resident_kernel_at(int cfg, std::index_sequence<I...>) {
    static const ResidentKernel table[] = {resident_kernel_ptr<T, (int)I>()...};
    return table[cfg];
}

// nullptr: no such row
template <typename T>
static ResidentKernel resident_kernel_for(int cfg) {
    if (cfg < 0 || cfg >= kResNumCfg) return nullptr;
    return resident_kernel_at<T>(cfg, std::make_index_sequence<kResNumCfg>{});
}

// Per-device state (slot array zeroed once); false when the resident path is
// unavailable on `dev`.  Caller holds g_res_mu.
static bool device_ready(int dev) {
    if (dev < 0 || dev >= 64) return false;
    ResidentDevice& d = g_res_dev[dev];
    if (!d.init) {
        d.init = true;
        int cus = 0, khz = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return false;
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess) return false;
        if (cus < 1 || cus > kResMaxGrid || khz < 1) return false;
        void* p = nullptr;
        const size_t bytes = sizeof(ResidentSlot) * kResSlots;
        if (hipMalloc(&p, bytes) != hipSuccess) return false;
        if (hipMemset(p, 0, bytes) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
            (void)hipFree(p);
            return false;
        }
        // no private stream: with GPU_MAX_HW_QUEUES = 4 one more stream shares a
        // hardware queue with the caller's streams and serialised, e.g., the
        // host-resident bench's H2D and D2H copies (43 -> 27 GiB/s)
        void* h = nullptr;
        if (hipHostMalloc(&h, sizeof(ResidentSlot::drained), hipHostMallocDefault) != hipSuccess) {
            (void)hipFree(p);
            return false;
        }
        d.probe_host = static_cast<uint64_t*>(h);
        d.slots = static_cast<ResidentSlot*>(p);
        d.grid = cus;
        d.clock_khz = khz;
        d.ok = true;
    }
    return d.ok;
}

// Waits until every workgroup launched on slot `idx` has let go of it (its
// `drained` count reaches the launched count).  The counter is read with a copy
// on `via` (a stream the caller knows to be alive: the stream being released,
// or the stream about to take the slot over), which is drained first; the old
// owner's launches may run on another stream, hence the loop.  Caller holds
// g_res_mu.  Rare: release, or more than kResSlots streams.
static int wait_slot_drained(int dev, int idx, hipStream_t via) {
    ResidentDevice& d = g_res_dev[dev];
    const uint64_t want = d.state[idx].launched;
    for (;;) {
        if (hipMemcpyAsync(d.probe_host, &d.slots[idx].drained[0][0], sizeof(ResidentSlot::drained),
                           hipMemcpyDeviceToHost, via) != hipSuccess ||
            hipStreamSynchronize(via) != hipSuccess) {
            g_last_hip_error = (int)hipGetLastError();
            return BAGUA_ERR_HIP;
        }
        uint64_t got = 0;
        for (int c = 0; c < kResLanes; ++c) got += d.probe_host[16 * c];
        if (got >= want) return BAGUA_OK;
        std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
}

// Slot of stream `s` on `dev` (caller holds g_res_mu; device_ready(dev) is
// true), or -1.  A new stream takes a free slot; when all kResSlots are owned
// the least recently used one is reclaimed once every launch issued on it has
// let go of it (wait_slot_drained), so no two launches ever run on one slot at
// once.  The ticket counter stays monotonic across owners.
static int acquire_slot_locked(int dev, hipStream_t s) {
    ResidentDevice& d = g_res_dev[dev];
    const StreamKey key = stream_key(s);
    int idx = -1;
    auto it = d.stream_slot.find(key);
    if (it != d.stream_slot.end()) {
        idx = it->second;
    } else {
        for (int i = 0; i < kResSlots && idx < 0; ++i)
            if (!d.state[i].used && !d.state[i].captured) idx = i;
        if (idx < 0) {
            for (int i = 0; i < kResSlots; ++i)
                if (!d.state[i].captured && (idx < 0 || d.state[i].last_use < d.state[idx].last_use)) idx = i;
            if (idx < 0) return -1;  // every slot is held by a captured graph
            SlotState& old = d.state[idx];
            if (wait_slot_drained(dev, idx, s) != BAGUA_OK) return -1;
            d.stream_slot.erase(old.owner);
            if (!d.warned_full) {
                d.warned_full = true;
                fprintf(stderr,
                        "[bagua-core] one-launch encode: %d streams in use on device %d; reclaiming the least "
                        "recently used slot (release streams with bagua_minmax_u8_release_stream)\n",
                        kResSlots, dev);
            }
        }
        SlotState& st = d.state[idx];
        st.used = true;
        st.owner = key;
        d.stream_slot.emplace(key, idx);
    }
    d.state[idx].last_use = ++d.clock;
    return idx;
}

// Launch plan of the one-launch encode; ok == false: not eligible (the caller
// runs the two-kernel encode)
struct ResidentPlan {
    bool ok = false;
    ResidentKernel kern = nullptr;
    int block = 0;
    int dev = 0;
    size_t lds = 0;
    ResidentArgs a{};
};

template <typename T>
static ResidentPlan resident_plan(const void* input, int64_t in_num_elem, int64_t cs, int p, uint8_t* out,
                                  int64_t out_bytes, int target, hipStream_t s) {
    using S = typename T::storage;
    ResidentPlan pl;
    const int cfg = tune_int("BAGUA_RESIDENT_CFG", resident_default_cfg<T>());
    if (tune_int("BAGUA_RESIDENT", 1) == 0 || cfg < 0 || cfg >= kResNumCfg || p <= 0) return pl;
    {
        std::lock_guard<std::mutex> lk(g_res_mu);
        if (resident_off_streams().count(s)) return pl;
    }
    const int nact = target < 0 ? p : 1;
    const int64_t chunk_offset = out_bytes / p;
    // whole chunks only, every active chunk fully valid, large enough to pay for the exchange
    if (in_num_elem < (target < 0 ? (int64_t)p * cs : ((int64_t)target + 1) * cs)) return pl;
    // below ~12 Mi elements the fixed cost of the exchange (~4 us: publish + sweep across
    // XCDs) and of starting one 512-thread workgroup per CU (~3 us) loses to the
    // two-kernel encode (crossover between 8 Mi and 16 Mi)
    if (cs * nact < tune_int("BAGUA_RESIDENT_MIN_ELEMS", 12 << 20)) return pl;
    for (int i = 0; i < nact; ++i) {
        const int c = target < 0 ? i : target;
        const uintptr_t src = (uintptr_t)(static_cast<const S*>(input) + (int64_t)c * cs);
        const uintptr_t pay = (uintptr_t)(out + (int64_t)c * chunk_offset + 32);
        if (src % sizeof(S) != 0 || common_alignment<T>(src, pay) < 0) return pl;
    }
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return pl;
    int grid = 0, khz = 0;
    {
        std::lock_guard<std::mutex> lk(g_res_mu);
        if (!device_ready(dev)) return pl;
        grid = g_res_dev[dev].grid;
        khz = g_res_dev[dev].clock_khz;
    }
    if (nact > grid) return pl;
    const ResidentCfg& c = kResCfg[cfg];
    const ResidentKernel kern = resident_kernel_for<T>(cfg);
    const void* kfn = reinterpret_cast<const void*>(kern);
    const size_t lds = resident_lds_bytes(c);
    {
        // once per (device, dtype, configuration): dynamic LDS above the default, and
        // one workgroup per CU must be admissible (the exchange needs the grid resident)
        static int admitted[64][kResNumCfg];  // 0 unknown, 1 yes, -1 no
        std::lock_guard<std::mutex> lk(g_res_mu);
        int& st = admitted[dev][cfg];
        if (st == 0) {
            int per_cu = 0;
            st = (hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess &&
                  hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kfn, c.block, lds) == hipSuccess &&
                  per_cu >= 1)
                     ? 1
                     : -1;
            (void)hipGetLastError();
        }
        if (st < 0) return pl;
    }
    ResidentArgs& a = pl.a;
    a.in = input;
    a.cs = cs;
    a.target = target;
    a.nact = nact;
    a.bpc = grid / nact;
    a.grid = grid;
    a.out = out;
    a.chunk_offset = chunk_offset;
    a.out_bytes = out_bytes;
    a.num_chunks = p;
    a.slot = nullptr;  // taken at launch (resident_compress_impl)
    // bounded wait: the exchange normally completes a few us after the slowest
    // workgroup's pass 1, which reads the active chunks; allow that pass to run
    // at as little as 0.5 TB/s before giving up (then the waiting workgroups
    // re-read the missing slices themselves)
    const int64_t active_bytes = cs * nact * (int64_t)sizeof(S);
    const int64_t us = tune_int("BAGUA_RESIDENT_TIMEOUT_US", (int)(200 + active_bytes / 500000));
    a.timeout_ticks = (uint64_t)(us < 0 ? 0 : us) * (uint64_t)khz / 1000u;
    a.trace = g_res_trace;
    pl.kern = kern;
    pl.block = c.block;
    pl.lds = lds;
    pl.dev = dev;
    pl.ok = true;
    return pl;
}

// BAGUA_ERR_UNSUPPORTED: not eligible (the caller runs the two-kernel encode)
template <typename T>
int resident_compress_impl(const void* input, int64_t in_num_elem, int64_t cs, int p, uint8_t* out,
                           int64_t out_bytes, int target, hipStream_t s) {
    ResidentPlan pl = resident_plan<T>(input, in_num_elem, cs, p, out, out_bytes, target, s);
    if (!pl.ok) return BAGUA_ERR_UNSUPPORTED;
    // slot choice, launch and the slot's launched count happen under one lock, so a
    // reclaim (acquire_slot_locked) always waits for the slot's latest launch
    std::lock_guard<std::mutex> lk(g_res_mu);
    ResidentDevice& d = g_res_dev[pl.dev];
    const int idx = acquire_slot_locked(pl.dev, s);
    if (idx < 0) return BAGUA_ERR_UNSUPPORTED;
    // A launch captured into a graph keeps this slot's address: every replay draws
    // tickets and bumps `drained` without the host knowing, so the slot can never
    // be handed to another stream again (16 KiB stays with the graph).
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cap) != hipSuccess) (void)hipGetLastError();
    if (cap != hipStreamCaptureStatusNone) d.state[idx].captured = true;
    pl.a.slot = d.slots + idx;
    const ResidentArgs& a = pl.a;
    launch(pl.kern, dim3(a.grid), dim3(pl.block), (uint32_t)pl.lds, s, a);
    const int rc = check_launch();
    if (rc == BAGUA_OK) d.state[idx].launched += (uint64_t)a.grid;  // each workgroup drains once
    return rc;
}

// Drops the slot of stream `s` on every device once the stream's one-launch
// encodes have let go of it (wait_slot_drained).  Safe to call for streams that never ran
// one; the next launch on `s` takes a slot again.
int release_stream_slot(hipStream_t s) {
    std::lock_guard<std::mutex> lk(g_res_mu);
    const StreamKey key = stream_key(s);
    int rc = BAGUA_OK;
    for (int dev = 0; dev < 64; ++dev) {
        ResidentDevice& d = g_res_dev[dev];
        if (!d.ok) continue;
        auto it = d.stream_slot.find(key);
        if (it == d.stream_slot.end()) continue;
        SlotState& st = d.state[it->second];
        if (st.captured) {  // a graph still holds it: unmap the stream, never reuse the slot
            d.stream_slot.erase(it);
            continue;
        }
        if (wait_slot_drained(dev, it->second, s) != BAGUA_OK) {
            rc = BAGUA_ERR_HIP;
            continue;  // faulted: keep the slot owned
        }
        st.used = false;
        st.last_use = 0;
        d.stream_slot.erase(it);
    }
    return rc;
}

// workgroups of stream `s`'s one-launch encodes that gave up waiting for their
// chunk's partials (measurement: contention with other streams' kernels).
// Synchronises `s`; *count = 0 when the stream never ran the one-launch encode.
int resident_give_ups(hipStream_t s, uint64_t* count) {
    std::lock_guard<std::mutex> lk(g_res_mu);
    *count = 0;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64 || !g_res_dev[dev].ok) return BAGUA_OK;
    ResidentDevice& d = g_res_dev[dev];
    auto it = d.stream_slot.find(stream_key(s));
    if (it == d.stream_slot.end()) return BAGUA_OK;
    if (hipMemcpyAsync(d.probe_host, &d.slots[it->second].gave_up, sizeof(uint64_t), hipMemcpyDeviceToHost, s) !=
            hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
        g_last_hip_error = (int)hipGetLastError();
        return BAGUA_ERR_HIP;
    }
    *count = *d.probe_host;
    return BAGUA_OK;
}

int resident_slots_in_use(int dev) {
    std::lock_guard<std::mutex> lk(g_res_mu);
    if (dev < 0 || dev >= 64 || !g_res_dev[dev].ok) return 0;
    return (int)g_res_dev[dev].stream_slot.size();
}

template <typename T>
int resident_eligible(const void* input, int64_t in_num_elem, int64_t cs, int p, uint8_t* out, int64_t out_bytes,
                      int target, hipStream_t s) {
    return resident_plan<T>(input, in_num_elem, cs, p, out, out_bytes, target, s).ok ? 1 : 0;
}

template int resident_compress_impl<F32>(const void*, int64_t, int64_t, int, uint8_t*, int64_t, int, hipStream_t);
template int resident_compress_impl<F16>(const void*, int64_t, int64_t, int, uint8_t*, int64_t, int, hipStream_t);
template int resident_compress_impl<BF16>(const void*, int64_t, int64_t, int, uint8_t*, int64_t, int, hipStream_t);

}  // namespace bagua

extern "C" int bagua_minmax_u8_release_stream(bagua_stream_t stream) {
    {
        std::lock_guard<std::mutex> lk(bagua::g_res_mu);
        bagua::resident_off_streams().erase(static_cast<hipStream_t>(stream));
    }
    return bagua::release_stream_slot(static_cast<hipStream_t>(stream));
}

extern "C" int bagua_minmax_u8_set_stream_resident(bagua_stream_t stream, int allowed) {
    std::lock_guard<std::mutex> lk(bagua::g_res_mu);
    if (allowed) bagua::resident_off_streams().erase(static_cast<hipStream_t>(stream));
    else bagua::resident_off_streams().insert(static_cast<hipStream_t>(stream));
    return BAGUA_OK;
}

extern "C" int bagua_minmax_u8_resident_slots_in_use(int device_id) { return bagua::resident_slots_in_use(device_id); }

extern "C" int bagua_minmax_u8_resident_give_ups(bagua_stream_t stream, uint64_t* count) {
    if (!count) return BAGUA_ERR_INVALID_ARG;
    return bagua::resident_give_ups(static_cast<hipStream_t>(stream), count);
}

extern "C" int bagua_minmax_u8_resident_trace(void* device_buffer) {
    std::lock_guard<std::mutex> lk(bagua::g_res_mu);
    bagua::g_res_trace = static_cast<uint64_t*>(device_buffer);
    return BAGUA_OK;
}

extern "C" int bagua_minmax_u8_resident_path(int dtype, const void* input, int input_num_element, int chunk_size,
                                             int num_chunks, uint8_t* output, size_t output_bytes, int target_chunk,
                                             bagua_stream_t stream) {
    using namespace bagua;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (num_chunks <= 0 || chunk_size < 0 || target_chunk < -1 || target_chunk >= num_chunks || !input || !output)
        return 0;
    switch (dtype) {
        case BAGUA_DTYPE_F32:
            return resident_eligible<F32>(input, input_num_element, chunk_size, num_chunks, output,
                                          (int64_t)output_bytes, target_chunk, s);
        case BAGUA_DTYPE_F16:
            return resident_eligible<F16>(input, input_num_element, chunk_size, num_chunks, output,
                                          (int64_t)output_bytes, target_chunk, s);
        case BAGUA_DTYPE_BF16:
            return resident_eligible<BF16>(input, input_num_element, chunk_size, num_chunks, output,
                                           (int64_t)output_bytes, target_chunk, s);
    }
    return 0;
}

extern "C" int bagua_minmax_u8_resident_default_cfg(int dtype) {
    using namespace bagua;
    switch (dtype) {
        case BAGUA_DTYPE_F32: return resident_default_cfg<F32>();
        case BAGUA_DTYPE_F16: return resident_default_cfg<F16>();
        case BAGUA_DTYPE_BF16: return resident_default_cfg<BF16>();
    }
    return -1;
}

extern "C" int bagua_minmax_u8_resident_cfg_geometry(int cfg, int* block, int* r, int* h, int* sb, int* stack) {
    using namespace bagua;
    if (cfg < 0 || cfg >= kResNumCfg || !block || !r || !h || !sb || !stack) return BAGUA_ERR_INVALID_ARG;
    *block = kResCfg[cfg].block;
    *r = kResCfg[cfg].r;
    *h = kResCfg[cfg].h;
    *sb = kResCfg[cfg].sb;
    *stack = kResCfg[cfg].stack;
    return BAGUA_OK;
}

extern "C" int bagua_minmax_u8_resident_cfg_order(int cfg, int* order, int* rl) {
    using namespace bagua;
    if (cfg < 0 || cfg >= kResNumCfg || !order || !rl) return BAGUA_ERR_INVALID_ARG;
    *order = kResCfg[cfg].rl != 0 ? 2 : (kResCfg[cfg].stack != 0 ? 1 : 0);
    *rl = kResCfg[cfg].rl;
    return BAGUA_OK;
}

extern "C" int bagua_minmax_u8_resident_cfg_info(int dtype, int cfg, int* num_regs, int* scratch_bytes) {
    using namespace bagua;
    if (!num_regs || !scratch_bytes) return BAGUA_ERR_INVALID_ARG;
    if (cfg < 0) cfg = bagua_minmax_u8_resident_default_cfg(dtype);
    ResidentKernel kern = nullptr;
    switch (dtype) {
        case BAGUA_DTYPE_F32: kern = resident_kernel_for<F32>(cfg); break;
        case BAGUA_DTYPE_F16: kern = resident_kernel_for<F16>(cfg); break;
        case BAGUA_DTYPE_BF16: kern = resident_kernel_for<BF16>(cfg); break;
    }
    if (!kern) return BAGUA_ERR_INVALID_ARG;
    hipFuncAttributes attr{};
    if (hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(kern)) != hipSuccess) {
        g_last_hip_error = (int)hipGetLastError();
        return BAGUA_ERR_HIP;
    }
    *num_regs = attr.numRegs;
    *scratch_bytes = (int)attr.localSizeBytes;
    return BAGUA_OK;
}
