// comm_ops.cpp — the compressed-gradient comm ops on one flat communication
// tensor, enqueued on the communicator's stream.
//
//   centralized (centralized_low_precision_synchronous.rs:30-71):
//     compress(p, all) -> alltoall -> decompress -> reduce_{mean,sum}(rank)
//     -> compress(p, rank) -> allgather -> decompress
//   here:  compress(p, all) -> ncclAllToAll (out of place)
//          -> [fused] dequantise p versions + reduce + min/max partials
//          -> requantise own chunk -> in-place ncclAllGather -> decompress
//   The fused middle reads the p received segments once (p*cs bytes) instead
//   of decompressing them to fp32 and re-reading that (SURVEY.md §7 "hard
//   parts"); every arithmetic step is unchanged, so the result is bitwise
//   that of the reference sequence.  `_unfused` keeps the reference order.
//
//   decentralized (decentralized_low_precision_synchronous.rs:42-152): ring
//   exchange of whole-bucket (n_chunks = 1) compressed diffs.
//
// All buffers come from the device pool; the op waits for its stream before
// returning them (the reference syncs in BaguaCommunicationTensor::drop,
// datatypes/mod.rs:1062-1066).
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include "bagua_core.h"
#include "comm_internal.hpp"
#include "runtime_util.hpp"
#include "schedule.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <mutex>
#include <cstdlib>
#include <vector>

using namespace bagua;

namespace bagua {
thread_local bool g_async_ops = false;
}

namespace {

// BAGUA_OP_PROFILE=1: host us per centralized op, by phase, printed at exit (measurement hook)
struct OpProfile {
    bool on = false;
    std::vector<double> us[5];
    size_t n = 0;
    std::mutex mu;
    OpProfile() {
        const char* e = std::getenv("BAGUA_OP_PROFILE");
        on = e && *e == '1';
    }
    static double median(std::vector<double> v) {
        if (v.empty()) return 0;
        std::nth_element(v.begin(), v.begin() + v.size() / 2, v.end());
        return v[v.size() / 2];
    }
    ~OpProfile() {
        if (on && n)
            fprintf(stderr, "[bagua-core] centralized op host us, medians (n=%zu): plan+alloc %.2f, compress %.2f, "
                            "middle %.2f, tail %.2f, finish %.2f\n", n, median(us[0]), median(us[1]), median(us[2]),
                    median(us[3]), median(us[4]));
    }
};
OpProfile g_op_prof;
struct OpTimer {
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    double lap() {
        const auto now = std::chrono::steady_clock::now();
        const double d = std::chrono::duration<double, std::micro>(now - t).count();
        t = now;
        return d;
    }
};

int plan(BaguaSingleCommunicatorC* c, const bagua_tensor_t* t, int method, Chunking* k) {
    if (!c || !c->t || !t) return BAGUA_ERR_INVALID_ARG;
    if (c->aborted.load()) return BAGUA_ERR_ABORTED;
    k->p = (int)c->nranks;
    k->rank = (int)c->rank;
    if (t->num_elem_allocated % (uint64_t)k->p) return BAGUA_ERR_INVALID_ARG;
    k->cs = t->num_elem_allocated / (uint64_t)k->p;
    k->S = bagua_compressed_size(method, t->dtype, (size_t)k->p, k->cs);
    if (!k->S) return BAGUA_ERR_UNSUPPORTED;
    if (k->S % (size_t)k->p) return BAGUA_ERR_INVALID_ARG;  // communicators/mod.rs:603-607 alltoall alignment
    return BAGUA_OK;
}

bagua_tensor_t u8_view(uint64_t ptr, size_t bytes, int device) {
    bagua_tensor_t v;
    v.ptr = ptr;
    v.num_elem = bytes;
    v.num_elem_allocated = bytes;
    v.dtype = BAGUA_DTYPE_U8;
    v.device_id = device;
    return v;
}

// end of an op: wait for its stream (the reference syncs in
// BaguaCommunicationTensor::drop, datatypes/mod.rs:1062-1066), or, async, return
// with the work enqueued (OpBuffers then go back to the pool behind the stream)
int finish(BaguaSingleCommunicatorC* c, int rc) {
    if (async_ops(c)) return rc;
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (rc) return rc;
    return e == hipSuccess ? BAGUA_OK : BAGUA_ERR_HIP;
}

// a pool buffer of one op: freed after the op's stream sync, or (async) behind the
// op's stream, which the side stream has joined by then (finish_both)
class OpBuffer {
   public:
    explicit OpBuffer(BaguaSingleCommunicatorC* c) : c_(c) {}
    OpBuffer(const OpBuffer&) = delete;
    OpBuffer& operator=(const OpBuffer&) = delete;
    ~OpBuffer() { release(); }
    int allocate(int device, size_t bytes) {
        release();
        return pool_alloc(device, bytes, &ptr_);
    }
    void release() {
        if (!ptr_) return;
        if (async_ops(c_)) {
            const uint64_t s = (uint64_t)(uintptr_t)c_->stream;
            (void)pool_free_after(ptr_, &s, 1);
        } else {
            (void)pool_free(ptr_);
        }
        ptr_ = 0;
    }
    uint64_t ptr() const { return ptr_; }
    template <typename P>
    P* as() const { return reinterpret_cast<P*>((uintptr_t)ptr_); }

   private:
    BaguaSingleCommunicatorC* c_;
    uint64_t ptr_ = 0;
};

#define TRY(x)                 \
    do {                       \
        rc = (x);              \
        if (rc) return finish(c, rc); \
    } while (0)

int env_int(const char* name, long dflt);
int check_schedule(BaguaSingleCommunicatorC* c, int op, int method, const bagua_tensor_t* t, uint64_t chunk,
                   int sched, int average);
enum { kOpCentralized = 1, kOpCentralizedUnfused, kOpCentralizedPipelined, kOpOneBitPipelined, kOpRing,
       kOpRingUnfused, kOpRingPipelined, kOpOneBitErrorFeedback, kOpMxfp4ErrorFeedback, kOpMxfp4Pipelined, kOpMxfp4Stochastic,
       kOpMxfp4StochasticPipelined, kOpMxfp8Pipelined };

// The alltoall of the unpieced ops: slot j of recv <- rank j's segment `rank`.  One rank
// receives its own bytes by a device copy (RCCL's single-rank copy kernel was slower: 1 GiB
// op 1.257 -> 1.222 ms).
int alltoall_or_copy(BaguaSingleCommunicatorC* c, const Chunking& k, const void* send, void* recv) {
    if (k.p > 1) return c->t->alltoall(send, recv, k.S / k.p, BAGUA_DTYPE_U8, c->stream);
    return hipMemcpyAsync(recv, send, k.S, hipMemcpyDeviceToDevice, c->stream) == hipSuccess ? BAGUA_OK : BAGUA_ERR_HIP;
}

// The composed middle step of an error-feedback op, for more chunks than its fused kernel
// takes (BAGUA_ERR_UNSUPPORTED): the reference's decode + reduce into the tensor, then the
// codec's worker encode with the server state on the own chunk alone -- compress_ef(own
// chunk, its segment, segment bytes): one chunk, into its segment of `sb`.
template <typename F>
int composed_ef_middle(const bagua_tensor_t* t, int method, const Chunking& k, int average, const OpBuffer& recv,
                       uint8_t* sb, uint64_t stream, F&& compress_ef) {
    const bagua_tensor_t rv = u8_view(recv.ptr(), k.S, t->device_id);
    const size_t co = k.S / k.p;
    int rc = bagua_tensor_decompress_from(t, method, k.p, &rv, stream);
    if (!rc) rc = bagua_tensor_reduce_inplace(t, k.p, k.rank, average, stream);
    if (rc) return rc;
    return compress_ef((const uint8_t*)(uintptr_t)t->ptr + (size_t)k.rank * k.cs * bagua_dtype_bytes(t->dtype),
                       sb + (size_t)k.rank * co, co);
}

// The keys of one execution of the MXFP4 op with stochastic rounding (MXFP4.md): stage 0,
// this rank's encode of every chunk, and stage 1, its re-encode of the reduced own chunk.
struct MxSrKeys {
    uint64_t worker, server;
};

// bagua_tensor_compress_into for the MXFP4 codec under a key; cs fits an int (plan, below)
int mxfp4_compress_keyed(const bagua_tensor_t* t, const Chunking& k, int target, uint64_t key, const bagua_tensor_t& out,
                         uint64_t stream) {
    if (k.cs > 0x7fffffffULL || t->num_elem > 0x7fffffffULL) return BAGUA_ERR_INVALID_ARG;
    return bagua_mxfp4_compress_sr(t->dtype, (const void*)(uintptr_t)t->ptr, (int)t->num_elem, (int)k.cs, k.p,
                                   (uint8_t*)(uintptr_t)out.ptr, k.S, target, key, (void*)(uintptr_t)stream);
}

// sr (MXFP4 only): both encodes round stochastically under its keys; every other step,
// buffer and collective is the plain op's
int centralized(BaguaSingleCommunicatorC* c, const bagua_tensor_t* t, int average, int method, bool fused,
                const MxSrKeys* sr = nullptr) {
    OpTimer tm;
    double ph[5] = {0, 0, 0, 0, 0};
    struct Commit {
        double* ph;
        ~Commit() {
            if (!g_op_prof.on) return;
            std::lock_guard<std::mutex> g(g_op_prof.mu);
            if (g_op_prof.n >= (1u << 20)) return;  // bounded: a measurement hook, not a log
            for (int i = 0; i < 5; ++i) g_op_prof.us[i].push_back(ph[i]);
            ++g_op_prof.n;
        }
    } commit{ph};
    Chunking k;
    int rc = plan(c, t, method, &k);
    if (rc) return rc;
    DeviceGuard guard(c->device_id);
    if ((rc = check_schedule(c, sr ? kOpMxfp4Stochastic : fused ? kOpCentralized : kOpCentralizedUnfused, method, t,
                             k.cs, 1, average)))
        return rc;
    const uint64_t s = (uint64_t)(uintptr_t)c->stream;
    if (k.p == 1 && fused && method == BAGUA_COMPRESSION_MINMAX_UINT8 && t->num_elem == t->num_elem_allocated &&
        k.cs <= 0x7fffffffULL && env_int("BAGUA_ONE_RANK_FUSED", 1) != 0) {
        // one rank: the whole sequence as the min/max pass + one table-driven pass over the
        // tensor (bagua_minmax_u8_centralized_one_rank: the second header follows from the
        // first), no compressed buffer at all; BAGUA_ONE_RANK_FUSED=0: the steps below (A/B)
        const size_t ws_bytes = bagua_minmax_u8_workspace_bytes((int)k.cs, 1);
        uint64_t ws = 0;
        if ((rc = stream_workspace(c->device_id, s, ws_bytes, &ws)) != BAGUA_OK) return finish(c, rc);
        ph[0] = tm.lap();
        rc = bagua_minmax_u8_centralized_one_rank(t->dtype, (void*)(uintptr_t)t->ptr, (int)k.cs, average,
                                                  (void*)(uintptr_t)ws, ws_bytes, (void*)(uintptr_t)s);
        ph[2] = tm.lap();
        return finish(c, rc);
    }
    if (k.p == 1 && fused && method == BAGUA_COMPRESSION_ONEBIT && t->num_elem == t->num_elem_allocated &&
        k.cs <= 0x7fffffffULL && env_int("BAGUA_ONE_RANK_FUSED", 1) != 0) {
        // the same for the 1-bit codec: encode pass, one workgroup for both scales, one
        // pass writing +-scale2 from the bits (bagua_onebit_centralized_one_rank)
        const size_t ws_bytes = bagua_onebit_one_rank_workspace_bytes((int)k.cs);
        uint64_t ws = 0;
        if ((rc = stream_workspace(c->device_id, s, ws_bytes, &ws)) != BAGUA_OK) return finish(c, rc);
        ph[0] = tm.lap();
        rc = bagua_onebit_centralized_one_rank(t->dtype, (void*)(uintptr_t)t->ptr, (int)k.cs, average,
                                               (void*)(uintptr_t)ws, ws_bytes, (void*)(uintptr_t)s);
        ph[2] = tm.lap();
        return finish(c, rc);
    }
    // 2. (below) alltoall.  One rank receives its own bytes: the MinMax steps below read them
    // from `send` itself (their reads and the requantise's writes are separate kernels in
    // stream order; no recv buffer), the 1-bit middle step -- one kernel that reads every
    // segment's header while rewriting its own -- from a device copy (alltoall_or_copy)
    const bool self_alias = k.p == 1 && method == BAGUA_COMPRESSION_MINMAX_UINT8;
    OpBuffer send(c), recv(c);
    TRY(send.allocate(c->device_id, k.S));
    if (!self_alias) TRY(recv.allocate(c->device_id, k.S));
    const bagua_tensor_t sv = u8_view(send.ptr(), k.S, c->device_id);
    const bagua_tensor_t rv = u8_view(recv.ptr(), k.S, c->device_id);
    ph[0] = tm.lap();
    // 1. compress every chunk (target -1)
    if (sr) TRY(mxfp4_compress_keyed(t, k, -1, sr->worker, sv, s));
    else TRY(bagua_tensor_compress_into(t, method, k.p, s, -1, &sv));
    ph[1] = tm.lap();
    if (!self_alias) TRY(alltoall_or_copy(c, k, send.as<void>(), recv.as<void>()));
    uint8_t* const rbuf = self_alias ? send.as<uint8_t>() : recv.as<uint8_t>();
    const bagua_tensor_t* const rview = self_alias ? &sv : &rv;
    // 3. reduce the p received versions of the own chunk and requantise it into send[rank]
    bool done = false;
    // the fused kernels treat every allocated element as valid (the reference
    // compresses num_elements(), datatypes/mod.rs:339): other tensors run unfused
    if (fused && method == BAGUA_COMPRESSION_MINMAX_UINT8 && t->num_elem == t->num_elem_allocated) {
        const size_t ws_bytes = bagua_minmax_u8_workspace_bytes((int)k.cs, k.p);
        uint64_t ws = 0;
        if ((rc = stream_workspace(c->device_id, s, ws_bytes, &ws)) != BAGUA_OK) return finish(c, rc);
        // the reduced chunk is dead (step 5's decompress rewrites every element): below
        // p = 2*sizeof(T) recomputing it from the p received segments moves fewer bytes
        // than storing it and reading it back (p*cs vs 2*cs*sizeof(T); p = 1: 10 -> 3 bytes
        // per element); BAGUA_REDUCE_RECOMPUTE=0/1 forces either way (A/B)
        const int rcm = env_int("BAGUA_REDUCE_RECOMPUTE", -1);
        const bool recompute = rcm >= 0 ? rcm != 0 : (size_t)k.p < 2 * bagua_dtype_bytes(t->dtype);
        if (recompute && k.p == 1) {
            // one rank: the own chunk is the whole tensor and nothing is gathered, so the
            // requantise writes the final decompressed values (no step-5 launch) and not the
            // requantised segment, which nothing would read
            rc = bagua_minmax_u8_reduce_requantize_final(t->dtype, rbuf, k.S, (int)k.cs, k.p, (void*)(uintptr_t)t->ptr,
                                                         average, nullptr, 0, k.rank,
                                                         (void*)(uintptr_t)ws, ws_bytes, (void*)(uintptr_t)s);
            ph[2] = tm.lap();
            if (rc == BAGUA_OK) {
                const int r = finish(c, BAGUA_OK);
                ph[4] = tm.lap();
                return r;
            }
        } else {
            rc = bagua_minmax_u8_reduce_requantize(t->dtype, rbuf, k.S, (int)k.cs, k.p,
                                                   recompute ? nullptr : (void*)(uintptr_t)t->ptr, average,
                                                   send.as<uint8_t>(), k.S, k.rank, (void*)(uintptr_t)ws, ws_bytes,
                                                   (void*)(uintptr_t)s);
        }
        if (rc == BAGUA_OK) done = true;
        else if (rc != BAGUA_ERR_UNSUPPORTED) return finish(c, rc);
    } else if (fused && method == BAGUA_COMPRESSION_ONEBIT && t->num_elem == t->num_elem_allocated) {
        const size_t ws_bytes = bagua_onebit_workspace_bytes((int)k.cs, 1);
        uint64_t ws = 0;
        if ((rc = stream_workspace(c->device_id, s, ws_bytes, &ws)) != BAGUA_OK) return finish(c, rc);
        // the reduced chunk is not stored: step 5's decompress rewrites every element
        rc = bagua_onebit_reduce_requantize(t->dtype, recv.as<uint8_t>(), k.S, (int)k.cs, k.p,
                                            nullptr, average, send.as<uint8_t>(), k.S, k.rank,
                                            (void*)(uintptr_t)ws, ws_bytes, (void*)(uintptr_t)s);
        if (rc == BAGUA_OK) done = true;
        else if (rc != BAGUA_ERR_UNSUPPORTED) return finish(c, rc);
    } else if (fused && method == BAGUA_COMPRESSION_MXFP4 && t->num_elem == t->num_elem_allocated) {
        // one kernel, no workspace; the reduced chunk is not stored (step 5 rewrites every element)
        rc = sr ? bagua_mxfp4_reduce_requantize_sr(t->dtype, recv.as<uint8_t>(), k.S, (int)k.cs, k.p, average,
                                                   send.as<uint8_t>(), k.S, k.rank, sr->server, (void*)(uintptr_t)s)
                : bagua_mxfp4_reduce_requantize(t->dtype, recv.as<uint8_t>(), k.S, (int)k.cs, k.p, nullptr, average,
                                                send.as<uint8_t>(), k.S, k.rank, (void*)(uintptr_t)s);
        if (rc == BAGUA_OK) done = true;
        else if (rc != BAGUA_ERR_UNSUPPORTED) return finish(c, rc);
    } else if (fused && method == BAGUA_COMPRESSION_MXFP8 && t->num_elem == t->num_elem_allocated) {
        // likewise (MXFP8.md)
        rc = bagua_mxfp8_reduce_requantize(t->dtype, recv.as<uint8_t>(), k.S, (int)k.cs, k.p, nullptr, average,
                                           send.as<uint8_t>(), k.S, k.rank, (void*)(uintptr_t)s);
        if (rc == BAGUA_OK) done = true;
        else if (rc != BAGUA_ERR_UNSUPPORTED) return finish(c, rc);
    }
    if (!done) {
        TRY(bagua_tensor_decompress_from(t, method, k.p, rview, s));
        TRY(bagua_tensor_reduce_inplace(t, k.p, k.rank, average, s));
        if (sr) TRY(mxfp4_compress_keyed(t, k, k.rank, sr->server, sv, s));
        else TRY(bagua_tensor_compress_into(t, method, k.p, s, k.rank, &sv));
    }
    // 4. allgather the requantised chunks in place (one rank: nothing to move), 5. decompress everything
    if (k.p > 1) TRY(bagua_comm_allgather_inplace(c, &sv));
    TRY(bagua_tensor_decompress_from(t, method, k.p, &sv, s));
    return finish(c, BAGUA_OK);
}

int env_int(const char* name, long dflt) {
    const char* v = std::getenv(name);
    return v && *v ? (int)std::strtol(v, nullptr, 10) : (int)dflt;
}

// ---- BAGUA_CHECK_SCHEDULE: ranks compare what they are about to post ---------
// Opt-in (ScheduleConfig::check, equal on every rank): before an op's first
// collective the ranks allgather a small descriptor of the op -- which op, codec,
// dtype, p, chunk size, tensor sizes, piece schedule, average, op number -- on the
// op's own communicator and stream, and every rank returns BAGUA_ERR_INVALID_ARG
// when any two differ, before any of them posts a collective the others do not
// match (which over RCCL hangs; centralized_low_precision_synchronous.rs:30-71 is
// the sequence every rank must post alike).  Costs one small allgather and a host
// round trip per op.
//
// The op number assumes ONE issuing thread per communicator (its lane views count on
// the parent): ops issued concurrently from several threads could number differently
// on different ranks and report a false mismatch.  A stream being captured into a HIP
// graph cannot be synchronised, so the check is refused there (BAGUA_ERR_UNSUPPORTED)
// rather than breaking the capture.
constexpr int kDescFields = 10;
const char* const kDescName[kDescFields] = {"op",       "method",         "dtype",   "nranks",  "chunk elements",
                                            "num_elem", "num_elem_alloc", "schedule", "average", "op number"};

int check_schedule(BaguaSingleCommunicatorC* c, int op, int method, const bagua_tensor_t* t, uint64_t chunk,
                   int sched, int average) {
    if (!c->cfg.check || c->nranks <= 1) return BAGUA_OK;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(c->stream, &cap) != hipSuccess) return BAGUA_ERR_HIP;
    if (cap != hipStreamCaptureStatusNone) {
        BAGUA_LOG(0, "BAGUA_CHECK_SCHEDULE: the op's stream is being captured; the check needs a host round trip");
        return BAGUA_ERR_UNSUPPORTED;
    }
    BaguaSingleCommunicatorC* root = c->parent ? c->parent : c;
    const int64_t mine[kDescFields] = {op, method, t->dtype, (int64_t)c->nranks, (int64_t)chunk, (int64_t)t->num_elem,
                                       (int64_t)t->num_elem_allocated, sched, average != 0,
                                       (int64_t)root->op_seq.fetch_add(1)};
    const size_t one = sizeof(mine), p = c->nranks;
    PoolBuffer buf;
    int rc = buf.allocate(c->device_id, one * p);
    if (rc) return rc;
    std::vector<int64_t> all(kDescFields * p);
    uint8_t* base = buf.as<uint8_t>();
    if (hipMemcpyAsync(base + c->rank * one, mine, one, hipMemcpyHostToDevice, c->stream) != hipSuccess)
        return BAGUA_ERR_HIP;
    if ((rc = c->t->allgather(base + c->rank * one, base, one, BAGUA_DTYPE_U8, c->stream)) != BAGUA_OK) return rc;
    if (hipMemcpyAsync(all.data(), base, one * p, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
        return BAGUA_ERR_HIP;
    for (size_t j = 0; j < p; ++j)
        for (int f = 0; f < kDescFields; ++f)
            if (all[j * kDescFields + f] != mine[f]) {
                BAGUA_LOG(0, "rank %zu: op schedule mismatch with rank %zu: %s %lld here, %lld there", c->rank, j,
                          kDescName[f], (long long)mine[f], (long long)all[j * kDescFields + f]);
                return BAGUA_ERR_INVALID_ARG;
            }
    return BAGUA_OK;
}

// Whether the op runs pipelined: every rank must decide alike (they would otherwise
// post different collectives), so only values equal on every rank enter -- sizes,
// dtype, p -- never this rank's pointer.  A rank whose tensor is not 16-B aligned
// runs the same schedule on an aligned staging copy (with_aligned_copy).
bool pipeline_fits(const bagua_tensor_t* t, const Chunking& k, size_t vec) {
    // vec: the codec's vector rule -- its kernels move 16-B vectors of the tensor, so a chunk
    // must be whole vectors and a segment whole multiples of the `vec` payload bytes one
    // vector encodes to (0: the codec takes any chunk).  p <= 16: the fused middle steps.
    // cs fits an int: the kernels' chunk_size (larger tensors fall back to the unpieced op,
    // whose compress refuses them).
    return k.p <= 16 && t->num_elem == t->num_elem_allocated && k.cs <= 0x7fffffffULL &&
           (!vec || ((k.S / k.p) % vec == 0 && (k.cs * bagua_dtype_bytes(t->dtype)) % 16 == 0));
}

// Runs op(descriptors) on 16-B aligned copies of the tensors that are not aligned:
// copied into one pool block on the op's stream first and back after the op (whose
// work, side stream included, the stream has joined by then).  The aligned tensors
// are passed as they are.
template <typename F>
int with_aligned_copy(BaguaSingleCommunicatorC* c, std::vector<const bagua_tensor_t*> ts, F&& op) {
    size_t total = 0;
    std::vector<size_t> off(ts.size(), 0);
    for (size_t i = 0; i < ts.size(); ++i)
        if (ts[i]->ptr % 16) {
            off[i] = total;
            total += (ts[i]->num_elem_allocated * bagua_dtype_bytes(ts[i]->dtype) + 255) / 256 * 256;
        }
    if (!total) return op(ts);
    OpBuffer stage(c);
    int rc = stage.allocate(c->device_id, total);
    if (rc) return finish(c, rc);
    std::vector<bagua_tensor_t> copies(ts.size());
    std::vector<const bagua_tensor_t*> use(ts.size());
    for (size_t i = 0; i < ts.size(); ++i) {
        use[i] = ts[i];
        if (!(ts[i]->ptr % 16)) continue;
        copies[i] = *ts[i];
        copies[i].ptr = stage.ptr() + off[i];
        use[i] = &copies[i];
        if (hipMemcpyAsync((void*)(uintptr_t)copies[i].ptr, (const void*)(uintptr_t)ts[i]->ptr,
                           ts[i]->num_elem_allocated * bagua_dtype_bytes(ts[i]->dtype), hipMemcpyDeviceToDevice,
                           c->stream) != hipSuccess)
            return finish(c, BAGUA_ERR_HIP);
    }
    rc = op(use);
    if (rc) return rc;  // the op finished (or enqueued) its own failure handling
    for (size_t i = 0; i < ts.size(); ++i)
        if (ts[i]->ptr % 16 &&
            hipMemcpyAsync((void*)(uintptr_t)ts[i]->ptr, (const void*)(uintptr_t)use[i]->ptr,
                           ts[i]->num_elem_allocated * bagua_dtype_bytes(ts[i]->dtype), hipMemcpyDeviceToDevice,
                           c->stream) != hipSuccess)
            return finish(c, BAGUA_ERR_HIP);
    return finish(c, BAGUA_OK);
}

// one piece of the alltoall (send -> recv) or of the in-place allgather (send): the byte
// ranges r[0 .. nr) of every segment in one group, each pair's transfers posted in range
// order on both ends; empty ranges move nothing
int exchange_ranges(BaguaSingleCommunicatorC* c, const Chunking& k, uint8_t* send, uint8_t* recv, const ByteRange* r,
                    int nr, bool alltoall) {
    bool any = false;
    for (int i = 0; i < nr; ++i) any = any || r[i].hi > r[i].lo;
    if (!any) return BAGUA_OK;
    const size_t co = k.S / k.p;
    hipStream_t s1 = c->side;
    for (int i = 0; i < nr && alltoall; ++i)
        if (r[i].hi > r[i].lo && hipMemcpyAsync(recv + k.rank * co + r[i].lo, send + k.rank * co + r[i].lo,
                                                r[i].hi - r[i].lo, hipMemcpyDeviceToDevice, s1) != hipSuccess)
            return BAGUA_ERR_HIP;
    if (k.p == 1) return BAGUA_OK;
    int rc = c->t->group_start();
    for (int j = 0; j < k.p && !rc; ++j) {
        if (j == k.rank) continue;
        for (int i = 0; i < nr && !rc; ++i) {
            if (r[i].hi <= r[i].lo) continue;
            const size_t lo = r[i].lo, len = r[i].hi - lo;
            if (alltoall) {
                rc = c->t->send(send + j * co + lo, len, BAGUA_DTYPE_U8, j, s1);
                if (!rc) rc = c->t->recv(recv + j * co + lo, len, BAGUA_DTYPE_U8, j, s1);
            } else {
                rc = c->t->send(send + k.rank * co + lo, len, BAGUA_DTYPE_U8, j, s1);
                if (!rc) rc = c->t->recv(send + j * co + lo, len, BAGUA_DTYPE_U8, j, s1);
            }
        }
    }
    const int rc_end = c->t->group_end();
    return rc ? rc : rc_end;
}

int finish_both(BaguaSingleCommunicatorC* c, int rc) {
    if (async_ops(c)) {
        // the op's stream takes over the side stream's tail: its completion is the op's
        if (hipEventRecord(c->join, c->side) != hipSuccess || hipStreamWaitEvent(c->stream, c->join, 0) != hipSuccess)
            return rc ? rc : BAGUA_ERR_HIP;
        return rc;
    }
    const hipError_t e1 = hipStreamSynchronize(c->side);
    const int r0 = finish(c, rc);
    if (r0) return r0;
    return e1 == hipSuccess ? BAGUA_OK : BAGUA_ERR_HIP;
}

#define TRY2(x)                          \
    do {                                 \
        rc = (x);                        \
        if (rc) return finish_both(c, rc); \
    } while (0)
#define HIP2(x) TRY2((x) == hipSuccess ? BAGUA_OK : BAGUA_ERR_HIP)

// What every pipelined body does between its preparation and its first kernel.  Before: the
// side stream and the op's events (ensure_side: those the op carves up and one more, the
// last, that only the fork uses), the piece table, buffers and workspace; a failure there
// returns through finish.  fork_side: the side stream starts after everything already
// queued on the op's stream; from here on a failure returns through finish_both.
int fork_side(BaguaSingleCommunicatorC* c, hipEvent_t start) {
    if (hipEventRecord(start, c->stream) != hipSuccess) return BAGUA_ERR_HIP;
    return hipStreamWaitEvent(c->side, start, 0) == hipSuccess ? BAGUA_OK : BAGUA_ERR_HIP;
}

// The side stream's part of one phase of an op whose pieces are exchanged one by one: piece
// q's group once ready[q] is recorded on the op's stream, then done[q] for its consumer.
int exchange_pieces(BaguaSingleCommunicatorC* c, const Chunking& k, uint8_t* sb, uint8_t* rb,
                    const std::vector<Piece>& tab, bool alltoall, hipEvent_t* ready, hipEvent_t* done) {
    for (size_t q = 0; q < tab.size(); ++q) {
        if (hipStreamWaitEvent(c->side, ready[q], 0) != hipSuccess) return BAGUA_ERR_HIP;
        const int rc = exchange_ranges(c, k, sb, rb, alltoall ? tab[q].a2a : tab[q].ag, 2, alltoall);
        if (rc) return rc;
        if (hipEventRecord(done[q], c->side) != hipSuccess) return BAGUA_ERR_HIP;
    }
    return BAGUA_OK;
}

// ---- pipelined centralized op ---------------------------------------------
// The same op as above with each chunk cut into `pieces` element ranges and
// two streams: the codec runs on the communicator's stream, the exchange of
// piece k on a side stream while the codec works on piece k+1:
//
//   stream: partials | Q0 Q1 .. Qk | R0 R1 .. Rk RQ | D0 D1 .. Dk
//   side  :             A0 A1 .. Ak            G0 G1 .. Gk
//   (Q quantise, A alltoall as grouped send/recv, R fused dequantise+reduce,
//    RQ requantise own chunk, G allgather, D dequantise; each arrow an event)
//
// A segment keeps one header per chunk and the pieces are disjoint byte ranges
// of it, so every buffer holds exactly the bytes of the unpieced op and the
// result is bit-identical to it (and to the reference sequence).
int centralized_pipelined(BaguaSingleCommunicatorC* c, const bagua_tensor_t* t, int average, int pieces) {
    Chunking k;
    if (!valid_schedule(pieces)) return BAGUA_ERR_INVALID_ARG;
    int rc = plan(c, t, BAGUA_COMPRESSION_MINMAX_UINT8, &k);
    if (rc) return rc;
    const int caller = pieces;
    pieces &= BAGUA_PIECES_COUNT_MASK;
    if (pieces < 1) pieces = k.p == 1 ? 1 : auto_pieces(c->cfg, k.cs);  // one rank: no exchange to hide
    const size_t vec = t->dtype == BAGUA_DTYPE_F32 ? 4 : 8;  // payload bytes per 16-B vector
    if (pieces == 1 || !pipeline_fits(t, k, vec)) return centralized(c, t, average, BAGUA_COMPRESSION_MINMAX_UINT8, true);
    if (t->ptr % 16)
        return with_aligned_copy(c, {t}, [&](const std::vector<const bagua_tensor_t*>& u) {
            return centralized_pipelined(c, u[0], average, pieces | (caller & BAGUA_PIECES_TAPERED));
        });
    const int sched = op_schedule(c->cfg, pieces, caller);
    DeviceGuard guard(c->device_id);
    if ((rc = check_schedule(c, kOpCentralizedPipelined, BAGUA_COMPRESSION_MINMAX_UINT8, t, k.cs, sched, average)))
        return rc;
    if (c->ensure_side(4 * (size_t)pieces + 1)) return finish(c, BAGUA_ERR_HIP);
    hipStream_t s0 = c->stream;
    hipEvent_t* quantised = c->events.data();
    hipEvent_t* exchanged = quantised + pieces;
    hipEvent_t* gathered = exchanged + pieces;
    hipEvent_t* requantised_piece = gathered + pieces;
    std::vector<Piece> tab;
    TRY(minmax_pieces(k, sched, &tab));
    const int dt = t->dtype, cs = (int)k.cs, p = k.p;
    void* x = (void*)(uintptr_t)t->ptr;
    OpBuffer send(c), recv(c);
    TRY(send.allocate(c->device_id, k.S));
    TRY(recv.allocate(c->device_id, k.S));
    uint8_t* sb = send.as<uint8_t>();
    uint8_t* rb = recv.as<uint8_t>();
    size_t ws_bytes = bagua_minmax_u8_workspace_bytes(cs, p);
    const size_t pws = bagua_minmax_u8_pipeline_workspace_bytes(cs, sched);
    if (pws > ws_bytes) ws_bytes = pws;
    uint64_t wsp = 0;
    if ((rc = stream_workspace(c->device_id, (uint64_t)(uintptr_t)s0, ws_bytes, &wsp)) != BAGUA_OK)
        return finish(c, rc);
    void* ws = (void*)(uintptr_t)wsp;
    TRY2(fork_side(c, requantised_piece[pieces]));
    // 1. min/max of every chunk, then quantise + exchange piece by piece
    // (backwards: the chunks' first pieces, quantised next, stay in the Infinity Cache)
    TRY2(bagua_minmax_u8_compress_stage(env_int("BAGUA_PARTIALS_FORWARD", 0) ? 1 : 5, dt, x, (int)t->num_elem, cs, p,
                                        sb, k.S, ws, ws_bytes, -1, s0));
    for (int q = 0; q < pieces; ++q) {
        const int b = tab[q].b, e = tab[q].e;
        if (q == 0 || b < e)
            TRY2(bagua_minmax_u8_quantize_range(dt, x, (int)t->num_elem, cs, p, sb, k.S, ws, ws_bytes, -1, b, e, s0));
        HIP2(hipEventRecord(quantised[q], s0));
    }
    TRY2(exchange_pieces(c, k, sb, rb, tab, true, quantised, exchanged));
    // 2. reduce the p received versions of the own chunk piece by piece, requantise it.
    // The reduced chunk need not be stored (the final dequantise rewrites the own chunk
    // of x): with `recompute` each reduce piece emits its min/max partials only and the
    // requantise recomputes the piece from the received segments, (2p + 1) L bytes per
    // piece of L elements instead of (p + 2 sizeof(T) + 1) L, at twice the table
    // lookups.  Measured on 1 GiB fp32 (tools/pipeline_kernels_probe.py,
    // profiles/r06_pipe_probe_p{4,8}.json) it pays at p = 2 only -- the middle step 71.0
    // -> 58.0 us with 4 pieces, 42.6 -> 35.4 with 8 -- and loses from p = 4 on (the
    // lookups, not the bytes, bound these kernels), so it runs where 2p <= sizeof(T).
    // BAGUA_PIPE_RECOMPUTE=0 / 1 forces either (A/B).
    const int rc_env = env_int("BAGUA_PIPE_RECOMPUTE", -1);
    const bool recompute = rc_env >= 0 ? rc_env != 0 : 2 * (size_t)p <= bagua_dtype_bytes(dt);
    // every piece dequantises the same p segment headers: reduce piece 0 leaves its tables
    // in the workspace and the later pieces (and the recompute requantise) copy them
    // (BAGUA_PIECES_TABLES; BAGUA_PIPE_TABLES=0: every launch builds its own, A/B)
    const int tsched = sched | (env_int("BAGUA_PIPE_TABLES", 1) != 0 ? BAGUA_PIECES_TABLES : 0);
    for (int q = 0; q < pieces; ++q) {
        HIP2(hipStreamWaitEvent(s0, exchanged[q], 0));
        TRY2(bagua_minmax_u8_reduce_piece(dt, rb, k.S, cs, p, recompute ? nullptr : x, average, k.rank, tsched, q, ws,
                                          ws_bytes, s0));
    }
    // requantise piece by piece, so the allgather of piece q starts while piece q+1 is
    // requantised.  Every requantise needs the whole chunk's min/max, and each of its
    // workgroups folds all pieces' partials itself.  BAGUA_PIPE_PREFOLD=1 folds them once
    // in one workgroup first (BAGUA_PIECES_FOLDED): measured no faster -- the middle step
    // 58.7 vs 58.9 us at p = 2, 43.4 vs 44.3 at p = 8 (profiles/r06_pipe_probe_p4_prefold.json)
    // -- the fold is not what bounds the requantise, so it is off (A/B switch)
    const bool prefold = env_int("BAGUA_PIPE_PREFOLD", 0) != 0;
    if (prefold) TRY2(bagua_minmax_u8_fold_piece_partials(dt, cs, sched, ws, ws_bytes, s0));
    const int rq_sched = tsched | (prefold ? BAGUA_PIECES_FOLDED : 0);
    for (int q = 0; q < pieces; ++q) {
        if (recompute)
            TRY2(bagua_minmax_u8_reduce_requantize_piece(dt, rb, k.S, cs, p, average, sb, k.S, k.rank, rq_sched, q, ws,
                                                         ws_bytes, s0));
        else
            TRY2(bagua_minmax_u8_requantize_piece(dt, x, cs, p, sb, k.S, k.rank, rq_sched, q, ws, ws_bytes, s0));
        HIP2(hipEventRecord(requantised_piece[q], s0));
    }
    // 3. allgather + dequantise piece by piece
    TRY2(exchange_pieces(c, k, sb, rb, tab, false, requantised_piece, gathered));
    for (int q = 0; q < pieces; ++q) {
        HIP2(hipStreamWaitEvent(s0, gathered[q], 0));
        if (tab[q].b < tab[q].e)
            TRY2(bagua_minmax_u8_decompress_range(dt, sb, k.S, cs, p, x, tab[q].b, tab[q].e, s0));
    }
    return finish_both(c, BAGUA_OK);
}

// The 1-bit op, pipelined the same way.  A 1-bit header (scale) needs the whole
// chunk's |x| partials, so the alltoall sends the sign bits of piece q as soon
// as they are encoded and the headers with the last piece; the fused middle
// step (which needs every received scale) runs once, after the last piece.
// The allgather sends the headers with piece 0 and the decode of piece q
// follows its arrival.
//
//   stream: E0 E1 .. Ek F | R+F | D0 D1 .. Dk
//   side  :    A0 A1 .. Ak+hdr   G0+hdr G1 .. Gk
//
// The same schedule runs the op with error feedback when `st` is given: E, F
// and R+F are then the `_ef` kernels.  The worker state (carry, one scale per chunk)
// compensates what this rank encodes for the alltoall, the server state (carry of
// the own chunk, one scale) what it re-encodes for the allgather; alltoall,
// allgather, final decode and segment sizes are the plain op's.  Each piece's encode
// reads the worker scales that the step's one finalize (after the last piece, same
// stream) then overwrites.
struct EfState {
    float *wc, *ws, *sc, *ss;
};

int onebit_schedule(BaguaSingleCommunicatorC* c, const bagua_tensor_t* t, int average, const Chunking& k, int pieces,
                    const EfState* st) {
    int rc;
    if (c->ensure_side(2 * (size_t)pieces + 3)) return finish(c, BAGUA_ERR_HIP);
    hipStream_t s0 = c->stream, s1 = c->side;
    hipEvent_t* encoded = c->events.data();
    hipEvent_t* gathered = encoded + pieces;
    hipEvent_t exchanged = gathered[pieces], requantised = gathered[pieces + 1];
    std::vector<Piece> tab;
    TRY(onebit_pieces(k, pieces, &tab));
    const int dt = t->dtype, cs = (int)k.cs, p = k.p, n = (int)t->num_elem;
    void* x = (void*)(uintptr_t)t->ptr;
    OpBuffer send(c), recv(c);
    TRY(send.allocate(c->device_id, k.S));
    TRY(recv.allocate(c->device_id, k.S));
    uint8_t* sb = send.as<uint8_t>();
    uint8_t* rb = recv.as<uint8_t>();
    const size_t ws_bytes = bagua_onebit_workspace_bytes(cs, p);
    uint64_t wsp = 0;
    if ((rc = stream_workspace(c->device_id, (uint64_t)(uintptr_t)s0, ws_bytes, &wsp)) != BAGUA_OK)
        return finish(c, rc);
    void* ws = (void*)(uintptr_t)wsp;
    TRY2(fork_side(c, gathered[pieces + 2]));
    // 1. (compensate +) encode piece by piece (bits + partials of every chunk; the carry in
    // place), headers (and the new worker scales) last
    for (int q = 0; q < pieces; ++q) {
        const int tb = tab[q].b, te = tab[q].e;
        if (te > tb)
            TRY2(st ? bagua_onebit_encode_range_ef(dt, x, n, cs, p, sb, k.S, ws, ws_bytes, tb, te, st->wc, st->ws, s0)
                    : bagua_onebit_encode_range(dt, x, n, cs, p, sb, k.S, ws, ws_bytes, tb, te, s0));
        if (q == pieces - 1)
            TRY2(st ? bagua_onebit_finalize_ef(ws, ws_bytes, n, cs, p, sb, k.S, st->ws, s0)
                    : bagua_onebit_finalize(ws, ws_bytes, n, cs, p, sb, k.S, s0));
        HIP2(hipEventRecord(encoded[q], s0));
    }
    for (int q = 0; q < pieces; ++q) {
        HIP2(hipStreamWaitEvent(s1, encoded[q], 0));
        // a group per range: the last piece's payload, then the headers
        for (const ByteRange& r : tab[q].a2a) TRY2(exchange_ranges(c, k, sb, rb, &r, 1, true));
    }
    HIP2(hipEventRecord(exchanged, s1));
    // 2. decode the p received segments of the own chunk, reduce, (compensate with the
    // server state,) re-encode it (the reduced chunk is not stored)
    HIP2(hipStreamWaitEvent(s0, exchanged, 0));
    if (!st) {
        rc = bagua_onebit_reduce_requantize(dt, rb, k.S, cs, p, nullptr, average, sb, k.S, k.rank, ws, ws_bytes, s0);
    } else {
        rc = bagua_onebit_reduce_requantize_ef(dt, rb, k.S, cs, p, average, sb, k.S, k.rank, ws, ws_bytes, st->sc, st->ss,
                                               s0);
        if (rc == BAGUA_ERR_UNSUPPORTED)
            rc = composed_ef_middle(t, BAGUA_COMPRESSION_ONEBIT, k, average, recv, sb, (uint64_t)(uintptr_t)s0,
                                    [&](const void* own, uint8_t* seg, size_t co) {
                                        return bagua_onebit_compress_ef(dt, own, cs, cs, 1, seg, co, ws, ws_bytes, -1,
                                                                        st->sc, st->ss, s0);
                                    });
    }
    TRY2(rc);
    HIP2(hipEventRecord(requantised, s0));
    // 3. allgather (headers with piece 0) + decode piece by piece
    HIP2(hipStreamWaitEvent(s1, requantised, 0));
    for (int q = 0; q < pieces; ++q) {
        TRY2(exchange_ranges(c, k, sb, rb, tab[q].ag, 2, false));
        HIP2(hipEventRecord(gathered[q], s1));
    }
    for (int q = 0; q < pieces; ++q) {
        HIP2(hipStreamWaitEvent(s0, gathered[q], 0));
        if (tab[q].e > tab[q].b) TRY2(bagua_onebit_decompress_range(dt, sb, k.S, cs, p, x, tab[q].b, tab[q].e, s0));
    }
    return finish_both(c, BAGUA_OK);
}

// The plain 1-bit op: pieced where every rank can tell that it fits, else unpieced.  An
// unaligned tensor runs as it is.
int centralized_pipelined_onebit(BaguaSingleCommunicatorC* c, const bagua_tensor_t* t, int average, int pieces) {
    Chunking k;
    if (!valid_schedule(pieces)) return BAGUA_ERR_INVALID_ARG;
    int rc = plan(c, t, BAGUA_COMPRESSION_ONEBIT, &k);
    if (rc) return rc;
    pieces &= BAGUA_PIECES_COUNT_MASK;  // 1-bit pieces are tile ranges: no tapered schedule
    if (pieces < 1) pieces = k.p == 1 ? 1 : auto_pieces(c->cfg, k.cs / 8);  // sign bits per chunk
    if (pieces == 1 || !pipeline_fits(t, k, 0)) return centralized(c, t, average, BAGUA_COMPRESSION_ONEBIT, true);
    DeviceGuard guard(c->device_id);
    if ((rc = check_schedule(c, kOpOneBitPipelined, BAGUA_COMPRESSION_ONEBIT, t, k.cs, pieces, average))) return rc;
    return onebit_schedule(c, t, average, k, pieces, nullptr);
}

// a state tensor: F32, on the op's device, exactly `n` elements, 16-B aligned
int ef_tensor(const bagua_tensor_t* s, uint64_t n, int device, float** out) {
    if (!s || !s->ptr) return BAGUA_ERR_INVALID_ARG;
    if (s->dtype != BAGUA_DTYPE_F32 || s->device_id != device) return BAGUA_ERR_INVALID_ARG;
    if (s->num_elem != n || s->num_elem_allocated != n || s->ptr % 16) return BAGUA_ERR_INVALID_ARG;
    *out = (float*)(uintptr_t)s->ptr;
    return BAGUA_OK;
}

// The 1-bit op with error feedback (validated by its C entry): every piece count -- one
// included, and one rank -- takes the one schedule above.
int centralized_onebit_ef(BaguaSingleCommunicatorC* c, const bagua_tensor_t* t, int average, const EfState& st,
                          int pieces) {
    Chunking k;
    int rc = plan(c, t, BAGUA_COMPRESSION_ONEBIT, &k);
    if (rc) return rc;
    const int caller = pieces;
    pieces &= BAGUA_PIECES_COUNT_MASK;  // 1-bit pieces are tile ranges: no tapered schedule
    if (pieces < 1) pieces = k.p == 1 ? 1 : auto_pieces(c->cfg, k.cs / 8);  // sign bits per chunk
    // (the entry admits fully valid tensors of at most INT_MAX elements only: this is p > 16)
    if (!pipeline_fits(t, k, 0)) pieces = 1;  // the composed middle step reads the whole tensor
    if (t->ptr % 16)
        // the caller's value, not the resolved count: ranks whose alignment differs
        // resolve it from the same input and build the same piece ranges
        return with_aligned_copy(c, {t}, [&](const std::vector<const bagua_tensor_t*>& u) {
            return centralized_onebit_ef(c, u[0], average, st, caller);
        });
    DeviceGuard guard(c->device_id);
    if ((rc = check_schedule(c, kOpOneBitErrorFeedback, BAGUA_COMPRESSION_ONEBIT, t, k.cs, pieces, average))) return rc;
    return onebit_schedule(c, t, average, k, pieces, &st);
}

// The MXFP4 op, pipelined (MXFP4.md, "Pipelined op").  Every 32-element block carries its
// own scale byte, so nothing of a chunk is needed before its first bytes leave and the
// middle step of a piece needs no other piece: piece q is encoded and sent, reduced and
// re-encoded as soon as it has arrived, gathered and decoded, independently of the others.
// No workspace.  A piece is a block range of every chunk (bagua_mxfp4_piece_range), in a
// segment the scale bytes [bb, be) and the payload bytes [sbytes + 16 bb, sbytes + 16 be);
// the last non-empty piece's ranges run to the end of their regions (the slack).
//
//   stream: E0 E1 .. Ek | M0 M1 .. Mk | D0 D1 .. Dk
//   side  :    A0 A1 .. Ak     G0 G1 .. Gk
//   (E encode piece q of all chunks, A its alltoall, M the fused middle step on piece q of
//    the own chunk, G its allgather, D decode piece q of all chunks; M_q waits for A_q
//    only, G_q for M_q, D_q for G_q; the side stream posts A0 .. Ak, then G0 .. Gk)
//
// sr: the same schedule with both encodes stochastic (MXFP4.md, "Stochastic rounding").  A
// word depends on the key and the element's index alone, so every piece count gives the
// unpieced op's bytes.
//
// The schedule serves both block codecs (MXFP8.md, "Pipelined op"): what differs is the three
// range entries, the piece table and the op kind.  sr: kMxfp4 only.
struct MxCodec {
    int method, op_kind;
    decltype(&bagua_mxfp4_compress_range) compress_range;
    decltype(&bagua_mxfp4_reduce_requantize_range) reduce_requantize_range;
    decltype(&bagua_mxfp4_decompress_range) decompress_range;
    decltype(&mxfp4_pieces) pieces;
};
const MxCodec kMxfp4{BAGUA_COMPRESSION_MXFP4,           kOpMxfp4Pipelined,
                     bagua_mxfp4_compress_range,        bagua_mxfp4_reduce_requantize_range,
                     bagua_mxfp4_decompress_range,      mxfp4_pieces};
const MxCodec kMxfp8{BAGUA_COMPRESSION_MXFP8,           kOpMxfp8Pipelined,
                     bagua_mxfp8_compress_range,        bagua_mxfp8_reduce_requantize_range,
                     bagua_mxfp8_decompress_range,      mxfp8_pieces};

int centralized_pipelined_mxfp4(BaguaSingleCommunicatorC* c, const bagua_tensor_t* t, int average, int pieces,
                                const MxSrKeys* sr = nullptr, const MxCodec& mx = kMxfp4) {
    Chunking k;
    if (!valid_schedule(pieces)) return BAGUA_ERR_INVALID_ARG;
    if (sr && mx.method != BAGUA_COMPRESSION_MXFP4) return BAGUA_ERR_UNSUPPORTED;  // the keyed kernels are MXFP4's
    int rc = plan(c, t, mx.method, &k);
    if (rc) return rc;
    const int caller = pieces;
    pieces &= BAGUA_PIECES_COUNT_MASK;
    if (pieces < 1) pieces = k.p == 1 ? 1 : auto_pieces(c->cfg, k.S / k.p);  // segment bytes per chunk
    // unpieced: one rank (no exchange to hide) and the shapes the fused middle step or the
    // vector paths cannot take -- decided from values equal on every rank only
    // (vec = 1: a segment is whole 32-B lines, only the chunk has to be whole 16-B vectors)
    if (pieces == 1 || k.p == 1 || !pipeline_fits(t, k, 1))
        return centralized(c, t, average, mx.method, true, sr);
    if (t->ptr % 16)  // this rank alone: the same schedule on an aligned staging copy
        return with_aligned_copy(c, {t}, [&](const std::vector<const bagua_tensor_t*>& u) {
            return centralized_pipelined_mxfp4(c, u[0], average, caller, sr, mx);
        });
    const int sched = op_schedule(c->cfg, pieces, caller);
    DeviceGuard guard(c->device_id);
    if ((rc = check_schedule(c, sr ? kOpMxfp4StochasticPipelined : mx.op_kind, mx.method, t, k.cs, sched, average)))
        return rc;
    if (c->ensure_side(4 * (size_t)pieces + 1)) return finish(c, BAGUA_ERR_HIP);
    hipStream_t s0 = c->stream;
    hipEvent_t* encoded = c->events.data();
    hipEvent_t* exchanged = encoded + pieces;
    hipEvent_t* requantised = exchanged + pieces;
    hipEvent_t* gathered = requantised + pieces;
    std::vector<Piece> tab;
    TRY(mx.pieces(k, sched, &tab));
    const int dt = t->dtype, cs = (int)k.cs, p = k.p;
    void* x = (void*)(uintptr_t)t->ptr;
    OpBuffer send(c), recv(c);
    TRY(send.allocate(c->device_id, k.S));
    TRY(recv.allocate(c->device_id, k.S));
    uint8_t* sb = send.as<uint8_t>();
    uint8_t* rb = recv.as<uint8_t>();
    TRY2(fork_side(c, gathered[pieces]));
    // 1. encode + alltoall piece by piece (an empty piece launches and moves nothing, its
    // events are recorded all the same)
    for (int q = 0; q < pieces; ++q) {
        if (tab[q].b < tab[q].e)
            TRY2(sr ? bagua_mxfp4_compress_sr_range(dt, x, (int)t->num_elem, cs, p, sb, k.S, tab[q].b, tab[q].e,
                                                    sr->worker, s0)
                    : mx.compress_range(dt, x, (int)t->num_elem, cs, p, sb, k.S, tab[q].b, tab[q].e, s0));
        HIP2(hipEventRecord(encoded[q], s0));
    }
    TRY2(exchange_pieces(c, k, sb, rb, tab, true, encoded, exchanged));
    // 2. the middle step of piece q as soon as it has arrived: decode the p received versions,
    // reduce, re-encode into the own segment (the reduced chunk is not stored)
    for (int q = 0; q < pieces; ++q) {
        HIP2(hipStreamWaitEvent(s0, exchanged[q], 0));
        if (tab[q].b < tab[q].e)
            TRY2(sr ? bagua_mxfp4_reduce_requantize_sr_range(dt, rb, k.S, cs, p, average, sb, k.S, k.rank, tab[q].b,
                                                             tab[q].e, sr->server, s0)
                    : mx.reduce_requantize_range(dt, rb, k.S, cs, p, average, sb, k.S, k.rank, tab[q].b, tab[q].e, s0));
        HIP2(hipEventRecord(requantised[q], s0));
    }
    // 3. allgather + decode piece by piece
    TRY2(exchange_pieces(c, k, sb, rb, tab, false, requantised, gathered));
    for (int q = 0; q < pieces; ++q) {
        HIP2(hipStreamWaitEvent(s0, gathered[q], 0));
        if (tab[q].b < tab[q].e) TRY2(mx.decompress_range(dt, sb, k.S, cs, p, x, tab[q].b, tab[q].e, s0));
    }
    return finish_both(c, BAGUA_OK);
}

// The MXFP4 op with error feedback (MXFP4.md): centralized()'s steps for the MXFP4 codec
// with the two `_ef` kernels.  The worker residual compensates what this rank encodes for
// the alltoall, the server residual the own chunk it re-encodes for the allgather; wire
// format, collectives, segment sizes and the final decode are the plain op's.  One stream,
// no pieces; one rank takes the same path (its own bytes arrive by a device copy).
int centralized_mxfp4_ef(BaguaSingleCommunicatorC* c, const bagua_tensor_t* t, int average, float* worker,
                         float* server) {
    Chunking k;
    int rc = plan(c, t, BAGUA_COMPRESSION_MXFP4, &k);
    if (rc) return rc;
    if (t->ptr % 16)
        return with_aligned_copy(c, {t}, [&](const std::vector<const bagua_tensor_t*>& u) {
            return centralized_mxfp4_ef(c, u[0], average, worker, server);
        });
    DeviceGuard guard(c->device_id);
    if ((rc = check_schedule(c, kOpMxfp4ErrorFeedback, BAGUA_COMPRESSION_MXFP4, t, k.cs, 1, average))) return rc;
    const uint64_t s = (uint64_t)(uintptr_t)c->stream;
    void* sp = (void*)(uintptr_t)s;
    const int dt = t->dtype, cs = (int)k.cs, p = k.p;
    OpBuffer send(c), recv(c);
    TRY(send.allocate(c->device_id, k.S));
    TRY(recv.allocate(c->device_id, k.S));
    const bagua_tensor_t sv = u8_view(send.ptr(), k.S, c->device_id);
    // 1. compensate + encode every chunk (worker residual in place)
    TRY(bagua_mxfp4_compress_ef(dt, (const void*)(uintptr_t)t->ptr, (int)t->num_elem, cs, p, send.as<uint8_t>(), k.S, -1,
                                worker, sp));
    // 2. alltoall: slot j of recv <- rank j's segment `rank`
    TRY(alltoall_or_copy(c, k, send.as<void>(), recv.as<void>()));
    // 3. decode the p received versions of the own chunk, reduce, compensate with the server
    // residual, re-encode into send[rank] (the reduced chunk is not stored)
    rc = bagua_mxfp4_reduce_requantize_ef(dt, recv.as<uint8_t>(), k.S, cs, p, average, send.as<uint8_t>(), k.S, k.rank,
                                          server, sp);
    if (rc == BAGUA_ERR_UNSUPPORTED)
        rc = composed_ef_middle(t, BAGUA_COMPRESSION_MXFP4, k, average, recv, send.as<uint8_t>(), s,
                                [&](const void* own, uint8_t* seg, size_t co) {
                                    return bagua_mxfp4_compress_ef(dt, own, cs, cs, 1, seg, co, -1, server, sp);
                                });
    TRY(rc);
    // 4. allgather the requantised chunks in place, 5. decode everything
    if (p > 1) TRY(bagua_comm_allgather_inplace(c, &sv));
    TRY(bagua_tensor_decompress_from(t, BAGUA_COMPRESSION_MXFP4, p, &sv, s));
    return finish(c, BAGUA_OK);
}

// one group of the ring exchange on the side stream
int ring_exchange_group(BaguaSingleCommunicatorC* c, const RingPlan& P, int g, uint8_t* const bufs[4]) {
    const std::vector<bagua_p2p_op_t> ops = ring_ops(P, g);
    if (ops.empty()) return BAGUA_OK;
    hipStream_t s1 = c->side;
    if (P.p == 1) {
        // one rank is its own left and right peer: every receive is a device copy of the
        // send with the same key (no RCCL self send/recv)
        for (const bagua_p2p_op_t& o : ops) {
            if (o.is_send) continue;
            for (const bagua_p2p_op_t& src : ops)
                if (src.is_send && src.key == o.key && src.bytes == o.bytes) {
                    if (hipMemcpyAsync(bufs[o.buffer] + o.offset, bufs[src.buffer] + src.offset, o.bytes,
                                       hipMemcpyDeviceToDevice, s1) != hipSuccess)
                        return BAGUA_ERR_HIP;
                    break;
                }
        }
        return BAGUA_OK;
    }
    int rc = c->t->group_start();
    for (const bagua_p2p_op_t& o : ops) {
        if (rc) break;
        uint8_t* ptr = bufs[o.buffer] + o.offset;
        rc = o.is_send ? c->t->send(ptr, o.bytes, BAGUA_DTYPE_U8, o.peer, s1)
                       : c->t->recv(ptr, o.bytes, BAGUA_DTYPE_U8, o.peer, s1);
    }
    const int rc_end = c->t->group_end();
    return rc ? rc : rc_end;
}

// Opt-in (BAGUA_PIECES_MULTIPATH in the op's `pieces`, or BAGUA_RING_MULTIPATH=1 read
// once at the communicator's creation): the only timing so far is RCCL's socket
// transport between processes on one GPU, where multipath was 5.3x slower than
// the direct exchange (profiles/r02_b_ar8_shared_gpu_rccl_socket.json); until an
// xGMI node shows it faster, the default is the reference's direct exchange
// (decentralized_low_precision_synchronous.rs:98-115).
bool ring_multipath_enabled(const BaguaSingleCommunicatorC* c) {
    return (int)c->nranks >= kRingMinMultipath && c->cfg.multipath;
}

}  // namespace

extern "C" {

int bagua_centralized_low_precision_pipelined(BaguaSingleCommunicatorC* c, const bagua_tensor_t* t, int average,
                                              int method, int pieces) {
    if (method == BAGUA_COMPRESSION_ONEBIT) return centralized_pipelined_onebit(c, t, average, pieces);
    if (method == BAGUA_COMPRESSION_MXFP4) return centralized_pipelined_mxfp4(c, t, average, pieces);
    if (method == BAGUA_COMPRESSION_MXFP8) return centralized_pipelined_mxfp4(c, t, average, pieces, nullptr, kMxfp8);
    if (method != BAGUA_COMPRESSION_MINMAX_UINT8) return centralized(c, t, average, method, true);
    return centralized_pipelined(c, t, average, pieces);
}

int bagua_centralized_onebit_error_feedback(BaguaSingleCommunicatorC* c, const bagua_tensor_t* t, int average,
                                            const bagua_tensor_t* worker_carry, const bagua_tensor_t* worker_scales,
                                            const bagua_tensor_t* server_carry, const bagua_tensor_t* server_scale,
                                            int pieces) {
    // every refusal before anything is launched or posted
    if (!c || !c->t || !t || !t->ptr) return BAGUA_ERR_INVALID_ARG;
    if (!valid_schedule(pieces)) return BAGUA_ERR_INVALID_ARG;
    if (!is_float_dtype(t->dtype)) return BAGUA_ERR_UNSUPPORTED;
    if (t->num_elem != t->num_elem_allocated) return BAGUA_ERR_UNSUPPORTED;  // partly valid tensors: the plain op only
    const uint64_t p = c->nranks;
    if (!t->num_elem || t->num_elem % p || t->num_elem > 0x7fffffffULL || t->device_id != (int)c->device_id)
        return BAGUA_ERR_INVALID_ARG;
    const uint64_t cs = t->num_elem / p;
    EfState st{};
    int rc;
    if ((rc = ef_tensor(worker_carry, t->num_elem, t->device_id, &st.wc)) ||
        (rc = ef_tensor(worker_scales, p, t->device_id, &st.ws)) ||
        (rc = ef_tensor(server_carry, cs, t->device_id, &st.sc)) ||
        (rc = ef_tensor(server_scale, 1, t->device_id, &st.ss)))
        return rc;
    return centralized_onebit_ef(c, t, average, st, pieces);
}

int bagua_centralized_mxfp4_error_feedback(BaguaSingleCommunicatorC* c, const bagua_tensor_t* t, int average,
                                           const bagua_tensor_t* worker_residual,
                                           const bagua_tensor_t* server_residual) {
    // every refusal before anything is launched or posted
    if (!c || !c->t || !t || !t->ptr) return BAGUA_ERR_INVALID_ARG;
    if (!is_float_dtype(t->dtype)) return BAGUA_ERR_UNSUPPORTED;
    if (t->num_elem != t->num_elem_allocated) return BAGUA_ERR_UNSUPPORTED;  // partly valid tensors: the plain op only
    const uint64_t p = c->nranks;
    if (!t->num_elem || t->num_elem % p || t->num_elem > 0x7fffffffULL || t->device_id != (int)c->device_id)
        return BAGUA_ERR_INVALID_ARG;
    float *worker = nullptr, *server = nullptr;
    int rc;
    if ((rc = ef_tensor(worker_residual, t->num_elem, t->device_id, &worker)) ||
        (rc = ef_tensor(server_residual, t->num_elem / p, t->device_id, &server)))
        return rc;
    return centralized_mxfp4_ef(c, t, average, worker, server);
}

int bagua_centralized_mxfp4_stochastic(BaguaSingleCommunicatorC* c, const bagua_tensor_t* t, int average,
                                       uint64_t seed, uint64_t step, int pieces) {
    // every refusal before anything is launched or posted
    if (!c || !c->t || !t || !t->ptr) return BAGUA_ERR_INVALID_ARG;
    if (!valid_schedule(pieces)) return BAGUA_ERR_INVALID_ARG;
    if (!is_float_dtype(t->dtype)) return BAGUA_ERR_UNSUPPORTED;
    // the keys are this rank's alone: no byte count and no collective depends on them
    const MxSrKeys sr{bagua_mxfp4_sr_key(seed, step, (int)c->rank, 0), bagua_mxfp4_sr_key(seed, step, (int)c->rank, 1)};
    return centralized_pipelined_mxfp4(c, t, average, pieces, &sr);
}

int bagua_centralized_low_precision_synchronous(BaguaSingleCommunicatorC* c, const bagua_tensor_t* t, int average,
                                                int method) {
    return bagua_centralized_low_precision_pipelined(c, t, average, method, 0);
}

int bagua_centralized_low_precision_synchronous_unfused(BaguaSingleCommunicatorC* c, const bagua_tensor_t* t,
                                                        int average, int method) {
    return centralized(c, t, average, method, false);
}

int bagua_centralized_full_precision_synchronous(BaguaSingleCommunicatorC* c, const bagua_tensor_t* t, int average) {
    // centralized_full_precision_synchronous.rs:44-50 (non-scattergather branch)
    if (!c) return BAGUA_ERR_INVALID_ARG;
    int rc = bagua_comm_allreduce_inplace(c, t, average ? BAGUA_OP_AVG : BAGUA_OP_SUM);
    return finish(c, rc);
}


static int decentralized(BaguaSingleCommunicatorC* c, const bagua_tensor_t* t, const bagua_tensor_t* weight,
                         const bagua_tensor_t* left, const bagua_tensor_t* right, int method, bool allow_fused,
                         int pieces = 1) {
    if (!c || !c->t || !t || !weight || !left || !right || !valid_schedule(pieces)) return BAGUA_ERR_INVALID_ARG;
    if (c->aborted.load()) return BAGUA_ERR_ABORTED;
    DeviceGuard guard(c->device_id);
    const uint64_t s = (uint64_t)(uintptr_t)c->stream;
    void* sp = (void*)(uintptr_t)s;
    int rc;
    if (t->num_elem_allocated > 0x7fffffffULL) return BAGUA_ERR_INVALID_ARG;
    const int n = (int)t->num_elem_allocated;
    const size_t S = bagua_compressed_size(method, t->dtype, 1, t->num_elem_allocated);
    if (!S) return BAGUA_ERR_UNSUPPORTED;
    // fused kernels (csrc/kernels/decentralized.hip, mxfp4_ring.hip) for fully valid,
    // same-shape MinMax and MXFP4 buckets; anything else runs the reference's op sequence.
    // The choice (and with it the pipelined exchange schedule) depends only on values equal
    // on every rank; a rank whose tensors are not 16-B aligned runs on aligned copies.
    // BAGUA_MXFP4_RING_FUSED=0 (read per call, A/B): the op sequence for MXFP4.  It changes
    // no byte on the wire and MXFP4 is never pipelined, so ranks need not agree on it.
    const bool mx = method == BAGUA_COMPRESSION_MXFP4 && env_int("BAGUA_MXFP4_RING_FUSED", 1) != 0;
    bool fused = allow_fused && (method == BAGUA_COMPRESSION_MINMAX_UINT8 || mx) &&
                 t->num_elem == t->num_elem_allocated;
    for (const bagua_tensor_t* o : {weight, left, right})
        fused = fused && o->dtype == t->dtype && o->num_elem == t->num_elem;
    if (fused && (t->ptr % 16 || weight->ptr % 16 || left->ptr % 16 || right->ptr % 16))
        return with_aligned_copy(c, {t, weight, left, right}, [&](const std::vector<const bagua_tensor_t*>& u) {
            return decentralized(c, u[0], u[1], u[2], u[3], method, allow_fused, pieces);
        });
    // the exchange schedule, from values equal on every rank (ScheduleConfig included)
    const int caller = pieces;
    pieces &= BAGUA_PIECES_COUNT_MASK;
    if (pieces < 1) pieces = c->nranks == 1 ? 1 : auto_pieces(c->cfg, (size_t)n);
    const int sched = op_schedule(c->cfg, pieces, caller);
    const bool multipath =
        (caller & BAGUA_PIECES_MULTIPATH) ? (int)c->nranks >= kRingMinMultipath : ring_multipath_enabled(c);
    // (MXFP4 stays unpieced: one mix, one exchange, one apply, whatever the schedule asks for)
    const bool pipelined = fused && !mx && (pieces > 1 || multipath);
    if ((rc = check_schedule(c, pipelined ? kOpRingPipelined : (allow_fused ? kOpRing : kOpRingUnfused), method, t,
                             (uint64_t)n, pipelined ? sched | (multipath ? BAGUA_PIECES_MULTIPATH : 0) : 1, 1)))
        return rc;
    if (mx && fused && c->nranks == 1 && env_int("BAGUA_ONE_RANK_FUSED", 1) != 0) {
        // one rank: one pass over the four tensors, no payload (bagua_ring_one_rank_mxfp4)
        rc = bagua_ring_one_rank_mxfp4(t->dtype, (void*)(uintptr_t)t->ptr, (void*)(uintptr_t)weight->ptr,
                                       (void*)(uintptr_t)left->ptr, (void*)(uintptr_t)right->ptr, n, sp);
        if (rc != BAGUA_ERR_UNSUPPORTED) return finish(c, rc);
    }
    if (fused && !mx && !pipelined && c->nranks == 1 && env_int("BAGUA_ONE_RANK_FUSED", 1) != 0) {
        // one rank: both peers' payloads are its own bytes, so the op is the mix pass and
        // one pass applying d = dq(q(mixed)) to all four tensors, no payload written
        // (bagua_ring_one_rank_minmax); BAGUA_ONE_RANK_FUSED=0: the steps below (A/B)
        const size_t wsb = bagua_minmax_u8_workspace_bytes(n, 1);
        uint64_t wsp = 0;
        if ((rc = stream_workspace(c->device_id, s, wsb, &wsp)) != BAGUA_OK) return finish(c, rc);
        rc = bagua_ring_one_rank_minmax(t->dtype, (void*)(uintptr_t)t->ptr, (void*)(uintptr_t)weight->ptr,
                                        (void*)(uintptr_t)left->ptr, (void*)(uintptr_t)right->ptr, n,
                                        (void*)(uintptr_t)wsp, wsb, sp);
        if (rc != BAGUA_ERR_UNSUPPORTED) return finish(c, rc);
    }
    OpBuffer mine(c), lbuf(c), rbuf(c);
    TRY(mine.allocate(c->device_id, S));
    TRY(lbuf.allocate(c->device_id, S));
    TRY(rbuf.allocate(c->device_id, S));
    const bagua_tensor_t mv = u8_view(mine.ptr(), S, c->device_id);
    const bagua_tensor_t lv = u8_view(lbuf.ptr(), S, c->device_id);
    const bagua_tensor_t rv = u8_view(rbuf.ptr(), S, c->device_id);
    void* tp = (void*)(uintptr_t)t->ptr;
    void* wp = (void*)(uintptr_t)weight->ptr;
    void* lp = (void*)(uintptr_t)left->ptr;
    void* rp = (void*)(uintptr_t)right->ptr;
    bool mixed = false;
    if (fused && mx) {
        // :45-64 in one pass: the segment of the mixed t, which itself is never stored (every
        // path below overwrites t before anything reads it)
        rc = bagua_ring_mix_mxfp4(t->dtype, tp, lp, rp, wp, n, mine.as<uint8_t>(), S, sp);
        if (rc == BAGUA_OK) mixed = true;
        else if (rc != BAGUA_ERR_UNSUPPORTED) return finish(c, rc);
    } else if (fused) {
        // :45-64 t += L/3 + R/3 - 5W/3 (three rounded steps) with the min/max partials, then quantise
        const size_t wsb = bagua_minmax_u8_workspace_bytes(n, 1);
        uint64_t wsp = 0;
        if ((rc = stream_workspace(c->device_id, s, wsb, &wsp)) != BAGUA_OK) return finish(c, rc);
        void* ws = (void*)(uintptr_t)wsp;
        rc = bagua_ring_mix_minmax(t->dtype, tp, lp, rp, wp, n, ws, wsb, sp);
        if (rc == BAGUA_OK) {
            if (pipelined) {
                // pipelined: quantise piece q -> exchange piece q (side stream) -> apply piece q;
                // one header for the whole bucket, travelling with piece 0.  Multipath: the
                // relayed slices of piece q arrive with group q + 1.
                RingPlan plan;
                TRY(ring_plan((int)c->nranks, (int)c->rank, n, sched, multipath, &plan));
                if (plan.k.S != S) return finish(c, BAGUA_ERR_INVALID_ARG);
                OpBuffer relay(c);
                if (ring_relay_bytes(plan)) TRY(relay.allocate(c->device_id, ring_relay_bytes(plan)));
                if (c->ensure_side(2 * (size_t)pieces + 1)) return finish(c, BAGUA_ERR_HIP);
                hipStream_t s1 = c->side;
                hipEvent_t* quantised = c->events.data();
                hipEvent_t* exchanged = quantised + pieces;
                uint8_t* mb = mine.as<uint8_t>();
                uint8_t* lb = lbuf.as<uint8_t>();
                uint8_t* rb = rbuf.as<uint8_t>();
                uint8_t* const bufs[4] = {mb, lb, rb, relay.as<uint8_t>()};
                TRY2(fork_side(c, exchanged[pieces]));
                for (int q = 0; q < pieces; ++q) {
                    const int b = plan.tab[q].b, e = plan.tab[q].e;
                    if (q == 0 || b < e)
                        TRY2(bagua_minmax_u8_quantize_range(t->dtype, tp, n, n, 1, mb, S, ws, wsb, -1, b, e, sp));
                    HIP2(hipEventRecord(quantised[q], c->stream));
                }
                for (int g = 0; g < plan.groups; ++g) {
                    if (g < pieces) HIP2(hipStreamWaitEvent(s1, quantised[g], 0));
                    TRY2(ring_exchange_group(c, plan, g, bufs));
                    const int done = plan.mp ? g - 1 : g;  // the piece this group completes
                    if (done >= 0) HIP2(hipEventRecord(exchanged[done], s1));
                }
                for (int q = 0; q < pieces; ++q) {
                    const int b = plan.tab[q].b, e = plan.tab[q].e;
                    HIP2(hipStreamWaitEvent(c->stream, exchanged[q], 0));
                    if (b < e)
                        TRY2(bagua_ring_apply_minmax_range(t->dtype, mb, lb, rb, S, n, b, e, tp, wp, lp, rp, sp));
                }
                return finish_both(c, BAGUA_OK);
            }
            TRY(bagua_minmax_u8_compress_stage(2, t->dtype, tp, n, n, 1, mine.as<uint8_t>(), S, ws, wsb, -1, sp));
            mixed = true;
        } else if (rc != BAGUA_ERR_UNSUPPORTED) {
            return finish(c, rc);
        }
    }
    if (!mixed) {
        // :45-60: t += L/3; t += R/3; t += W*(-5/3)  (f64 literals cast to f32)
        TRY(bagua_tensor_addmul_inplace(t, left, (float)(1.0 / 3.0), s));
        TRY(bagua_tensor_addmul_inplace(t, right, (float)(1.0 / 3.0), s));
        TRY(bagua_tensor_addmul_inplace(t, weight, (float)(-5.0 / 3.0), s));
        // :61-64 whole-bucket compress (n_chunks = 1)
        TRY(bagua_tensor_compress_into(t, method, 1, s, -1, &mv));
    }
    // :98-115 ring exchange inside one group.  One rank is its own left and right
    // peer: what it would receive are its own bytes, so the op reads `mine` in their
    // place (RCCL's self send/recv of 2 x S bytes took 206 us for 2^27 bf16).
    const int p = (int)c->nranks, r = (int)c->rank;
    const int lpeer = (r + p - 1) % p, rpeer = (r + 1) % p;
    if (p > 1) {
        TRY(c->t->group_start());
        rc = bagua_comm_send(c, &mv, lpeer);
        if (!rc) rc = bagua_comm_send(c, &mv, rpeer);
        if (!rc) rc = bagua_comm_recv(c, &lv, lpeer);
        if (!rc) rc = bagua_comm_recv(c, &rv, rpeer);
        const int rc_end = c->t->group_end();
        if (rc || rc_end) return finish(c, rc ? rc : rc_end);
    }
    const bagua_tensor_t* from_l = p > 1 ? &lv : &mv;
    const bagua_tensor_t* from_r = p > 1 ? &rv : &mv;
    // :126-151
    if (fused) {
        rc = (mx ? bagua_ring_apply_mxfp4 : bagua_ring_apply_minmax)(
            t->dtype, mine.as<uint8_t>(), (const uint8_t*)(uintptr_t)from_l->ptr,
            (const uint8_t*)(uintptr_t)from_r->ptr, S, n, tp, wp, lp, rp, sp);
        if (rc == BAGUA_OK) return finish(c, BAGUA_OK);
        if (rc != BAGUA_ERR_UNSUPPORTED) return finish(c, rc);
    }
    TRY(bagua_tensor_decompress_from(t, method, 1, from_l, s));
    TRY(bagua_tensor_add_inplace(left, t, s));
    TRY(bagua_tensor_decompress_from(t, method, 1, from_r, s));
    TRY(bagua_tensor_add_inplace(right, t, s));
    TRY(bagua_tensor_decompress_from(t, method, 1, &mv, s));
    TRY(bagua_tensor_add_inplace(t, weight, s));
    TRY(bagua_tensor_clone_from(weight, t, s));
    return finish(c, BAGUA_OK);
}

int bagua_comm_set_async(BaguaSingleCommunicatorC* c, int on) {
    if (!c) return BAGUA_ERR_INVALID_ARG;
    c->async = on != 0;
    return BAGUA_OK;
}

int bagua_decentralized_low_precision_synchronous(BaguaSingleCommunicatorC* c, const bagua_tensor_t* t,
                                                  const bagua_tensor_t* weight, const bagua_tensor_t* left,
                                                  const bagua_tensor_t* right, int method) {
    return decentralized(c, t, weight, left, right, method, true, 0);
}

}  // extern "C"

// communicators/mod.rs:390-427, execute_communication with a hierarchical
// communicator (:243-336): every rank of the node reduces (AVG or SUM) into the
// node leader (intranode rank 0, :264-283 / :312-325), the leader runs the op among
// the leaders on the internode communicator, and the leader broadcasts the result
// over the node (:286-294 / :327-330).  The leader's two communicators share one
// stream and device (:250-256, :356-360).
template <typename F>
static int hierarchical(BaguaSingleCommunicatorC* intra, BaguaSingleCommunicatorC* inter, const bagua_tensor_t* t,
                        bool intranode_average, F&& op) {
    if (!intra || !intra->t || !t) return BAGUA_ERR_INVALID_ARG;
    if (intra->aborted.load()) return BAGUA_ERR_ABORTED;
    const bool leader = intra->rank == 0;
    if (leader && (!inter || inter->stream != intra->stream || inter->device_id != intra->device_id))
        return BAGUA_ERR_INVALID_ARG;
    DeviceGuard guard(intra->device_id);
    int rc = bagua_comm_reduce_inplace(intra, t, 0, intranode_average ? BAGUA_OP_AVG : BAGUA_OP_SUM);
    if (!rc && leader) rc = op(inter);
    if (!rc) rc = bagua_comm_broadcast(intra, t, 0);
    return finish(intra, rc);
}

extern "C" {

int bagua_centralized_low_precision_hierarchical(BaguaSingleCommunicatorC* intranode,
                                                 BaguaSingleCommunicatorC* internode, const bagua_tensor_t* t,
                                                 int average, int method) {
    // centralized_low_precision_synchronous.rs:25-30: intranode average = the op's average
    return hierarchical(intranode, internode, t, average != 0, [&](BaguaSingleCommunicatorC* c) {
        return bagua_centralized_low_precision_synchronous(c, t, average, method);
    });
}

int bagua_centralized_full_precision_hierarchical(BaguaSingleCommunicatorC* intranode,
                                                  BaguaSingleCommunicatorC* internode, const bagua_tensor_t* t,
                                                  int average) {
    return hierarchical(intranode, internode, t, average != 0, [&](BaguaSingleCommunicatorC* c) {
        return bagua_centralized_full_precision_synchronous(c, t, average);
    });
}

int bagua_decentralized_low_precision_hierarchical(BaguaSingleCommunicatorC* intranode,
                                                   BaguaSingleCommunicatorC* internode, const bagua_tensor_t* t,
                                                   const bagua_tensor_t* weight, const bagua_tensor_t* left,
                                                   const bagua_tensor_t* right, int method) {
    // decentralized_low_precision_synchronous.rs:37-41: the node always averages
    return hierarchical(intranode, internode, t, true, [&](BaguaSingleCommunicatorC* c) {
        return bagua_decentralized_low_precision_synchronous(c, t, weight, left, right, method);
    });
}

int bagua_decentralized_low_precision_pipelined(BaguaSingleCommunicatorC* c, const bagua_tensor_t* t,
                                                const bagua_tensor_t* weight, const bagua_tensor_t* left,
                                                const bagua_tensor_t* right, int method, int pieces) {
    return decentralized(c, t, weight, left, right, method, true, pieces);
}

int bagua_decentralized_low_precision_synchronous_unfused(BaguaSingleCommunicatorC* c, const bagua_tensor_t* t,
                                                          const bagua_tensor_t* weight, const bagua_tensor_t* left,
                                                          const bagua_tensor_t* right, int method) {
    return decentralized(c, t, weight, left, right, method, false);
}

}  // extern "C"
