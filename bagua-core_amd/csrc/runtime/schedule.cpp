// schedule.cpp — piece counts, piece tables and the ring exchange schedule (schedule.hpp):
// host arithmetic on values equal on every rank, no HIP or transport call.
#include "schedule.hpp"

#include "comm_internal.hpp"

#include <algorithm>

namespace bagua {

int auto_pieces(const ScheduleConfig& cfg, size_t payload_bytes) {
    // BAGUA_PIPELINE_PIECES caps the count (1 disables), pieces keep at least
    // BAGUA_PIPELINE_MIN_PIECE payload bytes per chunk (= elements for MinMax
    // u8; the exchange of a piece is p times that); both read once, at the
    // communicator's creation (ScheduleConfig)
    const int kmax = cfg.pieces_cap;
    const int min_piece = cfg.min_piece;
    size_t k = payload_bytes / (size_t)(min_piece > 0 ? min_piece : 1);
    if (k > (size_t)kmax) k = (size_t)kmax;
    return k < 1 ? 1 : (int)k;
}

// The op's piece schedule (bagua_kernels.h: a count, optionally OR-ed with
// BAGUA_PIECES_TAPERED): the caller's, tapered from 3 pieces when the communicator's
// ScheduleConfig (equal on every rank) says so -- by default the schedules the op
// chose itself (the caller passed 0 pieces), since round 6: at the same count the
// first piece (quantised before any byte is on the wire) and the last one (reduced and
// dequantised after the wire) are half size, so the unhidden codec shrinks with the same
// number of exchange groups (1 GiB fp32, 4 pieces, one GPU's kernels: prefix 208 -> 183,
// suffix 56 -> 38 us, profiles/r06_pipe_probe_t4.json).  BAGUA_PIPELINE_TAPER=0 keeps
// every automatic schedule uniform, =1 tapers explicit counts too.  Fixed once per op
// and passed to every building block, so all of one op's ranges agree.
int op_schedule(const ScheduleConfig& cfg, int count, int caller) {
    int sched = count | (caller & BAGUA_PIECES_TAPERED);
    const bool automatic = (caller & BAGUA_PIECES_COUNT_MASK) == 0;
    const bool taper = cfg.taper > 0 || (cfg.taper < 0 && automatic);
    if (count >= 3 && !(sched & BAGUA_PIECES_TAPERED) && taper) sched |= BAGUA_PIECES_TAPERED;
    return sched;
}

bool valid_schedule(int pieces) {
    return (pieces & ~(BAGUA_PIECES_COUNT_MASK | BAGUA_PIECES_TAPERED | BAGUA_PIECES_MULTIPATH)) == 0;
}

// ---- piece tables ------------------------------------------------------------
// A segment keeps one header per chunk and the pieces are disjoint byte ranges of it, so
// every buffer holds exactly the bytes of the unpieced op.  The slack (the bytes of a
// segment past its last unit) travels with the piece whose unit range ends the chunk.
namespace {

template <typename Range, typename Bytes>
int fill_pieces(const Chunking& k, int sched, std::vector<Piece>* v, Range&& range, Bytes&& bytes) {
    const int n = sched & BAGUA_PIECES_COUNT_MASK;
    if (k.cs > 0x7fffffffULL || k.p < 1) return BAGUA_ERR_INVALID_ARG;
    v->assign((size_t)(n > 0 ? n : 0), Piece{});
    for (int q = 0; q < n; ++q) {
        Piece& pc = (*v)[(size_t)q];
        const int rc = range((int)k.cs, sched, q, &pc.b, &pc.e);
        if (rc) return rc;
        bytes(q, n, pc);
    }
    return n > 0 ? BAGUA_OK : BAGUA_ERR_INVALID_ARG;
}

}  // namespace

// MinMax (32-B header, one byte per element): both phases move [0, 32 + e) with piece 0
// (the header travels with it) and [32 + b, 32 + e) with a later piece; an empty later
// piece moves nothing
int minmax_pieces(const Chunking& k, int sched, std::vector<Piece>* v) {
    const size_t co = k.S / k.p;
    return fill_pieces(k, sched, v, bagua_minmax_u8_piece_range, [&](int q, int, Piece& pc) {
        if (q > 0 && pc.b == pc.e) return;
        pc.a2a[0] = ByteRange{q == 0 ? 0 : 32 + (size_t)pc.b, (size_t)pc.e == k.cs ? co : 32 + (size_t)pc.e};
        pc.ag[0] = pc.a2a[0];
    });
}

// 1-bit (32-B header, 128 B of sign bits per 1024-element tile): the payload of tiles
// [b, e) is [32 + 128 b, 32 + 128 e).  A header (scale) needs the whole chunk's |x|
// partials, so the alltoall moves it last, as a second range of the last piece -- a group
// of its own after that piece's payload, also when the payload is empty; the allgather
// moves it first, inside piece 0's range.  No tapered schedule: pieces are tile ranges.
int onebit_pieces(const Chunking& k, int sched, std::vector<Piece>* v) {
    const size_t co = k.S / k.p;
    const int tiles = (int)((k.cs + 1023) / 1024);
    return fill_pieces(k, sched & BAGUA_PIECES_COUNT_MASK, v, bagua_onebit_piece_range, [&](int q, int n, Piece& pc) {
        const size_t hi = pc.e >= tiles ? co : 32 + (size_t)pc.e * 128;
        if (pc.b < pc.e) pc.a2a[0] = ByteRange{32 + (size_t)pc.b * 128, hi};
        if (q == n - 1) pc.a2a[1] = ByteRange{0, 32};
        pc.ag[0] = q == 0 ? ByteRange{0, hi} : pc.a2a[0];
    });
}

// MXFP4 (MXFP4.md: align32(nb) scale bytes, then 16 payload bytes per 32-element block):
// blocks [b, e) are the scale bytes [b, e) and the payload bytes [sbytes + 16 b, sbytes +
// 16 e) in both phases; the ranges of the piece that ends the chunk run to the end of
// their regions
namespace {
template <typename Range>
int mx_block_pieces(const Chunking& k, int sched, std::vector<Piece>* v, Range&& range, size_t block_bytes) {
    const size_t nb = (k.cs + 31) / 32, sbytes = (nb + 31) / 32 * 32, co = k.S / k.p;
    return fill_pieces(k, sched, v, range, [&](int, int, Piece& pc) {
        if (pc.b >= pc.e) return;
        const bool last = (size_t)pc.e == nb;
        pc.a2a[0] = pc.ag[0] = ByteRange{(size_t)pc.b, last ? sbytes : (size_t)pc.e};
        pc.a2a[1] = pc.ag[1] =
            ByteRange{sbytes + block_bytes * (size_t)pc.b, last ? co : sbytes + block_bytes * (size_t)pc.e};
    });
}
}  // namespace

int mxfp4_pieces(const Chunking& k, int sched, std::vector<Piece>* v) {
    return mx_block_pieces(k, sched, v, bagua_mxfp4_piece_range, 16);
}

// MXFP8 (MXFP8.md): the same with 32 payload bytes per block, [sbytes + 32 b, sbytes + 32 e)
int mxfp8_pieces(const Chunking& k, int sched, std::vector<Piece>* v) {
    return mx_block_pieces(k, sched, v, bagua_mxfp8_piece_range, 32);
}

// ---- ring exchange schedule ------------------------------------------------
// The reference sends the whole compressed bucket straight to both ring peers
// (decentralized_low_precision_synchronous.rs:98-115).  On a fully connected
// xGMI node that loads 2 of each GPU's 7 links and leaves 5 idle.  From 6
// ranks on, each piece's bytes are cut into p slices: slices 0..2 go straight
// to the peer, slice k >= 3 is sent to relay rank r + (k-1) (for the right
// peer; r - (k-1) for the left one), which forwards it in the next group.
// Per directed link offset o the load is then (a = 3/p direct, b = 1/p per
// relay): o = +-1: a + b; o = +-2: 3b; others 4b, i.e. at most 4/p of the
// payload per link (8 ranks: 1/2) instead of all of it.  The schedule is
// deterministic and symmetric, and every transfer carries a key (hop, flow,
// slice) so that both ends post the transfers between two ranks in the same
// order (NCCL matches grouped p2p in posting order per pair).
namespace {

// p + 1 slice boundaries of bytes [lo, hi), inner ones on 64-B lines
void ring_slices(ByteRange r, int p, size_t* b) {
    const size_t lo = r.lo, hi = r.hi, len = hi - lo;
    b[0] = lo;
    b[p] = hi;
    for (int i = 1; i < p; ++i) {
        size_t x = (lo + len * (size_t)i / (size_t)p) & ~(size_t)63;
        if (x < b[i - 1]) x = b[i - 1];
        b[i] = x < hi ? x : hi;
    }
}

}  // namespace

int ring_plan(int nranks, int rank, int chunk_size, int pieces, bool multipath, RingPlan* P) {
    if (nranks < 1 || nranks > 64 || rank < 0 || rank >= nranks || chunk_size < 0 || !valid_schedule(pieces) ||
        (pieces & BAGUA_PIECES_COUNT_MASK) < 1)
        return BAGUA_ERR_INVALID_ARG;
    P->p = nranks;
    P->r = rank;
    P->sched = pieces;
    pieces &= BAGUA_PIECES_COUNT_MASK;
    P->pieces = pieces;
    P->mp = multipath && nranks >= kRingMinMultipath;
    P->groups = pieces + (P->mp ? 1 : 0);
    P->k.p = 1;
    P->k.cs = (size_t)chunk_size;
    P->k.S = bagua_minmax_u8_compressed_bytes(BAGUA_DTYPE_F32, chunk_size, 1);  // align32(n) + 32 for every dtype
    // one header for the whole bucket, travelling with piece 0: the MinMax table of one chunk
    const int rc = minmax_pieces(P->k, P->sched, &P->tab);
    if (rc) return rc;
    P->slot = 0;
    if (P->mp) {
        size_t b[65];
        for (const Piece& pc : P->tab) {
            if (pc.a2a[0].hi <= pc.a2a[0].lo) continue;
            ring_slices(pc.a2a[0], nranks, b);
            for (int i = 3; i < nranks; ++i)
                if (b[i + 1] - b[i] > P->slot) P->slot = b[i + 1] - b[i];
        }
        P->slot = (P->slot + 63) & ~(size_t)63;
    }
    return BAGUA_OK;
}

size_t ring_relay_bytes(const RingPlan& P) { return P.mp ? 4 * (size_t)(P.p - 3) * P.slot : 0; }

// transfers of group g: the direct slices and first hops of piece g (g < pieces),
// the relays' second hops of piece g - 1 (multipath, g > 0)
std::vector<bagua_p2p_op_t> ring_ops(const RingPlan& P, int g) {
    std::vector<bagua_p2p_op_t> v;
    const int p = P.p, r = P.r;
    auto rk = [&](int x) { return ((x % p) + p) % p; };
    auto key = [](int hop, int flow, int slice) { return hop * 4096 + flow * 2048 + slice; };
    auto add = [&](int peer, int send, int buf, int k, size_t off, size_t len) {
        if (len) v.push_back(bagua_p2p_op_t{peer, send, buf, k, (uint64_t)off, (uint64_t)len});
    };
    auto relay_off = [&](int q, int flow, int slice) {
        return ((size_t)((q & 1) * 2 + flow) * (size_t)(p - 3) + (size_t)(slice - 3)) * P.slot;
    };
    const int left = rk(r - 1), right = rk(r + 1);
    size_t b[65];
    if (g < P.pieces) {
        const ByteRange pr = P.tab[(size_t)g].a2a[0];
        const size_t lo = pr.lo, hi = pr.hi;
        if (hi > lo) {
            const size_t dhi = P.mp ? (ring_slices(pr, p, b), b[3]) : hi;
            // flow 0: towards the right peer (lands in its left buffer); flow 1: towards the left peer
            add(right, 1, kBufMine, key(0, 0, 0), lo, dhi - lo);
            add(left, 1, kBufMine, key(0, 1, 0), lo, dhi - lo);
            add(left, 0, kBufLeft, key(0, 0, 0), lo, dhi - lo);
            add(right, 0, kBufRight, key(0, 1, 0), lo, dhi - lo);
            if (P.mp)
                for (int i = 3; i < p; ++i) {
                    const int d = i - 1;
                    const size_t len = b[i + 1] - b[i];
                    add(rk(r + d), 1, kBufMine, key(1, 0, i), b[i], len);
                    add(rk(r - d), 1, kBufMine, key(1, 1, i), b[i], len);
                    add(rk(r - d), 0, kBufRelay, key(1, 0, i), relay_off(g, 0, i), len);  // source r-d's slice
                    add(rk(r + d), 0, kBufRelay, key(1, 1, i), relay_off(g, 1, i), len);  // source r+d's slice
                }
        }
    }
    if (P.mp && g > 0) {
        const int q = g - 1;
        const ByteRange pr = P.tab[(size_t)q].a2a[0];
        if (pr.hi > pr.lo) {
            ring_slices(pr, p, b);
            for (int i = 3; i < p; ++i) {
                const int d = i - 1;
                const size_t len = b[i + 1] - b[i];
                add(rk(r - d + 1), 1, kBufRelay, key(2, 0, i), relay_off(q, 0, i), len);  // source r-d -> its right
                add(rk(r + d - 1), 1, kBufRelay, key(2, 1, i), relay_off(q, 1, i), len);  // source r+d -> its left
                add(rk(r + d - 1), 0, kBufLeft, key(2, 0, i), b[i], len);    // left peer's slice via (r-1)+d
                add(rk(r - d + 1), 0, kBufRight, key(2, 1, i), b[i], len);   // right peer's slice via (r+1)-d
            }
        }
    }
    std::stable_sort(v.begin(), v.end(), [](const bagua_p2p_op_t& a, const bagua_p2p_op_t& c) {
        if (a.peer != c.peer) return a.peer < c.peer;
        if (a.is_send != c.is_send) return a.is_send > c.is_send;
        return a.key < c.key;
    });
    return v;
}

}  // namespace bagua

using namespace bagua;

extern "C" {

int bagua_centralized_piece_plan(int method, int dtype, int nranks, size_t chunk_size, int schedule, int piece,
                                 int phase, int* unit_begin, int* unit_end, size_t* byte_ranges) {
    if (nranks < 1 || chunk_size > 0x7fffffffULL || !valid_schedule(schedule) || (phase != 0 && phase != 1))
        return -BAGUA_ERR_INVALID_ARG;
    Chunking k{nranks, 0, chunk_size, 0};
    const int cs = (int)chunk_size;
    if (method == BAGUA_COMPRESSION_MINMAX_UINT8) k.S = bagua_minmax_u8_compressed_bytes(dtype, cs, nranks);
    else if (method == BAGUA_COMPRESSION_ONEBIT) k.S = bagua_onebit_compressed_bytes(cs, nranks);
    else if (method == BAGUA_COMPRESSION_MXFP4) k.S = bagua_mxfp4_compressed_bytes(cs, nranks);
    else return -BAGUA_ERR_UNSUPPORTED;  // no pieced op, or none this entry describes (MXFP8: MXFP8.md, "Pipelined op")
    if (!k.S) return -BAGUA_ERR_UNSUPPORTED;
    if (k.S % (size_t)k.p) return -BAGUA_ERR_INVALID_ARG;  // the ops refuse it too (alltoall alignment)
    std::vector<Piece> v;
    const int rc = method == BAGUA_COMPRESSION_MINMAX_UINT8 ? minmax_pieces(k, schedule, &v)
                   : method == BAGUA_COMPRESSION_ONEBIT     ? onebit_pieces(k, schedule, &v)
                                                            : mxfp4_pieces(k, schedule, &v);
    if (rc) return -rc;
    if (piece < 0 || (size_t)piece >= v.size()) return -BAGUA_ERR_INVALID_ARG;
    const Piece& pc = v[(size_t)piece];
    const ByteRange* r = phase == 0 ? pc.a2a : pc.ag;
    if (unit_begin) *unit_begin = pc.b;
    if (unit_end) *unit_end = pc.e;
    for (int i = 0; i < 2 && byte_ranges; ++i) {
        byte_ranges[2 * i] = r[i].lo;
        byte_ranges[2 * i + 1] = r[i].hi;
    }
    return (int)v.size();
}

int bagua_ring_exchange_plan(int nranks, int rank, int chunk_size, int pieces, int multipath, int* groups,
                             size_t* relay_bytes) {
    RingPlan P;
    const int rc = ring_plan(nranks, rank, chunk_size, pieces, multipath != 0, &P);
    if (rc) return rc;
    if (groups) *groups = P.groups;
    if (relay_bytes) *relay_bytes = ring_relay_bytes(P);
    return BAGUA_OK;
}

int bagua_ring_exchange_ops(int nranks, int rank, int chunk_size, int pieces, int multipath, int group,
                            bagua_p2p_op_t* ops, int max_ops) {
    RingPlan P;
    const int rc = ring_plan(nranks, rank, chunk_size, pieces, multipath != 0, &P);
    if (rc) return -rc;
    if (group < 0 || group >= P.groups) return -BAGUA_ERR_INVALID_ARG;
    const std::vector<bagua_p2p_op_t> v = ring_ops(P, group);
    if (!ops || (int)v.size() > max_ops) return -BAGUA_ERR_INVALID_ARG;
    std::copy(v.begin(), v.end(), ops);
    return (int)v.size();
}

}  // extern "C"
