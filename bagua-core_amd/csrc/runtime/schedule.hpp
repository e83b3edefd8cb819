// schedule.hpp — the pure arithmetic of the pipelined comm ops' schedules (schedule.cpp):
// how many pieces, which bytes of a segment each piece moves in each exchange, which
// transfers a ring group posts.  No HIP or transport call and nothing of one rank's own
// (pointers, alignment): every input is a value equal on every rank, so all ranks derive
// the same schedule.  comm_ops.cpp enqueues what these functions lay out; the host-only
// C entries over them (bagua_centralized_piece_plan, bagua_ring_exchange_plan / _ops) let
// tests replay a schedule without a GPU.
#pragma once

#include "bagua_core.h"

#include <cstddef>
#include <vector>

namespace bagua {

struct ScheduleConfig;  // comm_internal.hpp

// p chunks of cs elements, compressed into p segments of S / p bytes
struct Chunking {
    int p = 1, rank = 0;
    size_t cs = 0, S = 0;
};

struct ByteRange {
    size_t lo, hi;
};

// One piece of a pipelined centralized op: units [b, e) of every chunk (MinMax: elements,
// 1-bit: 1024-element tiles, MXFP4: 32-element blocks) and the byte ranges of every
// segment that its alltoall group(s) and its allgather group move.  Empty ranges (hi <= lo)
// move nothing.  Per phase the non-empty ranges of all pieces partition [0, S / p).
struct Piece {
    int b, e;
    ByteRange a2a[2];
    ByteRange ag[2];
};

int auto_pieces(const ScheduleConfig& cfg, size_t payload_bytes);
int op_schedule(const ScheduleConfig& cfg, int count, int caller);
bool valid_schedule(int pieces);

// The piece table of one op, filled once before the op forks its side stream.  `sched` is a
// count >= 1, optionally OR-ed with BAGUA_PIECES_TAPERED (ignored by the 1-bit codec, whose
// pieces are uniform tile ranges).  BAGUA_ERR_INVALID_ARG: cs > INT_MAX or what the codec's
// bagua_*_piece_range refuses.
int minmax_pieces(const Chunking& k, int sched, std::vector<Piece>* v);
int onebit_pieces(const Chunking& k, int sched, std::vector<Piece>* v);
int mxfp4_pieces(const Chunking& k, int sched, std::vector<Piece>* v);
int mxfp8_pieces(const Chunking& k, int sched, std::vector<Piece>* v);

constexpr int kRingMinMultipath = 6;

struct RingPlan {
    int p = 1, r = 0, pieces = 1, groups = 1;
    int sched = 1;  // piece schedule (count + BAGUA_PIECES_TAPERED)
    bool mp = false;
    Chunking k;
    std::vector<Piece> tab;  // the MinMax table of the one-chunk bucket
    size_t slot = 0;  // relay scratch bytes per slice
};

enum { kBufMine = 0, kBufLeft = 1, kBufRight = 2, kBufRelay = 3 };

int ring_plan(int nranks, int rank, int chunk_size, int pieces, bool multipath, RingPlan* P);
size_t ring_relay_bytes(const RingPlan& P);
std::vector<bagua_p2p_op_t> ring_ops(const RingPlan& P, int g);

}  // namespace bagua
