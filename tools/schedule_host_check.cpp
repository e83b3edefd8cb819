// schedule_host_check.cpp — the comm ops' schedule arithmetic (csrc/runtime/schedule.cpp) run
// on the CPU under the sanitisers.  Plain C++, no GPU; links the (uninstrumented) kernel
// library for the bagua_*_piece_range and segment-size functions.  From the repository root:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iinclude -Ibagua-core_amd/csrc/runtime \
//       tools/schedule_host_check.cpp bagua-core_amd/csrc/runtime/schedule.cpp \
//       -Lbagua-core_amd/lib -lbagua_kernels -Wl,-rpath,$PWD/bagua-core_amd/lib -o schedule_host_check
//   ./schedule_host_check
// Loops bagua_centralized_piece_plan over every codec, p, chunk size, schedule, piece and
// phase of tests/test_centralized_pieces_cpu.py (and over refused inputs), and
// bagua_ring_exchange_plan / _ops over p = 1 .. 64, both exchange patterns and every group.
// Checks only what needs no reference: ranges inside the segment, transfers inside their
// buffers; the sanitisers check the rest.  Prints the number of calls; exit status 0.
#include <cstdio>
#include <vector>

#include "bagua_core.h"

static int fail(const char* what, int a, int b, int c, int d) {
    fprintf(stderr, "schedule_host_check: %s (%d %d %d %d)\n", what, a, b, c, d);
    return 1;
}

static size_t segments(int method, int p, int cs) {
    if (method == BAGUA_COMPRESSION_MINMAX_UINT8) return bagua_minmax_u8_compressed_bytes(BAGUA_DTYPE_F32, cs, p);
    if (method == BAGUA_COMPRESSION_ONEBIT) return bagua_onebit_compressed_bytes(cs, p);
    return bagua_mxfp4_compressed_bytes(cs, p);
}

int main() {
    const int ranks[] = {1, 2, 3, 8, 16};
    const int schedules[] = {1, 2, 3, 4, 7, 3 | BAGUA_PIECES_TAPERED, 5 | BAGUA_PIECES_TAPERED, 8 | BAGUA_PIECES_TAPERED};
    const std::vector<int> chunks[5] = {{4096},  // methods 0 and 4: no pieced op, refused
                                        {1, 511, 512, 1536, 12345, 40000},
                                        {1, 1023, 1024, 1025, 5000, 12288},
                                        {1, 32, 4095, 4096, 4097, 12288, 40000},
                                        {4096}};
    long calls = 0;
    for (int method = 0; method <= 4; ++method)
        for (int p : ranks)
            for (int cs : chunks[method])
                for (int sched : schedules)
                    for (int phase = 0; phase < 2; ++phase)
                        for (int q = -1; q <= (sched & BAGUA_PIECES_COUNT_MASK); ++q) {
                            int b = 0, e = 0;
                            size_t r[4] = {0, 0, 0, 0};
                            const int n = bagua_centralized_piece_plan(method, BAGUA_DTYPE_F32, p, (size_t)cs, sched, q,
                                                                       phase, &b, &e, r);
                            ++calls;
                            if (n < 0) continue;
                            const size_t co = segments(method, p, cs) / (size_t)p;
                            if (n != (sched & BAGUA_PIECES_COUNT_MASK) || q < 0 || q >= n || b > e)
                                return fail("piece count or unit range", method, p, cs, sched);
                            for (int i = 0; i < 2; ++i)
                                if (r[2 * i + 1] > r[2 * i] && r[2 * i + 1] > co)
                                    return fail("range past the segment", method, p, cs, sched);
                        }
    const int ring_chunks[] = {0, 1, 511, 512, 1536, 12345, 40000};
    std::vector<bagua_p2p_op_t> ops(8 * 64 + 4);  // 4 direct, 4 per relayed slice and hop
    for (int p = 1; p <= 64; ++p)
        for (int n : ring_chunks)
            for (int sched : schedules)
                for (int mp = 0; mp < 2; ++mp) {
                    const int rank = (p * 7 + n) % p;
                    int groups = 0;
                    size_t relay = 0;
                    if (bagua_ring_exchange_plan(p, rank, n, sched, mp, &groups, &relay))
                        return fail("ring plan refused", p, n, sched, mp);
                    const size_t S = segments(BAGUA_COMPRESSION_MINMAX_UINT8, 1, n);
                    for (int g = -1; g <= groups; ++g) {
                        const int cnt = bagua_ring_exchange_ops(p, rank, n, sched, mp, g, ops.data(), (int)ops.size());
                        ++calls;
                        if ((cnt < 0) != (g < 0 || g >= groups)) return fail("ring group", p, n, sched, g);
                        for (int i = 0; i < cnt; ++i)
                            if (ops[i].peer < 0 || ops[i].peer >= p || ops[i].buffer < 0 || ops[i].buffer > 3 ||
                                ops[i].offset + ops[i].bytes > (ops[i].buffer == 3 ? relay : S))
                                return fail("ring transfer outside its buffer", p, n, sched, g);
                    }
                }
    printf("schedule_host_check: %ld calls, ok\n", calls);
    return 0;
}
