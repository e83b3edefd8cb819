// mxfp8_host_check.cpp — the MXFP8 kernels' block arithmetic (csrc/kernels/mxfp8_common.hpp)
// run on the CPU.  Plain C++, no GPU:
//   g++ -O1 -ffp-contract=off -std=c++17 -Ibagua-core_amd/csrc/kernels tools/mxfp8_host_check.cpp -o mxfp8_host_check
//   mxfp8_host_check encode MAXF_BITS < blocks.f32 > bytes       (32 f32 in, 1 scale byte + 32 payload bytes out, per block)
//   mxfp8_host_check decode MAXF_BITS DTYPE < bytes > values     (33 bytes in, 32 values as T stores them out)
// MAXF_BITS: the f32 bits of the largest finite T, in hex; DTYPE: 0 f32, 1 f16, 2 bf16.
// It has its own main, so it also builds with -fsanitize=address,undefined.
// tests/test_mxfp8_cpu.py and tests/test_mxfp8_boundary_cpu.py compare both directions with
// the numpy reference.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "mxfp8_common.hpp"

using namespace bagua;

template <int K>
static int run_decode(float maxf) {
    using T = MxT<K>;
    uint8_t in[1 + kMx8BlockBytes];
    while (fread(in, 1, sizeof(in), stdin) == sizeof(in)) {
        typename T::storage out[kMxBlock];
        for (int e = 0; e < kMxBlock; ++e) out[e] = T::from_f(mx8_decode(in[1 + e], in[0], maxf));
        fwrite(out, sizeof(out[0]), kMxBlock, stdout);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const float maxf = mx_float((uint32_t)strtoul(argv[2], nullptr, 16));
    if (argc == 3 && !strcmp(argv[1], "encode")) {
        float x[kMxBlock];
        while (fread(x, sizeof(float), kMxBlock, stdin) == (size_t)kMxBlock) {
            uint32_t byte, w[8];
            mx8_encode_block(x, maxf, byte, w);
            const uint8_t b = (uint8_t)byte;
            fwrite(&b, 1, 1, stdout);
            fwrite(w, 4, 8, stdout);
        }
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "decode")) {
        switch (atoi(argv[3])) {
            case 0: return run_decode<0>(maxf);
            case 1: return run_decode<1>(maxf);
            case 2: return run_decode<2>(maxf);
        }
    }
    return 2;
}
