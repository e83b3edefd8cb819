// mxfp6_host_check.cpp — the MXFP6 kernels' block arithmetic (csrc/kernels/mxfp6_common.hpp)
// run on the CPU.  Plain C++, no GPU:
//   g++ -O1 -ffp-contract=off -std=c++17 -Ibagua-core_amd/csrc/kernels tools/mxfp6_host_check.cpp -o mxfp6_host_check
//   mxfp6_host_check encode MAXF_BITS < blocks.f32 > bytes       (32 f32 in, 1 scale byte + 24 payload bytes out, per block)
//   mxfp6_host_check decode MAXF_BITS DTYPE < bytes > values     (25 bytes in, 32 values as T stores them out)
//   mxfp6_host_check ef MAXF_BITS DTYPE < blocks.f32 > out       (32 x then 32 residuals in; 1 scale byte, 24 payload
//                                                                 bytes and the 32 new residuals out, per block)
// MAXF_BITS: the f32 bits of the largest finite T, in hex; DTYPE: 0 f32, 1 f16, 2 bf16.
// It has its own main, so it also builds with -fsanitize=address,undefined.
// tests/test_mxfp6_cpu.py compares both directions with the numpy reference,
// tests/test_mxfp6_ef_cpu.py the error-feedback rule.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "mxfp6_common.hpp"

using namespace bagua;

template <int K>
static int run_decode(float maxf) {
    using T = MxT<K>;
    uint8_t in[1 + kMx6BlockBytes];
    while (fread(in, 1, sizeof(in), stdin) == sizeof(in)) {
        uint32_t w[kMx6BlockWords];
        memcpy(w, in + 1, sizeof(w));
        typename T::storage out[kMxBlock];
        for (int e = 0; e < kMxBlock; ++e) out[e] = T::from_f(mx6_decode(mx6_code_at(w, 6 * e), in[0], maxf));
        fwrite(out, sizeof(out[0]), kMxBlock, stdout);
    }
    return 0;
}

template <int K>
static int run_ef(float maxf) {
    float in[2 * kMxBlock];
    while (fread(in, sizeof(float), 2 * kMxBlock, stdin) == (size_t)(2 * kMxBlock)) {
        float x[kMxBlock], e[kMxBlock];
        memcpy(x, in, sizeof(x));
        memcpy(e, in + kMxBlock, sizeof(e));
        uint32_t byte, w[kMx6BlockWords];
        mx6_encode_block_ef<K>(x, e, maxf, byte, w);
        const uint8_t b = (uint8_t)byte;
        fwrite(&b, 1, 1, stdout);
        fwrite(w, 4, kMx6BlockWords, stdout);
        fwrite(e, sizeof(float), kMxBlock, stdout);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const float maxf = mx_float((uint32_t)strtoul(argv[2], nullptr, 16));
    if (argc == 3 && !strcmp(argv[1], "encode")) {
        float x[kMxBlock];
        while (fread(x, sizeof(float), kMxBlock, stdin) == (size_t)kMxBlock) {
            uint32_t byte, w[kMx6BlockWords];
            mx6_encode_block(x, maxf, byte, w);
            const uint8_t b = (uint8_t)byte;
            fwrite(&b, 1, 1, stdout);
            fwrite(w, 4, kMx6BlockWords, stdout);
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
    if (argc == 4 && !strcmp(argv[1], "ef")) {
        switch (atoi(argv[3])) {
            case 0: return run_ef<0>(maxf);
            case 1: return run_ef<1>(maxf);
            case 2: return run_ef<2>(maxf);
        }
    }
    return 2;
}
