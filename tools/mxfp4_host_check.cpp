// mxfp4_host_check.cpp — the MXFP4 kernels' block arithmetic (csrc/kernels/mxfp4_common.hpp)
// run on the CPU.  Plain C++, no GPU:
//   g++ -O1 -ffp-contract=off -std=c++17 -Ibagua-core_amd/csrc/kernels tools/mxfp4_host_check.cpp -o mxfp4_host_check
//   mxfp4_host_check encode MAXF_BITS < blocks.f32 > bytes    (32 f32 in, 1 scale byte + 16 payload bytes out, per block)
//   mxfp4_host_check decode MAXF_BITS < bytes > values.f32    (17 bytes in, 32 f32 out; NaN blocks as 0x7fc00000)
//   mxfp4_host_check ef MAXF_BITS DTYPE < blocks.f32 > out   (32 x then 32 residuals in; 1 scale byte, 16 payload
//                                                              bytes and the 32 new residuals out, per block)
// MAXF_BITS: the f32 bits of the largest finite T, in hex; DTYPE: 0 f32, 1 f16, 2 bf16.
// tests/test_mxfp4_cpu.py compares both directions with the numpy reference,
// tests/test_mxfp4_ef_cpu.py the error-feedback rule.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "mxfp4_common.hpp"

using namespace bagua;

template <int K>
static int run_ef(float maxf) {
    float in[2 * kMxBlock];
    while (fread(in, sizeof(float), 2 * kMxBlock, stdin) == (size_t)(2 * kMxBlock)) {
        float x[kMxBlock], e[kMxBlock];
        memcpy(x, in, sizeof(x));
        memcpy(e, in + kMxBlock, sizeof(e));
        uint32_t byte, w[4];
        mx_encode_block_ef<K>(x, e, maxf, byte, w);
        const uint8_t b = (uint8_t)byte;
        fwrite(&b, 1, 1, stdout);
        fwrite(w, 4, 4, stdout);
        fwrite(e, sizeof(float), kMxBlock, stdout);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && !strcmp(argv[1], "ef")) {
        const float m = mx_float((uint32_t)strtoul(argv[2], nullptr, 16));
        switch (atoi(argv[3])) {
            case 0: return run_ef<0>(m);
            case 1: return run_ef<1>(m);
            case 2: return run_ef<2>(m);
        }
        return 2;
    }
    if (argc != 3) return 2;
    const float maxf = mx_float((uint32_t)strtoul(argv[2], nullptr, 16));
    if (!strcmp(argv[1], "encode")) {
        float x[kMxBlock];
        while (fread(x, sizeof(float), kMxBlock, stdin) == (size_t)kMxBlock) {
            uint32_t byte, w[4];
            mx_encode_block(x, maxf, byte, w);
            const uint8_t b = (uint8_t)byte;
            fwrite(&b, 1, 1, stdout);
            fwrite(w, 4, 4, stdout);
        }
        return 0;
    }
    if (!strcmp(argv[1], "decode")) {
        uint8_t in[1 + kMxBlockBytes];
        while (fread(in, 1, sizeof(in), stdin) == sizeof(in)) {
            float out[kMxBlock];
            const float hs = mx_half_scale(in[0]);
            for (int e = 0; e < kMxBlock; ++e) {
                const uint32_t nib = (in[1 + e / 2] >> (4 * (e % 2))) & 15u;
                out[e] = in[0] == kMxNanScale ? mx_float(0x7fc00000u) : mx_dequant(nib, hs, maxf);
            }
            fwrite(out, sizeof(float), kMxBlock, stdout);
        }
        return 0;
    }
    return 2;
}
