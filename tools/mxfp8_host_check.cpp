// mxfp8_host_check.cpp — the MXFP8 kernels' block arithmetic (csrc/kernels/mxfp8_common.hpp)
// run on the CPU.  Plain C++, no GPU:
//   g++ -O1 -ffp-contract=off -std=c++17 -Ibagua-core_amd/csrc/kernels tools/mxfp8_host_check.cpp -o mxfp8_host_check
//   mxfp8_host_check encode MAXF_BITS < blocks.f32 > bytes       (32 f32 in, 1 scale byte + 32 payload bytes out, per block)
//   mxfp8_host_check decode MAXF_BITS DTYPE < bytes > values     (33 bytes in, 32 values as T stores them out)
//   mxfp8_host_check ef MAXF_BITS DTYPE < blocks.f32 > out       (32 x then 32 residuals in; 1 scale byte, 32 payload
//                                                                 bytes and the 32 new residuals out, per block)
//   mxfp8_host_check sr MAXF_BITS KEY J0 < blocks.f32 > bytes    (stochastic rounding under the 64-bit key KEY, hex:
//                                                                 consecutive blocks, the first element of the first
//                                                                 block having index J0 in its tensor; output as encode)
//   mxfp8_host_check srr MAXF_BITS < blocks > bytes              (32 f32, then the 32 elements' r as u32, in; output as
//                                                                 encode: mx8_quant_sr under explicit r values)
//   mxfp8_host_check srs MAXF_BITS SEED STEPS < blocks.f32 > bytes  (the blocks of one tensor from index 0, encoded once
//                                                                 per step 0 .. STEPS - 1 under mx_sr_key(SEED, step, 0, 0);
//                                                                 output as encode, step after step)
// MAXF_BITS: the f32 bits of the largest finite T, in hex; DTYPE: 0 f32, 1 f16, 2 bf16.
// It has its own main, so it also builds with -fsanitize=address,undefined.
// tests/test_mxfp8_cpu.py and tests/test_mxfp8_boundary_cpu.py compare both directions with
// the numpy reference, tests/test_mxfp8_ef_cpu.py the error-feedback rule,
// tests/test_mxfp8_sr_cpu.py stochastic rounding.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

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

template <int K>
static int run_ef(float maxf) {
    float in[2 * kMxBlock];
    while (fread(in, sizeof(float), 2 * kMxBlock, stdin) == (size_t)(2 * kMxBlock)) {
        float x[kMxBlock], e[kMxBlock];
        memcpy(x, in, sizeof(x));
        memcpy(e, in + kMxBlock, sizeof(e));
        uint32_t byte, w[8];
        mx8_encode_block_ef<K>(x, e, maxf, byte, w);
        const uint8_t b = (uint8_t)byte;
        fwrite(&b, 1, 1, stdout);
        fwrite(w, 4, 8, stdout);
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
            uint32_t byte, w[8];
            mx8_encode_block(x, maxf, byte, w);
            const uint8_t b = (uint8_t)byte;
            fwrite(&b, 1, 1, stdout);
            fwrite(w, 4, 8, stdout);
        }
        return 0;
    }
    if (argc == 5 && !strcmp(argv[1], "sr")) {
        const uint64_t key = strtoull(argv[3], nullptr, 16);
        uint32_t j = (uint32_t)strtoull(argv[4], nullptr, 10);
        float x[kMxBlock];
        for (; fread(x, sizeof(float), kMxBlock, stdin) == (size_t)kMxBlock; j += kMxBlock) {
            uint32_t byte, w[8];
            mx8_encode_block_sr(x, maxf, j, (uint32_t)key, (uint32_t)(key >> 32), byte, w);
            const uint8_t b = (uint8_t)byte;
            fwrite(&b, 1, 1, stdout);
            fwrite(w, 4, 8, stdout);
        }
        return 0;
    }
    if (argc == 5 && !strcmp(argv[1], "srs")) {
        const uint64_t seed = strtoull(argv[3], nullptr, 16);
        std::vector<float> x;
        float blk[kMxBlock];
        while (fread(blk, sizeof(float), kMxBlock, stdin) == (size_t)kMxBlock) x.insert(x.end(), blk, blk + kMxBlock);
        for (uint64_t step = 0; step < strtoull(argv[4], nullptr, 10); ++step) {
            const uint64_t key = mx_sr_key(seed, step, 0, 0);
            for (size_t j = 0; j < x.size(); j += kMxBlock) {
                uint32_t byte, w[8];
                memcpy(blk, &x[j], sizeof(blk));
                mx8_encode_block_sr(blk, maxf, (uint32_t)j, (uint32_t)key, (uint32_t)(key >> 32), byte, w);
                const uint8_t b = (uint8_t)byte;
                fwrite(&b, 1, 1, stdout);
                fwrite(w, 4, 8, stdout);
            }
        }
        return 0;
    }
    if (argc == 3 && !strcmp(argv[1], "srr")) {
        struct { float x[kMxBlock]; uint32_t r[kMxBlock]; } in;
        while (fread(&in, sizeof(in), 1, stdin) == 1) {
            uint32_t byte, w[8];
            mx8_encode_block(in.x, maxf, byte, w);  // the scale byte is the plain encode's
            if (byte != kMxNanScale) {
                const float inv = mx8_inv_scale(byte);
                memset(w, 0, sizeof(w));
                for (int e = 0; e < kMxBlock; ++e)
                    w[e / 4] |= mx8_quant_sr(mx_clamp(in.x[e], maxf), inv, in.r[e] & 0xffffu) << (8 * (e % 4));
            }
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
    if (argc == 4 && !strcmp(argv[1], "ef")) {
        switch (atoi(argv[3])) {
            case 0: return run_ef<0>(maxf);
            case 1: return run_ef<1>(maxf);
            case 2: return run_ef<2>(maxf);
        }
    }
    return 2;
}
