// mxfp4_host_check.cpp — the MXFP4 kernels' block arithmetic (csrc/kernels/mxfp4_common.hpp)
// run on the CPU.  Plain C++, no GPU:
//   g++ -O1 -ffp-contract=off -std=c++17 -Ibagua-core_amd/csrc/kernels tools/mxfp4_host_check.cpp -o mxfp4_host_check
//   mxfp4_host_check encode MAXF_BITS < blocks.f32 > bytes    (32 f32 in, 1 scale byte + 16 payload bytes out, per block)
//   mxfp4_host_check decode MAXF_BITS < bytes > values.f32    (17 bytes in, 32 f32 out; NaN blocks as 0x7fc00000)
//   mxfp4_host_check ef MAXF_BITS DTYPE < blocks.f32 > out   (32 x then 32 residuals in; 1 scale byte, 16 payload
//                                                              bytes and the 32 new residuals out, per block)
//   mxfp4_host_check ring MAXF_BITS DTYPE N < tensors > out  (t, w, l, r of N elements of T in; the four tensors
//                                                              after one rank's ring op, then the segment, out)
//   mxfp4_host_check sr MAXF_BITS KEY J0 < blocks.f32 > bytes  (stochastic rounding under the 64-bit key KEY, hex:
//                                                              consecutive blocks, the first element of the first
//                                                              block having index J0 in its tensor; output as encode)
//   mxfp4_host_check srr MAXF_BITS < blocks > bytes            (32 f32, then the 32 elements' r as u32, in; output as
//                                                              encode: mx_quant_sr under explicit r values)
// MAXF_BITS: the f32 bits of the largest finite T, in hex; DTYPE: 0 f32, 1 f16, 2 bf16.
// tests/test_mxfp4_cpu.py compares both directions with the numpy reference,
// tests/test_mxfp4_ef_cpu.py the error-feedback rule, tests/test_mxfp4_ring_cpu.py the ring op,
// tests/test_mxfp4_sr_cpu.py stochastic rounding.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mxfp4_common.hpp"
#include "ring_mix.hpp"

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

// One rank's decentralized ring op (its own left and right peer): N elements of t, w, l, r in,
// the four tensors after the op and the n_chunks = 1 segment of the mixed t out.
template <int K>
static int run_ring(int64_t n, float maxf) {
    using T = MxT<K>;
    using S = typename T::storage;
    if (n <= 0) return 2;
    std::vector<S> a[4];  // t, w, l, r
    for (auto& v : a) {
        v.resize((size_t)n);
        if (fread(v.data(), sizeof(S), (size_t)n, stdin) != (size_t)n) return 3;
    }
    const float f13 = mx_ring_factor(K, 1.0 / 3.0), f53 = mx_ring_factor(K, -5.0 / 3.0);
    const int64_t nb = mx_blocks(n), sbytes = mx_scale_bytes(n);
    std::vector<uint8_t> seg((size_t)mx_segment_bytes(n), 0);
    for (int64_t b = 0; b < nb; ++b) {
        float m[kMxBlock];
        for (int e = 0; e < kMxBlock; ++e) {  // elements at or past n count as +0 and are not read
            const int64_t j = b * kMxBlock + e;
            m[e] = j < n ? mix<T>(T::to_f(a[0][j]), T::to_f(a[2][j]), T::to_f(a[3][j]), T::to_f(a[1][j]), f13, f53) : 0.0f;
        }
        uint32_t byte, w[4];
        mx_encode_block(m, maxf, byte, w);
        seg[(size_t)b] = (uint8_t)byte;
        memcpy(&seg[(size_t)(sbytes + b * kMxBlockBytes)], w, kMxBlockBytes);
        for (int e = 0; e < kMxBlock; ++e) {
            const int64_t j = b * kMxBlock + e;
            if (j >= n) break;
            const float d = mx_dq<T>((w[e / 8] >> (4 * (e % 8))) & 15u, byte, maxf);
            float t = 0.0f, wt = T::to_f(a[1][j]), l = T::to_f(a[2][j]), r = T::to_f(a[3][j]);
            mx_ring_apply<T>(d, d, d, t, wt, l, r);
            a[0][j] = T::from_f(t);
            a[1][j] = T::from_f(wt);
            a[2][j] = T::from_f(l);
            a[3][j] = T::from_f(r);
        }
    }
    for (auto& v : a) fwrite(v.data(), sizeof(S), (size_t)n, stdout);
    fwrite(seg.data(), 1, seg.size(), stdout);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 5 && !strcmp(argv[1], "ring")) {
        const float m = mx_float((uint32_t)strtoul(argv[2], nullptr, 16));
        const int64_t n = strtoll(argv[4], nullptr, 10);
        switch (atoi(argv[3])) {
            case 0: return run_ring<0>(n, m);
            case 1: return run_ring<1>(n, m);
            case 2: return run_ring<2>(n, m);
        }
        return 2;
    }
    if (argc == 4 && !strcmp(argv[1], "ef")) {
        const float m = mx_float((uint32_t)strtoul(argv[2], nullptr, 16));
        switch (atoi(argv[3])) {
            case 0: return run_ef<0>(m);
            case 1: return run_ef<1>(m);
            case 2: return run_ef<2>(m);
        }
        return 2;
    }
    if (argc == 5 && !strcmp(argv[1], "sr")) {
        const float m = mx_float((uint32_t)strtoul(argv[2], nullptr, 16));
        const uint64_t key = strtoull(argv[3], nullptr, 16);
        uint32_t j = (uint32_t)strtoull(argv[4], nullptr, 10);
        float x[kMxBlock];
        for (; fread(x, sizeof(float), kMxBlock, stdin) == (size_t)kMxBlock; j += kMxBlock) {
            uint32_t byte, w[4];
            mx_encode_block_sr(x, m, j, (uint32_t)key, (uint32_t)(key >> 32), byte, w);
            const uint8_t b = (uint8_t)byte;
            fwrite(&b, 1, 1, stdout);
            fwrite(w, 4, 4, stdout);
        }
        return 0;
    }
    if (argc == 3 && !strcmp(argv[1], "srr")) {
        const float m = mx_float((uint32_t)strtoul(argv[2], nullptr, 16));
        struct { float x[kMxBlock]; uint32_t r[kMxBlock]; } in;
        while (fread(&in, sizeof(in), 1, stdin) == 1) {
            uint32_t byte, w[4];
            mx_encode_block(in.x, m, byte, w);  // the scale byte is the plain encode's
            if (byte != kMxNanScale) {
                const float inv = mx_inv_scale(byte);
                w[0] = w[1] = w[2] = w[3] = 0u;
                for (int e = 0; e < kMxBlock; ++e)
                    w[e / 8] |= mx_quant_sr(mx_clamp(in.x[e], m), inv, in.r[e] & 0xffffu) << (4 * (e % 8));
            }
            const uint8_t b = (uint8_t)byte;
            fwrite(&b, 1, 1, stdout);
            fwrite(w, 4, 4, stdout);
        }
        return 0;
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
