// mxfp4_sr_cvt_probe.hip — gfx950's v_cvt_scalef32_sr_pk_fp4_f32 on rows given by the caller
// (tools/mxfp4_sr_probe.py builds them from the MXFP4 boundary table and reads the answer).
// Stand-alone: one row is (x0, x1, scale, seed), the result byte holds the two nibbles the
// instruction packs into byte 0 of its destination (x0 low, x1 high).
//   hipcc --offload-arch=gfx950 -O2 tools/mxfp4_sr_cvt_probe.hip -o tools/mxfp4_sr_cvt_probe
//   mxfp4_sr_cvt_probe rows.bin out.bin      rows.bin: u64 n, then n x {f32 x0, f32 x1, f32 scale, u32 seed}
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

struct Row {
    float x0, x1, scale;
    uint32_t seed;
};

typedef float f32x2 __attribute__((ext_vector_type(2)));

__global__ void probe(const Row* __restrict__ rows, uint64_t n, uint8_t* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Row r = rows[i];
    f32x2 v;
    v.x = r.x0;
    v.y = r.x1;
    out[i] = (uint8_t)__builtin_amdgcn_cvt_scalef32_sr_pk_fp4_f32(0u, v, r.seed, r.scale, 0);
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    uint64_t n = 0;
    if (!f || fread(&n, sizeof(n), 1, f) != 1 || n == 0 || n > (1ull << 28)) return 2;
    std::vector<Row> rows(n);
    if (fread(rows.data(), sizeof(Row), n, f) != n) return 2;
    fclose(f);
    Row* d_rows = nullptr;
    uint8_t* d_out = nullptr;
    if (hipMalloc(&d_rows, n * sizeof(Row)) != hipSuccess || hipMalloc(&d_out, n) != hipSuccess) return 3;
    if (hipMemcpy(d_rows, rows.data(), n * sizeof(Row), hipMemcpyHostToDevice) != hipSuccess) return 3;
    probe<<<(unsigned)((n + 255) / 256), 256>>>(d_rows, n, d_out);
    if (hipDeviceSynchronize() != hipSuccess) return 3;
    std::vector<uint8_t> out(n);
    if (hipMemcpy(out.data(), d_out, n, hipMemcpyDeviceToHost) != hipSuccess) return 3;
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out.data(), 1, n, f) != n) return 4;
    fclose(f);
    return 0;
}
