// Probe of ds_read_b64_tr_b8 lane mapping on gfx950: lane l supplies the address of 8 bytes holding
// (l << 3) | byte index, and we print which (source lane, byte) every lane receives in each of its
// 8 result bytes. Build: hipcc --offload-arch=gfx950 -O2 probe_tr8.hip
// Result on an MI355X: within each 16-lane group, lane i receives in byte j the byte i % 8 of the 8 bytes
// addressed by lane 2 j + i / 8, i.e. with lane 2 q + p addressing bytes 8 p.. of matrix row q, lane i
// gets column i of rows 0..7 (attn_fp8.hip's V^T read).
#include <hip/hip_runtime.h>
#include <cstdio>
typedef int i32x2 __attribute__((ext_vector_type(2)));
__global__ void probe(unsigned short *out) {
    // a byte cannot name both a source lane (6 bits) and a byte index (3 bits): two planes, read twice
    __shared__ __attribute__((aligned(8))) unsigned char lo[64 * 8], hi[64 * 8];
    const int l = threadIdx.x;
    for (int e = 0; e < 8; e++) {
        lo[l * 8 + e] = (unsigned char)(((l & 31) << 3) | e);  // source lane (low 5 bits), byte
        hi[l * 8 + e] = (unsigned char)(l >> 5);               // source lane bit 5
    }
    __syncthreads();
    const i32x2 a = __builtin_amdgcn_ds_read_tr8_b64_v2i32(
        reinterpret_cast<__attribute__((address_space(3))) i32x2 *>(reinterpret_cast<uintptr_t>(lo + l * 8)));
    const i32x2 b = __builtin_amdgcn_ds_read_tr8_b64_v2i32(
        reinterpret_cast<__attribute__((address_space(3))) i32x2 *>(reinterpret_cast<uintptr_t>(hi + l * 8)));
    for (int e = 0; e < 8; e++) {
        const unsigned x = ((unsigned)a[e >> 2] >> (8 * (e & 3))) & 255, y = ((unsigned)b[e >> 2] >> (8 * (e & 3))) & 255;
        out[l * 8 + e] = (unsigned short)((y << 8) | x);
    }
}
int main() {
    unsigned short *d, h[512];
    if (hipMalloc(&d, sizeof(h)) != hipSuccess) return 1;
    hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, d);
    if (hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return 1;
    for (int l = 0; l < 64; l++) {
        printf("lane %2d:", l);
        for (int e = 0; e < 8; e++) printf(" (l%d,b%d)", ((h[l * 8 + e] >> 8) << 5) | ((h[l * 8 + e] & 255) >> 3), h[l * 8 + e] & 7);
        printf("\n");
    }
    return 0;
}
