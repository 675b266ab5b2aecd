// Q80 weights on gfx950: the tiled device layout (Q80Tiling, kernels.h) and its host tiler, the
// synthetic fill, and the decode GEMV's launcher (kernel: q80w_inst.h, instances: q80w_l16/32/64.hip;
// the batched GEMM: q80w_gemm.hip).
#include "../core/common.h"
#include "decode_dev.h"
#include "device_comm.h"

#include <algorithm>
#include <cstring>
#include <thread>
#include <vector>

namespace dl {
namespace hipk {

Q80Tiling q80Tiling(int rows, int n, int L) {
    Q80Tiling t;
    t.L = L;
    t.NG = kThreads / L;
    const int nb = n / 32;
    t.K = (nb + L - 1) / L;
    t.groups = (rows + 2 * t.NG - 1) / (2 * t.NG);
    t.chunks = (size_t)t.groups * t.K;
    t.qBytes = t.chunks * 4 * kThreads * 16;
    t.dBytes = t.chunks * kThreads * 4;
    return t;
}

// Pass groups [gBegin, gEnd) of the tiled planes from the file's 34-byte blocks.
static void tileQ80Groups(const uint8_t *const *rowBlocks, int rows, int nb, const Q80Tiling &t, int gBegin, int gEnd,
                          uint8_t *qOut, uint32_t *dOut) {
    const int L = t.L;
    for (int g = gBegin; g < gEnd; g++)
        for (int k = 0; k < t.K; k++) {
            const size_t c = (size_t)g * t.K + k;
            for (int tid = 0; tid < kThreads; tid++) {
                const int gi = tid / L, li = tid % L, j = li + k * L;
                uint32_t dd = 0;
                for (int r = 0; r < 2; r++) {
                    const int row = 2 * (g * t.NG + gi) + r;
                    uint8_t *lo = qOut + (((c * 2 + r) * 2 + 0) * kThreads + tid) * 16;
                    uint8_t *hi = qOut + (((c * 2 + r) * 2 + 1) * kThreads + tid) * 16;
                    if (row < rows && j < nb) {
                        const uint8_t *b = rowBlocks[row] + (size_t)j * kQ80BlockBytes;
                        uint16_t dv;
                        std::memcpy(&dv, b, 2);
                        std::memcpy(lo, b + 2, 16);
                        std::memcpy(hi, b + 18, 16);
                        dd |= (uint32_t)dv << (16 * r);
                    } else {
                        std::memset(lo, 0, 16);
                        std::memset(hi, 0, 16);
                    }
                }
                dOut[c * kThreads + tid] = dd;
            }
        }
}

// Pass groups are independent output ranges: split them over host threads (as tileQ40AoS).
void tileQ80AoS(const uint8_t *const *rowBlocks, int rows, int n, int L, uint8_t *qOut, uint32_t *dOut) {
    const Q80Tiling t = q80Tiling(rows, n, L);
    const int nb = n / 32;
    const int hw = (int)std::thread::hardware_concurrency();
    const int nThreads = std::max(1, std::min({hw > 0 ? hw : 1, 32, t.groups / 4}));
    if (nThreads == 1) {
        tileQ80Groups(rowBlocks, rows, nb, t, 0, t.groups, qOut, dOut);
        return;
    }
    std::vector<std::thread> pool;
    for (int ti = 0; ti < nThreads; ti++)
        pool.emplace_back([&, ti] {
            const int g0 = (int)((long)t.groups * ti / nThreads), g1 = (int)((long)t.groups * (ti + 1) / nThreads);
            tileQ80Groups(rowBlocks, rows, nb, t, g0, g1, qOut, dOut);
        });
    for (auto &th : pool) th.join();
}

__device__ __forceinline__ uint64_t q80wMix(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

__global__ void fillQ80wKernel(uint8_t *q, uint16_t *d, size_t nUnits, size_t nScales, float scale, uint64_t seed) {
    const size_t stride = (size_t)gridDim.x * blockDim.x, i0 = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    for (size_t i = i0; i < nUnits; i += stride) {
        const uint64_t r0 = q80wMix(seed ^ (i * 2)), r1 = q80wMix(seed ^ (i * 2 + 1));
        uint4 v;
        v.x = (uint32_t)r0;
        v.y = (uint32_t)(r0 >> 32);
        v.z = (uint32_t)r1;
        v.w = (uint32_t)(r1 >> 32);
        reinterpret_cast<uint4 *>(q)[i] = v;
    }
    for (size_t i = i0; i < nScales; i += stride) {
        const float u = (float)(q80wMix(~seed ^ i) >> 40) / 16777216.0f;
        d[i] = __half_as_ushort(__float2half(scale * (0.5f + u)));
    }
}

void launchFillQ80w(uint8_t *q, uint16_t *d, size_t nUnits, size_t nScales, float scale, uint64_t seed, hipStream_t s) {
    hipLaunchKernelGGL(fillQ80wKernel, dim3(4096), dim3(256), 0, s, q, d, nUnits, nScales, scale, seed);
}

const void *gemvQ80wFnL16(int B, int pro, int epi);
const void *gemvQ80wFnL32(int B, int pro, int epi);
const void *gemvQ80wFnL64(int B, int pro, int epi);

const void *gemvQ80wDepthFnL16(int depth);
const void *gemvQ80wDepthFnL32(int depth);
const void *gemvQ80wDepthFnL64(int depth);

void launchGemvQ80w(const GemvArgs &a, int B, int pro, int epi, hipStream_t s, int depth) {
    const int L = a.lanes;
    if (L != 16 && L != 32 && L != 64) throw Error("launchGemvQ80w: lanes must be the tiling's 16, 32 or 64");
    if (a.passes < 1 || a.n % 32 || a.rows < 1) throw Error("launchGemvQ80w: bad shape");
    const int R = (kThreads / L) * 2 * a.passes;
    if (epi == EPI_ACT_Q80 && R % 64) throw Error("launchGemvQ80w: SwiGLU -> Q80 needs whole 64-row workgroups");
    if ((epi == EPI_ACT || epi == EPI_ACT_Q80 || epi == EPI_QKV) && a.rows % 2)
        throw Error("launchGemvQ80w: row-pair epilogues need an even row count");
    const void *fn = L == 16 ? gemvQ80wFnL16(B, pro, epi) : L == 32 ? gemvQ80wFnL32(B, pro, epi) : gemvQ80wFnL64(B, pro, epi);
    if (depth > 0) {  // a depth-sweep instance
        if (B != 1 || pro != PRO_GLOBAL || epi != EPI_STORE) throw Error("launchGemvQ80w: depth instances are one row, global, store");
        fn = L == 16 ? gemvQ80wDepthFnL16(depth) : L == 32 ? gemvQ80wDepthFnL32(depth) : gemvQ80wDepthFnL64(depth);
    }
    if (!fn) throw Error("launchGemvQ80w: unsupported prologue / epilogue / batch combination");
    const size_t lds = gemvLdsBytes(a.n, B, true, R, PRO_RESNORM);
    if (lds > 65536) allowLds(fn, lds);
    GemvArgs args = a;
    void *kargs[] = {&args};
    DL_HIP(hipLaunchKernel(fn, dim3((a.rows + R - 1) / R), dim3(kThreads), kargs, lds, s));
}

}  // namespace hipk
}  // namespace dl
