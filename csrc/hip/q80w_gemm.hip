// Batched matmul for Q80 weights on MFMA (1..64 tokens per launch):
//   out[t][row] = sum_j f32(dw[row][j]) * (sum_i qw[row][j][i] * x[t][32 j + i]),  x f16.
// A wave owns 16 weight rows on the MFMA's N side; lane (col, h) streams the 8 bytes 8h .. 8h+7 of
// every Q80 block of its row `col` straight from the tiled int8 plane into VGPRs (Q80Tiling: the
// weights are read once per launch, no LDS) with the block's f16 scale, and the matching 16 B of f16
// activations per token tile (L2-resident, shared by the workgroup's waves). int8 -> f16 is exact
// (bytes biased to 0..255 under exponent byte 0x64 = 1024 + b, minus 1152), one
// v_mfma_f32_16x16x32_f16 per block and token tile goes into a zeroed block accumulator whose four
// registers all belong to the lane's weight row, so the scale is one scalar per lane: acc += f32(dw)
// * blockAcc, four FMAs. q * d is never rounded to f16. kQ80wGemmU blocks are issued per iteration
// (8 B + 2 B + MT x 16 B per lane and block in flight). Split-K, the deterministic combine and the
// fused epilogues are the other batched GEMMs' (gemmFinish).
#include "gemm_dev.h"

namespace dl {
namespace hipk {

static constexpr int kQ80wGemmU = 4;
#ifndef DL_Q80W_GEMM_FETCH
#define DL_Q80W_GEMM_FETCH 16
#endif
// weight bytes per lane and load, 8 or 16. 16: 8B wcls / w13 at 16 tokens 319-343 / 78-81 us vs 409-416 /
// 100-101 at 8, at 64 tokens 650 / 175 vs 805 / 190; wo 18 vs 18 and 38 vs 36 (profiles/q80_weights.md)
static constexpr int kQ80wGemmFetch = DL_Q80W_GEMM_FETCH;
static constexpr int kGemmScaleFloats = 128 + 256;  // gemmFinish: per-token RMS scales + per-thread slices

// (int8 -> f16: q80ToF16x8, gemm_dev.h.)
// FETCH = 16: the same product with one 16-byte weight load per lane and block pair. Lane (col, h)
// loads the whole unit (block j + (h & 1), half h >> 1) of its row and the matching 2 x 16 B of
// activations; each block of the pair takes two MFMAs (the unit's first and second 8 bytes) in which
// the lanes holding the other block feed zeros, so the two blocks keep separate accumulators for
// their scales. Twice the MFMAs of the 8-byte form for half the weight load instructions; which
// form a launch runs is decided by measurement (kQ80wGemmFetch, profiles/q80_weights.md).
template <int MT, int EPI>
__global__ __launch_bounds__(kThreads) void gemmQ80wKernel16(GemmArgs ga) {
    const GemvArgs &a = ga.e;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int *flag = reinterpret_cast<int *>(smem + MT * 16 * kGemmRows * 4);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 15, h = lane >> 4;
    const int hh = h >> 1, sb = h & 1;
    const int n = a.n, nb = n >> 5, L = a.lanes, lg = __builtin_ctz(L), K = (nb + L - 1) >> lg;
    const int nbs = nb / ga.splits, j0 = blockIdx.y * nbs;  // nbs and j0 even (launcher)
    const int row = min(blockIdx.x * kGemmRows + wave * 16 + col, a.rows - 1);
    const int NG = kThreads / L, g = row / (2 * NG), gi = (row % (2 * NG)) >> 1, r = row & 1;
    const uint8_t *qb = a.qs + (size_t)g * K * 16384 + r * 8192 + hh * 4096 + gi * L * 16;
    const uint16_t *db = a.wd + ((size_t)g * K * kThreads + gi * L) * 2 + r;
    const _Float16 *xp = ga.x + (size_t)col * n + 16 * hh;
    f32x4 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; t++) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto wOff = [&](int j) { return (size_t)(j >> lg) * 16384 + (size_t)(j & (L - 1)) * 16; };
    auto dOff = [&](int j) { return ((size_t)(j >> lg) * kThreads + (j & (L - 1))) * 2; };
    const half8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
    constexpr int U = 2;  // block pairs per iteration
    for (int jj = 0; jj < nbs; jj += 2 * U) {
        u32x4 w[U];
        uint16_t d[U][2];
        half8 xv[U][MT][2];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int j = min(j0 + jj + 2 * u, j0 + nbs - 2);  // a pair past the split: re-read, dropped below
            w[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(qb + wOff(j + sb)));
            d[u][0] = db[dOff(j)];
            d[u][1] = db[dOff(j + 1)];
#pragma unroll
            for (int t = 0; t < MT; t++) {
                const _Float16 *p = xp + (size_t)t * 16 * n + (size_t)(j + sb) * 32;
                xv[u][t][0] = *reinterpret_cast<const half8 *>(p);
                xv[u][t][1] = *reinterpret_cast<const half8 *>(p + 8);
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            if (jj + 2 * u >= nbs) break;
            const half8 w0 = q80ToF16x8(u32x2{w[u].x, w[u].y}), w1 = q80ToF16x8(u32x2{w[u].z, w[u].w});
#pragma unroll
            for (int b = 0; b < 2; b++) {
                const half8 b0 = sb == b ? w0 : zero, b1 = sb == b ? w1 : zero;
                const float dw = __half2float(__ushort_as_half(d[u][b]));
#pragma unroll
                for (int t = 0; t < MT; t++) {
                    f32x4 s = __builtin_amdgcn_mfma_f32_16x16x32_f16(xv[u][t][0], b0, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                    s = __builtin_amdgcn_mfma_f32_16x16x32_f16(xv[u][t][1], b1, s, 0, 0, 0);
#pragma unroll
                    for (int i = 0; i < 4; i++) acc[t][i] = fmaf(dw, s[i], acc[t][i]);
                }
            }
        }
    }
    gemmFinish<MT, EPI>(ga, acc, smem, flag, blockIdx.x, gridDim.x);
}

template <int MT, int EPI>
__global__ __launch_bounds__(kThreads) void gemmQ80wKernel(GemmArgs ga) {
    const GemvArgs &a = ga.e;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int *flag = reinterpret_cast<int *>(smem + MT * 16 * kGemmRows * 4);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 15, h = lane >> 4;
    const int n = a.n, nb = n >> 5, L = a.lanes, lg = __builtin_ctz(L), K = (nb + L - 1) >> lg;
    const int nbs = nb / ga.splits, j0 = blockIdx.y * nbs;
    const int row = min(blockIdx.x * kGemmRows + wave * 16 + col, a.rows - 1);  // clamped: outputs dropped
    // the lane's 8 bytes of block j: qb + (j / L) * 16 KB + (j % L) * 16 (kernels.h q80Off)
    const int NG = kThreads / L, g = row / (2 * NG), gi = (row % (2 * NG)) >> 1, r = row & 1;
    const uint8_t *qb = a.qs + (size_t)g * K * 16384 + r * 8192 + (h >> 1) * 4096 + gi * L * 16 + (h & 1) * 8;
    const uint16_t *db = a.wd + ((size_t)g * K * kThreads + gi * L) * 2 + r;
    const _Float16 *xp = ga.x + (size_t)col * n + 8 * h;
    f32x4 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; t++) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto block = [&](u32x2 wv, uint16_t d16, const half8 (&xv)[MT]) {
        const half8 b = q80ToF16x8(wv);
        const float dw = __half2float(__ushort_as_half(d16));
#pragma unroll
        for (int t = 0; t < MT; t++) {
            const f32x4 s = __builtin_amdgcn_mfma_f32_16x16x32_f16(xv[t], b, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 4; i++) acc[t][i] = fmaf(dw, s[i], acc[t][i]);
        }
    };
    auto wOff = [&](int j) { return (size_t)(j >> lg) * 16384 + (size_t)(j & (L - 1)) * 16; };
    auto dOff = [&](int j) { return ((size_t)(j >> lg) * kThreads + (j & (L - 1))) * 2; };
    constexpr int U = kQ80wGemmU;
    int jj = 0;
    for (; jj + U <= nbs; jj += U) {
        u32x2 w[U];
        uint16_t d[U];
        half8 xv[U][MT];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int j = j0 + jj + u;
            w[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x2 *>(qb + wOff(j)));
            d[u] = db[dOff(j)];
#pragma unroll
            for (int t = 0; t < MT; t++) xv[u][t] = *reinterpret_cast<const half8 *>(xp + (size_t)t * 16 * n + (size_t)j * 32);
        }
#pragma unroll
        for (int u = 0; u < U; u++) block(w[u], d[u], xv[u]);
    }
    for (; jj < nbs; jj++) {
        const int j = j0 + jj;
        half8 xv[MT];
#pragma unroll
        for (int t = 0; t < MT; t++) xv[t] = *reinterpret_cast<const half8 *>(xp + (size_t)t * 16 * n + (size_t)j * 32);
        block(__builtin_nontemporal_load(reinterpret_cast<const u32x2 *>(qb + wOff(j))), db[dOff(j)], xv);
    }
    gemmFinish<MT, EPI>(ga, acc, smem, flag, blockIdx.x, gridDim.x);
}

void launchGemmQ80w(const GemmArgs &ga, int epi, hipStream_t s, int fetch) {
    const int tiles = (ga.e.rows + kGemmRows - 1) / kGemmRows, L = ga.e.lanes;
    if (L != 16 && L != 32 && L != 64) throw Error("launchGemmQ80w: lanes must be the tiling's 16, 32 or 64");
    if (ga.M < 1 || ga.M > kGemmF32MaxTokens) throw Error("launchGemmQ80w: 1..64 tokens per launch");
    if (ga.e.n % 32 || ga.splits < 1 || (ga.e.n / 32) % ga.splits) throw Error("launchGemmQ80w: splits must divide n / 32");
    if (ga.tpx) throw Error("launchGemmQ80w: no tile exchange");
    if (ga.splits > 1 && ga.partFloats && (size_t)ga.splits * tiles * gemmTokenPad(ga.M) * kGemmRows > ga.partFloats)
        throw Error("launchGemmQ80w: split-K partials exceed the engine's buffer");
    const int MT = gemmTokenPad(ga.M) / 16;
    const dim3 grid(tiles, ga.splits);
    const size_t lds = (size_t)MT * 16 * kGemmRows * 4 + 16 + kGemmScaleFloats * 4;  // + flag, row scales
    // the 16-byte form walks block pairs: an even number of blocks per split
    const bool f16 = (fetch ? fetch : kQ80wGemmFetch) == 16 && (ga.e.n / 32 / ga.splits) % 2 == 0;
#define DL_GEMMQ8_CASE(M_, E)                                                              \
    if (MT == M_ && epi == E && f16) {                                                     \
        if (lds > 65536) allowLds((const void *)gemmQ80wKernel16<M_, E>, lds);             \
        hipLaunchKernelGGL((gemmQ80wKernel16<M_, E>), grid, dim3(kThreads), lds, s, ga);   \
        return;                                                                            \
    }                                                                                      \
    if (MT == M_ && epi == E) {                                                            \
        if (lds > 65536) allowLds((const void *)gemmQ80wKernel<M_, E>, lds);               \
        hipLaunchKernelGGL((gemmQ80wKernel<M_, E>), grid, dim3(kThreads), lds, s, ga);     \
        return;                                                                            \
    }
#define DL_GEMMQ8_CASES(M_)                                                                \
    DL_GEMMQ8_CASE(M_, EPI_STORE) DL_GEMMQ8_CASE(M_, EPI_ACT) DL_GEMMQ8_CASE(M_, EPI_QKV)  \
    DL_GEMMQ8_CASE(M_, EPI_ACT_F16) DL_GEMMQ8_CASE(M_, EPI_RES)
    DL_GEMMQ8_CASES(1) DL_GEMMQ8_CASES(2) DL_GEMMQ8_CASES(4)
#undef DL_GEMMQ8_CASES
#undef DL_GEMMQ8_CASE
    throw Error("launchGemmQ80w: unsupported epilogue");
}

}  // namespace hipk
}  // namespace dl
