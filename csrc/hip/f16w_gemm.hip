// F16 weights on gfx950: the narrow batched MFMA GEMM (1..64 tokens per launch; forwards of >= 65
// tokens take the wide LDS-staged kernel of f16w_gemm_wide.hip, gemmChunkTokens), the decode GEMV's
// launcher (kernel: f16w_inst.h, instances: f16w_l16/32/64.hip) and the synthetic fill.
//
//   out[t][row] = sum_k w[row][k] * x[t][k]      w f16 row-major [rows][n], x f16
//
// f16 x f16 products are exact in f32 and v_mfma_f32_16x16x32_f16 accumulates in f32, so rounding x
// to f16 once (the caller's, as on the F32 and Q80 batched paths) is the only rounding. The geometry
// is gemmF32Kernel's: 64-row tiles, a wave owns 16 rows on the MFMA's N side, MT token tiles, grid =
// row tiles x K splits. Per 64-k step lane (col, h) streams 32 contiguous bytes of its row `col`
// (k = 16h .. 16h+15 of the step: the four h lanes of a row cover one whole 128-byte line) straight
// into VGPRs - the weights are read once, no LDS, no conversion - and the matching 2 x 16 B of f16
// activations per token tile (L2-resident, shared by the workgroup's waves). Each 16-byte half is the
// B operand of one MFMA whose A operand is the activations read at the same offsets: lane (col, h)
// element e of MFMA q carries k = 16h + 8q + e on both operands, a permutation of k common to both.
// kF16wGemmU steps are issued per iteration (kF16wGemmU x 32 B of weights per lane in flight). A 32-k
// remainder step (per-split K = 64 m + 32) reads 16 B per lane, k = 8h .. 8h+7. Split-K, the
// deterministic combine and the fused epilogues are the other batched GEMMs' (gemmFinish).
#include "gemm_dev.h"
#include "device_comm.h"
#include "f16w_inst.h"

namespace dl {
namespace hipk {

static constexpr int kF16wGemmU = 4;
static constexpr int kGemmScaleFloats = 128 + 256;  // gemmFinish: per-token RMS scales + per-thread slices

template <int MT, int EPI>
__global__ __launch_bounds__(kThreads) void gemmF16wKernel(GemmArgs ga) {
    const GemvArgs &a = ga.e;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int *flag = reinterpret_cast<int *>(smem + MT * 16 * kGemmRows * 4);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 15, h = lane >> 4;
    const int n = a.n, kps = n / ga.splits, k0 = blockIdx.y * kps;  // kps a multiple of 32 (launcher)
    const int row = min(blockIdx.x * kGemmRows + wave * 16 + col, a.rows - 1);  // clamped: outputs dropped
    const _Float16 *wp = a.wh + (size_t)row * n + k0;
    const _Float16 *xp = ga.x + (size_t)col * n + k0;
    f32x4 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; t++) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    constexpr int U = kF16wGemmU;
    const int k64 = kps & ~63;
    // steps [k, k + 64 * cnt), cnt <= U: all loads of the group go out before its first MFMA
    auto group = [&](int k, int cnt) {
        half8 w[U][2], xv[U][MT][2];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int ku = k + 64 * min(u, cnt - 1) + 16 * h;  // a step past the group: re-read, dropped below
            w[u][0] = __builtin_nontemporal_load(reinterpret_cast<const half8 *>(wp + ku));
            w[u][1] = __builtin_nontemporal_load(reinterpret_cast<const half8 *>(wp + ku + 8));
#pragma unroll
            for (int t = 0; t < MT; t++) {
                const _Float16 *p = xp + (size_t)t * 16 * n + ku;
                xv[u][t][0] = *reinterpret_cast<const half8 *>(p);
                xv[u][t][1] = *reinterpret_cast<const half8 *>(p + 8);
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            if (u >= cnt) break;
#pragma unroll
            for (int q = 0; q < 2; q++)
#pragma unroll
                for (int t = 0; t < MT; t++)
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xv[u][t][q], w[u][q], acc[t], 0, 0, 0);
        }
    };
    int k = 0;
    for (; k + 64 * U <= k64; k += 64 * U) group(k, U);
    if (k < k64) group(k, (k64 - k) >> 6);
    if (k64 < kps) {  // the 32-k remainder
        const half8 w = __builtin_nontemporal_load(reinterpret_cast<const half8 *>(wp + k64 + 8 * h));
#pragma unroll
        for (int t = 0; t < MT; t++) {
            const half8 xv = *reinterpret_cast<const half8 *>(xp + (size_t)t * 16 * n + k64 + 8 * h);
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(xv, w, acc[t], 0, 0, 0);
        }
    }
    gemmFinish<MT, EPI>(ga, acc, smem, flag, blockIdx.x, gridDim.x);
}

void launchGemmF16w(const GemmArgs &ga, int epi, hipStream_t s) {
    const int tiles = (ga.e.rows + kGemmRows - 1) / kGemmRows;
    if (ga.M < 1 || ga.M > kGemmF32MaxTokens) throw Error("launchGemmF16w: 1..64 tokens per launch");
    if (!ga.e.wh || ga.e.rows < 1) throw Error("launchGemmF16w: no F16 weights");
    if (ga.e.n % 32 || ga.splits < 1 || (ga.e.n / 32) % ga.splits) throw Error("launchGemmF16w: splits must divide n / 32");
    if (ga.tpx) throw Error("launchGemmF16w: no tile exchange");
    if (ga.splits > 1 && ga.partFloats && (size_t)ga.splits * tiles * gemmTokenPad(ga.M) * kGemmRows > ga.partFloats)
        throw Error("launchGemmF16w: split-K partials exceed the engine's buffer");
    const int MT = gemmTokenPad(ga.M) / 16;
    const dim3 grid(tiles, ga.splits);
    const size_t lds = (size_t)MT * 16 * kGemmRows * 4 + 16 + kGemmScaleFloats * 4;  // + flag, row scales
#define DL_GEMMH_CASE(M_, E)                                                               \
    if (MT == M_ && epi == E) {                                                            \
        if (lds > 65536) allowLds((const void *)gemmF16wKernel<M_, E>, lds);               \
        hipLaunchKernelGGL((gemmF16wKernel<M_, E>), grid, dim3(kThreads), lds, s, ga);     \
        return;                                                                            \
    }
#define DL_GEMMH_CASES(M_)                                                                 \
    DL_GEMMH_CASE(M_, EPI_STORE) DL_GEMMH_CASE(M_, EPI_ACT) DL_GEMMH_CASE(M_, EPI_QKV)     \
    DL_GEMMH_CASE(M_, EPI_ACT_F16) DL_GEMMH_CASE(M_, EPI_RES)
    DL_GEMMH_CASES(1) DL_GEMMH_CASES(2) DL_GEMMH_CASES(4)
#undef DL_GEMMH_CASES
#undef DL_GEMMH_CASE
    throw Error("launchGemmF16w: unsupported epilogue");
}

// ---- decode GEMV launcher ----------------------------------------------------------------------
const void *gemvF16wFnL16(int B, int pro, int epi);
const void *gemvF16wFnL32(int B, int pro, int epi);
const void *gemvF16wFnL64(int B, int pro, int epi);

int gemvF16wRowsPerPass(int lanes) { return kThreads / lanes * kF16wRG; }

int gemvF16wLanes(int n, int rows, int B) {
    int L = gemvLanesPerRow(n, rows, B, false);
    while (L < 64 && rows / gemvF16wRowsPerPass(L) < 256) L *= 2;  // the grid still covers the CUs
    return L;
}

void launchGemvF16w(const GemvArgs &a, int B, int pro, int epi, hipStream_t s) {
    if (!a.wh || a.passes < 1 || a.n % 32 || a.rows < 1) throw Error("launchGemvF16w: bad shape");
    const int L = a.lanes > 0 ? a.lanes : gemvF16wLanes(a.n, a.rows, B);
    if (L != 16 && L != 32 && L != 64) throw Error("launchGemvF16w: lanes must be 16, 32 or 64");
    if ((epi == EPI_ACT || epi == EPI_QKV) && a.rows % 2) throw Error("launchGemvF16w: row-pair epilogues need an even row count");
    const void *fn = L == 16 ? gemvF16wFnL16(B, pro, epi) : L == 32 ? gemvF16wFnL32(B, pro, epi) : gemvF16wFnL64(B, pro, epi);
    if (!fn) throw Error("launchGemvF16w: unsupported prologue / epilogue / batch combination");
    const int R = gemvF16wRowsPerPass(L) * a.passes;
    const size_t lds = gemvLdsBytes(a.n, B, false, R, pro);
    if (lds > 65536) allowLds(fn, lds);
    GemvArgs args = a;
    void *kargs[] = {&args};
    DL_HIP(hipLaunchKernel(fn, dim3((a.rows + R - 1) / R), dim3(kThreads), kargs, lds, s));
}

// ---- synthetic weights: launchFillF32Uniform's values, rounded to f16 ----------------------------
__device__ __forceinline__ uint64_t f16wMix(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

__global__ void fillF16Kernel(_Float16 *p, size_t n, float amp, uint64_t seed) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float u = (float)(f16wMix(seed ^ i) >> 40) / 16777216.0f;
        p[i] = (_Float16)(amp * (2.0f * u - 1.0f));
    }
}

void launchFillF16Uniform(_Float16 *p, size_t n, float amp, uint64_t seed, hipStream_t s) {
    hipLaunchKernelGGL(fillF16Kernel, dim3(4096), dim3(256), 0, s, p, n, amp, seed);
}

}  // namespace hipk
}  // namespace dl
