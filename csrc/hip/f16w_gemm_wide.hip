// Wide batched GEMM for F16 weights on MFMA (prefill chunks and serving batches above the wide
// threshold, gemmUsesWide): the frame of gemm_wide.hip / q80w_gemm_wide.hip with the numerics of
// f16w_gemm.hip,
//   out[t][row] = sum_k w[row][k] * f16(x[t][k])      w f16 row-major [rows][n] (GemvArgs::wh)
// f16 x f16 products are exact in f32 and v_mfma_f32_16x16x32_f16 accumulates in f32, so the caller's
// rounding of x is the only one. One launch covers every token tile of a forward (grid = row tiles x
// token tiles x K splits, mapped XCD-aware so a row tile's token tiles and splits share one L2), where
// the narrow kernel re-streams the weights per 64 tokens and re-reads the activations per wave.
//
// Workgroup: 256 threads = 4 waves in 2 x 2, wave (wr, wt) owning rows [64 wr, 64 wr + 64) x tokens
// [64 wt, 64 wt + 64) of a 128 x 128 tile: 4 x 4 accumulators (64 VGPRs). K advances 64 per pipeline
// stage. The two operands take one path: a stage is two panels of the same shape, the tile's 128
// weight rows x 64 k and its 128 tokens x 64 k, 128 lines of 128 B = 1024 16-byte units each. Both
// are copied HBM / L2 -> LDS by global_load_lds, 4 + 4 wave-instructions per thread and stage; within
// an instruction 8 lanes fetch one row's 128 contiguous bytes (a whole line of the row-major matrix),
// 8 rows per instruction. Both panels use gemm_wide.hip's activation image: unit u of row / token r
// sits at 16-byte position u ^ ((r >> 1) & 7) of its line, conflict-free for the 16-lane ds_read_b128
// fragment read. The copy writes LDS in lane order, so the lane at position p of line r fetches
// global unit p ^ ((r >> 1) & 7). There is no dequantisation and there are no scales: a lane's
// ds_read_b128 of its weight row at unit 4 kb + h is the MFMA's B operand as it sits in memory, the
// activation read at the same unit the A operand. Per 32-k block a wave issues 4 + 4 ds_read_b128 and
// 16 MFMAs straight into acc[f][t].
//
// Stage depth: kHWStages stages of 32 KB; the output tile (66 KB) bounds the footprint from below.
// Two stages (64 KB, under the tile) let two workgroups share a CU's 160 KB, one stage in flight each;
// three (96 KB) leave one workgroup per CU with two in flight. profiles/f16_wide_gemm.md has both.
// Split-K (whole stages per split), the deterministic combine, the per-token RMS scales of a fused
// norm consumer and the fused epilogues are the shared ones (decode_common.h, gemm_dev.h); split
// counts, partial and counter sizes are gemm_wide.hip's (gemmWideSplits / PartFloats / Counters).
#include "gemm_dev.h"

namespace dl {
namespace hipk {

static constexpr int kHWRows = 128, kHWTok = 128, kHWK = 64, kHWStages = 2;
static constexpr int kHWPanel = kHWRows * kHWK * 2;  // [128 rows or tokens][8 x 16 B], swizzled
static constexpr int kHWNld = 2 * kHWPanel / (kThreads * 16);  // copies per thread and stage: 4 + 4
static constexpr int kHWStage = 2 * kHWPanel;
static constexpr int kHWTileLd = kHWRows + 4;  // padded f32 row stride of the output tile
static constexpr int kHWMain = kHWStages * kHWStage > kHWTok * kHWTileLd * 4 ? kHWStages * kHWStage : kHWTok * kHWTileLd * 4;
static constexpr size_t kHWLds = kHWMain + 16 + (128 + 256) * 4;  // + flag + row scales / scratch
static_assert(kHWRows == kHWTok && kHWStages >= 2 && (kHWStages - 1) * kHWNld < 64, "one panel shape; vmcnt is 6 bits");

// this thread's copies of the oldest stage landed: at most D younger stages stay in flight, `younger`
// (0..D) of them issued
template <int D>
__device__ __forceinline__ void waitStage(int younger) {
    if constexpr (D > 0) {
        if (younger == D) {
            asm volatile("s_waitcnt vmcnt(%0)" ::"i"(D * kHWNld) : "memory");
            return;
        }
        waitStage<D - 1>(younger);
    } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
}

template <int EPI>
__global__ __launch_bounds__(kThreads) void gemmF16wWideKernel(GemmArgs ga, int rowTiles, int tokTiles) {
    const GemvArgs &a = ga.e;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int *flag = reinterpret_cast<int *>(smem + kHWMain);
    float *rsL = reinterpret_cast<float *>(flag + 4);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int col = lane & 15, h = lane >> 4, wr = wave & 1, wt = wave >> 1;
    // XCD-aware order (gemm_wide.hip): logical tile Lg runs on XCD Lg / (G / 8)
    const int G = gridDim.x, id = blockIdx.x;
    const int Lg = (G & 7) == 0 ? (id & 7) * (G >> 3) + (id >> 3) : id;
    const int S = ga.splits, per = tokTiles * S;
    const int rt = Lg / per, rem = Lg - rt * per, tt = rem / S, sp = rem - tt * S;
    const int R0 = rt * kHWRows, T0 = tt * kHWTok;
    const int n = a.n, kps = n / S, k0 = sp * kps;  // kps a whole number of stages (launcher)

    // this thread's part of a panel copy: instruction q moves lines 8 (wave + 4 q) .. + 7, this lane
    // position lane & 7 of line rl + 32 q. (line >> 1) & 7 does not depend on q: one global unit.
    const int rl = wave * 8 + (lane >> 3), u = (lane & 7) ^ ((rl >> 1) & 7);
    const _Float16 *wsrc[4], *xsrc[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        wsrc[q] = a.wh + (size_t)min(R0 + rl + 32 * q, a.rows - 1) * n + k0 + u * 8;  // clamped: outputs dropped
        xsrc[q] = ga.x + (size_t)(T0 + rl + 32 * q) * n + k0 + u * 8;                 // rows past M: the zero pad
    }
    auto issue = [&](int c, int b) {  // global -> LDS copies of K stage c into stage buffer b
        char *st = smem + b * kHWStage + wave * 1024;
#pragma unroll
        for (int q = 0; q < 4; q++) glds16(wsrc[q] + c * kHWK, st + q * 4096);
#pragma unroll
        for (int q = 0; q < 4; q++) glds16(xsrc[q] + c * kHWK, st + kHWPanel + q * 4096);
    };

    f32x4 acc[4][4];
#pragma unroll
    for (int f = 0; f < 4; f++)
#pragma unroll
        for (int t = 0; t < 4; t++) acc[f][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    // fragment reads: line 64 wr (wt) + 16 f (t) + col, whose swizzle (line >> 1) & 7 is col's alone
    const int sw = (col >> 1) & 7;
    const int offW = (wr * 64 + col) * 128, offX = kHWPanel + (wt * 64 + col) * 128;
    constexpr int PF = kHWStages - 1;
    const int nch = kps / kHWK;
    for (int c = 0; c < PF && c < nch; c++) issue(c, c);
    for (int c = 0; c < nch; c++) {
        if (c + PF < nch) issue(c + PF, (c + PF) % kHWStages);
        // stage c landed for this thread (the younger stages may stay in flight), then for all
        waitStage<PF>(min(nch - 1, c + PF) - c);
        __builtin_amdgcn_s_barrier();
        const char *st = smem + (c % kHWStages) * kHWStage;
#pragma unroll
        for (int kb = 0; kb < kHWK / 32; kb++) {
            const int pos = ((kb * 4 + h) ^ sw) * 16;
            half8 b[4], av[4];
#pragma unroll
            for (int f = 0; f < 4; f++) b[f] = *reinterpret_cast<const half8 *>(st + offW + f * 2048 + pos);
#pragma unroll
            for (int t = 0; t < 4; t++) av[t] = *reinterpret_cast<const half8 *>(st + offX + t * 2048 + pos);
#pragma unroll
            for (int t = 0; t < 4; t++)
#pragma unroll
                for (int f = 0; f < 4; f++) acc[f][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av[t], b[f], acc[f][t], 0, 0, 0);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();  // stage c % kHWStages is refilled at iteration c + 1
    }

    // C layout: acc[f][t][i] = out[token 64 wt + 16 t + 4 h + i][row 64 wr + 16 f + col]
    float *tile = reinterpret_cast<float *>(smem);  // [128 tokens][kHWTileLd], the stages are free
    if (S == 1) {
#pragma unroll
        for (int f = 0; f < 4; f++)
#pragma unroll
            for (int t = 0; t < 4; t++)
#pragma unroll
                for (int i = 0; i < 4; i++)
                    tile[(wt * 64 + t * 16 + h * 4 + i) * kHWTileLd + wr * 64 + f * 16 + col] = acc[f][t][i];
    } else {
        const int lt = rt * tokTiles + tt;
        const size_t tileF = (size_t)kHWTok * kHWRows, stride = (size_t)rowTiles * tokTiles * tileF;
        float *part = ga.part + sp * stride + lt * tileF;
#pragma unroll
        for (int f = 0; f < 4; f++)
#pragma unroll
            for (int t = 0; t < 4; t++)
#pragma unroll
                for (int i = 0; i < 4; i++)
                    wtStore(part + (wt * 64 + t * 16 + h * 4 + i) * kHWRows + wr * 64 + f * 16 + col, acc[f][t][i]);
        if (!splitArrive(ga.counters + lt, S, flag)) return;
        splitCombine(ga.part + lt * tileF, stride, S, (int)(tileF / 4), reinterpret_cast<f32x4 *>(tile), kHWRows / 4,
                     kHWTileLd / 4);
    }
    __syncthreads();
    if (ga.ssIn) gemmRowScales(ga, T0, kHWTok, rsL, rsL + 128);
    gemmEpilogue<EPI, kHWRows / 2>(ga, tile, kHWTileLd, 0, min(kHWTok, ga.M - T0), T0, R0, rt * 2,
                                   ga.ssIn ? rsL : nullptr);
}

// preloadModules(): one kernel of this translation unit's code object
const void *gemmF16wWideModuleKernel() { return (const void *)gemmF16wWideKernel<EPI_STORE>; }

void launchGemmF16wWide(const GemmArgs &ga, int epi, hipStream_t s) {
    const int rowTiles = (ga.e.rows + kHWRows - 1) / kHWRows, tokTiles = (ga.M + kHWTok - 1) / kHWTok;
    if (!ga.e.wh || ga.M < 1 || ga.e.rows < 1) throw Error("launchGemmF16wWide: no F16 weights or bad shape");
    if (!gemmWideAccepts(ga.e.n, ga.splits)) throw Error("launchGemmF16wWide: bad K split (whole 64-k stages per split)");
    if (ga.tpx) throw Error("launchGemmF16wWide: no tile exchange");
    if (ga.splits > 1 && (!ga.part || !ga.counters)) throw Error("launchGemmF16wWide: split-K without buffers");
    if (ga.splits > 1 && ga.partFloats && (size_t)ga.splits * rowTiles * tokTiles * kHWRows * kHWTok > ga.partFloats)
        throw Error("launchGemmF16wWide: split-K partials exceed the engine's buffer");
    const dim3 grid(rowTiles * tokTiles * ga.splits);
#define DL_GEMMHW_CASE(E)                                                                                  \
    if (epi == E) {                                                                                        \
        allowLds((const void *)gemmF16wWideKernel<E>, kHWLds);                                             \
        hipLaunchKernelGGL((gemmF16wWideKernel<E>), grid, dim3(kThreads), kHWLds, s, ga, rowTiles, tokTiles); \
        return;                                                                                            \
    }
    DL_GEMMHW_CASE(EPI_STORE) DL_GEMMHW_CASE(EPI_ACT) DL_GEMMHW_CASE(EPI_QKV) DL_GEMMHW_CASE(EPI_ACT_F16)
    DL_GEMMHW_CASE(EPI_RES)
#undef DL_GEMMHW_CASE
    throw Error("launchGemmF16wWide: unsupported epilogue");
}

}  // namespace hipk
}  // namespace dl
