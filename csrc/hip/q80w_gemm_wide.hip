// Wide batched GEMM for Q80 weights on MFMA (prefill chunks and serving batches above the wide
// threshold, gemmUsesWide): gemm_wide.hip's geometry with the numerics of q80w_gemm.hip,
//   out[t][row] = sum_j f32(dw[row][j]) * (sum_i qw[row][j][i] * f16(x[t][32 j + i])).
// One launch covers every token tile of a forward (grid = row tiles x token tiles x K splits, mapped
// XCD-aware so a row tile's token tiles and splits share one L2), where the narrow kernel re-streams
// the weights per 64 tokens and re-reads the activations per wave from L1 / L2.
//
// Workgroup: 256 threads = 4 waves in 2 x 2, wave (wr, wt) owning rows [64 wr, 64 wr + 64) x tokens
// [64 wt, 64 wt + 64) of a 128 x 128 tile: 4 x 4 accumulators of v_mfma_f32_16x16x32_f16 (64 VGPRs).
// K advances two Q80 blocks (64) per pipeline stage. A stage holds the tile's 128 weight rows as
// 512 16-byte units of the tiled int8 plane (Q80Tiling, no other weight layout: unit = half hh of
// block kb of a row, address q80Off), their f16 scales as the plane's u32 row pairs, and the 128
// tokens' 64 f16 activations, all copied HBM / L2 -> LDS by global_load_lds: 2 + 1 + 4
// wave-instructions per thread and stage, 3 stages = 2 in flight (counted s_waitcnt vmcnt, raw
// barriers), 25 KB per stage, ~77 KB per workgroup (two workgroups per CU).
//
// Per block a wave walks its four weight fragments one at a time: ds_read_b64 of the lane's 8 codes,
// int8 -> f16 (exact, q80ToF16x8), four MFMAs (one per token fragment) into zeroed block
// accumulators, then acc[f][t] += f32(dw) * blockAcc: in the C layout all four registers of
// acc[f][t] belong to weight row `col`, so the block scale is one scalar per lane and fragment.
// q * d is never rounded to f16. The block accumulators take 16 VGPRs, reused by the next fragment.
//
// LDS images, bank-conflict free:
//   int8 units  position (hh * 128 + row) * 2 + (kb ^ ((row >> 3) & 1)): lanes 2m, 2m + 1 of a copy
//               fetch blocks j, j + 1 of one (row, hh), 32 contiguous bytes of the plane, and a
//               row's two blocks swap places for rows 8..15 of each 16. A fragment's ds_read_b64
//               serves 32 lanes (16 rows x the two 8-byte halves of unit hh) per pass: rows 0..7 sit at
//               even + kb, rows 8..15 at odd - kb 16-byte positions of one 512-byte span, all 16
//               distinct modulo 256 B = the 64 banks.
//   scales      [kb][64 row pairs] u32; the lanes of a fragment read 8 consecutive words (broadcast
//               within a pair and across h).
//   activations gemm_wide.hip's: unit u of token t at position u ^ ((t >> 1) & 7).
// Split-K (whole stages per split), the deterministic combine, the per-token RMS scales of a fused
// norm consumer and the fused epilogues are the shared ones (decode_common.h, gemm_dev.h); split
// counts, partial and counter sizes are gemm_wide.hip's (gemmWideSplits / PartFloats / Counters).
#include "gemm_dev.h"

namespace dl {
namespace hipk {

static constexpr int kQWRows = 128, kQWTok = 128, kQWKB = 2, kQWStages = 3, kQWNld = 7;
static constexpr int kQWStW = kQWRows * kQWKB * 32;  // [2 halves][128 rows][2 blocks] x 16 B
static constexpr int kQWStD = 2 * kQWKB * 64 * 4;    // [2 blocks][64 row pairs] u32 scales + a dummy copy
static constexpr int kQWStX = kQWTok * kQWKB * 64;   // [128 tokens][8 x 16 B], swizzled
static constexpr int kQWStage = kQWStW + kQWStD + kQWStX;
static constexpr int kQWTileLd = kQWRows + 4;  // padded f32 row stride of the output tile
static constexpr int kQWMain = kQWStages * kQWStage > kQWTok * kQWTileLd * 4 ? kQWStages * kQWStage : kQWTok * kQWTileLd * 4;
static constexpr size_t kQWLds = kQWMain + 16 + (128 + 256) * 4;  // + flag + row scales / scratch

template <int EPI>
__global__ __launch_bounds__(kThreads) void gemmQ80wWideKernel(GemmArgs ga, int rowTiles, int tokTiles) {
    const GemvArgs &a = ga.e;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int *flag = reinterpret_cast<int *>(smem + kQWMain);
    float *rsL = reinterpret_cast<float *>(flag + 4);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int col = lane & 15, h = lane >> 4, wr = wave & 1, wt = wave >> 1;
    // XCD-aware order (gemm_wide.hip): logical tile Lg runs on XCD Lg / (G / 8)
    const int G = gridDim.x, id = blockIdx.x;
    const int Lg = (G & 7) == 0 ? (id & 7) * (G >> 3) + (id >> 3) : id;
    const int S = ga.splits, per = tokTiles * S;
    const int rt = Lg / per, rem = Lg - rt * per, tt = rem / S, sp = rem - tt * S;
    const int R0 = rt * kQWRows, T0 = tt * kQWTok;
    const int n = a.n, nb = n >> 5, L = a.lanes, lg = __builtin_ctz(L), K = (nb + L - 1) >> lg;
    const int bps = nb / S, j0 = sp * bps;  // bps and j0 even (launcher): j, j + 1 share a tiling step
    const uint32_t *wd2 = reinterpret_cast<const uint32_t *>(a.wd);

    // this thread's part of a stage's copies, as plane offsets at block 0: the int8 unit of row
    // 32 wave + lane / 2 (block parity below, half q), the scale word of row pair `lane`
    const int rlW = wave * 32 + (lane >> 1), kbW = (lane & 1) ^ ((rlW >> 3) & 1);
    const int rowW = min(R0 + rlW, a.rows - 1), rowD = min(R0 + 2 * lane, a.rows - 1);
    const uint8_t *qW = a.qs + q80Off(L, K, rowW, 0, 0);
    const uint32_t *dW = wd2 + q80ScaleOff(L, K, rowD, 0);
    auto issue = [&](int j, int b) {  // global -> LDS copies of blocks j, j + 1 into stage buffer b
        char *st = smem + b * kQWStage;
        const int jw = j + kbW, jd = j + (wave & 1);
        const size_t wo = (size_t)(jw >> lg) * 16384 + (size_t)(jw & (L - 1)) * 16;
#pragma unroll
        for (int q = 0; q < 2; q++) glds16(qW + wo + q * 4096, st + (wave + 4 * q) * 1024);
        // scales of block j + (wave & 1) (waves 2, 3 repeat into a dummy copy: one count for vmcnt)
        glds4(dW + (size_t)(jd >> lg) * kThreads + (jd & (L - 1)), st + kQWStW + wave * 256);
#pragma unroll
        for (int q = 0; q < 4; q++) {  // activations: 16 wave-instructions of 64 x 16 B
            const int k = wave + 4 * q, slot = k * 64 + lane, t = slot >> 3, u = (slot & 7) ^ ((t >> 1) & 7);
            glds16(ga.x + (size_t)(T0 + t) * n + (size_t)(j + (u >> 2)) * 32 + (u & 3) * 8,
                   st + kQWStW + kQWStD + k * 1024);
        }
    };

    f32x4 acc[4][4];
#pragma unroll
    for (int f = 0; f < 4; f++)
#pragma unroll
        for (int t = 0; t < 4; t++) acc[f][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    constexpr int PF = kQWStages - 1;
    const int nch = bps / kQWKB;
    for (int c = 0; c < PF && c < nch; c++) issue(j0 + kQWKB * c, c);
    for (int c = 0; c < nch; c++) {
        if (c + PF < nch) issue(j0 + kQWKB * (c + PF), (c + PF) % kQWStages);
        // chunk c landed for this thread (the younger chunks may stay in flight), then for all
        switch (min(nch - 1, c + PF) - c) {
            case 2: asm volatile("s_waitcnt vmcnt(%0)" ::"i"(2 * kQWNld) : "memory"); break;
            case 1: asm volatile("s_waitcnt vmcnt(%0)" ::"i"(kQWNld) : "memory"); break;
            default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
        }
        __builtin_amdgcn_s_barrier();
        const char *st = smem + (c % kQWStages) * kQWStage;
#pragma unroll
        for (int kb = 0; kb < kQWKB; kb++) {
            half8 av[4];
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const int tok = wt * 64 + t * 16 + col;
                av[t] = *reinterpret_cast<const half8 *>(st + kQWStW + kQWStD + (tok * 8 + ((kb * 4 + h) ^ ((tok >> 1) & 7))) * 16);
            }
#pragma unroll
            for (int f = 0; f < 4; f++) {
                const int rl = wr * 64 + f * 16 + col;
                // opaque addresses: single ds_read_b64 / _b32 (the 64-bank rule this image is
                // conflict-free for), not the fragments paired into ds_read2st64 (gemm_wide.hip)
                uint32_t aw = (uint32_t)((((h >> 1) * kQWRows + rl) * 2 + (kb ^ ((rl >> 3) & 1))) * 16 + (h & 1) * 8);
                uint32_t ad = (uint32_t)(kQWStW + (kb * 64 + (rl >> 1)) * 4);
                asm volatile("" : "+v"(aw), "+v"(ad));
                const u32x2 wv = *reinterpret_cast<const u32x2 *>(st + aw);
                const uint32_t d2 = *reinterpret_cast<const uint32_t *>(st + ad);
                const half8 b = q80ToF16x8(wv);
                const float dw = __half2float(__ushort_as_half((uint16_t)((rl & 1) ? d2 >> 16 : d2 & 0xFFFFu)));
                f32x4 s[4];
#pragma unroll
                for (int t = 0; t < 4; t++) s[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av[t], b, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
                for (int t = 0; t < 4; t++)
#pragma unroll
                    for (int i = 0; i < 4; i++) acc[f][t][i] = fmaf(dw, s[t][i], acc[f][t][i]);
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();  // stage c % kQWStages is refilled at iteration c + 1
    }

    // C layout: acc[f][t][i] = out[token 64 wt + 16 t + 4 h + i][row 64 wr + 16 f + col]
    float *tile = reinterpret_cast<float *>(smem);  // [128 tokens][kQWTileLd], the stages are free
    if (S == 1) {
#pragma unroll
        for (int f = 0; f < 4; f++)
#pragma unroll
            for (int t = 0; t < 4; t++)
#pragma unroll
                for (int i = 0; i < 4; i++)
                    tile[(wt * 64 + t * 16 + h * 4 + i) * kQWTileLd + wr * 64 + f * 16 + col] = acc[f][t][i];
    } else {
        const int lt = rt * tokTiles + tt;
        const size_t tileF = (size_t)kQWTok * kQWRows, stride = (size_t)rowTiles * tokTiles * tileF;
        float *part = ga.part + sp * stride + lt * tileF;
#pragma unroll
        for (int f = 0; f < 4; f++)
#pragma unroll
            for (int t = 0; t < 4; t++)
#pragma unroll
                for (int i = 0; i < 4; i++)
                    wtStore(part + (wt * 64 + t * 16 + h * 4 + i) * kQWRows + wr * 64 + f * 16 + col, acc[f][t][i]);
        if (!splitArrive(ga.counters + lt, S, flag)) return;
        splitCombine(ga.part + lt * tileF, stride, S, (int)(tileF / 4), reinterpret_cast<f32x4 *>(tile), kQWRows / 4,
                     kQWTileLd / 4);
    }
    __syncthreads();
    if (ga.ssIn) gemmRowScales(ga, T0, kQWTok, rsL, rsL + 128);
    gemmEpilogue<EPI, kQWRows / 2>(ga, tile, kQWTileLd, 0, min(kQWTok, ga.M - T0), T0, R0, rt * 2,
                                   ga.ssIn ? rsL : nullptr);
}

// preloadModules(): one kernel of this translation unit's code object
const void *gemmQ80wWideModuleKernel() { return (const void *)gemmQ80wWideKernel<EPI_STORE>; }

void launchGemmQ80wWide(const GemmArgs &ga, int epi, hipStream_t s) {
    const int rowTiles = (ga.e.rows + kQWRows - 1) / kQWRows, tokTiles = (ga.M + kQWTok - 1) / kQWTok, L = ga.e.lanes;
    if (L != 16 && L != 32 && L != 64) throw Error("launchGemmQ80wWide: lanes must be the tiling's 16, 32 or 64");
    if (ga.M < 1 || ga.e.rows < 1) throw Error("launchGemmQ80wWide: bad shape");
    if (!gemmWideAccepts(ga.e.n, ga.splits)) throw Error("launchGemmQ80wWide: bad K split (whole two-block stages per split)");
    if (ga.tpx) throw Error("launchGemmQ80wWide: no tile exchange");
    if (ga.splits > 1 && (!ga.part || !ga.counters)) throw Error("launchGemmQ80wWide: split-K without buffers");
    if (ga.splits > 1 && ga.partFloats && (size_t)ga.splits * rowTiles * tokTiles * kQWRows * kQWTok > ga.partFloats)
        throw Error("launchGemmQ80wWide: split-K partials exceed the engine's buffer");
    const dim3 grid(rowTiles * tokTiles * ga.splits);
#define DL_GEMMQW_CASE(E)                                                                                  \
    if (epi == E) {                                                                                        \
        allowLds((const void *)gemmQ80wWideKernel<E>, kQWLds);                                             \
        hipLaunchKernelGGL((gemmQ80wWideKernel<E>), grid, dim3(kThreads), kQWLds, s, ga, rowTiles, tokTiles); \
        return;                                                                                            \
    }
    DL_GEMMQW_CASE(EPI_STORE) DL_GEMMQW_CASE(EPI_ACT) DL_GEMMQW_CASE(EPI_QKV) DL_GEMMQW_CASE(EPI_ACT_F16)
    DL_GEMMQW_CASE(EPI_RES)
#undef DL_GEMMQW_CASE
    throw Error("launchGemmQ80wWide: unsupported epilogue");
}

}  // namespace hipk
}  // namespace dl
