// Batched (prefill / multi-user decode) matmuls on MFMA for gfx950: Q40 and F32 weights, the
// split-K combine and fused epilogues, and the residual + RMS norm -> f16 staging kernel.
#include "gemm_dev.h"

#include <cstdlib>

namespace dl {
namespace hipk {

// ------------------------------------------------------------------------------------------------
// Batched GEMM design notes (measured, profiles/r2_gemm_designs.md): two alternatives were built
// and measured slower than this kernel on every shape - (v2) weights HBM -> VGPR ring with the
// activations refilled through a 4-deep LDS ring (shared vmcnt capped the weight stream at 3 steps
// in flight), (v3) activations resident in LDS with a deep weight ring and 4 or 8 waves (1.4-1.7
// TB/s on w13, issue-stall bound per PMC: SQ_WAIT_INST_ANY 46 % of wave cycles). This v1 stays.
// Batched Q40 matmul on MFMA (prefill / multi-user decode, 2..32 tokens per launch).
//   out[t][row] = sum_k W[row][k] * x[t][k], W Q40 (the GEMV's tiled layout), x f16.
// Each workgroup owns 64 weight rows (4 waves x 16) and one K split, streamed in chunks of 16
// Q40 blocks. Both operands are copied HBM/L2 -> LDS with global_load_lds_dwordx4 (no VGPR
// staging; one 16-B unit per lane, contiguous 256-B+ runs per wave instruction), multi-buffered
// with counted vmcnt waits and raw barriers (kGemmStages buffers), into XOR-swizzled images so the fragment reads are
// bank-conflict free. Per block a lane dequantizes 8 nibbles of its row ((1024+q) - 1032 exact in
// f16, times d) into the B fragment of v_mfma_f32_16x16x32_f16; A fragments are read as is.
// Split-K partials are combined in split order by the last-arriving workgroup (agent-scope
// release/acquire counter: deterministic), which runs the fused epilogues (store / SwiGLU /
// SwiGLU -> f16 / SwiGLU -> Q80 / RoPE + KV append).
// ------------------------------------------------------------------------------------------------
static constexpr int kGemmCh = 8;  // Q40 blocks per pipeline stage (~25 KB at 32 tokens)

// Split-K degree: grow S until the grid reaches the workgroup target or a split would get fewer
// than kGemmCh blocks. The target is sized so every CU holds its 3 resident workgroups: with one
// chunk in flight per workgroup, bytes in flight per CU (and so HBM bandwidth) scale with
// resident workgroups, not with tiles (targets 128-1024 and 2-16 splits re-swept in round 3:
// profiles/raw/r3_gemm_knobs.md).
static int gemmEnvInt(const char *name, int dflt) {
    const char *e = std::getenv(name);
    return e && std::atoi(e) > 0 ? std::atoi(e) : dflt;
}
static int gemmWgTarget() { static const int v = gemmEnvInt("DL_GEMM_WG_TARGET", 256); return v; }
static int gemmMaxSplits() { static const int v = gemmEnvInt("DL_GEMM_MAX_SPLITS", 8); return v; }

GemmPlan gemmPlan(int rows, int n, int M) {
    GemmPlan p;
    p.rt = 1;
    p.tiles = (rows + kGemmRows - 1) / kGemmRows;
    p.splits = gemmSplits(rows, n, M);
    return p;
}

bool gemmSupported(int n) { return n % 32 == 0; }

// 16-lane tilings at <= 16 tokens run the 16-block-chunk kernel (gemmQ40L16Kernel): its splits
// keep every split a whole number of 16-block tiling steps. (At 32 tokens its 50 KB stages leave
// one workgroup per CU: w13 42.8 vs 32.5 us, so those stay on gemmQ40Kernel.)
static constexpr int kG16Ch = 16;
static bool gemmL16On() {
    static const bool v = [] {
        const char *e = std::getenv("DL_GEMM_L16");
        return !(e && *e == '0');
    }();
    return v;
}
// 64-row tiles per narrow workgroup by token tile width (gemmQ40Kernel RT; DL_GEMM_RT1/2/4)
static int gemmRowTiles(int M) {
    auto env = [](const char *name, int dflt) {
        const char *e = std::getenv(name);
        const int v = e ? std::atoi(e) : dflt;
        return v == 1 || v == 2 ? v : dflt;
    };
    static const int r1 = env("DL_GEMM_RT1", 1), r2 = env("DL_GEMM_RT2", 1), r4 = env("DL_GEMM_RT4", 1);
    const int MT = gemmTokenPad(M) / 16;
    return MT == 1 ? r1 : MT == 2 ? r2 : MT == 4 ? r4 : 1;
}
static bool gemmL16Eligible(int n, int M, int lanes) {
    return gemmL16On() && lanes == 16 && M <= 16 && (n / 32) % kG16Ch == 0 && !gemmUsesWide(M) && gemmRowTiles(M) == 1;
}

int gemmSplits(int rows, int n, int M, int lanes) {
    if (gemmUsesWide(M)) return gemmWideSplits(rows, n, M);
    const int tiles = (rows + kGemmRows - 1) / kGemmRows, nb = n / 32;
    if (gemmL16Eligible(n, M, lanes)) {
        const int ks = nb / kG16Ch;  // tiling steps
        int S = 1;
        const int target = gemmWgTarget(), maxS = gemmMaxSplits();
        while (2 * S <= maxS && tiles * S < target && ks % (2 * S) == 0) S *= 2;
        while (2 * S <= maxS && tiles * 2 * S <= 2 * target && ks % (2 * S) == 0 && ks / (2 * S) >= 4) S *= 2;
        return S;
    }
    const int target = gemmWgTarget(), maxS = gemmMaxSplits();
    const int wgs = (rows + kGemmRows * gemmRowTiles(M) - 1) / (kGemmRows * gemmRowTiles(M));
    int S = 1;
    while (2 * S <= maxS && wgs * S < target && nb % (2 * S) == 0 && nb / (2 * S) >= kGemmCh) S *= 2;
    // deep K (w2: 4096 x 14336): keep splitting up to two workgroups per CU while every split
    // still streams >= 4 chunks (measured w2 M=8 23.9 -> 19.6 us; shallower matrices lose)
    while (2 * S <= maxS && wgs * 2 * S <= 2 * target && nb % (2 * S) == 0 && nb / (2 * S) >= 4 * kGemmCh) S *= 2;
    return S;
}

int gemmTokenPad(int M) { return M <= 16 ? 16 : M <= 32 ? 32 : M <= 64 ? 64 : 128; }

size_t gemmPartFloats(int rows, int n, int maxTokens) {
    // narrow launches carry <= 128 tokens (the wide kernel takes the larger ones when enabled)
    const int mt = std::min(maxTokens, kGemmMaxTokens);
    const int tiles = (rows + kGemmRows - 1) / kGemmRows;
    size_t best = 0;
    for (int m = 16; m <= gemmTokenPad(mt); m *= 2) {
        if (gemmUsesWide(m)) break;
        const int S = std::max(gemmSplits(rows, n, m), gemmSplits(rows, n, m, 16));  // either kernel
        if (S > 1) best = std::max(best, (size_t)S * tiles * m * kGemmRows);
    }
    if (gemmUsesWide(maxTokens)) best = std::max(best, gemmWidePartFloats(rows, n, maxTokens));
    return best;
}

size_t gemmPartFloatsFixed(int rows, int n) {
    // batch-invariant engines: narrow launches of up to 128 tokens with the 16-token split count
    const int S = gemmSplits(rows, n, 16, 0), tiles = (rows + kGemmRows - 1) / kGemmRows;
    return S > 1 ? (size_t)S * tiles * kGemmMaxTokens * kGemmRows : 0;
}

int gemmCounterInts(int rows, int maxTokens) {
    const int narrow = (rows + kGemmRows - 1) / kGemmRows;
    return std::max(narrow, gemmUsesWide(maxTokens) ? gemmWideCounters(rows, maxTokens) : 0);
}

// stage layout (bytes): weights [64 RT rows][8 units] x 16 B | scales [32 RT pairs][8] u32 | x [MP][32 units] x 16 B
static constexpr int kStW = kGemmRows * kGemmCh * 16, kStD = (kGemmRows / 2) * kGemmCh * 4;
__host__ __device__ static constexpr int gemmStageBytes(int MT, int RT = 1) {
    return RT * (kStW + kStD) + MT * 16 * kGemmCh * 64;
}
#ifndef DL_GEMM_STAGES
#define DL_GEMM_STAGES 2  // 3 stages (2 WGs/CU) measured slower: batch-32 8.1k vs 8.8k tok/s
#endif
static constexpr int kGemmStages = DL_GEMM_STAGES;  // stage buffers (kGemmStages-1 chunks in flight)
static constexpr int kGemmScaleFloats = 128 + 256;  // gemmFinish: per-token RMS scales + per-thread slices
static size_t gemmLds(int MT, int stages, int RT = 1) {
    return stages * (size_t)gemmStageBytes(MT, RT) + 16 + kGemmScaleFloats * 4;  // + flag
}

// STG = stage buffers: 2 double-buffers the chunk stream inside a workgroup; 1 (the 64-token
// tile) drops that to fit 3 workgroups per CU, which then overlap each other's loads.
// RT = 64-row tiles per workgroup (each wave owns 16 rows of every tile): one activation stage
// then feeds RT x 64 rows. At 64 tokens a 64-row tile stages 32 KB of activations per 9 KB of
// weights (PMC: waves wait 47 % of their cycles on those stages), so RT = 2 halves the bytes a
// workgroup moves per weight byte; the A fragments read from LDS are shared by the RT tiles too.
template <int MT, int EPI, int STG, int RT = 1>
__global__ __launch_bounds__(kThreads) void gemmQ40Kernel(GemmArgs ga) {
    const GemvArgs &a = ga.e;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int SB = gemmStageBytes(MT, RT);
    constexpr int SW = RT * kStW, SD = RT * kStD;  // weight / scale bytes of a stage
    constexpr int NW = RT * kGemmRows * kGemmCh / kThreads, NX = MT * 16 * kGemmCh * 4 / kThreads;
    constexpr int NLD = NW + RT + NX;  // glds instructions per thread per stage
    int *flag = reinterpret_cast<int *>(smem + STG * SB);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int col = lane & 15, h = lane >> 4;
    const int n = a.n, nb = n >> 5, L = a.lanes, NG = kThreads / L, KS = (nb + L - 1) / L;
    const int lgL = 31 - __builtin_clz(L);
    const int sp = blockIdx.y, S = ga.splits;
    const int R0 = blockIdx.x * kGemmRows * RT;
    const int bps = nb / S, j0 = sp * bps, j1 = j0 + bps;
    const int nch = (bps + kGemmCh - 1) / kGemmCh;
    const uint8_t *qs = a.qs;
    const uint32_t *wd2 = reinterpret_cast<const uint32_t *>(a.wd);
    auto unitOf = [&](int row, int j) -> size_t {  // tiled 16-B unit of (row, block j), clamped
        row = min(row, a.rows - 1);
        j = min(j, j1 - 1);
        const int g = row / (2 * NG), rem = row % (2 * NG), gi = rem >> 1, rpar = rem & 1;
        const int k = j >> lgL, li = j & (L - 1);
        return (((size_t)g * KS + k) * 2 + rpar) * kThreads + gi * L + li;
    };
    auto scaleIdx = [&](int pairRow, int j) -> size_t {  // tiled u32 pair scale of (row pair, block j)
        const int row = min(pairRow, a.rows - 1);
        j = min(j, j1 - 1);
        const int g = row / (2 * NG), rem = row % (2 * NG), gi = rem >> 1;
        const int k = j >> lgL, li = j & (L - 1);
        return ((size_t)g * KS + k) * kThreads + gi * L + li;
    };
    // issue the copies of chunk c into stage buffer b
    auto issue = [&](int c, int b) {
        char *st = smem + b * SB;
        const int c0 = j0 + c * kGemmCh;
        // weights: unit u = s*256 + tid -> (row_l = u/8, position p = u%8) holds block p ^ ((row_l>>1)&7)
#pragma unroll
        for (int s = 0; s < NW; s++) {
            const int u = s * kThreads + tid, rl = u / kGemmCh, pp = u % kGemmCh;
            const size_t unit = unitOf(R0 + rl, c0 + (pp ^ ((rl >> 1) & (kGemmCh - 1))));
            glds16<true>(qs + unit * 16, st + (size_t)(s * kThreads + wave * 64) * 16);
        }
        // pair scales: u = d*256 + tid -> (pair_l = u/8, block u%8), 4 B each
#pragma unroll
        for (int d = 0; d < RT; d++) {
            const int u = d * kThreads + tid, pl = u / kGemmCh, jj = u % kGemmCh;
            glds4(wd2 + scaleIdx(R0 + 2 * pl, c0 + jj), st + SW + (size_t)(d * kThreads + wave * 64) * 4);
        }
        // activations: token row t = 4*kGemmCh units of 8 f16; position p holds unit p ^ (t&15)
#pragma unroll
        for (int s = 0; s < NX; s++) {
            const int u = s * kThreads + tid, t = u / (4 * kGemmCh), pp = u % (4 * kGemmCh);
            const int uu = pp ^ (t & 15);
            const int cb = min(c0 + (uu >> 2), j1 - 1);  // block of this unit (clamped)
            const _Float16 *src = ga.x + (size_t)t * n + (size_t)cb * 32 + (uu & 3) * 8;
            glds16(src, st + SW + SD + (size_t)(s * kThreads + wave * 64) * 16);
        }
    };

    const unsigned long long tEntry = a.trace ? wall_clock64() : 0ull;
    unsigned long long tFirst = 0ull;
    f32x4 acc[RT][MT];
#pragma unroll
    for (int r = 0; r < RT; r++)
#pragma unroll
        for (int t = 0; t < MT; t++) acc[r][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int byteHalf = h & 1, nibHi = h >> 1;

    constexpr int PF = STG - 1;  // chunks in flight ahead of the one consumed
    for (int c = 0; c < PF && c < nch; c++) issue(c, c);
    for (int c = 0; c < nch; c++) {
        if (c + PF < nch) issue(c + PF, (c + PF) % STG);
        // wait until chunk c landed (this thread): the chunks issued after it may stay in flight
        const int after = min(nch - 1, c + PF) - c;
        if (after >= 3)
            asm volatile("s_waitcnt vmcnt(%0)" ::"i"(3 * NLD) : "memory");
        else if (after == 2)
            asm volatile("s_waitcnt vmcnt(%0)" ::"i"(2 * NLD) : "memory");
        else if (after == 1)
            asm volatile("s_waitcnt vmcnt(%0)" ::"i"(NLD) : "memory");
        else
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();  // ... and for every thread
        if (a.trace && c == 0) tFirst = wall_clock64();
        const char *st = smem + (c % STG) * SB;
        const int cn = min(kGemmCh, bps - c * kGemmCh);
        // Software-pipelined over the chunk's blocks: block jj + 1's LDS operands (weights, scale,
        // activation fragments) are read before block jj is dequantized and fed to the MFMAs, so
        // each block waits on a counted lgkmcnt instead of a full LDS round trip + the dequant
        // chain (the serial form spent 38 % of its wave cycles waiting, PMC r5).
        struct Ops {
            u32x2 wv[RT];
            uint32_t dh[RT];
            half8 av[MT];
        };
        auto ldOps = [&](int jj, Ops &o) {
#pragma unroll
            for (int r = 0; r < RT; r++) {
                const int rl = r * kGemmRows + wave * 16 + col;  // this lane's weight row in tile r (local)
                // swizzle key (rl >> 1) & 7: the 16 rows of a wave's ds_read_b64 (two 8-B halves per
                // 16-B unit) land on 32 distinct bank pairs (rows 128 B apart alias every other row;
                // the old key rl & 7 left 2-way conflicts: SQ_LDS_BANK_CONFLICT 25 % of LDS cycles)
                const int pp = jj ^ ((rl >> 1) & (kGemmCh - 1));
                o.wv[r] = *reinterpret_cast<const u32x2 *>(st + (size_t)(rl * kGemmCh + pp) * 16 + byteHalf * 8);
                // this row's f16 half of the pair scale, read directly (no per-lane shift)
                o.dh[r] = *reinterpret_cast<const uint16_t *>(st + SW + (size_t)((rl >> 1) * kGemmCh + jj) * 4 + (rl & 1) * 2);
            }
#pragma unroll
            for (int t = 0; t < MT; t++) {
                const int tok = t * 16 + col, up = (jj * 4 + h) ^ (tok & 15);
                o.av[t] = *reinterpret_cast<const half8 *>(st + SW + SD + (size_t)(tok * 4 * kGemmCh + up) * 16);
            }
        };
        Ops ops[2];
        ldOps(0, ops[0]);
#pragma unroll
        for (int jj = 0; jj < kGemmCh; jj++) {
            Ops &cur = ops[jj & 1];
            if (jj + 1 < kGemmCh) ldOps(jj + 1, ops[(jj + 1) & 1]);
            half8 b[RT];
#pragma unroll
            for (int r = 0; r < RT; r++) b[r] = dequantQ40x8(cur.wv[r], nibHi, jj < cn ? cur.dh[r] : 0u);
#pragma unroll
            for (int t = 0; t < MT; t++)
#pragma unroll
                for (int r = 0; r < RT; r++)
                    acc[r][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(cur.av[t], b[r], acc[r][t], 0, 0, 0);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();  // stage c % STG is refilled at iteration c + 1
    }

    const unsigned long long tLoop = a.trace ? wall_clock64() : 0ull;
    const int tiles = (a.rows + kGemmRows - 1) / kGemmRows;
#pragma unroll
    for (int r = 0; r < RT; r++) {  // one 64-row tile at a time through the split-K combine + epilogue
        const int tileIdx = blockIdx.x * RT + r;
        if (tileIdx >= tiles) break;
        if (r) __syncthreads();  // the previous tile's epilogue read the LDS tile
        gemmFinish<MT, EPI>(ga, acc[r], smem, flag, tileIdx, tiles, tEntry, tFirst, tLoop);
    }
}

// 16-lane tilings (Q40Tiling L = 16: qkv / w13 / logits of 8B, every layer matrix of 70B and
// 405B) at <= 16 tokens. A chunk is 16 blocks = one step k of the tiling, so each wave instruction
// of the weight DMA reads one contiguous 1 KB of the tiled matrix (4 row pairs x 16 blocks of one
// (group, step, row parity)); the 8-block chunks of gemmQ40Kernel read 128-B runs 256 B apart, and
// HBM served those at ~2.4 TB/s (w13 at 8 tokens, bench_gemm.py). The LDS weight image keeps the
// global order of each 1-KB piece with the block slot XOR-swizzled by ((pair & 7) * 2 + parity):
// a wave's 16 rows read one block at 16 distinct 16-B columns (conflict-free ds_read_b64). Scales
// are staged in global order ([group][pair][block] u32 pairs), activations as in gemmQ40Kernel
// (64 units of 8 f16 per token row, unit u of token t at u ^ (t & 15)).
static constexpr int kG16W = kGemmRows * kG16Ch * 16, kG16D = (kGemmRows / 2) * kG16Ch * 4;
__host__ __device__ static constexpr int gemm16StageBytes(int MT) { return kG16W + kG16D + MT * 16 * kG16Ch * 64; }
__device__ __forceinline__ int g16Swz(int pair, int rpar) { return ((pair & 7) * 2 + rpar) & 15; }

template <int MT, int EPI, int STG>
__global__ __launch_bounds__(kThreads) void gemmQ40L16Kernel(GemmArgs ga) {
    const GemvArgs &a = ga.e;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int SB = gemm16StageBytes(MT);
    constexpr int NW = kG16W / 16 / kThreads, ND = kG16D / 4 / kThreads, NX = MT * 16 * kG16Ch * 4 / kThreads;
    constexpr int NLD = NW + ND + NX;  // DMA instructions per thread per stage
    int *flag = reinterpret_cast<int *>(smem + STG * SB);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int col = lane & 15, h = lane >> 4;
    const int n = a.n, nb = n >> 5, KS = nb / kG16Ch;
    const int tileIdx = blockIdx.x, sp = blockIdx.y, S = ga.splits;
    const int R0 = tileIdx * kGemmRows, g0 = R0 / 32;  // first 32-row group of the tile
    const int bps = nb / S, j0 = sp * bps;
    const int nch = bps / kG16Ch;
    const uint8_t *qs = a.qs;
    const uint32_t *wd2 = reinterpret_cast<const uint32_t *>(a.wd);
    const int lastRow = a.rows - 1;
    // issue the copies of chunk c (tiling step k0 + c) into stage buffer b
    auto issue = [&](int c, int b) {
        char *st = smem + b * SB;
        const int k = j0 / kG16Ch + c;
#pragma unroll
        for (int s = 0; s < NW; s++) {  // piece = (group, parity, 4-pair block), lane = (pair, slot)
            const int piece = s * 4 + wave, gl = piece >> 3, rpar = (piece >> 2) & 1, gi = (piece & 3) * 4 + (lane >> 4);
            const int li = (lane & 15) ^ g16Swz(gi, rpar);
            int row = R0 + gl * 32 + gi * 2 + rpar;
            size_t unit;
            if (row <= lastRow) {
                unit = (((size_t)(g0 + gl) * KS + k) * 2 + rpar) * kThreads + gi * 16 + li;
            } else {  // past the matrix: the last row's unit (outputs dropped)
                row = lastRow;
                unit = (((size_t)(row / 32) * KS + k) * 2 + (row & 1)) * kThreads + ((row % 32) >> 1) * 16 + li;
            }
            glds16<true>(qs + unit * 16, st + (size_t)piece * 1024);
        }
#pragma unroll
        for (int s = 0; s < ND; s++) {  // pair scales in global order: [group][pair][block]
            const int u = s * kThreads + tid, gl = u >> 8;
            const int gg = min(g0 + gl, lastRow / 32);
            glds4(wd2 + ((size_t)gg * KS + k) * kThreads + (u & 255), st + kG16W + (size_t)(s * kThreads + wave * 64) * 4);
        }
#pragma unroll
        for (int s = 0; s < NX; s++) {  // activations: one token row (64 units) per wave instruction
            const int u = s * kThreads + tid, t = u >> 6, pp = u & 63, uu = pp ^ (t & 15);
            const _Float16 *src = ga.x + (size_t)t * n + (size_t)(k * kG16Ch + (uu >> 2)) * 32 + (uu & 3) * 8;
            glds16(src, st + kG16W + kG16D + (size_t)(s * kThreads + wave * 64) * 16);
        }
    };

    const unsigned long long tEntry = a.trace ? wall_clock64() : 0ull;
    unsigned long long tFirst = 0ull;
    f32x4 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; t++) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int rl = wave * 16 + col;  // this lane's weight row (local)
    const int byteHalf = h & 1, nibHi = h >> 1;
    const int gl = rl >> 5, rpar = rl & 1, gi = (rl >> 1) & 15;
    const int wBase = (((gl * 2 + rpar) * 4 + (gi >> 2)) * 64 + (gi & 3) * 16) * 16 + byteHalf * 8;
    const int swz = g16Swz(gi, rpar);
    const int dBase = (gl * 256 + gi * 16) * 4 + rpar * 2;  // this row's f16 half of the pair scale

    constexpr int PF = STG - 1;  // chunks in flight ahead of the one consumed
    for (int c = 0; c < PF && c < nch; c++) issue(c, c);
    for (int c = 0; c < nch; c++) {
        if (c + PF < nch) issue(c + PF, (c + PF) % STG);
        const int after = min(nch - 1, c + PF) - c;  // chunks issued after c, still in flight
        if (after >= 2)
            asm volatile("s_waitcnt vmcnt(%0)" ::"i"(2 * NLD) : "memory");
        else if (after == 1)
            asm volatile("s_waitcnt vmcnt(%0)" ::"i"(NLD) : "memory");
        else
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();  // ... and for every thread
        if (a.trace && c == 0) tFirst = wall_clock64();
        const char *st = smem + (c % STG) * SB;
        // software-pipelined as gemmQ40Kernel: block jj + 1's LDS operands are read before block jj
        // is dequantized
        struct Ops {
            u32x2 wv;
            uint32_t d16;
            half8 av[MT];
        };
        auto ldOps = [&](int jj, Ops &o) {
            o.wv = *reinterpret_cast<const u32x2 *>(st + wBase + (jj ^ swz) * 16);
            o.d16 = *reinterpret_cast<const uint16_t *>(st + kG16W + dBase + jj * 4);
#pragma unroll
            for (int t = 0; t < MT; t++) {
                const int tok = t * 16 + col, up = (jj * 4 + h) ^ (tok & 15);
                o.av[t] = *reinterpret_cast<const half8 *>(st + kG16W + kG16D + (size_t)(tok * 64 + up) * 16);
            }
        };
        Ops ops[2];
        ldOps(0, ops[0]);
#pragma unroll
        for (int jj = 0; jj < kG16Ch; jj++) {
            Ops &cur = ops[jj & 1];
            if (jj + 1 < kG16Ch) ldOps(jj + 1, ops[(jj + 1) & 1]);
            const half8 b = dequantQ40x8(cur.wv, nibHi, cur.d16);
#pragma unroll
            for (int t = 0; t < MT; t++) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(cur.av[t], b, acc[t], 0, 0, 0);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();  // stage c % STG is refilled at iteration c + 1
    }

    gemmFinish<MT, EPI>(ga, acc, smem, flag, blockIdx.x, gridDim.x, tEntry, tFirst, a.trace ? wall_clock64() : 0ull);
}

// The 128-token tile (prefill chunks): one stage buffer (73 KB), two workgroups per CU; each
// weight chunk feeds 8 MFMA token tiles, so a 128-token slice streams the weights once instead of
// twice.
// stage buffers per token-tile width (re-swept in round 3: profiles/raw/r3_gemm_knobs.md)
static int envStages(const char *name, int dflt) {
    const char *e = std::getenv(name);
    const int v = e ? std::atoi(e) : dflt;
    return v >= 1 && v <= 4 ? v : dflt;
}
static int gemmStages4() { static const int v = envStages("DL_GEMM_STG4", 1); return v; }
static int gemmStages2() { static const int v = envStages("DL_GEMM_STG2", kGemmStages); return v; }
static int gemmStages1() { static const int v = envStages("DL_GEMM_STG1", kGemmStages); return v; }

bool gemmTpxFits(int M, int world, bool q80) {
    if (M < 1 || M > 64 || world > kTpMaxRanks) return false;
    const int MT = gemmTokenPad(M) / 16;
    const int stg = MT == 4 ? gemmStages4() : MT == 2 ? gemmStages2() : gemmStages1();
    const size_t need = (size_t)MT * 16 * kGemmRows * 4 + (q80 ? tpTileQ80Lds(M, world) : 0);
    return need <= (size_t)stg * gemmStageBytes(MT, gemmRowTiles(M));
}

GemmKernel gemmKernelFor(int n, int M, int lanes, int splits, bool fixed) {
    if (fixed) return GEMM_NARROW;
    if (gemmUsesWide(M)) return GEMM_WIDE;
    return gemmL16Eligible(n, M, lanes) && splits > 0 && (n / 32 / kG16Ch) % splits == 0 ? GEMM_L16 : GEMM_NARROW;
}

int gemmChunkTokens(int n, int M, bool q40, bool fixed) {
    if (!q40) return kGemmF32MaxTokens;
    if (!gemmUsesWide(M) || fixed) return kGemmMaxTokens;
    return gemmWideAccepts(n, 1) ? M : std::min(kGemmMaxTokens, gemmWideMin() - 1);
}

void launchGemmQ40(const GemmArgs &ga, int epi, hipStream_t s) {
    const GemmKernel kernel = gemmKernelFor(ga.e.n, ga.M, ga.e.lanes, ga.splits, ga.fixed != 0);
    if (kernel == GEMM_WIDE) {
        launchGemmWide(ga, epi, s);
        return;
    }
    if (ga.M > kGemmMaxTokens) throw Error("launchGemmQ40: more than 128 tokens per narrow launch");
    if (ga.splits > 1 && ga.partFloats &&
        (size_t)ga.splits * ((ga.e.rows + kGemmRows - 1) / kGemmRows) * gemmTokenPad(ga.M) * kGemmRows > ga.partFloats)
        throw Error("launchGemmQ40: split-K partials exceed the engine's buffer");
    if (ga.tpx && !gemmTpxFits(ga.M, ga.e.tp.world, ga.e.tp.q80 != 0))
        throw Error("launchGemmQ40: the tile exchange does not fit this launch's LDS");
    const int tiles = (ga.e.rows + kGemmRows - 1) / kGemmRows;
    const int MT = gemmTokenPad(ga.M) / 16;
    const dim3 grid(tiles, ga.splits);
    if (kernel == GEMM_L16) {
        const size_t lds = 2 * (size_t)gemm16StageBytes(MT) + 16 + kGemmScaleFloats * 4;
#define DL_G16_CASE(M_, E)                                                                         \
    if (MT == M_ && epi == E) {                                                                    \
        if (lds > 65536) allowLds((const void *)gemmQ40L16Kernel<M_, E, 2>, lds);                  \
        hipLaunchKernelGGL((gemmQ40L16Kernel<M_, E, 2>), grid, dim3(kThreads), lds, s, ga);        \
        return;                                                                                    \
    }
#define DL_G16_CASES(M_)                                                                           \
    DL_G16_CASE(M_, EPI_STORE) DL_G16_CASE(M_, EPI_ACT) DL_G16_CASE(M_, EPI_ACT_Q80)               \
    DL_G16_CASE(M_, EPI_QKV) DL_G16_CASE(M_, EPI_ACT_F16) DL_G16_CASE(M_, EPI_RES)
        DL_G16_CASES(1)
#undef DL_G16_CASES
#undef DL_G16_CASE
    }
    const int stg = MT == 8 ? 1 : MT == 4 ? gemmStages4() : MT == 2 ? gemmStages2() : gemmStages1();
    const int RT = MT == 8 || ga.fixed ? 1 : gemmRowTiles(ga.M);
    const size_t lds = gemmLds(MT, stg, RT);
    const dim3 gridRt((ga.e.rows + kGemmRows * RT - 1) / (kGemmRows * RT), ga.splits);
#define DL_GEMM_CASE(M_, E, G, R)                                                                     \
    if (MT == M_ && epi == E && stg == G && RT == R) {                                                \
        if (lds > 65536) allowLds((const void *)gemmQ40Kernel<M_, E, G, R>, lds); /* per device */   \
        hipLaunchKernelGGL((gemmQ40Kernel<M_, E, G, R>), gridRt, dim3(kThreads), lds, s, ga);        \
        return;                                                                                       \
    }
#define DL_GEMM_CASES(M_, G, R)                                                                         \
    DL_GEMM_CASE(M_, EPI_STORE, G, R) DL_GEMM_CASE(M_, EPI_ACT, G, R) DL_GEMM_CASE(M_, EPI_ACT_Q80, G, R) \
    DL_GEMM_CASE(M_, EPI_QKV, G, R) DL_GEMM_CASE(M_, EPI_ACT_F16, G, R) DL_GEMM_CASE(M_, EPI_RES, G, R)
    DL_GEMM_CASES(1, kGemmStages, 1) DL_GEMM_CASES(1, 3, 1) DL_GEMM_CASES(1, 4, 1) DL_GEMM_CASES(2, kGemmStages, 1)
    DL_GEMM_CASES(2, 1, 1) DL_GEMM_CASES(2, 3, 1) DL_GEMM_CASES(2, 4, 1) DL_GEMM_CASES(4, 1, 1) DL_GEMM_CASES(4, 2, 1)
    DL_GEMM_CASES(4, 3, 1) DL_GEMM_CASES(8, 1, 1)
    DL_GEMM_CASES(1, kGemmStages, 2) DL_GEMM_CASES(2, kGemmStages, 2) DL_GEMM_CASES(4, 1, 2)
#undef DL_GEMM_CASES
#undef DL_GEMM_CASE
    throw Error("launchGemmQ40: no narrow kernel instance for this stage / row-tile choice");
}

// Batched matmul for F32 weights on MFMA (the reference runs F32 batches through
// llamafile_sgemm, nn-cpu-ops.cpp:1018-1037): out[t][row] = sum_k W[row][k] x[t][k], W f32
// row-major [rows][n] (exact: v_mfma_f32_16x16x4_f32), x f16 as on the Q40 path (the only
// rounding). A wave owns 16 rows; per 32-k step lane (col, h) streams 32 B of its row col
// (k = 8h .. 8h+7: 4 lanes cover a 128-B line) straight into VGPRs - no LDS for the weights,
// which are read once - and the matching 16 B of f16 activations per token tile (L2-resident,
// shared by the workgroup's waves). Element e of those 8 feeds MFMA e on both operands (k = 8h+e,
// a permutation of k). 4 steps are issued per iteration so 4 x 32 B per lane stay in flight.
// Split-K, the deterministic combine and the fused epilogues are the Q40 GEMM's (gemmFinish).
template <int MT, int EPI>
__global__ __launch_bounds__(kThreads) void gemmF32Kernel(GemmArgs ga) {
    const GemvArgs &a = ga.e;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int *flag = reinterpret_cast<int *>(smem + MT * 16 * kGemmRows * 4);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 15, h = lane >> 4;
    const int n = a.n, kps = n / ga.splits, k0 = blockIdx.y * kps;
    const int row = min(blockIdx.x * kGemmRows + wave * 16 + col, a.rows - 1);  // clamped: outputs dropped
    const float *wp = a.wf + (size_t)row * n + k0 + 8 * h;
    const _Float16 *xp = ga.x + (size_t)col * n + k0 + 8 * h;
    f32x4 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; t++) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    constexpr int U = 4;
    int k = 0;
    for (; k + 32 * U <= kps; k += 32 * U) {
        f32x4 w[U][2];
        half8 xv[U][MT];
#pragma unroll
        for (int u = 0; u < U; u++) {
            w[u][0] = *reinterpret_cast<const f32x4 *>(wp + k + 32 * u);
            w[u][1] = *reinterpret_cast<const f32x4 *>(wp + k + 32 * u + 4);
#pragma unroll
            for (int t = 0; t < MT; t++) xv[u][t] = *reinterpret_cast<const half8 *>(xp + (size_t)t * 16 * n + k + 32 * u);
        }
#pragma unroll
        for (int u = 0; u < U; u++)
#pragma unroll
            for (int e = 0; e < 8; e++)
#pragma unroll
                for (int t = 0; t < MT; t++)
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32((float)xv[u][t][e], w[u][e >> 2][e & 3], acc[t], 0, 0, 0);
    }
    for (; k < kps; k += 32) {  // remainder steps (kps is a multiple of 32)
        const f32x4 w0 = *reinterpret_cast<const f32x4 *>(wp + k), w1 = *reinterpret_cast<const f32x4 *>(wp + k + 4);
#pragma unroll
        for (int t = 0; t < MT; t++) {
            const half8 xv = *reinterpret_cast<const half8 *>(xp + (size_t)t * 16 * n + k);
#pragma unroll
            for (int e = 0; e < 8; e++)
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32((float)xv[e], e < 4 ? w0[e] : w1[e - 4], acc[t], 0, 0, 0);
        }
    }
    gemmFinish<MT, EPI>(ga, acc, smem, flag, blockIdx.x, gridDim.x);
}

void launchGemmF32(const GemmArgs &ga, int epi, hipStream_t s) {
    const int tiles = (ga.e.rows + kGemmRows - 1) / kGemmRows;
    if (ga.M > kGemmF32MaxTokens) throw Error("launchGemmF32: more than 64 tokens per launch");
    if (ga.splits > 1 && ga.partFloats && (size_t)ga.splits * tiles * gemmTokenPad(ga.M) * kGemmRows > ga.partFloats)
        throw Error("launchGemmF32: split-K partials exceed the engine's buffer");
    const int MT = gemmTokenPad(ga.M) / 16;
    const dim3 grid(tiles, ga.splits);
    const size_t lds = (size_t)MT * 16 * kGemmRows * 4 + 16 + kGemmScaleFloats * 4;  // + flag, row scales
#define DL_GEMMF_CASE(M_, E)                                                              \
    if (MT == M_ && epi == E) {                                                           \
        if (lds > 65536) allowLds((const void *)gemmF32Kernel<M_, E>, lds);               \
        hipLaunchKernelGGL((gemmF32Kernel<M_, E>), grid, dim3(kThreads), lds, s, ga);     \
        return;                                                                           \
    }
#define DL_GEMMF_CASES(M_)                                                                \
    DL_GEMMF_CASE(M_, EPI_STORE) DL_GEMMF_CASE(M_, EPI_ACT) DL_GEMMF_CASE(M_, EPI_QKV)    \
    DL_GEMMF_CASE(M_, EPI_ACT_F16) DL_GEMMF_CASE(M_, EPI_RES)
    DL_GEMMF_CASES(1) DL_GEMMF_CASES(2) DL_GEMMF_CASES(4)
#undef DL_GEMMF_CASES
#undef DL_GEMMF_CASE
    throw Error("launchGemmF32: unsupported epilogue");
}

// Residual add + RMS norm (optional) of M rows -> f16 (one workgroup per row): the batched
// path's replacement for the GEMV's per-workgroup norm prologue.
__global__ __launch_bounds__(kThreads) void normF16Kernel(GemvArgs a, _Float16 *out) {
    __shared__ float scratch[64];
    constexpr int PV = 8;  // float4 per thread kept in registers (n <= 8192 in one pass)
    const int b = blockIdx.x, n = a.n, tid = threadIdx.x;
    const float *x = a.in + (size_t)b * a.ldIn;
    const float *y = a.addIn ? a.addIn + (size_t)b * a.ldIn : nullptr;
    float *xo = a.xNext ? a.xNext + (size_t)b * a.ldIn : nullptr;
    _Float16 *o = out + (size_t)b * n;
    const bool inReg = n <= kThreads * 4 * PV;
    float4 v[PV], gw[PV];
    float ss = 0.f;
    if (inReg) {
        // every load (x, the residual delta and the norm weights) is issued before any is used:
        // one memory round trip before the reduction instead of three
        float4 w[PV];
#pragma unroll
        for (int k = 0; k < PV; k++) {
            const int i = min((tid + k * kThreads) * 4, n - 4);
            v[k] = ld4(x + i);
            w[k] = y ? ld4(y + i) : make_float4(0.f, 0.f, 0.f, 0.f);
            gw[k] = a.normW ? ld4(a.normW + i) : make_float4(1.f, 1.f, 1.f, 1.f);
        }
#pragma unroll
        for (int k = 0; k < PV; k++) {
            const int i = (tid + k * kThreads) * 4;
            if (i < n) {
                v[k].x += w[k].x; v[k].y += w[k].y; v[k].z += w[k].z; v[k].w += w[k].w;
                if (xo) st4(xo + i, v[k]);
                ss += v[k].x * v[k].x + v[k].y * v[k].y + v[k].z * v[k].z + v[k].w * v[k].w;
            }
        }
    } else {
        for (int i = tid * 4; i < n; i += kThreads * 4) {
            float4 u = ld4(x + i);
            if (y) {
                const float4 w = ld4(y + i);
                u.x += w.x; u.y += w.y; u.z += w.z; u.w += w.w;
            }
            if (xo) st4(xo + i, u);
            ss += u.x * u.x + u.y * u.y + u.z * u.z + u.w * u.w;
        }
    }
    float inv = 1.0f;
    if (a.normW) {
        ss = blockSum<kThreads>(ss, scratch);
        inv = 1.0f / sqrtf(ss / (float)n + a.eps);
    }
    auto emit = [&](int i, float4 u, const float4 *gp) {
        const float4 g = gp ? *gp : (a.normW ? ld4(a.normW + i) : make_float4(1.f, 1.f, 1.f, 1.f));
        typedef _Float16 h4 __attribute__((ext_vector_type(4)));
        const h4 r = {(_Float16)(g.x * (inv * u.x)), (_Float16)(g.y * (inv * u.y)), (_Float16)(g.z * (inv * u.z)),
                      (_Float16)(g.w * (inv * u.w))};
        *reinterpret_cast<h4 *>(o + i) = r;
    };
    if (inReg) {
#pragma unroll
        for (int k = 0; k < PV; k++) {
            const int i = (tid + k * kThreads) * 4;
            if (i < n) emit(i, v[k], &gw[k]);
        }
    } else {
        for (int i = tid * 4; i < n; i += kThreads * 4) {
            float4 u = xo ? ld4(xo + i) : ld4(x + i);
            if (!xo && y) {
                const float4 w = ld4(y + i);
                u.x += w.x; u.y += w.y; u.z += w.z; u.w += w.w;
            }
            emit(i, u, nullptr);
        }
    }
}

// preloadModules(): one kernel of this translation unit's code object
const void *gemmModuleKernel() { return (const void *)normF16Kernel; }

void launchNormF16(const GemvArgs &a, _Float16 *out, int M, hipStream_t s) {
    hipLaunchKernelGGL(normF16Kernel, dim3(M), dim3(kThreads), 0, s, a, out);
}

}  // namespace hipk
}  // namespace dl
