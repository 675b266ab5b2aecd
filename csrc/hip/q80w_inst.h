// Decode GEMV on Q80 weights (gemvQ80wKernel) and its per-(batch, prologue, epilogue) instance
// table, compiled once per lanes-per-row L in q80w_l16/32/64.hip (parallel builds).
//
// Work split: the Q40 ring GEMV's (Q80Tiling, kernels.h): a lane group of L lanes owns row pairs,
// lane li walks blocks j = li, li + L, ... of both rows for every pass of the workgroup as one flat
// sequence of T = passes * K steps, each step one contiguous 16 KB + 1 KB region of the tiled
// planes per workgroup. A step is 2 rows x 32 B (four 16-byte non-temporal loads) and one 32-bit
// scale pair per lane; two groups of kQ80wDepth steps alternate in registers, the next group's loads
// issued before the current one is consumed, so 2 * 132 * kQ80wDepth bytes per lane are in flight
// while a group computes (loads scheduled by the compiler: no register is live in an inline-asm
// wait, so none of the ring's register rules apply). Activations are Q80 blocks in LDS, read once
// per block and shared by the two rows; the block dot is 8 v_dot4_i32_i8 per row into an exact
// int32, scaled by f32(dw) * dx into an f32 accumulator per (row, batch row).
#pragma once
#include "decode_dev.h"

namespace dl {
namespace hipk {

// 2: 8B wcls / w13 / wo at their default lanes 82.1 / 21.0 / 5.4 us; 1: 83.0 / 21.1 / 5.4; 3: 82.3 / 22.3 /
// 5.9; 4: 82.6 / 22.1 / 7.0 (profiles/q80_weights.md)
#ifndef DL_Q80W_DEPTH
#define DL_Q80W_DEPTH 2
#endif
static constexpr int kQ80wDepth = DL_Q80W_DEPTH;  // steps per register group (two groups alternate)

struct Q80wStep {
    u32x4 w[2][2];  // [row of the pair][half of the block]
    uint32_t d;     // the pair's f16 scales
};

// One Q80 weight block of 2 rows against B activation blocks (loaded once, shared by the rows).
template <int B>
__device__ __forceinline__ void q80wBlock(float (&acc)[2][B], const Q80wStep &s, const float (&dw)[2], int j, int n,
                                          int nb, const int8_t *act, const float2 *asc) {
#pragma unroll
    for (int b = 0; b < B; b++) {
        const int4 *xp = reinterpret_cast<const int4 *>(act + (size_t)b * n + j * 32);
        const int4 xa = xp[0], xb = xp[1];
        const float dx = asc[b * nb + j].x;
#pragma unroll
        for (int r = 0; r < 2; r++) {
            int t = dot4((int)s.w[r][0].x, xa.x, 0);
            t = dot4((int)s.w[r][0].y, xa.y, t);
            t = dot4((int)s.w[r][0].z, xa.z, t);
            t = dot4((int)s.w[r][0].w, xa.w, t);
            t = dot4((int)s.w[r][1].x, xb.x, t);
            t = dot4((int)s.w[r][1].y, xb.y, t);
            t = dot4((int)s.w[r][1].z, xb.z, t);
            t = dot4((int)s.w[r][1].w, xb.w, t);
            acc[r][b] += (dw[r] * dx) * (float)t;
        }
    }
}

template <int L, int B, int PRO, int EPI, int D = kQ80wDepth>
__global__ __launch_bounds__(kThreads) void gemvQ80wKernel(GemvArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NG = kThreads / L, RP = NG * 2;
    const int n = a.n, nb = n >> 5, K = (nb + L - 1) / L, P = a.passes, T = P * K;
    const int R = RP * P;
    const GemvLds lay = gemvLayout(n, B, true, R, PRO_RESNORM);  // the Q40 GEMV's activation image
    float *scratch = reinterpret_cast<float *>(smem + lay.scratch);
    float *hbuf = reinterpret_cast<float *>(smem + lay.hbuf);
    int8_t *sq = reinterpret_cast<int8_t *>(smem + lay.act);
    float2 *ssc = reinterpret_cast<float2 *>(smem + lay.sc);
    float2 *sRope = reinterpret_cast<float2 *>(smem + lay.rope);
    const int tid = threadIdx.x, gi = tid / L, li = tid % L, blk = blockIdx.x;
    const int rowBase = blk * R;

    // this workgroup's chunks are [blk * T, blk * T + T) of the tiled planes; loads past the last
    // step, or past the matrix's last chunk, re-read the last one (defined registers, dropped rows)
    const u32x4 *qp = reinterpret_cast<const u32x4 *>(a.qs);
    const uint32_t *dp = reinterpret_cast<const uint32_t *>(a.wd);
    const size_t cBase = (size_t)blk * T;
    const size_t cLast = (size_t)((a.rows + RP - 1) / RP) * K - 1;
    auto load = [&](int t, Q80wStep &s) {
        const size_t c = min(cBase + (size_t)min(t, T - 1), cLast);
        const u32x4 *p = qp + c * 4 * kThreads + tid;
        s.w[0][0] = __builtin_nontemporal_load(p);
        s.w[0][1] = __builtin_nontemporal_load(p + kThreads);
        s.w[1][0] = __builtin_nontemporal_load(p + 2 * kThreads);
        s.w[1][1] = __builtin_nontemporal_load(p + 3 * kThreads);
        s.d = dp[c * kThreads + tid];
    };
    Q80wStep g0[D], g1[D];
#pragma unroll
    for (int i = 0; i < D; i++) load(i, g0[i]);  // in flight across the prologue

    int posB[B], slotB[B];
#pragma unroll
    for (int b = 0; b < B; b++) {
        posB[b] = EPI == EPI_QKV ? a.pos[b] : 0;
        slotB[b] = EPI == EPI_QKV ? a.slot[b] : 0;
    }
    if constexpr (EPI == EPI_QKV) {  // the prologue's barrier publishes these
        const int h2 = a.hs >> 1;
        for (int i = tid; i < B * h2; i += kThreads) {
            const int b = i / h2;
            sRope[b * (kMaxHeadSize / 2) + i % h2] = a.rope[(size_t)posB[b] * h2 + i % h2];
        }
    }
    if constexpr (PRO == PRO_RESNORM) resNormPrologue<B, true>(a, scratch, sq, ssc, nullptr);
    else stageQ80<B>(a, sq, ssc);

    float acc[2][B];
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
        for (int b = 0; b < B; b++) acc[r][b] = 0.f;
    int cp = 0, ck = 0;  // consume cursor: pass, step of the pass
    auto consume = [&](const Q80wStep &s) {
        const int j = li + ck * L;
        const bool use = j < nb;
        float dw[2];
        dw[0] = use ? __half2float(__ushort_as_half((uint16_t)(s.d & 0xFFFFu))) : 0.f;
        dw[1] = use ? __half2float(__ushort_as_half((uint16_t)(s.d >> 16))) : 0.f;
        q80wBlock<B>(acc, s, dw, min(j, nb - 1), n, nb, sq, ssc);
        if (++ck < K) return;
        // end of a row pair: reduce over the lane group, fused epilogue on its lane 0
#pragma unroll
        for (int r = 0; r < 2; r++)
#pragma unroll
            for (int b = 0; b < B; b++) acc[r][b] = groupSum<L>(acc[r][b]);
        const int r0 = rowBase + cp * RP + gi * 2;
        if (li == 0 && r0 < a.rows) {
#pragma unroll
            for (int b = 0; b < B; b++) {
                const float v0 = acc[0][b], v1 = acc[1][b];
                if constexpr (EPI == EPI_STORE) {
                    float *o = a.out + (size_t)b * a.ldOut + r0;
                    o[0] = v0;
                    if (r0 + 1 < a.rows) o[1] = v1;
                } else if constexpr (EPI == EPI_ACT) {
                    a.out[(size_t)b * a.ldOut + (r0 >> 1)] = gateAct(a, v0) * v1;
                } else if constexpr (EPI == EPI_ACT_Q80) {
                    hbuf[b * (R >> 1) + ((r0 - rowBase) >> 1)] = gateAct(a, v0) * v1;
                } else {
                    qkvPairStore(a, r0, v0, v1, sRope + b * (kMaxHeadSize / 2), posB[b], slotB[b],
                                 a.out + (size_t)b * a.ldOut);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < 2; r++)
#pragma unroll
            for (int b = 0; b < B; b++) acc[r][b] = 0.f;
        ck = 0;
        ++cp;
    };
    // two register groups alternate: the other group's loads go out before this one is consumed
    for (int t = 0; t < T; t += 2 * D) {
#pragma unroll
        for (int i = 0; i < D; i++) load(t + D + i, g1[i]);
#pragma unroll
        for (int i = 0; i < D; i++)
            if (t + i < T) consume(g0[i]);
#pragma unroll
        for (int i = 0; i < D; i++) load(t + 2 * D + i, g0[i]);
#pragma unroll
        for (int i = 0; i < D; i++)
            if (t + D + i < T) consume(g1[i]);
    }
    if constexpr (EPI == EPI_ACT_Q80) {
        __syncthreads();
        storeHiddenQ80<B>(a, hbuf, R >> 1, rowBase >> 1);
    }
}

// Kernel instance of one launch configuration (null: unsupported combination).
template <int L, int B>
static const void *gemvQ80wFnPE(int pro, int epi) {
#define DL_Q80W_CASE(P, E) \
    if (pro == P && epi == E) return (const void *)gemvQ80wKernel<L, B, P, E>;
    DL_Q80W_CASE(PRO_GLOBAL, EPI_STORE)
    DL_Q80W_CASE(PRO_RESNORM, EPI_STORE)
    DL_Q80W_CASE(PRO_RESNORM, EPI_QKV)
    DL_Q80W_CASE(PRO_RESNORM, EPI_ACT)
    DL_Q80W_CASE(PRO_RESNORM, EPI_ACT_Q80)
#undef DL_Q80W_CASE
    return nullptr;
}

// Depth sweep instances (one row, producer's blocks, store): the measurements of profiles/q80_weights.md.
template <int L>
static const void *gemvQ80wDepthFn(int depth) {
    switch (depth) {
        case 1: return (const void *)gemvQ80wKernel<L, 1, PRO_GLOBAL, EPI_STORE, 1>;
        case 2: return (const void *)gemvQ80wKernel<L, 1, PRO_GLOBAL, EPI_STORE, 2>;
        case 3: return (const void *)gemvQ80wKernel<L, 1, PRO_GLOBAL, EPI_STORE, 3>;
        case 4: return (const void *)gemvQ80wKernel<L, 1, PRO_GLOBAL, EPI_STORE, 4>;
        default: return nullptr;
    }
}

template <int L>
static const void *gemvQ80wFnB(int B, int pro, int epi) {
    switch (B) {
        case 1: return gemvQ80wFnPE<L, 1>(pro, epi);
        case 2: return gemvQ80wFnPE<L, 2>(pro, epi);
        case 4: return gemvQ80wFnPE<L, 4>(pro, epi);
        default: return nullptr;
    }
}

}  // namespace hipk
}  // namespace dl
