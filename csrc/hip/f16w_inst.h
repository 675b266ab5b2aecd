// Decode GEMV on F16 weights (gemvF16wKernel) and its per-(batch, prologue, epilogue) instance
// table, compiled once per lanes-per-row L in f16w_l16/32/64.hip (parallel builds).
//
//   out[b][r] = sum_k f32(w[r][k]) * x[b][k]     w f16 row-major [rows][n], x f32
//
// every term one f32 FMA into an f32 accumulator (the widening of the f16 weight is exact and is
// folded into the FMA by the compiler: v_fma_mix_f32). Work split: a lane group of L lanes owns
// kF16wRG consecutive rows per pass; lane li walks the 16-byte units (8 weights) li, li + L, ... of
// each of them. One iteration issues kF16wRG x kF16wU nontemporal 16-byte loads per lane before any
// is consumed (F16 rows are half the bytes of F32 rows, so one row per lane group at the F32
// kernel's unroll would leave half the bytes in flight); the 8 f32 activations of a step are read
// once (LDS after the norm prologue, the caller's rows otherwise) and feed kF16wRG x 8 FMAs per batch
// row. Whole iterations run unguarded; the last steps (n / 8 no multiple of L x kF16wU, or fewer
// units than lanes) re-read the row's last unit and drop it. Row pairs (2k, 2k + 1) sit in one lane
// group, so the pair epilogues (SwiGLU, RoPE + KV append) run on the group's lane 0 from registers.
#pragma once
#include "decode_dev.h"

namespace dl {
namespace hipk {

// rows per lane group (even: pair epilogues) x steps per iteration: 16-byte loads in flight per lane
#ifndef DL_F16W_RG
#define DL_F16W_RG 2
#endif
#ifndef DL_F16W_U
#define DL_F16W_U 4
#endif
static constexpr int kF16wRG = DL_F16W_RG, kF16wU = DL_F16W_U;
static_assert(kF16wRG == 2 || kF16wRG == 4, "row pairs stay in one lane group");

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

template <int L, int B, int PRO, int EPI>
__global__ __launch_bounds__(kThreads) void gemvF16wKernel(GemvArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int RG = kF16wRG, U = kF16wU;
    constexpr int RP = kThreads / L * RG;  // rows per pass
    const int n = a.n, nu = n >> 3;        // 16-byte units per row
    const int R = RP * a.passes;
    const GemvLds lay = gemvLayout(n, B, false, R, PRO);
    float *scratch = reinterpret_cast<float *>(smem + lay.scratch);
    const int tid = threadIdx.x, gi = tid / L, li = tid % L;
    const int rowBase = blockIdx.x * R;

    // activation source: normalized copy in LDS or the caller's f32 rows
    const float *actF = PRO == PRO_RESNORM ? reinterpret_cast<const float *>(smem + lay.act) : a.in;
    const int ldx = PRO == PRO_RESNORM ? n : a.ldIn;
    if constexpr (PRO == PRO_RESNORM)
        resNormPrologue<B, false>(a, scratch, nullptr, nullptr, reinterpret_cast<float *>(smem + lay.act));

    const int full = nu / (L * U) * U;      // steps of whole iterations: every lane in range
    const int steps = (nu + L - 1) / L;
    for (int p = 0; p < a.passes; p++) {
        const int row0 = rowBase + p * RP + gi * RG;
        const u32x4 *wrow[RG];
#pragma unroll
        for (int r = 0; r < RG; r++)  // rows past the end: clamped for the loads, dropped at the store
            wrow[r] = reinterpret_cast<const u32x4 *>(a.wh + (size_t)min(row0 + r, a.rows - 1) * n);
        float acc[RG][B];
#pragma unroll
        for (int r = 0; r < RG; r++)
#pragma unroll
            for (int b = 0; b < B; b++) acc[r][b] = 0.f;

        // U steps from step s0 on; GUARD: units past the row's end are clamped and dropped
        auto iter = [&](int s0, auto guard) {
            constexpr bool GUARD = decltype(guard)::value;
            u32x4 w[U][RG];
            int unit[U];
#pragma unroll
            for (int i = 0; i < U; i++) {
                unit[i] = li + (s0 + i) * L;
                const int uc = GUARD ? min(unit[i], nu - 1) : unit[i];
#pragma unroll
                for (int r = 0; r < RG; r++) w[i][r] = __builtin_nontemporal_load(wrow[r] + uc);
            }
#pragma unroll
            for (int i = 0; i < U; i++) {
                if (GUARD && unit[i] >= nu) continue;
#pragma unroll
                for (int b = 0; b < B; b++) {
                    const float *xp = actF + (size_t)b * ldx + unit[i] * 8;
                    const float4 x0 = ld4(xp), x1 = ld4(xp + 4);
                    const float xv[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
#pragma unroll
                    for (int r = 0; r < RG; r++) {
                        const f16x8 wv = __builtin_bit_cast(f16x8, w[i][r]);
#pragma unroll
                        for (int e = 0; e < 8; e++) acc[r][b] = fmaf((float)wv[e], xv[e], acc[r][b]);
                    }
                }
            }
        };
        int s = 0;
        for (; s < full; s += U) iter(s, std::false_type{});
        for (; s < steps; s += U) iter(s, std::true_type{});

#pragma unroll
        for (int r = 0; r < RG; r++)
#pragma unroll
            for (int b = 0; b < B; b++) acc[r][b] = groupSum<L>(acc[r][b]);
        if (li != 0) continue;
#pragma unroll
        for (int q = 0; q < RG; q += 2) {
            const int r0 = row0 + q;
#pragma unroll
            for (int b = 0; b < B; b++) {
                const float v0 = acc[q][b], v1 = acc[q + 1][b];
                if constexpr (EPI == EPI_STORE) {
                    float *o = a.out + (size_t)b * a.ldOut + r0;
                    if (r0 < a.rows) o[0] = v0;
                    if (r0 + 1 < a.rows) o[1] = v1;
                } else if constexpr (EPI == EPI_ACT) {
                    // interleaved rows: 2i = gate (w1), 2i+1 = up (w3)
                    if (r0 < a.rows) a.out[(size_t)b * a.ldOut + (r0 >> 1)] = gateAct(a, v0) * v1;
                } else {
                    static_assert(EPI == EPI_QKV, "gemvF16wKernel: store, SwiGLU or RoPE + KV append");
                    if (r0 < a.rows)
                        qkvPairStore(a, r0, v0, v1, a.rope + (size_t)a.pos[b] * (a.hs >> 1), a.pos[b], a.slot[b],
                                     a.out + (size_t)b * a.ldOut);
                }
            }
        }
    }
}

// Kernel instance of one launch configuration (null: unsupported combination).
template <int L, int B>
static const void *gemvF16wFnPE(int pro, int epi) {
#define DL_F16W_CASE(P, E) \
    if (pro == P && epi == E) return (const void *)gemvF16wKernel<L, B, P, E>;
    DL_F16W_CASE(PRO_GLOBAL, EPI_STORE)
    DL_F16W_CASE(PRO_RESNORM, EPI_STORE)
    DL_F16W_CASE(PRO_RESNORM, EPI_QKV)
    DL_F16W_CASE(PRO_RESNORM, EPI_ACT)
#undef DL_F16W_CASE
    return nullptr;
}

template <int L>
static const void *gemvF16wFnB(int B, int pro, int epi) {
    switch (B) {
        case 1: return gemvF16wFnPE<L, 1>(pro, epi);
        case 2: return gemvF16wFnPE<L, 2>(pro, epi);
        case 4: return gemvF16wFnPE<L, 4>(pro, epi);
        default: return nullptr;
    }
}

}  // namespace hipk
}  // namespace dl
