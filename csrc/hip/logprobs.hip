// Per-token log-probabilities of the logits rows (LogprobArgs in kernels.h): the chosen token's
// log_softmax value and the k best tokens of the row, so that a request for logprobs moves
// (1 + 20) x 8 bytes per row to the host instead of the row's 128256 logits.
//
// grid (logprobGroups(vocab), B). A workgroup reads its slice of the row once, in tiles of 8192
// logits held in registers (one tile for vocabularies up to 64 x 8192), and keeps
//   - per thread the max and the sum of exp(x - max) of its elements, reduced over the workgroup
//     in a fixed order;
//   - the slice's k best, by k rounds of a workgroup argmax: round r takes the best element that
//     comes strictly after round r - 1's winner in the (logit descending, id ascending) order, so
//     nothing is sorted and the held elements are never changed. A further tile competes against
//     the list of the tiles before it (one list entry per thread as an extra element).
// The partials go to the row's scratch with agent-scope stores; the row's last-arriving workgroup
// (the fence-free hand-off, splitArrive in decode_common.h) combines the (max, sum) pairs in workgroup
// order, runs the same k rounds over the groups x k candidates and writes the row's output. No
// float atomics in memory and no dependence on B or on the arrival order: a row's output is
// bitwise reproducible.
#include "row_dev.h"

namespace dl {
namespace hipk {

static constexpr int kLgpVals = 32;  // logits per thread per tile
static constexpr int kLgpTile = kRowWg * kLgpVals;
static constexpr int kLgpNone = 0x7fffffff;
static constexpr int kLgpCands = kLogprobMaxGroups * kLogprobTop / kRowWg;  // candidates per thread, last arriver
static_assert(kLogprobMaxGroups * kLogprobTop % kRowWg == 0, "candidates per thread");
static_assert(kLogprobTop <= kRowWg && kLogprobSlots <= kRowWg, "one thread per list entry / output slot");
static_assert(sizeof(LogprobEntry) == 8, "LogprobEntry layout");

int logprobGroups(int vocab) {
    const int G = (vocab + kLgpTile - 1) / kLgpTile;
    return G < 1 ? 1 : (G > kLogprobMaxGroups ? kLogprobMaxGroups : G);
}

// (v, i) comes strictly after (pv, pi) in the (value descending, index ascending) order
__device__ __forceinline__ bool lgpAfter(float v, int i, float pv, int pi) { return v < pv || (v == pv && i > pi); }

// The workgroup's winner, in every thread. sv / si: two sets of one word per wave; consecutive
// calls alternate `par`, so one barrier per call is enough (a thread two calls ahead has passed the
// barrier of the call in between, which every thread reaches after its reads of this one).
__device__ __forceinline__ void lgpBlockBest(float &bv, int &bi, float (*sv)[kRowWaves], int (*si)[kRowWaves], int par) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) argBetter(bv, bi, __shfl_xor(bv, off), __shfl_xor(bi, off));
    if ((threadIdx.x & 63) == 0) {
        sv[par][threadIdx.x >> 6] = bv;
        si[par][threadIdx.x >> 6] = bi;
    }
    __syncthreads();
    bv = sv[par][0];
    bi = si[par][0];
#pragma unroll
    for (int w = 1; w < kRowWaves; w++) argBetter(bv, bi, sv[par][w], si[par][w]);
}

__global__ __launch_bounds__(kRowWg) void logprobsKernel(LogprobArgs a) {
    __shared__ float sv[2][kRowWaves];
    __shared__ int si[2][kRowWaves];
    __shared__ float listV[2][kLogprobTop];  // the slice's best so far (double-buffered over tiles)
    __shared__ int listI[2][kLogprobTop];
    __shared__ float red[kRowWaves];
    __shared__ float lse[2];
    __shared__ int last;
    const int g = blockIdx.x, b = blockIdx.y, G = gridDim.x, tid = threadIdx.x, V = a.vocab;
    const int req = (int)a.spec[b].w;
    if (req <= 0) return;  // no request: the row's output stays as it is
    const int k = min(req - 1, kLogprobTop);
    const float *x = a.logits + (size_t)b * V;
    const int C = (V + G - 1) / G;
    const int c0 = min(g * C, V), c1 = min(c0 + C, V);
    if (tid < kLogprobTop) {
        listV[0][tid] = listV[1][tid] = -INFINITY;
        listI[0][tid] = listI[1][tid] = kLgpNone;
    }
    __syncthreads();
    float m = -INFINITY, s = 0.f;  // this thread's elements: max, sum of exp(x - max)
    int cur = 0, par = 0;
    for (int r0 = c0; r0 < c1; r0 += kLgpTile) {
        float v[kLgpVals];
#pragma unroll
        for (int j = 0; j < kLgpVals; j++) v[j] = x[min(r0 + j * kRowWg + tid, c1 - 1)];
        __builtin_amdgcn_sched_barrier(0);  // all loads issued before the first use
        float tm = -INFINITY;
#pragma unroll
        for (int j = 0; j < kLgpVals; j++)
            if (r0 + j * kRowWg + tid < c1) tm = fmaxf(tm, v[j]);
        if (tm > -INFINITY) {
            float ts = 0.f;
#pragma unroll
            for (int j = 0; j < kLgpVals; j++)
                if (r0 + j * kRowWg + tid < c1) ts += __expf(v[j] - tm);
            if (tm > m) {
                s = s * __expf(m - tm) + ts;
                m = tm;
            } else {
                s += ts * __expf(tm - m);
            }
        }
        if (k == 0) continue;
        // the list of the tiles before this one: entry tid is this thread's extra element
        const float ov = tid < kLogprobTop ? listV[cur][tid] : -INFINITY;
        const int oi = tid < kLogprobTop ? listI[cur][tid] : kLgpNone;
        float pv = INFINITY;
        int pi = -1;
        for (int r = 0; r < k; r++) {
            float bv = -INFINITY;
            int bi = kLgpNone;
#pragma unroll
            for (int j = 0; j < kLgpVals; j++) {
                const int i = r0 + j * kRowWg + tid;
                if (i < c1 && lgpAfter(v[j], i, pv, pi)) argBetter(bv, bi, v[j], i);
            }
            if (oi != kLgpNone && lgpAfter(ov, oi, pv, pi)) argBetter(bv, bi, ov, oi);
            lgpBlockBest(bv, bi, sv, si, par);
            par ^= 1;
            if (tid == 0) {  // (nothing left: the (-inf, none) pair, after which nothing comes)
                listV[cur ^ 1][r] = bv;
                listI[cur ^ 1][r] = bi;
            }
            pv = bv;
            pi = bi;
        }
        cur ^= 1;
        __syncthreads();
    }
    const float M = wgReduce(m, red, [](float p, float q) { return fmaxf(p, q); });
    const float S = wgReduce(m == -INFINITY ? 0.f : s * __expf(m - M), red, [](float p, float q) { return p + q; });
    const size_t slot = (size_t)b * kLogprobMaxGroups + g;
    if (tid == 0) {
        wtStore(a.scratch.partM + slot, M);
        wtStore(a.scratch.partS + slot, S);
    }
    if (tid < k) {
        wtStore(a.scratch.candV + slot * kLogprobTop + tid, listV[cur][tid]);
        wtStore(a.scratch.candI + slot * kLogprobTop + tid, listI[cur][tid]);
    }
    if (!splitArrive(a.scratch.counters + b, G, &last)) return;

    // ---- the row's last arriver
    const size_t row = (size_t)b * kLogprobMaxGroups;
    LogprobEntry *out = a.out + (size_t)b * kLogprobSlots;
    if (tid == 0) {
        float gm = -INFINITY;
        for (int j = 0; j < G; j++) gm = fmaxf(gm, wtLoad(a.scratch.partM + row + j));
        float z = 0.f;
        for (int j = 0; j < G; j++) {
            const float pm = wtLoad(a.scratch.partM + row + j);
            if (pm != -INFINITY) z += wtLoad(a.scratch.partS + row + j) * expf(pm - gm);
        }
        const float lz = logf(z);
        lse[0] = gm;
        lse[1] = lz;
        const int tg = a.target ? a.target[b] : -1;  // a row that scores a given token draws none
        const int id = tg >= 0 ? tg : a.ids[b];
        const bool ok = id >= 0 && id < V;
        LogprobEntry e;
        e.logprob = ok ? (x[ok ? id : 0] - gm) - lz : 0.f;
        e.id = ok ? id : -1;
        out[0] = e;
    }
    __syncthreads();
    const float gm = lse[0], lz = lse[1];
    float cv[kLgpCands];
    int ci[kLgpCands];
#pragma unroll
    for (int q = 0; q < kLgpCands; q++) {
        const int c = q * kRowWg + tid;  // group c / kLogprobTop, its entry c % kLogprobTop
        const bool ok = c < G * kLogprobTop && c % kLogprobTop < k;
        cv[q] = ok ? wtLoad(a.scratch.candV + row * kLogprobTop + c) : -INFINITY;
        ci[q] = ok ? wtLoad(a.scratch.candI + row * kLogprobTop + c) : kLgpNone;
    }
    float pv = INFINITY;
    int pi = -1;
    for (int r = 0; r < k; r++) {
        float bv = -INFINITY;
        int bi = kLgpNone;
#pragma unroll
        for (int q = 0; q < kLgpCands; q++)
            if (ci[q] != kLgpNone && lgpAfter(cv[q], ci[q], pv, pi)) argBetter(bv, bi, cv[q], ci[q]);
        lgpBlockBest(bv, bi, sv, si, par);
        par ^= 1;
        if (tid == 0) {
            LogprobEntry e;
            e.logprob = bi == kLgpNone ? 0.f : (bv - gm) - lz;
            e.id = bi == kLgpNone ? -1 : bi;  // fewer than k tokens in the vocabulary
            out[1 + r] = e;
        }
        pv = bv;
        pi = bi;
    }
    if (tid > k && tid < kLogprobSlots) {
        LogprobEntry e;
        e.logprob = 0.f;
        e.id = -1;
        out[tid] = e;
    }
}

void launchLogprobs(const LogprobArgs &a, int B, hipStream_t s) {
    hipLaunchKernelGGL(logprobsKernel, dim3(logprobGroups(a.vocab), B), dim3(kRowWg), 0, s, a);
}

}  // namespace hipk
}  // namespace dl
