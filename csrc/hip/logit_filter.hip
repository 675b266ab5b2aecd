// Candidate filter ahead of the device sampler (LogitFilterArgs in kernels.h): top_k and min_p mask
// a row's logits in place, so that requests that use them still leave the device as token ids only.
//
// grid (sampleGroups(B), B), 256 threads, four dependent launches (kernel boundaries are the only
// grid-wide synchronisation, as in the sampler). A workgroup works on its share of the row
// (RowShare, row_dev.h) in every launch.
//   select 0-2  exact k-th largest: an 11/11/10-bit radix search, from the top digit down, over the
//               order-preserving key of x (-0.0 folded onto +0.0). A workgroup counts the elements
//               of its share whose key matches the digits found so far into a 2048-bin histogram
//               (one LDS copy per wave; lanes that share a bin add once), stores it to its slot of
//               `hist`, and the row's last arriver sums the slots and picks the bin in which the
//               descending cumulative count reaches what is left of k. Pass 0 also reduces the row
//               maximum. Counts are integers: the sum does not depend on its order.
//   mask        thr = max(float of the found key, maximum + delta); elements below it become -inf.
// Cross-workgroup values go through the fence-free hand-off (splitArrive, decode_common.h: no
// __threadfence, no float atomics); the row state a launch leaves is read by the next launch.
#include "row_dev.h"

namespace dl {
namespace hipk {

struct LfRowState {  // LogitFilterArgs::state
    uint32_t prefix;  // the key's digits found so far
    int rem;          // rank of the k-th largest among the keys matching them (0: no selection)
    float mx;         // the row maximum
    int counter;      // last-arriver counter of the current launch (back to 0 after each)
};
static_assert(sizeof(LfRowState) == kLogitFilterStateWords * 4, "LfRowState size");

// the value of an order-preserving key (orderKeyFolded, row_dev.h)
__device__ __forceinline__ float lfKeyValue(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

struct LfRowPlan {
    bool run;     // the row is filtered at all
    bool select;  // top-k is on
    bool minP;
};

__device__ __forceinline__ LfRowPlan lfPlan(const LogitFilterArgs &a, int b, const LogitFilterRow &r) {
    LfRowPlan p;
    const bool drawn = r.active != 0 && a.spec[b].x > 0.f;
    p.select = drawn && r.topK >= 1 && r.topK < a.vocab;
    p.minP = drawn && r.delta > -INFINITY;
    p.run = p.select || p.minP;
    return p;
}

template <int PASS>
__global__ __launch_bounds__(kRowWg) void logitFilterSelectKernel(LogitFilterArgs a) {
    __shared__ uint32_t h[kRowBins * kRowWaves];  // one histogram per wave (32 KB)
    __shared__ float red[kRowWaves];
    __shared__ uint32_t wtot[kRowWaves];
    __shared__ int flag[1];
    __shared__ int sSel[2];
    const int b = blockIdx.y, g = blockIdx.x, G = gridDim.x, tid = threadIdx.x;
    const LogitFilterRow row = a.rows[b];
    const LfRowPlan plan = lfPlan(a, b, row);
    if (!plan.run || (PASS > 0 && !plan.select)) return;  // (uniform over the row's workgroups)
    LfRowState *st = reinterpret_cast<LfRowState *>(a.state) + b;
    const int rem = PASS == 0 ? row.topK : st->rem;
    if (PASS > 0 && rem <= 0) return;
    const uint32_t prefix = PASS == 0 ? 0u : st->prefix;
    constexpr int shift = PASS == 0 ? 21 : (PASS == 1 ? 10 : 0);
    constexpr uint32_t width = PASS == 2 ? 10 : 11, mask = (1u << width) - 1u;
    constexpr int hiShift = shift + (int)width;  // bits above this digit (32 for pass 0)
    const float *x = a.logits + (size_t)b * a.vocab;
    const RowShare sh = rowShare(a.vocab);
    uint32_t *hw = h + (tid >> 6) * kRowBins;  // this wave's histogram
    uint32_t *gh = a.hist + ((size_t)b * G + g) * kRowBins;
    float *part = a.part + (size_t)b * kSampleMaxGroups;

    if (plan.select) {
        for (int i = tid; i < kRowBins * kRowWaves; i += kRowWg) h[i] = 0u;
        __syncthreads();
    }
    float mx = -INFINITY;
    forShare(x, sh, [&](float v, bool ok) {
        if (PASS == 0 && ok) mx = fmaxf(mx, v);
        if (!plan.select) return;
        const uint32_t k = orderKeyFolded(v);
        if (hiShift < 32) ok = ok && (k >> (hiShift & 31)) == (prefix >> (hiShift & 31));
        histAddWave(hw, ok, (k >> shift) & mask, 1u);
    });
    if (PASS == 0) {  // the share's maximum -> its partial slot
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
        if ((tid & 63) == 0) red[tid >> 6] = mx;
    }
    __syncthreads();
    if (PASS == 0 && tid == 0) {
        float m = red[0];
#pragma unroll
        for (int w = 1; w < kRowWaves; w++) m = fmaxf(m, red[w]);
        wtStore(&part[g], m);
    }
    if (plan.select) histStorePartial(h, gh);
    if (!splitArrive(&st->counter, G, flag)) return;
    // ---- the row's last arriver
    if (PASS == 0 && tid == 0) {
        float m = -INFINITY;
        for (int j = 0; j < G; j++) m = fmaxf(m, wtLoad(&part[j]));
        st->mx = m;
    }
    if (!plan.select) return;
    // sum the G partial histograms into LDS, then pick the highest bin whose count together with
    // the bins above it reaches rem
    if (tid == 0) sSel[0] = -1;
    histSumPartials(a.hist + (size_t)b * G * kRowBins, G, h);
    constexpr int PER = kRowBinsPer;
    uint32_t v[PER];
    uint32_t acc = suffixAbove(h, wtot, v);  // count in the bins of higher threads
    const uint32_t need = (uint32_t)rem;
    // (at most one thread: acc < rem <= acc + tot)
#pragma unroll
    for (int j = PER - 1; j >= 0; j--) {
        if (acc < need && acc + v[j] >= need) {
            sSel[0] = tid * PER + j;
            sSel[1] = (int)acc;
        }
        acc += v[j];
    }
    __syncthreads();
    if (tid == 0) {
        const int bin = sSel[0];
        // (fewer matching keys than rem cannot happen for 1 <= topK < vocab; then: no selection)
        st->prefix = bin < 0 ? 0u : (prefix | ((uint32_t)bin << shift));
        st->rem = bin < 0 ? 0 : rem - sSel[1];
    }
}

__global__ __launch_bounds__(kRowWg) void logitFilterMaskKernel(LogitFilterArgs a) {
    const int b = blockIdx.y;
    const LogitFilterRow row = a.rows[b];
    const LfRowPlan plan = lfPlan(a, b, row);
    if (!plan.run) return;
    const LfRowState *st = reinterpret_cast<const LfRowState *>(a.state) + b;
    const float thrK = plan.select && st->rem > 0 ? lfKeyValue(st->prefix) : -INFINITY;
    const float thrP = plan.minP ? st->mx + row.delta : -INFINITY;
    const float thr = fmaxf(thrK, thrP);
    float *x = a.logits + (size_t)b * a.vocab;
    const RowShare sh = rowShare(a.vocab);
    mapShare(sh, x, x, x, [&](float v, float) { return v >= thr ? v : -INFINITY; });
}

void launchLogitFilter(const LogitFilterArgs &a, int B, hipStream_t s) {
    const dim3 grid(sampleGroups(B), B);
    hipLaunchKernelGGL(logitFilterSelectKernel<0>, grid, dim3(kRowWg), 0, s, a);
    hipLaunchKernelGGL(logitFilterSelectKernel<1>, grid, dim3(kRowWg), 0, s, a);
    hipLaunchKernelGGL(logitFilterSelectKernel<2>, grid, dim3(kRowWg), 0, s, a);
    hipLaunchKernelGGL(logitFilterMaskKernel, grid, dim3(kRowWg), 0, s, a);
}

// (preloadModules: any kernel of this code object)
const void *logitFilterModuleKernel() { return (const void *)logitFilterMaskKernel; }

}  // namespace hipk
}  // namespace dl
