// Candidate filter ahead of the device sampler (LogitFilterArgs in kernels.h): top_k and min_p mask
// a row's logits in place, so that requests that use them still leave the device as token ids only.
//
// grid (sampleGroups(B), B), 256 threads, four dependent launches (kernel boundaries are the only
// grid-wide synchronisation, as in the sampler). The row is cut into 16-byte vectors; workgroup g
// owns the vectors [g * vpg, (g + 1) * vpg) and the last workgroup also the vocab % 4 scalar tail,
// in every launch. Rows of a [B][vocab] buffer start on 4-byte boundaries when vocab % 4 != 0, so
// the vectors are typed with 4-byte alignment (global 16-byte accesses need no more).
//   select 0-2  exact k-th largest: an 11/11/10-bit radix search, from the top digit down, over the
//               order-preserving key of x (-0.0 folded onto +0.0). A workgroup counts the elements
//               of its share whose key matches the digits found so far into a 2048-bin histogram
//               (one LDS copy per wave; lanes that share a bin add once), stores it to its slot of
//               `hist`, and the row's last arriver sums the slots and picks the bin in which the
//               descending cumulative count reaches what is left of k. Pass 0 also reduces the row
//               maximum. Counts are integers: the sum does not depend on its order.
//   mask        thr = max(float of the found key, maximum + delta); elements below it become -inf.
// Cross-workgroup values are written and read with agent-scope relaxed atomics behind the
// last-arriver handshake of the sampler (sample.hip, lastArrival: no __threadfence, no float
// atomics); the row state a launch leaves is read by the next launch.
#include "decode_common.h"

namespace dl {
namespace hipk {

static constexpr int kLfThreads = 256;
static constexpr int kLfWaves = kLfThreads / 64;
static constexpr int kLfBins = 2048;
static constexpr int kLfU = 4;  // vectors in flight per thread per round

typedef float lfF4 __attribute__((ext_vector_type(4), aligned(4)));

struct LfRowState {  // LogitFilterArgs::state
    uint32_t prefix;  // the key's digits found so far
    int rem;          // rank of the k-th largest among the keys matching them (0: no selection)
    float mx;         // the row maximum
    int counter;      // last-arriver counter of the current launch (back to 0 after each)
};
static_assert(sizeof(LfRowState) == kLogitFilterStateWords * 4, "LfRowState size");

// order-preserving key of x, -0.0 on +0.0's
__device__ __forceinline__ uint32_t lfKey(float x) {
    const uint32_t u = __float_as_uint(x);
    if (x == 0.f) return 0x80000000u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float lfKeyValue(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

struct LfShare {  // a workgroup's share of its row
    int v0, v1;   // vectors
    int nvec, vocab;
    bool tailOwner;
};

__device__ __forceinline__ LfShare lfShare(int vocab) {
    LfShare s;
    s.vocab = vocab;
    s.nvec = vocab / 4;
    const int G = (int)gridDim.x, vpg = (s.nvec + G - 1) / G;
    s.v0 = min((int)blockIdx.x * vpg, s.nvec);
    s.v1 = min(s.v0 + vpg, s.nvec);
    s.tailOwner = (int)blockIdx.x == G - 1;
    return s;
}

// f(value, valid) for every element of the share, uniformly on every lane of the workgroup (the
// vector index is clamped, so the loads are unconditional and issued before the first use).
template <typename F>
__device__ __forceinline__ void lfForShare(const float *x, const LfShare &s, F f) {
    for (int r0 = s.v0; r0 < s.v1; r0 += kLfU * kLfThreads) {
        lfF4 v[kLfU];
#pragma unroll
        for (int u = 0; u < kLfU; u++)
            v[u] = reinterpret_cast<const lfF4 *>(x)[min(r0 + u * kLfThreads + (int)threadIdx.x, s.v1 - 1)];
#pragma unroll
        for (int u = 0; u < kLfU; u++) {
            const bool ok = r0 + u * kLfThreads + (int)threadIdx.x < s.v1;
            f(v[u].x, ok);
            f(v[u].y, ok);
            f(v[u].z, ok);
            f(v[u].w, ok);
        }
    }
    if (s.tailOwner && 4 * s.nvec < s.vocab) {
        const int e = 4 * s.nvec + (int)threadIdx.x;
        f(x[min(e, s.vocab - 1)], e < s.vocab);
    }
}

// Lanes that share the first active lane's bin are counted with one ballot and added once (three
// times), the rest add directly: a flat distribution puts nearly every element of the top-digit
// pass in a few bins, where per-lane LDS atomics would serialise.
__device__ __forceinline__ void lfHistAddWave(uint32_t *h, bool act, uint32_t bin) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int rep = 0; rep < 3; rep++) {
        const unsigned long long am = __ballot(act);
        if (am == 0ull) return;
        const int leader = __builtin_ctzll(am);
        const uint32_t b0 = __shfl(bin, leader);
        const bool mine = act && bin == b0;
        const unsigned long long mm = __ballot(mine);
        if (lane == leader) atomicAdd(&h[b0], (uint32_t)__builtin_popcountll(mm));
        act = act && !mine;
    }
    if (act) atomicAdd(&h[bin], 1u);
}

// the sampler's last-arriver handshake (sample.hip, lastArrival)
__device__ __forceinline__ bool lfLastArrival(LfRowState *st, int G, int *flag) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0)
        flag[0] = __hip_atomic_fetch_add(&st->counter, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == G - 1;
    __syncthreads();
    if (!flag[0]) return false;
    if (threadIdx.x == 0) __hip_atomic_store(&st->counter, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return true;
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
__global__ __launch_bounds__(kLfThreads) void logitFilterSelectKernel(LogitFilterArgs a) {
    __shared__ uint32_t h[kLfBins * kLfWaves];  // one histogram per wave (32 KB)
    __shared__ float red[kLfWaves];
    __shared__ int wtot[kLfWaves];
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
    const LfShare sh = lfShare(a.vocab);
    uint32_t *hw = h + (tid >> 6) * kLfBins;  // this wave's histogram
    constexpr int PER = kLfBins / kLfThreads;  // 8 bins per thread
    uint32_t *gh = a.hist + ((size_t)b * G + g) * kLfBins;
    float *part = a.part + (size_t)b * kSampleMaxGroups;

    if (plan.select) {
        for (int i = tid; i < kLfBins * kLfWaves; i += kLfThreads) h[i] = 0u;
        __syncthreads();
    }
    float mx = -INFINITY;
    lfForShare(x, sh, [&](float v, bool ok) {
        if (PASS == 0 && ok) mx = fmaxf(mx, v);
        if (!plan.select) return;
        const uint32_t k = lfKey(v);
        if (hiShift < 32) ok = ok && (k >> (hiShift & 31)) == (prefix >> (hiShift & 31));
        lfHistAddWave(hw, ok, (k >> shift) & mask);
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
        for (int w = 1; w < kLfWaves; w++) m = fmaxf(m, red[w]);
        __hip_atomic_store(&part[g], m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (plan.select) {
        // this workgroup's histogram (the waves' copies summed) -> its partial slot; lane-consecutive
        // bins: every store instruction is one 1 KB run
#pragma unroll
        for (int j = 0; j < PER; j++) {
            const int bin = j * kLfThreads + tid;
            uint32_t v = 0u;
#pragma unroll
            for (int w = 0; w < kLfWaves; w++) v += h[w * kLfBins + bin];
            __hip_atomic_store(&gh[bin], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (!lfLastArrival(st, G, flag)) return;
    // ---- the row's last arriver
    if (PASS == 0 && tid == 0) {
        float m = -INFINITY;
        for (int j = 0; j < G; j++)
            m = fmaxf(m, __hip_atomic_load(&part[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        st->mx = m;
    }
    if (!plan.select) return;
    // sum the G partial histograms into LDS, then pick the highest bin whose count together with
    // the bins above it reaches rem
    {
        const uint32_t *rowh = a.hist + (size_t)b * G * kLfBins;
        uint32_t acc8[PER];
#pragma unroll
        for (int j = 0; j < PER; j++) acc8[j] = 0u;
        for (int g0 = 0; g0 < G; g0 += 4) {
            uint32_t t4[4][PER];
#pragma unroll
            for (int q = 0; q < 4; q++)
#pragma unroll
                for (int j = 0; j < PER; j++)
                    t4[q][j] = __hip_atomic_load(&rowh[(size_t)min(g0 + q, G - 1) * kLfBins + j * kLfThreads + tid],
                                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (g0 + q < G)
#pragma unroll
                    for (int j = 0; j < PER; j++) acc8[j] += t4[q][j];
        }
#pragma unroll
        for (int j = 0; j < PER; j++) h[j * kLfThreads + tid] = acc8[j];
    }
    if (tid == 0) sSel[0] = -1;
    __syncthreads();
    int v[PER];
    int tot = 0;
#pragma unroll
    for (int j = 0; j < PER; j++) {
        v[j] = (int)h[tid * PER + j];
        tot += v[j];
    }
    // count in the bins of higher threads (exclusive suffix over threads)
    int inc = tot;  // inclusive suffix within the wave (lanes >= this lane)
    const int lane = tid & 63, wv = tid >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int y = __shfl_down(inc, off);
        if (lane + off < 64) inc += y;
    }
    if (lane == 0) wtot[wv] = inc;
    __syncthreads();
    int acc = inc - tot;
    for (int w = wv + 1; w < kLfWaves; w++) acc += wtot[w];
    // (at most one thread: acc < rem <= acc + tot)
#pragma unroll
    for (int j = PER - 1; j >= 0; j--) {
        if (acc < rem && acc + v[j] >= rem) {
            sSel[0] = tid * PER + j;
            sSel[1] = acc;
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

__global__ __launch_bounds__(kLfThreads) void logitFilterMaskKernel(LogitFilterArgs a) {
    const int b = blockIdx.y;
    const LogitFilterRow row = a.rows[b];
    const LfRowPlan plan = lfPlan(a, b, row);
    if (!plan.run) return;
    const LfRowState *st = reinterpret_cast<const LfRowState *>(a.state) + b;
    const float thrK = plan.select && st->rem > 0 ? lfKeyValue(st->prefix) : -INFINITY;
    const float thrP = plan.minP ? st->mx + row.delta : -INFINITY;
    const float thr = fmaxf(thrK, thrP);
    float *x = a.logits + (size_t)b * a.vocab;
    const LfShare sh = lfShare(a.vocab);
    for (int i0 = sh.v0 + (int)threadIdx.x; i0 < sh.v1; i0 += kLfU * kLfThreads) {
        lfF4 v[kLfU];
#pragma unroll
        for (int u = 0; u < kLfU; u++) {
            const int i = i0 + u * kLfThreads;
            if (i < sh.v1) v[u] = reinterpret_cast<const lfF4 *>(x)[i];
        }
#pragma unroll
        for (int u = 0; u < kLfU; u++) {
            const int i = i0 + u * kLfThreads;
            if (i < sh.v1) {
                lfF4 y;
                y.x = v[u].x >= thr ? v[u].x : -INFINITY;
                y.y = v[u].y >= thr ? v[u].y : -INFINITY;
                y.z = v[u].z >= thr ? v[u].z : -INFINITY;
                y.w = v[u].w >= thr ? v[u].w : -INFINITY;
                reinterpret_cast<lfF4 *>(x)[i] = y;
            }
        }
    }
    if (sh.tailOwner) {
        const int e = 4 * sh.nvec + (int)threadIdx.x;
        if (e < sh.vocab) x[e] = x[e] >= thr ? x[e] : -INFINITY;
    }
}

void launchLogitFilter(const LogitFilterArgs &a, int B, hipStream_t s) {
    const dim3 grid(sampleGroups(B), B);
    hipLaunchKernelGGL(logitFilterSelectKernel<0>, grid, dim3(kLfThreads), 0, s, a);
    hipLaunchKernelGGL(logitFilterSelectKernel<1>, grid, dim3(kLfThreads), 0, s, a);
    hipLaunchKernelGGL(logitFilterSelectKernel<2>, grid, dim3(kLfThreads), 0, s, a);
    hipLaunchKernelGGL(logitFilterMaskKernel, grid, dim3(kLfThreads), 0, s, a);
}

// (preloadModules: any kernel of this code object)
const void *logitFilterModuleKernel() { return (const void *)logitFilterMaskKernel; }

}  // namespace hipk
}  // namespace dl
