// Argmax and device sampling of the logits rows (ArgmaxArgs / SampleArgs in kernels.h).
#include "decode_dev.h"
#include "row_dev.h"

#include <cstdlib>
#include <utility>

namespace dl {
namespace hipk {

constexpr int kArgmaxBlocks = 64;

// The row's winner: ids, and for a chained decode the next step's token / position / history.
__device__ __forceinline__ void argmaxStore(const ArgmaxArgs &a, int b, int bi) {
    a.ids[b] = bi;
    if (a.tokens) {
        const int p = a.pos[b];
        a.hist[(size_t)b * a.seqLen + p] = bi;
        a.tokens[b] = bi;
        a.pos[b] = p + 1;
    }
}

// grid (kArgmaxBlocks, B): each workgroup reduces a slice; the last arriver reduces the partials.
__global__ __launch_bounds__(256) void argmaxKernel(ArgmaxArgs a) {
    __shared__ float sv[4];
    __shared__ int si[4];
    __shared__ int last;
    const int b = blockIdx.y;
    const float *x = a.logits + (size_t)b * a.vocab;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    // 8 loads in flight per thread per round (a plain grid-stride loop waits for each load in turn)
    constexpr int U = 8;
    const int stride = gridDim.x * blockDim.x;
    for (int i0 = blockIdx.x * blockDim.x + threadIdx.x; i0 < a.vocab; i0 += U * stride) {
        float v[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int i = i0 + u * stride;
            v[u] = i < a.vocab ? x[i] : -INFINITY;
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int i = i0 + u * stride;
            if (i < a.vocab) argBetter(bv, bi, v[u], i);
        }
    }
    blockArgmax(bv, bi, sv, si);
    // fence-free hand-off (see gemmFinish): agent-scope atomic stores / loads of the partials
    if (threadIdx.x == 0) {
        __hip_atomic_store(a.partV + b * kArgmaxBlocks + blockIdx.x, bv, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(a.partI + b * kArgmaxBlocks + blockIdx.x, bi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int old = __hip_atomic_fetch_add(a.counters + b, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last = old == (int)gridDim.x - 1;
    }
    __syncthreads();
    if (!last) return;
    if (threadIdx.x == 0) __hip_atomic_store(a.counters + b, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    bv = -INFINITY;
    bi = 0x7fffffff;
    for (int i = threadIdx.x; i < (int)gridDim.x; i += blockDim.x)
        argBetter(bv, bi, __hip_atomic_load(a.partV + b * kArgmaxBlocks + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                  __hip_atomic_load(a.partI + b * kArgmaxBlocks + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    blockArgmax(bv, bi, sv, si);
    if (a.pairs) {
        if (threadIdx.x == 0) {
            a.pairs[2 * b] = bv;
            a.pairs[2 * b + 1] = __int_as_float(bi + a.vocabStart);
        }
        return;
    }
    if (threadIdx.x == 0 && a.tp.world > 1) {
        // tensor parallel: every rank offers its slice's winner (value, global index)
        bi += a.vocabStart;
        tpDispatch(a.tp.world, [&](auto wm) { tpArgmaxPick<decltype(wm)::value>(a.tp, b, bv, bi); });
    }
    if (threadIdx.x == 0) argmaxStore(a, b, bi);
}

// One thread per row: the global winner of the all-gathered per-rank pairs, in rank order.
__global__ __launch_bounds__(64) void argmaxPickKernel(ArgmaxArgs a, const float *all, int B, int W) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int p = 0; p < W; p++)
        argBetter(bv, bi, all[(size_t)p * 2 * B + 2 * b], __float_as_int(all[(size_t)p * 2 * B + 2 * b + 1]));
    argmaxStore(a, b, bi);
}

void launchArgmax(const ArgmaxArgs &a, int B, hipStream_t s) {
    hipLaunchKernelGGL(argmaxKernel, dim3(kArgmaxBlocks, B), dim3(256), 0, s, a);
}

void launchArgmaxPick(const ArgmaxArgs &a, const float *all, int B, int W, hipStream_t s) {
    hipLaunchKernelGGL(argmaxPickKernel, dim3((B + 63) / 64), dim3(64), 0, s, a, all, B, W);
}

// ------------------------------------------------------------------------------------------------
// Device sampling (SampleArgs in kernels.h), G workgroups per row and 8 dependent phases (kernel
// boundaries are the only grid-wide synchronisation; inside a phase the last-arriving workgroup of
// a row reduces what the row's workgroups produced and writes the row's state for the next phase).
// x = logit / T; the order-preserving key of x ranks probabilities; searches are 11/11/10-bit radix
// passes over that key, each building a 2048-bin histogram of probability mass (one LDS copy per
// wave, wave-aggregated adds); each workgroup stores its histogram and the row's last arriver
// sums them in workgroup order, so the result is bit-reproducible (no float atomics in memory).
//   0  stats: online max / sum of exp per workgroup, combined by the last arriver (T == 0: argmax)
//   1-3 nucleus cut (top-p): key where the descending cumulative mass first exceeds p
//       (multinomial rows, p <= 0 or >= 1: 1 = per-chunk mass, 2 = the chunk holding the coin
//        scans its elements in index order)
//   4-6 the draw: same search for coin * nucleus mass among keys >= the cut
//   7  the index: lowest index whose key is the drawn key
// Round 2's first version ran one 1024-thread workgroup per row through 11 passes over the
// vocabulary (607 us for 64 x 128256 logits, flat distribution; profiles/r2_sampler.md).
// ------------------------------------------------------------------------------------------------
struct SampleRow {  // per-row state (SampleScratch::state, kSampleStateWords u32)
    float m, invZ, above, nucleus;
    uint32_t prefix, cutKey;
    int mode;     // 0 done, 1 nucleus, 2 multinomial
    int counter;  // last-arriver counter of the current phase (back to 0 after each phase)
    int chunk;    // multinomial: the chunk holding the coin
    float base;   // multinomial: mass of the chunks before it
    int result;
    int pad[5];
};
static_assert(sizeof(SampleRow) == kSampleStateWords * 4, "SampleRow size");

struct SamplePhaseCtx {
    const float *l;
    int V, g, G, c0, c1;
    float T, P, coin;
    SampleRow *st;
    float *gh;    // the row's partial histograms [G][kRowBins] (every slot rewritten each pass)
    float *part;  // the row's per-chunk values [G]
    int *partI;
};

// Visit the workgroup's chunk: per round every thread loads kSampleVals elements (coalesced,
// index clamped so the loads are unconditional) before using any, so a phase costs about one
// memory round trip per 8192 elements instead of one per 256 (the first version's loop was
// latency-bound at ~25 us per phase). f(i, value, valid) runs uniformly on every lane.
static constexpr int kSampleVals = 32;
template <typename F>
__device__ __forceinline__ void forChunk(const SamplePhaseCtx &c, F f) {
    for (int r0 = c.c0; r0 < c.c1; r0 += kSampleVals * kRowWg) {
        float v[kSampleVals];
#pragma unroll
        for (int j = 0; j < kSampleVals; j++) v[j] = c.l[min(r0 + j * kRowWg + (int)threadIdx.x, c.c1 - 1)];
        __builtin_amdgcn_sched_barrier(0);  // all loads issued before the first use
#pragma unroll
        for (int j = 0; j < kSampleVals; j++) {
            const int i = r0 + j * kRowWg + (int)threadIdx.x;
            f(i, v[j], i < c.c1);
        }
    }
}

// One radix pass (digit `pass` of 0..2) of a search for `target` among candidates with
// p >= cutoff and key >= minKey whose key matches st->prefix above this digit.
__device__ void sampleRadixPass(const SamplePhaseCtx &c, int pass, bool draw, float *h, float *red, int *flag) {
    const int tid = threadIdx.x;
    const int shift = pass == 0 ? 21 : (pass == 1 ? 10 : 0);
    const uint32_t width = pass == 2 ? 10 : 11, mask = (1u << width) - 1u;
    SampleRow *st = c.st;
    const float invT = 1.0f / c.T, m = st->m, invZ = st->invZ;
    const float cutoff = (1.0f - c.P) / (float)(c.V - 1);
    const uint32_t minKey = draw ? st->cutKey : 0u;
    const uint32_t prefix = pass == 0 ? 0u : st->prefix;
    const int hiShift = shift + (int)width;  // bits above this digit (32 for pass 0)
    float *hw = h + (tid >> 6) * kRowBins;  // this wave's histogram
    for (int i = tid; i < kRowBins * kRowWaves; i += kRowWg) h[i] = 0.f;
    __syncthreads();
    forChunk(c, [&](int, float lv, bool act) {
        const float x = lv * invT;
        const float p = __expf(x - m) * invZ;
        const uint32_t k = orderKey(x);
        act = act && p >= cutoff && k >= minKey;
        if (hiShift < 32) act = act && (k >> hiShift) == (prefix >> hiShift);
        histAddWave(hw, act, (k >> shift) & mask, p);
    });
    __syncthreads();
    histStorePartial(h, c.gh + (size_t)c.g * kRowBins);
    if (!splitArrive(&st->counter, c.G, flag)) return;
    // ---- last arriver: the G partial histograms summed in workgroup order, then the bin where
    // the descending cumulative mass crosses the target
    constexpr int PER = kRowBinsPer;
    histSumPartials(c.gh, c.G, h);
    float v[PER];
    const float higher = suffixAbove(h, red, v);  // mass of the bins of higher threads
    const float above0 = pass == 0 ? 0.f : st->above;
    const float target = draw ? st->nucleus * c.coin : c.P;
    const float t = target - above0;
    // highest bin b with (mass of bins > b) + v[b] > t
    int sel = -1;
    float selAbove = 0.f, acc = higher;
#pragma unroll
    for (int j = PER - 1; j >= 0; j--) {
        if (sel < 0 && v[j] > 0.f && acc + v[j] > t) {
            sel = tid * PER + j;
            selAbove = acc;
        }
        acc += v[j];
    }
    // lowest non-empty bin, for a target never exceeded (rounding)
    int low = 0x7fffffff;
    float lowAbove = 0.f;
    acc = higher;
#pragma unroll
    for (int j = PER - 1; j >= 0; j--) {
        if (v[j] > 0.f) {
            low = tid * PER + j;
            lowAbove = acc;
        }
        acc += v[j];
    }
    __shared__ int sSel[2];
    __shared__ float sAbove[2];
    if (tid == 0) {
        sSel[0] = -1;
        sSel[1] = 0x7fffffff;
    }
    __syncthreads();
    if (sel >= 0) atomicMax(&sSel[0], sel);
    if (low != 0x7fffffff) atomicMin(&sSel[1], low);
    __syncthreads();
    const int bin = sSel[0] >= 0 ? sSel[0] : sSel[1];
    if (bin != 0x7fffffff && bin / PER == tid) {  // the bin's owner publishes its numbers
        sAbove[0] = sSel[0] >= 0 ? selAbove : lowAbove;
        float bm = 0.f;
#pragma unroll
        for (int j = 0; j < PER; j++)
            if (tid * PER + j == bin) bm = v[j];
        sAbove[1] = bm;
    }
    __syncthreads();
    if (tid == 0 && bin != 0x7fffffff) {
        const float binMass = sAbove[1];
        st->prefix = prefix | ((uint32_t)bin << shift);
        st->above = above0 + sAbove[0];
        if (pass == 2) {
            if (!draw) {
                st->cutKey = st->prefix;
                st->nucleus = st->above + binMass;  // mass of keys >= the cut
            }
        }
    }
}

template <int PHASE>
__global__ __launch_bounds__(kRowWg) void samplePhaseKernel(SampleArgs a) {
    __shared__ float h[kRowBins * kRowWaves];  // one histogram per wave (32 KB)
    __shared__ float red[kRowWaves + 2];
    __shared__ int flag[1];
    const int g = blockIdx.x, b = blockIdx.y, G = gridDim.x, tid = threadIdx.x, V = a.vocab;
    SampleRow *st = reinterpret_cast<SampleRow *>(a.scratch.state) + b;
    const float4 sp = a.spec[b];
    SamplePhaseCtx c;
    c.l = a.logits + (size_t)b * V;
    c.V = V;
    c.g = g;
    c.G = G;
    const int C = (V + G - 1) / G;
    c.c0 = min(g * C, V);
    c.c1 = min(c.c0 + C, V);
    c.T = sp.x;
    c.P = sp.y;
    c.coin = sp.z;
    c.st = st;
    c.gh = a.scratch.hist + (size_t)b * G * kRowBins;
    c.part = a.scratch.part + (size_t)b * G;
    c.partI = a.scratch.partI + (size_t)b * G;
    const bool multinomial = c.P <= 0.f || c.P >= 1.f;

    if constexpr (PHASE == 0) {
        if (c.T < 0.f) {
            if (g == 0 && tid == 0) {
                a.ids[b] = -1;
                st->mode = 0;
            }
            return;
        }
        if (c.T == 0.f) {  // greedy row: lowest index of the maximum
            float bv = -INFINITY;
            int bi = 0x7fffffff;
            forChunk(c, [&](int i, float lv, bool ok) {
                if (ok) argBetter(bv, bi, lv, i);
            });
            const float mv = wgReduce(bv, red, [](float x, float y) { return fmaxf(x, y); });
            if (tid == 0) flag[0] = 0x7fffffff;
            __syncthreads();
            if (bv == mv && bi != 0x7fffffff) atomicMin(&flag[0], bi);
            __syncthreads();
            if (tid == 0) {
                wtStore(&c.part[g], mv);
                wtStore(&c.partI[g], flag[0]);
            }
            if (!splitArrive(&st->counter, G, flag)) return;
            if (tid == 0) {
                float best = -INFINITY;
                int bestI = 0x7fffffff;
                for (int j = 0; j < G; j++) {
                    const float pv = wtLoad(&c.part[j]);
                    const int pi = wtLoad(&c.partI[j]);
                    if (pi != 0x7fffffff) argBetter(best, bestI, pv, pi);
                }
                a.ids[b] = bestI == 0x7fffffff ? 0 : bestI;
                st->mode = 0;
            }
            return;
        }
        // online max / sum of exp(x - max) over the chunk
        const float invT = 1.0f / c.T;
        float mx = -INFINITY, sm = 0.f;
        forChunk(c, [&](int, float lv, bool ok) {
            const float x = lv * invT;
            if (!ok) return;
            if (x > mx) {
                sm = sm * __expf(mx - x) + 1.f;
                mx = x;
            } else if (x != -INFINITY) {  // a masked candidate (launchLogitFilter): -inf - -inf is NaN
                sm += __expf(x - mx);
            }
        });
        const float M = wgReduce(mx, red, [](float x, float y) { return fmaxf(x, y); });
        const float S = wgReduce(mx == -INFINITY ? 0.f : sm * __expf(mx - M), red, [](float x, float y) { return x + y; });
        if (tid == 0) {
            wtStore(&c.part[g], M);
            wtStore(&c.partI[g], __float_as_int(S));
        }
        if (!splitArrive(&st->counter, G, flag)) return;
        if (tid == 0) {
            float gm = -INFINITY;
            for (int j = 0; j < G; j++) gm = fmaxf(gm, wtLoad(&c.part[j]));
            float z = 0.f;
            for (int j = 0; j < G; j++) {
                const float pm = wtLoad(&c.part[j]);
                const float ps = __int_as_float(wtLoad(&c.partI[j]));
                if (pm != -INFINITY) z += ps * __expf(pm - gm);
            }
            st->m = gm;
            st->invZ = 1.0f / z;
            st->mode = multinomial ? 2 : 1;
            st->result = 0x7fffffff;
        }
        return;
    } else {
        if (st->mode == 0) return;
        if (st->mode == 2) {  // multinomial in index order
            const float invT = 1.0f / c.T, m = st->m, invZ = st->invZ;
            if constexpr (PHASE == 1) {
                float s = 0.f;
                forChunk(c, [&](int, float lv, bool ok) {
                    if (ok) s += __expf(lv * invT - m) * invZ;
                });
                s = wgReduce(s, red, [](float x, float y) { return x + y; });
                if (tid == 0) wtStore(&c.part[g], s);
                if (!splitArrive(&st->counter, G, flag)) return;
                if (tid == 0) {
                    float base = 0.f;
                    int ch = -1;
                    for (int j = 0; j < G; j++) {
                        const float pj = wtLoad(&c.part[j]);
                        if (ch < 0 && c.coin >= base && c.coin < base + pj) {
                            ch = j;
                            break;
                        }
                        base += pj;
                    }
                    st->chunk = ch;
                    st->base = base;
                    if (ch < 0) {  // the coin fell past the total mass (rounding): last token
                        a.ids[b] = V - 1;
                        st->mode = 0;
                    }
                }
            } else if constexpr (PHASE == 2) {
                if (g != st->chunk) return;
                // thread t owns a contiguous sub-range of the chunk (index order)
                const int n = c.c1 - c.c0, per = (n + kRowWg - 1) / kRowWg;
                const int i0 = c.c0 + min(tid * per, n), i1 = c.c0 + min(tid * per + per, n);
                // the thread's run, loaded at once (per <= kSampleVals for the chunk sizes used)
                float pv[kSampleVals];
                float s = 0.f;
#pragma unroll
                for (int k = 0; k < kSampleVals; k++) pv[k] = c.l[min(i0 + k, c.c1 - 1)];
#pragma unroll
                for (int k = 0; k < kSampleVals; k++) {
                    pv[k] = __expf(pv[k] * invT - m) * invZ;
                    if (i0 + k < i1) s += pv[k];
                }
                if (per > kSampleVals)  // large chunks (few rows, small G): the rest one by one
                    for (int i = i0 + kSampleVals; i < i1; i++) s += __expf(c.l[i] * invT - m) * invZ;
                float inc = s;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const float y = __shfl_up(inc, off);
                    if ((tid & 63) >= off) inc += y;
                }
                if ((tid & 63) == 63) red[tid >> 6] = inc;
                if (tid == 0) flag[0] = c.c1 - 1;
                __syncthreads();
                float base = st->base + inc - s;
                for (int w = 0; w < (tid >> 6); w++) base += red[w];
                if (i1 > i0 && c.coin >= base && c.coin < base + s) {
                    float cdf = base;
                    int pick = -1;
#pragma unroll
                    for (int k = 0; k < kSampleVals; k++)
                        if (pick < 0 && i0 + k < i1) {
                            cdf += pv[k];
                            if (c.coin < cdf) pick = i0 + k;
                        }
                    for (int i = i0 + kSampleVals; pick < 0 && i < i1; i++) {
                        cdf += __expf(c.l[i] * invT - m) * invZ;
                        if (c.coin < cdf) pick = i;
                    }
                    atomicMin(&flag[0], pick < 0 ? i1 - 1 : pick);
                }
                __syncthreads();
                if (tid == 0) {
                    a.ids[b] = flag[0];
                    st->mode = 0;
                }
            }
            return;
        }
        // nucleus rows
        if constexpr (PHASE >= 1 && PHASE <= 6) {
            sampleRadixPass(c, (PHASE - 1) % 3, PHASE >= 4, h, red, flag);
        } else if constexpr (PHASE == 7) {
            const float invT = 1.0f / c.T;
            const uint32_t key = st->prefix;
            if (tid == 0) flag[0] = 0x7fffffff;
            __syncthreads();
            int mine = 0x7fffffff;
            forChunk(c, [&](int i, float lv, bool ok) {
                if (ok && orderKey(lv * invT) == key) mine = min(mine, i);
            });
            if (mine != 0x7fffffff) atomicMin(&flag[0], mine);
            __syncthreads();
            if (tid == 0 && flag[0] != 0x7fffffff) atomicMin(&st->result, flag[0]);
            if (!splitArrive(&st->counter, G, flag)) return;
            if (tid == 0) {
                const int r = wtLoad(&st->result);
                a.ids[b] = r == 0x7fffffff ? 0 : r;
                st->mode = 0;
            }
        }
    }
}

int sampleGroups(int B) {
    int G = 1024 / (B > 0 ? B : 1);
    return G < 8 ? 8 : (G > kSampleMaxGroups ? kSampleMaxGroups : G);
}

template <int... PHASE>
static void launchSamplePhases(const SampleArgs &a, dim3 grid, hipStream_t s, std::integer_sequence<int, PHASE...>) {
    ([&] { hipLaunchKernelGGL(samplePhaseKernel<PHASE>, grid, dim3(kRowWg), 0, s, a); }(), ...);
}

void launchSample(const SampleArgs &a, int B, hipStream_t s) {
    launchSamplePhases(a, dim3(sampleGroups(B), B), s, std::make_integer_sequence<int, 8>{});  // phases 0..7 in order
}

// (preloadModules: any kernel of this code object)
const void *sampleModuleKernel() { return (const void *)argmaxKernel; }

}  // namespace hipk
}  // namespace dl
