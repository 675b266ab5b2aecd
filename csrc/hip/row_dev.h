// Building blocks of the row kernels over a [B][vocab] logits buffer (sample.hip, logit_filter.hip,
// logprobs.hip, logit_proc.hip): 256 threads, G workgroups per row, and what the row's workgroups
// hand to its last arriver goes through wtStore / splitArrive / wtLoad (decode_common.h).
#pragma once

#include "decode_common.h"

namespace dl {
namespace hipk {

static constexpr int kRowWg = 256;
static constexpr int kRowWaves = kRowWg / 64;
static constexpr int kRowBins = 2048;                 // one radix digit (11/11/10-bit passes)
static constexpr int kRowBinsPer = kRowBins / kRowWg;  // 8 consecutive bins per thread

// order-preserving key of x (-0.0 below +0.0), and the same with -0.0 folded onto +0.0
__device__ __forceinline__ uint32_t orderKey(float x) {
    const uint32_t u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ uint32_t orderKeyFolded(float x) { return x == 0.f ? 0x80000000u : orderKey(x); }

// Workgroup reduction in a fixed order (wave butterfly, then the waves in wave order), in every
// thread. No trailing barrier: the leading one of the next call orders this call's reads of `red`
// before its writes, and no caller touches `red` otherwise before its next barrier.
template <typename F>
__device__ __forceinline__ float wgReduce(float v, float *red, F op) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = op(v, __shfl_xor(v, off));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = red[0];
#pragma unroll
    for (int w = 1; w < kRowWaves; w++) r = op(r, red[w]);
    return r;
}

// h[bin] += w of the active lanes, h one wave's LDS histogram. Lanes that share the first active
// lane's bin are combined and added once (three times), the rest add directly: a flat distribution
// puts nearly every element of the top-digit pass in a few bins, where per-lane LDS atomics would
// serialise 64-fold. float: w summed by a butterfly; uint32_t: w is 1, a ballot's popcount.
template <typename T>
__device__ __forceinline__ void histAddWave(T *h, bool act, uint32_t bin, T w) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int rep = 0; rep < 3; rep++) {
        const unsigned long long am = __ballot(act);
        if (am == 0ull) return;
        const int leader = __builtin_ctzll(am);
        const uint32_t b0 = __shfl(bin, leader);
        const bool mine = act && bin == b0;
        T v;
        if constexpr (std::is_same<T, float>::value) {
            v = mine ? w : 0.f;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
        } else {
            v = (T)__builtin_popcountll(__ballot(mine));
        }
        if (lane == leader) atomicAdd(&h[b0], v);
        act = act && !mine;
    }
    if (act) atomicAdd(&h[bin], w);
}

// The workgroup's histogram (h: one copy per wave, summed in wave order) -> its partial slot;
// lane-consecutive bins: every store instruction is one 1 KB run.
template <typename T>
__device__ __forceinline__ void histStorePartial(const T *h, T *slot) {
#pragma unroll
    for (int j = 0; j < kRowBinsPer; j++) {
        const int bin = j * kRowWg + (int)threadIdx.x;
        T v = 0;
#pragma unroll
        for (int w = 0; w < kRowWaves; w++) v += h[w * kRowBins + bin];
        wtStore(&slot[bin], v);
    }
}

// Last arriver: the row's G partial slots summed in workgroup order (deterministic for float) into
// h[0, kRowBins), the loads of 4 slots in flight before their adds; ends with a barrier.
template <typename T>
__device__ __forceinline__ void histSumPartials(const T *slots, int G, T *h) {
    const int tid = threadIdx.x;
    T acc8[kRowBinsPer];
#pragma unroll
    for (int j = 0; j < kRowBinsPer; j++) acc8[j] = 0;
    for (int g0 = 0; g0 < G; g0 += 4) {
        T t4[4][kRowBinsPer];
#pragma unroll
        for (int q = 0; q < 4; q++)
#pragma unroll
            for (int j = 0; j < kRowBinsPer; j++)
                t4[q][j] = wtLoad(&slots[(size_t)min(g0 + q, G - 1) * kRowBins + j * kRowWg + tid]);
#pragma unroll
        for (int q = 0; q < 4; q++)
            if (g0 + q < G)
#pragma unroll
                for (int j = 0; j < kRowBinsPer; j++) acc8[j] += t4[q][j];
    }
#pragma unroll
    for (int j = 0; j < kRowBinsPer; j++) h[j * kRowWg + tid] = acc8[j];
    __syncthreads();
}

// v = this thread's 8 bins of h (bins 8 tid ...); returns the total of the bins of higher threads
// (exclusive suffix over threads; wave totals through wtot[kRowWaves]).
template <typename T>
__device__ __forceinline__ T suffixAbove(const T *h, T *wtot, T (&v)[kRowBinsPer]) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    T tot = 0;
#pragma unroll
    for (int j = 0; j < kRowBinsPer; j++) {
        v[j] = h[tid * kRowBinsPer + j];
        tot += v[j];
    }
    T inc = tot;  // inclusive suffix within the wave (lanes >= this lane)
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T y = __shfl_down(inc, off);
        if (lane + off < 64) inc += y;
    }
    if (lane == 0) wtot[wv] = inc;
    __syncthreads();
    T higher = inc - tot;
    for (int w = wv + 1; w < kRowWaves; w++) higher += wtot[w];
    return higher;
}

// A workgroup's share of its row, in every launch over the row: the row is cut into 16-byte vectors,
// workgroup g owns the vectors [g * vpg, (g + 1) * vpg) and the last workgroup also the vocab % 4
// scalar tail. Rows of a [B][vocab] buffer start on 4-byte boundaries when vocab % 4 != 0, so the
// vectors are typed with 4-byte alignment (global 16-byte accesses need no more).
static constexpr int kRowU = 4;  // vectors in flight per thread per round
template <typename T>
using RowVec4 = T __attribute__((ext_vector_type(4), aligned(4)));

// Store tail of the token masks (json_mask.hip, grammar_mask.hip), one thread per token t of `row`
// with verdict ok (lanes behind the row pass true), called by every lane of the wave: the verdicts of
// four neighbouring lanes meet through a ballot in the lane of the vector's first element: all
// allowed - nothing is touched; none - one 16-byte store of -inf; mixed - the vector is loaded, the
// rejected elements replaced and the vector stored. The vocab % 4 tail is stored per element.
__device__ __forceinline__ void maskStoreTail(float *row, int t, int vocab, bool ok) {
    const int lane = (int)threadIdx.x & 63;
    const unsigned long long verdicts = __ballot(ok);
    if ((t | 3) < vocab) {  // the whole vector lies in the row: its first lane stores it
        if ((lane & 3) != 0) return;
        const unsigned keep = (unsigned)(verdicts >> lane) & 0xfu;
        if (keep == 0xfu) return;
        RowVec4<float> *p = reinterpret_cast<RowVec4<float> *>(row + t);
        RowVec4<float> v;
        if (keep != 0u) v = *p;
        if (!(keep & 1u)) v.x = -INFINITY;
        if (!(keep & 2u)) v.y = -INFINITY;
        if (!(keep & 4u)) v.z = -INFINITY;
        if (!(keep & 8u)) v.w = -INFINITY;
        *p = v;
    } else if (t < vocab && !ok) {
        row[t] = -INFINITY;
    }
}

struct RowShare {
    int v0, v1;  // vectors
    int nvec, vocab;
    bool tailOwner;
    __device__ bool owns(int e) const { return e >= 4 * nvec ? tailOwner : (e / 4 >= v0 && e / 4 < v1); }
};

__device__ __forceinline__ RowShare rowShare(int vocab) {
    RowShare s;
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
__device__ __forceinline__ void forShare(const float *x, const RowShare &s, F f) {
    for (int r0 = s.v0; r0 < s.v1; r0 += kRowU * kRowWg) {
        RowVec4<float> v[kRowU];
#pragma unroll
        for (int u = 0; u < kRowU; u++)
            v[u] = reinterpret_cast<const RowVec4<float> *>(x)[min(r0 + u * kRowWg + (int)threadIdx.x, s.v1 - 1)];
#pragma unroll
        for (int u = 0; u < kRowU; u++) {
            const bool ok = r0 + u * kRowWg + (int)threadIdx.x < s.v1;
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

// out[e] = f(a[e], b[e]) for every element e of the share (out may be a): kRowU vectors of each
// stream are loaded before the first is used. One stream: pass it twice (the loads are the same).
template <typename B, typename F>
__device__ __forceinline__ void mapShare(const RowShare &s, float *out, const float *a, const B *b, F f) {
    for (int i0 = s.v0 + (int)threadIdx.x; i0 < s.v1; i0 += kRowU * kRowWg) {
        RowVec4<float> x[kRowU];
        RowVec4<B> c[kRowU];
#pragma unroll
        for (int u = 0; u < kRowU; u++) {
            const int i = i0 + u * kRowWg;
            if (i < s.v1) {
                x[u] = reinterpret_cast<const RowVec4<float> *>(a)[i];
                c[u] = reinterpret_cast<const RowVec4<B> *>(b)[i];
            }
        }
#pragma unroll
        for (int u = 0; u < kRowU; u++) {
            const int i = i0 + u * kRowWg;
            if (i < s.v1) {
                RowVec4<float> y;
                y.x = f(x[u].x, c[u].x);
                y.y = f(x[u].y, c[u].y);
                y.z = f(x[u].z, c[u].z);
                y.w = f(x[u].w, c[u].w);
                reinterpret_cast<RowVec4<float> *>(out)[i] = y;
            }
        }
    }
    if (s.tailOwner) {
        const int e = 4 * s.nvec + (int)threadIdx.x;
        if (e < s.vocab) out[e] = f(a[e], b[e]);
    }
}

}  // namespace hipk
}  // namespace dl
