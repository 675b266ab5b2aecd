// Device-side pieces the row-block prefill attention kernels share (attn_prefill.hip: bf16 and f32
// caches; attn_fp8.hip: e4m3 caches): the workgroup shape and the split epilogue.
#pragma once

#include "decode_dev.h"

namespace dl {
namespace hipk {

static constexpr int kPfThreads = 256, kPfWaves = 4;

// Shared tail of the prefill kernels: normalize and store (one chunk), or publish the chunk's
// partials and let the last-arriving chunk combine them. wts ([64 columns][nSplit]) and tot ([64])
// reuse the workgroup's K / V tile LDS.
template <int HS>
__device__ __forceinline__ void pfFinish(const AttnArgs &a, int nRows, const f32x4 (&o)[HS / 16], float m, float lsum,
                                         int nSplit, int rb, int g, int c, int b0, int row, int head, float *wts,
                                         float *tot, int &flagL) {
    constexpr int NT = HS / 16;
    const int tid = threadIdx.x, lane = tid & 63, h = lane >> 4;
    const int kvMul = a.kvMul, rpb = kPfWaves * (16 / kvMul), nKv = a.nHeads0 / kvMul;
    const bool rowOk = row < nRows;
    lsum += __shfl_xor(lsum, 16);
    lsum += __shfl_xor(lsum, 32);
    // O^T accumulators: lane holds O[column][dim 16 n + 4 h + i]
    auto writeOut = [&](int r, int hd, int d, const float (&v)[4]) {
        const size_t at = (size_t)r * a.ldOut + (size_t)hd * HS + d;
        if (a.outH) {
            typedef _Float16 h4 __attribute__((ext_vector_type(4)));
            *reinterpret_cast<h4 *>(a.outH + at) = h4{(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]};
        } else {
            *reinterpret_cast<float4 *>(a.out + at) = make_float4(v[0], v[1], v[2], v[3]);
        }
    };
    if (nSplit == 1) {
        if (rowOk) {
            const float il = lsum > 0.f ? 1.0f / lsum : 0.f;
#pragma unroll
            for (int n = 0; n < NT; n++) {
                const float v[4] = {o[n][0] * il, o[n][1] * il, o[n][2] * il, o[n][3] * il};
                writeOut(row, head, 16 * n + 4 * h, v);
            }
        }
        return;
    }
    // several chunks: publish (every column of the block, masked ones as (-inf, 0, 0)), count in,
    // the last arriver combines
    const int G = a.splitGrid;
    // fence-free hand-off (splitArrive, decode_common.h)
    if (rowOk) {
        const size_t pb = ((size_t)row * a.nHeads0 + head) * G + c;
#pragma unroll
        for (int n = 0; n < NT; n++)
#pragma unroll
            for (int e = 0; e < 4; e++) wtStore(a.partO + pb * HS + 16 * n + 4 * h + e, o[n][e]);
        if (h == 0) {
            wtStore(a.partML + pb * 2, m);
            wtStore(a.partML + pb * 2 + 1, lsum);
        }
    }
    // splitArrive (decode_common.h), open-coded: the call compiles to other code in this kernel
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int *cnt = a.counters + (size_t)rb * nKv + g;
    if (tid == 0) flagL = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nSplit - 1;
    __syncthreads();
    if (!flagL) return;
    if (tid == 0) __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // per column: chunk weights exp(m_c - M) and the total sum (LDS: the tiles are free now)
    const int nCol = rpb * kvMul;  // 64 columns
    if (tid < nCol) {
        const int r = b0 + tid / kvMul, hd = g * kvMul + tid % kvMul;
        float M = -INFINITY, L = 0.f;
        if (r < nRows) {
            const float *ml = a.partML + ((size_t)r * a.nHeads0 + hd) * G * 2;
            for (int cc = 0; cc < nSplit; cc++) M = fmaxf(M, wtLoad(ml + 2 * cc));
            for (int cc = 0; cc < nSplit; cc++) {
                const float mc = wtLoad(ml + 2 * cc);
                const float w = (M == -INFINITY || mc == -INFINITY) ? 0.f : __expf(mc - M);
                wts[tid * nSplit + cc] = w;
                L += w * wtLoad(ml + 2 * cc + 1);
            }
        }
        tot[tid] = L;
    }
    __syncthreads();
    for (int i = tid; i < nCol * (HS / 4); i += kPfThreads) {
        const int cl = i / (HS / 4), d = (i % (HS / 4)) * 4;
        const int r = b0 + cl / kvMul, hd = g * kvMul + cl % kvMul;
        if (r >= nRows) continue;
        const float *po = a.partO + ((size_t)r * a.nHeads0 + hd) * G * HS + d;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int cc = 0; cc < nSplit; cc++) {
            const float w = wts[cl * nSplit + cc];
            const float *x = po + (size_t)cc * HS;
            acc[0] += w * wtLoad(x); acc[1] += w * wtLoad(x + 1); acc[2] += w * wtLoad(x + 2); acc[3] += w * wtLoad(x + 3);
        }
        const float il = tot[cl] > 0.f ? 1.0f / tot[cl] : 0.f;
        const float v[4] = {acc[0] * il, acc[1] * il, acc[2] * il, acc[3] * il};
        writeOut(r, hd, d, v);
    }
}

}  // namespace hipk
}  // namespace dl
