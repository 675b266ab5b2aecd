// Ragged prefill attention for f32 KV caches: row blocks that start at any row and have any length.
//
// The row-block prefill kernels (attn_prefill.hip) cut a forward into aligned blocks of rpb = 64 / KM
// rows and need every block in one slot, so a serving forward of d decode rows ahead of a prompt chunk
// (d no multiple of rpb), or of two requests' chunks, falls back to the per-row decode kernel and reads
// a prompt row's context once per row. Here the host cuts the rows into *segments* - maximal runs of at
// most rpb consecutive rows of one slot (attnRaggedSegments) - and a workgroup owns one (segment, KV
// head, key chunk): grid (nKv * nRows, splitGrid), the worst case of one segment per row, so a captured
// graph stays valid while the table changes; workgroups with seg >= nSeg leave before touching memory.
//
// One kernel, two schedules, chosen per segment (uniform in the workgroup):
//   row-block   segments wider than one wave's 16 (row, head) columns (rows > 16 / KM): wave w holds
//               rows w * 16 / KM ... of the segment, every wave consumes every key of the tile
//               (attnPrefillF32Kernel's schedule);
//   key-split   narrower segments (decode rows, chunk tails): the rows fit one wave's columns, so all
//               four waves hold the same columns and wave w takes keys [16 w, 16 w + 16) of every
//               64-key tile; the waves' (max, sum, O) merge through LDS in wave order at the end, as
//               attnDecodeF32MfmaKernel merges its waves. Without it a decode row would leave three
//               waves idle.
// Both run v_mfma_f32_16x16x4_f32 with the operand roles of attnPrefillF32Kernel: S^T = K . Q^T (lane
// (col, h) holds K[key 16 u + col][QD h + e] and Q[column col][QD h + e]), the online softmax on the
// S^T accumulators (lane holds S[key 16 u + 4 h + i][col]), O^T += V^T . P^T with P staying in place.
//
// LDS image: the padded row-major image of attn_prefill.hip (row stride HS + 4 floats), not the
// XOR-swizzled DMA image of attn_mfma_f32.hip. The DMA image is private to a wave (each wave issues
// and counts its own tiles), which suits the key-split schedule only; the row-block schedule needs one
// tile that all four waves read, staged by all 256 threads. With the padded image both schedules share
// one staging path (global -> registers -> LDS, the next tile's loads in flight during the MFMAs) and
// one set of LDS read addresses; they differ only in which rows of the tile a wave multiplies. The tile
// is 64 keys for both (16 per wave in the key-split schedule): 2 x 64 x (HS + 4) floats, 66 KB at head
// size 128, two workgroups per CU.
//
// Keys split into chunks of ~256 over grid.y by attnPrefillSplit with a fixed chunk size (a row's
// result must not depend on what else is in the launch); chunks publish partials and the last arriver
// combines them (pfFinish, attn_prefill_dev.h, called with the segment's end as the row bound and the
// segment index as the counter row). Paged caches: the chunk's page ids go to LDS once. Outputs f32 or
// f16; like the prefill kernels this one has no Q80 writer, and the launcher refuses outQ.
#include "attn_prefill_dev.h"

#include <string>

namespace dl {
namespace hipk {

static constexpr int kRgTile = 64, kRgSub = kAttnPrefillTile, kRgChunk = kAttnPrefillChunk;
static constexpr int kRgMaxSubs = 256;  // 32-key page entries per chunk in LDS
__host__ __device__ constexpr size_t rgLdsBytes(int hs) {
    return (size_t)2 * kRgTile * (hs + 4) * sizeof(float) + kRgMaxSubs * sizeof(int) + 16;
}

template <int KM, int HS>
__global__ __launch_bounds__(kPfThreads) void attnRaggedF32Kernel(AttnArgs a) {
    constexpr int NT = HS / 16, QD = HS / 4, SR = HS + 4, RPW = 16 / KM;
    constexpr int U4 = HS / 4;                       // 16-byte units per key row
    constexpr int PER = kRgTile * U4 / kPfThreads;   // 16-byte units per thread per operand and tile
    static_assert(PER >= 1 && kRgTile * U4 % kPfThreads == 0, "tile / workgroup shape");
    static_assert(kRgTile * SR >= 64 * (HS / 2) && kRgTile * SR >= kPfWaves * 16 * (HS + 2), "combine weights / wave merge fit the K tile");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *kT = reinterpret_cast<float *>(smem), *vT = kT + kRgTile * SR;
    int *pageL = reinterpret_cast<int *>(vT + kRgTile * SR);
    int &flagL = pageL[kRgMaxSubs];
    const int nKv = a.nHeads0 / KM;
    const int g = blockIdx.x % nKv, seg = blockIdx.x / nKv, c = blockIdx.y;
    if (seg >= a.nSeg[0]) return;  // the grid is sized for one segment per row
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 15, h = lane >> 4;
    const int b0 = a.segRow[seg], n = a.segRows[seg], bEnd = b0 + n;
    const bool rowBlock = n > RPW;
    const int maxLen = rowsMaxLen(a.pos, b0, n, bEnd);
    int nSplit, ch;
    attnPrefillSplit(maxLen, a.splitGrid, HS, kRgChunk, nSplit, ch);
    if (c >= nSplit) return;
    const int k0 = c * ch, k1 = min(k0 + ch, maxLen);
    const int sl = a.slot[b0];  // every row of the segment (attnRaggedSegments)
    // this lane's column: the key-split waves all hold the segment's first 16 / KM rows
    const int rIn = (rowBlock ? wave * RPW : 0) + col / KM;
    const bool rowOk = rIn < n;
    const int row = b0 + rIn, head = g * KM + col % KM;
    const int myLen = rowOk ? a.pos[row] + 1 : 0;
    const float scale = 1.0f / sqrtf((float)HS);
    float q[QD];
#pragma unroll
    for (int e = 0; e < QD; e += 4) {
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (rowOk) x = ld4(a.q + (size_t)row * a.ldq + (size_t)head * HS + QD * h + e);
        q[e] = x.x * scale; q[e + 1] = x.y * scale; q[e + 2] = x.z * scale; q[e + 3] = x.w * scale;
    }
    const float *kc = reinterpret_cast<const float *>(a.kcache);
    const float *vc = reinterpret_cast<const float *>(a.vcache);
    const bool any = k0 < k1;  // attnPrefillSplit's rounding can leave the last chunk empty
    if (a.kvMap.table && any)
        for (int i = tid; i < (k1 - k0 + kRgSub - 1) / kRgSub; i += kPfThreads)
            pageL[i] = (int)kvPageOf(a.kvMap, sl, k0 + i * kRgSub);
    __syncthreads();
    f32x4 kr[PER], vr[PER];
    auto gload = [&](int t0) {
#pragma unroll
        for (int u = 0; u < PER; u++) {
            const int e = tid + u * kPfThreads;
            const int key = min(t0 + e / U4, k1 - 1);  // past the range: masked in compute (and mapped)
            const size_t blk = a.kvMap.table ? (size_t)pageL[(key - k0) / kRgSub] : (size_t)sl;
            const size_t off = kvOffAt(a.kvMap, a.seqLen, nKv, HS, blk, key, g) + (e % U4) * 4;
            kr[u] = *reinterpret_cast<const f32x4 *>(kc + off);
            vr[u] = *reinterpret_cast<const f32x4 *>(vc + off);
        }
    };
    auto lstore = [&] {
#pragma unroll
        for (int u = 0; u < PER; u++) {
            const int e = tid + u * kPfThreads, at = (e / U4) * SR + (e % U4) * 4;
            *reinterpret_cast<f32x4 *>(&kT[at]) = kr[u];
            *reinterpret_cast<f32x4 *>(&vT[at]) = vr[u];
        }
    };
    f32x4 o[NT];
#pragma unroll
    for (int n2 = 0; n2 < NT; n2++) o[n2] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, lsum = 0.f;
    // 16 NU keys from LDS row r0 on (global key t0 on) against this wave's 16 columns
    auto compute = [&](auto nuTag, int r0, int t0) {
        constexpr int NU = decltype(nuTag)::value;
        f32x4 st[NU], sx[NU];  // two accumulator chains per subtile (even / odd pieces), summed below
#pragma unroll
        for (int u = 0; u < NU; u++) st[u] = sx[u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < QD; e += 4) {
#pragma unroll
            for (int u = 0; u < NU; u++) {
                const f32x4 kf = *reinterpret_cast<const f32x4 *>(&kT[(r0 + 16 * u + col) * SR + QD * h + e]);
                f32x4 &acc = (e & 4) ? sx[u] : st[u];
#pragma unroll
                for (int j = 0; j < 4; j++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[j], q[e + j], acc, 0, 0, 0);
            }
        }
        float mx = -INFINITY;
#pragma unroll
        for (int u = 0; u < NU; u++) {
            st[u] += sx[u];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int t = t0 + 16 * u + 4 * h + i;
                if (t >= k1 || t >= myLen) st[u][i] = -INFINITY;
                mx = fmaxf(mx, st[u][i]);
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16));
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float mn = fmaxf(m, mx);
        const float corr = m == -INFINITY ? 0.f : __expf(m - mn);
        float p[4 * NU], ps = 0.f;
#pragma unroll
        for (int u = 0; u < NU; u++)
#pragma unroll
            for (int i = 0; i < 4; i++) {
                p[4 * u + i] = st[u][i] == -INFINITY ? 0.f : __expf(st[u][i] - mn);
                ps += p[4 * u + i];
            }
        lsum = lsum * corr + ps;
        m = mn;
#pragma unroll
        for (int n2 = 0; n2 < NT; n2++) o[n2] *= corr;
#pragma unroll
        for (int j = 0; j < 4 * NU; j++) {
            const float *vrow = &vT[(r0 + 16 * (j >> 2) + 4 * h + (j & 3)) * SR + col];
#pragma unroll
            for (int n2 = 0; n2 < NT; n2++) o[n2] = __builtin_amdgcn_mfma_f32_16x16x4f32(vrow[16 * n2], p[j], o[n2], 0, 0, 0);
        }
    };
    using N1 = std::integral_constant<int, 1>;
    using N2 = std::integral_constant<int, 2>;
    if (any) {
        gload(k0);
        lstore();
        __syncthreads();
        // tile t in LDS, tile t + 1's loads in flight during its MFMAs
        for (int t0 = k0; t0 < k1; t0 += kRgTile) {
            const bool more = t0 + kRgTile < k1;
            if (more) gload(t0 + kRgTile);
            if (rowBlock) {
                compute(N2{}, 0, t0);
                if (t0 + kRgSub < k1) compute(N2{}, kRgSub, t0 + kRgSub);
            } else if (t0 + 16 * wave < k1) {  // wave-uniform
                compute(N1{}, 16 * wave, t0 + 16 * wave);
            }
            __syncthreads();
            if (more) {
                lstore();
                __syncthreads();
            }
        }
    }
    int outRow = row;
    if (!rowBlock) {
        // merge the four waves' key shares of the same 16 columns (LDS: the tiles are free now), in
        // wave order on every wave; wave 0 alone carries the result into the tail
        float *oW = kT, *mW = kT + kPfWaves * 16 * HS, *lW = mW + kPfWaves * 16;  // [4][16][HS], [4][16], [4][16]
        lsum += __shfl_xor(lsum, 16);
        lsum += __shfl_xor(lsum, 32);
        if (h == 0) {
            mW[wave * 16 + col] = m;
            lW[wave * 16 + col] = lsum;
        }
#pragma unroll
        for (int n2 = 0; n2 < NT; n2++)
            *reinterpret_cast<f32x4 *>(&oW[(wave * 16 + col) * HS + 16 * n2 + 4 * h]) = o[n2];
        __syncthreads();
        float M = -INFINITY;
#pragma unroll
        for (int w = 0; w < kPfWaves; w++) M = fmaxf(M, mW[w * 16 + col]);
        float L = 0.f;
#pragma unroll
        for (int n2 = 0; n2 < NT; n2++) o[n2] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int w = 0; w < kPfWaves; w++) {
            const float mw = mW[w * 16 + col];
            const float e = mw == -INFINITY ? 0.f : __expf(mw - M);
            L += e * lW[w * 16 + col];
#pragma unroll
            for (int n2 = 0; n2 < NT; n2++) o[n2] += e * *reinterpret_cast<const f32x4 *>(&oW[(w * 16 + col) * HS + 16 * n2 + 4 * h]);
        }
        m = M;
        lsum = h == 0 ? L : 0.f;  // pfFinish sums the four lane groups' shares
        if (wave != 0) outRow = bEnd;  // not a row of the segment: nothing published or written
        __syncthreads();  // the merge's reads retire before the tail reuses the tiles
    }
    pfFinish<HS>(a, bEnd, o, m, lsum, nSplit, seg, g, c, b0, outRow, head, kT, vT, flagL);
}

int attnRaggedSegments(const int *slots, int nRows, int kvMul, int *segRow, int *segRows) {
    const int rpb = attnPrefillRowsPerBlock(kvMul);
    int nSeg = 0;
    for (int b = 0; b < nRows;) {
        int e = b + 1;
        while (e < nRows && e - b < rpb && slots[e] == slots[b]) e++;
        segRow[nSeg] = b;
        segRows[nSeg++] = e - b;
        b = e;
    }
    return nSeg;
}

bool attnRaggedRowBlock(int rows, int kvMul) { return rows > 16 / kvMul; }

bool attnRaggedSupported(const AttnArgs &a) {
    return !a.kvBf16 && !a.kvFp8 && (a.hs == 64 || a.hs == 128) && (a.kvMul == 1 || a.kvMul == 2 || a.kvMul == 4 || a.kvMul == 8) &&
           a.nHeads0 % a.kvMul == 0;
}

const char *attnRaggedRefusal(const AttnArgs &a) {
    if (a.kvBf16 || a.kvFp8) return "launchAttentionRagged: f32 KV caches only (bf16 and fp8 caches take the aligned prefill kernels)";
    if (!attnRaggedSupported(a)) return "launchAttentionRagged: head size 64 or 128 and kvMul 1, 2, 4 or 8";
    if (a.outQ) return "launchAttentionRagged: the prefill kernels ignore outQ (no Q80 output)";
    // the longest split chunk's 32-key page entries fit the kernel's LDS page list
    const int minSplits = std::max(1, std::min(a.splitGrid, a.hs / 2));
    if (a.kvMap.table && ((a.seqLen + minSplits - 1) / minSplits + kRgSub - 1) / kRgSub + 1 > kRgMaxSubs)
        return "launchAttentionRagged: paged context too long for the per-chunk page list";
    return nullptr;
}

const char *attnRaggedTableRefusal(const int *segRow, const int *segRows, int nSeg, const int *slots, int nRows, int kvMul) {
    const int rpb = attnPrefillRowsPerBlock(kvMul);
    int at = 0;
    for (int s = 0; s < nSeg; s++) {
        if (segRow[s] != at || segRows[s] < 1 || segRows[s] > rpb || at + segRows[s] > nRows)
            return "launchAttentionRagged: the segments do not tile [0, nRows)";
        for (int b = at; b < at + segRows[s]; b++)
            if (slots[b] != slots[at]) return "launchAttentionRagged: a segment spans slots";
        at += segRows[s];
    }
    return at == nRows ? nullptr : "launchAttentionRagged: the segments do not tile [0, nRows)";
}

std::string attnRaggedKernelName(const AttnArgs &a) {
    return "attnRaggedF32Kernel<" + std::to_string(a.kvMul) + "," + std::to_string(a.hs) + ">";
}

void launchAttentionRagged(const AttnArgs &a, int nRows, hipStream_t s) {
    if (const char *why = attnRaggedRefusal(a)) throw Error(why);
    if (!a.segRow || !a.segRows || !a.nSeg) throw Error("launchAttentionRagged: no segment table");
    const dim3 grid(a.nHeads0 / a.kvMul * nRows, a.splitGrid);
    const size_t lds = rgLdsBytes(a.hs);
#define DL_RG_CASE(K, H)                                                                          \
    if (a.kvMul == K && a.hs == H) {                                                              \
        if (lds > 65536) allowLds((const void *)attnRaggedF32Kernel<K, H>, lds);                  \
        hipLaunchKernelGGL((attnRaggedF32Kernel<K, H>), grid, dim3(kPfThreads), lds, s, a);       \
        return;                                                                                   \
    }
    DL_RG_CASE(1, 128) DL_RG_CASE(2, 128) DL_RG_CASE(4, 128) DL_RG_CASE(8, 128)
    DL_RG_CASE(1, 64) DL_RG_CASE(2, 64) DL_RG_CASE(4, 64) DL_RG_CASE(8, 64)
#undef DL_RG_CASE
    throw Error("launchAttentionRagged: head size 64 or 128 and kvMul 1, 2, 4 or 8");
}

// preloadModules(): one kernel of this translation unit's code object
const void *attnRaggedModuleKernel() { return (const void *)attnRaggedF32Kernel<4, 128>; }

}  // namespace hipk
}  // namespace dl
