// Pooled, L2-normalised final hidden states of a forward's rows (PoolArgs in kernels.h): what
// /v1/embeddings returns, so that dim floats per request reach the host instead of rows x dim hidden
// values (or rows x vocab logits).
//
// poolScaleKernel, grid (1, B): a taking-part row's sum of squares over in + add, per thread in
// element order, then over the workgroup in a fixed order (wgReduce) -> scale[b] = 1 / rms.
// poolKernel, grid (poolGroups(dim), B): only the workgroups of a kPoolHead row work. Workgroup g owns
// the 16-byte vectors of its share of dim (rowShare) and walks the slot's rows of this launch in
// launch order, 4 rows' loads in flight, adding h = normW * (scale * (in + add)) to the slot's
// accumulator held in registers: one unfused f32 add per element per row, whatever the launch holds
// besides. A slot whose last row is in the launch is finalised: the slice's p goes back to the
// accumulator with write-through stores, its sum of squares to `part`, and the slot's last-arriving
// workgroup (the fence-free hand-off, splitArrive in decode_common.h) sums the partials in workgroup
// order and writes p / sqrt(sum) for the whole of dim. No float atomics in memory; nothing depends
// on B, on the other slots or on the arrival order.
#include <string>
#include <vector>

#include "row_dev.h"

namespace dl {
namespace hipk {

static_assert(sizeof(PoolRow) == 32, "PoolRow layout");

int poolGroups(int dim) {
    const int G = (dim / 4 + kRowWg - 1) / kRowWg;  // one vector per thread up to kPoolMaxGroups x 1024
    return G < 1 ? 1 : (G > kPoolMaxGroups ? kPoolMaxGroups : G);
}

int poolPlan(PoolRow *rows, int *idx, int B) {
    auto fail = [](const std::string &what) { throw Error("pooling: " + what); };
    int slots = 0;
    for (int b = 0; b < B; b++) {
        rows[b].flags &= ~kPoolHead;
        rows[b].start = rows[b].len = 0;
        if (rows[b].flags & kPoolTake) {
            if (rows[b].slot < 0) fail("slot out of range");
            slots = rows[b].slot + 1 > slots ? rows[b].slot + 1 : slots;
        }
    }
    std::vector<int> head(slots, -1), lastRow(slots, -1);
    for (int b = 0; b < B; b++) {
        if (!(rows[b].flags & kPoolTake)) continue;
        const int s = rows[b].slot;
        if (head[s] < 0) {
            head[s] = b;
            rows[b].flags |= kPoolHead;
        } else {
            if (rows[b].flags & kPoolFirst) fail("a slot's first row follows another of its rows");
            if ((rows[b].flags ^ rows[head[s]].flags) & kPoolModeLast) fail("the rows of a slot disagree on the mode");
            if (rows[lastRow[s]].flags & kPoolLast) fail("a row follows its slot's last row");
        }
        if ((rows[b].flags & kPoolLast) && rows[b].count < 1) fail("the last row carries the request's row count");
        lastRow[s] = b;
        rows[head[s]].len++;
    }
    int n = 0;
    for (int b = 0; b < B; b++)  // the slots' runs, in the order of their head rows
        if (rows[b].flags & kPoolHead) {
            rows[b].start = n;
            n += rows[b].len;
            rows[b].len = 0;
        }
    for (int b = 0; b < B; b++)
        if (rows[b].flags & kPoolTake) {
            PoolRow &h = rows[head[rows[b].slot]];
            idx[h.start + h.len++] = b;
        }
    return n;
}

using PoolVec = RowVec4<float>;

__global__ __launch_bounds__(kRowWg) void poolScaleKernel(PoolArgs a) {
    __shared__ float red[kRowWaves];
    const int b = blockIdx.y;
    if (!(a.rows[b].flags & kPoolTake)) return;
    const PoolVec *x = reinterpret_cast<const PoolVec *>(a.in + (size_t)b * a.ld);
    const PoolVec *y = a.add ? reinterpret_cast<const PoolVec *>(a.add + (size_t)b * a.ld) : nullptr;
    const int nvec = a.dim / 4;
    float ss = 0.f;
    for (int v0 = 0; v0 < nvec; v0 += kRowU * kRowWg) {
        PoolVec xv[kRowU], yv[kRowU];
#pragma unroll
        for (int u = 0; u < kRowU; u++) {
            const int v = min(v0 + u * kRowWg + (int)threadIdx.x, nvec - 1);
            xv[u] = x[v];
            if (y) yv[u] = y[v];
        }
#pragma unroll
        for (int u = 0; u < kRowU; u++) {
            if (v0 + u * kRowWg + (int)threadIdx.x >= nvec) continue;
            PoolVec t = xv[u];
            if (y) t += yv[u];
            ss += t.x * t.x;
            ss += t.y * t.y;
            ss += t.z * t.z;
            ss += t.w * t.w;
        }
    }
    ss = wgReduce(ss, red, [](float p, float q) { return p + q; });
    if (threadIdx.x == 0) a.scale[b] = 1.0f / sqrtf(ss / (float)a.dim + a.eps);
}

// acc = acc + w * (sc * xs) with nothing contracted: the add is the accumulator's one rounding per row
__device__ __forceinline__ float poolAdd(float acc, float w, float sc, float xs, bool mean) {
    const float h = __fmul_rn(w, __fmul_rn(sc, xs));
    return mean ? __fadd_rn(acc, h) : h;
}

__global__ __launch_bounds__(kRowWg) void poolKernel(PoolArgs a) {
    __shared__ float red[kRowWaves];
    __shared__ int flag;
    const int g = blockIdx.x, G = gridDim.x, tid = threadIdx.x;
    const PoolRow head = a.rows[blockIdx.y];
    if (!(head.flags & kPoolHead)) return;
    const bool mean = !(head.flags & kPoolModeLast);
    const RowShare s = rowShare(a.dim);
    float *accRow = a.acc + (size_t)head.slot * a.dim;
    const int *run = a.idx + head.start;
    const PoolRow tail = a.rows[run[head.len - 1]];
    const bool finish = (tail.flags & kPoolLast) != 0;
    const float cnt = (float)tail.count;
    float ss = 0.f;
    for (int v = s.v0 + tid; v < s.v1; v += kRowWg) {  // (one round for dim <= kPoolMaxGroups x 1024)
        const PoolVec w = reinterpret_cast<const PoolVec *>(a.normW)[v];
        PoolVec p = {0.f, 0.f, 0.f, 0.f};
        if (!(head.flags & kPoolFirst)) p = reinterpret_cast<const PoolVec *>(accRow)[v];
        for (int i0 = 0; i0 < head.len; i0 += kRowU) {
            int r[kRowU];
#pragma unroll
            for (int u = 0; u < kRowU; u++) r[u] = run[min(i0 + u, head.len - 1)];
            PoolVec xv[kRowU], yv[kRowU];
            float sc[kRowU];
            int fl[kRowU];
#pragma unroll
            for (int u = 0; u < kRowU; u++) {
                xv[u] = reinterpret_cast<const PoolVec *>(a.in + (size_t)r[u] * a.ld)[v];
                if (a.add) yv[u] = reinterpret_cast<const PoolVec *>(a.add + (size_t)r[u] * a.ld)[v];
                sc[u] = a.scale[r[u]];
                fl[u] = a.rows[r[u]].flags;
            }
#pragma unroll
            for (int u = 0; u < kRowU; u++) {
                if (i0 + u >= head.len) continue;
                if (!mean && !(fl[u] & kPoolLast)) continue;  // last: only the request's last row counts
                PoolVec t = xv[u];
                if (a.add) t += yv[u];
                p.x = poolAdd(p.x, w.x, sc[u], t.x, mean);
                p.y = poolAdd(p.y, w.y, sc[u], t.y, mean);
                p.z = poolAdd(p.z, w.z, sc[u], t.z, mean);
                p.w = poolAdd(p.w, w.w, sc[u], t.w, mean);
            }
        }
        if (!finish) {
            reinterpret_cast<PoolVec *>(accRow)[v] = p;
            continue;
        }
        if (mean) {
            p.x = __fdiv_rn(p.x, cnt);
            p.y = __fdiv_rn(p.y, cnt);
            p.z = __fdiv_rn(p.z, cnt);
            p.w = __fdiv_rn(p.w, cnt);
        }
        ss += p.x * p.x;
        ss += p.y * p.y;
        ss += p.z * p.z;
        ss += p.w * p.w;
        stF2<true>(accRow + 4 * (size_t)v, p.x, p.y);  // read by the slot's last arriver
        stF2<true>(accRow + 4 * (size_t)v + 2, p.z, p.w);
    }
    if (!finish) return;
    ss = wgReduce(ss, red, [](float p, float q) { return p + q; });
    if (tid == 0) wtStore(a.part + (size_t)head.slot * kPoolMaxGroups + g, ss);
    if (!splitArrive(a.counters + head.slot, G, &flag)) return;

    // ---- the slot's last arriver: the partials in workgroup order, then the whole of dim
    float tot = 0.f;
    for (int j = 0; j < G; j++) tot += wtLoad(a.part + (size_t)head.slot * kPoolMaxGroups + j);
    const float nrm = sqrtf(tot);
    float *outRow = a.out + (size_t)head.slot * a.dim;
    for (int v = tid; v < a.dim / 4; v += kRowWg) {
        const uint64_t lo = ldWT64(accRow + 4 * (size_t)v), hi = ldWT64(accRow + 4 * (size_t)v + 2);
        PoolVec p = {__uint_as_float((uint32_t)lo), __uint_as_float((uint32_t)(lo >> 32)), __uint_as_float((uint32_t)hi),
                     __uint_as_float((uint32_t)(hi >> 32))};
        PoolVec o = {0.f, 0.f, 0.f, 0.f};
        if (tot > 0.f) {
            o.x = __fdiv_rn(p.x, nrm);
            o.y = __fdiv_rn(p.y, nrm);
            o.z = __fdiv_rn(p.z, nrm);
            o.w = __fdiv_rn(p.w, nrm);
        }
        reinterpret_cast<PoolVec *>(outRow)[v] = o;
    }
}

void launchPool(const PoolArgs &a, int B, hipStream_t s) {
    hipLaunchKernelGGL(poolScaleKernel, dim3(1, B), dim3(kRowWg), 0, s, a);
    hipLaunchKernelGGL(poolKernel, dim3(poolGroups(a.dim), B), dim3(kRowWg), 0, s, a);
}

}  // namespace hipk
}  // namespace dl
