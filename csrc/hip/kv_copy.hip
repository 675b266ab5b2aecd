// Prefix copy between KV slots (kernels.h KvCopyArgs): positions [0, n) of srcSlot to dstSlot for
// K and V of every layer and every local KV head in one launch. Both addresses go through kvOff,
// so the same kernel serves the contiguous cache [slot][kvh][pos][hs] and the paged pool
// [page][kvh][pagePos][hs] with arbitrary source and destination pages.
//
// A pure byte stream: for one (layer, K|V, KV head) the positions of a chunk are contiguous on both
// sides (a chunk never crosses a page), so a workgroup copies chunkPos * hs elements front to back
// with 16-byte accesses, lane i at base + 16 i (1 KiB per wave instruction), four loads issued
// before their stores (16 KiB in flight per workgroup). The page ids of a chunk are looked up once,
// by uniform addresses, not per position.
#include "../core/common.h"
#include "device_comm.h"
#include "kernels.h"

namespace dl {
namespace hipk {

namespace {

constexpr int kCopyThreads = 256;
constexpr int kCopyUnroll = 4;
constexpr int kCopyChunkBytes = 64 * 1024;  // per workgroup (and per page when pages are smaller)

typedef unsigned int Vec16 __attribute__((ext_vector_type(4)));  // one 16-byte access

// V: the access type, Vec16 when a head row (hs * elemBytes) is a multiple of 16 bytes, else the
// cache element itself (every head vector starts at a multiple of its own size from the
// allocation's base, so V-sized accesses are always aligned)
template <typename V>
__global__ __launch_bounds__(kCopyThreads) void kvCopyPrefixKernel(KvCopyArgs a) {
    const int run = blockIdx.y;  // (layer * 2 + K|V) * nKv + KV head
    const int kvh = run % a.nKv;
    const int p0 = blockIdx.x * a.chunkPos;
    const int cnt = min(a.chunkPos, a.n - p0);
    if (cnt <= 0) return;
    // the bases come out of a pointer table: tell the compiler they are global memory (global_load /
    // global_store, not flat accesses)
    typedef V __attribute__((address_space(1))) GV;
    const uintptr_t base = reinterpret_cast<uintptr_t>(a.bases[run / a.nKv]);
    const size_t so = kvOff(a.kvMap, a.seqLen, a.nKv, a.hs, a.srcSlot, p0, kvh) * (size_t)a.elemBytes;
    const size_t dof = kvOff(a.kvMap, a.seqLen, a.nKv, a.hs, a.dstSlot, p0, kvh) * (size_t)a.elemBytes;
    const GV *__restrict__ src = reinterpret_cast<const GV *>(base + so);
    GV *__restrict__ dst = reinterpret_cast<GV *>(base + dof);
    const int nv = (int)((size_t)cnt * a.hs * a.elemBytes / sizeof(V));
    constexpr int kStep = kCopyThreads * kCopyUnroll;
    int i0 = 0;
    for (; i0 + kStep <= nv; i0 += kStep) {  // whole steps: every lane in bounds, loads before stores
        V r[kCopyUnroll];
#pragma unroll
        for (int u = 0; u < kCopyUnroll; u++) r[u] = src[i0 + u * kCopyThreads + threadIdx.x];
#pragma unroll
        for (int u = 0; u < kCopyUnroll; u++) dst[i0 + u * kCopyThreads + threadIdx.x] = r[u];
    }
    for (int i = i0 + threadIdx.x; i < nv; i += kCopyThreads) dst[i] = src[i];  // the last partial step
}

}  // namespace

int kvCopyChunkPos(int hs, int elemBytes, int pageShift) {
    int c = 1;
    while (2 * c * hs * elemBytes <= kCopyChunkBytes) c *= 2;
    return pageShift > 0 ? std::min(c, 1 << pageShift) : c;
}

void launchKvCopyPrefix(const KvCopyArgs &a, hipStream_t s) {
    DL_CHECK(a.n >= 1 && a.n <= a.seqLen && a.srcSlot != a.dstSlot && a.chunkPos >= 1, "kvCopyPrefix: bad arguments");
    DL_CHECK(!a.kvMap.table || a.chunkPos <= (1 << a.kvMap.pageShift), "kvCopyPrefix: a chunk crosses a page");
    const dim3 grid((a.n + a.chunkPos - 1) / a.chunkPos, a.nLayers * 2 * a.nKv);
    DL_CHECK(grid.y <= 65535, "kvCopyPrefix: too many (layer, head) runs for one launch");
    const int rowBytes = a.hs * a.elemBytes;
    if (rowBytes % 16 == 0)
        hipLaunchKernelGGL(kvCopyPrefixKernel<Vec16>, grid, dim3(kCopyThreads), 0, s, a);
    else if (a.elemBytes == 4)
        hipLaunchKernelGGL(kvCopyPrefixKernel<uint32_t>, grid, dim3(kCopyThreads), 0, s, a);
    else
        hipLaunchKernelGGL(kvCopyPrefixKernel<uint16_t>, grid, dim3(kCopyThreads), 0, s, a);
    DL_HIP(hipGetLastError());
}

}  // namespace hipk
}  // namespace dl
