// One-to-many prefix copy between KV slots (kernels.h KvForkArgs): positions [0, n) of srcSlot to
// every slot of dstSlots[0 .. nDst) for K and V of every layer and every local KV head in one
// launch. The geometry is kv_copy.hip's: one (layer, K|V, KV head) run per blockIdx.y, one chunk of
// chunkPos positions per workgroup, a chunk never crosses a page, every address through kvOff (the
// contiguous cache and the paged pool alike).
//
// What differs: a lane issues its kCopyUnroll 16-byte loads of the source once per step and stores
// those registers to each destination in turn, so forking m siblings reads the prefix once instead
// of m times (1 + m prefix-sized transfers where m copies move 2m). 16 KiB of loads in flight per
// workgroup, as in the copy; the stores of a step (up to kMaxForkDst x 16 KiB) drain behind the next
// step's loads. The destinations' bases are uniform: their page ids are looked up once per chunk
// per destination, not per position, and live in scalar registers (the loop over destinations is
// unrolled with a uniform guard, so no base is indexed dynamically).
#include "../core/common.h"
#include "device_comm.h"
#include "kernels.h"

namespace dl {
namespace hipk {

namespace {

constexpr int kCopyThreads = 256;
constexpr int kCopyUnroll = 4;

typedef unsigned int Vec16 __attribute__((ext_vector_type(4)));  // one 16-byte access

// V: the access type, chosen as in kvCopyPrefixKernel (Vec16 when a head row is a multiple of 16
// bytes, else the cache element itself: always aligned)
template <typename V>
__global__ __launch_bounds__(kCopyThreads) void kvForkPrefixKernel(KvForkArgs a) {
    const int run = blockIdx.y;  // (layer * 2 + K|V) * nKv + KV head
    const int kvh = run % a.nKv;
    const int p0 = blockIdx.x * a.chunkPos;
    const int cnt = min(a.chunkPos, a.n - p0);
    if (cnt <= 0) return;
    typedef V __attribute__((address_space(1))) GV;  // global memory, not flat accesses
    const uintptr_t base = reinterpret_cast<uintptr_t>(a.bases[run / a.nKv]);
    const size_t so = kvOff(a.kvMap, a.seqLen, a.nKv, a.hs, a.srcSlot, p0, kvh) * (size_t)a.elemBytes;
    const GV *__restrict__ src = reinterpret_cast<const GV *>(base + so);
    GV *dst[kMaxForkDst];
#pragma unroll
    for (int d = 0; d < kMaxForkDst; d++) {
        // (slots past nDst alias the first destination and are never stored to)
        const int slot = a.dstSlots[d < a.nDst ? d : 0];
        dst[d] = reinterpret_cast<GV *>(base + kvOff(a.kvMap, a.seqLen, a.nKv, a.hs, slot, p0, kvh) * (size_t)a.elemBytes);
    }
    const int nv = (int)((size_t)cnt * a.hs * a.elemBytes / sizeof(V));
    constexpr int kStep = kCopyThreads * kCopyUnroll;
    int i0 = 0;
    for (; i0 + kStep <= nv; i0 += kStep) {  // whole steps: every lane in bounds, loads before stores
        V r[kCopyUnroll];
#pragma unroll
        for (int u = 0; u < kCopyUnroll; u++) r[u] = src[i0 + u * kCopyThreads + threadIdx.x];
#pragma unroll
        for (int d = 0; d < kMaxForkDst; d++) {
            if (d < a.nDst) {
#pragma unroll
                for (int u = 0; u < kCopyUnroll; u++) dst[d][i0 + u * kCopyThreads + threadIdx.x] = r[u];
            }
        }
    }
    for (int i = i0 + threadIdx.x; i < nv; i += kCopyThreads) {  // the last partial step
        const V r = src[i];
#pragma unroll
        for (int d = 0; d < kMaxForkDst; d++)
            if (d < a.nDst) dst[d][i] = r;
    }
}

}  // namespace

void launchKvForkPrefix(const KvForkArgs &a, hipStream_t s) {
    DL_CHECK(a.n >= 1 && a.n <= a.seqLen && a.chunkPos >= 1 && a.nDst >= 1 && a.nDst <= kMaxForkDst,
             "kvForkPrefix: bad arguments");
    for (int d = 0; d < a.nDst; d++) {
        DL_CHECK(a.dstSlots[d] != a.srcSlot, "kvForkPrefix: a destination is the source");
        for (int e = 0; e < d; e++) DL_CHECK(a.dstSlots[d] != a.dstSlots[e], "kvForkPrefix: a destination is named twice");
    }
    DL_CHECK(!a.kvMap.table || a.chunkPos <= (1 << a.kvMap.pageShift), "kvForkPrefix: a chunk crosses a page");
    const dim3 grid((a.n + a.chunkPos - 1) / a.chunkPos, a.nLayers * 2 * a.nKv);
    DL_CHECK(grid.y <= 65535, "kvForkPrefix: too many (layer, head) runs for one launch");
    const int rowBytes = a.hs * a.elemBytes;
    if (rowBytes % 16 == 0)
        hipLaunchKernelGGL(kvForkPrefixKernel<Vec16>, grid, dim3(kCopyThreads), 0, s, a);
    else if (a.elemBytes == 4)
        hipLaunchKernelGGL(kvForkPrefixKernel<uint32_t>, grid, dim3(kCopyThreads), 0, s, a);
    else
        hipLaunchKernelGGL(kvForkPrefixKernel<uint16_t>, grid, dim3(kCopyThreads), 0, s, a);
    DL_HIP(hipGetLastError());
}

}  // namespace hipk
}  // namespace dl
