// Logit processors ahead of the device sampler (LogitProcArgs in kernels.h): frequency / presence
// penalties over dense per-slot token counts and a per-slot logit bias, so that requests that use
// them still leave the device as token ids only.
//
// grid (logitProcGroups(vocab), B), 256 threads. The row is cut into 16-byte vectors; workgroup g
// owns the vectors [g * vpg, (g + 1) * vpg) and the last workgroup also the vocab % 4 scalar tail.
// Dense pass: a thread loads kLpU vectors of logits and of counts, applies the penalties where the
// count is positive and stores the vectors. Rows of a [B][vocab] buffer start on 4-byte boundaries
// when vocab % 4 != 0, so the vectors are typed with 4-byte alignment (global 16-byte accesses
// need no more). Bias pass, after a workgroup barrier: thread j takes the slot's entries j,
// j + 256; an entry whose element this workgroup owns is recomputed from the raw logit and count
// and stored again - ordered after the dense pass's store of the same element by the barrier.
#include "decode_common.h"

namespace dl {
namespace hipk {

static constexpr int kLpThreads = 256;
static constexpr int kLpU = 4;  // vectors in flight per thread per round
static constexpr int kLpMaxGroups = 64;

typedef float lpF4 __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t lpU4 __attribute__((ext_vector_type(4), aligned(4)));

int logitProcGroups(int vocab) {
    const int nvec = vocab / 4;
    const int G = (nvec + kLpThreads * kLpU - 1) / (kLpThreads * kLpU);
    return G < 1 ? 1 : (G > kLpMaxGroups ? kLpMaxGroups : G);
}

// The formula's steps are separate f32 operations, each rounded to nearest: the arithmetic below is
// written out under contract(off) (the __f*_rn intrinsics are inline functions of a header that is
// compiled with contraction allowed, and fuse after inlining).
#pragma clang fp contract(off)

// x - frequency * float(c) - presence for c > 0, each operation rounded on its own
__device__ __forceinline__ float lpPenalize(float x, uint32_t c, float presence, float frequency) {
    if (c == 0) return x;
    const float fc = frequency * (float)c;
    x = x - fc;
    return x - presence;
}

__global__ __launch_bounds__(kLpThreads) void logitProcKernel(LogitProcArgs a) {
    const int b = blockIdx.y;
    if (a.spec[b].x < 0.f) return;  // not drawn: the row's output stays as it is
    const float4 pr = a.proc[b];
    const bool active = pr.z != 0.f;
    const int vocab = a.vocab, nvec = vocab / 4, G = (int)gridDim.x;
    const int vpg = (nvec + G - 1) / G;
    const int v0 = (int)blockIdx.x * vpg, v1 = min(v0 + vpg, nvec);
    const bool tailOwner = (int)blockIdx.x == G - 1;
    const float *in = a.logits + (size_t)b * vocab;
    float *out = a.out + (size_t)b * vocab;
    if (!active) {  // a plain copy
        for (int i0 = v0 + (int)threadIdx.x; i0 < v1; i0 += kLpU * kLpThreads) {
            lpF4 x[kLpU];
#pragma unroll
            for (int u = 0; u < kLpU; u++) {
                const int i = i0 + u * kLpThreads;
                if (i < v1) x[u] = reinterpret_cast<const lpF4 *>(in)[i];
            }
#pragma unroll
            for (int u = 0; u < kLpU; u++) {
                const int i = i0 + u * kLpThreads;
                if (i < v1) reinterpret_cast<lpF4 *>(out)[i] = x[u];
            }
        }
        if (tailOwner) {
            const int e = 4 * nvec + (int)threadIdx.x;
            if (e < vocab) out[e] = in[e];
        }
        return;
    }
    const int slot = a.slots[b];
    const uint32_t *cnt = a.counts + (size_t)slot * vocab;
    const float presence = pr.x, frequency = pr.y;
    for (int i0 = v0 + (int)threadIdx.x; i0 < v1; i0 += kLpU * kLpThreads) {
        lpF4 x[kLpU];
        lpU4 c[kLpU];
#pragma unroll
        for (int u = 0; u < kLpU; u++) {
            const int i = i0 + u * kLpThreads;
            if (i < v1) {
                x[u] = reinterpret_cast<const lpF4 *>(in)[i];
                c[u] = reinterpret_cast<const lpU4 *>(cnt)[i];
            }
        }
#pragma unroll
        for (int u = 0; u < kLpU; u++) {
            const int i = i0 + u * kLpThreads;
            if (i < v1) {
                lpF4 y;
                y.x = lpPenalize(x[u].x, c[u].x, presence, frequency);
                y.y = lpPenalize(x[u].y, c[u].y, presence, frequency);
                y.z = lpPenalize(x[u].z, c[u].z, presence, frequency);
                y.w = lpPenalize(x[u].w, c[u].w, presence, frequency);
                reinterpret_cast<lpF4 *>(out)[i] = y;
            }
        }
    }
    if (tailOwner) {
        const int e = 4 * nvec + (int)threadIdx.x;
        if (e < vocab) out[e] = lpPenalize(in[e], cnt[e], presence, frequency);
    }
    int nb = a.nBias[slot];
    nb = nb < 0 ? 0 : (nb > kMaxLogitBias ? kMaxLogitBias : nb);
    if (nb == 0) return;  // (uniform over the workgroup)
    __syncthreads();      // the dense pass's stores of this workgroup come before the bias stores
    const LogitBiasEntry *bias = a.bias + (size_t)slot * kMaxLogitBias;
    for (int j = (int)threadIdx.x; j < nb; j += kLpThreads) {
        const LogitBiasEntry e = bias[j];
        if (e.id < 0 || e.id >= vocab) continue;
        const bool mine = e.id >= 4 * nvec ? tailOwner : (e.id / 4 >= v0 && e.id / 4 < v1);
        if (!mine) continue;
        out[e.id] = lpPenalize(in[e.id], cnt[e.id], presence, frequency) + e.v;
    }
}

// One thread per row.
__global__ __launch_bounds__(64) void logitProcCountKernel(LogitProcArgs a, int B) {
    const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (b >= B || a.proc[b].z == 0.f) return;
    const int id = a.ids[b];
    if (id < 0 || id >= a.vocab) return;
    uint32_t *c = a.counts + (size_t)a.slots[b] * a.vocab + id;
    *c = *c + 1u;
}

void launchLogitProc(const LogitProcArgs &a, int B, hipStream_t s) {
    hipLaunchKernelGGL(logitProcKernel, dim3(logitProcGroups(a.vocab), B), dim3(kLpThreads), 0, s, a);
}

void launchLogitProcCount(const LogitProcArgs &a, int B, hipStream_t s) {
    hipLaunchKernelGGL(logitProcCountKernel, dim3((B + 63) / 64), dim3(64), 0, s, a, B);
}

// (preloadModules: any kernel of this code object)
const void *logitProcModuleKernel() { return (const void *)logitProcKernel; }

}  // namespace hipk
}  // namespace dl
