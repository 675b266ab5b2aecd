// Logit processors ahead of the device sampler (LogitProcArgs in kernels.h): frequency / presence
// penalties over dense per-slot token counts and a per-slot logit bias, so that requests that use
// them still leave the device as token ids only.
//
// grid (logitProcGroups(vocab), B), 256 threads; a workgroup works on its share of the row
// (RowShare / mapShare, row_dev.h). Dense pass: a thread loads kRowU vectors of logits and of
// counts, applies the penalties where the count is positive and stores the vectors. Bias pass, after a workgroup barrier: thread j takes the slot's entries j,
// j + 256; an entry whose element this workgroup owns is recomputed from the raw logit and count
// and stored again - ordered after the dense pass's store of the same element by the barrier.
#include "row_dev.h"

namespace dl {
namespace hipk {

static constexpr int kLpMaxGroups = 64;

int logitProcGroups(int vocab) {
    const int nvec = vocab / 4;
    const int G = (nvec + kRowWg * kRowU - 1) / (kRowWg * kRowU);
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

__global__ __launch_bounds__(kRowWg) void logitProcKernel(LogitProcArgs a) {
    const int b = blockIdx.y;
    if (a.spec[b].x < 0.f) return;  // not drawn: the row's output stays as it is
    const float4 pr = a.proc[b];
    const bool active = pr.z != 0.f;
    const int vocab = a.vocab;
    const RowShare sh = rowShare(vocab);
    const float *in = a.logits + (size_t)b * vocab;
    float *out = a.out + (size_t)b * vocab;
    if (!active) {  // a plain copy
        mapShare(sh, out, in, in, [](float x, float) { return x; });
        return;
    }
    const int slot = a.slots[b];
    const uint32_t *cnt = a.counts + (size_t)slot * vocab;
    const float presence = pr.x, frequency = pr.y;
    mapShare(sh, out, in, cnt, [&](float x, uint32_t c) { return lpPenalize(x, c, presence, frequency); });
    int nb = a.nBias[slot];
    nb = nb < 0 ? 0 : (nb > kMaxLogitBias ? kMaxLogitBias : nb);
    if (nb == 0) return;  // (uniform over the workgroup)
    __syncthreads();      // the dense pass's stores of this workgroup come before the bias stores
    const LogitBiasEntry *bias = a.bias + (size_t)slot * kMaxLogitBias;
    for (int j = (int)threadIdx.x; j < nb; j += kRowWg) {
        const LogitBiasEntry e = bias[j];
        if (e.id < 0 || e.id >= vocab) continue;
        if (!sh.owns(e.id)) continue;
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
    hipLaunchKernelGGL(logitProcKernel, dim3(logitProcGroups(a.vocab), B), dim3(kRowWg), 0, s, a);
}

void launchLogitProcCount(const LogitProcArgs &a, int B, hipStream_t s) {
    hipLaunchKernelGGL(logitProcCountKernel, dim3((B + 63) / 64), dim3(64), 0, s, a, B);
}

// (preloadModules: any kernel of this code object)
const void *logitProcModuleKernel() { return (const void *)logitProcKernel; }

}  // namespace hipk
}  // namespace dl
