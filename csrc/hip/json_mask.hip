// JSON mode on the device (ConstraintArgs in kernels.h): the token mask ahead of the sampler and the
// automaton's advance behind it, so that a constrained request still leaves the device as token ids
// only. The automaton is csrc/core/json_grammar.h, the same functions the host runs.
//
// Mask: grid (ceil(vocab / 256), B), 256 threads, one thread per token. Thread 0 reads the row's
// 16-byte state, the workgroup takes it from LDS. A thread loads its token's (offset, length | class)
// and walks the piece's bytes, one 4-byte word of the table per four bytes, through jsonStep until a
// byte rejects or the piece ends, so a wave runs as long as its longest surviving token. The
// verdicts are stored by maskStoreTail (row_dev.h). Nothing is shared between workgroups.
#include "../core/json_grammar.h"
#include "row_dev.h"

namespace dl {
namespace hipk {

__device__ __forceinline__ JsonState jsonUnpack(const uint4 v) {
    JsonState s;
    s.lex = (uint8_t)(v.x & 0xffu);
    s.aux = (uint8_t)((v.x >> 8) & 0xffu);
    s.ws = (uint8_t)((v.x >> 16) & 0xffu);
    s.depth = (uint8_t)(v.x >> 24);
    s.pad = 0;
    s.stack = (uint64_t)v.z | (uint64_t)v.w << 32;
    return s;
}

__device__ __forceinline__ uint4 jsonPack(const JsonState &s) {
    uint4 v;
    v.x = (uint32_t)s.lex | (uint32_t)s.aux << 8 | (uint32_t)s.ws << 16 | (uint32_t)s.depth << 24;
    v.y = 0u;
    v.z = (uint32_t)s.stack;
    v.w = (uint32_t)(s.stack >> 32);
    return v;
}

__device__ __forceinline__ bool jsonRowOn(const ConstraintArgs &a, int b) {
    return a.spec[b].x >= 0.f && a.proc[b].w == kRowKindJson;
}

__global__ __launch_bounds__(kRowWg) void jsonMaskKernel(ConstraintArgs a) {
    const int b = blockIdx.y;
    if (!jsonRowOn(a, b)) return;  // (uniform over the workgroup) the row is neither read nor written
    __shared__ uint4 shState;
    if (threadIdx.x == 0) shState = a.jsonStates[a.slots[b]];
    __syncthreads();
    const JsonState st = jsonUnpack(shState);
    const int vocab = a.vocab;
    const int t = (int)blockIdx.x * kRowWg + (int)threadIdx.x;
    bool ok = true;  // (lanes behind the row store nothing)
    if (t < vocab) {
        const uint2 m = a.table.meta[t];
        ok = !jsonRejected(jsonStepToken(st, a.table.words, m.x, m.y));
    }
    float *row = a.logits + (size_t)b * vocab;
    maskStoreTail(row, t, vocab, ok);
}

// One thread per row.
__global__ __launch_bounds__(64) void jsonAdvanceKernel(ConstraintArgs a, int B) {
    const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (b >= B || !jsonRowOn(a, b)) return;
    const int id = a.ids[b];
    if (id < 0 || id >= a.vocab) return;
    uint4 *sp = a.jsonStates + a.slots[b];
    const uint2 m = a.table.meta[id];
    const JsonState next = jsonStepToken(jsonUnpack(*sp), a.table.words, m.x, m.y);
    if (jsonRejected(next)) return;
    *sp = jsonPack(next);
}

void launchJsonMask(const ConstraintArgs &a, int B, hipStream_t s) {
    hipLaunchKernelGGL(jsonMaskKernel, dim3((a.vocab + kRowWg - 1) / kRowWg, B), dim3(kRowWg), 0, s, a);
}

void launchJsonAdvance(const ConstraintArgs &a, int B, hipStream_t s) {
    hipLaunchKernelGGL(jsonAdvanceKernel, dim3((B + 63) / 64), dim3(64), 0, s, a, B);
}

// (preloadModules: any kernel of this code object)
const void *jsonMaskModuleKernel() { return (const void *)jsonMaskKernel; }

}  // namespace hipk
}  // namespace dl
