// Structured outputs on the device (ConstraintArgs in kernels.h): the token mask of rows that
// follow a compiled byte DFA, ahead of the sampler, and the state's advance behind it. The walk is
// grammarStepToken of csrc/core/grammar_dfa.h, the same function the host runs, over a view of the
// tables.
//
// Mask: grid (ceil(vocab / 256), B), 256 threads, one thread per token. The workgroup stages, once:
// the slot's class map (256 bytes, one 4-byte load by each of 64 lanes) and the transition row of
// the row's state (nClasses u16, one per lane) in LDS; the state, nClasses, nStates and the state's
// accept bit are uniform loads. A thread loads its token's (offset, length | class) and walks the
// piece's bytes. The first byte is answered from LDS - most tokens reject there - and so is every
// later byte that finds the walk still in the row's state (the loop of a free string); the others
// follow next[] in global memory, one dependent load per byte, so a wave runs as long as its longest
// surviving token. The verdicts are stored by maskStoreTail (row_dev.h). Nothing is shared between
// workgroups.
#include "../core/grammar_dfa.h"
#include "row_dev.h"

namespace dl {
namespace hipk {

namespace {

struct GrammarSlotTables {
    const uint16_t *next;
    const uint8_t *classOf;
    const uint32_t *accept;
    uint32_t nClasses, nStates;
};

__device__ __forceinline__ GrammarSlotTables grammarSlotTables(const ConstraintArgs &a, int slot) {
    const uint8_t *base = a.grammarTables + (size_t)slot * kGrammarSlotBytes;
    GrammarSlotTables t;
    t.next = reinterpret_cast<const uint16_t *>(base);
    t.classOf = base + kGrammarClassOff;
    t.accept = reinterpret_cast<const uint32_t *>(base + kGrammarAcceptOff);
    const uint32_t *head = reinterpret_cast<const uint32_t *>(base + kGrammarHeadOff);
    // (clamped: whatever the block holds, an index built from these stays inside it)
    t.nClasses = min(head[0], 256u);
    t.nStates = min(head[1], kGrammarMaxStates);
    if ((size_t)t.nClasses * t.nStates > kGrammarMaxEntries) t.nStates = 0;
    return t;
}

__device__ __forceinline__ bool grammarRowOn(const ConstraintArgs &a, int b) {
    return a.spec[b].x >= 0.f && a.proc[b].w == kRowKindGrammar;
}

// The mask kernel's view: class map and the row's state in LDS.
struct GrammarLdsView {
    const uint8_t *shClass;   // LDS [256]
    const uint16_t *shRow;    // LDS [nClasses]: next[state0][.]
    const uint16_t *next;     // global
    uint32_t state0, nClasses, nStates;
    bool accept0;
    __device__ __forceinline__ uint32_t cls(uint8_t c) const { return shClass[c]; }
    __device__ __forceinline__ uint32_t step(uint32_t s, uint32_t k) const {
        if (s == state0) return shRow[k];
        return s < nStates ? next[s * nClasses + k] : kGrammarDead;  // (never indexes past the tables)
    }
    __device__ __forceinline__ bool accepting(uint32_t) const { return accept0; }  // (asked of state0 only)
    __device__ __forceinline__ uint32_t states() const { return nStates; }
};

}  // namespace

__global__ __launch_bounds__(kRowWg) void grammarMaskKernel(ConstraintArgs a) {
    const int b = blockIdx.y;
    if (!grammarRowOn(a, b)) return;  // (uniform over the workgroup) the row is neither read nor written
    __shared__ uint32_t shClass[64];
    __shared__ uint16_t shRow[256];
    const int slot = a.slots[b];
    const GrammarSlotTables tb = grammarSlotTables(a, slot);
    const uint32_t state = a.grammarStates[slot];
    const bool inside = state < tb.nStates;
    const int tid = (int)threadIdx.x;
    if (tid < 64) shClass[tid] = reinterpret_cast<const uint32_t *>(tb.classOf)[tid];
    if (tid < (int)tb.nClasses) shRow[tid] = inside ? tb.next[state * tb.nClasses + tid] : (uint16_t)kGrammarDead;
    __syncthreads();
    GrammarLdsView v;
    v.shClass = reinterpret_cast<const uint8_t *>(shClass);
    v.shRow = shRow;
    v.next = tb.next;
    v.state0 = state;
    v.nClasses = tb.nClasses;
    v.nStates = tb.nStates;
    v.accept0 = inside && ((tb.accept[state >> 5] >> (state & 31u)) & 1u);
    const int vocab = a.vocab;
    const int t = (int)blockIdx.x * kRowWg + tid;
    bool ok = true;  // (lanes behind the row store nothing)
    if (t < vocab) {
        const uint2 m = a.table.meta[t];
        ok = grammarStepToken(v, state, a.table.words, m.x, m.y) != kGrammarReject;
    }
    maskStoreTail(a.logits + (size_t)b * vocab, t, vocab, ok);
}

// One thread per row.
__global__ __launch_bounds__(64) void grammarAdvanceKernel(ConstraintArgs a, int B) {
    const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (b >= B || !grammarRowOn(a, b)) return;
    const int id = a.ids[b];
    if (id < 0 || id >= a.vocab) return;
    const int slot = a.slots[b];
    const GrammarSlotTables tb = grammarSlotTables(a, slot);
    GrammarView v;
    v.classOf = tb.classOf;
    v.next = tb.next;
    v.accept = tb.accept;
    v.nClasses = tb.nClasses;
    v.nStates = tb.nStates;
    const uint2 m = a.table.meta[id];
    const uint32_t next = grammarStepToken(v, a.grammarStates[slot], a.table.words, m.x, m.y);
    if (next == kGrammarReject) return;
    a.grammarStates[slot] = next;
}

void launchGrammarMask(const ConstraintArgs &a, int B, hipStream_t s) {
    hipLaunchKernelGGL(grammarMaskKernel, dim3((a.vocab + kRowWg - 1) / kRowWg, B), dim3(kRowWg), 0, s, a);
}

void launchGrammarAdvance(const ConstraintArgs &a, int B, hipStream_t s) {
    hipLaunchKernelGGL(grammarAdvanceKernel, dim3((B + 63) / 64), dim3(64), 0, s, a, B);
}

// (preloadModules: any kernel of this code object)
const void *grammarMaskModuleKernel() { return (const void *)grammarMaskKernel; }

}  // namespace hipk
}  // namespace dl
