// Single-kernel entry points for kernel-level numerics tests and the Python `ops` package.
//
// Each call uploads host operands, runs ONE of the gfx950 kernels of csrc/hip/kernels.hip exactly as
// the engine launches it (same tiling, same fused prologue/epilogue), and copies the result back.
// They are not on the inference hot path; they exist so that every hot kernel can be compared
// against a plain PyTorch fp32 reference of the same op (tests/test_gpu_ops.py).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../core/grammar_dfa.h"

namespace dl {
namespace ops {

// Q40 GEMV (decode kernel, B rows <= 4) over `blocks` = [rows][n/32] Q40 blocks in file layout
// (18 bytes: f16 d + 16 nibble bytes). Prologue: in (+ residual) -> RMS norm with normW (if given,
// else plain) -> Q80 in LDS. epi 0: out[b][r] = W[r] . xq; epi 1: rows interleaved (w1, w3) pairs,
// out[b][r/2] = silu(W[2i] . xq) * (W[2i+1] . xq). Returns out; xNext (if residual) = in + residual.
//
// Launch geometry of the Q40 ring GEMV ops (gemvQ40, gemvQ40Q80In, qkvRope and the ones below):
// `lanes` = lanes per row L of the weight tiling and the launch (0: the GEMV's own choice for the
// shape, else 16, 32 or 64), `passes` = row passes per workgroup (0: the default for the shape,
// else >= 1). A launch the kernel cannot run is refused (a lane count that has no instance, an
// LDS footprint beyond the CU's 160 KB, SwiGLU -> Q80 with workgroups of other than whole 64-row
// blocks). Every output buffer carries a guard region of a fixed bit pattern after each batch
// row's last valid element (at least one workgroup's rows); the op throws when a launch changed it.
std::vector<float> gemvQ40(const std::vector<uint8_t> &blocks, int rows, int n, const std::vector<float> &in,
                           const std::vector<float> &residual, const std::vector<float> &normW, float eps, int B,
                           int epi, std::vector<float> *xNext, int lanes = 0, int passes = 0);

// Same weights, activations already Q80 (the wo / w2 path: prologue-free, Q80 blocks read from
// global): `in` is quantized on the host with the reference Q80 quantizer first.
std::vector<float> gemvQ40Q80In(const std::vector<uint8_t> &blocks, int rows, int n, const std::vector<float> &in,
                                int B, int lanes = 0, int passes = 0);

// The w13 hand-off of a decode step (PRO_RESNORM + EPI_ACT_Q80): rows are interleaved (w1, w3)
// pairs, rows % 64 == 0; the SwiGLU row is quantized to Q80 blocks of 32 hidden units. codes =
// [B][rows/2] int8, scales = [B][rows/64] (d, sum of codes) pairs as [B][rows/64][2] floats.
void gemvQ40SwigluQ80(const std::vector<uint8_t> &blocks, int rows, int n, const std::vector<float> &in,
                      const std::vector<float> &residual, const std::vector<float> &normW, float eps, int B,
                      int lanes, int passes, std::vector<int8_t> &codes, std::vector<float> &scales);

// The fused greedy logits GEMV (PRO_RESNORM + EPI_ARGMAX, one row, one rank): returns
// vocabStart + the argmax row (ties -> lowest). The partials are sized to the launch's grid and the
// arrival counter starts at zero; `repeat` launches run on the same scratch (the counter resets
// itself) and must all give the same id; the op throws if they do not or if the counter is not
// back to zero.
int gemvQ40Argmax(const std::vector<uint8_t> &blocks, int rows, int n, const std::vector<float> &in,
                  const std::vector<float> &residual, const std::vector<float> &normW, float eps, int vocabStart,
                  int lanes, int passes, int repeat);

// F32-weight GEMV (gemvKernel; w = [rows][n] row-major), B = 1, 2 or 4. pro 0: PRO_GLOBAL (f32
// rows read straight from global; no residual, no norm), 1: PRO_RESNORM (in (+ residual) -> RMS norm
// with normW if given -> f32 in LDS). epi 0: EPI_STORE, 1: EPI_ACT (interleaved (w1, w3) rows;
// PRO_RESNORM only: the engine never launches PRO_GLOBAL + EPI_ACT and no instance exists, refused).
// lanes / passes as above (one row per lane group: 256 / L rows per pass).
std::vector<float> gemvF32(const std::vector<float> &w, int rows, int n, const std::vector<float> &in,
                           const std::vector<float> &residual, const std::vector<float> &normW, float eps, int B,
                           int pro, int epi, int lanes, int passes, std::vector<float> *xNext);

// Host side of the launches above, no device needed. gemvDefaults: the (lanes, passes) the engine
// takes for a matrix of this shape (gemvLanesPerRow at one row, gemvDefaultPasses with that tiling;
// epi: 0 store, 1 SwiGLU, 2 QKV, 3 SwiGLU -> Q80, 7 argmax). tileQ40Host: the tiled device image
// (Q40Tiling, kernels.h) of `blocks` written by tileQ40 (aos false: from split nibble / scale
// arrays) or tileQ40AoS (from the file's 18-byte blocks).
void gemvDefaults(int rows, int n, int B, bool q40, int epi, int &lanes, int &passes);
void tileQ40Host(const std::vector<uint8_t> &blocks, int rows, int n, int lanes, bool aos, std::vector<uint8_t> &qs,
                 std::vector<uint32_t> &d);

// Batched F32 matmul on MFMA: norm kernel -> f16 -> gemmF32Kernel (store epilogue).
std::vector<float> gemmF32(const std::vector<float> &w, int rows, int n, const std::vector<float> &in,
                           const std::vector<float> &normW, float eps, int M);
std::vector<float> gemmQ40(const std::vector<uint8_t> &blocks, int rows, int n, const std::vector<float> &in,
                           const std::vector<float> &residual, const std::vector<float> &normW, float eps, int M,
                           int splits = 0);  // Batched Q40 matmul on MFMA (narrow <= 64 tokens, wide above);
                                             // splits > 0 forces the K split (must divide n / 32)

// One batched GEMM of the forward schedule, launched as the engine's gemmBatched launches it: Q40
// (`blocks`, tiled at `lanes`: 0 = the GEMV's choice for the shape, else 16 / 32 / 64) or F32 (`wf`
// [rows][n]) weights, one of three input modes, one of the four epilogues the engine fuses into a
// GEMM, the engine's chunking (gemmChunkTokens: one wide launch, or <= 128 (Q40) / <= 64 (F32) tokens
// per narrow launch, every operand pointer advanced by the chunk's first token, ldSS held fixed).
//   input  GEMM_IN_NORM:    in (+ residual) -> launchNormF16 (normW empty: no norm) per chunk
//          GEMM_IN_F16:     `in` rounded to f16 on the host (the wo / w2 operand)
//          GEMM_IN_PRENORM: `in` = x' * w * 2^-5 rows (rounded to f16) and `ss` = [ssTiles][ldSS]
//                           partial sums of squares of x' (the EPI_RES producer's outputs)
//   epi    EPI_STORE:   out [M][rows]
//          EPI_ACT_F16: interleaved (w1, w3) rows, SiLU; out [M][rows / 2] (the f16 values)
//          EPI_RES:     resIn [M][rows], resW [rows] -> out = resOut [M][rows], resX [M][rows] (the
//                       f16 values), ssOut [ceil(rows / 64)][ldSS] (unwritten slots read back NaN)
//          EPI_QKV:     rows = q0 + 2 kv0; rope / pos / slot as ops::qkvRope, nSlots caches slots;
//                       out = q [M][q0], kOut / vOut the appended rows [M][kv0]
// splits: 0 = the launcher's gemmSplits with the tiling's L per launch, as the engine passes it;
// fixed: the batch-invariant narrow launch (the caller sets splits as such an engine does). chunk:
// 0 = the engine's rule, else the tokens per launch forced.
// Every output carries guard regions of a fixed bit pattern (after each token row's last valid
// element, after the last token, for ssOut after column M of every tile row and after the last tile
// row, for the caches everywhere but the appended rows); the op throws when a launch changed one.
// A launch the launchers refuse (or whose operands do not fit their contract) throws before any
// device work. The report names the kernel of every launch by the launcher's own predicates.
enum GemmInput : int { GEMM_IN_NORM = 0, GEMM_IN_F16 = 1, GEMM_IN_PRENORM = 2 };
struct GemmBatchedArgs {
    std::vector<uint8_t> blocks;
    std::vector<float> wf;
    int rows = 0, n = 0, lanes = 0;
    int input = GEMM_IN_NORM;
    std::vector<float> in, residual, normW;
    float eps = 1e-5f;
    int M = 0;
    std::vector<float> ss;
    int ssTiles = 0, ldSS = 0;
    int epi = 0;
    std::vector<float> resIn, resW;
    int q0 = 0, kv0 = 0, hs = 0, seqLen = 0, nSlots = 0;
    std::vector<float> rope;
    std::vector<int> pos, slot;
    bool kvBf16 = true;
    int splits = 0, fixed = 0, chunk = 0;
};
struct GemmLaunch {
    int c0 = 0, M = 0, kernel = 0 /* GemmKernel, 3 = F32 */, splits = 1, grid = 0 /* workgroups */;
};
struct GemmBatchedResult {
    std::vector<float> out, resX, ssOut, k, v;
    std::vector<GemmLaunch> launches;
};
// the launches of the call (kernels, splits, grids) and its refusals; no device needed
std::vector<GemmLaunch> gemmBatchedPlan(const GemmBatchedArgs &a);
GemmBatchedResult gemmBatched(const GemmBatchedArgs &a);
// hipk::gemmSplits: the K splits the launcher takes for M tokens on a matrix tiled at `lanes`
int gemmSplitsFor(int rows, int n, int M, int lanes);

// QKV GEMV with the RoPE + KV-append epilogue (rows = q0 + 2*kv0, head size hs): returns rotated q
// [B][q0]; kOut/vOut receive the appended cache rows [B][kv0] (f32 view of the bf16 or f32 cache).
// rope = [seqLen][hs/2] (cos, sin) pairs; pos[b] < seqLen; each row b writes cache slot b.
std::vector<float> qkvRope(const std::vector<uint8_t> &blocks, int q0, int kv0, int hs, int n,
                           const std::vector<float> &in, const std::vector<float> &normW, float eps,
                           const std::vector<float> &rope, int seqLen, const std::vector<int> &pos, bool kvBf16,
                           std::vector<float> *kOut, std::vector<float> *vOut, int lanes = 0, int passes = 0);

// Decode attention over caches k/v [nSlots][seqLen][kv0] (f32 values, stored bf16 when kvBf16),
// q [B][nHeads0*hs] (already rotated), row b at position pos[b] in slot slot[b]. Returns f32 [B][q0].
std::vector<float> attention(const std::vector<float> &q, const std::vector<float> &k, const std::vector<float> &v,
                             int nSlots, int seqLen, int nHeads0, int kvMul, int hs, const std::vector<int> &pos,
                             const std::vector<int> &slot, bool kvBf16, int impl = 0);
// attention impl: 0 = launchAttention's choice, 1 = MFMA prefill kernel, 2 = VALU decode kernel,
// 3 = MFMA decode kernel

// One attention launch as the engine's attnArgs / enqueueAttention set it up (engine_forward.cpp),
// which ops::attention above cannot: a page table, the single-row split geometry, the f16 and Q80
// writers, a pinned head group, strided rows and reused scratch.
//   kernel   ATTN_AUTO: launchAttention's choice (decode) / launchAttentionPrefill's (prefill);
//            ATTN_VALU / ATTN_MFMA: that decode kernel; ATTN_PREFILL: the prefill launcher
//   mode     ATTN_DECODE or ATTN_PREFILL_ROWS (blocks of attnPrefillRowsPerBlock rows share a slot)
//   single   the engine's single-row setup: shortLen = kAttnShortLen, splitGrid =
//            attnSplitGrid(seqLen, true), chunkMax from the *batched* grid attnSplitGrid(seqLen, false);
//            else the batched setup (shortLen 0). splitGrid > 0 forces the grid (chunkMax =
//            attnChunkMax(seqLen, splitGrid)).
//   headGroup 0 (the launcher's pick) or 1 / 2 / 4 / 8 (AttnArgs::headGroup)
//   out      ATTN_OUT_F32 / _F16 (outH) / _Q80 (outQ + outS; decode kernels only: the prefill
//            kernels ignore outQ, so that combination is refused)
//   ldq / ldOut  row strides, 0 = q0, else >= q0 (multiples of 4 / 32: vector loads, Q80 blocks)
//   pageSize 0: contiguous caches; else a power of two >= 32: the caches go to a page pool in the
//            engine's paged layout (kvOff with a table), pageOf = [nSlots][ceil(seqLen / pageSize)]
//            pool pages (ids below nSlots * pagesPerSlot), -1 = not mapped. The pool has one extra
//            *poison page* every unmapped entry points to; it and every pool page no entry names hold
//            poisonK / poisonV ([kv0] each, zeros when empty) at every position.
//   repeat   launches on the same scratch and output buffer (re-filled with the guard pattern in
//            between): all must give bitwise the same result and leave every counter zero.
// Guards of the fixed pattern of gemmBatched: after each output row's valid part (ldOut > q0), after
// the last row, behind partO, partML and counters; for f16 / Q80 around the code and scale arrays
// separately. The op throws when a launch changed one. A launch the launchers refuse, or whose
// operands are outside their contract, throws before any device work (attentionPlan).
enum AttnKernelSel : int { ATTN_AUTO = 0, ATTN_VALU = 1, ATTN_MFMA = 2, ATTN_PREFILL = 3 };
enum AttnMode : int { ATTN_DECODE = 0, ATTN_PREFILL_ROWS = 1 };
enum AttnOut : int { ATTN_OUT_F32 = 0, ATTN_OUT_F16 = 1, ATTN_OUT_Q80 = 2 };
struct AttnLaunchArgs {
    std::vector<float> q, k, v;  // q [B][ldq], k / v [nSlots][seqLen][kv0]
    int nSlots = 0, seqLen = 0, nHeads0 = 0, kvMul = 1, hs = 0;
    std::vector<int> pos, slot;
    bool kvBf16 = true;
    int kernel = ATTN_AUTO, mode = ATTN_DECODE;
    bool single = false;
    int splitGrid = 0, headGroup = 0;
    int out = ATTN_OUT_F32;
    int ldq = 0, ldOut = 0;
    int pageSize = 0;
    std::vector<int> pageOf;
    std::vector<float> poisonK, poisonV;
    int repeat = 1;
    // optional [B]: one launch with these positions (same rows, slots and caches) runs first on the
    // same scratch and output buffer, so that the measured launches find its partials and counters
    std::vector<int> warmPos;
};
// Host side of the launch, from the launchers' own predicates; no device needed.
struct AttnLaunchPlan {
    std::string kernel;       // the instance, e.g. "attnKernel<2,128,bf16>", "attnDecodeMfmaKernel<4>"
    int hg = 0;               // VALU decode: heads per workgroup (attnValuHeadGroup); else 0
    int grid[3] = {0, 0, 0};
    int splitGrid = 0, chunkMax = 0, shortLen = 0;
    std::vector<int> nSplit, ch;  // decode: attnSplit of every row; prefill: attnPrefillSplit of every row block
};
struct AttnLaunchResult {
    std::vector<float> out;     // [B][q0]: f32, the f16 values, or the Q80 codes
    std::vector<float> scales;  // Q80: [B][q0 / 32][2] (d, sum of codes)
    AttnLaunchPlan plan;
};
AttnLaunchPlan attentionPlan(const AttnLaunchArgs &a);
AttnLaunchResult attentionLaunch(const AttnLaunchArgs &a);

// Parallel argmax over [B][vocab] (ties -> lowest index).
std::vector<int> argmax(const std::vector<float> &logits, int B, int vocab);
// device sampler (launchSample): spec rows (temperature, topp, coin, -)
std::vector<int> sample(const std::vector<float> &logits, int B, int vocab, const std::vector<float> &specs);

// launchLogprobs over [B][vocab] logits: ids[b] the row's chosen token, requests[b] = 0 (none) or
// 1 + k (SampleSpec::logprobs). Returns [B][21] (logprob, id) pairs as two arrays; the output is
// pre-filled with (0, -2), which rows without a request keep. `warm` (optional): logits and ids of
// an earlier call with the same requests, run first on the same scratch and output buffer (without
// targets). `targets` (optional, [B]): LogprobArgs::target, the given token a row scores (< 0: ids[b]).
void logprobs(const std::vector<float> &logits, int B, int vocab, const std::vector<int> &ids,
              const std::vector<int> &requests, std::vector<float> &outLogprobs, std::vector<int> &outIds,
              const std::vector<float> *warmLogits = nullptr, const std::vector<int> *warmIds = nullptr,
              const std::vector<int> *targets = nullptr);
// Device microseconds per launch of launchLogprobs (request 1 + k on every row) and of launchArgmax
// on the same [B][vocab] logits: `iters` launches of each between two events, after a warm-up.
// targets: every row scores a given token (b * 7919 % vocab) instead of the argmax kernel's id.
void benchLogprobs(const std::vector<float> &logits, int B, int vocab, int k, int iters, double &logprobsUs,
                   double &argmaxUs, bool targets = false);

// launchLogitProc over [B][vocab] logits. Row b: temps[b] (< 0: the row is not drawn and its output
// keeps `fill`), slots[b] in [0, nSlots), active[b], presence[b], frequency[b]. counts is the
// [nSlots][vocab] table, biasIds / biasVals [nSlots][300] with nBias[s] entries used per slot.
// Returns the [B][vocab] output, which is pre-filled with `fill`; a write behind its last row is
// an error.
std::vector<float> logitProc(const std::vector<float> &logits, int B, int vocab, const std::vector<float> &temps,
                             const std::vector<int> &slots, const std::vector<int> &active,
                             const std::vector<float> &presence, const std::vector<float> &frequency,
                             const std::vector<uint32_t> &counts, int nSlots, const std::vector<int> &biasIds,
                             const std::vector<float> &biasVals, const std::vector<int> &nBias, float fill);
// launchLogitProcCount on a [nSlots][vocab] table: returns the table after the launch.
std::vector<uint32_t> logitProcCount(const std::vector<uint32_t> &counts, int nSlots, int vocab,
                                     const std::vector<int> &ids, const std::vector<int> &slots,
                                     const std::vector<int> &active);
// Device microseconds per launch of launchLogitProc (B active rows, row b on slot b, a third of the
// counts positive, nBias entries per slot) and of launchLogitProcCount: `iters` launches of each
// between two events, after a warm-up.
void benchLogitProc(int B, int vocab, int nBias, int iters, double &procUs, double &countUs);

// launchPool, one launch per entry of `launches` on the same per-slot state (accumulators, outputs,
// counters), in order. A launch holds B rows x[B][dim] (+ add[B][dim], may be empty); row b belongs
// to slots[b] and flags[b] carries kPoolTake / kPoolFirst / kPoolLast / kPoolModeLast (kernels.h),
// counts[b] the request's row count at its last row. out / acc [nSlots][dim] come in as the buffers'
// initial contents (sentinels) and go out as the launches left them; every slot's counter must be
// back to zero.
struct PoolLaunch {
    std::vector<float> x, add;
    std::vector<int> slots, flags, counts;
};
void pool(const std::vector<PoolLaunch> &launches, int dim, int nSlots, const std::vector<float> &normW, float eps,
          std::vector<float> &out, std::vector<float> &acc);
// Device microseconds per launchPool over B rows of dim (+ add), `slots` requests of B / slots rows
// each, all finalised (mean), and per device copy of the same B x dim x 4 bytes (x 2 with add).
void benchPool(int B, int dim, int slots, bool withAdd, int iters, double &poolUs, double &copyUs);

// launchLogitFilter over a copy of [B][vocab] logits. Row b: temps[b], topK[b], delta[b] (-inf: min_p
// off), active[b]. Returns the [B][vocab] buffer after the launch; a write behind its last row, or a
// row counter left non-zero, is an error.
std::vector<float> logitFilter(const std::vector<float> &logits, int B, int vocab, const std::vector<float> &temps,
                               const std::vector<int> &topK, const std::vector<float> &delta,
                               const std::vector<int> &active);
// Device microseconds, each over `iters` back-to-back repeats between two events after a warm-up, on
// B active rows of bell-shaped logits at temperature 0.8: a device copy of the logits; that copy
// followed by launchLogitFilter(topK, delta) on the copy (the filter works in place, so every launch
// gets fresh rows); launchSample (top-p 0.9) on the filtered rows.
void benchLogitFilter(int B, int vocab, int topK, float delta, int iters, double &copyUs, double &copyFilterUs,
                      double &sampleUs);

// JSON mode's kernels on their own. The token table is JsonTokenTable's three arrays (backend.h), a
// state is a JsonState as 4 words; row b takes part when on[b] and temps[b] >= 0, and its state is
// states[b]. jsonMask: launchJsonMask over a copy of [B][vocab] logits, returns the buffer after the
// launch; a write behind its last row, or a state that changed, is an error. jsonAdvance:
// launchJsonAdvance with the drawn ids, returns the states after the launch.
std::vector<float> jsonMask(const std::vector<float> &logits, int B, int vocab, const std::vector<float> &temps,
                            const std::vector<int> &on, const std::vector<uint32_t> &off,
                            const std::vector<uint32_t> &info, const std::vector<uint32_t> &words,
                            const std::vector<uint32_t> &states);
std::vector<uint32_t> jsonAdvance(int vocab, const std::vector<float> &temps, const std::vector<int> &on,
                                  const std::vector<int> &ids, const std::vector<uint32_t> &off,
                                  const std::vector<uint32_t> &info, const std::vector<uint32_t> &words,
                                  const std::vector<uint32_t> &states);
// Device microseconds as in benchLogitFilter, on B constrained rows that all sit in `state`: a device
// copy of the logits; the copy + launchJsonMask; launchJsonAdvance (by token 0); the copy +
// launchLogitFilter (top_k 40) on the same logits; launchSample on the masked rows.
void benchJsonMask(int B, int vocab, const std::vector<uint32_t> &off, const std::vector<uint32_t> &info,
                   const std::vector<uint32_t> &words, const std::vector<uint32_t> &state, int iters, double &copyUs,
                   double &copyMaskUs, double &advanceUs, double &copyFilterUs, double &sampleUs);

// The structured-output kernels on their own. The token table is JsonTokenTable's three arrays;
// slot s holds grammars[s] (null: an empty table block) in state states[s]; row b is of kind
// kinds[b] (0 none, 1 JSON mode, 2 grammar), sits in slot slots[b] and takes part when its kind is 2
// and temps[b] >= 0. grammarMask: launchGrammarMask over a copy of [B][vocab] logits, returns the
// buffer after the launch; a write behind its last row, or a state that changed, is an error.
// grammarAdvance: launchGrammarAdvance with the drawn ids, returns the slots' states after it.
std::vector<float> grammarMask(const std::vector<float> &logits, int B, int vocab, const std::vector<float> &temps,
                               const std::vector<int> &kinds, const std::vector<int> &slots,
                               const std::vector<uint32_t> &off, const std::vector<uint32_t> &info,
                               const std::vector<uint32_t> &words, const std::vector<const GrammarDfa *> &grammars,
                               const std::vector<uint32_t> &states);
std::vector<uint32_t> grammarAdvance(int vocab, const std::vector<float> &temps, const std::vector<int> &kinds,
                                     const std::vector<int> &slots, const std::vector<int> &ids,
                                     const std::vector<uint32_t> &off, const std::vector<uint32_t> &info,
                                     const std::vector<uint32_t> &words, const std::vector<const GrammarDfa *> &grammars,
                                     const std::vector<uint32_t> &states);
// Device microseconds as in benchJsonMask, on B grammar rows (one slot each) that all sit in `state`:
// a device copy of the logits; the copy + launchGrammarMask; launchGrammarAdvance (by token 0); the
// copy + launchJsonMask on the same rows at START; launchSample on the masked rows.
void benchGrammarMask(int B, int vocab, const std::vector<uint32_t> &off, const std::vector<uint32_t> &info,
                      const std::vector<uint32_t> &words, const GrammarDfa &grammar, uint32_t state, int iters,
                      double &copyUs, double &copyMaskUs, double &advanceUs, double &copyJsonUs, double &sampleUs);

// Embedding row gather: table [vocab][dim] -> [B][dim].
std::vector<float> embedding(const std::vector<float> &table, int vocab, int dim, const std::vector<int> &tokens);

}  // namespace ops
}  // namespace dl
