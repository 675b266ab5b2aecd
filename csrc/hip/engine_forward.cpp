// The per-forward kernel schedule of the HIP engine (engine_impl.h): inputs and context buckets,
// GEMV / batched GEMM / attention / fused attention block launches, tensor-parallel collectives.
#include "engine_impl.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace dl {
namespace engine_detail {

// Context buckets: decode capacity seqLen is covered by buckets of 256 x 4^k positions (and seqLen
// itself); a forward whose rows reach at most position p runs the launches of the smallest bucket
// holding p + 1 positions. Within a bucket the sequence split of every row is the one the full
// capacity would give (attnSplit caps ceil(len / 256) chunks at the bucket's split grid, which is
// >= that count), so a bucketed forward is bitwise the forward of an engine sized to the bucket.
void HipEngineImpl::setupBuckets() {
    buckets_.clear();
    for (int len = 256; len < (int)h_.seqLen; len *= 4) {
        CtxBucket b;
        b.maxLen = len;
        buckets_.push_back(b);
    }
    CtxBucket last;
    last.maxLen = (int)h_.seqLen;
    buckets_.push_back(last);
    DL_CHECK(buckets_.size() <= kKeyMaxBucket + 1, "too many context buckets");  // (the graph key's field)
    for (CtxBucket &b : buckets_) {
        b.splitGrid = hipk::attnSplitGrid(b.maxLen, true);
        b.splitGridBat = hipk::attnSplitGrid(b.maxLen, false);
        b.chunkMax = hipk::attnChunkMax(b.maxLen, b.splitGridBat);
    }
    bucket_ = (int)buckets_.size() - 1;
}

const CtxBucket &HipEngineImpl::bucketFor(int maxPos) const {
    for (const CtxBucket &b : buckets_)
        if (maxPos < b.maxLen) return b;
    return buckets_.back();
}

void HipEngineImpl::setInputs(int n, const int *tokens, const int *positions, const int *slots, const SampleSpec *specs,
                              int ahead, const float *procRows, const hipk::LogitFilterRow *filterRows) {
    DL_CHECK(n >= 1 && (u32)n <= cfg_.maxBatch, "batch size out of range");
    DL_CHECK(chainHead_ == chainTail_, "a chained decode step is still in flight");
    for (int b = 0; b < n; b++) {
        DL_CHECK(tokens[b] >= 0 && (u32)tokens[b] < h_.vocabSize, "token out of range");
        DL_CHECK(positions[b] >= 0 && (u32)positions[b] < h_.seqLen, "position out of range");
        DL_CHECK(slots[b] >= 0 && (u32)slots[b] < cfg_.nSlots, "slot out of range");
    }
    mapPages(n, positions, slots, ahead);
    // decode attention kernel for this forward (part of the graph key): the MFMA kernel once a
    // row's context reaches kAttnMfmaMinPos keys (measured faster from ~1.5K keys, slower on
    // short contexts: profiles/r3_prefill_attention.md) or the forward has kAttnMfmaMinRows rows
    // (batch 16 / 64 at 150 keys: 8.2 / 17.2 us vs 9.5 / 22.8 on the VALU kernel, which stays
    // ahead up to batch 8: profiles/r5_batched_attention.md), else the VALU kernel
    int maxPos = 0;
    for (int b = 0; b < n; b++) maxPos = std::max(maxPos, positions[b] + ahead);
    attnLong_ = !invariant_ && (maxPos >= kAttnMfmaMinPos || n >= kAttnMfmaMinRows);
    bucket_ = (int)(&bucketFor(maxPos) - buckets_.data());
    const u32 MB = cfg_.maxBatch;
    // keep the pinned staging buffer stable while a previous copy may still read it (every
    // public entry point ends with a stream sync, so this only waits after an async path)
    if (inputsInFlight_) DL_HIP(hipStreamSynchronize(stream_));
    std::memcpy(hIn_, tokens, n * sizeof(int));
    std::memcpy(hIn_ + MB, positions, n * sizeof(int));
    std::memcpy(hIn_ + 2 * MB, slots, n * sizeof(int));
    size_t words = 2 * (size_t)MB + n;
    // prefill attention on MFMA: every block of rows it assigns to one workgroup is one slot
    prefillOk_ = !invariant_ && hipk::attnPrefillSupported(plan_.headSize, plan_.kvMul, kvBf16_);
    const int rpb = prefillOk_ ? hipk::attnPrefillRowsPerBlock(plan_.kvMul) : 1;
    for (int b = 0; prefillOk_ && b < n; b++) prefillOk_ = slots[b] == slots[b - b % rpb];
    // f32 caches: the f32 MFMA prefill kernel from 128 keys on; below, the per-row decode attention
    // is faster (a 32-row chunk at positions 0-63: eval 0.0957 vs 0.0993 ms/token; crossover ~135
    // keys from the 4k-prompt slopes, profiles/r6_decode.md). DL_PREFILL_F32_MIN overrides.
    if (prefillOk_ && !kvBf16_) {
        static const int f32Min = [] {
            const char *e = std::getenv("DL_PREFILL_F32_MIN");
            return e ? std::atoi(e) : 128;
        }();
        int mx = 0;
        for (int b = 0; b < n; b++) mx = std::max(mx, positions[b] + 1);
        prefillOk_ = mx >= f32Min;
    }
    if (specs) {
        static_assert(sizeof(SampleSpec) == 4 * sizeof(float), "spec layout");
        std::memcpy(hIn_ + 3 * MB, specs, n * sizeof(SampleSpec));
        words = 3 * (size_t)MB + 4 * (size_t)n;
    }
    if (procRows) {  // the rows' logit processors, behind the specs
        std::memcpy(hIn_ + 7 * MB, procRows, (size_t)n * 4 * sizeof(float));
        words = 7 * (size_t)MB + 4 * (size_t)n;
    }
    if (filterRows) {  // the rows' candidate filters, behind the processors
        static_assert(sizeof(hipk::LogitFilterRow) == 4 * sizeof(int), "filter row layout");
        std::memcpy(hIn_ + 11 * MB, filterRows, (size_t)n * sizeof(hipk::LogitFilterRow));
        words = 11 * (size_t)MB + 4 * (size_t)n;
    }
    // one copy of the row arrays (the unused tail of each is never read)
    DL_HIP(hipMemcpyAsync(dTok_, hIn_, words * sizeof(int), hipMemcpyHostToDevice, stream_));
    inputsInFlight_ = true;
}

int HipEngineImpl::batchChunk(const DevMat &m, int pro, int epi) const {
    // largest batch chunk (1/2/4) whose LDS footprint stays <= 64 KiB for this input width (8 rows
    // measured 2x slower than the MFMA GEMM: the GEMV's per-row int8 dots are VALU-bound there)
    int bc = 4;
    while (bc > 1) {
        const int rp = q40_ ? 256 / m.lanes * hipk::gemvRowGroup(bc, true) : hipk::gemvRowsPerPass(m.n, m.rows, bc, false);
        const int rpw = rp * passesFor(m, epi, bc);
        if (hipk::gemvLdsBytes(m.n, bc, q40_, rpw, pro) <= 64 * 1024) break;  // B > 1 only; B = 1 may use up to 160 KB
        bc >>= 1;
    }
    return bc;
}

// The exchange fields of a launch: a fused-exchange region (tpVec_ / tpArg_) and this exchange's measured-sync words.
void HipEngineImpl::fillXchg(hipk::TpXchg &tp, const hipk::TpXchg &region) const {
    tp = region;
    tp.ticks = syncTicks();
    tp.span = syncSpan();
}

// The EPI_QKV fields (RoPE, KV append into layer L's cache) of a GEMV / GEMM launch over the rows
// from c0 on. kvMul is read by the fused attention block's qkv role only.
void HipEngineImpl::fillLayerKv(hipk::GemvArgs &a, const DevLayer &L, int c0) const {
    a.q0 = plan_.q0;
    a.kv0 = plan_.kv0;
    a.hs = plan_.headSize;
    a.kvMul = plan_.kvMul;
    a.seqLen = h_.seqLen;
    a.rope = dRope_;
    a.pos = dPos_ + c0;
    a.slot = dSlot_ + c0;
    a.kcache = L.k;
    a.kvMap = kvMap();
    a.vcache = L.v;
    a.kvBf16 = kvBf16_ ? 1 : 0;
}

// Arguments of one GEMV launch over rows [c0, c0 + bc) of the batch (see gemv()).
hipk::GemvArgs HipEngineImpl::gemvArgs(const DevMat &m, int c0, int bc, int epi, const MatOperands &o) const {
    DL_CHECK(!o.xh && !o.ssIn && !o.outH && !o.rf.resIn, "GEMM operand on a GEMV launch");
    hipk::GemvArgs a;
    a.qs = m.qs;
    a.wd = m.d;
    a.wf = m.f;
    a.rows = m.rows;
    a.n = m.n;
    a.passes = o.tp ? tpPasses(m, bc) : passesFor(m, epi, bc);
    a.lanes = m.lanes;
    if (o.tp) fillXchg(a.tp, tpVec_);
    a.in = o.in ? o.in + (size_t)c0 * o.ldIn : nullptr;
    a.aq = o.aq ? o.aq + (size_t)c0 * m.n : nullptr;
    a.as = o.as ? o.as + (size_t)c0 * (m.n / 32) : nullptr;
    a.oq = o.oq ? o.oq + (size_t)c0 * o.ldOut : nullptr;
    a.os = o.os ? o.os + (size_t)c0 * (o.ldOut / 32) : nullptr;
    a.ldIn = o.ldIn;
    a.addIn = o.add ? o.add + (size_t)c0 * o.ldIn : nullptr;
    a.xNext = o.xNext ? o.xNext + (size_t)c0 * o.ldIn : nullptr;
    a.normW = o.normW;
    a.eps = h_.normEpsilon;
    a.out = o.out ? o.out + (size_t)c0 * o.ldOut : nullptr;
    a.ldOut = o.ldOut;
    a.act = h_.hiddenAct == HiddenAct::GELU ? 0 : 1;
    if (o.layer) fillLayerKv(a, *o.layer, c0);
    return a;
}

// Launch a GEMV over all n rows, in batch chunks of <= 4. o.tp: all-reduce the EPI_STORE output
// over the tensor-parallel ranks in the kernel tail (fused exchange).
void HipEngineImpl::gemv(const DevMat &m, int n, int pro, int epi, const MatOperands &o) {
    if (o.tp) epi = hipk::EPI_STORE_TP;
    const int bcMax = batchChunk(m, pro, epi);
    xChunk_ = 0;  // each launch's exchange waits in a measured-sync slot of its own
    for (int c0 = 0; c0 < n; xChunk_++) {
        int bc = n - c0;
        if (bc > bcMax) bc = bcMax;
        while (bc & (bc - 1)) bc &= bc - 1;  // 1, 2 or 4 rows per launch
        hipk::launchGemv(gemvArgs(m, c0, bc, epi, o), bc, pro, epi, q40_, stream_);
        c0 += bc;
    }
    xChunk_ = 0;
}

// The qkv launch reading the residual dX_[cur] through the norm prologue (layers > 0: plus the
// previous layer's delta dY_, the sum kept in the other residual buffer).
HipEngineImpl::MatOperands HipEngineImpl::qkvOperands(const DevLayer &L, int cur, bool hasDelta) const {
    return {.in = dX_[cur], .ldIn = dim(), .add = hasDelta ? dY_ : nullptr, .xNext = hasDelta ? dX_[cur ^ 1] : nullptr,
            .normW = L.rmsAtt, .out = dQ_, .ldOut = q0(), .layer = &L};
}

hipk::GemvArgs HipEngineImpl::woRowArgs(const DevLayer &L, int epi) const {
    return gemvArgs(L.wo, 0, 1, epi,
                    {.ldIn = q0(), .aq = dAttQ_, .as = dAttS_, .out = dY_, .ldOut = dim(), .tp = epi != hipk::EPI_STORE});
}

hipk::GemvArgs HipEngineImpl::w2ProducerArgs(const DevLayer &L) const {
    return gemvArgs(L.w2, 0, 1, hipk::EPI_RESQ_TP,
                    {.in = hQ80_ ? nullptr : dH_, .ldIn = hidden0(), .aq = hQ80_ ? dHQ_ : nullptr,
                     .as = hQ80_ ? dHS_ : nullptr, .out = dY_, .ldOut = dim(), .tp = true});
}

hipk::GemvArgs HipEngineImpl::w13ConsumerArgs(const DevLayer &L) const {
    return gemvArgs(L.w13, 0, 1, w13Epi(), {.ldIn = dim(), .out = dH_, .ldOut = hidden0(), .oq = dHQ_, .os = dHS_});
}

// Decode attention of this layer (rows 0..n of the forward).
hipk::AttnArgs HipEngineImpl::attnArgs(const DevLayer &L, bool bat) const {
    const ShardPlan &p = plan_;
    hipk::AttnArgs a;
    a.q = dQ_;
    a.ldq = p.q0;
    a.kcache = L.k;
    a.kvMap = kvMap();
    a.vcache = L.v;
    a.pos = dPos_;
    a.slot = dSlot_;
    a.nHeads0 = p.nHeads0;
    a.kvMul = p.kvMul;
    a.hs = p.headSize;
    a.kv0 = p.kv0;
    a.seqLen = h_.seqLen;
    a.splitGrid = bat ? buckets_[bucket_].splitGridBat : buckets_[bucket_].splitGrid;
    a.shortLen = bat ? 0 : hipk::kAttnShortLen;
    a.chunkMax = buckets_[bucket_].chunkMax;
    a.chunkMin = hipk::attnChunkMin();
    a.partO = dPartO_;
    a.partML = dPartML_;
    a.out = dAtt_;
    a.outQ = q40_ && !bat ? dAttQ_ : nullptr;
    a.outS = q40_ && !bat ? dAttS_ : nullptr;
    a.outH = bat ? dAttH_ : nullptr;
    a.ldOut = p.q0;
    a.kvBf16 = kvBf16_ ? 1 : 0;
    a.mfma = attnLong_ ? 1 : 0;
    // batch-invariant engines: one query head per workgroup whatever the rows of the launch (the
    // launch would group 2+ heads from 33 rows x 8 heads on, which reorders a row's sums: a prompt
    // prefilled next to others then left other KV than the same prompt prefilled alone)
    a.headGroup = invariant_ ? 1 : 0;
    a.counters = dAttCnt_;
    return a;
}

// The fused attention block of a single decode row (kernels.h AttnBlockArgs): qkv GEMV +
// attention + wo GEMV in one launch. Layer l, residual input dX_[cur].
hipk::AttnBlockArgs HipEngineImpl::attnBlockArgs(const DevLayer &L, u32 l, int cur) const {
    hipk::AttnBlockArgs b;
    b.qkv = gemvArgs(L.qkv, 0, 1, hipk::EPI_QKV, qkvOperands(L, cur, l > 0));
    b.at = attnArgs(L, false);
    b.wo = woRowArgs(L, woEpi());
    b.qkv.passes *= blockPassMul_;  // same-GPU rehearsals: longer workgroups (setupAttnBlock)
    b.wo.passes *= blockPassMul_;
    b.hg = hipk::attnBlockHG(b.at);
    b.layer = (int)l;
    b.nLayers = (int)h_.nLayers;
    b.epoch = dEpoch_;
    b.qkvCnt = dBlockCnt_;
    b.attnCnt = dBlockCnt_ + kMaxKvGroups * 64;
    b.attnFlag = dBlockCnt_ + kMaxKvGroups * 64 + 64;
    b.qkvExpect = dBlockExpect_;
    b.error = dBlockErr_;
    return b;
}

// Decide once per context bucket whether decode rows run the fused attention block: Q40 weights, a
// compiled instance for this shape, <= 64 KV groups, and the whole grid (whose attention role grows
// with the bucket's sequence splits) co-resident, shared with the other ranks on this GPU.
// DL_ATTN_BLOCK=0 keeps the three separate launches.
void HipEngineImpl::setupAttnBlock() {
    const char *e = std::getenv("DL_ATTN_BLOCK");
    if ((e && *e == '0') || !q40_ || plan_.nKvHeads0 > kMaxKvGroups) return;
    // one KV group per rank (8 KV heads at TP8): the attention role is a handful of workgroups
    // the whole wo role waits on - measured 2x the three launches (8B TP8 rank: 38 vs ~18 us per
    // layer, profiles/r5_tp_rank.md); DL_ATTN_BLOCK=1 forces it
    if (plan_.nKvHeads0 < 2 && !(e && *e == '1')) return;
    const int keep = bucket_;
    // qkv / wo passes per workgroup: the GEMVs' own grids. A grid beyond one round of co-resident
    // workgroups keeps the three launches: longer qkv / wo workgroups measured slower on a GPU of
    // its own (70B 8.10 -> 8.26, 405B 40.4 -> 43.3 ms/token) and in same-GPU rehearsals (ranks
    // sharing one GPU's resident slots: 8B TP2 2.91 vs 1.63 ms/token with the three launches), so
    // a rehearsal makes the production choice. Only a forced block (DL_ATTN_BLOCK=1, tests of the
    // block's exchange on one GPU) doubles the passes until the shared slots hold it.
    const bool forced = e && *e == '1';
    bucket_ = 0;
    for (blockPassMul_ = 1; forced && ranksSharingDevice() > 1 && blockPassMul_ < 8; blockPassMul_ *= 2) {
        const hipk::AttnBlockArgs b = attnBlockArgs(layers_[0], 0, 0);
        if (!hipk::attnBlockPlan(b, fusedTp(false)).fn || fitsResident(hipk::attnBlockResidency(b, fusedTp(false)))) break;
    }
    int lastOn = -1;
    hipk::GemvResidency off;
    for (size_t i = 0; i < buckets_.size(); i++) {
        bucket_ = (int)i;
        const hipk::AttnBlockArgs b = attnBlockArgs(layers_[0], 0, 0);
        if (!hipk::attnBlockPlan(b, fusedTp(false)).fn) break;
        const hipk::GemvResidency r = hipk::attnBlockResidency(b, fusedTp(false));
        if (!fitsResident(r)) {
            off = r;
            break;
        }
        buckets_[i].block = true;
        lastOn = (int)i;
        if (!blockOn_) {
            std::vector<unsigned> expect(kMaxKvGroups, 0);
            hipk::attnBlockExpect(b.qkv, (int)plan_.nKvHeads0, expect.data());
            DL_HIP(hipMemcpy(dBlockExpect_, expect.data(), expect.size() * sizeof(unsigned), hipMemcpyHostToDevice));
            blockOn_ = true;
        }
    }
    bucket_ = keep;
    if (lastOn < 0 && off.grid > 0)
        std::fprintf(stderr, "ℹ️  fused attention block off: grid %d > %d co-resident workgroups per rank\n", off.grid,
                     residentLimit(off));
}

// Pre-normalized hand-off between the single-row GEMVs of a tensor-parallel rank (kernels.h
// PRO_PRENORM / EPI_RESQ_TP): the wo / w2 exchange tails, which already hold the rank-summed rows,
// also apply the residual update and the next RMS norm's weights and quantize x * normW to Q80
// blocks, plus one sum of squares per workgroup; the consumers (qkv, w13, logits) copy those blocks
// and fold in 1 / rms instead of re-reading x and the delta and reducing 4096 values in every
// workgroup. Measured per launch (scripts/trace_gemv.py, norm vs copy prologue): qkv 5.71 vs 4.69
// us at TP1 shapes, and at a TP8 rank's shards qkv 4.35 vs 3.13, w13 5.18 vs 3.96.
// Needs producers whose workgroups own whole 32-row blocks (the Q80 exchange's tpPasses) and at
// most kMaxSsp of them, the fused exchange (separate collectives keep the norm prologue) and
// no attention block in the forward (the block's roles keep theirs). DL_PRENORM=0 disables it.
void HipEngineImpl::setupPrenorm() {
    prenormOn_ = false;
    const char *e = std::getenv("DL_PRENORM");
    if ((e && *e == '0') || !q40_ || !fusedTp(false) || h_.dim % 32 || h_.dim > 16384) return;
    const hipk::GemvArgs producers[2] = {woRowArgs(layers_[0], hipk::EPI_RESQ_TP), w2ProducerArgs(layers_[0])};
    const int pros[2] = {hipk::PRO_GLOBAL, w2Pro()};
    for (int w = 0; w < 2; w++) {
        const hipk::GemvArgs &a = producers[w];
        if (rowsPerWorkgroup(a) % 32 || gemvGrid(a) > kMaxSsp) return;
        if (!fitsResident(hipk::gemvResidency(a, 1, pros[w], hipk::EPI_RESQ_TP, true))) return;
    }
    prenormOn_ = true;
}

// The logits GEMV `a` of one greedy decode row, ending in the row's argmax (EPI_ARGMAX; under TP the
// winners trade over the fused exchange's region; CHAIN also feeds the token back, as ArgmaxArgs).
void HipEngineImpl::launchArgmaxTail(hipk::GemvArgs a, int pro, GraphKind kind) {
    a.am.ids = dIds_;
    a.am.partV = dArgV_;
    a.am.partI = dArgI_;
    a.am.counter = dArgCnt_;
    a.am.vocabStart = plan_.vocabStart();
    if (kind == GraphKind::CHAIN) {
        a.am.tokens = dTok_;
        a.am.pos = dPos_;
        a.am.hist = dHist_;
    }
    if (plan_.nRanks > 1) fillXchg(a.tp, tpArg_);
    hipk::launchGemv(a, 1, pro, hipk::EPI_ARGMAX, true, stream_);
}

// The layers + logits of one decode row with the pre-normalized hand-offs (setupPrenorm). The
// residual lives in dX_[cur]; its Q80 image for the next consumer in dXQ_ / dXS_ [cur] with sspN
// partial sums in dSSP_[cur]; each producer writes the other parity and flips cur.
void HipEngineImpl::enqueuePrenormLayers(const FwdPath &f, GraphKind kind) {
    int cur = 0, sspN[2] = {0, 0};
    auto consumer = [&](hipk::GemvArgs a) {
        a.aq = dXQ_[cur];
        a.as = dXS_[cur];
        a.sspIn = dSSP_[cur];
        a.nSsp = sspN[cur];
        return a;
    };
    auto producer = [&](hipk::GemvArgs a, const float *normW) {
        a.rq.resIn = dX_[cur];
        a.rq.resOut = dX_[cur ^ 1];
        a.rq.resW = normW;
        a.rq.xq = dXQ_[cur ^ 1];
        a.rq.xs = dXS_[cur ^ 1];
        a.rq.ssp = dSSP_[cur ^ 1];
        sspN[cur ^ 1] = gemvGrid(a);
        return a;
    };
    for (u32 l = 0; l < h_.nLayers; l++) {
        DevLayer &L = layers_[l];
        xSlot_ = 2 * (int)l;
        xChunk_ = 0;
        // layer 0's qkv normalizes the embedding's row itself (norm prologue): the one-workgroup
        // embedding kernel measured 12.8 vs 4.9 us with the pre-normalized output (PrenormOut)
        if (l == 0) {
            enqueueQkv(f, L, 0, false);
        } else {
            ProfScope ps(this, "gemv_qkv");
            const hipk::GemvArgs a =
                consumer(gemvArgs(L.qkv, 0, 1, hipk::EPI_QKV, {.ldIn = dim(), .out = dQ_, .ldOut = q0(), .layer = &L}));
            hipk::launchGemv(a, 1, hipk::PRO_PRENORM, hipk::EPI_QKV, true, stream_);
        }
        enqueueAttention(f, L);
        {
            ProfScope ps(this, "gemv_wo");
            const hipk::GemvArgs a = producer(woRowArgs(L, hipk::EPI_RESQ_TP), L.rmsFfn);
            hipk::launchGemv(a, 1, hipk::PRO_GLOBAL, hipk::EPI_RESQ_TP, true, stream_);
            cur ^= 1;
        }
        xSlot_ = 2 * (int)l + 1;
        const hipk::GemvArgs a13 = consumer(w13ConsumerArgs(L));
        const hipk::GemvArgs a2 = producer(w2ProducerArgs(L), nextNormW(l));
        {
            ProfScope ps(this, "gemv_w13");
            hipk::launchGemv(a13, 1, hipk::PRO_PRENORM, w13Epi(), true, stream_);
        }
        {
            ProfScope ps(this, "gemv_w2");
            hipk::launchGemv(a2, 1, w2Pro(), hipk::EPI_RESQ_TP, true, stream_);
        }
        cur ^= 1;
    }
    xSlot_ = 2 * (int)h_.nLayers;  // logits gather / argmax winners
    ProfScope ps(this, "gemv_logits");
    const int epi = f.argTail ? hipk::EPI_ARGMAX : hipk::EPI_STORE;
    const hipk::GemvArgs a =
        consumer(gemvArgs(wcls_, 0, 1, epi, {.ldIn = dim(), .out = f.argTail ? nullptr : dLogits_, .ldOut = vocab0()}));
    if (f.argTail)
        launchArgmaxTail(a, hipk::PRO_PRENORM, kind);
    else
        hipk::launchGemv(a, 1, hipk::PRO_PRENORM, hipk::EPI_STORE, true, stream_);
}

// A fused-block wait gave up (a workgroup of the launch never arrived): reset the monotonic
// counters and the epoch so the engine stays usable, then raise.
void HipEngineImpl::resetAttnBlockState() {
    DL_HIP(hipMemsetAsync(dBlockCnt_, 0, sizeof(unsigned) * kBlockCntWords, stream_));
    DL_HIP(hipMemsetAsync(dEpoch_, 0, sizeof(unsigned), stream_));
    DL_HIP(hipMemsetAsync(dBlockErr_, 0, sizeof(int), stream_));
    DL_HIP(hipStreamSynchronize(stream_));
}

// Batched path (>= gemmMinTokens rows, Q40 or F32 weights): per chunk of <= 64 tokens, a norm kernel (f32 ->
// f16, RESNORM) or the producer's f16 rows (xh) feed the MFMA GEMM with the fused epilogue.
// Residual + norm fusion between batched GEMMs at TP1 (DL_GEMM_FUSE_NORM=0 disables, read at
// construction): wo / w2 end with EPI_RES (x' = x + out, x' * normW -> f16, per-tile sums of squares)
// and the next GEMM applies the RMS scale per token in its epilogue: no norm kernel between.
// At TP > 1 the batched path keeps the fused residual + norm too when the wo / w2 tiles can be
// all-reduced inside their GEMM epilogue (GemmArgs::tpx over the fused exchange: narrow
// launches of <= 64 rows whose tile + Q80 staging fit the launch's LDS); otherwise a separate
// all-reduce kernel and a norm kernel follow each of them. DL_TP_BATCHED=0 disables it.
bool HipEngineImpl::tpBatchedOk(int n) const {
    static const bool on = [] {
        const char *e = std::getenv("DL_TP_BATCHED");
        return !(e && *e == '0');
    }();
    return on && !invariant_ && tpFused_ && q40_ && !hipk::gemmUsesWide(n) &&
           (size_t)n * h_.dim <= (size_t)tpVec_.stride && hipk::gemmTpxFits(n, plan_.nRanks, tpVec_.q80 != 0);
}

void HipEngineImpl::gemmBatched(const DevMat &m, int n, int epi, const MatOperands &o) {
    DL_CHECK(!o.aq && !o.as && !o.oq && !o.os && !o.tp, "GEMV operand on a GEMM launch");
    // tokens per launch: the wide Q40 kernel takes the whole forward in one launch (one weight
    // pass per token tile, all tiles of a row tile on one XCD), the narrow one <= 128
    // (batch-invariant engines: narrow launches only, the split count of a 16-token launch for all)
    // (a width the wide kernel cannot split into its two-block stages: narrow launches too)
    const int chunk = hipk::gemmChunkTokens(m.n, n, q40_, invariant_);
    for (int c0 = 0; c0 < n; c0 += chunk) {
        const int bc = std::min(chunk, n - c0);
        xChunk_ = c0 / chunk;  // each launch's tile exchange waits in a measured-sync slot of its own
        hipk::GemmArgs g;
        hipk::GemvArgs &a = g.e;
        a.qs = m.qs;
        a.wd = m.d;
        a.wf = m.f;
        a.rows = m.rows;
        a.n = m.n;
        a.lanes = m.lanes;
        a.eps = h_.normEpsilon;
        if (o.ssIn) {  // input = the producer's x' * normW rows; RMS scale applied per token
            g.x = dXh_ + (size_t)c0 * m.n;
            g.ssIn = dSS_ + c0;
            g.ssTiles = (h_.dim + 63) / 64;
            g.ldSS = (int)cfg_.maxBatch;
        } else if (!o.xh) {
            hipk::GemvArgs nq;
            nq.n = m.n;
            nq.in = o.in + (size_t)c0 * o.ldIn;
            nq.ldIn = o.ldIn;
            nq.addIn = o.add ? o.add + (size_t)c0 * o.ldIn : nullptr;
            nq.xNext = o.xNext ? o.xNext + (size_t)c0 * o.ldIn : nullptr;
            nq.normW = o.normW;
            nq.eps = h_.normEpsilon;
            hipk::launchNormF16(nq, dXh_, bc, stream_);
            g.x = dXh_;
        } else {
            g.x = o.xh + (size_t)c0 * m.n;
        }
        a.out = o.out ? o.out + (size_t)c0 * o.ldOut : nullptr;
        g.outH = o.outH ? o.outH + (size_t)c0 * o.ldOut : nullptr;
        a.ldOut = o.ldOut;
        a.act = h_.hiddenAct == HiddenAct::GELU ? 0 : 1;
        if (o.layer) fillLayerKv(a, *o.layer, c0);
        if (o.rf.resIn && plan_.nRanks > 1) {  // the residual update needs the rank-summed tile
            g.tpx = 1;
            fillXchg(a.tp, tpVec_);
        }
        if (o.rf.resIn) {
            g.resIn = o.rf.resIn + (size_t)c0 * o.ldOut;
            g.resOut = o.rf.resOut + (size_t)c0 * o.ldOut;
            g.resW = o.rf.w;
            g.resX = dXh_ + (size_t)c0 * o.ldOut;
            g.ssOut = dSS_ + c0;
            g.ldSS = (int)cfg_.maxBatch;
        }
        g.M = bc;
        g.splits = invariant_ ? hipk::gemmSplits(m.rows, m.n, 16, 0) : hipk::gemmSplits(m.rows, m.n, bc, q40_ ? m.lanes : 0);
        g.fixed = invariant_ ? 1 : 0;
        g.part = dPart_;
        g.partFloats = partFloats_;
        g.counters = dGemmCnt_;
        if (q40_)
            hipk::launchGemmQ40(g, epi, stream_);
        else
            hipk::launchGemmF32(g, epi, stream_);
    }
}

// Separate all-reduce of partial sums (batched path, RCCL, f32 weights). Q80 sync: every rank's
// partial is first rounded through Q80 blocks, as the reference's ZQ cast (llm.cpp:308-314).
void HipEngineImpl::allReduce(float *buf, size_t count) {
    if (plan_.nRanks > 1) {
        ProfScope ps(this, "allreduce");
        stamped([&] {
            if (syncQ80_) hipk::launchQ80Roundtrip(buf, count, stream_);
            comm_->allReduceSum(buf, count, stream_);
        });
    }
}

// The per-matrix steps of a layer (enqueueForward): each picks its launch from the forward's path -
// the fused-norm GEMM (input: the producer GEMM's rows), the GEMM behind a norm kernel, or the GEMV.
void HipEngineImpl::enqueueQkv(const FwdPath &f, const DevLayer &L, int cur, bool hasDelta) {
    ProfScope ps(this, "gemv_qkv");
    if (f.fz && hasDelta)
        gemmBatched(L.qkv, f.n, hipk::EPI_QKV, {.ssIn = true, .out = dQ_, .ldOut = q0(), .layer = &L});
    else if (f.bat)
        gemmBatched(L.qkv, f.n, hipk::EPI_QKV, qkvOperands(L, cur, hasDelta));
    else
        gemv(L.qkv, f.n, hipk::PRO_RESNORM, hipk::EPI_QKV, qkvOperands(L, cur, hasDelta));
}

void HipEngineImpl::enqueueAttention(const FwdPath &f, const DevLayer &L) {
    ProfScope ps(this, "attention");
    const hipk::AttnArgs a = attnArgs(L, f.bat);
    for (int r0 = 0; r0 < f.n; r0 += attRows_) {  // one launch unless the partials cap the rows
        const int nr = std::min(attRows_, f.n - r0);
        hipk::AttnArgs ar = a;
        ar.q += (size_t)r0 * a.ldq;
        ar.pos += r0;
        ar.slot += r0;
        ar.out += (size_t)r0 * a.ldOut;
        if (ar.outH) ar.outH += (size_t)r0 * a.ldOut;
        if (ar.outQ) ar.outQ += (size_t)r0 * a.ldOut;
        if (ar.outS) ar.outS += (size_t)r0 * (a.ldOut / 32);
        if (f.bat && prefillOk_)
            hipk::launchAttentionPrefill(ar, nr, stream_);
        else
            hipk::launchAttention(ar, nr, stream_);
    }
}

void HipEngineImpl::enqueueWo(const FwdPath &f, const DevLayer &L, int cur) {
    ProfScope ps(this, "gemv_wo");
    if (f.fz)
        gemmBatched(L.wo, f.n, hipk::EPI_RES, {.xh = dAttH_, .ldOut = dim(), .rf = {dX_[cur], dX_[cur ^ 1], L.rmsFfn}});
    else if (f.bat)
        gemmBatched(L.wo, f.n, hipk::EPI_STORE, {.xh = dAttH_, .out = dY_, .ldOut = dim()});
    else
        gemv(L.wo, f.n, hipk::PRO_GLOBAL, hipk::EPI_STORE,
             {.in = q40_ ? nullptr : dAtt_, .ldIn = q0(), .aq = dAttQ_, .as = dAttS_, .out = dY_, .ldOut = dim(),
              .tp = fusedTp(false)});
}

void HipEngineImpl::enqueueW13(const FwdPath &f, const DevLayer &L, int cur) {
    ProfScope ps(this, "gemv_w13");
    if (f.fz)
        gemmBatched(L.w13, f.n, hipk::EPI_ACT_F16, {.ssIn = true, .ldOut = hidden0(), .outH = dHh_});
    else if (f.bat)
        gemmBatched(L.w13, f.n, hipk::EPI_ACT_F16,
                    {.in = dX_[cur], .ldIn = dim(), .add = dY_, .xNext = dX_[cur ^ 1], .normW = L.rmsFfn,
                     .ldOut = hidden0(), .outH = dHh_});
    else
        gemv(L.w13, f.n, hipk::PRO_RESNORM, w13Epi(),
             {.in = dX_[cur], .ldIn = dim(), .add = dY_, .xNext = dX_[cur ^ 1], .normW = L.rmsFfn, .out = dH_,
              .ldOut = hidden0(), .oq = dHQ_, .os = dHS_});
}

void HipEngineImpl::enqueueW2(const FwdPath &f, u32 l, int cur) {
    ProfScope ps(this, "gemv_w2");
    const DevLayer &L = layers_[l];
    if (f.fz)
        gemmBatched(L.w2, f.n, hipk::EPI_RES, {.xh = dHh_, .ldOut = dim(), .rf = {dX_[cur], dX_[cur ^ 1], nextNormW(l)}});
    else if (f.bat)
        gemmBatched(L.w2, f.n, hipk::EPI_STORE, {.xh = dHh_, .out = dY_, .ldOut = dim()});
    else if (!q40_ || hQ80_)
        gemv(L.w2, f.n, hipk::PRO_GLOBAL, hipk::EPI_STORE,
             {.in = q40_ ? nullptr : dH_, .ldIn = hidden0(), .aq = dHQ_, .as = dHS_, .out = dY_, .ldOut = dim(),
              .tp = fusedTp(false)});
    else
        gemv(L.w2, f.n, hipk::PRO_RESNORM, hipk::EPI_STORE,
             {.in = dH_, .ldIn = hidden0(), .out = dY_, .ldOut = dim(), .tp = fusedTp(false)});
}

// The logits of the forward's rows from the residual dX_[cur] + dY_ (argTail: the row's argmax).
void HipEngineImpl::enqueueLogits(const FwdPath &f, GraphKind kind, int cur) {
    xSlot_ = 2 * (int)h_.nLayers;  // logits gather / argmax winners
    ProfScope ps(this, "gemv_logits");
    const MatOperands o{.in = dX_[cur], .ldIn = dim(), .add = dY_, .normW = rmsFinal_,
                        .out = f.argTail ? nullptr : dLogits_, .ldOut = vocab0()};
    if (f.fz)
        gemmBatched(wcls_, f.n, hipk::EPI_STORE, {.ssIn = true, .out = dLogits_, .ldOut = vocab0()});
    else if (f.bat)
        gemmBatched(wcls_, f.n, hipk::EPI_STORE, o);
    else if (f.argTail)
        launchArgmaxTail(gemvArgs(wcls_, 0, 1, hipk::EPI_ARGMAX, o), hipk::PRO_RESNORM, kind);
    else
        gemv(wcls_, f.n, hipk::PRO_RESNORM, hipk::EPI_STORE, o);
}

// From the logits of n rows to their token ids: (gather) -> argmax / draw.
void HipEngineImpl::enqueueTokenPick(int n, FwdKind k) {
    const ShardPlan &p = plan_;
    const GraphKind kind = k.kind;
    const float *full = dLogits_;
    // greedy rows under tensor parallelism: each rank reduces its own vocab slice and only the
    // (value, index) winners cross the links (reference: logits gathered to the root,
    // llm.cpp:432) - inside the argmax kernel on the fused data plane, else as one all-gather of
    // 2 floats per row; the full logits are gathered only when the host samples them
    const bool greedy = kind == GraphKind::ARGMAX || kind == GraphKind::CHAIN;
    const bool distArgmax = p.nRanks > 1 && greedy;
    // logits for the host (LOGITS) and sampled rows (SAMPLE) are needed on the root only: the
    // vocab slices are gathered to rank 0 (the reference's SYNC_NODE_SLICES_EXCEPT_ROOT), the
    // other ranks publish theirs and skip the unshard and the draw (the root's ids are used)
    const bool rootOnly = kind == GraphKind::LOGITS || kind == GraphKind::SAMPLE;
    if (p.nRanks > 1 && !distArgmax) {
        ProfScope ps(this, "allgather");
        stamped([&] {
            if (rootOnly)
                comm_->gatherToRoot(dLogits_, dLogitsAll_, (size_t)n * p.vocab0, stream_);
            else
                comm_->allGather(dLogits_, dLogitsAll_, (size_t)n * p.vocab0, stream_);
        });
        if (!rootOnly || rank() == 0) hipk::launchUnshardLogits(dLogitsAll_, dLogitsFull_, p.nRanks, n, p.vocab0, stream_);
        full = dLogitsFull_;
    }
    if (kind == GraphKind::SAMPLE) {
        if (p.nRanks == 1 || rank() == 0) enqueueDraw(n, k.stages, full);  // the other ranks' ids are not used
    } else if (kind != GraphKind::LOGITS) {
        ProfScope ps(this, "argmax");
        hipk::ArgmaxArgs g;
        g.logits = full;
        g.vocab = h_.vocabSize;
        if (distArgmax) {
            g.vocab = p.vocab0;
            g.vocabStart = p.vocabStart();
            // fused winners exchange up to its region's rows (2 words per row), else one all-gather
            if (tpFused_ && (size_t)2 * n <= (size_t)tpArg_.stride)
                fillXchg(g.tp, tpArg_);
            else
                g.pairs = dArgPairs_;
        }
        g.ids = dIds_;
        g.partV = dArgV_;
        g.partI = dArgI_;
        g.counters = dArgCnt_;
        if (kind == GraphKind::CHAIN) {
            // feed the sampled token back: tokens := ids, hist[b][pos] := ids, pos += 1
            g.tokens = dTok_;
            g.pos = dPos_;
            g.hist = dHist_;
            g.seqLen = h_.seqLen;
        }
        hipk::launchArgmax(g, n, stream_);
        if (g.pairs) {
            stamped([&] { comm_->allGather(dArgPairs_, dArgPairsAll_, 2 * (size_t)n, stream_); });
            hipk::launchArgmaxPick(g, dArgPairsAll_, n, p.nRanks, stream_);
        }
    }
}

// The draw of n sampled rows from their full logits, with the forward's stages around the sampler
// (root only). PROC: the drawn rows' penalties and bias into the processed buffer, which every later
// stage and the sampler read instead; the raw logits stay for the log-probabilities; the drawn tokens
// are counted behind the draw. JSON, GRAMMAR: the token masks on the processed rows (each takes the
// rows of its own kind) ahead of the filter, so top_k counts allowed tokens only, and the slots'
// states advanced by the drawn tokens behind the draw. FILTER: top_k / min_p mask the processed rows
// in place; the filter's partial histograms and maxima live in the sampler's scratch, which the
// sampler rewrites before it reads it.
void HipEngineImpl::enqueueDraw(int n, unsigned stages, const float *full) {
    const bool proc = stages & PROC;
    auto stage = [&](DrawStage st, const char *name, auto &&launch) {
        if (!(stages & st)) return;
        ProfScope ps(this, name);
        launch();
    };
    stage(PROC, "logit_proc", [&] { hipk::launchLogitProc(logitProcArgs(full), n, stream_); });
    stage(JSON, "json_mask", [&] { hipk::launchJsonMask(constraintArgs(), n, stream_); });
    stage(GRAMMAR, "grammar_mask", [&] { hipk::launchGrammarMask(constraintArgs(), n, stream_); });
    stage(FILTER, "logit_filter", [&] {
        hipk::LogitFilterArgs f;
        f.logits = dProcLogits_;
        f.vocab = h_.vocabSize;
        f.spec = dSpec_;
        f.rows = dFilter_;
        f.hist = reinterpret_cast<uint32_t *>(sampleScratch_.hist);
        f.part = sampleScratch_.part;
        f.state = dFilterState_;
        hipk::launchLogitFilter(f, n, stream_);
    });
    {
        ProfScope ps(this, "sample");
        hipk::SampleArgs g;
        g.logits = proc ? dProcLogits_ : full;
        g.vocab = h_.vocabSize;
        g.spec = dSpec_;
        g.ids = dIds_;
        g.scratch = sampleScratch_;
        hipk::launchSample(g, n, stream_);
    }
    stage(PROC, "logit_proc", [&] { hipk::launchLogitProcCount(logitProcArgs(full), n, stream_); });
    stage(JSON, "json_mask", [&] { hipk::launchJsonAdvance(constraintArgs(), n, stream_); });
    stage(GRAMMAR, "grammar_mask", [&] { hipk::launchGrammarAdvance(constraintArgs(), n, stream_); });
}

// The forward of n rows: embedding -> nLayers x [qkv (+RoPE, KV append) -> attention -> wo
// (-> all-reduce) -> w13 (SwiGLU) -> w2 (-> all-reduce)] -> logits -> (gather) -> argmax / sample.
// Single decode rows (GEMV path) run qkv + attention + wo as one fused attention-block launch when
// the context bucket allows it; batched rows run the MFMA GEMMs with residual + norm fused into
// their epilogues (reference step list: llm.cpp:200-434, ~840 barrier steps per forward).
void HipEngineImpl::enqueueForward(int n, FwdKind k) {
    const GraphKind kind = k.kind;
    FwdPath f{.n = n, .bat = batchedPath(n)};
    f.fz = f.bat && fuseNorm(n);
    f.blk = blockOn_ && buckets_[bucket_].block && n == 1 && !f.bat;
    const bool row = n == 1 && !f.bat && !f.blk;  // a single decode row outside the block
    // (an all-embedding forward keeps the norm-prologue schedule, whose final residual is the
    //  dX_ / dY_ pair the pooling kernel reads; the pre-normalized hand-off holds Q80 images instead)
    f.pre = prenormOn_ && row && kind != GraphKind::EMBED;
    // one greedy decode row: the logits GEMV ends in the row's argmax (EPI_ARGMAX: no logits
    // written, no argmax launch; under TP the winners trade over the fused exchange's region)
    f.argTail = argTailOn_ && q40_ && !f.bat && !f.fz && n == 1 &&
                (kind == GraphKind::ARGMAX || kind == GraphKind::CHAIN) &&
                (plan_.nRanks == 1 || (tpFused_ && tpArg_.stride >= 2));
    {
        ProfScope ps(this, "embedding");
        // the epoch counts the forwards that run the fused attention block (its counters' targets)
        unsigned *ep = f.blk ? dEpoch_ : nullptr;
        hipk::launchEmbedding(emb_, dTok_, dX_[0], dim(), n, stream_, ep,
                              plan_.nRanks > 1 ? dSync_ : nullptr, plan_.nRanks > 1 ? syncSlots() : 0);
    }
    const bool sepReduce = !fusedTp(f.bat) && !f.fz;  // wo / w2 partial sums: a separate all-reduce
    int cur = 0;
    for (u32 l = 0; l < h_.nLayers && !f.pre; l++) {
        DevLayer &L = layers_[l];
        const bool hasDelta = l > 0;
        xSlot_ = 2 * (int)l;  // the wo exchange (fused in the wo kernel, or the all-reduce after it)
        if (f.blk) {
            ProfScope ps(this, "attn_block");
            hipk::AttnBlockArgs ba = attnBlockArgs(L, l, cur);
            if ((int)l == traceLayer_) ba.trace = traceBuf_;
            hipk::launchAttnBlock(ba, fusedTp(false), stream_);
            if (hasDelta) cur ^= 1;
        } else {
            enqueueQkv(f, L, cur, hasDelta);
            if (hasDelta) cur ^= 1;
            enqueueAttention(f, L);
            enqueueWo(f, L, cur);
        }
        if (sepReduce) allReduce(dY_, (size_t)n * dim());
        xSlot_ = 2 * (int)l + 1;  // the w2 exchange
        enqueueW13(f, L, cur);
        cur ^= 1;
        enqueueW2(f, l, cur);
        if (sepReduce) allReduce(dY_, (size_t)n * dim());
    }
    if (kind == GraphKind::EMBED) {  // no wcls, no logits exchange, no token pick on any rank
        DL_CHECK(cur == 1, "final residual parity");  // what poolArgs reads
        if (poolStaged_) enqueuePool(n);
    } else {
        if (f.pre)
            enqueuePrenormLayers(f, kind);
        else
            enqueueLogits(f, kind, cur);
        if (!f.argTail) enqueueTokenPick(n, k);
    }
    DL_HIP(hipGetLastError());
}

}  // namespace engine_detail
}  // namespace dl
