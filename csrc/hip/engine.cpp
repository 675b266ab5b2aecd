// HipEngine: construction, public entry points, hipGraph cache and error checks (engine_impl.h
// lists the other translation units of the engine).
#include "engine_impl.h"

#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace dl {

int hipDeviceCount() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

namespace engine_detail {

HipEngineImpl::HipEngineImpl(const EngineConfig &cfg, DeviceComm *comm) : cfg_(cfg), comm_(comm) {
    const int nDev = hipDeviceCount();
    if (nDev <= 0) throw Error("No HIP device available");
    dev_ = cfg.gpuIndex >= 0 ? cfg.gpuIndex : 0;
    DL_CHECK(dev_ < nDev, "gpu index out of range");
    DL_HIP(hipSetDevice(dev_));
    DL_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));

    const u32 nRanks = comm_ ? comm_->size() : 1, rank = comm_ ? comm_->rank() : 0;
    if (cfg.synthetic) {
        h_ = cfg.syntheticHeader;
        h_.origSeqLen = h_.seqLen;
        if (cfg.maxSeqLen > 0 && h_.seqLen > cfg.maxSeqLen) h_.seqLen = cfg.maxSeqLen;
    } else {
        file_.reset(new ModelFile(cfg.modelPath, cfg.maxSeqLen));
        h_ = file_->header();
    }
    plan_ = ShardPlan::make(h_, nRanks, rank);
    q40_ = h_.weightType == FloatType::Q40;
    if (q40_ && cfg.bufferType != FloatType::Q80)
        throw Error("This version supports only Q40 weights with Q80 sync type");
    if (!q40_ && h_.weightType != FloatType::F32) throw Error("unsupported weight type");
    DL_CHECK(h_.headSize() == 64 || h_.headSize() == 128, "GPU kernels support head size 64 or 128");
    DL_CHECK(cfg.maxBatch >= 1 && cfg.nSlots >= 1, "maxBatch/nSlots");
    DL_CHECK(cfg.maxBatch <= kKeyMaxRows, "maxBatch: more rows than a graph key holds");
    kvBf16_ = cfg.kvBf16;
    syncQ80_ = cfg.syncType == FloatType::Q80;
    decodeRows_ = (int)(cfg.maxDecode ? std::min(cfg.maxDecode, cfg.maxBatch) : cfg.maxBatch);
    if (comm_ && plan_.nRanks > 1) {
        const char *e = std::getenv("DL_TP_FUSED");  // 0: separate all-reduce kernels (comparison)
        tpFused_ = !(e && *e == '0') && comm_->fusedXchg(0, &tpVec_) && comm_->fusedXchg(1, &tpArg_) &&
                   (size_t)std::min<u32>(cfg.maxBatch, 4) * h_.dim <= (size_t)tpVec_.stride &&
                   (size_t)2 * decodeRows_ <= (size_t)tpArg_.stride;  // larger argmax forwards: all-gather
        tpVec_.q80 = syncQ80_ ? 1 : 0;
    }
    checkFits();
    {
        const char *hq = std::getenv("DL_H_Q80");
        hQ80_ = hq && *hq ? *hq == '1' : plan_.hidden0 / 32 >= 192;
    }
    if (tpFused_) checkFusedResidency();
    {  // path knobs, read once: a captured graph replays the path it was captured with
        const char *e = std::getenv("DL_GEMM_MIN");
        gemmMin_ = e && *e ? std::atoi(e) : (plan_.nRanks > 1 ? 5 : 3);
        // batch-invariant serving: every row of every forward takes the narrow MFMA GEMMs (fixed
        // splits, no 16-lane / wide variants) and the VALU decode attention, so a row's math does
        // not depend on how many rows share its forward (EngineConfig::batchInvariant)
        invariant_ = cfg.batchInvariant;
        if (invariant_) gemmMin_ = 1;
        const char *f = std::getenv("DL_GEMM_FUSE_NORM");
        fuseNormEnv_ = !(f && *f == '0');
    }
    Timer timer;
    allocBuffers();
    if (cfg.synthetic)
        loadSynthetic();
    else
        loadFromFile();
    uploadRope();
    DL_HIP(hipStreamSynchronize(stream_));
    setupAttnBlock();
    setupPrenorm();
    hipk::preloadModules();  // no code-object load inside the first forwards
    load_.ms = timer.elapsedMs();
    load_.deviceBytes = deviceBytes_;
}

HipEngineImpl::~HipEngineImpl() {
    (void)hipSetDevice(dev_);
    for (auto &kv : graphs_) (void)hipGraphExecDestroy(kv.second);
    for (void *p : allocs_) (void)hipFree(p);
    for (void *p : hostAllocs_) (void)hipHostFree(p);
    if (hLogits_) (void)hipHostFree(hLogits_);
    for (auto &e : chainEv_)
        if (e) (void)hipEventDestroy(e);
    if (stream_) (void)hipStreamDestroy(stream_);
}

std::vector<unsigned long long> HipEngineImpl::traceAttnBlock(int token, int pos, int slot, int layer) {
    if (!blockOn_) return {};
    bucket_ = (int)(&bucketFor(pos) - buckets_.data());
    if (!buckets_[bucket_].block) return {};
    const hipk::AttnBlockPlan pl = hipk::attnBlockPlan(attnBlockArgs(layers_[0], 0, 0), fusedTp(false));
    const int g[3] = {pl.gq, pl.ga, pl.gw};
    const size_t words = 8 * (size_t)(g[0] + g[1] + g[2]);
    traceBuf_ = dalloc<unsigned long long>(words);
    DL_HIP(hipMemsetAsync(traceBuf_, 0, words * 8, stream_));
    traceLayer_ = layer;
    setInputs(1, &token, &pos, &slot);
    enqueueForward(1, GraphKind::LOGITS);
    syncAndCheckComm();
    inputsInFlight_ = false;
    std::vector<unsigned long long> out(3 + words);
    for (int i = 0; i < 3; i++) out[i] = (unsigned long long)g[i];
    DL_HIP(hipMemcpy(out.data() + 3, traceBuf_, words * 8, hipMemcpyDeviceToHost));
    traceLayer_ = -1;
    traceBuf_ = nullptr;  // (one small buffer per call, released with the engine)
    return out;
}

void HipEngineImpl::forward(int n, const int *tokens, const int *positions, const int *slots, float *logits) {
    Timer t;
    setInputs(n, tokens, positions, slots);
    runGraph(n, GraphKind::LOGITS);
    const bool root = rank() == 0;
    if (root && logits && (size_t)n * h_.vocabSize > hLogitsCap_) {  // pinned staging, grown on demand
        if (hLogits_) DL_HIP(hipHostFree(hLogits_));
        hLogitsCap_ = (size_t)n * h_.vocabSize;
        DL_HIP(hipHostMalloc(reinterpret_cast<void **>(&hLogits_), hLogitsCap_ * sizeof(float), hipHostMallocDefault));
    }
    if (root && logits) {
        const float *src = plan_.nRanks > 1 ? dLogitsFull_ : dLogits_;
        DL_HIP(hipMemcpyAsync(hLogits_, src, (size_t)n * h_.vocabSize * sizeof(float), hipMemcpyDeviceToHost, stream_));
    }
    syncAndCheckComm();
    inputsInFlight_ = false;
    if (root && logits) std::memcpy(logits, hLogits_, (size_t)n * h_.vocabSize * sizeof(float));
    stats_.computeMs = t.elapsedMs();
    setSyncStats(readSync(hSync_, false), stats_.computeMs);
}

void HipEngineImpl::forwardArgmax(int n, const int *tokens, const int *positions, const int *slots, int *out) {
    Timer t;
    setInputs(n, tokens, positions, slots);
    runGraph(n, GraphKind::ARGMAX);
    DL_HIP(hipMemcpyAsync(hIds_, dIds_, n * sizeof(int), hipMemcpyDeviceToHost, stream_));
    syncAndCheckComm();
    inputsInFlight_ = false;
    std::memcpy(out, hIds_, n * sizeof(int));
    stats_.computeMs = t.elapsedMs();
    setSyncStats(readSync(hSync_, false), stats_.computeMs);
}

void HipEngineImpl::forwardSample(int n, const int *tokens, const int *positions, const int *slots,
                                  const SampleSpec *specs, int *out) {
    Timer t;
    enqueueSampled(n, tokens, positions, slots, specs);
    syncAndCheckComm();
    inputsInFlight_ = false;
    std::memcpy(out, hIds_, n * sizeof(int));
    readLogprobs();
    readPooled();
    stats_.computeMs = t.elapsedMs();
    setSyncStats(readSync(hSync_, false), stats_.computeMs);
}

// Pipelined serving: the forward and the D2H copy of its ids are enqueued; the host returns at
// once (inputs are staged in pinned memory: the previous forward was collected before).
void HipEngineImpl::launchIds(int n, const int *tokens, const int *positions, const int *slots,
                              const SampleSpec *specs) {
    DL_CHECK(pendingN_ == 0, "launchIds: the previous forward was not collected");
    Timer t;
    enqueueSampled(n, tokens, positions, slots, specs);
    pendingN_ = n;
    stats_.computeMs = t.elapsedMs();  // host enqueue time; the sync is read when collected
}

void HipEngineImpl::collectIds(int *out) {
    DL_CHECK(pendingN_ > 0, "collectIds: nothing launched");
    const int n = pendingN_;
    pendingN_ = 0;
    syncAndCheckComm();
    inputsInFlight_ = false;
    std::memcpy(out, hIds_, n * sizeof(int));
    readLogprobs();
    readPooled();
    setSyncStats(readSync(hSync_, false), -1);
}

// A forward whose result is one id per row (forwardSample, launchIds; specs null: argmax), enqueued up
// to the D2H copy of the ids. With a pooling handed over (Backend::setPooling) and a taking-part row:
// an all-embedding forward (no row draws) runs the EMBED kind, whose ids are all -1; any other keeps
// its kind and the graphs it always replayed, and launchPool follows the token pick on the same
// stream - not inside the graph, like launchLogprobs.
void HipEngineImpl::enqueueSampled(int n, const int *tokens, const int *positions, const int *slots,
                                   const SampleSpec *specs) {
    const std::vector<int> targets = takeLogprobTargets(n, specs);  // (checked before anything is enqueued)
    std::vector<LogitProc> procs;
    FwdKind k(GraphKind::SAMPLE, beginProcs(n, slots, specs, procs));
    const std::vector<PoolSpec> pool = beginPooling(n, positions, slots);
    if (!pool.empty()) {
        if (!specs) throw Error("launchIds: pooling needs a sampled forward (specs)");
        if (noRowDraws(n, specs))  // (no row draws: beginProcs found no active row either)
            k = GraphKind::EMBED;
        else  // (a single row takes paths that keep the residual elsewhere: setupPrenorm)
            DL_CHECK(n >= 2, "pooling: a pooled row that draws needs a forward of its own kind with >= 2 rows");
    }
    setInputs(n, tokens, positions, slots, specs, 0, k.has(PROC) ? procRows_.data() : nullptr,
              k.has(FILTER) ? filterRows_.data() : nullptr);
    if (k.has(PROC)) enqueueProcState(n, slots, procs);
    stagePooling(n, slots, pool);
    runGraph(n, specs ? k : GraphKind::ARGMAX);
    if (k.kind == GraphKind::EMBED) {
        logprobReq_.clear();
        DL_HIP(hipMemsetAsync(dIds_, 0xff, n * sizeof(int), stream_));  // no row drew: ids -1
    } else {
        enqueueLogprobs(n, specs, targets);
        if (poolStaged_) {
            enqueuePool(n);
            DL_HIP(hipGetLastError());
        }
    }
    enqueuePoolReadback();
    DL_HIP(hipMemcpyAsync(hIds_, dIds_, n * sizeof(int), hipMemcpyDeviceToHost, stream_));
}

// The all-embedding forward on its own: the root pools (a setPooling precedes it), the other ranks
// run the same layers and skip wcls and the logits exchange with it.
void HipEngineImpl::forwardEmbed(int n, const int *tokens, const int *positions, const int *slots) {
    Timer t;
    DL_CHECK(pendingN_ == 0, "forwardEmbed: the previous forward was not collected");
    const std::vector<PoolSpec> pool = beginPooling(n, positions, slots);
    if (rank() == 0 && pool.empty()) throw Error("forwardEmbed: no row takes part (setPooling)");
    logprobReq_.clear();
    setInputs(n, tokens, positions, slots);
    stagePooling(n, slots, pool);
    runGraph(n, GraphKind::EMBED);
    enqueuePoolReadback();
    syncAndCheckComm();
    inputsInFlight_ = false;
    readLogprobs();
    readPooled();
    stats_.computeMs = t.elapsedMs();
    setSyncStats(readSync(hSync_, false), stats_.computeMs);
}

std::vector<PoolSpec> HipEngineImpl::beginPooling(int n, const int *positions, const int *slots) {
    if (pendingPool_.empty()) return {};
    std::vector<PoolSpec> pool = takePooling(n, positions, slots);
    if (rank() != 0) pool.clear();  // the final residual is replicated: the root pools
    return pool;
}

void HipEngineImpl::stagePooling(int n, const int *slots, const std::vector<PoolSpec> &pool) {
    poolStaged_ = false;
    poolDone_.clear();
    if (pool.empty()) return;
    DL_CHECK(h_.dim % 4 == 0, "pooling needs dim % 4 == 0");
    int *idx = reinterpret_cast<int *>(hPoolRows_ + n);
    for (int b = 0; b < n; b++) {
        const PoolSpec &p = pool[b];
        hipk::PoolRow r{};
        r.slot = slots[b];
        r.flags = !p.active ? 0
                            : hipk::kPoolTake | (p.first ? hipk::kPoolFirst : 0) | (p.last ? hipk::kPoolLast : 0) |
                                  (p.mode == PoolMode::LAST ? hipk::kPoolModeLast : 0);
        r.count = p.count;
        hPoolRows_[b] = r;
        if (p.active && p.last) poolDone_.push_back(slots[b]);
    }
    hipk::poolPlan(hPoolRows_, idx, n);
    DL_HIP(hipMemcpyAsync(dPoolRows_, hPoolRows_, (size_t)n * (sizeof(hipk::PoolRow) + sizeof(int)),
                          hipMemcpyHostToDevice, stream_));
    poolStaged_ = true;
}

// The final residual of a forward of n rows: enqueueForward leaves it in dX_[1] + dY_ (the parity
// after any number of layers), or whole in dX_[0] when the batched GEMMs fuse the residual update.
hipk::PoolArgs HipEngineImpl::poolArgs(int n) const {
    const bool fz = batchedPath(n) && fuseNorm(n);
    hipk::PoolArgs a;
    a.in = fz ? dX_[0] : dX_[1];
    a.add = fz ? nullptr : dY_;
    a.ld = dim();
    a.normW = rmsFinal_;
    a.eps = h_.normEpsilon;
    a.dim = dim();
    a.rows = dPoolRows_;
    a.idx = reinterpret_cast<const int *>(dPoolRows_ + n);
    a.scale = dPoolScale_;
    a.acc = dPoolAcc_;
    a.out = dPoolOut_;
    a.part = dPoolPart_;
    a.counters = dPoolCnt_;
    return a;
}

void HipEngineImpl::enqueuePool(int n) {
    ProfScope ps(this, "pool");
    hipk::launchPool(poolArgs(n), n, stream_);
}

void HipEngineImpl::enqueuePoolReadback() {
    for (size_t k = 0; k < poolDone_.size(); k++)
        DL_HIP(hipMemcpyAsync(hPoolOut_ + k * h_.dim, dPoolOut_ + (size_t)poolDone_[k] * h_.dim, h_.dim * sizeof(float),
                              hipMemcpyDeviceToHost, stream_));
}

void HipEngineImpl::readPooled() {
    pooled_.slots = poolDone_;
    pooled_.values.assign(hPoolOut_ ? hPoolOut_ : nullptr, hPoolOut_ ? hPoolOut_ + poolDone_.size() * h_.dim : nullptr);
    poolDone_.clear();
    poolStaged_ = false;
}

// The logit processors handed over for this forward (Backend::setLogitProcs). Ranks other than the
// root drop them: they neither hold the full logits nor draw, and run their SAMPLE schedule with
// the same collectives in the same order. Returns the sampled forward's draw stages: none without an
// active row, else PROC with procRows_ filled, FILTER with filterRows_ filled too when one of the
// active rows has top_k or min_p on, and JSON / GRAMMAR when one of them is constrained that way.
unsigned HipEngineImpl::beginProcs(int n, const int *slots, const SampleSpec *specs, std::vector<LogitProc> &procs) {
    if (pendingProcs_.empty()) return 0;
    if (!specs) {
        pendingProcs_.clear();
        throw Error("launchIds: logit processors need a sampled forward (specs)");
    }
    procs = takeLogitProcs(n);
    if (procs.empty() || rank() != 0) return 0;
    std::vector<int> seen;
    procRows_.assign((size_t)n * 4, 0.f);
    filterRows_.assign((size_t)n, hipk::LogitFilterRow{0, -INFINITY, 0, 0});
    unsigned stages = 0;
    for (int b = 0; b < n; b++) {
        const LogitProc &p = procs[b];
        if (!p.active || specs[b].temperature < 0.f) continue;
        DL_CHECK(slots[b] >= 0 && (u32)slots[b] < cfg_.nSlots, "slot out of range");
        seen.push_back(slots[b]);
        procRows_[(size_t)b * 4] = p.presence;
        procRows_[(size_t)b * 4 + 1] = p.frequency;
        procRows_[(size_t)b * 4 + 2] = 1.f;
        stages |= PROC;
        if (p.filter(specs[b].temperature, (int)h_.vocabSize)) {
            filterRows_[b] = hipk::LogitFilterRow{p.topK, minPDelta(specs[b].temperature, p.minP), 1, 0};
            stages |= FILTER;
        }
        if (p.json) {
            DL_CHECK(dJsonMeta_ != nullptr, "json mode: no token table (setJsonTable)");
            procRows_[(size_t)b * 4 + 3] = hipk::kRowKindJson;
            stages |= JSON;
        }
        if (p.grammar) {  // (takeLogitProcs: never next to json; a fresh row's tables are checked)
            DL_CHECK(dJsonMeta_ != nullptr, "json_schema: no token table (setJsonTable)");
            DL_CHECK(p.fresh || slotGrammar_[(size_t)slots[b]] == p.grammar,
                     "json_schema: a row that is not fresh carries another grammar than its slot's");
            procRows_[(size_t)b * 4 + 3] = hipk::kRowKindGrammar;
            stages |= GRAMMAR;
        }
    }
    std::sort(seen.begin(), seen.end());
    DL_CHECK(std::adjacent_find(seen.begin(), seen.end()) == seen.end(),
             "logit processors: two drawn rows of one forward share a slot");
    return stages;
}

// Before the forward, in stream order: a fresh slot's counts are zeroed and its bias entries and
// their number uploaded from the pinned staging (free: the previous forward was collected).
void HipEngineImpl::enqueueProcState(int n, const int *slots, const std::vector<LogitProc> &procs) {
    static_assert(sizeof(hipk::LogitBiasEntry) == sizeof(LogitBias) && hipk::kMaxLogitBias == kMaxLogitBias,
                  "device and host bias layouts");
    for (int b = 0; b < n; b++) {
        const LogitProc &p = procs[b];
        if (procRows_[(size_t)b * 4 + 2] == 0.f || !p.fresh) continue;
        const size_t s = (size_t)slots[b], nb = p.bias.size();
        if (p.json) DL_HIP(hipMemsetAsync(dJsonStates_ + s, 0, sizeof(uint4), stream_));  // START is all zero bits
        if (p.grammar) enqueueGrammarInstall(s, p.grammar);
        DL_HIP(hipMemsetAsync(dProcCounts_ + s * h_.vocabSize, 0, (size_t)h_.vocabSize * sizeof(uint32_t), stream_));
        hProcNBias_[s] = (int)nb;
        DL_HIP(hipMemcpyAsync(dProcNBias_ + s, hProcNBias_ + s, sizeof(int), hipMemcpyHostToDevice, stream_));
        if (nb == 0) continue;
        std::memcpy(hProcBias_ + s * kMaxLogitBias, p.bias.data(), nb * sizeof(LogitBias));
        DL_HIP(hipMemcpyAsync(dProcBias_ + s * kMaxLogitBias, hProcBias_ + s * kMaxLogitBias, nb * sizeof(LogitBias),
                              hipMemcpyHostToDevice, stream_));
    }
}

// The token table of JSON mode, uploaded once (root rank: the root draws). The memory check reserved
// an estimate (procBytes); the table's real size is checked against what is free now.
void HipEngineImpl::setJsonTable(std::shared_ptr<const JsonTokenTable> table) {
    Backend::setJsonTable(table);
    if (!table || rank() != 0) return;
    DL_CHECK(pendingN_ == 0 && !dJsonMeta_, "json mode: the token table is set once, with no forward in flight");
    DL_HIP(hipSetDevice(dev_));
    size_t freeB = 0, totalB = 0;
    DL_HIP(hipMemGetInfo(&freeB, &totalB));
    if (table->bytes() + ((size_t)64 << 20) > freeB)
        throw Error("json mode: the token table (" + std::to_string(table->bytes() >> 20) + " MB) does not fit on the GPU (" +
                    std::to_string(freeB >> 20) + " MB free)");
    const size_t V = h_.vocabSize;
    std::vector<uint2> meta(V);
    for (size_t t = 0; t < V; t++) {
        DL_CHECK((size_t)table->off[t] + (jsonTokenLen(table->info[t]) + 3) / 4 <= table->words.size(), "json mode: malformed token table");
        meta[t] = make_uint2(table->off[t], table->info[t]);
    }
    dJsonMeta_ = dalloc<uint2>(V);
    dJsonWords_ = dalloc<uint32_t>(table->words.size());
    DL_HIP(hipMemcpy(dJsonMeta_, meta.data(), V * sizeof(uint2), hipMemcpyHostToDevice));
    DL_HIP(hipMemcpy(dJsonWords_, table->words.data(), table->words.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
}

// A fresh row's grammar goes to its slot's table block, and the slot's state to the start state, in
// stream order ahead of the forward. The copies read the grammar's own arrays (installGrammarTables):
// slotGrammar_ keeps them alive until the slot's next fresh row, whose forward is launched after this
// one was collected.
void HipEngineImpl::enqueueGrammarInstall(size_t slot, const std::shared_ptr<const GrammarDfa> &g) {
    slotGrammar_[slot] = g;
    hipk::installGrammarTables(dGrammarTables_ + slot * hipk::kGrammarSlotBytes, *g, stream_);
    DL_HIP(hipMemcpyAsync(dGrammarStates_ + slot, &g->start, sizeof(uint32_t), hipMemcpyHostToDevice, stream_));
}

hipk::ConstraintArgs HipEngineImpl::constraintArgs() const {
    static_assert(sizeof(JsonState) == sizeof(uint4), "device and host state layouts");
    hipk::ConstraintArgs g;
    g.logits = dProcLogits_;
    g.vocab = h_.vocabSize;
    g.spec = dSpec_;
    g.proc = dProc_;
    g.slots = dSlot_;
    g.table.meta = dJsonMeta_;
    g.table.words = dJsonWords_;
    g.ids = dIds_;
    g.jsonStates = dJsonStates_;
    g.grammarTables = dGrammarTables_;
    g.grammarStates = dGrammarStates_;
    return g;
}

hipk::LogitProcArgs HipEngineImpl::logitProcArgs(const float *raw) const {
    hipk::LogitProcArgs g;
    g.logits = raw;
    g.out = dProcLogits_;
    g.vocab = h_.vocabSize;
    g.spec = dSpec_;
    g.proc = dProc_;
    g.slots = dSlot_;
    g.counts = dProcCounts_;
    g.bias = dProcBias_;
    g.nBias = dProcNBias_;
    g.ids = dIds_;
    return g;
}

// Rows of the SAMPLE forward just enqueued ask for log-probabilities (SampleSpec::logprobs): one
// launchLogprobs behind the graph on the same stream - not inside it, so forwards without a request
// replay exactly the graphs they always did - over the full logits and the ids the sampler wrote,
// and the (1 + 20) pairs per row copied to pinned memory with the ids. Root only: the other ranks
// of a tensor-parallel forward neither hold the full logits nor draw.
void HipEngineImpl::enqueueLogprobs(int n, const SampleSpec *specs, const std::vector<int> &targets) {
    logprobReq_.clear();
    if (!specs || rank() != 0) return;
    bool any = false;
    for (int b = 0; b < n; b++) any = any || specs[b].logprobs >= 1.f;
    if (!any) return;
    logprobReq_.resize(n);
    for (int b = 0; b < n; b++) logprobReq_[b] = (int)specs[b].logprobs;
    hipk::LogprobArgs g;
    g.logits = plan_.nRanks > 1 ? dLogitsFull_ : dLogits_;
    g.vocab = h_.vocabSize;
    g.ids = dIds_;
    g.spec = dSpec_;
    g.scratch = logprobScratch_;
    g.out = dLogprobs_;
    if (!targets.empty()) {  // (the pinned staging is free: the previous forward was collected)
        std::memcpy(hLogprobTargets_, targets.data(), (size_t)n * sizeof(int));
        DL_HIP(hipMemcpyAsync(dLogprobTargets_, hLogprobTargets_, (size_t)n * sizeof(int), hipMemcpyHostToDevice, stream_));
        g.target = dLogprobTargets_;
    }
    hipk::launchLogprobs(g, n, stream_);
    DL_HIP(hipGetLastError());
    DL_HIP(hipMemcpyAsync(hLogprobs_, dLogprobs_, (size_t)n * hipk::kLogprobSlots * sizeof(hipk::LogprobEntry),
                          hipMemcpyDeviceToHost, stream_));
}

// After the forward's stream sync: Backend::lastLogprobs() of the forward (rows without a request,
// which the kernel leaves untouched, hold id -1).
void HipEngineImpl::readLogprobs() {
    static_assert(hipk::kLogprobSlots == kLogprobEntries && sizeof(hipk::LogprobEntry) == sizeof(TokenLogprob),
                  "device and host logprob layouts");
    logprobs_.assign(logprobReq_.size() * kLogprobEntries, TokenLogprob{0.f, -1});
    for (size_t b = 0; b < logprobReq_.size(); b++)
        if (logprobReq_[b] >= 1)
            std::memcpy(&logprobs_[b * kLogprobEntries], hLogprobs_ + b * hipk::kLogprobSlots,
                        kLogprobEntries * sizeof(TokenLogprob));
    logprobReq_.clear();
}

// Chained decode for the CLI: the CHAIN graph (forward -> argmax -> tokens := ids, pos += 1 on
// the device) per step, each followed by the D2H copy of its id into a ring slot and an event. The
// host keeps a step in flight while it decodes and prints the previous one (the reference's loop
// waits for every token before starting the next: dllama.cpp:74-96). Graph / bucket choice
// follow the step's position as in setInputs; error words are checked at every collect.
void HipEngineImpl::chainLaunch(int token, int pos, int slot) {
    DL_CHECK(pendingN_ == 0, "chainLaunch: a launchIds forward was not collected");
    DL_CHECK(chainHead_ - chainTail_ < kChainDepth, "chainLaunch: too many steps in flight");
    DL_CHECK(pos >= 0 && (u32)pos < h_.seqLen, "position out of range");
    if (!hChain_) {
        hChain_ = halloc<int>(kChainDepth);
        for (auto &e : chainEv_) DL_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    if (token >= 0) {
        DL_CHECK(chainHead_ == chainTail_, "chainLaunch: a chain restarted with steps in flight");
        setInputs(1, &token, &pos, &slot, nullptr, 0);
        chainSlot_ = slot;
    } else {  // dTok_ / dPos_ hold the previous step's id and position + 1 (written on the device)
        DL_CHECK(chainHead_ > 0, "chainLaunch: no chain started");
        mapPages(1, &pos, &chainSlot_, 0);
        attnLong_ = !invariant_ && pos >= kAttnMfmaMinPos;
        bucket_ = (int)(&bucketFor(pos) - buckets_.data());
    }
    const int k = (int)(chainHead_ % kChainDepth);
    runGraph(1, GraphKind::CHAIN, hSyncAt(1 + k));  // this step's own copy (steps in flight overlap)
    DL_HIP(hipMemcpyAsync(hChain_ + k, dIds_, sizeof(int), hipMemcpyDeviceToHost, stream_));
    enqueueErrorCopies();
    DL_HIP(hipEventRecord(chainEv_[k], stream_));
    chainHead_++;
}

int HipEngineImpl::chainCollect() {
    DL_CHECK(chainHead_ > chainTail_, "chainCollect: no step in flight");
    const int k = (int)(chainTail_ % kChainDepth);
    DL_HIP(hipEventSynchronize(chainEv_[k]));
    chainTail_++;
    if (chainTail_ == chainHead_) inputsInFlight_ = false;
    checkErrorWords();
    setSyncStats(readSync(hSyncAt(1 + k), false), -1);
    return hChain_[k];
}

double HipEngineImpl::decodeGreedyBatch(int steps, int nSeq, const int *tokens, const int *pos, const int *slots,
                                        int *outTokens) {
    DL_CHECK(nSeq >= 1 && nSeq <= decodeRows_, "nSeq exceeds the engine's decode rows (max_decode)");
    for (int b = 0; b < nSeq; b++) DL_CHECK((u32)(pos[b] + steps) <= h_.seqLen, "decode exceeds seqLen");
    if (!tpTested_) tpFusedSelfTest();
    setInputs(nSeq, tokens, pos, slots, nullptr, steps - 1);
    // the history window the chain writes: rows 0..nSeq, positions [p0, p1) (not the whole
    // maxBatch x seqLen buffer: 16 MB at a 131072-position capacity, set and copied every call)
    int p0 = pos[0], p1 = pos[0] + steps;
    for (int b = 1; b < nSeq; b++) {
        p0 = std::min(p0, pos[b]);
        p1 = std::max(p1, pos[b] + steps);
    }
    const size_t pitch = sizeof(int) * (size_t)h_.seqLen, width = sizeof(int) * (size_t)(p1 - p0);
    DL_HIP(hipMemset2DAsync(dHist_ + p0, pitch, 0xff, width, nSeq, stream_));
    hipEvent_t e0, e1;
    DL_HIP(hipEventCreate(&e0));
    DL_HIP(hipEventCreate(&e1));
    // measured sync of every step: the slots and running totals start at zero, each step's
    // embedding folds the previous step's slots into the totals, one copy after the last step
    if (plan_.nRanks > 1)
        DL_HIP(hipMemsetAsync(dSync_, 0, hipk::syncFoldWords(syncSlots()) * sizeof(unsigned), stream_));
    // the chained graph: forward -> argmax -> (tokens := ids, pos += 1)
    DL_HIP(hipEventRecord(e0, stream_));
    for (int s = 0; s < steps; s++) runGraph(nSeq, GraphKind::CHAIN, s + 1 == steps ? hSync_ : nullptr);
    accountForward(nSeq, GraphKind::CHAIN, steps);
    DL_HIP(hipEventRecord(e1, stream_));
    DL_HIP(hipEventSynchronize(e1));
    float ms = 0;
    DL_HIP(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    syncAndCheckComm();
    inputsInFlight_ = false;
    setSyncStats(readSync(hSync_, true), ms);  // every step's exchanges, measured
    if (outTokens) {
        const int w = p1 - p0;
        std::vector<int> hist((size_t)nSeq * w);
        DL_HIP(hipMemcpy2D(hist.data(), width, dHist_ + p0, pitch, width, nSeq, hipMemcpyDeviceToHost));
        for (int b = 0; b < nSeq; b++)
            for (int s = 0; s < steps; s++) outTokens[b * steps + s] = hist[(size_t)b * w + pos[b] - p0 + s];
    }
    return ms;
}

void HipEngineImpl::profileForward(int n, const int *tokens, const int *positions, const int *slots) {
    const std::map<std::string, double> agg = profileClasses(n, tokens, positions, slots, nullptr, nullptr);
    double total = 0;
    for (auto &kv : agg) total += kv.second;
    std::printf("⏱️  per-kernel-class device time (eager, batch %d):\n", n);
    for (auto &kv : agg) std::printf("   %-14s %8.3f ms (%5.1f%%)\n", kv.first.c_str(), kv.second, 100.0 * kv.second / total);
    std::printf("   %-14s %8.3f ms\n", "total", total);
}

std::map<std::string, double> HipEngineImpl::profileClasses(int n, const int *tokens, const int *positions,
                                                            const int *slots, const SampleSpec *specs,
                                                            const PoolSpec *pool) {
    DL_CHECK(plan_.nRanks == 1, "profileClasses: single-process engines");
    GraphKind kind = GraphKind::LOGITS;
    std::vector<PoolSpec> pl;
    if (specs) {
        kind = GraphKind::SAMPLE;
        if (pool) setPooling(n, pool);
        pl = beginPooling(n, positions, slots);
        if (!pl.empty() && noRowDraws(n, specs)) kind = GraphKind::EMBED;
        DL_CHECK(pl.empty() || kind == GraphKind::EMBED || n >= 2, "pooling: a pooled row that draws needs >= 2 rows");
    }
    setInputs(n, tokens, positions, slots, specs);
    stagePooling(n, slots, pl);
    profile_ = true;
    profTimes_.clear();
    enqueueForward(n, kind);
    if (kind != GraphKind::EMBED && poolStaged_) enqueuePool(n);
    DL_HIP(hipStreamSynchronize(stream_));
    inputsInFlight_ = false;
    profile_ = false;
    poolDone_.clear();
    poolStaged_ = false;
    std::map<std::string, double> agg;
    for (auto &p : profTimes_) {
        float ms = 0;
        DL_HIP(hipEventElapsedTime(&ms, p.second.first, p.second.second));
        agg[p.first] += ms;
        (void)hipEventDestroy(p.second.first);
        (void)hipEventDestroy(p.second.second);
    }
    profTimes_.clear();
    return agg;
}

// Wait for the stream, then turn a tensor-parallel transport failure into an exception (the
// worker loop re-serves, the root reports it) instead of returning results computed from a
// peer's stale data: the xGMI collectives flag a peer that did not arrive within 2 s, RCCL
// reports asynchronous errors (the communicator is then released without waiting).
void HipEngineImpl::syncAndCheckComm() {
    enqueueErrorCopies();
    DL_HIP(hipStreamSynchronize(stream_));
    checkErrorWords();
}

// The device error words (transport timeout, in-launch hand-off timeout) to pinned host words, in
// stream order behind the work they judge.
void HipEngineImpl::enqueueErrorCopies() {
    const int *flag = comm_ ? comm_->deviceErrorFlag() : nullptr;
    if (flag) DL_HIP(hipMemcpyAsync(hErr_, flag, sizeof(int), hipMemcpyDeviceToHost, stream_));
    if (blockOn_) DL_HIP(hipMemcpyAsync(hErr_ + 1, dBlockErr_, sizeof(int), hipMemcpyDeviceToHost, stream_));
}

void HipEngineImpl::checkErrorWords() {
    const int *flag = comm_ ? comm_->deviceErrorFlag() : nullptr;
    if (blockOn_ && hErr_[1] != 0) {  // the kernel with in-launch hand-offs
        const int code = hErr_[1];
        hErr_[1] = 0;
        resetAttnBlockState();
        throw Error("in-launch hand-off wait timed out (code " + std::to_string(code) +
                    ": attention block 2 qkv->attention, 3 attention->wo, 4 qkv phase; not all workgroups "
                    "resident?)");
    }
    if (flag && *hErr_ != 0)
        throw Error(std::string("tensor-parallel collective timed out: a peer rank did not arrive in time (2 s; 20 s for ranks sharing a GPU; ") +
                    (*hErr_ == 1 ? "all-reduce / all-gather" : *hErr_ == 2 ? "low-latency all-reduce" : "fused exchange") +
                    "; worker lost?)");
    if (comm_) {
        const std::string e = comm_->asyncError();
        if (!e.empty()) {
            comm_->shutdownNow();
            throw Error("tensor-parallel transport failed: " + e);
        }
    }
}

// Tensor-parallel data-plane bytes of one forward of n rows on this rank, in the reference's
// accounting (nn-network.cpp:493-508 counts socket payload): every residual update
// sends this rank's partial [n][dim] to each peer and receives each peer's (Q80 blocks of 34 B per
// 32 values with --sync-type q80, the reference's ZQ format, else f32), two per layer; greedy rows
// then trade one (value, index) winner per row (in the fused exchange or one all-gather), host
// logits and sampled rows gather the vocab slices to the root. The transport's own framing (the 8-byte
// {value, epoch} words of the fused exchange) is not payload and not counted.
void HipEngineImpl::accountForward(int n, GraphKind kind, int times) {
    stats_.sentBytes = stats_.recvBytes = 0;
    const ShardPlan &p = plan_;
    if (p.nRanks <= 1) return;
    const u64 peers = p.nRanks - 1;
    const u64 row = syncQ80_ ? (u64)h_.dim / 32 * 34 : (u64)h_.dim * 4;
    u64 sent = 2ull * h_.nLayers * peers * (u64)n * row, recv = sent;
    const u64 slice = (u64)n * p.vocab0 * 4;
    if (kind == GraphKind::ARGMAX || kind == GraphKind::CHAIN) {  // (value, index) winners only
        sent += peers * (u64)n * 8;
        recv += peers * (u64)n * 8;
    } else if (kind == GraphKind::EMBED) {  // nothing but the residual updates crosses the links
    } else if (rank() == 0) {  // LOGITS / SAMPLE: the vocab slices go to the root
        recv += peers * slice;
    } else {
        sent += slice;
    }
    stats_.sentBytes = sent * (u64)times;
    stats_.recvBytes = recv * (u64)times;
}

// Measured sync of a forward (a host copy of its slots, enqueued by runGraph), summed over the
// forward's exchanges and their launches: wait = per exchange launch the longest time a wave of the
// fused exchange waited for peers' words (tpWaitReport); span = the longest exchange tail of a
// workgroup (DL_SYNC_MEASURE=2); a separate collective counts its stamped span (launch gaps
// included) in both. totals: plus the device running totals of every earlier folded forward (a
// whole decode chain). The reference times its sync steps per forward (nn-executor.cpp:150-155,
// printed per token dllama.cpp:57-64).
HipEngineImpl::SyncRead HipEngineImpl::readSync(const unsigned *buf, bool totals) const {
    SyncRead r;
    if (plan_.nRanks <= 1 || !buf) return r;
    const int S = syncSlots();
    const unsigned long long *st = reinterpret_cast<const unsigned long long *>(buf + 2 * S);
    const unsigned long long *acc = reinterpret_cast<const unsigned long long *>(buf + 6 * S);
    double wait = 0, span = 0, stamp = 0;
    for (int i = 0; i < S; i++) {
        wait += buf[i];
        span += buf[S + i];
        if (st[2 * i] && st[2 * i + 1] > st[2 * i]) stamp += (double)(st[2 * i + 1] - st[2 * i]);
    }
    if (totals) {
        wait += (double)acc[0];
        span += (double)acc[1];
        stamp += (double)acc[2];
    }
    r.waitMs = (wait + stamp) * 1e-5;  // s_memrealtime: 100 MHz
    if (syncLevel_ >= 2 || stamp > 0) r.spanMs = (span + stamp) * 1e-5;
    return r;
}

// capMs >= 0: the forward's wall time bounds both (a wait cannot exceed the forward it is part of)
void HipEngineImpl::setSyncStats(const SyncRead &r, double capMs) {
    stats_.syncMs = capMs >= 0 ? std::min(r.waitMs, capMs) : r.waitMs;
    stats_.xchgMs = r.spanMs < 0 ? -1 : (capMs >= 0 ? std::min(r.spanMs, capMs) : r.spanMs);
}

void HipEngineImpl::launchStampAt(unsigned long long *p) { hipk::launchStamp(p, stream_); }

// The first forward of a tensor-parallel engine with the fused exchange runs its self-test on the
// real devices (every rank reaches this point in the same forward: the ranks run forwards in
// lockstep). Pass: rank-order sums of known element-dependent values through both exchange
// regions, no peer timed out, and every rank's verdict exchanged over region 0 sums to the world
// size. Anything else switches the fused exchange off on every rank (the verdict sum is the same
// everywhere), which then runs the separate collectives of the same comm (xGMI all-reduce, itself
// self-tested at start-up, or RCCL). DL_TP_FUSED=fail makes rank 1 report a failure (tests).
void HipEngineImpl::tpFusedSelfTest() {
    tpTested_ = true;
    if (!tpFused_ || comm_->computeOnly()) return;
    const int W = plan_.nRanks, me = rank();
    const char *e = std::getenv("DL_TP_FUSED");
    bool ok = !(e && std::strcmp(e, "fail") == 0 && me == 1);
    const int *errFlag = comm_->deviceErrorFlag();
    auto timedOut = [&]() {
        if (!errFlag) return false;
        int v = 0;
        DL_HIP(hipMemcpy(&v, errFlag, sizeof(int), hipMemcpyDeviceToHost));
        return v != 0;
    };
    // the first pass is also the rendezvous: ranks reach their first forward seconds apart (model
    // load / synthetic init time differs per rank), so the self-test waits up to 60 s for a peer
    // instead of the data plane's 2 s
    auto patient = [](hipk::TpXchg x) {
        x.timeoutTicks = 6000LL * 1000 * 1000;
        return x;
    };
    std::vector<float> got;
    std::string why = ok ? "" : "DL_TP_FUSED=fail";
    for (int r = 0; r < 2; r++) {
        const hipk::TpXchg &x = r == 0 ? tpVec_ : tpArg_;
        // dY_ holds maxBatch x dim floats: a small engine tests fewer elements
        const int n = (int)std::min<long long>(std::min<long long>(4096, x.stride), (long long)cfg_.maxBatch * h_.dim);
        hipk::launchTpSelfTest(patient(x), dY_, n, (float)(me + 1), stream_);
        DL_HIP(hipStreamSynchronize(stream_));
        got.resize(n);
        DL_HIP(hipMemcpy(got.data(), dY_, n * sizeof(float), hipMemcpyDeviceToHost));
        for (int el = 0; el < n && ok; el++) {
            const float want = (float)(W * (W + 1) / 2) + (float)(W * (el & 1023));
            if (got[el] != want) {
                ok = false;
                why = "region " + std::to_string(r) + " element " + std::to_string(el) + ": got " +
                      std::to_string(got[el]) + ", want " + std::to_string(want);
            }
        }
    }
    if (timedOut()) {
        ok = false;
        why += " (a peer wait timed out)";
    }
    comm_->resetError();
    hipk::launchTpSelfTest(patient(tpVec_), dY_, 1, ok ? 1.f : 0.f, stream_);  // the verdicts (+ element 0's 0)
    DL_HIP(hipStreamSynchronize(stream_));
    float all = 0.f;
    DL_HIP(hipMemcpy(&all, dY_, sizeof(float), hipMemcpyDeviceToHost));
    bool allOk = !timedOut() && all == (float)W;
    comm_->resetError();
    // The decision must be the same on every rank: a rank whose verdict wait timed out (a peer
    // more than 60 s late) would switch the fused exchange off while the late peer, seeing every
    // verdict, keeps it, and their next forward would wait on different data planes. So the ranks
    // agree through the separate collectives (self-tested at start-up) on the sum of verdicts.
    float agree = allOk ? 1.f : 0.f;
    DL_HIP(hipMemcpy(dY_, &agree, sizeof(float), hipMemcpyHostToDevice));
    comm_->allReduceSum(dY_, 1, stream_);
    DL_HIP(hipStreamSynchronize(stream_));
    DL_HIP(hipMemcpy(&agree, dY_, sizeof(float), hipMemcpyDeviceToHost));
    if (timedOut()) throw Error("tensor-parallel self-test: a peer never reached the verdict agreement");
    if (agree != (float)W && allOk) why = "a peer's verdict";
    allOk = agree == (float)W;
    if (allOk) return;
    std::fprintf(stderr, "⚠️  rank %d: fused tensor-parallel exchange self-test failed (%s); using the separate "
                 "%s collectives\n", me, ok ? "on a peer" : ("here: " + why).c_str(), comm_->name().c_str());
    tpFused_ = false;
    blockOn_ = false;  // the attention block's wo role was chosen for the fused exchange: decide again
    for (CtxBucket &b : buckets_) b.block = false;
    setupAttnBlock();
    setupPrenorm();
}

void HipEngineImpl::runGraph(int n, FwdKind kind, unsigned *syncDst) {
    if (!tpTested_) tpFusedSelfTest();
    accountForward(n, kind.kind, 1);
    auto copySync = [&]() {  // the forward's measured-sync slots to the host (read after the sync)
        if (plan_.nRanks > 1 && syncDst)
            DL_HIP(hipMemcpyAsync(syncDst, dSync_, hipk::syncFoldWords(syncSlots()) * sizeof(unsigned),
                                  hipMemcpyDeviceToHost, stream_));
    };
    if (!cfg_.useGraphs || graphsBroken_) {
        enqueueForward(n, kind);
        copySync();
        return;
    }
    const GraphKey key = graphKey({.bucket = (unsigned)bucket_, .attnLong = attnLong_, .prefillOk = prefillOk_,
                                   .stages = kind.stages, .kind = kind.kind, .rows = (unsigned)n});
    auto it = graphs_.find(key);
    if (it == graphs_.end()) {
        // capture on the second use of a shape: a one-off row count (the tail chunk of a prompt,
        // a serving batch seen once) runs eagerly instead of paying capture + instantiation
        // (several ms for ~170 kernel nodes) for a graph that would never be replayed
        if (graphSeen_.insert(key).second) {
            enqueueForward(n, kind);
            copySync();
            return;
        }
        hipGraphExec_t ge = captureForward(n, kind);
        if (!ge) {
            // e.g. a collective library build that cannot be stream-captured: stay correct, run eagerly
            graphsBroken_ = true;
            std::fprintf(stderr, "⚠️  hipGraph capture failed; falling back to eager launches\n");
            enqueueForward(n, kind);
            copySync();
            return;
        }
        it = graphs_.emplace(key, ge).first;
    }
    DL_HIP(hipGraphLaunch(it->second, stream_));
    copySync();
}

hipGraphExec_t HipEngineImpl::captureForward(int n, FwdKind kind) {
    hipGraph_t g = nullptr;
    hipGraphExec_t ge = nullptr;
    if (hipStreamBeginCapture(stream_, hipStreamCaptureModeThreadLocal) != hipSuccess) return nullptr;
    bool ok = true;
    try {
        enqueueForward(n, kind);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "capture error: %s\n", e.what());
        ok = false;
    }
    const hipError_t ec = hipStreamEndCapture(stream_, &g);
    if (ec != hipSuccess || !ok || !g) {
        if (g) (void)hipGraphDestroy(g);
        (void)hipGetLastError();
        return nullptr;
    }
    const hipError_t ei = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (ei != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return ge;
}

}  // namespace engine_detail

// (kernels.h; host code, shared with ops.cpp)
void hipk::installGrammarTables(uint8_t *block, const GrammarDfa &g, hipStream_t s) {
    static_assert(kGrammarMaxEntries * sizeof(uint16_t) <= hipk::kGrammarClassOff && kGrammarMaxStates / 8 <= 512, "table block layout");
    static_assert(offsetof(GrammarDfa, nStates) == offsetof(GrammarDfa, nClasses) + sizeof(uint32_t), "the head is (nClasses, nStates)");
    DL_HIP(hipMemcpyAsync(block, g.next.data(), g.next.size() * sizeof(uint16_t), hipMemcpyHostToDevice, s));
    DL_HIP(hipMemcpyAsync(block + hipk::kGrammarClassOff, g.classOf, 256, hipMemcpyHostToDevice, s));
    DL_HIP(hipMemcpyAsync(block + hipk::kGrammarAcceptOff, g.accept.data(), g.accept.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    DL_HIP(hipMemcpyAsync(block + hipk::kGrammarHeadOff, &g.nClasses, 2 * sizeof(uint32_t), hipMemcpyHostToDevice, s));
}

std::unique_ptr<HipEngine> makeHipEngine(const EngineConfig &cfg, DeviceComm *comm) {
    return std::unique_ptr<HipEngine>(new engine_detail::HipEngineImpl(cfg, comm));
}

}  // namespace dl
