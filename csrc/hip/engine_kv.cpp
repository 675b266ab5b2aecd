// Paged KV cache of the HIP engine (engine_impl.h).
#include "engine_impl.h"

namespace dl {
namespace engine_detail {

// ---------------------------------------------------------------- paged KV cache
// With cfg.kvPages > 0 each layer's K / V cache is a pool of kvPages pages of kvPageSize
// positions and a page table maps (slot, pos) to a pool row (kernels.h KvMap): a slot holds only
// the pages its sequence reached, so many slots can share HBM sized for the tokens actually in
// flight instead of nSlots x seqLen. Pages are mapped at setInputs for every position a forward
// (or a decode chain) writes and released when a slot restarts at position 0: the same
// deterministic rule on every tensor-parallel rank, so no page messages are exchanged.
void HipEngineImpl::releaseSlot(int slot) {
    if (!paged() || slot < 0 || (u32)slot >= cfg_.nSlots) return;
    for (int i = 0; i < slotPages_[slot]; i++) {
        int &e = hostTable_[(size_t)slot * pagesPerSlot_ + i];
        freePages_.push_back(e);
        e = -1;
    }
    if (slotPages_[slot]) tableDirty_ = true;  // uploaded with the next forward's mapping
    slotPages_[slot] = 0;
}

void HipEngineImpl::setupPages() {
    if (!paged()) return;
    const u32 P = cfg_.kvPageSize;
    DL_CHECK(P >= 32 && (P & (P - 1)) == 0, "--kv-page-size must be a power of two >= 32");
    pageShift_ = 0;
    while ((1u << pageShift_) < P) pageShift_++;
    pagesPerSlot_ = (int)((h_.seqLen + P - 1) / P);
    const size_t entries = (size_t)cfg_.nSlots * pagesPerSlot_;
    hostTable_.assign(entries, -1);
    slotPages_.assign(cfg_.nSlots, 0);
    for (int pg = (int)cfg_.kvPages - 1; pg >= 0; pg--) freePages_.push_back(pg);
    dKvTable_ = dalloc<int>(entries);
    // unmapped entries read page 0 (valid memory, masked out): never a stray address
    DL_HIP(hipMemsetAsync(dKvTable_, 0, entries * sizeof(int), stream_));
    for (int i = 0; i < 2; i++) hTableStage_[i] = halloc<int>(entries);
}

hipk::KvMap HipEngineImpl::kvMap() const {
    hipk::KvMap m;
    if (paged()) {
        m.table = dKvTable_;
        m.pageShift = pageShift_;
        m.pagesPerSlot = pagesPerSlot_;
    }
    return m;
}

// Map the pages every row's positions [pos, pos + ahead] need; a row at position 0 starts a new
// sequence in its slot and releases the slot's old pages first. Uploads the table if it changed
// (stream-ordered before the forward that reads it).
void HipEngineImpl::mapPages(int n, const int *positions, const int *slots, int ahead) {
    if (!paged()) return;
    bool dirty = tableDirty_;
    tableDirty_ = false;
    auto release = [&](int s) {
        for (int i = 0; i < slotPages_[s]; i++) {
            int &e = hostTable_[(size_t)s * pagesPerSlot_ + i];
            freePages_.push_back(e);
            e = -1;
        }
        if (slotPages_[s]) dirty = true;
        slotPages_[s] = 0;
    };
    for (int b = 0; b < n; b++)
        if (positions[b] == 0) release(slots[b]);
    for (int b = 0; b < n; b++) {
        const int s = slots[b];
        const int need = std::min(pagesPerSlot_, ((positions[b] + ahead) >> pageShift_) + 1);
        while (slotPages_[s] < need) {
            if (freePages_.empty())
                throw Error("KV page pool exhausted: " + std::to_string(cfg_.kvPages) + " pages of " +
                            std::to_string(cfg_.kvPageSize) + " positions are all mapped; raise --kv-pages " +
                            "or lower the concurrent context");
            hostTable_[(size_t)s * pagesPerSlot_ + slotPages_[s]++] = freePages_.back();
            freePages_.pop_back();
            dirty = true;
        }
    }
    if (dirty) uploadTable();
}

// The host table to the device, stream-ordered before whatever reads it next.
void HipEngineImpl::uploadTable() {
    // a pinned copy per upload, alternating: the previous upload may still be reading the other
    int *st = hTableStage_[tableFlip_ ^= 1];
    if (inputsInFlight_) DL_HIP(hipStreamSynchronize(stream_));
    for (size_t i = 0; i < hostTable_.size(); i++) st[i] = hostTable_[i] < 0 ? 0 : hostTable_[i];
    DL_HIP(hipMemcpyAsync(dKvTable_, st, hostTable_.size() * sizeof(int), hipMemcpyHostToDevice, stream_));
}

// ---------------------------------------------------------------- prefix copy between slots
// copyPrefix(src, dst, n): dst's positions [0, n) become a byte copy of src's, for every layer and
// this rank's KV heads (hipk::launchKvCopyPrefix, one launch). Launched eagerly on the engine's
// stream: after the forwards already enqueued, before the next one. Under tensor parallelism every
// rank copies its own shard; slots and pages follow the same deterministic rule on every rank.
// Paged: dst gives its pages back (as a row at position 0 would) and maps ceil(n / pageSize) fresh
// ones; a pool that cannot supply them leaves dst without pages.
void HipEngineImpl::setupKvCopy() {
    std::vector<void *> bases;
    for (const DevLayer &L : layers_) {
        bases.push_back(L.k);
        bases.push_back(L.v);
    }
    dKvBases_ = dalloc<void *>(bases.size());
    DL_HIP(hipMemcpy(dKvBases_, bases.data(), bases.size() * sizeof(void *), hipMemcpyHostToDevice));
}

void HipEngineImpl::copyPrefix(int src, int dst, int n) {
    DL_CHECK(src != dst, "copyPrefix: source and destination slot are the same");
    DL_CHECK(src >= 0 && (u32)src < cfg_.nSlots && dst >= 0 && (u32)dst < cfg_.nSlots, "copyPrefix: slot out of range");
    DL_CHECK(n >= 1 && (u32)n < h_.seqLen, "copyPrefix: prefix length out of range");
    DL_CHECK(pendingN_ == 0, "copyPrefix: a launchIds forward was not collected");
    DL_CHECK(chainInFlight() == 0, "copyPrefix: a chained decode step is still in flight");
    if (paged()) {
        DL_CHECK(n <= slotPages_[src] << pageShift_, "copyPrefix: the source slot never reached that position");
        const int need = (n + (int)cfg_.kvPageSize - 1) >> pageShift_;
        const bool fits = (size_t)need <= freePages_.size() + (size_t)slotPages_[dst];
        releaseSlot(dst);
        if (!fits)
            throw Error("KV page pool exhausted: " + std::to_string(cfg_.kvPages) + " pages of " +
                        std::to_string(cfg_.kvPageSize) + " positions cannot hold a prefix copy of " +
                        std::to_string(n) + " positions; raise --kv-pages or lower the concurrent context");
        while (slotPages_[dst] < need) {
            hostTable_[(size_t)dst * pagesPerSlot_ + slotPages_[dst]++] = freePages_.back();
            freePages_.pop_back();
        }
        tableDirty_ = false;
        uploadTable();
        inputsInFlight_ = true;  // the upload reads pinned staging: the next one waits for it
    }
    hipk::KvCopyArgs a;
    a.bases = dKvBases_;
    a.kvMap = kvMap();
    a.nLayers = (int)h_.nLayers;
    a.nKv = (int)(plan_.kv0 / plan_.headSize);
    a.hs = (int)plan_.headSize;
    a.seqLen = (int)h_.seqLen;
    a.elemBytes = kvBf16_ ? 2 : 4;
    a.srcSlot = src;
    a.dstSlot = dst;
    a.n = n;
    a.chunkPos = hipk::kvCopyChunkPos(a.hs, a.elemBytes, paged() ? pageShift_ : 0);
    hipk::launchKvCopyPrefix(a, stream_);
}

// forkPrefix(src, dsts, m, n): copyPrefix(src, dsts[i], n) for every i, the source read once per
// launch of up to hipk::kMaxForkDst destinations (hipk::launchKvForkPrefix). Paged: every
// destination gives its pages back and maps ceil(n / pageSize) fresh ones; the pool is checked for
// all m before any destination is touched, so a refusal leaves every slot as it was. One table upload,
// then ceil(m / kMaxForkDst) launches.
void HipEngineImpl::forkPrefix(int src, const int *dsts, int m, int n) {
    DL_CHECK(m >= 1 && dsts != nullptr, "forkPrefix: no destination slot");
    DL_CHECK(src >= 0 && (u32)src < cfg_.nSlots, "forkPrefix: slot out of range");
    for (int i = 0; i < m; i++) {
        DL_CHECK(dsts[i] >= 0 && (u32)dsts[i] < cfg_.nSlots, "forkPrefix: slot out of range");
        DL_CHECK(dsts[i] != src, "forkPrefix: source and destination slot are the same");
        for (int j = 0; j < i; j++) DL_CHECK(dsts[i] != dsts[j], "forkPrefix: a destination slot is named twice");
    }
    DL_CHECK(n >= 1 && (u32)n < h_.seqLen, "forkPrefix: prefix length out of range");
    DL_CHECK(pendingN_ == 0, "forkPrefix: a launchIds forward was not collected");
    DL_CHECK(chainInFlight() == 0, "forkPrefix: a chained decode step is still in flight");
    if (paged()) {
        DL_CHECK(n <= slotPages_[src] << pageShift_, "forkPrefix: the source slot never reached that position");
        const int need = (n + (int)cfg_.kvPageSize - 1) >> pageShift_;
        size_t avail = freePages_.size();
        for (int i = 0; i < m; i++) avail += (size_t)slotPages_[dsts[i]];
        if ((size_t)need * (size_t)m > avail)
            throw Error("KV page pool exhausted: " + std::to_string(cfg_.kvPages) + " pages of " +
                        std::to_string(cfg_.kvPageSize) + " positions cannot hold " + std::to_string(m) +
                        " prefix copies of " + std::to_string(n) + " positions; raise --kv-pages or lower the concurrent context");
        for (int i = 0; i < m; i++) releaseSlot(dsts[i]);
        for (int i = 0; i < m; i++) {
            const int dst = dsts[i];
            while (slotPages_[dst] < need) {
                hostTable_[(size_t)dst * pagesPerSlot_ + slotPages_[dst]++] = freePages_.back();
                freePages_.pop_back();
            }
        }
        tableDirty_ = false;
        uploadTable();
        inputsInFlight_ = true;  // the upload reads pinned staging: the next one waits for it
    }
    hipk::KvForkArgs a;
    a.bases = dKvBases_;
    a.kvMap = kvMap();
    a.nLayers = (int)h_.nLayers;
    a.nKv = (int)(plan_.kv0 / plan_.headSize);
    a.hs = (int)plan_.headSize;
    a.seqLen = (int)h_.seqLen;
    a.elemBytes = kvBf16_ ? 2 : 4;
    a.srcSlot = src;
    a.n = n;
    a.chunkPos = hipk::kvCopyChunkPos(a.hs, a.elemBytes, paged() ? pageShift_ : 0);
    for (int i0 = 0; i0 < m; i0 += hipk::kMaxForkDst) {
        a.nDst = std::min(hipk::kMaxForkDst, m - i0);
        for (int d = 0; d < hipk::kMaxForkDst; d++) a.dstSlots[d] = dsts[i0 + (d < a.nDst ? d : 0)];
        hipk::launchKvForkPrefix(a, stream_);
    }
}

}  // namespace engine_detail

int hipMaxForkDst() { return hipk::kMaxForkDst; }

}  // namespace dl
