#include "scheduler.h"

#include <algorithm>
#include <cstring>
#include <limits>

namespace dl {

std::string GenRequest::wait() {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return done; });
    return text;
}

bool GenRequest::nextDelta(std::string &out) {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return done || !deltas.empty(); });
    if (!deltas.empty()) {
        out = std::move(deltas.front());
        deltas.pop_front();
        return true;
    }
    return false;
}

bool GenRequest::tryNextDelta(std::string &out, bool &ended) {
    std::lock_guard<std::mutex> lk(mu);
    ended = false;
    if (!deltas.empty()) {
        out = std::move(deltas.front());
        deltas.pop_front();
        return true;
    }
    ended = done;
    return false;
}

void GenRequest::signalGroup() {
    if (!signal) return;
    std::lock_guard<std::mutex> lk(signal->mu);
    signal->events++;
    signal->cv.notify_all();
}

void GenRequest::waitPromptLogprobs() {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return done || promptLogprobs.size() >= prompt.size(); });
}

void GenRequest::emit(const std::string &d) {
    if (d.empty()) return;
    {
        std::lock_guard<std::mutex> lk(mu);
        text += d;
        deltas.push_back(d);
        cv.notify_all();
    }
    signalGroup();
}

void GenRequest::finish(const std::string &reason) {
    {
        std::lock_guard<std::mutex> lk(mu);
        finishReason = reason;
        done = true;
        cv.notify_all();
    }
    signalGroup();
}

Scheduler::Scheduler(InferenceSession &sess) : sess_(sess), tok_(sess.tokenizer()) {
    for (int s = sess.nSlots() - 1; s >= 0; s--) freeSlots_.push_back(s);
    pagesTotal_ = sess.kvPagesFree();
    pageSize_ = sess.kvPageSize();
    slotPages_.assign(sess.nSlots(), 0);
    prefixOn_ = sess.args().prefixCache;
    prefixMin_ = (size_t)std::max(1, sess.args().prefixCacheMin);
    resident_.assign(sess.nSlots(), {});
    lastUse_.assign(sess.nSlots(), 0);
    slotReach_.assign(sess.nSlots(), 0);
    thread_ = std::thread([this] { loop(); });
}

Scheduler::~Scheduler() { stop(); }

void Scheduler::stop() {
    {
        std::lock_guard<std::mutex> lk(mu_);
        if (stop_) return;
        stop_ = true;
    }
    cv_.notify_all();
    if (thread_.joinable()) thread_.join();
    // fail anything still pending
    for (auto &r : queue_) r->finish("error");
    for (auto &r : active_) r->finish("error");
    for (auto &g : groups_)
        for (auto &r : g->waiting) r->finish("error");
}

std::shared_ptr<GenRequest> Scheduler::submit(std::vector<int> prompt, const GenParams &params) {
    auto r = std::make_shared<GenRequest>();
    r->prompt = std::move(prompt);
    r->params = params;
    {
        std::lock_guard<std::mutex> lk(mu_);
        r->id = nextId_++;
        if (stop_) {
            r->error = "scheduler stopped";
            r->finish("error");
            return r;
        }
        queue_.push_back(r);
    }
    cv_.notify_all();
    return r;
}

std::vector<std::shared_ptr<GenRequest>> Scheduler::submitGroup(std::vector<int> prompt, const GenParams &params,
                                                                int count) {
    DL_CHECK(count >= 1, "submitGroup: a group has at least one member");
    std::vector<std::shared_ptr<GenRequest>> members;
    auto signal = count > 1 ? std::make_shared<GroupSignal>() : nullptr;
    for (int i = 0; i < count; i++) {
        auto r = std::make_shared<GenRequest>();
        r->signal = signal;
        r->prompt = prompt;
        r->params = params;
        r->params.seed = params.seed + (u64)i;
        members.push_back(r);
    }
    {
        std::lock_guard<std::mutex> lk(mu_);
        for (auto &r : members) r->id = nextId_++;
        if (stop_) {
            for (auto &r : members) {
                r->error = "scheduler stopped";
                r->finish("error");
            }
            return members;
        }
        queue_.push_back(members[0]);
        // nothing to fork from a one-token prompt, nor for requests that need every prompt row
        // themselves (embeddings, prompt scores: they take no prefix hit either)
        const bool fork = count > 1 && prompt.size() > 1 && params.embed == EmbedMode::OFF && !params.promptLogprobs;
        if (fork) {
            auto g = std::make_shared<Group>();
            g->members = members;
            g->waiting.assign(members.begin() + 1, members.end());
            groups_.push_back(g);
        } else {
            for (int i = 1; i < count; i++) queue_.push_back(members[i]);
        }
    }
    cv_.notify_all();
    return members;
}

SchedulerStats Scheduler::stats() {
    std::lock_guard<std::mutex> lk(mu_);
    SchedulerStats s = stats_;
    s.queued = (int)queue_.size();
    for (auto &g : groups_) s.queued += (int)g->waiting.size();
    return s;
}

void Scheduler::loop() {
    while (true) {
        {
            std::unique_lock<std::mutex> lk(mu_);
            cv_.wait(lk, [&] { return stop_ || !queue_.empty() || !active_.empty() || inflight_ || !groups_.empty(); });
            if (stop_) break;
        }
        try {
            step();
        } catch (const std::exception &e) {
            // a failed forward poisons every in-flight request; the session stays usable
            failAll(e.what());
        }
    }
    if (inflight_) {  // leave no forward running on the backend
        try {
            std::vector<int> ids(flight_.n);
            sess_.collectIds(flight_.n, ids.data());
        } catch (const std::exception &) {
        }
        inflight_ = false;
    }
}

// Under mu_. A request's slot becomes free. With a paged KV cache its pages go back to the pool
// on every rank first: the slot waits in releasing_ until flushReleases() has sent the RELEASE
// (network I/O, never under mu_, so submit() / stats() on the HTTP threads do not stall).
void Scheduler::returnSlot(int slot) {
    if (prefixOn_) {  // idle, not forgotten: the slot keeps its record and the pages that hold it
        lastUse_[slot] = ++useStamp_;
        if (pagesTotal_ >= 0) slotPages_[slot] = pagesFor(slotReach_[slot]);
        freeSlots_.push_back(slot);
        return;
    }
    if (pagesTotal_ >= 0 && slotPages_[slot])
        releasing_.push_back(slot);
    else
        freeSlots_.push_back(slot);
}

// Scheduler thread, without mu_: release the pages of the slots returned since the last call,
// then make the slots admissible again (before the next admission / launch).
void Scheduler::flushReleases() {
    std::vector<int> rel;
    {
        std::lock_guard<std::mutex> lk(mu_);
        rel.swap(releasing_);
    }
    if (rel.empty()) return;
    for (int s : rel) {
        try {
            sess_.releaseSlot(s);
        } catch (const std::exception &) {  // a lost worker surfaces on the next forward
        }
    }
    std::lock_guard<std::mutex> lk(mu_);
    for (int s : rel) {
        slotPages_[s] = 0;
        freeSlots_.push_back(s);
    }
}

void Scheduler::failAll(const std::string &what) {
    // the launched forward (if any) is collected first: it still writes the slots handed back
    // below, and the backend refuses the next launch until it has been collected
    bool hadFlight;
    {
        std::lock_guard<std::mutex> lk(mu_);
        hadFlight = inflight_;
    }
    if (hadFlight) {
        try {
            std::vector<int> ids(flight_.n);
            sess_.collectIds(flight_.n, ids.data());
        } catch (const std::exception &) {
        }
    }
    {
        std::lock_guard<std::mutex> lk(mu_);
        inflight_ = false;
        flight_.picks.clear();
        for (auto &r : active_) {
            r->error = what;
            r->finished = true;
            r->finish("error");
            returnSlot(r->slot);
        }
        for (auto &r : draining_) returnSlot(r->slot);
        active_.clear();
        draining_.clear();
        for (auto &g : groups_)  // followers that waited for a fork from the failed members
            for (auto &r : g->waiting) {
                r->error = what;
                r->finish("error");
            }
        groups_.clear();
        if (prefixOn_) {  // the device state is unknown after a failed forward: forget every record
            for (auto &rec : resident_) rec.clear();
            std::vector<int> keep;
            for (int s : freeSlots_) {
                slotReach_[s] = 0;
                if (pagesTotal_ >= 0 && slotPages_[s])
                    releasing_.push_back(s);
                else
                    keep.push_back(s);
            }
            freeSlots_.swap(keep);
        }
    }
    flushReleases();
}

// Under mu_. Finished requests leave active_; their KV slot is reused only once no forward in
// flight still writes it (rows launched before the host saw the EOS are dropped at collection).
void Scheduler::finishRequest(const std::shared_ptr<GenRequest> &r, const char *reason) {
    r->finished = true;
    r->finish(reason);
    if (prefixOn_) resident_[r->slot] = residentOf(*r);  // frozen here: rows still in flight lie beyond it
    bool inFlight = false;
    if (inflight_)
        for (auto &p : flight_.picks)
            if (p.r == r) inFlight = true;
    if (inFlight)
        draining_.push_back(r);
    else
        returnSlot(r->slot);
    active_.erase(std::remove(active_.begin(), active_.end(), r), active_.end());
}

// Scheduler thread. Row i of the prompt scored token i + 1: the record of position i + 1 comes from
// the pick's batch row of position i; position 0 gets the empty record.
void Scheduler::appendPromptRecords(const Pick &p, const std::vector<TokenLogprob> &logprobs) {
    GenRequest *r = p.r.get();
    const int N = (int)r->prompt.size(), k = r->params.topLogprobs;
    std::vector<TokenRecord> recs;
    if (p.start == 0) recs.push_back(TokenRecord{TokenLogprob{0.f, -1}, {}});
    for (int i = 0; i < p.prefill && p.start + i + 1 < N; i++) {
        const size_t row = (size_t)(p.firstRow() + i);
        TokenRecord rec{TokenLogprob{0.f, -1}, {}};
        if (logprobs.size() >= (row + 1) * kLogprobEntries) {
            const TokenLogprob *e = &logprobs[row * kLogprobEntries];
            rec.chosen = e[0];
            for (int j = 1; j < kLogprobEntries && j <= k && e[j].id >= 0; j++) rec.top.push_back(e[j]);
        }
        recs.push_back(std::move(rec));
    }
    std::lock_guard<std::mutex> rl(r->mu);
    for (auto &rec : recs) r->promptLogprobs.push_back(std::move(rec));
    r->cv.notify_all();
}

// Under mu_. The request takes the slot and starts with its first `prefilled` prompt tokens' KV
// already in place (0 without prefix reuse).
void Scheduler::startRequest(const std::shared_ptr<GenRequest> &r, int slot, size_t prefilled) {
    const int vocab = (int)sess_.header().vocabSize;
    r->slot = slot;
    r->prefilled = prefilled;
    r->sampler.reset(new Sampler(vocab, r->params.temperature, r->params.topp, r->params.seed));
    r->decoder.reset(new TokenDecoder(tok_));
    ChatStops cs(tok_);
    std::vector<std::string> stops = cs.stops;
    size_t maxLen = cs.maxStopLength;
    for (auto &s : r->params.stop)
        if (!s.empty()) {
            stops.push_back(s);
            maxLen = std::max(maxLen, s.size());
        }
    std::vector<int> eosIds = tok_.eosTokenIds();
    while (eosIds.size() < stops.size()) eosIds.push_back(-1);
    r->eos.reset(new EosDetector(eosIds, stops, (int)maxLen, (int)maxLen));
    active_.push_back(r);
}

// The tokens whose KV the request's slot holds: those fed as inputs of forwards already collected
// (the last generated token has not been fed yet; rows in flight are not counted).
std::vector<int> Scheduler::residentOf(const GenRequest &r) const {
    std::vector<int> rec(r.prompt.begin(), r.prompt.begin() + std::min(r.prefilled, r.prompt.size()));
    if (!r.generated.empty()) rec.insert(rec.end(), r.generated.begin(), r.generated.end() - 1);
    return rec;
}

static size_t commonPrefix(const std::vector<int> &a, const std::vector<int> &b, size_t cap) {
    const size_t n = std::min({a.size(), b.size(), cap});
    size_t i = 0;
    while (i < n && a[i] == b[i]) i++;
    return i;
}

// Scheduler thread, between the collection of a forward and the next launch (nothing is in flight).
// Admits the request at the head of the queue behind the longest prefix of its prompt that a slot
// holds (capped at prompt - 1: one row must run to yield logits):
//   the best slot is idle   -> the request takes that slot in place, no device work;
//   the best slot is active -> copyPrefix into the least recently used idle slot;
//   no prefix >= prefixMin_ -> the least recently used idle slot, prefilled from 0.
// Paged cache: an idle slot's pages stay accounted; when the pool lacks unreserved pages for the
// request, idle slots are evicted in LRU order until it fits. Only a request that the active
// requests' reservations alone keep out waits (so an idle slot never blocks an admission). The
// decision is taken under mu_; the device work (releases, the copy) runs after it, without mu_.
bool Scheduler::admitWithPrefix() {
    const u32 seqLen = sess_.header().seqLen;
    std::vector<int> evict;
    int target = -1, src = -1;
    size_t L = 0;
    bool releaseTarget = false;
    {
        std::lock_guard<std::mutex> lk(mu_);
        if (queue_.empty()) return false;
        auto r = queue_.front();
        if (r->isCancelled()) {
            queue_.pop_front();
            r->finish("cancelled");
            stats_.cancelled++;
            return true;
        }
        if (r->prompt.empty() || promptTooLong(*r, seqLen)) {
            queue_.pop_front();
            r->error = r->prompt.empty() ? "empty prompt" : "prompt longer than the context";
            r->finish("error");
            return true;
        }
        if (freeSlots_.empty()) return false;
        // (an embedding request never takes a hit: mean pooling needs every row's hidden state; nor
        //  does one that scores its prompt: every row's logits are needed)
        const size_t cap = r->params.embed != EmbedMode::OFF || r->params.promptLogprobs ? 0 : r->prompt.size() - 1;
        int idleBest = -1, lru = freeSlots_.back();
        size_t idleL = 0, activeL = 0;
        for (auto it = freeSlots_.rbegin(); it != freeSlots_.rend(); ++it) {
            const size_t l = commonPrefix(r->prompt, resident_[*it], cap);
            if (l > idleL) idleL = l, idleBest = *it;
            if (lastUse_[*it] < lastUse_[lru]) lru = *it;
        }
        for (auto &a : active_) {
            const size_t l = commonPrefix(r->prompt, residentOf(*a), cap);
            if (l > activeL) activeL = l, src = a->slot;
        }
        bool inPlace = false;
        if (idleL >= prefixMin_ && idleL >= activeL) {
            inPlace = true;
            target = idleBest;
            L = idleL;
            src = -1;
        } else if (activeL >= prefixMin_) {
            target = lru;
            L = activeL;
        } else {
            target = lru;
            src = -1;
        }
        if (pagesTotal_ >= 0) {
            const int need = pagesFor(std::min<u64>(spanOf(*r, seqLen), seqLen));
            if (need > pagesTotal_) {
                queue_.pop_front();
                r->error = "request needs more KV pages than the pool holds";
                r->finish("error");
                return true;
            }
            int held = 0, idleHeld = 0;
            for (int p : slotPages_) held += p;
            for (int s : freeSlots_) idleHeld += slotPages_[s];
            if (need > pagesTotal_ - (held - idleHeld)) return false;  // wait for pages (as without reuse)
            // pages after admission: an in-place slot keeps what it has mapped; any other target
            // gives its pages back first (copyPrefix does, a plain start is released below)
            auto after = [&]() { return held - slotPages_[target] + (inPlace ? std::max(need, slotPages_[target]) : need); };
            std::vector<int> order(freeSlots_);
            std::sort(order.begin(), order.end(), [&](int a, int b) { return lastUse_[a] < lastUse_[b]; });
            for (int s : order) {
                if (after() <= pagesTotal_) break;
                if (s == target || slotPages_[s] == 0) continue;
                held -= slotPages_[s];
                slotPages_[s] = 0;
                slotReach_[s] = 0;
                resident_[s].clear();
                evict.push_back(s);
                stats_.prefixEvictions++;
            }
            if (after() > pagesTotal_) {  // an in-place slot mapped beyond what the pool can spare: start it over
                inPlace = false;
                L = 0;
                src = -1;
            }
            releaseTarget = !inPlace && src < 0 && slotPages_[target] > 0;
            slotPages_[target] = inPlace ? std::max(need, slotPages_[target]) : need;
        }
        if (!inPlace) slotReach_[target] = L;  // a copy maps the pages of [0, L); a plain start none
        resident_[target].clear();
        queue_.pop_front();
        freeSlots_.erase(std::find(freeSlots_.begin(), freeSlots_.end(), target));
        startRequest(r, target, L);
        r->cachedTokens = (int)L;
        if (L > 0) {
            stats_.prefixHits++;
            stats_.prefixTokens += L;
            if (src >= 0) stats_.prefixCopies++;
        }
    }
    if (releaseTarget) evict.push_back(target);
    for (int s : evict) {
        try {
            sess_.releaseSlot(s);
        } catch (const std::exception &) {  // a lost worker surfaces on the next forward
        }
    }
    if (src >= 0) sess_.copyPrefix(src, target, (int)L);  // a failure fails the step (failAll)
    return true;
}

// ---------------------------------------------------------------- request groups (submitGroup)
GenRequest *Scheduler::forkSource(const Group &g) const {
    for (auto &m : g.members)
        if (m->slot >= 0 && !m->finished && m->prefilled + 1 >= m->prompt.size()) return m.get();
    return nullptr;
}

// Under mu_. The followers that could join now, slots permitting. Cancelled followers are dropped; a
// group whose members have all ended (none active, the leader no longer queued) hands its followers
// to the queue as ordinary requests.
int Scheduler::readyFollowers() {
    int ready = 0;
    for (size_t gi = 0; gi < groups_.size();) {
        Group &g = *groups_[gi];
        for (auto it = g.waiting.begin(); it != g.waiting.end();) {
            if ((*it)->isCancelled()) {
                (*it)->finish("cancelled");
                stats_.cancelled++;
                it = g.waiting.erase(it);
            } else {
                ++it;
            }
        }
        bool alive = false;
        for (auto &m : g.members)
            alive = alive || (m->slot >= 0 ? !m->finished : std::find(queue_.begin(), queue_.end(), m) != queue_.end());
        if (!alive)
            for (auto &r : g.waiting) queue_.push_back(r);
        if (!alive || g.waiting.empty()) {
            groups_.erase(groups_.begin() + gi);
            continue;
        }
        if (forkSource(g)) ready += (int)g.waiting.size();
        gi++;
    }
    return ready;
}

// Scheduler thread, between the collection of a forward and the next launch, after the queue's
// admission. Every waiting follower of a group with a fork source takes an idle slot (the least
// recently used one under --prefix-cache, its record dropped, as a copyPrefix target's is) while
// slots and, paged, unreserved pages last; idle slots are evicted for pages in LRU order as in
// admitWithPrefix. One forkPrefix per group serves all that joined. Decided under mu_, the device
// work runs after it.
void Scheduler::admitFollowers() {
    const u32 seqLen = sess_.header().seqLen;
    struct Fork {
        int src;
        size_t L;
        std::vector<int> dsts;
    };
    std::vector<Fork> forks;
    std::vector<int> evict;
    {
        std::lock_guard<std::mutex> lk(mu_);
        for (auto &gp : groups_) {
            Group &g = *gp;
            const GenRequest *s = forkSource(g);
            if (!s) continue;
            Fork f{s->slot, s->prompt.size() - 1, {}};
            while (!g.waiting.empty() && !freeSlots_.empty()) {
                auto r = g.waiting.front();
                if (r->isCancelled()) {
                    g.waiting.pop_front();
                    r->finish("cancelled");
                    stats_.cancelled++;
                    continue;
                }
                int target = freeSlots_.back();
                if (prefixOn_)
                    for (auto it = freeSlots_.rbegin(); it != freeSlots_.rend(); ++it)
                        if (lastUse_[*it] < lastUse_[target]) target = *it;
                if (pagesTotal_ >= 0) {
                    const int need = pagesFor(std::min<u64>(spanOf(*r, seqLen), seqLen));
                    if (need > pagesTotal_) {
                        g.waiting.pop_front();
                        r->error = "request needs more KV pages than the pool holds";
                        r->finish("error");
                        continue;
                    }
                    int held = 0, idleHeld = 0;
                    for (int p : slotPages_) held += p;
                    for (int fs : freeSlots_) idleHeld += slotPages_[fs];
                    if (need > pagesTotal_ - (held - idleHeld)) break;  // wait for pages
                    // the target gives its pages back first (forkPrefix does)
                    std::vector<int> order(freeSlots_);
                    std::sort(order.begin(), order.end(), [&](int a, int b) { return lastUse_[a] < lastUse_[b]; });
                    for (int e : order) {
                        if (held - slotPages_[target] + need <= pagesTotal_) break;
                        if (e == target || slotPages_[e] == 0) continue;
                        held -= slotPages_[e];
                        slotPages_[e] = 0;
                        slotReach_[e] = 0;
                        resident_[e].clear();
                        evict.push_back(e);
                        stats_.prefixEvictions++;
                    }
                    slotPages_[target] = need;
                }
                slotReach_[target] = f.L;  // the fork maps the pages of [0, L)
                resident_[target].clear();
                g.waiting.pop_front();
                freeSlots_.erase(std::find(freeSlots_.begin(), freeSlots_.end(), target));
                startRequest(r, target, f.L);
                f.dsts.push_back(target);
                stats_.forkedRequests++;
                stats_.forkTokens += f.L;
            }
            if (f.dsts.empty()) continue;
            if (!g.counted) stats_.forkGroups++;
            g.counted = true;
            forks.push_back(std::move(f));
        }
        groups_.erase(std::remove_if(groups_.begin(), groups_.end(), [](const std::shared_ptr<Group> &g) { return g->waiting.empty(); }),
                      groups_.end());
    }
    for (int s : evict) {
        try {
            sess_.releaseSlot(s);
        } catch (const std::exception &) {  // a lost worker surfaces on the next forward
        }
    }
    for (auto &f : forks) sess_.forkPrefix(f.src, f.dsts.data(), (int)f.dsts.size(), (int)f.L);  // a failure fails the step (failAll)
}

bool Scheduler::step() {
    const u32 seqLen = sess_.header().seqLen;

    // 0) collect the forward in flight: token ids and prompt progress only (cheap); the text work
    //    for these tokens runs after the next forward has been launched (step 4)
    std::vector<Pick> done;
    std::vector<int> ids;
    std::vector<TokenLogprob> doneLogprobs;
    int doneRows = 0, doneDecode = 0;
    double doneMs = 0;
    if (inflight_) {
        ids.resize(flight_.n);
        sess_.collectIds(flight_.n, ids.data());
        doneLogprobs = sess_.lastLogprobs();  // (empty unless a row asked; the next launch overwrites them)
        doneMs = flight_.t.elapsedMs();
        doneRows = flight_.n;
        doneDecode = flight_.nDecode;
        for (auto &p : flight_.picks) {
            GenRequest *r = p.r.get();
            if (r->finished) continue;  // finished while its row was in flight: dropped
            if (r->params.promptLogprobs && p.prefill > 0) appendPromptRecords(p, doneLogprobs);
            r->prefilled += p.prefill;
            if (p.sample) r->generated.push_back(ids[p.row]);
        }
        const PooledSlots &pooled = sess_.lastEmbeddings();  // (the next launch overwrites them)
        done.swap(flight_.picks);
        inflight_ = false;
        std::lock_guard<std::mutex> lk(mu_);
        for (auto &r : draining_) returnSlot(r->slot);  // their last rows have completed
        draining_.clear();
        // an embedding request ends with the forward that carried its last prompt row: the vector is
        // stored and its slot goes back to the pool before this step's admission
        for (auto &p : done) {
            if (!p.embedDone || p.r->finished) continue;
            const size_t dim = sess_.header().dim;
            const auto it = std::find(pooled.slots.begin(), pooled.slots.end(), p.r->slot);
            if (it == pooled.slots.end() || pooled.values.size() < pooled.slots.size() * dim) {
                p.r->error = "the backend returned no embedding";
                finishRequest(p.r, "error");
                continue;
            }
            const float *v = &pooled.values[(size_t)(it - pooled.slots.begin()) * dim];
            {
                std::lock_guard<std::mutex> rl(p.r->mu);
                p.r->embedding.assign(v, v + dim);
            }
            stats_.completed++;
            stats_.embeddingRequests++;
            finishRequest(p.r, "stop");
        }
        // so does an echo request with max_tokens 0: its last prompt row asked for nothing
        for (auto &p : done) {
            if (p.r->finished) continue;
            if (p.r->params.promptLogprobs)  // (the last prompt row scores nothing)
                stats_.scoredPromptTokens += (u64)std::max(0, std::min(p.prefill, (int)p.r->prompt.size() - 1 - p.start));
            if (!p.scoreDone) continue;
            stats_.completed++;
            if (p.r->params.completion) stats_.completionRequests++;
            finishRequest(p.r, "length");
        }
    }
    flushReleases();  // slots freed by the previous step's text work and by the collection above

    // 1) admission: one free KV slot per request (and, with a paged KV cache, the pages its prompt +
    //    max_tokens can reach; FIFO: the head waits until enough pages are free); cancelled requests
    //    give their slot back
    //    Followers of request groups join behind it (admitFollowers). When they and the queue together
    //    want more slots than are free, the queue takes its share of them (scheduler.h: dealt one
    //    at a time, the side served second goes first next time) and the followers the rest.
    int queueQuota = std::numeric_limits<int>::max();
    bool anyGroups;
    {
        std::lock_guard<std::mutex> lk(mu_);
        anyGroups = !groups_.empty();
        const int F = anyGroups ? readyFollowers() : 0, Q = (int)queue_.size(), S = (int)freeSlots_.size();
        if (F > 0 && Q > 0 && S > 0 && F + Q > S) {
            const int forkShare = std::min(F, forkFirst_ ? (S + 1) / 2 : S / 2);
            queueQuota = S - forkShare;
            forkFirst_ = !forkFirst_;
        }
    }
    if (prefixOn_)
        for (int k = 0; k < queueQuota && admitWithPrefix(); k++) {
        }
    {
        std::unique_lock<std::mutex> lk(mu_);
        int admitted = 0;
        while (!prefixOn_ && !queue_.empty() && !freeSlots_.empty() && admitted < queueQuota) {
            auto r = queue_.front();
            if (r->isCancelled()) {
                queue_.pop_front();
                r->finish("cancelled");
                stats_.cancelled++;
                continue;
            }
            if (r->prompt.empty() || promptTooLong(*r, seqLen)) {
                queue_.pop_front();
                r->error = r->prompt.empty() ? "empty prompt" : "prompt longer than the context";
                r->finish("error");
                continue;
            }
            const int slot = freeSlots_.back();
            if (pagesTotal_ >= 0) {
                const int need = (int)((std::min<u64>(spanOf(*r, seqLen), seqLen) + pageSize_ - 1) / pageSize_);
                int held = 0;  // pages reserved by the active requests
                for (int p : slotPages_) held += p;
                if (need > pagesTotal_) {
                    queue_.pop_front();
                    r->error = "request needs more KV pages than the pool holds";
                    r->finish("error");
                    continue;
                }
                if (need > pagesTotal_ - held) break;  // wait for pages
                slotPages_[slot] = need;
            }
            queue_.pop_front();
            freeSlots_.pop_back();
            startRequest(r, slot, 0);
            admitted++;
        }
        if (anyGroups) {
            lk.unlock();
            admitFollowers();
            lk.lock();
        }
        // the cancel flag is read ONCE per request (cancel() runs on HTTP threads without mu_)
        std::vector<std::shared_ptr<GenRequest>> cancelled;
        for (auto &r : active_)
            if (r->isCancelled()) cancelled.push_back(r);
        for (auto &r : cancelled) {
            finishRequest(r, "cancelled");
            stats_.cancelled++;
        }
        stats_.active = (int)active_.size();
    }

    // 2) build the next batch: decode rows first (latency), then prefill chunks with the remaining
    //    budget. A decode row is launched before the host has decoded the previous token: a request
    //    whose last token turns out to end it (EOS / stop string) wastes one row, dropped at collection.
    // decode rows first (<= --max-batch), then prompt rows up to the prefill chunk
    const int maxRows = std::max(sess_.maxBatch(), sess_.prefillChunk());
    std::vector<int> tokens, positions, slots;
    Flight next;
    for (auto &rp : active_) {
        GenRequest *r = rp.get();
        if (r->prefilled < r->prompt.size() || r->params.drawsNothing()) continue;
        if ((int)tokens.size() >= sess_.maxBatch()) break;
        const int pos = (int)(r->prompt.size() + r->generated.size()) - 1;
        if ((r->params.maxTokens > 0 && (int)r->generated.size() >= r->params.maxTokens) || (u32)(pos + 1) >= seqLen)
            continue;  // ends at this step's text work (length)
        tokens.push_back(r->generated.back());
        positions.push_back(pos);
        slots.push_back(r->slot);
        next.picks.push_back({rp, (int)tokens.size() - 1, true, 0});
    }
    next.nDecode = (int)tokens.size();
    for (auto &rp : active_) {
        GenRequest *r = rp.get();
        if (r->prefilled >= r->prompt.size()) continue;
        const int budget = maxRows - (int)tokens.size();
        if (budget <= 0) break;
        const int take = (int)std::min<size_t>(budget, r->prompt.size() - r->prefilled);
        for (int i = 0; i < take; i++) {
            tokens.push_back(r->prompt[r->prefilled + i]);
            positions.push_back((int)(r->prefilled + i));
            slots.push_back(r->slot);
        }
        const bool completes = r->prefilled + take == r->prompt.size();
        const bool embed = r->params.embed != EmbedMode::OFF, none = r->params.drawsNothing();  // draws no token
        next.picks.push_back({rp, (int)tokens.size() - 1, completes && !none, take, completes && embed,
                              completes && none && !embed, (int)r->prefilled});
    }
    next.n = (int)tokens.size();

    // 3) launch: device argmax when every sampled row is greedy; otherwise per-row draws on the
    //    backend (the device sampler on GPUs) with each request's own temperature / top-p and the
    //    coin its own seeded generator yields, so only token ids come back
    if (next.n > 0) {
        if (prefixOn_)  // positions each slot's cache (and, paged, its mapped pages) reaches
            for (int i = 0; i < next.n; i++) slotReach_[slots[i]] = std::max<size_t>(slotReach_[slots[i]], (size_t)positions[i] + 1);
        // (a greedy request that wants log-probabilities takes the sampler at temperature 0 - the
        //  same lowest-index argmax - because the argmax paths keep no logits to score; so does one
        //  with penalties or a logit bias, which act between the logits and the draw)
        // (a forward with rows of an embedding request takes the specs too: they say which rows draw,
        //  and a forward in which none does computes no logits at all)
        // (so does one with prompt rows that score their next token: only a sampled forward keeps logits)
        bool allGreedy = true, anyProc = false, anyPool = false, anyTarget = false;
        for (auto &p : next.picks) {
            if (p.r->params.embed != EmbedMode::OFF) allGreedy = false, anyPool = true;
            if (p.r->params.promptLogprobs && p.prefill > 0 && p.start + 1 < (int)p.r->prompt.size()) allGreedy = false, anyTarget = true;
            if (!p.sample) continue;
            if (p.r->params.temperature != 0.0f || p.r->params.logprobs || p.r->params.logitProc()) allGreedy = false;
            anyProc = anyProc || p.r->params.logitProc();
        }
        next.t.reset();
        if (allGreedy) {
            sess_.launchIds(next.n, tokens.data(), positions.data(), slots.data(), nullptr);
        } else {
            std::vector<SampleSpec> specs(next.n);
            for (auto &sp : specs) sp.temperature = -1.f;  // rows that are not sampled
            for (auto &p : next.picks) {
                if (!p.sample) continue;
                SampleSpec &sp = specs[p.row];
                sp.temperature = p.r->params.temperature;
                sp.topp = p.r->params.topp;
                sp.coin = p.r->sampler->drawCoin();
                if (p.r->params.logprobs)
                    sp.logprobs = 1.f + (float)std::min(std::max(p.r->params.topLogprobs, 0), kMaxTopLogprobs);
            }
            if (anyProc) {  // the rows' logit processors; a request's first drawn row resets its slot's state
                std::vector<LogitProc> procs(next.n);
                for (auto &p : next.picks) {
                    const GenParams &gp = p.r->params;
                    if (!p.sample || !gp.logitProc()) continue;
                    LogitProc &lp = procs[p.row];
                    lp.active = true;
                    lp.presence = gp.presencePenalty;
                    lp.frequency = gp.frequencyPenalty;
                    lp.fresh = p.r->generated.empty();
                    if (lp.fresh) lp.bias = gp.logitBias;
                    lp.topK = gp.topK;
                    lp.minP = gp.minP;
                    lp.json = gp.jsonObject;
                    lp.grammar = gp.grammar;
                }
                sess_.setLogitProcs(next.n, procs.data());
            }
            if (anyTarget) {  // prompt row i scores token i + 1, which may lie in the next chunk: the host knows it
                std::vector<int> targets(next.n, -1);
                for (auto &p : next.picks) {
                    const GenParams &gp = p.r->params;
                    if (!gp.promptLogprobs) continue;
                    const int N = (int)p.r->prompt.size();
                    for (int i = 0; i < p.prefill && p.start + i + 1 < N; i++) {
                        targets[p.firstRow() + i] = p.r->prompt[p.start + i + 1];
                        specs[p.firstRow() + i].logprobs = 1.f + (float)std::min(std::max(gp.topLogprobs, 0), kMaxTopLogprobs);
                    }
                }
                sess_.setLogprobTargets(next.n, targets.data());
            }
            if (anyPool) {  // the prompt rows of the embedding requests: their picks' last `prefill` rows
                std::vector<PoolSpec> pool(next.n);
                for (auto &p : next.picks) {
                    const GenParams &gp = p.r->params;
                    if (gp.embed == EmbedMode::OFF) continue;
                    const size_t N = p.r->prompt.size();
                    for (int i = 0; i < p.prefill; i++) {
                        PoolSpec &ps = pool[p.row - p.prefill + 1 + i];
                        const size_t at = p.r->prefilled + i;
                        ps.active = true;
                        ps.first = at == 0;
                        ps.last = at + 1 == N;
                        ps.count = (int)N;
                        ps.mode = gp.embed == EmbedMode::LAST ? PoolMode::LAST : PoolMode::MEAN;
                    }
                }
                sess_.setPooling(next.n, pool.data());
            }
            sess_.launchIds(next.n, tokens.data(), positions.data(), slots.data(), specs.data());
        }
        std::lock_guard<std::mutex> lk(mu_);
        flight_ = std::move(next);
        inflight_ = true;
    }

    // 4) text work of the collected forward (overlaps the forward just launched): decode, detect
    //    stops, stream deltas, finish
    std::lock_guard<std::mutex> lk(mu_);
    if (doneRows > 0) {
        stats_.forwards++;
        stats_.rows += doneRows;
        stats_.decodeRows += doneDecode;
        stats_.prefillRows += doneRows - doneDecode;
        stats_.busyMs += doneMs;
    }
    for (auto &p : done) {
        const std::shared_ptr<GenRequest> &rp = p.r;
        GenRequest *r = rp.get();
        if (!p.sample || r->finished) continue;
        const int token = ids[p.row];
        r->completionTokens = (int)r->generated.size();
        if (r->params.logprobs && doneLogprobs.size() >= (size_t)(p.row + 1) * kLogprobEntries) {
            const TokenLogprob *e = &doneLogprobs[(size_t)p.row * kLogprobEntries];
            TokenRecord rec;
            rec.chosen = e[0];
            for (int i = 1; i < kLogprobEntries && i <= r->params.topLogprobs && e[i].id >= 0; i++) rec.top.push_back(e[i]);
            std::lock_guard<std::mutex> rl(r->mu);
            r->logprobs.push_back(std::move(rec));
        }
        std::string piece, delta;
        const bool has = r->decoder->decode(token, piece);
        const EosResult er = r->eos->append(token, has ? piece.c_str() : nullptr);
        if (er == EosResult::NOT_EOS || er == EosResult::EOS) {
            if (r->eos->getDelta(delta)) r->emit(delta);
            r->eos->reset();
        }
        const int nextPos = (int)(r->prompt.size() + r->generated.size());
        const char *reason = nullptr;
        if (er == EosResult::EOS)
            reason = "stop";
        else if ((r->params.maxTokens > 0 && (int)r->generated.size() >= r->params.maxTokens) || (u32)nextPos >= seqLen)
            reason = "length";
        if (reason) {
            stats_.completed++;
            if (r->params.penalized()) stats_.logitProcRequests++;
            if (r->params.logitFilter()) stats_.logitFilterRequests++;
            if (r->params.jsonObject) stats_.jsonRequests++;
            if (r->params.grammar) stats_.schemaRequests++;
            if (r->params.completion) stats_.completionRequests++;
            stats_.generatedTokens += r->generated.size();
            finishRequest(rp, reason);
        }
    }
    stats_.active = (int)active_.size();
    return next.n > 0 || doneRows > 0;
}

}  // namespace dl
