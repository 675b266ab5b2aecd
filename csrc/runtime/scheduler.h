// Multi-user continuous-batching scheduler (replaces the reference's Request/RequestQueue +
// inference_loop, src/Request.hpp:11-64, src/app.cpp:314-402).
//
// Fixes the reference defects SURVEY §2.9 Q1-Q5: every request owns a KV-cache slot and its own
// positions; prompts are really prefilled (chunked, mixed with other requests' decode rows in the
// same forward); each request has its own sampler/seed/temperature/stop strings and UTF-8 decoder;
// the loop has a lifecycle (stop()) and the API front end is concurrent.
#pragma once

#include <atomic>
#include <condition_variable>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "app.h"

namespace dl {

// An embedding request (POST /v1/embeddings) draws no token: its prompt rows are prefilled like any
// prompt and their final hidden states pooled (Backend PoolSpec: mean over the rows, or the last row).
enum class EmbedMode { OFF, MEAN, LAST };

struct GenParams {
    int maxTokens = 128;      // reference default (Request.hpp:33); <= 0 = until EOS / context end
    float temperature = 0.8f;
    float topp = 0.9f;
    u64 seed = 0;
    std::vector<std::string> stop;  // extra stop strings
    // per-token log-probabilities (log_softmax of the raw logits, whatever temperature / top-p):
    // the generated token's, plus the topLogprobs (0..kMaxTopLogprobs) best tokens of its row
    bool logprobs = false;
    int topLogprobs = 0;
    // logit processors (Backend LogitProc): OpenAI's penalties over the tokens generated so far and a
    // per-token bias, applied before the draw; all three at their defaults: none
    float presencePenalty = 0.f;
    float frequencyPenalty = 0.f;
    std::vector<LogitBias> logitBias;  // distinct token ids, at most kMaxLogitBias
    // candidate filter (logitFilterHost) behind them: the topK best logits (ties kept) and / or the
    // tokens with at least minP times the best token's probability; 0: off (a topK >= the vocabulary
    // size is off too: callers pass 0). A greedy request ignores both: the argmax always survives.
    int topK = 0;
    float minP = 0.f;
    EmbedMode embed = EmbedMode::OFF;
    // JSON mode (response_format json_object): every drawn token keeps the generated text a prefix of
    // a JSON object (jsonMaskHost), between the bias and the candidate filter; greedy requests too
    bool jsonObject = false;
    // structured outputs (response_format json_schema): the compiled schema every drawn token follows
    // (grammarMaskHost), in the JSON mask's place; never set together with jsonObject
    std::shared_ptr<const GrammarDfa> grammar;
    // POST /v1/completions: `echo` returns the prompt with the completion and makes maxTokens == 0
    // legal (the request then draws nothing: it ends with the forward that carries its last prompt
    // row, finish_reason "length"); promptLogprobs (echo && logprobs) scores the prompt too: row i of
    // the prompt scores token i + 1 (Backend::setLogprobTargets), with topLogprobs alternatives
    bool completion = false;  // the request came through /v1/completions (SchedulerStats)
    bool echo = false;
    bool promptLogprobs = false;
    // the request never goes beyond its prompt: an embedding, or an echo with max_tokens 0
    bool drawsNothing() const { return embed != EmbedMode::OFF || (echo && maxTokens == 0); }
    bool penalized() const { return presencePenalty != 0.f || frequencyPenalty != 0.f || !logitBias.empty(); }
    bool logitFilter() const { return temperature != 0.f && (topK > 0 || minP > 0.f); }
    // the request's drawn rows carry a LogitProc
    bool logitProc() const { return penalized() || logitFilter() || jsonObject || grammar != nullptr; }
};

// One generated token's log-probability record (GenParams::logprobs).
struct TokenRecord {
    TokenLogprob chosen;
    std::vector<TokenLogprob> top;  // (logit descending, id ascending)
};

// Wakes a reader that waits on several requests at once (the members of a Scheduler::submitGroup
// group streamed into one response): every emit / finish of a member counts one event.
struct GroupSignal {
    std::mutex mu;
    std::condition_variable cv;
    u64 events = 0;
};

class GenRequest {
  public:
    u64 id = 0;
    std::vector<int> prompt;
    GenParams params;

    // ---- results (guarded by mu) ----
    std::mutex mu;
    std::condition_variable cv;
    std::deque<std::string> deltas;  // streamed text pieces not yet consumed
    std::string text;                // full generated text
    std::string finishReason;        // "stop" | "length" | "error"
    std::string error;
    bool done = false;
    int completionTokens = 0;
    std::vector<TokenRecord> logprobs;  // one per generated token (params.logprobs), the last one included
    // params.promptLogprobs: one per prompt token, appended in position order as the forwards that
    // carry the prompt are collected; entry 0 is empty (chosen.id -1: the first token has no context)
    std::vector<TokenRecord> promptLogprobs;
    int cachedTokens = 0;  // prompt tokens whose KV was reused instead of prefilled (--prefix-cache)
    std::vector<float> embedding;  // params.embed: the pooled, L2-normalised vector [dim]

    // The client went away (e.g. a streaming connection dropped): the scheduler finishes the
    // request at its next step and frees its KV slot instead of generating to max_tokens.
    void cancel() { cancelled.store(true); }
    bool isCancelled() const { return cancelled.load(); }

    // Blocks until finished; returns the full text.
    std::string wait();
    // Pops the next delta (blocking); returns false once the request is done and drained.
    bool nextDelta(std::string &out);
    // The same without blocking: false when no delta is ready; `ended` then says done and drained.
    bool tryNextDelta(std::string &out, bool &ended);
    std::shared_ptr<GroupSignal> signal;  // set for the members of a group of more than one
    // Blocks until every prompt token has its record (params.promptLogprobs) or the request is done.
    void waitPromptLogprobs();

  private:
    friend class Scheduler;
    std::atomic<bool> cancelled{false};
    bool finished = false;  // scheduler thread only: finish() ran (rows still in flight are dropped)
    int slot = -1;
    size_t prefilled = 0;
    std::vector<int> generated;
    std::unique_ptr<Sampler> sampler;
    std::unique_ptr<TokenDecoder> decoder;
    std::unique_ptr<EosDetector> eos;
    void emit(const std::string &d);
    void finish(const std::string &reason);
    void signalGroup();
};

struct SchedulerStats {
    u64 forwards = 0, rows = 0, prefillRows = 0, decodeRows = 0, completed = 0, generatedTokens = 0, cancelled = 0;
    double busyMs = 0;
    int active = 0, queued = 0;
    // --prefix-cache: requests admitted behind a reused prefix, the prompt tokens that saved, the
    // hits that needed a device copy (source slot still active), idle slots evicted for their pages
    u64 prefixHits = 0, prefixTokens = 0, prefixCopies = 0, prefixEvictions = 0;
    u64 logitProcRequests = 0;  // finished requests that used penalties or a logit bias
    u64 logitFilterRequests = 0;  // finished requests with top_k or min_p on
    u64 jsonRequests = 0;         // finished requests in JSON mode
    u64 schemaRequests = 0;       // finished requests constrained by a JSON schema
    u64 embeddingRequests = 0;  // finished embedding requests
    u64 completionRequests = 0;  // finished /v1/completions requests (one per prompt item)
    u64 scoredPromptTokens = 0;  // prompt tokens scored for them (echo with logprobs)
    // parallel sampling (submitGroup): groups of more than one whose followers were forked at least
    // once, the followers that started behind a fork, the prompt tokens those skipped (no prefix-cache
    // hits: the prefix* counters and the followers' cachedTokens do not move)
    u64 forkGroups = 0, forkedRequests = 0, forkTokens = 0;
};

class Scheduler {
  public:
    explicit Scheduler(InferenceSession &sess);
    ~Scheduler();
    std::shared_ptr<GenRequest> submit(std::vector<int> prompt, const GenParams &params);
    // Parallel sampling (the chat API's n): `count` requests over one prompt that share one prefill.
    // Member i is an ordinary GenRequest with seed params.seed + i. Member 0, the leader, goes through
    // the queue like any request; the followers wait in a group record and, once a member's collected
    // prefill has reached L = prompt - 1 (one row runs in every member for its own logits), take free
    // slots behind one Backend::forkPrefix(srcSlot, dsts, L) per admission step, each starting at
    // prefilled = L. Followers that find no slot (or, paged, no pages) wait and fork later from any
    // member still active; when none is left they enter the queue as ordinary requests, as they do
    // at submission when L == 0. A cancelled follower that has not joined is dropped.
    // Fairness: when ready followers and queued requests together want more slots than are free, the
    // free slots are dealt to the two sides one at a time, and the side that was served second at one
    // contended admission is served first at the next, so neither starves the other.
    std::vector<std::shared_ptr<GenRequest>> submitGroup(std::vector<int> prompt, const GenParams &params, int count);
    void stop();
    SchedulerStats stats();

  private:
    // One batched forward in flight (pipelined serving): while the device runs it, the host
    // decodes, EOS-checks and streams the previous forward's tokens.
    struct Pick {
        std::shared_ptr<GenRequest> r;
        int row;      // the request's last batch row in the forward: the row whose id belongs to it
        bool sample;  // that row yields the request's next token
        int prefill;  // prompt tokens consumed by this forward: batch rows [row - prefill + 1, row]
        bool embedDone = false;  // the row is an embedding request's last prompt row
        bool scoreDone = false;  // the row is the last prompt row of an echo request with max_tokens 0
        int start = 0;           // prompt position of the first of the prefill rows
        int firstRow() const { return prefill > 0 ? row - prefill + 1 : row; }
    };
    // the records of the prompt rows of a collected pick, in position order (params.promptLogprobs)
    void appendPromptRecords(const Pick &p, const std::vector<TokenLogprob> &logprobs);
    struct Flight {
        std::vector<Pick> picks;
        int n = 0, nDecode = 0;
        Timer t;
    };
    void loop();
    bool step();  // collect the forward in flight, launch the next, post-process the collected one
    void finishRequest(const std::shared_ptr<GenRequest> &r, const char *reason);
    void failAll(const std::string &what);

    InferenceSession &sess_;
    Tokenizer &tok_;
    std::mutex mu_;
    std::condition_variable cv_;
    std::deque<std::shared_ptr<GenRequest>> queue_;
    std::vector<std::shared_ptr<GenRequest>> active_;
    std::vector<std::shared_ptr<GenRequest>> draining_;  // finished, rows still in the forward in flight
    std::vector<int> freeSlots_;
    // paged KV cache: pages reserved for each slot's request at admission (prompt + max_tokens);
    // returned to the pool through releaseSlot (a RELEASE to every rank) when the slot is freed,
    // see flushReleases; admission needs enough unreserved pages
    int pagesTotal_ = -1, pageSize_ = 0;
    std::vector<int> slotPages_;
    std::vector<int> releasing_;  // freed slots whose pages are not released yet (under mu_)
    void returnSlot(int slot);
    void flushReleases();
    void startRequest(const std::shared_ptr<GenRequest> &r, int slot, size_t prefilled);

    // Prefix reuse (--prefix-cache 1; everything below is unused otherwise). resident_[slot] is the
    // token sequence whose KV an idle slot holds: the tokens fed as inputs of collected forwards,
    // frozen when its request finished (an active slot's record is read off its request). Freed
    // slots stay in freeSlots_ with their record, a last-use stamp and, with a paged cache, the pages
    // the record occupies still accounted in slotPages_ (not released). Admission starts a request
    // behind the longest prefix of its prompt found in any record: in place when that slot is idle,
    // through copyPrefix into the least recently used idle slot when it is active.
    bool prefixOn_ = false;
    size_t prefixMin_ = 32;
    std::vector<std::vector<int>> resident_;
    std::vector<u64> lastUse_;
    std::vector<size_t> slotReach_;  // positions launched into each slot (its mapped pages, paged)
    u64 useStamp_ = 0;
    std::vector<int> residentOf(const GenRequest &r) const;
    // positions a request may reach: one that draws nothing never goes beyond its prompt
    static u64 spanOf(const GenRequest &r, u32 seqLen) {
        if (r.params.drawsNothing()) return r.prompt.size();
        return r.params.maxTokens > 0 ? (u64)r.prompt.size() + (u64)r.params.maxTokens + 1 : seqLen;
    }
    // (a chat prompt leaves room for one generated token; one that draws nothing may fill the context)
    static bool promptTooLong(const GenRequest &r, u32 seqLen) {
        return r.params.drawsNothing() ? r.prompt.size() > seqLen : r.prompt.size() >= seqLen;
    }
    int pagesFor(size_t positions) const { return (int)((positions + pageSize_ - 1) / pageSize_); }
    bool admitWithPrefix();  // one request from the head of the queue; false: nothing admitted

    // Request groups (submitGroup) that still have followers waiting to join.
    struct Group {
        std::vector<std::shared_ptr<GenRequest>> members;  // all of them, the leader first
        std::deque<std::shared_ptr<GenRequest>> waiting;   // followers that have not joined
        bool counted = false;                              // in stats_.forkGroups
    };
    std::vector<std::shared_ptr<Group>> groups_;
    bool forkFirst_ = false;  // the side served first at the next contended admission
    // a member whose slot holds [0, L) of the group's prompt (active, prefill collected up to L)
    GenRequest *forkSource(const Group &g) const;
    int readyFollowers();  // under mu_: drops cancelled followers, dissolves groups without a member left
    void admitFollowers();
    Flight flight_;
    bool inflight_ = false;
    bool stop_ = false;
    u64 nextId_ = 1;
    SchedulerStats stats_;
    std::vector<float> logits_;
    std::thread thread_;
};

}  // namespace dl
