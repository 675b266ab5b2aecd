// Backend interface shared by the CPU reference backend and the HIP (MI355X) engine.
//
// One Backend instance = one rank's shard of the model. A forward call processes `n` rows;
// every row carries its own token, position and KV slot, so rows of different requests
// (multi-user batching) and rows of one prompt chunk (prefill) can be mixed in one call.
// This replaces the reference's pipes + executor step list (nn-executor.cpp:124-187,
// app.cpp:169-209) with a fixed per-layer schedule.
#pragma once

#include <memory>
#include <string>
#include <vector>

#include "../core/grammar_dfa.h"
#include "../core/json_grammar.h"
#include "../core/model_file.h"
#include "../core/plan.h"

namespace dl {

struct EngineConfig {
    std::string modelPath;          // .m file (ignored when synthetic)
    u32 maxSeqLen = 0;              // clamp of header seqLen (0 = model's)
    u32 maxBatch = 32;              // max rows per forward (reference nBatches, app.cpp:37)
    u32 maxDecode = 0;              // rows of decode-only state (greedy-chain history, fused argmax
                                    // exchange); 0 = maxBatch. The CLI / API set --max-batch here and
                                    // size maxBatch by the (larger) prefill chunk.
    u32 nSlots = 1;                 // independent KV-cache slots (concurrent sequences)
    FloatType bufferType = FloatType::F32;  // activation quantization: Q80 or F32
    FloatType syncType = FloatType::F32;    // CPU tensor-parallel wire format of partial sums:
                                            // F32 (exact, TP=N == TP=1) or Q80 (the reference's
                                            // quantized all-gather, llm.cpp:150, 3.8x fewer bytes)
    int nThreads = 1;               // CPU backend threads
    int gpuIndex = -1;              // HIP device ordinal (-1 = CPU backend)
    bool useGraphs = true;          // capture per-batch-size hipGraphs
    bool kvBf16 = true;             // GPU KV cache dtype (bf16 default, f32 when false)
    u32 kvPages = 0;                // GPU paged KV cache: pool pages per layer (0 = contiguous
                                    // nSlots x seqLen, no page table)
    u32 kvPageSize = 256;           // positions per page (power of two, >= 32)
    bool synthetic = false;         // random-init weights of the header's shape (no file)
    ModelHeader syntheticHeader;    // used when synthetic
    u64 seed = 1234;                // synthetic weight seed
    bool batchInvariant = false;    // GPU: every row takes the same kernels and reduction order
                                    // whatever else shares its forward (reproducible serving: a
                                    // request's tokens do not depend on who else is being served)
};

struct ForwardStats {
    double computeMs = 0;
    double syncMs = 0;
    double xchgMs = -1;  // exchange span (GPU: DL_SYNC_MEASURE=2 or separate collectives; CPU: = syncMs); < 0 unmeasured
    u64 sentBytes = 0;
    u64 recvBytes = 0;
};

// Per-row sampling request (reference Sampler::sample, tokenizer.cpp:416-502): temperature 0 =
// greedy, < 0 = row not sampled (prefill rows), otherwise softmax(logits / temperature) then a
// multinomial draw (topp <= 0 or >= 1) or nucleus (top-p) draw with the given coin in [0, 1).
// logprobs is the row's log-probability request: 0 = none, 1 + k = the drawn token plus the k best
// tokens of the row (0 <= k <= kMaxTopLogprobs); the draw itself ignores it.
struct SampleSpec {
    float temperature = 0.f;
    float topp = 0.f;
    float coin = 0.f;
    float logprobs = 0.f;
};
static_assert(sizeof(SampleSpec) == 16, "SampleSpec is part of the worker protocol");

// Per-token log-probabilities: log_softmax of the row's raw logits (independent of temperature and
// top-p). A row's result is 1 + kMaxTopLogprobs entries: [0] the drawn token (id -1 when the row drew
// none), [1 .. k] the k best tokens ordered by (logit descending, id ascending), the rest id -1.
constexpr int kMaxTopLogprobs = 20;
constexpr int kLogprobEntries = 1 + kMaxTopLogprobs;
struct TokenLogprob {
    float logprob;
    int id;
};
// Host implementation (the CPU path and the reference for the device kernel): out[kLogprobEntries].
void logprobsHost(const float *logits, int vocab, int chosen, int k, TokenLogprob *out);

// Host implementation of one row's draw (the CPU path and the reference for the device sampler).
int sampleHost(float *logits, int vocab, const SampleSpec &s);

// Logit processors of a sampled row (OpenAI's frequency_penalty / presence_penalty / logit_bias),
// applied to the row's logits before the draw; counts[t] is how often the row's sequence has
// generated token t so far (prompt tokens are not counted):
//   x = logits[t];  if counts[t] > 0: x = x - frequency * float(counts[t]);  x = x - presence
//   if t has a bias entry: x = x + its value
// every step one f32 operation rounded to nearest (nothing contracted to an FMA); elements with a
// zero count and no bias are copied bit for bit. Log-probabilities keep scoring the raw logits.
constexpr int kMaxLogitBias = 300;  // OpenAI's limit on logit_bias entries
struct LogitBias {
    int id;
    float value;
};
struct LogitProc {
    bool active = false;     // the row's request uses a processor (a row that does not ignores the rest)
    float presence = 0.f;
    float frequency = 0.f;
    bool fresh = false;      // the row's slot starts a generation: zero its counts, take `bias`
    std::vector<LogitBias> bias;  // read when fresh: distinct ids in [0, vocab), at most kMaxLogitBias
    // candidate filter behind the penalties and the bias (logitFilterHost), re-sent every row like the
    // penalties; acts on rows drawn at a temperature > 0
    int topK = 0;     // 0 or >= vocab: off
    float minP = 0.f;  // 0: off
    bool filter(float temperature, int vocab) const {
        return active && temperature > 0.f && ((topK >= 1 && topK < vocab) || minP > 0.f);
    }
    // JSON mode (jsonMaskHost): the row's draw is confined to the tokens that keep its sequence's
    // generated text a prefix of a JSON object; acts on every drawn row (greedy too), between the
    // bias and the candidate filter. The backend keeps the automaton's state per KV slot: a fresh
    // row restarts it, every drawn token advances it. Needs Backend::setJsonTable.
    bool json = false;
    // Structured outputs (grammarMaskHost): the draw is confined to the tokens that keep the generated
    // text a prefix of a document of the compiled schema; sits where the JSON mask sits and acts on
    // every drawn row. Every row of the request carries the grammar; a fresh row installs it in its
    // KV slot (tables and start state), every drawn token advances the slot's state. Needs
    // Backend::setJsonTable (the token table is shared). Exclusive with `json`.
    std::shared_ptr<const GrammarDfa> grammar;
};
// Host implementation (the CPU path and the reference for the device kernel); out may be logits.
void logitProcHost(const float *logits, int vocab, const u32 *counts, float presence, float frequency,
                   const LogitBias *bias, int nBias, float *out);

// Candidate filter of a sampled row (top_k / min_p), in place on the row's logits after the
// penalties and the bias, ahead of the draw at temperature T > 0:
//   thr_k = the topK-th largest value of x, counted with multiplicity  (1 <= topK < vocab, else -inf)
//   thr_p = max(x) + delta, delta = minPDelta(T, min_p)                (delta == -inf: off)
//   x[t]  = x[t] >= max(thr_k, thr_p) ? x[t] : -inf                    (f32 comparison)
// so ties at the k-th value all survive (top_k keeps at least k tokens), survivors keep their bits and
// the maximum always survives. min_p keeps t iff p[t] >= min_p * p_max under softmax(x / T), which is
// x[t] >= max(x) + T * log(min_p): minPDelta is that one f32 product (-inf for min_p <= 0), the only
// place a logarithm is taken.
float minPDelta(float T, float minP);
void logitFilterHost(float *x, int vocab, int topK, float delta);

// JSON mode (`response_format: json_object`, csrc/core/json_grammar.h). The table holds every
// token's bytes (the vocabulary piece, as the logprobs `bytes` field reports it) zero-padded to
// 4-byte words, its offset in words and its length | class << 16: ids below bosId are regular
// pieces, eosIds are EOS, every other special token is banned. A token is allowed in state s iff
// jsonStepToken does not reject: a regular piece of >= 1 byte whose bytes all step, or an EOS in DONE.
struct JsonTokenTable {
    std::vector<u32> off, info, words;
    int vocab() const { return (int)info.size(); }
    size_t bytes() const { return (off.size() + info.size() + words.size()) * sizeof(u32); }
};
JsonTokenTable makeJsonTokenTable(const std::vector<std::string> &pieces, int bosId, const std::vector<int> &eosIds);
// x[t] = -inf for the tokens that are not allowed in `state`; the others pass bit for bit.
void jsonMaskHost(float *x, int vocab, const JsonTokenTable &table, const JsonState &state);
// The state behind a drawn token; a token that is not allowed (or no token: id outside the table)
// leaves the state as it is.
JsonState jsonAdvanceHost(const JsonTokenTable &table, const JsonState &state, int token);
// Startup check: in every lexer state, with the whitespace run and the depth at their caps and
// under both container kinds, some single-byte regular token must be allowed (in DONE: an EOS must
// exist). Returns the first state without one as text, empty when the vocabulary cannot dead-end.
std::string jsonDeadEnd(const JsonTokenTable &table);

// Structured outputs (`response_format: json_schema`, csrc/core/grammar_dfa.h), over the same token
// table. x[t] = -inf for the tokens that grammarStepToken rejects in `state`; the others pass bit
// for bit. grammarAdvanceHost: the state behind a drawn token; a token that is not allowed, or an id
// outside the table, leaves the state as it is.
void grammarMaskHost(float *x, int vocab, const JsonTokenTable &table, const GrammarDfa &dfa, u32 state);
u32 grammarAdvanceHost(const JsonTokenTable &table, const GrammarDfa &dfa, u32 state, int token);

// Embeddings: the pooled, L2-normalised final hidden state of a request's prompt rows. For a request
// whose prompt is N >= 1 rows at positions 0 .. N - 1, with x[i] row i's final residual:
//   h[i]  = rmsnorm(x[i]) * normW          (the vector the logits matmul consumes for row i: same
//                                           epsilon, same residual, before any Q80 quantisation)
//   mean: p = (h[0] + h[1] + ... + h[N-1]) / N   (f32, added in position order, one add per row per element)
//   last: p = h[N-1]
//   out   = p / sqrt(sum_d p[d]^2)         (f32; all zeros when the sum is 0)
// The rows may arrive over several forwards: a PoolSpec per row of a forward says whether the row
// takes part, whether it is its request's first row (the slot's accumulator restarts) and whether
// it is the last one (the slot is finalised; count is then N).
enum class PoolMode : int { MEAN = 0, LAST = 1 };
struct PoolSpec {
    bool active = false;
    bool first = false;
    bool last = false;
    int count = 0;
    PoolMode mode = PoolMode::MEAN;
};
// Host implementation (the CPU path and the reference for the device kernel), in the two steps a
// request split over forwards takes: poolAddHost adds row x (+ add, may be null) to acc[dim] (first:
// acc restarts; last mode: acc becomes the row's h), poolFinishHost turns acc into out[dim] (out may
// be acc). The two norms' sums of squares are taken in double and rounded once. poolHost is both
// over the N rows x[N][dim] of one request.
void poolAddHost(float *acc, const float *x, const float *add, int dim, const float *normW, float eps, bool first,
                 PoolMode mode);
void poolFinishHost(const float *acc, int dim, int count, PoolMode mode, float *out);
void poolHost(const float *x, const float *add, int n, int dim, const float *normW, float eps, PoolMode mode, float *out);
// Finalised slots of a forward and their vectors [slots.size()][dim], in the order of their last rows.
struct PooledSlots {
    std::vector<int> slots;
    std::vector<float> values;
};

class Backend {
  public:
    virtual ~Backend() = default;
    virtual const ModelHeader &header() const = 0;
    virtual const ShardPlan &plan() const = 0;
    // logits (root only, may be null): [n][vocabSize] full vocabulary.
    virtual void forward(int n, const int *tokens, const int *positions, const int *slots, float *logits) = 0;
    // Greedy decode helper: out[i] = argmax over the full vocabulary (every rank gets it).
    virtual void forwardArgmax(int n, const int *tokens, const int *positions, const int *slots, int *out) = 0;
    // Forward + per-row sampling: out[i] = the sampled token (-1 for rows with temperature < 0).
    // Default: full logits to the root, host draw, ids shared through forwardArgmax's channel.
    virtual void forwardSample(int n, const int *tokens, const int *positions, const int *slots,
                               const SampleSpec *specs, int *out);
    // Pipelined serving (scheduler.cpp): launchIds enqueues a forward whose result is one token id
    // per row (argmax when specs is null, else per-row sampling) and may return before it ran;
    // collectIds waits for it and writes the ids. At most one launch is outstanding. The default
    // runs the forward synchronously inside launchIds (host backends: no overlap).
    virtual void launchIds(int n, const int *tokens, const int *positions, const int *slots, const SampleSpec *specs);
    virtual void collectIds(int *out);
    // Logit processors of the next forwardSample / launchIds (with specs) of n rows, which consumes
    // them: procs[i] belongs to row i and acts when that row is drawn. The backend keeps per KV slot
    // the counts of the tokens drawn by active rows since the slot's last `fresh` row, and the bias
    // that row brought. Root only (the root draws); without a call, forwards run as they always did.
    virtual void setLogitProcs(int n, const LogitProc *procs);
    // The token table of JSON mode (LogitProc::json), once, before the first such row. Root only.
    virtual void setJsonTable(std::shared_ptr<const JsonTokenTable> table);
    // Log-probabilities of the last forwardSample / collectIds: [n][kLogprobEntries] when a row of
    // that forward asked for them (SampleSpec::logprobs; rows that did not hold id -1 throughout),
    // empty otherwise and on ranks other than the root. Valid until the next forward is launched.
    virtual const std::vector<TokenLogprob> &lastLogprobs() const { return logprobs_; }
    // Given tokens to score (prompt log-probabilities) in the next forwardSample / launchIds (with
    // specs) of n rows, which consumes them: targets[i] >= 0 makes row i's entry 0 of lastLogprobs()
    // (log_softmax[targets[i]], targets[i]) instead of the drawn token's; entries 1..k are as ever.
    // Such a row draws nothing (temperature < 0) and asks for log-probabilities (SampleSpec::logprobs
    // = 1 + k), else the forward throws. targets[i] < 0: the row behaves as without a call. Root only
    // (the root scores the gathered logits): workers and the worker protocol take no part.
    virtual void setLogprobTargets(int n, const int *targets);
    // Pooling of the next forwardSample / launchIds (with specs) / forwardEmbed of n rows, which
    // consumes it: pool[i] belongs to row i. Rows of one slot appear in a forward in ascending
    // position. Root only (the final residual is replicated: the root pools); without a call,
    // forwards run as they always did. A forward whose rows all have temperature < 0 and that has a
    // taking-part row computes no logits at all (the GPU engine: its own graph kind, which ends in
    // the pooling kernel instead of wcls, the logits exchange and the token pick); any other keeps
    // its kind and pools behind the token pick.
    virtual void setPooling(int n, const PoolSpec *pool);
    // The all-embedding forward on its own (no row draws, no logits, no ids): what a worker rank
    // runs next to the root's forwardSample / launchIds of such a forward, and a synchronous entry
    // point for the root (which needs a setPooling before it).
    virtual void forwardEmbed(int n, const int *tokens, const int *positions, const int *slots);
    // The slots finalised by the last forwardSample / forwardEmbed / collectIds, on the root only.
    // Valid until the next forward is launched.
    virtual const PooledSlots &lastEmbeddings() const { return pooled_; }
    // Chained greedy decode of one sequence (GPU engines; dllama inference): each step's input
    // token is the previous step's argmax, fed back on the device, so step k + 1 is enqueued
    // before the host has read step k (the host decodes and prints while the device runs).
    // chainLaunch: token >= 0 starts a chain at (token, pos, slot); token < 0 enqueues the next
    // step, at position pos. chainCollect waits for the oldest step in flight and returns its id.
    virtual bool chainSupported() const { return false; }
    virtual void chainLaunch(int token, int pos, int slot);
    virtual int chainCollect();
    virtual int chainInFlight() const { return 0; }
    virtual ForwardStats lastStats() const { return stats_; }
    // Weight residency: time to load (file read + repack + upload, or on-device init), bytes read
    // from the model file by this rank, bytes resident on its device (0 for host backends).
    struct LoadStats {
        double ms = 0;
        u64 fileBytes = 0, deviceBytes = 0;
    };
    virtual LoadStats loadStats() const { return {}; }
    // Paged KV cache (GPU, EngineConfig::kvPages > 0): free pages of the pool and positions per page
    // (the scheduler admits requests by pages); -1 / 0 when the cache is contiguous per slot.
    virtual int kvPagesFree() const { return -1; }
    virtual int kvPageSize() const { return 0; }
    // The sequence in this slot ended: a paged cache returns its pages to the pool (no-op otherwise).
    virtual void releaseSlot(int slot) { (void)slot; }
    // Prefix reuse (scheduler.cpp, --prefix-cache): the KV of positions [0, n) of slot src is copied
    // to slot dst, byte for byte, for every layer and this rank's KV heads; dst's earlier contents
    // are dropped (a paged cache returns dst's pages and maps the ones the copy needs). 1 <= n <
    // seqLen, src != dst, no forward launched and not collected. The copy is ordered after the
    // forwards already issued and before the next one. Default: not supported.
    virtual void copyPrefix(int src, int dst, int n);
    // Parallel sampling (Scheduler::submitGroup): copyPrefix(src, dsts[i], n) for every i < m, ordered
    // like copyPrefix. m >= 1, every dst in range, distinct and != src, 1 <= n < seqLen. Default: a
    // loop over copyPrefix (a backend without it throws); the HIP engine reads the source once per
    // launch and, paged, checks the pool for all m destinations before it touches any.
    virtual void forkPrefix(int src, const int *dsts, int m, int n);
    virtual int kvSlots() const = 0;  // EngineConfig::nSlots
    virtual std::string name() const = 0;

    // Host backends, for the default pooling: the forward with the rows' final residual (before the
    // final norm) copied to hidden[n][dim] (may be null); withLogits false: wcls and the logits gather are
    // skipped on every rank. finalNormWeights: the final norm's weights [dim].
    virtual void forwardHidden(int n, const int *tokens, const int *positions, const int *slots, float *hidden,
                               bool withLogits, float *logits);
    virtual const float *finalNormWeights() const { return nullptr; }

  protected:
    ForwardStats stats_;
    std::vector<int> pendingIds_;  // default launchIds / collectIds
    std::vector<TokenLogprob> logprobs_;
    std::vector<LogitProc> pendingProcs_;  // setLogitProcs, until the next sampled forward takes them
    // takes pendingProcs_ for a forward of n rows (empty: none set); checks sizes, bias ids and counts
    std::vector<LogitProc> takeLogitProcs(int n);
    std::vector<int> pendingTargets_;  // setLogprobTargets, until the next sampled forward takes them
    // takes pendingTargets_ for a forward of n rows (empty: none set, or no row has one); checks the
    // size, the ids and that a target row neither draws nor lacks a request
    std::vector<int> takeLogprobTargets(int n, const SampleSpec *specs);
    // host state of the default forwardSample, per slot (allocated at a slot's first fresh row)
    std::vector<std::vector<u32>> procCounts_;
    std::vector<std::vector<LogitBias>> procBias_;
    std::shared_ptr<const JsonTokenTable> jsonTable_;
    // what confines a slot's draws in the default forwardSample: the JSON automaton's state, or a
    // grammar with its state; a fresh row begins its kind's, each row masks and advances by its kind
    struct ConstraintSlot {
        JsonState json = jsonStart();
        std::shared_ptr<const GrammarDfa> dfa;
        u32 state = 0;
        void begin(const LogitProc &p);
        void mask(float *row, int vocab, const JsonTokenTable &table, bool grammar) const;
        void advance(const JsonTokenTable &table, bool grammar, int id);
    };
    std::vector<ConstraintSlot> constraintSlots_;
    std::vector<PoolSpec> pendingPool_;  // setPooling, until the next forward takes it
    PooledSlots pooled_;
    // takes pendingPool_ for a forward of n rows (empty: none set, or no row takes part); checks the
    // sizes and that each slot's taking-part rows come in ascending position
    std::vector<PoolSpec> takePooling(int n, const int *positions, const int *slots);
    // no row of the forward needs logits: none draws (specs null: every row draws) and none asks for
    // log-probabilities (a prompt row that scores a given token)
    static bool noRowDraws(int n, const SampleSpec *specs);
    std::vector<std::vector<float>> poolAcc_;  // default pooling: per slot
    void poolRowsHost(int n, const int *slots, const std::vector<PoolSpec> &pool, const float *hidden);
};

// Host data plane used by the CPU backend for tensor parallelism.
class HostComm {
  public:
    virtual ~HostComm() = default;
    virtual int rank() const = 0;
    virtual int size() const = 0;
    virtual void allReduceSum(float *data, u64 n) = 0;
    // Reference semantics of SYNC_NODE_SLICES with Q80 buffers (nn-network.cpp:537-569,
    // llm.cpp:212-217): every rank's partial is quantized to Q80 once, every rank receives all
    // ranks' quantized partials and sums them dequantized in rank order (identical on all ranks).
    virtual void allReduceSumQ80(float *data, u64 n) { allReduceSum(data, n); }
    // every rank contributes nLocal floats; root receives size()*nLocal floats in rank order
    virtual void gatherToRoot(const float *local, u64 nLocal, float *out) = 0;
    virtual void stats(u64 &sent, u64 &recv) const {
        sent = 0;
        recv = 0;
    }
};

class LocalComm : public HostComm {
  public:
    int rank() const override { return 0; }
    int size() const override { return 1; }
    void allReduceSum(float *, u64) override {}
    void gatherToRoot(const float *local, u64 nLocal, float *out) override;
};

// `world` ranks of one process (threads) exchanging through shared memory with exactly the TCP
// data plane's arithmetic (f32 sum in rank order; Q80: every partial quantized once, dequantized
// sums in rank order). Used to pin the GPU tensor-parallel paths against the CPU reference in
// tests without sockets.
class ThreadGroupComm : public HostComm {
  public:
    struct Group;
    static std::vector<std::unique_ptr<ThreadGroupComm>> make(int world);
    int rank() const override { return rank_; }
    int size() const override;
    void allReduceSum(float *data, u64 n) override;
    void allReduceSumQ80(float *data, u64 n) override;
    void gatherToRoot(const float *local, u64 nLocal, float *out) override;

  private:
    ThreadGroupComm(std::shared_ptr<Group> g, int rank) : g_(std::move(g)), rank_(rank) {}
    std::shared_ptr<Group> g_;
    int rank_;
    std::vector<float> tmp_;
};

std::unique_ptr<Backend> makeCpuBackend(const EngineConfig &cfg, HostComm *comm);

}  // namespace dl
