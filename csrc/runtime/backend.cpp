// Backend defaults: host-side sampling used by the CPU backend and as the reference for the
// device sampler (csrc/hip/kernels.hip sampleKernel).
#include "backend.h"

#include <algorithm>
#include <cmath>
#include <functional>
#include <numeric>
#include <string>
#include <vector>

#include "../text/tokenizer.h"

namespace dl {

int sampleHost(float *logits, int vocab, const SampleSpec &s) {
    if (s.temperature < 0.f) return -1;
    Sampler smp(vocab, s.temperature, s.topp, 0);
    return smp.sampleWithCoin(logits, s.coin);
}

void logprobsHost(const float *logits, int vocab, int chosen, int k, TokenLogprob *out) {
    // log sum exp in double: the result rounds to f32 once, at the subtraction below
    double mx = -INFINITY, sum = 0.0;
    for (int i = 0; i < vocab; i++) mx = std::max(mx, (double)logits[i]);
    for (int i = 0; i < vocab; i++) sum += std::exp((double)logits[i] - mx);
    const double lse = mx + std::log(sum);
    for (int i = 0; i < kLogprobEntries; i++) out[i] = TokenLogprob{0.f, -1};
    if (chosen >= 0 && chosen < vocab) out[0] = TokenLogprob{(float)((double)logits[chosen] - lse), chosen};
    k = std::min({k, kMaxTopLogprobs, vocab});
    if (k <= 0) return;
    std::vector<int> order(vocab);
    std::iota(order.begin(), order.end(), 0);
    std::partial_sort(order.begin(), order.begin() + k, order.end(), [&](int a, int b) {
        return logits[a] > logits[b] || (logits[a] == logits[b] && a < b);
    });
    for (int i = 0; i < k; i++) out[1 + i] = TokenLogprob{(float)((double)logits[order[i]] - lse), order[i]};
}

// volatile intermediates: every step is rounded to f32 on its own whatever the compiler's
// contraction setting (g++ fuses a * b - c into an FMA by default where the target has one)
void logitProcHost(const float *logits, int vocab, const u32 *counts, float presence, float frequency,
                   const LogitBias *bias, int nBias, float *out) {
    for (int t = 0; t < vocab; t++) {
        float x = logits[t];
        if (counts[t] > 0) {
            volatile float fc = frequency * (float)counts[t];
            volatile float y = x - fc;
            volatile float z = y - presence;
            x = z;
        }
        out[t] = x;
    }
    for (int j = 0; j < nBias; j++) {
        if (bias[j].id < 0 || bias[j].id >= vocab) continue;
        volatile float y = out[bias[j].id] + bias[j].value;
        out[bias[j].id] = y;
    }
}

float minPDelta(float T, float minP) {
    if (!(minP > 0.f)) return -INFINITY;
    volatile float l = std::log(minP);  // (f32 overload; the product is rounded on its own)
    return T * l;
}

void logitFilterHost(float *x, int vocab, int topK, float delta) {
    float thr = -INFINITY;
    if (topK >= 1 && topK < vocab) {
        std::vector<float> v(x, x + vocab);
        std::nth_element(v.begin(), v.begin() + (topK - 1), v.end(), std::greater<float>());
        thr = v[topK - 1];
    }
    if (delta > -INFINITY) {
        volatile float tp = *std::max_element(x, x + vocab) + delta;
        thr = std::max(thr, (float)tp);
    }
    for (int t = 0; t < vocab; t++)
        if (!(x[t] >= thr)) x[t] = -INFINITY;
}

JsonTokenTable makeJsonTokenTable(const std::vector<std::string> &pieces, int bosId, const std::vector<int> &eosIds) {
    JsonTokenTable t;
    const size_t V = pieces.size();
    t.off.resize(V);
    t.info.resize(V);
    for (size_t id = 0; id < V; id++) {
        const std::string &p = pieces[id];
        if (p.size() > 0xffffu) throw Error("json mode: a vocabulary piece is longer than 65535 bytes");
        u32 cls = (int)id < bosId ? JT_REGULAR : JT_BANNED;
        if (std::find(eosIds.begin(), eosIds.end(), (int)id) != eosIds.end()) cls = JT_EOS;
        t.off[id] = (u32)t.words.size();
        t.info[id] = (u32)p.size() | cls << 16;
        for (size_t i = 0; i < p.size(); i += 4) {
            u32 w = 0;
            for (size_t j = i; j < std::min(i + 4, p.size()); j++) w |= (u32)(u8)p[j] << (8 * (j - i));
            t.words.push_back(w);
        }
    }
    t.words.push_back(0);  // (never empty: an all-special vocabulary still uploads)
    return t;
}

void jsonMaskHost(float *x, int vocab, const JsonTokenTable &table, const JsonState &state) {
    if (vocab != table.vocab()) throw Error("json mode: the token table is not the model's vocabulary");
    for (int t = 0; t < vocab; t++)
        if (jsonRejected(jsonStepToken(state, table.words.data(), table.off[t], table.info[t]))) x[t] = -INFINITY;
}

JsonState jsonAdvanceHost(const JsonTokenTable &table, const JsonState &state, int token) {
    if (token < 0 || token >= table.vocab()) return state;
    const JsonState next = jsonStepToken(state, table.words.data(), table.off[token], table.info[token]);
    return jsonRejected(next) ? state : next;
}

void grammarMaskHost(float *x, int vocab, const JsonTokenTable &table, const GrammarDfa &dfa, u32 state) {
    if (vocab != table.vocab()) throw Error("json_schema: the token table is not the model's vocabulary");
    const GrammarView v = dfa.view();
    for (int t = 0; t < vocab; t++)
        if (grammarStepToken(v, state, table.words.data(), table.off[t], table.info[t]) == kGrammarReject) x[t] = -INFINITY;
}

u32 grammarAdvanceHost(const JsonTokenTable &table, const GrammarDfa &dfa, u32 state, int token) {
    if (token < 0 || token >= table.vocab()) return state;
    const u32 next = grammarStepToken(dfa.view(), state, table.words.data(), table.off[token], table.info[token]);
    return next == kGrammarReject ? state : next;
}

std::string jsonDeadEnd(const JsonTokenTable &table) {
    bool eos = false;
    std::vector<u8> single;  // the bytes that some regular one-byte piece spells
    for (int t = 0; t < table.vocab(); t++) {
        if (jsonTokenClass(table.info[t]) == JT_EOS) eos = true;
        if (jsonTokenClass(table.info[t]) == JT_REGULAR && jsonTokenLen(table.info[t]) == 1)
            single.push_back((u8)(table.words[table.off[t]] & 0xffu));
    }
    if (!eos) return "the vocabulary has no EOS token to end a finished object with";
    for (int lex = 0; lex < JL_DONE; lex++) {
        std::vector<u8> auxes = {0};
        if (lex == JL_KEY_HEX || lex == JL_STR_HEX) auxes = {1, 2, 3, 4};
        if (lex == JL_KEY_UTF8 || lex == JL_STR_UTF8) auxes = {1, 2, 3, 2 | 1 << 2, 2 | 2 << 2, 3 | 3 << 2, 3 | 4 << 2};
        if (lex == JL_LIT) auxes = {1, 2, 3, 1 << 4 | 1, 1 << 4 | 2, 1 << 4 | 3, 1 << 4 | 4, 2 << 4 | 1, 2 << 4 | 2, 2 << 4 | 3};
        for (u8 aux : auxes)
            for (int obj = 0; obj < 2; obj++) {
                JsonState s = jsonStart();
                s.lex = (u8)lex;
                s.aux = aux;
                if (lex != JL_START) {
                    const bool between = lex <= JL_KEY_NEXT || (lex >= JL_COLON && lex <= JL_ARR_OPEN) || lex == JL_AFTER;
                    s.ws = between ? kJsonMaxWs : 0;
                    s.depth = kJsonMaxDepth;
                    s.stack = obj ? ~0ull : ~0ull >> 1;
                } else {
                    s.ws = kJsonMaxWs;
                }
                // (a state's kind of innermost container is fixed where it opens or names one)
                if ((lex == JL_OBJ_OPEN || lex == JL_KEY_NEXT || (lex >= JL_KEY && lex <= JL_COLON)) && !obj) continue;
                if (lex == JL_ARR_OPEN && obj) continue;
                bool ok = false;
                for (u8 c : single) ok = ok || !jsonRejected(jsonStep(s, c));
                if (!ok)
                    return "no single-byte token continues lexer state " + std::to_string(lex) + " (aux " +
                           std::to_string((int)aux) + ", inside an " + (obj ? "object" : "array") + ")";
            }
    }
    return "";
}

void poolAddHost(float *acc, const float *x, const float *add, int dim, const float *normW, float eps, bool first,
                 PoolMode mode) {
    if (mode == PoolMode::LAST) first = true;
    double ss = 0.0;
    for (int d = 0; d < dim; d++) {
        const float xs = add ? x[d] + add[d] : x[d];
        ss += (double)xs * (double)xs;
    }
    const float inv = (float)(1.0 / std::sqrt(ss / (double)dim + (double)eps));
    for (int d = 0; d < dim; d++) {
        const float xs = add ? x[d] + add[d] : x[d];
        volatile float t = inv * xs;  // (volatile: every step rounded on its own, nothing fused)
        volatile float h = normW[d] * t;
        volatile float sum = first ? h : acc[d] + h;
        acc[d] = sum;
    }
}

void poolFinishHost(const float *acc, int dim, int count, PoolMode mode, float *out) {
    double ss = 0.0;
    for (int d = 0; d < dim; d++) {
        volatile float p = mode == PoolMode::MEAN ? acc[d] / (float)count : acc[d];
        out[d] = p;
        ss += (double)p * (double)p;
    }
    const float nrm = (float)std::sqrt(ss);
    for (int d = 0; d < dim; d++) out[d] = ss > 0.0 ? out[d] / nrm : 0.f;
}

void poolHost(const float *x, const float *add, int n, int dim, const float *normW, float eps, PoolMode mode, float *out) {
    std::vector<float> acc(dim, 0.f);
    for (int i = 0; i < n; i++)
        if (mode == PoolMode::MEAN || i == n - 1)
            poolAddHost(acc.data(), x + (size_t)i * dim, add ? add + (size_t)i * dim : nullptr, dim, normW, eps, i == 0, mode);
    poolFinishHost(acc.data(), dim, n, mode, out);
}

void Backend::setPooling(int n, const PoolSpec *pool) { pendingPool_.assign(pool, pool + n); }

std::vector<PoolSpec> Backend::takePooling(int n, const int *positions, const int *slots) {
    std::vector<PoolSpec> pool;
    pool.swap(pendingPool_);
    if (pool.empty()) return pool;
    if ((int)pool.size() != n) throw Error("setPooling: one spec per row of the forward");
    bool any = false;
    std::vector<std::pair<int, int>> seen;  // (slot, its latest position) of the taking-part rows
    for (int i = 0; i < n; i++) {
        if (!pool[i].active) continue;
        any = true;
        if (pool[i].last && pool[i].count < 1) throw Error("setPooling: the last row carries the request's row count");
        auto it = std::find_if(seen.begin(), seen.end(), [&](const std::pair<int, int> &e) { return e.first == slots[i]; });
        if (it == seen.end())
            seen.push_back({slots[i], positions[i]});
        else if (positions[i] <= it->second)
            throw Error("setPooling: the rows of a slot come in ascending position");
        else
            it->second = positions[i];
    }
    if (!any) pool.clear();
    return pool;
}

bool Backend::noRowDraws(int n, const SampleSpec *specs) {
    if (!specs) return false;
    for (int i = 0; i < n; i++)
        if (specs[i].temperature >= 0.f || specs[i].logprobs >= 1.f) return false;
    return true;
}

void Backend::forwardHidden(int, const int *, const int *, const int *, float *, bool, float *) {
    throw Error(name() + " backend: no host pooling");
}

// Default pooling (host backends): the rows' final residuals through poolAddHost / poolFinishHost.
void Backend::poolRowsHost(int n, const int *slots, const std::vector<PoolSpec> &pool, const float *hidden) {
    const int dim = (int)header().dim;
    const float *w = finalNormWeights();
    if (!w) throw Error(name() + " backend: no host pooling");
    for (int i = 0; i < n; i++) {
        if (!pool[i].active) continue;
        const size_t s = (size_t)slots[i];
        if (poolAcc_.size() <= s) poolAcc_.resize(s + 1);
        if (poolAcc_[s].empty()) poolAcc_[s].assign(dim, 0.f);
        if (pool[i].mode == PoolMode::MEAN || pool[i].last)
            poolAddHost(poolAcc_[s].data(), hidden + (size_t)i * dim, nullptr, dim, w, header().normEpsilon, pool[i].first,
                        pool[i].mode);
        if (!pool[i].last) continue;
        pooled_.slots.push_back(slots[i]);
        pooled_.values.resize(pooled_.slots.size() * dim);
        poolFinishHost(poolAcc_[s].data(), dim, pool[i].count, pool[i].mode, &pooled_.values[(pooled_.slots.size() - 1) * dim]);
    }
}

void Backend::forwardEmbed(int n, const int *tokens, const int *positions, const int *slots) {
    const std::vector<PoolSpec> pool = takePooling(n, positions, slots);
    pooled_ = PooledSlots{};
    logprobs_.clear();
    if (plan().rank != 0) {
        forwardHidden(n, tokens, positions, slots, nullptr, false, nullptr);
        return;
    }
    if (pool.empty()) throw Error("forwardEmbed: no row takes part (setPooling)");
    std::vector<float> hidden((size_t)n * header().dim);
    forwardHidden(n, tokens, positions, slots, hidden.data(), false, nullptr);
    poolRowsHost(n, slots, pool, hidden.data());
}

void Backend::setLogitProcs(int n, const LogitProc *procs) { pendingProcs_.assign(procs, procs + n); }

void Backend::setLogprobTargets(int n, const int *targets) { pendingTargets_.assign(targets, targets + n); }

std::vector<int> Backend::takeLogprobTargets(int n, const SampleSpec *specs) {
    std::vector<int> targets;
    targets.swap(pendingTargets_);
    if (targets.empty()) return targets;
    auto fail = [&](const char *what) {  // the forward does not run: what was handed over for it goes with it
        pendingProcs_.clear();
        pendingPool_.clear();
        throw Error(std::string("setLogprobTargets: ") + what);
    };
    if (!specs) fail("targets need a sampled forward (specs)");
    if ((int)targets.size() != n) fail("one target per row of the forward");
    const int vocab = (int)header().vocabSize;
    bool any = false;
    for (int i = 0; i < n; i++) {
        if (targets[i] < 0) continue;
        any = true;
        if (targets[i] >= vocab) fail("token id out of range");
        if (specs[i].temperature >= 0.f) fail("a row with a target draws no token (temperature < 0)");
        if (!(specs[i].logprobs >= 1.f)) fail("a row with a target asks for log-probabilities (SampleSpec::logprobs)");
    }
    if (!any) targets.clear();  // no row has one: the forward is the plain one
    return targets;
}

void Backend::setJsonTable(std::shared_ptr<const JsonTokenTable> table) {
    if (table && table->vocab() != (int)header().vocabSize) throw Error("json mode: the token table is not the model's vocabulary");
    jsonTable_ = std::move(table);
}

std::vector<LogitProc> Backend::takeLogitProcs(int n) {
    std::vector<LogitProc> procs;
    procs.swap(pendingProcs_);
    if (procs.empty()) return procs;
    if ((int)procs.size() != n) throw Error("setLogitProcs: one processor per row of the forward");
    const int vocab = (int)header().vocabSize;
    bool any = false;
    for (const LogitProc &p : procs) {
        if (!p.active) continue;
        any = true;
        if (p.topK < 0) throw Error("top_k: a count >= 0");
        if (!(p.minP >= 0.f && p.minP <= 1.f)) throw Error("min_p: a number from 0 to 1");
        if ((p.json || p.grammar) && plan().rank == 0 && !jsonTable_)
            throw Error(std::string(p.json ? "json mode" : "json_schema") + ": no token table (setJsonTable)");
        if (p.grammar) {
            if (p.json) throw Error("logit processors: a row is either in JSON mode or follows a grammar, not both");
            if (p.fresh) {  // (the slot keeps the grammar its fresh row brought: checked once)
                const std::string bad = grammarCheck(*p.grammar);
                if (!bad.empty()) throw Error("json_schema: malformed grammar tables: " + bad);
            }
        }
        if (!p.fresh) continue;
        if (p.bias.size() > (size_t)kMaxLogitBias) throw Error("logit_bias: at most 300 entries");
        std::vector<int> seen;
        for (const LogitBias &e : p.bias) {
            if (e.id < 0 || e.id >= vocab) throw Error("logit_bias: token id out of range");
            seen.push_back(e.id);
        }
        std::sort(seen.begin(), seen.end());
        if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) throw Error("logit_bias: duplicate token id");
    }
    if (!any) procs.clear();  // no active row: the forward is the plain one
    return procs;
}

// (a request is of one kind throughout: a fresh row begins its own kind's state and leaves the other,
//  and every row masks and advances by its own kind)
void Backend::ConstraintSlot::begin(const LogitProc &p) {
    if (p.grammar) {
        dfa = p.grammar;
        state = dfa->start;
    } else {
        json = jsonStart();
    }
}

void Backend::ConstraintSlot::mask(float *row, int vocab, const JsonTokenTable &table, bool grammar) const {
    if (grammar)
        grammarMaskHost(row, vocab, table, *dfa, state);
    else
        jsonMaskHost(row, vocab, table, json);
}

void Backend::ConstraintSlot::advance(const JsonTokenTable &table, bool grammar, int id) {
    if (grammar)
        state = grammarAdvanceHost(table, *dfa, state, id);
    else
        json = jsonAdvanceHost(table, json, id);
}

void Backend::forwardSample(int n, const int *tokens, const int *positions, const int *slots, const SampleSpec *specs,
                            int *out) {
    const int vocab = (int)header().vocabSize;
    const std::vector<int> targets = takeLogprobTargets(n, specs);
    const std::vector<LogitProc> procs = takeLogitProcs(n);
    if (plan().rank != 0) {  // workers take part in the forward; the root draws
        pendingPool_.clear();
        pooled_ = PooledSlots{};
        forward(n, tokens, positions, slots, nullptr);
        for (int i = 0; i < n; i++) out[i] = -1;
        logprobs_.clear();
        return;
    }
    if (!pendingPool_.empty() && noRowDraws(n, specs)) {  // an all-embedding forward: no logits at all
        forwardEmbed(n, tokens, positions, slots);
        for (int i = 0; i < n; i++) out[i] = -1;
        return;
    }
    const std::vector<PoolSpec> pool = takePooling(n, positions, slots);
    pooled_ = PooledSlots{};
    std::vector<float> logits((size_t)n * vocab);
    if (pool.empty()) {
        forward(n, tokens, positions, slots, logits.data());
    } else {  // a mixed forward: the logits as ever, the taking-part rows pooled behind them
        std::vector<float> hidden((size_t)n * header().dim);
        forwardHidden(n, tokens, positions, slots, hidden.data(), true, logits.data());
        poolRowsHost(n, slots, pool, hidden.data());
    }
    bool anyLogprobs = false;
    for (int i = 0; i < n; i++) anyLogprobs = anyLogprobs || specs[i].logprobs >= 1.f;
    logprobs_.assign(anyLogprobs ? (size_t)n * kLogprobEntries : 0, TokenLogprob{0.f, -1});
    std::vector<float> raw;
    for (int i = 0; i < n; i++) {
        float *row = &logits[(size_t)i * vocab];
        const int req = (int)specs[i].logprobs;
        if (req >= 1) raw.assign(row, row + vocab);  // the draw rewrites the row in place
        const bool proc = !procs.empty() && procs[i].active && specs[i].temperature >= 0.f;
        if (proc) {  // penalties and bias ahead of the draw; the log-probabilities score the raw row
            const LogitProc &p = procs[i];
            const size_t s = (size_t)slots[i];
            if (procCounts_.size() <= s) {
                procCounts_.resize(s + 1);
                procBias_.resize(s + 1);
            }
            if (p.fresh || procCounts_[s].empty()) procCounts_[s].assign(vocab, 0);
            if (p.fresh) procBias_[s] = p.bias;
            logitProcHost(row, vocab, procCounts_[s].data(), p.presence, p.frequency, procBias_[s].data(),
                          (int)procBias_[s].size(), row);
            if (p.json || p.grammar) {  // behind the bias, ahead of the candidate filter: top_k counts allowed tokens
                if (constraintSlots_.size() <= s) constraintSlots_.resize(s + 1);
                if (p.fresh) constraintSlots_[s].begin(p);
                if (p.grammar && constraintSlots_[s].dfa != p.grammar) throw Error("json_schema: a row that is not fresh carries another grammar than its slot's");
                constraintSlots_[s].mask(row, vocab, *jsonTable_, p.grammar != nullptr);
            }
            if (p.filter(specs[i].temperature, vocab))
                logitFilterHost(row, vocab, p.topK, minPDelta(specs[i].temperature, p.minP));
        }
        out[i] = sampleHost(row, vocab, specs[i]);
        if (proc && out[i] >= 0 && out[i] < vocab) procCounts_[(size_t)slots[i]][out[i]]++;
        if (proc && (procs[i].json || procs[i].grammar)) constraintSlots_[(size_t)slots[i]].advance(*jsonTable_, procs[i].grammar != nullptr, out[i]);
        if (req >= 1)
            logprobsHost(raw.data(), vocab, !targets.empty() && targets[i] >= 0 ? targets[i] : out[i], std::min(req - 1, kMaxTopLogprobs),
                         &logprobs_[(size_t)i * kLogprobEntries]);
    }
}

void Backend::launchIds(int n, const int *tokens, const int *positions, const int *slots, const SampleSpec *specs) {
    pendingIds_.assign(n, -1);
    if (specs)
        forwardSample(n, tokens, positions, slots, specs, pendingIds_.data());
    else {
        if (!pendingProcs_.empty()) {
            pendingProcs_.clear();
            throw Error("launchIds: logit processors need a sampled forward (specs)");
        }
        if (!pendingPool_.empty()) {
            pendingPool_.clear();
            throw Error("launchIds: pooling needs a sampled forward (specs)");
        }
        takeLogprobTargets(n, nullptr);
        pooled_ = PooledSlots{};
        logprobs_.clear();
        forwardArgmax(n, tokens, positions, slots, pendingIds_.data());
    }
}

void Backend::collectIds(int *out) {
    std::copy(pendingIds_.begin(), pendingIds_.end(), out);
    pendingIds_.clear();
}

void Backend::chainLaunch(int, int, int) { throw Error(name() + " backend: no chained decode"); }
int Backend::chainCollect() { throw Error(name() + " backend: no chained decode"); }
void Backend::copyPrefix(int, int, int) { throw Error(name() + " backend: prefix copy not supported"); }

void Backend::forkPrefix(int src, const int *dsts, int m, int n) {
    const int nSlots = kvSlots();  // every check before the first copy
    DL_CHECK(m >= 1 && dsts != nullptr, "forkPrefix: no destination slot");
    DL_CHECK(src >= 0 && src < nSlots, "forkPrefix: slot out of range");
    for (int i = 0; i < m; i++) {
        DL_CHECK(dsts[i] >= 0 && dsts[i] < nSlots, "forkPrefix: slot out of range");
        DL_CHECK(dsts[i] != src, "forkPrefix: source and destination slot are the same");
        for (int j = 0; j < i; j++) DL_CHECK(dsts[i] != dsts[j], "forkPrefix: a destination slot is named twice");
    }
    DL_CHECK(n >= 1 && (u32)n < header().seqLen, "forkPrefix: prefix length out of range");
    for (int i = 0; i < m; i++) copyPrefix(src, dsts[i], n);
}

}  // namespace dl
