// `dllama-api` — OpenAI-style HTTP server over the multi-user scheduler
// (reference: src/dllama-api.cpp:250-410, src/api-types.hpp).
//
//   POST /v1/chat/completions  {"messages":[...], "max_tokens", "temperature", "top_p", "seed",
//                               "stop", "stream", "logprobs", "top_logprobs"}
//        -> {"generated_text": ...} (the reference/web-ui shape) plus the OpenAI
//           {"id","object","created","model","choices":[...],"usage":{...}} fields;
//           "stream": true -> server-sent events with chat.completion.chunk objects + [DONE]
//           "logprobs": true (+ "top_logprobs": 0..20) -> choices[0].logprobs.content, one entry
//           per generated token: log_softmax of the raw logits, whatever temperature / top_p
//   POST /v1/embeddings        {"input": <string | [strings] | [token ids] | [[token ids]]>, "model",
//                               "encoding_format": "float"|"base64", "pooling": "mean"|"last"}
//        -> {"object":"list","data":[{"object":"embedding","index":i,"embedding":[...]}...],
//            "model":...,"usage":{"prompt_tokens","total_tokens"}}: per input the L2-normalised mean
//           (or last row) of its prompt rows' final hidden states; the inputs batch with each other
//           and with the chat traffic; "pooling" is this server's extension
//   GET  /v1/models            {"object":"list","data":[{"id":<model file name>, ...}]}
//   GET  /health               scheduler counters (JSON)
//   GET  /v1/metrics           the same counters in Prometheus text format
//   GET  /, /app.js, /style.css  the chat web UI (--web-ui <dir>, default ./web-ui when present)
// Requests run concurrently (thread per connection); the scheduler batches them into shared forwards.
#include <cmath>
#include <csignal>
#include <cstdio>
#include <ctime>
#include <fstream>
#include <sstream>
#include <string>

#include "../net/http.h"
#include "../net/json.h"
#include "../runtime/scheduler.h"

using namespace dl;
using json::Value;

namespace {

std::string modelName(const AppArgs &a) {
    if (!a.synthetic.empty()) return a.synthetic;
    const size_t p = a.modelPath.find_last_of("/\\");
    return p == std::string::npos ? a.modelPath : a.modelPath.substr(p + 1);
}

struct Api {
    AppArgs args;
    InferenceSession *sess;
    Scheduler *sched;
    std::unique_ptr<ChatTemplateGenerator> tmpl;
    std::string model;
    std::atomic<u64> counter{0};
    std::string jsonUnavailable;  // why response_format json_object cannot be served (empty: it can)

    std::vector<int> buildPrompt(const Value &messages) {
        std::vector<ChatItem> items;
        for (const Value &m : messages.items()) items.push_back(ChatItem{m["role"].asString(), m["content"].asString()});
        Tokenizer &tok = sess->tokenizer();
        if (tmpl) {
            GeneratedChat g = tmpl->generate(items, true);
            return tok.encode(g.content, true, true);
        }
        // reference behaviour when no chat template is available: "role: content\n" lines
        std::string flat;
        for (auto &it : items) flat += it.role + ": " + it.message + "\n";
        return tok.encode(flat, true, false);
    }

    // The vocabulary piece as a valid JSON string: every maximal invalid part of a UTF-8 sequence (a
    // piece may be part of a character) becomes one U+FFFD; "bytes" carries the piece exactly.
    static std::string validUtf8(const std::string &s) {
        std::string out;
        const size_t n = s.size();
        for (size_t i = 0; i < n;) {
            const unsigned char c = (unsigned char)s[i];
            const size_t len = c < 0x80 ? 1 : (c >= 0xC2 && c <= 0xDF) ? 2 : (c >= 0xE0 && c <= 0xEF) ? 3 : (c >= 0xF0 && c <= 0xF4) ? 4 : 0;
            size_t got = len ? 1 : 0;  // bytes of the sequence that are well-formed so far
            for (; got >= 1 && got < len && i + got < n; got++) {
                const unsigned char d = (unsigned char)s[i + got];
                unsigned char lo = 0x80, hi = 0xBF;
                if (got == 1) {  // no overlong forms, no surrogates, nothing beyond U+10FFFF
                    if (c == 0xE0) lo = 0xA0;
                    if (c == 0xED) hi = 0x9F;
                    if (c == 0xF0) lo = 0x90;
                    if (c == 0xF4) hi = 0x8F;
                }
                if (d < lo || d > hi) break;
            }
            if (len && got == len) {
                out.append(s, i, len);
                i += len;
            } else {
                out += "\xEF\xBF\xBD";
                i += got ? got : 1;
            }
        }
        return out;
    }

    Value tokenJson(const TokenLogprob &t) {
        Tokenizer &tok = sess->tokenizer();
        const std::string piece = t.id >= 0 && t.id < tok.vocabSize() ? tok.piece(t.id) : std::string();
        Value v = Value::object();
        v.set("token", validUtf8(piece));
        v.set("token_id", t.id);
        v.set("logprob", (double)t.logprob);
        Value bytes = Value::array();
        for (unsigned char c : piece) bytes.push((int)c);
        v.set("bytes", bytes);
        return v;
    }

    // choices[0].logprobs for the request's records [from, size): {"content": [...]}; `from` moves on
    Value logprobsJson(GenRequest &r, size_t &from) {
        std::vector<TokenRecord> recs;
        {
            std::lock_guard<std::mutex> lk(r.mu);
            recs.assign(r.logprobs.begin() + std::min(from, r.logprobs.size()), r.logprobs.end());
        }
        from += recs.size();
        Value content = Value::array();
        for (const TokenRecord &rec : recs) {
            Value e = tokenJson(rec.chosen);
            Value top = Value::array();
            for (const TokenLogprob &t : rec.top) top.push(tokenJson(t));
            e.set("top_logprobs", top);
            content.push(e);
        }
        Value lp = Value::object();
        lp.set("content", content);
        return lp;
    }

    void complete(const HttpRequest &req, HttpConnection &conn) {
        Value body;
        try {
            body = Value::parse(req.body);
            if (!body["messages"].isArray() || body["messages"].size() == 0) throw std::runtime_error("messages required");
        } catch (const std::exception &e) {
            Value err = Value::object();
            err.set("error", std::string("Invalid request: ") + e.what());
            conn.writeJson(400, err.dump());
            return;
        }
        GenParams p;
        p.temperature = args.temperature;
        p.topp = args.topp;
        p.seed = args.seed + counter.fetch_add(1);
        if (body["max_tokens"].isNumber()) p.maxTokens = (int)body["max_tokens"].asNumber();
        if (body["temperature"].isNumber()) p.temperature = (float)body["temperature"].asNumber();
        if (body["top_p"].isNumber()) p.topp = (float)body["top_p"].asNumber();
        if (body["seed"].isNumber()) p.seed = (u64)body["seed"].asNumber();
        if (body["stop"].isString()) p.stop.push_back(body["stop"].asString());
        if (body["stop"].isArray())
            for (const Value &s : body["stop"].items())
                if (s.isString()) p.stop.push_back(s.asString());
        const bool stream = body["stream"].isBool() && body["stream"].asBool();
        {
            const Value &lp = body["logprobs"], &top = body["top_logprobs"];
            std::string bad;
            if (!lp.isNull() && !lp.isBool()) bad = "logprobs must be a boolean";
            p.logprobs = lp.isBool() && lp.asBool();
            if (bad.empty() && !top.isNull()) {
                if (!top.isNumber() || top.asNumber() != std::floor(top.asNumber()) || top.asNumber() < 0 ||
                    top.asNumber() > kMaxTopLogprobs)
                    bad = "top_logprobs must be an integer from 0 to " + std::to_string(kMaxTopLogprobs);
                else if (!p.logprobs)
                    bad = "top_logprobs requires logprobs: true";
                else
                    p.topLogprobs = (int)top.asNumber();
            }
            if (!bad.empty()) {
                Value err = Value::object();
                err.set("error", "Invalid request: " + bad);
                conn.writeJson(400, err.dump());
                return;
            }
        }
        {
            std::string bad;
            auto penalty = [&](const char *name, float &dst) {
                const Value &v = body[name];
                if (v.isNull() || !bad.empty()) return;
                if (!v.isNumber() || !(v.asNumber() >= -2.0 && v.asNumber() <= 2.0))
                    bad = std::string(name) + " must be a number from -2 to 2";
                else
                    dst = (float)v.asNumber();
            };
            penalty("frequency_penalty", p.frequencyPenalty);
            penalty("presence_penalty", p.presencePenalty);
            const Value &tk = body["top_k"], &mp = body["min_p"];
            if (bad.empty() && !tk.isNull()) {
                if (!tk.isNumber() || tk.asNumber() != std::floor(tk.asNumber()) || tk.asNumber() < 0)
                    bad = "top_k must be an integer >= 0";
                else  // the whole vocabulary or more: off
                    p.topK = tk.asNumber() >= (double)sess->header().vocabSize ? 0 : (int)tk.asNumber();
            }
            if (bad.empty() && !mp.isNull()) {
                if (!mp.isNumber() || !(mp.asNumber() >= 0.0 && mp.asNumber() <= 1.0))
                    bad = "min_p must be a number from 0 to 1";
                else
                    p.minP = (float)mp.asNumber();
            }
            const Value &rf = body["response_format"];
            if (bad.empty() && !rf.isNull()) {
                const std::string type = rf.isObject() && rf["type"].isString() ? rf["type"].asString() : "";
                if (type == "json_object") {
                    if (jsonUnavailable.empty())
                        p.jsonObject = true;
                    else
                        bad = "response_format json_object is unavailable with this tokenizer: " + jsonUnavailable;
                } else if (type != "text") {
                    bad = "response_format must be {\"type\": \"text\"} or {\"type\": \"json_object\"}";
                }
            }
            const Value &lb = body["logit_bias"];
            if (bad.empty() && !lb.isNull()) {
                const int vocab = (int)sess->header().vocabSize;
                if (!lb.isObject())
                    bad = "logit_bias must be an object of token id: bias";
                else if (lb.size() > (size_t)kMaxLogitBias)
                    bad = "logit_bias holds at most " + std::to_string(kMaxLogitBias) + " entries";
                for (size_t e = 0; bad.empty() && e < lb.size(); e++) {
                    const auto &kv = lb.members()[e];
                    const std::string &k = kv.first;
                    const bool digits = !k.empty() && k.size() <= 9 && k.find_first_not_of("0123456789") == std::string::npos;
                    const int id = digits ? std::atoi(k.c_str()) : -1;
                    if (!digits || id >= vocab)
                        bad = "logit_bias keys must be token ids from 0 to " + std::to_string(vocab - 1);
                    else if (!kv.second.isNumber() || !(kv.second.asNumber() >= -100.0 && kv.second.asNumber() <= 100.0))
                        bad = "logit_bias values must be numbers from -100 to 100";
                    else {
                        for (const LogitBias &e : p.logitBias)
                            if (e.id == id) bad = "logit_bias names token " + std::to_string(id) + " twice";
                        p.logitBias.push_back(LogitBias{id, (float)kv.second.asNumber()});
                    }
                }
            }
            if (!bad.empty()) {
                Value err = Value::object();
                err.set("error", "Invalid request: " + bad);
                conn.writeJson(400, err.dump());
                return;
            }
        }
        std::vector<int> prompt;
        try {
            prompt = buildPrompt(body["messages"]);
        } catch (const std::exception &e) {
            Value err = Value::object();
            err.set("error", std::string("Invalid messages: ") + e.what());
            conn.writeJson(400, err.dump());
            return;
        }
        const int promptTokens = (int)prompt.size();
        auto r = sched->submit(std::move(prompt), p);
        // if this handler unwinds early (client gone: a write throws), stop generating for it
        struct CancelOnExit {
            GenRequest *r;
            ~CancelOnExit() { r->cancel(); }
        } cancelGuard{r.get()};
        const std::string id = "chatcmpl-" + std::to_string(r->id);
        const long created = (long)std::time(nullptr);
        size_t lpSent = 0;  // log-probability records already written (streaming)
        if (stream) {
            conn.beginSse();
            bool first = true;
            std::string d;
            while (r->nextDelta(d)) {
                Value chunk = Value::object();
                chunk.set("id", id);
                chunk.set("object", "chat.completion.chunk");
                chunk.set("created", created);
                chunk.set("model", model);
                Value ch = Value::object();
                ch.set("index", 0);
                Value delta = Value::object();
                if (first) delta.set("role", "assistant");
                delta.set("content", d);
                ch.set("delta", delta);
                ch.set("logprobs", p.logprobs ? logprobsJson(*r, lpSent) : Value());
                ch.set("finish_reason", Value());
                chunk.set("choices", Value::array()).push(ch);
                conn.writeSse(chunk.dump());
                first = false;
            }
            Value chunk = Value::object();
            chunk.set("id", id);
            chunk.set("object", "chat.completion.chunk");
            chunk.set("created", created);
            chunk.set("model", model);
            Value ch = Value::object();
            ch.set("index", 0);
            ch.set("delta", Value::object());
            ch.set("logprobs", p.logprobs ? logprobsJson(*r, lpSent) : Value());  // the records not sent yet
            ch.set("finish_reason", r->finishReason);
            chunk.set("choices", Value::array()).push(ch);
            conn.writeSse(chunk.dump());
            conn.writeSse("[DONE]");
            return;
        }
        const std::string text = r->wait();
        if (r->finishReason == "error") {
            Value err = Value::object();
            err.set("error", r->error.empty() ? "generation failed" : r->error);
            conn.writeJson(500, err.dump());
            return;
        }
        Value resp = Value::object();
        resp.set("id", id);
        resp.set("object", "chat.completion");
        resp.set("created", created);
        resp.set("model", model);
        Value choice = Value::object();
        choice.set("index", 0);
        Value msg = Value::object();
        msg.set("role", "assistant");
        msg.set("content", text);
        choice.set("message", msg);
        choice.set("logprobs", p.logprobs ? logprobsJson(*r, lpSent) : Value());
        choice.set("finish_reason", r->finishReason);
        resp.set("choices", Value::array()).push(choice);
        Value usage = Value::object();
        usage.set("prompt_tokens", promptTokens);
        usage.set("completion_tokens", r->completionTokens);
        usage.set("total_tokens", promptTokens + r->completionTokens);
        Value details = Value::object();  // OpenAI shape; 0 without --prefix-cache or without a hit
        details.set("cached_tokens", r->cachedTokens);
        usage.set("prompt_tokens_details", details);
        resp.set("usage", usage);
        resp.set("generated_text", text);
        conn.writeJson(200, resp.dump());
        if (logLevel() >= 1) {
            std::printf("🔶 %s: %d prompt + %d completion tokens (%s)\n", id.c_str(), promptTokens, r->completionTokens,
                        r->finishReason.c_str());
            std::fflush(stdout);
        }
    }

    static std::string base64(const unsigned char *p, size_t n) {
        static const char *tab = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";
        std::string out;
        out.reserve((n + 2) / 3 * 4);
        for (size_t i = 0; i < n; i += 3) {
            const unsigned v = (unsigned)p[i] << 16 | (i + 1 < n ? (unsigned)p[i + 1] << 8 : 0u) | (i + 2 < n ? (unsigned)p[i + 2] : 0u);
            out.push_back(tab[v >> 18 & 63]);
            out.push_back(tab[v >> 12 & 63]);
            out.push_back(i + 1 < n ? tab[v >> 6 & 63] : '=');
            out.push_back(i + 2 < n ? tab[v & 63] : '=');
        }
        return out;
    }

    // One item of "input" as token ids: a string is tokenised as a raw prompt (BOS as for any
    // prompt, no chat template), a list of token ids is taken as it is. Throws what the 400 says.
    std::vector<int> embeddingInput(const Value &item, size_t index) {
        const std::string at = "input[" + std::to_string(index) + "]";
        const int vocab = (int)sess->header().vocabSize;
        std::vector<int> ids;
        if (item.isString()) {
            if (item.asString().empty()) throw std::runtime_error(at + " is an empty string");
            ids = sess->tokenizer().encode(item.asString(), true, false);
        } else if (item.isArray()) {
            if (item.size() == 0) throw std::runtime_error(at + " is an empty list of token ids");
            for (const Value &t : item.items()) {
                if (!t.isNumber() || t.asNumber() != std::floor(t.asNumber()) || t.asNumber() < 0 || t.asNumber() >= vocab)
                    throw std::runtime_error(at + " holds a token id outside 0.." + std::to_string(vocab - 1));
                ids.push_back((int)t.asNumber());
            }
        } else {
            throw std::runtime_error(at + " must be a string or a list of token ids");
        }
        if (ids.empty()) throw std::runtime_error(at + " has no tokens");
        if (ids.size() > sess->header().seqLen)
            throw std::runtime_error(at + " has " + std::to_string(ids.size()) + " tokens, the context holds " +
                                     std::to_string(sess->header().seqLen));
        return ids;
    }

    // POST /v1/embeddings: every item of "input" becomes one embedding request; they are submitted
    // together, so they batch with each other and with the chat traffic.
    void embeddings(const HttpRequest &req, HttpConnection &conn) {
        constexpr size_t kMaxItems = 2048;
        std::vector<std::vector<int>> inputs;
        GenParams p;
        p.embed = EmbedMode::MEAN;
        p.maxTokens = 0;
        bool b64 = false;
        try {
            const Value body = Value::parse(req.body);
            if (!body.isObject()) throw std::runtime_error("a JSON object is required");
            const Value &in = body["input"];
            if (in.isString()) {
                inputs.push_back(embeddingInput(in, 0));
            } else if (in.isArray()) {
                if (in.size() == 0) throw std::runtime_error("input is empty");
                if (in.items()[0].isNumber()) {  // one list of token ids
                    inputs.push_back(embeddingInput(in, 0));
                } else {
                    if (in.size() > kMaxItems) throw std::runtime_error("input holds at most " + std::to_string(kMaxItems) + " items");
                    const bool strings = in.items()[0].isString();
                    for (size_t i = 0; i < in.size(); i++) {
                        if (in.items()[i].isString() != strings) throw std::runtime_error("input mixes strings and token lists");
                        inputs.push_back(embeddingInput(in.items()[i], i));
                    }
                }
            } else {
                throw std::runtime_error("input required: a string, a list of strings, a list of token ids or a list of such lists");
            }
            if (!body["dimensions"].isNull()) throw std::runtime_error("dimensions is not supported");
            const Value &ef = body["encoding_format"], &pl = body["pooling"];
            if (!ef.isNull()) {
                if (!ef.isString() || (ef.asString() != "float" && ef.asString() != "base64"))
                    throw std::runtime_error("encoding_format must be \"float\" or \"base64\"");
                b64 = ef.asString() == "base64";
            }
            if (!pl.isNull()) {
                if (!pl.isString() || (pl.asString() != "mean" && pl.asString() != "last"))
                    throw std::runtime_error("pooling must be \"mean\" or \"last\"");
                if (pl.asString() == "last") p.embed = EmbedMode::LAST;
            }
        } catch (const std::exception &e) {
            Value err = Value::object();
            err.set("error", std::string("Invalid request: ") + e.what());
            conn.writeJson(400, err.dump());
            return;
        }
        std::vector<std::shared_ptr<GenRequest>> reqs;
        struct CancelOnExit {  // the client went away, or one item failed: drop the rest
            std::vector<std::shared_ptr<GenRequest>> &rs;
            ~CancelOnExit() {
                for (auto &r : rs) r->cancel();
            }
        } cancelGuard{reqs};
        size_t promptTokens = 0;
        for (auto &ids : inputs) {
            promptTokens += ids.size();
            reqs.push_back(sched->submit(std::move(ids), p));
        }
        Value data = Value::array();
        for (size_t i = 0; i < reqs.size(); i++) {
            GenRequest &r = *reqs[i];
            r.wait();
            if (r.finishReason != "stop") {
                Value err = Value::object();
                err.set("error", r.error.empty() ? "embedding failed" : r.error);
                conn.writeJson(500, err.dump());
                return;
            }
            Value e = Value::object();
            e.set("object", "embedding");
            e.set("index", (int)i);
            if (b64) {
                e.set("embedding", base64(reinterpret_cast<const unsigned char *>(r.embedding.data()), r.embedding.size() * sizeof(float)));
            } else {
                Value v = Value::array();
                for (float x : r.embedding) v.push((double)x);
                e.set("embedding", v);
            }
            data.push(e);
        }
        Value resp = Value::object();
        resp.set("object", "list");
        resp.set("data", data);
        resp.set("model", model);
        Value usage = Value::object();
        usage.set("prompt_tokens", (double)promptTokens);
        usage.set("total_tokens", (double)promptTokens);
        resp.set("usage", usage);
        conn.writeJson(200, resp.dump());
        if (logLevel() >= 1) {
            std::printf("🔷 embeddings: %zu inputs, %zu prompt tokens\n", reqs.size(), promptTokens);
            std::fflush(stdout);
        }
    }

    void models(const HttpRequest &, HttpConnection &conn) {
        Value m = Value::object();
        m.set("id", model);
        m.set("object", "model");
        m.set("created", 0);
        m.set("owned_by", "user");
        Value list = Value::object();
        list.set("object", "list");
        list.set("data", Value::array()).push(m);
        conn.writeJson(200, list.dump());
    }

    // Prometheus text exposition of the scheduler counters (SURVEY §5.5 "GET /v1/metrics").
    void metrics(const HttpRequest &, HttpConnection &conn, int connections) {
        const SchedulerStats s = sched->stats();
        std::string out;
        auto metric = [&](const char *name, const char *type, const char *help, double v) {
            char line[256];
            std::snprintf(line, sizeof(line), "# HELP %s %s\n# TYPE %s %s\n%s %.17g\n", name, help, name, type, name, v);
            out += line;
        };
        metric("dllama_forwards_total", "counter", "Batched forward passes run by the scheduler.", (double)s.forwards);
        metric("dllama_rows_total", "counter", "Token rows processed (prefill + decode).", (double)s.rows);
        metric("dllama_prefill_rows_total", "counter", "Prompt token rows prefilled.", (double)s.prefillRows);
        metric("dllama_decode_rows_total", "counter", "Decode token rows.", (double)s.decodeRows);
        metric("dllama_requests_completed_total", "counter", "Finished requests.", (double)s.completed);
        metric("dllama_generated_tokens_total", "counter", "Tokens generated for finished requests.", (double)s.generatedTokens);
        metric("dllama_requests_cancelled_total", "counter", "Requests dropped after their client disconnected.",
               (double)s.cancelled);
        metric("dllama_busy_seconds_total", "counter", "Time spent in forward passes.", s.busyMs / 1000.0);
        metric("dllama_prefix_hits_total", "counter", "Requests admitted behind a reused KV prefix.", (double)s.prefixHits);
        metric("dllama_prefix_tokens_total", "counter", "Prompt tokens served from reused KV instead of prefill.",
               (double)s.prefixTokens);
        metric("dllama_prefix_copies_total", "counter", "Prefix hits that copied KV from an active slot.",
               (double)s.prefixCopies);
        metric("dllama_prefix_evictions_total", "counter", "Idle slots evicted to free KV pages.",
               (double)s.prefixEvictions);
        metric("dllama_logit_proc_requests_total", "counter", "Finished requests that used penalties or a logit bias.",
               (double)s.logitProcRequests);
        metric("dllama_logit_filter_requests_total", "counter", "Finished requests with top_k or min_p on.",
               (double)s.logitFilterRequests);
        metric("dllama_embedding_requests_total", "counter", "Finished embedding requests.", (double)s.embeddingRequests);
        metric("dllama_json_requests_total", "counter", "Finished requests in JSON mode.", (double)s.jsonRequests);
        metric("dllama_active_requests", "gauge", "Requests holding a KV slot.", (double)s.active);
        metric("dllama_queued_requests", "gauge", "Requests waiting for a KV slot.", (double)s.queued);
        metric("dllama_kv_slots", "gauge", "KV-cache slots (max concurrent sequences).", (double)sess->nSlots());
        metric("dllama_nodes", "gauge", "Tensor-parallel ranks.", (double)sess->nNodes());
        metric("dllama_http_connections", "gauge", "Open HTTP connections.", (double)connections);
        conn.writeResponse(200, "text/plain; version=0.0.4; charset=utf-8", out);
    }

    void health(const HttpRequest &, HttpConnection &conn) {
        SchedulerStats s = sched->stats();
        Value v = Value::object();
        v.set("status", "ok");
        v.set("model", model);
        v.set("backend", sess->isGpu() ? "hip" : "cpu");
        v.set("nodes", sess->nNodes());
        v.set("slots", sess->nSlots());
        v.set("active", s.active);
        v.set("queued", s.queued);
        v.set("forwards", (double)s.forwards);
        v.set("rows", (double)s.rows);
        v.set("prefill_rows", (double)s.prefillRows);
        v.set("decode_rows", (double)s.decodeRows);
        v.set("completed", (double)s.completed);
        v.set("cancelled", (double)s.cancelled);
        v.set("generated_tokens", (double)s.generatedTokens);
        v.set("busy_ms", s.busyMs);
        v.set("prefix_hits", (double)s.prefixHits);
        v.set("prefix_tokens", (double)s.prefixTokens);
        v.set("prefix_copies", (double)s.prefixCopies);
        v.set("prefix_evictions", (double)s.prefixEvictions);
        v.set("logit_proc_requests", (double)s.logitProcRequests);
        v.set("logit_filter_requests", (double)s.logitFilterRequests);
        v.set("json_requests", (double)s.jsonRequests);
        v.set("embedding_requests", (double)s.embeddingRequests);
        conn.writeJson(200, v.dump());
    }
};

bool readFile(const std::string &path, std::string &out) {
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    std::ostringstream ss;
    ss << f.rdbuf();
    out = ss.str();
    return true;
}

void serveWebUi(HttpServer &server, const std::string &dir) {
    static const char *files[][3] = {{"/", "index.html", "text/html; charset=utf-8"},
                                     {"/app.js", "app.js", "application/javascript"},
                                     {"/style.css", "style.css", "text/css"}};
    for (auto &f : files) {
        const std::string path = dir + "/" + f[1], type = f[2];
        server.route("GET", f[0], [path, type](const HttpRequest &, HttpConnection &c) {
            std::string body;
            if (readFile(path, body))
                c.writeResponse(200, type, body);
            else
                c.writeJson(404, "{\"error\":\"web ui file missing\"}");
        });
    }
}

void usage() {
    std::fprintf(stderr,
                 "Usage: dllama-api {--model <path>} {--tokenizer <path>} [--port <p>]\n"
                 "        [--buffer-float-type {f32|f16|q40|q80}]\n"
                 "        [--max-seq-len <max>] [--slots <n>] [--max-batch <n>] [--prefill-chunk <n>]\n"
                 "        [--kv-pages <n> --kv-page-size <p>]   (GPU paged KV: slots share a page pool)\n"
                 "        [--prefix-cache {0|1}] [--prefix-cache-min <n>]   (reuse the KV of shared prompt prefixes)\n"
                 "        [--nthreads <n>] [--gpu-index <i>]\n"
                 "        [--workers <ip:port> ...]\n"
                 "        [--temperature <temp>] [--topp <t>] [--seed <s>] [--chat-template <t>]\n"
                 "        [--web-ui <dir>] [--metrics <file|->]\n");
}

}  // namespace

int main(int argc, char **argv) {
#ifdef SIGPIPE
    std::signal(SIGPIPE, SIG_IGN);
#endif
    try {
        AppArgs args = AppArgs::parse(argc, argv, false);
        if (args.help) {
            usage();
            return 0;
        }
        InferenceSession sess(args, args.slots > 0 ? args.slots : 8);
        Api api;
        api.args = args;
        api.sess = &sess;
        api.model = modelName(args);
        ChatStops stops(sess.tokenizer());
        if (!stops.stops.empty() && (sess.tokenizer().hasChatTemplate() || args.chatTemplate != ChatTemplateType::UNKNOWN)) {
            try {
                api.tmpl.reset(new ChatTemplateGenerator(args.chatTemplate, sess.tokenizer().chatTemplate(), stops.stops[0]));
            } catch (const std::exception &e) {
                std::printf("⚠️  chat template unavailable (%s); using role-prefixed prompts\n", e.what());
            }
        }
        api.jsonUnavailable = sess.enableJsonMode();
        if (!api.jsonUnavailable.empty())
            std::printf("⚠️  response_format json_object is unavailable: %s\n", api.jsonUnavailable.c_str());
        Scheduler sched(sess);
        api.sched = &sched;
        HttpServer server(args.port);
        server.route("POST", "/v1/chat/completions", [&](const HttpRequest &r, HttpConnection &c) { api.complete(r, c); });
        server.route("POST", "/v1/embeddings", [&](const HttpRequest &r, HttpConnection &c) { api.embeddings(r, c); });
        server.route("GET", "/v1/models", [&](const HttpRequest &r, HttpConnection &c) { api.models(r, c); });
        server.route("GET", "/health", [&](const HttpRequest &r, HttpConnection &c) { api.health(r, c); });
        server.route("GET", "/v1/metrics",
                     [&](const HttpRequest &r, HttpConnection &c) { api.metrics(r, c, server.activeConnections()); });
        std::string ui = args.webUi;
        std::string probe;
        if (ui.empty() && readFile("web-ui/index.html", probe)) ui = "web-ui";
        if (!ui.empty()) {
            serveWebUi(server, ui);
            std::printf("Web UI: http://127.0.0.1:%d/\n", args.port);
        }
        std::printf("Server URL: http://127.0.0.1:%d/v1/\n", args.port);
        std::fflush(stdout);
        server.serveForever();
    } catch (const std::exception &e) {
        std::printf("🚨 Critical error: %s\n", e.what());
        return 1;
    }
    return 0;
}
