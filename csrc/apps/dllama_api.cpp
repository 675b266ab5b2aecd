// `dllama-api` — OpenAI-style HTTP server over the multi-user scheduler
// (reference: src/dllama-api.cpp:250-410, src/api-types.hpp).
//
//   POST /v1/chat/completions  {"messages":[...], "max_tokens", "temperature", "top_p", "seed",
//                               "stop", "stream", "logprobs", "top_logprobs", "n"}
//        -> {"generated_text": ...} (the reference/web-ui shape) plus the OpenAI
//           {"id","object","created","model","choices":[...],"usage":{...}} fields;
//           "stream": true -> server-sent events with chat.completion.chunk objects + [DONE]
//           "logprobs": true (+ "top_logprobs": 0..20) -> choices[0].logprobs.content, one entry
//           per generated token: log_softmax of the raw logits, whatever temperature / top_p
//           "n": 1..--slots -> that many choices over one prompt, choice i drawn with seed + i; the
//           prompt is prefilled once and its KV forked to the siblings (Scheduler::submitGroup);
//           usage counts the prompt once and sums the completions; streamed chunks carry their
//           choice's index, each index ends with its own finish_reason chunk, one [DONE] closes all
//   POST /v1/completions       {"prompt": <string | [strings] | [token ids] | [[token ids]]>, "max_tokens",
//                               "echo", "logprobs": null | 0..20, and the sampling fields of the chat endpoint}
//        -> {"object":"text_completion","choices":[{"text","index","logprobs","finish_reason"}...],"usage"};
//           "echo": true returns the prompt with the completion and, with "logprobs", scores the
//           prompt's tokens too (OpenAI's legacy arrays plus "token_ids" / "top_ids"); "max_tokens": 0
//           then scores without generating; "stream": true -> text_completion chunks + [DONE]
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

    SchemaDfaCache schemaCache{32};  // compiled grammars of response_format json_schema, by schema text

    // response_format {"type": "json_schema", "json_schema": {"name", "schema", "strict", "description"}}:
    // the schema is compiled here, in the handler's thread (or taken from the cache), never in the
    // scheduler loop. Returns what is wrong with the request, empty when p carries the grammar.
    std::string schemaParams(const Value &rf, GenParams &p) {
        const Value &js = rf["json_schema"];
        if (!js.isObject()) return "response_format json_schema needs a json_schema object";
        for (auto &m : js.members())
            if (m.first != "name" && m.first != "schema" && m.first != "strict" && m.first != "description")
                return "response_format json_schema: the member '" + m.first + "' is not supported";
        if (js.contains("name") && !js["name"].isString()) return "response_format json_schema: name must be a string";
        if (js.contains("strict") && !js["strict"].isBool()) return "response_format json_schema: strict must be a boolean";
        if (!js["schema"].isObject()) return "response_format json_schema needs json_schema.schema, an object";
        if (!sess->grammarVocab()) return "response_format json_schema is unavailable: no tokenizer";
        try {
            p.grammar = schemaCache.get(js["schema"], sess->grammarVocab());
        } catch (const SchemaError &e) {
            return e.what();
        }
        return "";
    }

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

    // The request fields that /v1/chat/completions and /v1/completions share: temperature, top_p,
    // seed, stop, stream, max_tokens (taken when a number; each endpoint has its own rule for it),
    // the penalties, logit_bias, top_k, min_p and response_format. Returns what the 400 says (empty: fine).
    std::string sharedParams(const Value &body, GenParams &p, bool &stream) {
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
        stream = body["stream"].isBool() && body["stream"].asBool();
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
            } else if (type == "json_schema") {
                bad = schemaParams(rf, p);
            } else if (type != "text") {
                bad = "response_format must be {\"type\": \"text\"}, {\"type\": \"json_object\"} or {\"type\": \"json_schema\", \"json_schema\": {...}}";
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
        return bad;
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
        bool stream = false;
        int choices = 1;  // "n"
        {
            const std::string shared = sharedParams(body, p, stream);
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
            if (bad.empty()) bad = shared;  // (reported in the order they always were)
            const Value &nv = body["n"];
            if (bad.empty() && !nv.isNull()) {
                if (!nv.isNumber() || nv.asNumber() != std::floor(nv.asNumber()) || nv.asNumber() < 1 || nv.asNumber() > sess->nSlots())
                    bad = "n must be an integer from 1 to the number of KV slots (--slots " + std::to_string(sess->nSlots()) + ")";
                else
                    choices = (int)nv.asNumber();
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
        if (choices > 1) {
            completeGroup(conn, std::move(prompt), p, choices, stream);
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

    // "n" > 1: the choices are the members of one scheduler group (one prefill, the prompt's KV forked
    // to the siblings); member i draws with seed p.seed + i and answers as choice i.
    void completeGroup(HttpConnection &conn, std::vector<int> prompt, const GenParams &p, int n, bool stream) {
        const int promptTokens = (int)prompt.size();
        std::vector<std::shared_ptr<GenRequest>> reqs = sched->submitGroup(std::move(prompt), p, n);
        struct CancelOnExit {  // the client went away, or one choice failed: drop every member
            std::vector<std::shared_ptr<GenRequest>> &rs;
            ~CancelOnExit() {
                for (auto &r : rs) r->cancel();
            }
        } cancelGuard{reqs};
        const std::string id = "chatcmpl-" + std::to_string(reqs[0]->id);
        const long created = (long)std::time(nullptr);
        auto envelope = [&](const char *object) {
            Value v = Value::object();
            v.set("id", id);
            v.set("object", object);
            v.set("created", created);
            v.set("model", model);
            return v;
        };
        if (stream) {
            conn.beginSse();
            std::vector<size_t> lpSent(n, 0);
            std::vector<char> started(n, 0), closed(n, 0);
            GroupSignal &sig = *reqs[0]->signal;
            int open = n;
            while (open > 0) {
                u64 seen;
                {
                    std::lock_guard<std::mutex> lk(sig.mu);
                    seen = sig.events;
                }
                for (int i = 0; i < n; i++) {
                    if (closed[i]) continue;
                    GenRequest &r = *reqs[i];
                    std::string d;
                    bool ended = false;
                    while (r.tryNextDelta(d, ended)) {
                        Value chunk = envelope("chat.completion.chunk");
                        Value ch = Value::object();
                        ch.set("index", i);
                        Value delta = Value::object();
                        if (!started[i]) delta.set("role", "assistant");
                        delta.set("content", d);
                        ch.set("delta", delta);
                        ch.set("logprobs", p.logprobs ? logprobsJson(r, lpSent[i]) : Value());
                        ch.set("finish_reason", Value());
                        chunk.set("choices", Value::array()).push(ch);
                        conn.writeSse(chunk.dump());
                        started[i] = 1;
                    }
                    if (!ended) continue;
                    Value chunk = envelope("chat.completion.chunk");
                    Value ch = Value::object();
                    ch.set("index", i);
                    Value delta = Value::object();
                    if (!started[i]) delta.set("role", "assistant");  // (a choice that produced no text)
                    ch.set("delta", delta);
                    ch.set("logprobs", p.logprobs ? logprobsJson(r, lpSent[i]) : Value());  // the records not sent yet
                    ch.set("finish_reason", r.finishReason);
                    chunk.set("choices", Value::array()).push(ch);
                    conn.writeSse(chunk.dump());
                    closed[i] = 1;
                    open--;
                }
                if (open > 0) {
                    std::unique_lock<std::mutex> lk(sig.mu);
                    sig.cv.wait(lk, [&] { return sig.events != seen; });
                }
            }
            conn.writeSse("[DONE]");
            return;
        }
        Value choices = Value::array();
        int completionTokens = 0;
        std::string first;
        for (int i = 0; i < n; i++) {
            GenRequest &r = *reqs[i];
            const std::string text = r.wait();
            if (r.finishReason == "error") {
                Value err = Value::object();
                err.set("error", r.error.empty() ? "generation failed" : r.error);
                conn.writeJson(500, err.dump());
                return;
            }
            if (i == 0) first = text;
            size_t lpSent = 0;
            Value choice = Value::object();
            choice.set("index", i);
            Value msg = Value::object();
            msg.set("role", "assistant");
            msg.set("content", text);
            choice.set("message", msg);
            choice.set("logprobs", p.logprobs ? logprobsJson(r, lpSent) : Value());
            choice.set("finish_reason", r.finishReason);
            choices.push(choice);
            completionTokens += r.completionTokens;
        }
        Value resp = envelope("chat.completion");
        resp.set("choices", choices);
        Value usage = Value::object();
        usage.set("prompt_tokens", promptTokens);  // the prompt counts once, the completions add up
        usage.set("completion_tokens", completionTokens);
        usage.set("total_tokens", promptTokens + completionTokens);
        Value details = Value::object();
        details.set("cached_tokens", reqs[0]->cachedTokens);  // the leader's: forked siblings are no cache hits
        usage.set("prompt_tokens_details", details);
        resp.set("usage", usage);
        resp.set("generated_text", first);  // choice 0, as the web UI reads it
        conn.writeJson(200, resp.dump());
        if (logLevel() >= 1) {
            std::printf("🔶 %s: %d choices, %d prompt + %d completion tokens\n", id.c_str(), n, promptTokens, completionTokens);
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

    // One item of "input" (embeddings) or "prompt" (completions) as token ids: a string is tokenised
    // as a raw prompt (BOS as for any prompt, no chat template), a list of token ids is taken as it
    // is. Throws what the 400 says.
    std::vector<int> embeddingInput(const Value &item, size_t index, const char *field = "input") {
        const std::string at = std::string(field) + "[" + std::to_string(index) + "]";
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
        std::vector<std::vector<int>> inputs;
        GenParams p;
        p.embed = EmbedMode::MEAN;
        p.maxTokens = 0;
        bool b64 = false;
        try {
            const Value body = Value::parse(req.body);
            if (!body.isObject()) throw std::runtime_error("a JSON object is required");
            inputs = tokenItems(body["input"], "input");
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

    // The items of "input" / "prompt": a string, a list of token ids, a non-empty list of strings or a
    // list of token-id lists, at most kMaxItems of them. Throws what the 400 says.
    static constexpr size_t kMaxItems = 2048;
    std::vector<std::vector<int>> tokenItems(const Value &in, const char *field, std::vector<std::string> *texts = nullptr) {
        const std::string f = field;
        std::vector<std::vector<int>> items;
        auto take = [&](const Value &item, size_t i) {
            items.push_back(embeddingInput(item, i, field));
            if (texts) texts->push_back(item.isString() ? item.asString() : decodeIds(items.back()));
        };
        if (in.isString()) {
            take(in, 0);
        } else if (in.isArray()) {
            if (in.size() == 0) throw std::runtime_error(f + " is empty");
            if (in.items()[0].isNumber()) {  // one list of token ids
                take(in, 0);
            } else {
                if (in.size() > kMaxItems) throw std::runtime_error(f + " holds at most " + std::to_string(kMaxItems) + " items");
                const bool strings = in.items()[0].isString();
                for (size_t i = 0; i < in.size(); i++) {
                    if (in.items()[i].isString() != strings) throw std::runtime_error(f + " mixes strings and token lists");
                    take(in.items()[i], i);
                }
            }
        } else {
            throw std::runtime_error(f + " required: a string, a list of strings, a list of token ids or a list of such lists");
        }
        return items;
    }

    // The tokenizer's decode of a token-id prompt (what `echo` returns for it).
    std::string decodeIds(const std::vector<int> &ids) {
        TokenDecoder dec(sess->tokenizer());
        std::string text, piece;
        for (int t : ids)
            if (dec.decode(t, piece)) text += piece;
        return text;
    }

    // choices[i].logprobs of /v1/completions, OpenAI's legacy arrays, for records [0, recs.size()) of
    // tokens `ids`: "tokens" (the piece as a JSON string), "token_logprobs", "top_logprobs" (one
    // {token string: logprob} object per token; on a string collision the better entry wins),
    // "text_offset" (bytes of the preceding tokens' pieces, special tokens counting 0; `offset` moves
    // on) and, because token strings are ambiguous, "token_ids" and "top_ids" ([id, logprob] pairs in
    // (logit descending, id ascending) order). A record without a token (the first echoed token, which
    // has no context) gives null in the three logprob arrays.
    Value legacyLogprobsJson(const std::vector<int> &ids, const std::vector<TokenRecord> &recs, size_t &offset) {
        Tokenizer &tok = sess->tokenizer();
        auto pieceOf = [&](int id) { return id >= 0 && id < tok.vocabSize() ? tok.piece(id) : std::string(); };
        Value tokens = Value::array(), tlp = Value::array(), top = Value::array(), offs = Value::array(),
              tids = Value::array(), topIds = Value::array();
        for (size_t i = 0; i < recs.size() && i < ids.size(); i++) {
            const TokenRecord &rec = recs[i];
            const std::string piece = pieceOf(ids[i]);
            tokens.push(validUtf8(piece));
            tids.push(ids[i]);
            offs.push((double)offset);
            if (ids[i] < tok.bosId()) offset += piece.size();
            if (rec.chosen.id < 0) {
                tlp.push(Value());
                top.push(Value());
                topIds.push(Value());
                continue;
            }
            tlp.push((double)rec.chosen.logprob);
            Value o = Value::object(), l = Value::array();
            for (const TokenLogprob &t : rec.top) {
                const std::string key = validUtf8(pieceOf(t.id));
                if (!o.contains(key)) o.set(key, (double)t.logprob);
                Value pair = Value::array();
                pair.push(t.id);
                pair.push((double)t.logprob);
                l.push(pair);
            }
            top.push(o);
            topIds.push(l);
        }
        Value lp = Value::object();
        lp.set("tokens", tokens);
        lp.set("token_logprobs", tlp);
        lp.set("top_logprobs", top);
        lp.set("text_offset", offs);
        lp.set("token_ids", tids);
        lp.set("top_ids", topIds);
        return lp;
    }

    // The records of a completions request not yet written: the prompt's (echo with logprobs) from
    // `promptSent`, then the generated tokens' from `genSent`; both move on, with the byte offset.
    struct LegacyCursor {
        size_t promptSent = 0, genSent = 0, offset = 0;
    };
    Value legacyLogprobsJson(GenRequest &r, LegacyCursor &c) {
        std::vector<int> ids;
        std::vector<TokenRecord> recs;
        {
            std::lock_guard<std::mutex> lk(r.mu);
            for (size_t i = c.promptSent; i < r.promptLogprobs.size() && i < r.prompt.size(); i++) {
                ids.push_back(r.prompt[i]);
                recs.push_back(r.promptLogprobs[i]);
            }
            c.promptSent = std::max(c.promptSent, r.promptLogprobs.size());
            for (size_t i = c.genSent; i < r.logprobs.size(); i++) {
                ids.push_back(r.logprobs[i].chosen.id);
                recs.push_back(r.logprobs[i]);
            }
            c.genSent = std::max(c.genSent, r.logprobs.size());
        }
        return legacyLogprobsJson(ids, recs, c.offset);
    }

    // POST /v1/completions: every item of "prompt" becomes one scheduler request; they are submitted
    // together, so they batch with each other and with the chat traffic. `echo` returns the prompt
    // with the completion; with `logprobs` the prompt's tokens are scored too (row i scores token
    // i + 1), and `max_tokens: 0` then scores without generating.
    void completions(const HttpRequest &req, HttpConnection &conn) {
        std::vector<std::vector<int>> prompts;
        std::vector<std::string> texts;
        GenParams p;
        p.completion = true;
        p.maxTokens = 16;
        bool stream = false;
        try {
            const Value body = Value::parse(req.body);
            if (!body.isObject()) throw std::runtime_error("a JSON object is required");
            const std::string bad = sharedParams(body, p, stream);
            if (!bad.empty()) throw std::runtime_error(bad);
            auto integer = [](const Value &v, double lo, double hi) {
                return v.isNumber() && v.asNumber() == std::floor(v.asNumber()) && v.asNumber() >= lo && v.asNumber() <= hi;
            };
            const Value &echo = body["echo"], &lp = body["logprobs"], &mt = body["max_tokens"];
            if (!echo.isNull() && !echo.isBool()) throw std::runtime_error("echo must be a boolean");
            p.echo = echo.isBool() && echo.asBool();
            if (!mt.isNull() && !integer(mt, 0, 2147483647.0)) throw std::runtime_error("max_tokens must be an integer >= 0");
            if (p.maxTokens == 0 && !p.echo) throw std::runtime_error("max_tokens: 0 requires echo: true");
            if (!lp.isNull()) {
                if (!integer(lp, 0, kMaxTopLogprobs))
                    throw std::runtime_error("logprobs must be null or an integer from 0 to " + std::to_string(kMaxTopLogprobs));
                p.logprobs = true;
                p.topLogprobs = (int)lp.asNumber();
            }
            p.promptLogprobs = p.echo && p.logprobs;
            for (const char *one : {"n", "best_of"})
                if (!body[one].isNull() && !(body[one].isNumber() && body[one].asNumber() == 1.0))
                    throw std::runtime_error(std::string(one) + " other than 1 is not supported");
            if (!body["suffix"].isNull()) throw std::runtime_error("suffix is not supported");
            if (!body["top_logprobs"].isNull())
                throw std::runtime_error("top_logprobs belongs to /v1/chat/completions; here logprobs is the count");
            prompts = tokenItems(body["prompt"], "prompt", &texts);
            const size_t seqLen = sess->header().seqLen;
            for (size_t i = 0; i < prompts.size(); i++)  // (one that generates leaves room for a token)
                if (!p.drawsNothing() && prompts[i].size() >= seqLen)
                    throw std::runtime_error("prompt[" + std::to_string(i) + "] has " + std::to_string(prompts[i].size()) +
                                             " tokens, the context holds " + std::to_string(seqLen) + " with the completion");
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
        for (size_t i = 0; i < prompts.size(); i++) {
            GenParams pi = p;
            pi.seed = p.seed + i;  // (items of one request draw from their own generators)
            promptTokens += prompts[i].size();
            reqs.push_back(sched->submit(prompts[i], pi));
        }
        const std::string id = "cmpl-" + std::to_string(reqs[0]->id);
        const long created = (long)std::time(nullptr);
        auto envelope = [&]() {
            Value v = Value::object();
            v.set("id", id);
            v.set("object", "text_completion");
            v.set("created", created);
            v.set("model", model);
            return v;
        };
        if (stream) {
            conn.beginSse();
            for (size_t i = 0; i < reqs.size(); i++) {
                GenRequest &r = *reqs[i];
                LegacyCursor cur;
                auto send = [&](const std::string &text, bool last) {
                    Value chunk = envelope();
                    Value ch = Value::object();
                    ch.set("text", text);
                    ch.set("index", (int)i);
                    ch.set("logprobs", p.logprobs ? legacyLogprobsJson(r, cur) : Value());
                    ch.set("finish_reason", last ? Value(r.finishReason) : Value());
                    chunk.set("choices", Value::array()).push(ch);
                    conn.writeSse(chunk.dump());
                };
                if (p.echo) {  // the prompt and, once every row was scored, its records
                    if (p.promptLogprobs) r.waitPromptLogprobs();
                    send(texts[i], false);
                }
                std::string d;
                while (r.nextDelta(d)) send(d, false);
                send("", true);  // the records not sent yet
            }
            conn.writeSse("[DONE]");
            return;
        }
        Value choices = Value::array();
        int completionTokens = 0, cachedTokens = 0;
        for (size_t i = 0; i < reqs.size(); i++) {
            GenRequest &r = *reqs[i];
            const std::string text = r.wait();
            if (r.finishReason == "error") {
                Value err = Value::object();
                err.set("error", r.error.empty() ? "generation failed" : r.error);
                conn.writeJson(500, err.dump());
                return;
            }
            LegacyCursor cur;
            Value ch = Value::object();
            ch.set("text", p.echo ? texts[i] + text : text);
            ch.set("index", (int)i);
            ch.set("logprobs", p.logprobs ? legacyLogprobsJson(r, cur) : Value());
            ch.set("finish_reason", r.finishReason);
            choices.push(ch);
            completionTokens += r.completionTokens;
            cachedTokens += r.cachedTokens;
        }
        Value resp = envelope();
        resp.set("choices", choices);
        Value usage = Value::object();
        usage.set("prompt_tokens", (double)promptTokens);
        usage.set("completion_tokens", completionTokens);
        usage.set("total_tokens", (double)promptTokens + completionTokens);
        Value details = Value::object();
        details.set("cached_tokens", cachedTokens);
        usage.set("prompt_tokens_details", details);
        resp.set("usage", usage);
        conn.writeJson(200, resp.dump());
        if (logLevel() >= 1) {
            std::printf("🔶 %s: %zu prompts, %zu prompt + %d completion tokens\n", id.c_str(), reqs.size(), promptTokens, completionTokens);
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
        metric("dllama_fork_groups_total", "counter", "Request groups (n > 1) whose siblings were forked from one prefill.",
               (double)s.forkGroups);
        metric("dllama_forked_requests_total", "counter", "Sibling requests that started behind a forked prompt KV.",
               (double)s.forkedRequests);
        metric("dllama_fork_tokens_total", "counter", "Prompt tokens the forked siblings did not prefill.", (double)s.forkTokens);
        metric("dllama_logit_proc_requests_total", "counter", "Finished requests that used penalties or a logit bias.",
               (double)s.logitProcRequests);
        metric("dllama_logit_filter_requests_total", "counter", "Finished requests with top_k or min_p on.",
               (double)s.logitFilterRequests);
        metric("dllama_embedding_requests_total", "counter", "Finished embedding requests.", (double)s.embeddingRequests);
        metric("dllama_json_requests_total", "counter", "Finished requests in JSON mode.", (double)s.jsonRequests);
        metric("dllama_schema_requests_total", "counter", "Finished requests constrained by a JSON schema.", (double)s.schemaRequests);
        metric("dllama_completion_requests_total", "counter", "Finished /v1/completions requests (one per prompt item).",
               (double)s.completionRequests);
        metric("dllama_scored_prompt_tokens_total", "counter", "Prompt tokens scored (echo with logprobs).",
               (double)s.scoredPromptTokens);
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
        v.set("fork_groups", (double)s.forkGroups);
        v.set("forked_requests", (double)s.forkedRequests);
        v.set("fork_tokens", (double)s.forkTokens);
        v.set("logit_proc_requests", (double)s.logitProcRequests);
        v.set("logit_filter_requests", (double)s.logitFilterRequests);
        v.set("json_requests", (double)s.jsonRequests);
        v.set("schema_requests", (double)s.schemaRequests);
        v.set("embedding_requests", (double)s.embeddingRequests);
        v.set("completion_requests", (double)s.completionRequests);
        v.set("scored_prompt_tokens", (double)s.scoredPromptTokens);
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
                 "        (chat requests may ask for \"n\": 1..slots choices: one prefill, forked to the siblings)\n"
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
        server.route("POST", "/v1/completions", [&](const HttpRequest &r, HttpConnection &c) { api.completions(r, c); });
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
