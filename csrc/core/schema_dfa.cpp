#include "schema_dfa.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>

namespace dl {

std::string GrammarDfa::tableBytes() const {
    std::string out((const char *)classOf, 256);
    const u32 head[3] = {nClasses, nStates, start};
    out.append((const char *)head, sizeof(head));
    out.append((const char *)next.data(), next.size() * sizeof(uint16_t));
    out.append((const char *)accept.data(), accept.size() * sizeof(uint32_t));
    return out;
}

std::string grammarCheck(const GrammarDfa &g) {
    if (g.nClasses < 1 || g.nClasses > 256) return "nClasses must be 1..256";
    if (g.nStates < 1 || g.nStates > kGrammarMaxStates) return "nStates must be 1.." + std::to_string(kGrammarMaxStates);
    if ((size_t)g.nStates * g.nClasses > kGrammarMaxEntries)
        return "more than " + std::to_string(kGrammarMaxEntries) + " table entries (nStates * nClasses)";
    if (g.next.size() != (size_t)g.nStates * g.nClasses) return "next must hold nStates * nClasses entries";
    if (g.accept.size() != (g.nStates + 31) / 32) return "accept must hold one bit per state, in 32-bit words";
    if (g.start >= g.nStates) return "start is not a state";
    for (int c = 0; c < 256; c++)
        if (g.classOf[c] >= g.nClasses) return "classOf names a class >= nClasses";
    for (uint16_t n : g.next)
        if (n != kGrammarDead && n >= g.nStates) return "next names a state >= nStates";
    for (u32 s = g.nStates; s < (u32)g.accept.size() * 32; s++)
        if ((g.accept[s >> 5] >> (s & 31u)) & 1u) return "an accept bit behind the last state";
    return "";
}

GrammarVocab makeGrammarVocab(const std::vector<uint32_t> &off, const std::vector<uint32_t> &info, const std::vector<uint32_t> &words) {
    GrammarVocab v;
    for (size_t t = 0; t < info.size(); t++) {
        if (jsonTokenClass(info[t]) == JT_EOS) v.eos = true;
        if (jsonTokenClass(info[t]) == JT_REGULAR && jsonTokenLen(info[t]) == 1 && off[t] < words.size())
            v.single[words[off[t]] & 0xffu] = true;
    }
    return v;
}

namespace {

using json::Value;

struct Nfa {
    struct Edge {
        u8 lo, hi;
        int to;
    };
    std::vector<std::vector<Edge>> edges;
    std::vector<std::vector<int>> eps;
    int add() {
        if (edges.size() >= kSchemaMaxNfaStates)
            throw SchemaError("json_schema: the schema is too large: more than " + std::to_string(kSchemaMaxNfaStates) +
                              " NFA states (cap)");
        edges.emplace_back();
        eps.emplace_back();
        return (int)edges.size() - 1;
    }
    void edge(int from, int lo, int hi, int to) { edges[from].push_back(Edge{(u8)lo, (u8)hi, to}); }
    void edge(int from, int c, int to) { edge(from, c, c, to); }
    void e(int from, int to) { eps[from].push_back(to); }
    int lit(int from, const std::string &bytes) {
        for (unsigned char c : bytes) {
            const int to = add();
            edge(from, c, to);
            from = to;
        }
        return from;
    }
    // one optional 0x20
    int optSpace(int from) {
        const int to = add();
        e(from, to);
        edge(from, 0x20, to);
        return to;
    }
};

bool wellFormedUtf8(const std::string &s) {
    size_t i = 0;
    const size_t n = s.size();
    while (i < n) {
        const u8 c = (u8)s[i];
        int need = 0;
        u8 lo = 0x80, hi = 0xBF;
        if (c < 0x80) {
            i++;
            continue;
        } else if (c >= 0xC2 && c <= 0xDF) {
            need = 1;
        } else if (c >= 0xE0 && c <= 0xEF) {
            need = 2;
            if (c == 0xE0) lo = 0xA0;
            if (c == 0xED) hi = 0x9F;
        } else if (c >= 0xF0 && c <= 0xF4) {
            need = 3;
            if (c == 0xF0) lo = 0x90;
            if (c == 0xF4) hi = 0x8F;
        } else {
            return false;
        }
        if (i + (size_t)need >= n) return false;
        for (int k = 1; k <= need; k++) {
            const u8 d = (u8)s[i + k];
            if (d < lo || d > hi) return false;
            lo = 0x80, hi = 0xBF;
        }
        i += 1 + need;
    }
    return true;
}

// the one spelling of a string in an enum, a const or a property name
std::string spellString(const std::string &s, const std::string &where) {
    if (!wellFormedUtf8(s)) throw SchemaError("json_schema: " + where + ": a string that is not well-formed UTF-8");
    std::string out = "\"";
    for (unsigned char c : s) {
        if (c == '"') {
            out += "\\\"";
        } else if (c == '\\') {
            out += "\\\\";
        } else if (c < 0x20) {
            char buf[8];
            std::snprintf(buf, sizeof(buf), "\\u%04x", c);
            out += buf;
        } else {
            out.push_back((char)c);
        }
    }
    out.push_back('"');
    return out;
}

// -?(0|[1-9][0-9]*)(\.[0-9]+)?([eE][+-]?[0-9]+)?; sets integer when there is no fraction or exponent
bool numberTextOk(const std::string &t, bool &integer) {
    size_t i = 0;
    const size_t n = t.size();
    auto digit = [&](size_t k) { return k < n && t[k] >= '0' && t[k] <= '9'; };
    if (i < n && t[i] == '-') i++;
    if (!digit(i)) return false;
    if (t[i] == '0') {
        i++;
    } else {
        while (digit(i)) i++;
    }
    integer = true;
    if (i < n && t[i] == '.') {
        integer = false;
        i++;
        if (!digit(i)) return false;
        while (digit(i)) i++;
    }
    if (i < n && (t[i] == 'e' || t[i] == 'E')) {
        integer = false;
        i++;
        if (i < n && (t[i] == '+' || t[i] == '-')) i++;
        if (!digit(i)) return false;
        while (digit(i)) i++;
    }
    return i == n;
}

// the cache's key: the schema's text, numbers as their source spells them
void serialise(const Value &v, std::string &out) {
    switch (v.type()) {
    case Value::NUMBER:
        out += v.numberText().empty() ? v.dump() : v.numberText();
        break;
    case Value::ARRAY:
        out.push_back('[');
        for (size_t i = 0; i < v.items().size(); i++) {
            if (i) out.push_back(',');
            serialise(v.items()[i], out);
        }
        out.push_back(']');
        break;
    case Value::OBJECT:
        out.push_back('{');
        for (size_t i = 0; i < v.members().size(); i++) {
            if (i) out.push_back(',');
            out += Value(v.members()[i].first).dump();
            out.push_back(':');
            serialise(v.members()[i].second, out);
        }
        out.push_back('}');
        break;
    default:
        out += v.dump();
    }
}

const char *const kIgnored[] = {"title", "description", "default", "examples", "$schema", "$defs"};
const char *const kKnown[] = {"type",  "properties", "required", "additionalProperties", "items",     "minItems", "maxItems",
                              "enum",  "const",      "anyOf",    "$ref",                 "minLength", "maxLength"};
const char *const kTypes[] = {"string", "number", "integer", "boolean", "null", "object", "array"};

template <size_t N>
bool among(const char *const (&list)[N], const std::string &k) {
    for (const char *s : list)
        if (k == s) return true;
    return false;
}

class Compiler {
  public:
    explicit Compiler(const Value &root) : root_(root) {}

    std::shared_ptr<const GrammarDfa> run(const GrammarVocab *vocab) {
        if (!root_.isObject()) throw SchemaError("json_schema: schema must be an object");
        const Value &type = root_["type"];
        if (!type.isString() || type.asString() != "object")
            throw SchemaError("json_schema: the top level must be of type object");
        const int start = nfa_.add();
        final_ = value(root_, start, "#");
        return determinise(start, vocab);
    }

  private:
    const Value &root_;
    Nfa nfa_;
    int final_ = -1;
    std::vector<std::string> refStack_;

    static std::string at(const std::string &path) { return " (at " + path + ")"; }

    // `build(from)` for every alternative, joined behind a common end state
    template <class F>
    int alternatives(int from, size_t n, F build) {
        const int end = nfa_.add();
        for (size_t i = 0; i < n; i++) {
            const int s = nfa_.add();
            nfa_.e(from, s);
            const int t = build(i, s);
            if (t >= 0) nfa_.e(t, end);
        }
        return end;
    }

    void siblings(const Value &node, const char *alone, const std::string &path) {
        for (auto &m : node.members())
            if (m.first != alone && !among(kIgnored, m.first))
                throw SchemaError(std::string("json_schema: '") + alone + "' next to the keyword '" + m.first + "' is not supported" + at(path));
    }

    int intKeyword(const Value &node, const char *key, int dflt, int cap, const std::string &path) {
        const Value &v = node[key];
        if (v.isNull() && !node.contains(key)) return dflt;
        if (!v.isNumber() || v.asNumber() != std::floor(v.asNumber()) || v.asNumber() < 0 || v.asNumber() > cap)
            throw SchemaError(std::string("json_schema: '") + key + "' must be an integer from 0 to " + std::to_string(cap) + at(path));
        return (int)v.asNumber();
    }

    int value(const Value &node, int from, const std::string &path) {
        if (!node.isObject()) throw SchemaError("json_schema: a schema must be an object" + at(path));
        for (auto &m : node.members())
            if (!among(kIgnored, m.first) && !among(kKnown, m.first))
                throw SchemaError("json_schema: the keyword '" + m.first + "' is not supported" + at(path));
        if (node.contains("$ref")) {
            siblings(node, "$ref", path);
            const Value &r = node["$ref"];
            const std::string prefix = "#/$defs/";
            if (!r.isString() || r.asString().compare(0, prefix.size(), prefix) != 0)
                throw SchemaError("json_schema: '$ref' must be \"#/$defs/NAME\"" + at(path));
            const std::string name = r.asString().substr(prefix.size());
            if (!root_["$defs"].isObject() || !root_["$defs"].contains(name))
                throw SchemaError("json_schema: '$ref' to an unknown definition '" + name + "'" + at(path));
            if (std::find(refStack_.begin(), refStack_.end(), name) != refStack_.end())
                throw SchemaError("json_schema: recursive '$ref' to '" + name + "' is not supported" + at(path));
            refStack_.push_back(name);
            const int end = value(root_["$defs"][name], from, "#/$defs/" + name);
            refStack_.pop_back();
            return end;
        }
        if (node.contains("anyOf")) {
            siblings(node, "anyOf", path);
            const Value &a = node["anyOf"];
            if (!a.isArray() || a.size() == 0) throw SchemaError("json_schema: 'anyOf' must be a non-empty array" + at(path));
            return alternatives(from, a.size(), [&](size_t i, int s) { return value(a.items()[i], s, path + "/anyOf/" + std::to_string(i)); });
        }
        std::vector<std::string> types;
        if (node.contains("type")) {
            const Value &t = node["type"];
            if (t.isString()) {
                types.push_back(t.asString());
            } else if (t.isArray() && t.size() > 0) {
                for (auto &x : t.items()) {
                    if (!x.isString()) throw SchemaError("json_schema: 'type' must be a name or a list of names" + at(path));
                    if (std::find(types.begin(), types.end(), x.asString()) == types.end()) types.push_back(x.asString());
                }
            } else {
                throw SchemaError("json_schema: 'type' must be a name or a non-empty list of names" + at(path));
            }
            for (auto &t2 : types)
                if (!among(kTypes, t2)) throw SchemaError("json_schema: 'type' names '" + t2 + "', which is not a JSON type" + at(path));
        }
        if (node.contains("enum") || node.contains("const")) {
            if (node.contains("enum") && node.contains("const"))
                throw SchemaError("json_schema: 'enum' next to the keyword 'const' is not supported" + at(path));
            std::vector<Value> vals;
            if (node.contains("const")) {
                vals.push_back(node["const"]);
            } else {
                if (!node["enum"].isArray() || node["enum"].size() == 0)
                    throw SchemaError("json_schema: 'enum' must be a non-empty array" + at(path));
                vals = node["enum"].items();
            }
            const char *kw = node.contains("const") ? "const" : "enum";
            std::vector<std::string> spelled;
            for (auto &v : vals) {
                std::string s, kind;
                if (v.isString()) {
                    s = spellString(v.asString(), kw), kind = "string";
                } else if (v.isNumber()) {
                    bool integer = false;
                    s = v.numberText();
                    if (!numberTextOk(s, integer))
                        throw SchemaError(std::string("json_schema: '") + kw + "': the number '" + s + "' is not spelled as JSON spells numbers" + at(path));
                    kind = integer ? "integer" : "number";
                } else if (v.isBool()) {
                    s = v.asBool() ? "true" : "false", kind = "boolean";
                } else if (v.isNull()) {
                    s = "null", kind = "null";
                } else {
                    throw SchemaError(std::string("json_schema: '") + kw + "' supports scalar values only" + at(path));
                }
                if (!types.empty()) {
                    bool match = std::find(types.begin(), types.end(), kind) != types.end();
                    if (kind == "integer" && std::find(types.begin(), types.end(), "number") != types.end()) match = true;
                    if (!match) continue;
                }
                if (std::find(spelled.begin(), spelled.end(), s) == spelled.end()) spelled.push_back(s);
            }
            if (spelled.empty())
                throw SchemaError(std::string("json_schema: '") + kw + "' has no value of the schema's 'type'" + at(path));
            return alternatives(from, spelled.size(), [&](size_t i, int s) { return nfa_.lit(s, spelled[i]); });
        }
        if (types.empty())
            throw SchemaError("json_schema: a schema without 'type', 'enum', 'const', 'anyOf' or '$ref' accepts any value, which is not supported" + at(path));
        if (types.size() == 1) return typed(types[0], node, from, path);
        return alternatives(from, types.size(), [&](size_t i, int s) { return typed(types[i], node, s, path); });
    }

    int typed(const std::string &type, const Value &node, int from, const std::string &path) {
        if (type == "string") return string(node, from, path);
        if (type == "number") return number(from, false);
        if (type == "integer") return number(from, true);
        if (type == "boolean")
            return alternatives(from, 2, [&](size_t i, int s) { return nfa_.lit(s, i ? "false" : "true"); });
        if (type == "null") return nfa_.lit(from, "null");
        if (type == "object") return object(node, from, path);
        return array(node, from, path);
    }

    int number(int from, bool integer) {
        Nfa &n = nfa_;
        const int s1 = n.add();
        n.e(from, s1);
        n.edge(from, '-', s1);
        const int intEnd = n.add(), d = n.add();
        n.edge(s1, '0', intEnd);
        n.edge(s1, '1', '9', d);
        n.edge(d, '0', '9', d);
        n.e(d, intEnd);
        if (integer) return intEnd;
        const int fracEnd = n.add(), dot = n.add(), f = n.add();
        n.e(intEnd, fracEnd);
        n.edge(intEnd, '.', dot);
        n.edge(dot, '0', '9', f);
        n.edge(f, '0', '9', f);
        n.e(f, fracEnd);
        const int end = n.add(), ex = n.add(), sg = n.add(), x = n.add();
        n.e(fracEnd, end);
        n.edge(fracEnd, 'e', ex);
        n.edge(fracEnd, 'E', ex);
        n.e(ex, sg);
        n.edge(ex, '+', sg);
        n.edge(ex, '-', sg);
        n.edge(sg, '0', '9', x);
        n.edge(x, '0', '9', x);
        n.e(x, end);
        return end;
    }

    // one code point inside a string: a plain byte, an escape or a well-formed UTF-8 sequence
    void codePoint(int from, int to) {
        Nfa &n = nfa_;
        n.edge(from, 0x20, 0x21, to);
        n.edge(from, 0x23, 0x5B, to);
        n.edge(from, 0x5D, 0x7F, to);
        const int c1 = n.add(), c2 = n.add();  // one / two continuation bytes owed
        n.edge(c1, 0x80, 0xBF, to);
        n.edge(c2, 0x80, 0xBF, c1);
        n.edge(from, 0xC2, 0xDF, c1);
        const int e0 = n.add(), ed = n.add();
        n.edge(from, 0xE0, e0);
        n.edge(e0, 0xA0, 0xBF, c1);
        n.edge(from, 0xE1, 0xEC, c2);
        n.edge(from, 0xEE, 0xEF, c2);
        n.edge(from, 0xED, ed);
        n.edge(ed, 0x80, 0x9F, c1);
        const int f0 = n.add(), f13 = n.add(), f4 = n.add();
        n.edge(from, 0xF0, f0);
        n.edge(f0, 0x90, 0xBF, c2);
        n.edge(from, 0xF1, 0xF3, f13);
        n.edge(f13, 0x80, 0xBF, c2);
        n.edge(from, 0xF4, f4);
        n.edge(f4, 0x80, 0x8F, c2);
        const int esc = n.add();
        n.edge(from, '\\', esc);
        for (char c : std::string("\"\\/bfnrt")) n.edge(esc, (u8)c, to);
        int h = n.add();
        n.edge(esc, 'u', h);
        for (int k = 0; k < 4; k++) {
            const int nx = k == 3 ? to : n.add();
            n.edge(h, '0', '9', nx);
            n.edge(h, 'a', 'f', nx);
            n.edge(h, 'A', 'F', nx);
            h = nx;
        }
    }

    int string(const Value &node, int from, const std::string &path) {
        const int minLen = intKeyword(node, "minLength", 0, kSchemaMaxLength, path);
        const int maxLen = intKeyword(node, "maxLength", -1, kSchemaMaxLength, path);
        if (maxLen >= 0 && minLen > maxLen) throw SchemaError("json_schema: 'minLength' is greater than 'maxLength'" + at(path));
        Nfa &n = nfa_;
        int q = n.add();
        n.edge(from, '"', q);
        const int end = n.add();
        for (int i = 0; i < minLen; i++) {
            const int nx = n.add();
            codePoint(q, nx);
            q = nx;
        }
        if (maxLen < 0) {
            codePoint(q, q);
            n.edge(q, '"', end);
            return end;
        }
        for (int i = minLen; i < maxLen; i++) {
            n.edge(q, '"', end);
            const int nx = n.add();
            codePoint(q, nx);
            q = nx;
        }
        n.edge(q, '"', end);
        return end;
    }

    int object(const Value &node, int from, const std::string &path) {
        if (!node["properties"].isObject())
            throw SchemaError("json_schema: an object schema needs 'properties' (an object without them accepts any members)" + at(path));
        const Value &props = node["properties"];
        if (node.contains("additionalProperties")) {
            const Value &ap = node["additionalProperties"];
            if (!ap.isBool() || ap.asBool())
                throw SchemaError("json_schema: 'additionalProperties' must be false or absent" + at(path));
        }
        std::vector<std::string> req;
        if (node.contains("required")) {
            if (!node["required"].isArray()) throw SchemaError("json_schema: 'required' must be an array of names" + at(path));
            for (auto &r : node["required"].items()) {
                if (!r.isString()) throw SchemaError("json_schema: 'required' must be an array of names" + at(path));
                req.push_back(r.asString());
            }
        }
        std::vector<std::string> seen;
        for (auto &m : props.members()) {
            if (std::find(req.begin(), req.end(), m.first) == req.end())
                throw SchemaError("json_schema: the property '" + m.first + "' is missing from 'required' (optional properties are not supported)" + at(path));
            if (std::find(seen.begin(), seen.end(), m.first) != seen.end())
                throw SchemaError("json_schema: 'properties' names '" + m.first + "' twice" + at(path));
            seen.push_back(m.first);
        }
        for (auto &r : req)
            if (!props.contains(r)) throw SchemaError("json_schema: 'required' names '" + r + "', which is not in 'properties'" + at(path));
        Nfa &n = nfa_;
        int q = n.lit(from, "{");
        bool first = true;
        for (auto &m : props.members()) {
            if (!first) q = n.optSpace(n.lit(q, ","));
            first = false;
            q = n.lit(q, spellString(m.first, "properties"));
            q = n.optSpace(n.lit(q, ":"));
            q = value(m.second, q, path + "/properties/" + m.first);
        }
        return n.lit(q, "}");
    }

    int array(const Value &node, int from, const std::string &path) {
        if (!node.contains("items")) throw SchemaError("json_schema: an array schema needs 'items'" + at(path));
        const int minItems = intKeyword(node, "minItems", 0, kSchemaMaxItems, path);
        const int maxItems = intKeyword(node, "maxItems", -1, kSchemaMaxItems, path);
        if (maxItems >= 0 && minItems > maxItems) throw SchemaError("json_schema: 'minItems' is greater than 'maxItems'" + at(path));
        Nfa &n = nfa_;
        const Value &items = node["items"];
        const std::string ipath = path + "/items";
        const int open = n.lit(from, "[");
        const int end = n.add();
        if (minItems == 0) n.edge(open, ']', end);
        if (maxItems == 0) return end;
        int q = value(items, open, ipath);  // behind the first item
        int count = 1;
        while (true) {
            if (count >= minItems) n.edge(q, ']', end);
            if (maxItems >= 0 && count >= maxItems) break;
            if (maxItems < 0 && count >= std::max(minItems, 1)) {  // unbounded: loop
                const int sep = n.optSpace(n.lit(q, ","));
                const int back = value(items, sep, ipath);
                n.e(back, q);
                break;
            }
            q = value(items, n.optSpace(n.lit(q, ",")), ipath);
            count++;
        }
        return end;
    }

    std::shared_ptr<const GrammarDfa> determinise(int start, const GrammarVocab *vocab) {
        const size_t N = nfa_.edges.size();
        std::vector<u32> stamp(N, 0);
        u32 tick = 0;
        std::vector<int> stack;
        auto closure = [&](std::vector<int> &set) {  // in: seeds; out: sorted closure
            tick++;
            stack.clear();
            std::vector<int> out;
            for (int s : set)
                if (stamp[s] != tick) stamp[s] = tick, stack.push_back(s), out.push_back(s);
            while (!stack.empty()) {
                const int s = stack.back();
                stack.pop_back();
                for (int t : nfa_.eps[s])
                    if (stamp[t] != tick) stamp[t] = tick, stack.push_back(t), out.push_back(t);
            }
            std::sort(out.begin(), out.end());
            set.swap(out);
        };
        std::map<std::vector<int>, int> ids;
        std::vector<std::vector<int>> sets;
        std::vector<std::vector<uint16_t>> trans;  // [state][256]
        auto intern = [&](std::vector<int> &set) {
            auto it = ids.find(set);
            if (it != ids.end()) return it->second;
            if (sets.size() >= kGrammarMaxStates)
                throw SchemaError("json_schema: the schema is too large: more than " + std::to_string(kGrammarMaxStates) + " DFA states (cap)");
            const int id = (int)sets.size();
            ids.emplace(set, id);
            sets.push_back(set);
            trans.emplace_back(256, (uint16_t)kGrammarDead);
            return id;
        };
        std::vector<int> s0 = {start};
        closure(s0);
        intern(s0);
        std::vector<const Nfa::Edge *> es;
        for (size_t i = 0; i < sets.size(); i++) {
            es.clear();
            bool cut[257] = {false};
            const std::vector<int> members = sets[i];  // (sets grows below)
            for (int s : members)
                for (auto &e : nfa_.edges[s]) {
                    es.push_back(&e);
                    cut[e.lo] = true;
                    cut[(int)e.hi + 1] = true;
                }
            int a = 0;
            while (a < 256) {
                int b = a + 1;
                while (b < 256 && !cut[b]) b++;
                std::vector<int> target;
                for (auto *e : es)
                    if (e->lo <= a && a <= e->hi) target.push_back(e->to);
                if (!target.empty()) {
                    closure(target);
                    const int id = intern(target);
                    for (int c = a; c < b; c++) trans[i][c] = (uint16_t)id;
                }
                a = b;
            }
        }
        const size_t S = sets.size();
        std::vector<char> acc(S, 0), live(S, 0);
        for (size_t i = 0; i < S; i++) acc[i] = std::binary_search(sets[i].begin(), sets[i].end(), final_);
        // trim: keep the states that reach an accepting one
        std::vector<std::vector<int>> rev(S);
        for (size_t i = 0; i < S; i++) {
            int last = -1;
            for (int c = 0; c < 256; c++) {
                const int t = trans[i][c];
                if (t != (int)kGrammarDead && t != last) rev[t].push_back((int)i), last = t;
            }
        }
        std::vector<int> work;
        for (size_t i = 0; i < S; i++)
            if (acc[i]) live[i] = 1, work.push_back((int)i);
        while (!work.empty()) {
            const int s = work.back();
            work.pop_back();
            for (int p : rev[s])
                if (!live[p]) live[p] = 1, work.push_back(p);
        }
        if (!live[0]) throw SchemaError("json_schema: the schema accepts no document");
        std::vector<int> remap(S, -1);
        u32 nStates = 0;
        for (size_t i = 0; i < S; i++)
            if (live[i]) remap[i] = (int)nStates++;
        // classes: bytes with the same column, numbered in byte order
        auto g = std::make_shared<GrammarDfa>();
        std::map<std::vector<uint16_t>, int> classes;
        std::vector<std::vector<uint16_t>> columns;
        for (int c = 0; c < 256; c++) {
            std::vector<uint16_t> col;
            col.reserve(nStates);
            for (size_t i = 0; i < S; i++) {
                if (!live[i]) continue;
                const int t = trans[i][c];
                col.push_back(t == (int)kGrammarDead || !live[t] ? (uint16_t)kGrammarDead : (uint16_t)remap[t]);
            }
            auto it = classes.find(col);
            if (it == classes.end()) {
                it = classes.emplace(col, (int)columns.size()).first;
                columns.push_back(col);
            }
            g->classOf[c] = (u8)it->second;
        }
        g->nClasses = (u32)columns.size();
        g->nStates = nStates;
        g->start = 0;
        if ((size_t)nStates * g->nClasses > kGrammarMaxEntries)
            throw SchemaError("json_schema: the schema is too large: more than " + std::to_string(kGrammarMaxEntries) +
                              " table entries (" + std::to_string(nStates) + " states x " + std::to_string(g->nClasses) + " byte classes; cap)");
        g->next.resize((size_t)nStates * g->nClasses);
        for (u32 k = 0; k < g->nClasses; k++)
            for (u32 s = 0; s < nStates; s++) g->next[(size_t)s * g->nClasses + k] = columns[k][s];
        g->accept.assign((nStates + 31) / 32, 0);
        for (size_t i = 0; i < S; i++)
            if (live[i] && acc[i]) g->accept[remap[i] >> 5] |= 1u << (remap[i] & 31);
        const std::string bad = grammarCheck(*g);
        if (!bad.empty()) throw Error("json_schema: internal error: " + bad);
        if (vocab) {
            for (u32 s = 0; s < nStates; s++) {
                bool ok = vocab->eos && g->accepting(s);
                for (int c = 0; c < 256 && !ok; c++) ok = vocab->single[c] && g->stepByte(s, (u8)c) != kGrammarDead;
                if (!ok)
                    throw SchemaError("json_schema: dead end: this tokenizer has no single-byte token that continues state " +
                                      std::to_string(s) + " of the schema's automaton" + (g->accepting(s) ? " and no EOS token" : ""));
            }
        }
        return g;
    }
};

}  // namespace

std::shared_ptr<const GrammarDfa> compileSchemaDfa(const json::Value &schema, const GrammarVocab *vocab) {
    try {
        Compiler c(schema);
        return c.run(vocab);
    } catch (const SchemaError &) {
        throw;
    } catch (const Error &) {
        throw;
    } catch (const std::runtime_error &e) {  // json::Value accessors on a malformed schema
        throw SchemaError(std::string("json_schema: malformed schema: ") + e.what());
    }
}

std::shared_ptr<const GrammarDfa> SchemaDfaCache::get(const json::Value &schema, const GrammarVocab *vocab) {
    std::string key;
    serialise(schema, key);
    {
        std::lock_guard<std::mutex> lk(mu_);
        for (size_t i = 0; i < items_.size(); i++)
            if (items_[i].first == key) {
                auto hit = items_[i];
                items_.erase(items_.begin() + (long)i);
                items_.insert(items_.begin(), hit);
                hits_++;
                return hit.second;
            }
    }
    std::shared_ptr<const GrammarDfa> g = compileSchemaDfa(schema, vocab);  // (outside the lock: other schemas compile meanwhile)
    std::lock_guard<std::mutex> lk(mu_);
    for (auto &it : items_)
        if (it.first == key) return it.second;
    items_.insert(items_.begin(), std::make_pair(key, g));
    if (items_.size() > cap_) items_.pop_back();
    return g;
}

size_t SchemaDfaCache::size() const {
    std::lock_guard<std::mutex> lk(mu_);
    return items_.size();
}

}  // namespace dl
