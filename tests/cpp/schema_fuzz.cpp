// Stand-alone check of the schema compiler (csrc/core/schema_dfa.cpp) under the host sanitizers:
// `make schema-fuzz` builds this file and the compiler with -fsanitize=address,undefined and runs
// it. The compiler parses text from the network, so it is fed a set of schemas and a fixed-seed
// set of mutations of their text (bytes flipped, dropped and doubled, keywords and numbers
// swapped); whatever compiles is checked (grammarCheck) and walked by a few documents and tokens.
// Host code only: no GPU, no Python.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../csrc/core/schema_dfa.h"

using namespace dl;

static const char *const kSchemas[] = {
    R"({"type":"object","properties":{"s":{"type":"string"},"n":{"type":"number"},"i":{"type":"integer"},"b":{"type":"boolean"},"z":{"type":"null"}},"required":["s","n","i","b","z"],"additionalProperties":false})",
    R"({"type":"object","properties":{"a":{"type":"object","properties":{"b":{"type":"object","properties":{},"required":[]}},"required":["b"]}},"required":["a"]})",
    R"({"type":"object","properties":{"l":{"type":"array","items":{"type":"object","properties":{"x":{"type":"integer"}},"required":["x"]},"minItems":1,"maxItems":3}},"required":["l"]})",
    R"({"type":"object","properties":{"e":{"enum":["say \"hi\"\\","\u00e9\n",1,2.50,-3e2,true,null]},"c":{"const":"k"}},"required":["e","c"]})",
    R"({"type":"object","properties":{"v":{"anyOf":[{"type":"integer"},{"type":"string","maxLength":2},{"type":"array","items":{"type":"null"},"maxItems":2}]}},"required":["v"]})",
    R"({"type":"object","properties":{"v":{"type":["string","null"]},"w":{"type":["integer","boolean"]}},"required":["v","w"]})",
    R"({"$defs":{"p":{"type":"object","properties":{"x":{"type":"number"},"y":{"type":"number"}},"required":["x","y"]}},"type":"object","properties":{"a":{"$ref":"#/$defs/p"},"b":{"$ref":"#/$defs/p"}},"required":["a","b"]})",
    R"({"type":"object","properties":{"s":{"type":"string","minLength":2,"maxLength":4}},"required":["s"]})",
    R"({"type":"object","properties":{"l":{"type":"array","items":{"type":"boolean"},"minItems":2}},"required":["l"]})",
    R"({"$defs":{"r":{"type":"object","properties":{"r":{"$ref":"#/$defs/r"}},"required":["r"]}},"type":"object","properties":{"r":{"$ref":"#/$defs/r"}},"required":["r"]})",
    R"({"type":"object","properties":{"a":{"type":"array","maxItems":16,"items":{"anyOf":[{"type":"array","maxItems":16,"items":{"anyOf":[{"type":"array","maxItems":16,"items":{"type":"string","maxLength":64}},{"type":"integer"}]}},{"type":"number"}]}}},"required":["a"]})",
    R"({"type":"object","properties":{"s":{"type":"string","pattern":"^a"}},"required":["s"]})",
};

static const char *const kSwaps[] = {"type",   "properties", "required", "items",    "minItems", "maxItems", "enum",     "const", "anyOf",
                                     "$ref",   "$defs",      "object",   "array",    "string",   "integer",  "number",   "null",  "boolean",
                                     "oneOf",  "minLength",  "maxLength", "additionalProperties", "true", "false", "16", "17", "-1", "0", "64", "65", "1e99", "{}", "[]"};

static uint32_t rngState = 20240607u;
static uint32_t rnd() {
    rngState = rngState * 1664525u + 1013904223u;
    return rngState >> 8;
}

static std::string mutate(std::string s) {
    const int edits = 1 + (int)(rnd() % 3);
    for (int e = 0; e < edits && !s.empty(); e++) {
        const size_t at = rnd() % s.size();
        switch (rnd() % 5) {
        case 0: s[at] = (char)(rnd() & 0xff); break;
        case 1: s.erase(at, 1 + rnd() % 4); break;
        case 2: s.insert(at, s.substr(at, 1 + rnd() % 8)); break;
        case 3: {  // one quoted word or number for another
            const std::string a = kSwaps[rnd() % (sizeof(kSwaps) / sizeof(kSwaps[0]))], b = kSwaps[rnd() % (sizeof(kSwaps) / sizeof(kSwaps[0]))];
            const size_t p = s.find(a);
            if (p != std::string::npos) s.replace(p, a.size(), b);
            break;
        }
        default: s.insert(at, 1, "{}[]\",:\\0-9e.u"[rnd() % 15]); break;
        }
    }
    return s;
}

static int compiled = 0, refused = 0, unparsed = 0;

static void exercise(const GrammarDfa &g) {
    const std::string bad = grammarCheck(g);
    if (!bad.empty()) {
        std::fprintf(stderr, "schema_fuzz: the compiler returned malformed tables: %s\n", bad.c_str());
        std::exit(1);
    }
    // random documents: at every step a byte with a live transition when there is one
    for (int doc = 0; doc < 4; doc++) {
        uint32_t s = g.start;
        for (int i = 0; i < 200; i++) {
            const uint8_t first = (uint8_t)rnd();
            uint32_t n = kGrammarDead;
            for (int k = 0; k < 256 && n == kGrammarDead; k++) n = g.stepByte(s, (uint8_t)(first + k));
            if (n == kGrammarDead) {
                if (!g.accepting(s)) {
                    std::fprintf(stderr, "schema_fuzz: state %u neither continues nor accepts\n", s);
                    std::exit(1);
                }
                break;
            }
            s = n;
        }
    }
    // tokens through grammarStepToken: two words of bytes, every length, every class
    const GrammarView v = g.view();
    for (int t = 0; t < 64; t++) {
        const uint32_t words[2] = {rnd() | rnd() << 24, rnd() | rnd() << 24};
        const uint32_t info = (rnd() % 9) | (rnd() % 3) << 16;
        (void)grammarStepToken(v, rnd() % (g.nStates + 1), words, 0, info);
    }
}

static void feed(const std::string &text, const GrammarVocab *vocab) {
    json::Value schema;
    try {
        schema = json::Value::parse(text);
    } catch (const std::exception &) {
        unparsed++;
        return;
    }
    try {
        const std::shared_ptr<const GrammarDfa> g = compileSchemaDfa(schema, vocab);
        compiled++;
        exercise(*g);
    } catch (const SchemaError &) {
        refused++;
    }
}

int main() {
    GrammarVocab all, noQuote;
    for (int c = 0; c < 256; c++) all.single[c] = noQuote.single[c] = true;
    all.eos = noQuote.eos = true;
    noQuote.single['"'] = false;
    SchemaDfaCache cache(4);
    for (const char *text : kSchemas) {
        feed(text, nullptr);
        feed(text, &all);
        feed(text, &noQuote);
        try {  // the cache, over its capacity
            const json::Value v = json::Value::parse(text);
            if (cache.get(v, &all) != cache.get(v, &all)) {
                std::fprintf(stderr, "schema_fuzz: the cache compiled one schema twice\n");
                return 1;
            }
        } catch (const SchemaError &) {
        }
        for (int m = 0; m < 120; m++) feed(mutate(text), (m & 1) ? &all : nullptr);
    }
    std::printf("schema_fuzz: %d compiled, %d refused, %d not JSON\n", compiled, refused, unparsed);
    if (compiled < 20 || refused < 20) {
        std::fprintf(stderr, "schema_fuzz: the mutations exercised too little\n");
        return 1;
    }
    return 0;
}
