// Structured outputs: a JSON schema (OpenAI's strict subset) compiled into a byte DFA (grammar_dfa.h).
//
// The accepted language is the compact serialisation of a JSON value that satisfies the schema: one
// optional 0x20 behind every `:` and every `,` and no other whitespace; object members in the order
// of `properties`, each exactly once; strings, numbers and literals by the byte rules of
// json_grammar.h (well-formed UTF-8, the RFC escapes, \u + 4 hex digits, the RFC number grammar;
// `integer` is -?(0|[1-9][0-9]*)).
//
// Supported: a top level of type object; `type` (one of the seven names or a list of them);
// `properties` with `required` naming every property and `additionalProperties` absent or false;
// `items` (required for arrays) with `minItems` / `maxItems` in 0..16 (no maxItems: unbounded);
// `enum` / `const` over scalars, one spelling each (strings with `"` and `\` escaped, control bytes
// as \u00XX, everything else raw UTF-8; numbers as the schema's text spells them); `anyOf`; `$ref`
// to #/$defs/NAME, expanded inline; `minLength` / `maxLength` in code points (an escape counts as
// one), at most 64. `title`, `description`, `default`, `examples`, `$schema` and `$defs` are
// ignored. Every other keyword, additionalProperties true, a property missing from `required`, an
// object without `properties`, a schema that constrains nothing, a recursive `$ref` and a top level
// that is not an object are refused with a SchemaError that names the keyword or the reason.
//
// Construction: byte-level NFA fragments (Thompson, with epsilon edges), subset construction in
// byte order from the start state, states that cannot reach an accepting state trimmed (so an
// allowed token always leaves the text a prefix of a valid document), bytes that behave the same in
// every state merged into classes in byte order. Every step is a function of the schema alone: the
// same schema gives the same table bytes.
//
// Caps, enforced while constructing (a hostile schema fails in bounded work):
//   kSchemaMaxNfaStates  NFA states (checked at every state a fragment adds)
//   kGrammarMaxStates    DFA states (checked at every state the subset construction adds)
//   kGrammarMaxEntries   table entries nStates * nClasses (checked once the classes are known)
// These are policy limits, not measured optima.
#pragma once

#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../net/json.h"
#include "common.h"
#include "grammar_dfa.h"

namespace dl {

constexpr uint32_t kSchemaMaxNfaStates = 32768;
constexpr int kSchemaMaxItems = 16;
constexpr int kSchemaMaxLength = 64;

// A schema that cannot be served; the API answers 400 with the message.
class SchemaError : public Error {
  public:
    using Error::Error;
};

// What the dead-end check needs of the vocabulary: which byte values exist as single-byte regular
// tokens, and whether there is an EOS token.
struct GrammarVocab {
    bool single[256] = {false};
    bool eos = false;
};
GrammarVocab makeGrammarVocab(const std::vector<uint32_t> &off, const std::vector<uint32_t> &info, const std::vector<uint32_t> &words);

// Compiles `schema` (the `schema` member of `json_schema`). With a vocabulary, every state must have
// a live transition on a single-byte regular token, or accept with an EOS available; a schema with
// a state that has neither is refused (the draw could be left without any token there).
std::shared_ptr<const GrammarDfa> compileSchemaDfa(const json::Value &schema, const GrammarVocab *vocab);

// LRU cache of compiled grammars keyed by the schema's serialised text (thread-safe: the HTTP
// handler threads compile). Failures are not cached.
class SchemaDfaCache {
  public:
    explicit SchemaDfaCache(size_t capacity = 32) : cap_(capacity) {}
    std::shared_ptr<const GrammarDfa> get(const json::Value &schema, const GrammarVocab *vocab);
    size_t size() const;
    u64 hits() const { return hits_; }

  private:
    size_t cap_;
    mutable std::mutex mu_;
    std::vector<std::pair<std::string, std::shared_ptr<const GrammarDfa>>> items_;  // most recent first
    u64 hits_ = 0;
};

}  // namespace dl
