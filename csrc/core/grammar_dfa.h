// Structured outputs (`response_format: json_schema`): the table-driven byte DFA behind the token
// mask, one walk for the host (grammarMaskHost, the CPU backend, the compiler's checks) and the
// device (csrc/hip/grammar_mask.hip). csrc/core/schema_dfa.h compiles a schema into a GrammarDfa.
//
// A DFA is: classOf[256] (byte -> class), next[nStates][nClasses] (u16, kGrammarDead = no
// transition), the start state and one accept bit per state. A sequence's state is one u32. Every
// entry of next is < nStates or kGrammarDead (grammarCheck), so a walk never leaves the tables.
#pragma once

#include <stdint.h>

#include <string>
#include <vector>

#include "json_grammar.h"

namespace dl {

constexpr uint32_t kGrammarDead = 0xFFFFu;           // next[]: no transition
constexpr uint32_t kGrammarReject = 0xFFFFFFFFu;     // grammarStepToken: the token is not allowed
constexpr uint32_t kGrammarMaxStates = 4096;
constexpr uint32_t kGrammarMaxEntries = 131072;      // nStates * nClasses: 256 KB of u16

// What a walk needs of a DFA. The device mask kernel has a view of its own that answers the
// current state's row and the class map from LDS (grammar_mask.hip); this one reads the arrays.
struct GrammarView {
    const uint8_t *classOf = nullptr;  // [256]
    const uint16_t *next = nullptr;    // [nStates][nClasses]
    const uint32_t *accept = nullptr;  // [(nStates + 31) / 32] bit s: state s accepts
    uint32_t nClasses = 0, nStates = 0;
    DL_JSON_HD uint32_t cls(uint8_t c) const { return classOf[c]; }
    // (a state outside the tables has no transitions: a walk never indexes past them)
    DL_JSON_HD uint32_t step(uint32_t s, uint32_t k) const { return s < nStates ? next[s * nClasses + k] : kGrammarDead; }
    DL_JSON_HD bool accepting(uint32_t s) const { return (accept[s >> 5] >> (s & 31u)) & 1u; }
    DL_JSON_HD uint32_t states() const { return nStates; }
};

// The state behind the token's bytes, kGrammarReject when the token is not allowed in `state`: a
// regular piece of at least one byte none of whose bytes reaches the dead state, or an EOS in an
// accepting state (which stays where it is). Every other special token, the empty piece and a state
// outside the DFA reject. The token table is JSON mode's (JsonTokenTable).
template <class View>
DL_JSON_HD uint32_t grammarStepToken(const View &v, uint32_t state, const uint32_t *words, uint32_t off, uint32_t info) {
    if (state >= v.states()) return kGrammarReject;
    const uint32_t cls = jsonTokenClass(info), len = jsonTokenLen(info);
    if (cls == JT_EOS) return v.accepting(state) ? state : kGrammarReject;
    if (cls != JT_REGULAR || len == 0) return kGrammarReject;
    uint32_t w = 0;
    for (uint32_t i = 0; i < len; i++) {
        if ((i & 3u) == 0) w = words[off + (i >> 2)];
        state = v.step(state, v.cls((uint8_t)(w & 0xffu)));
        if (state == kGrammarDead) return kGrammarReject;
        w >>= 8;
    }
    return state;
}

// A compiled grammar (host). Immutable once built; shared between the requests of one schema.
struct GrammarDfa {
    uint8_t classOf[256] = {0};
    uint32_t nClasses = 0, nStates = 0, start = 0;
    std::vector<uint16_t> next;    // [nStates * nClasses]
    std::vector<uint32_t> accept;  // [(nStates + 31) / 32]
    GrammarView view() const {
        GrammarView v;
        v.classOf = classOf;
        v.next = next.data();
        v.accept = accept.data();
        v.nClasses = nClasses;
        v.nStates = nStates;
        return v;
    }
    bool accepting(uint32_t s) const { return s < nStates && ((accept[s >> 5] >> (s & 31u)) & 1u); }
    // the state behind byte c, kGrammarDead when there is none
    uint32_t stepByte(uint32_t s, uint8_t c) const { return s < nStates ? next[(size_t)s * nClasses + classOf[c]] : kGrammarDead; }
    // the table bytes in the order classOf, next, accept (the determinism tests compare them)
    std::string tableBytes() const;
};

// Empty when the tables are well formed (1 <= nClasses <= 256, 1 <= nStates <= kGrammarMaxStates,
// nStates * nClasses <= kGrammarMaxEntries, the vectors' sizes, classOf < nClasses, start < nStates,
// every entry of next < nStates or kGrammarDead, no accept bit behind nStates), else what is wrong.
std::string grammarCheck(const GrammarDfa &g);

}  // namespace dl
