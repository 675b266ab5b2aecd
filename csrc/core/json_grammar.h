// JSON mode (`response_format: json_object`): the byte automaton behind the token mask, one
// definition for the host (jsonMaskHost, the CPU backend, the startup check) and the device
// (csrc/hip/json_mask.hip).
//
// jsonStep(state, byte) accepts exactly the byte strings that are prefixes of an RFC 8259 text with
//   - an object at the top level; after its closing `}` the state is DONE, which accepts no byte
//   - at most kJsonMaxWs whitespace bytes (0x20 0x09 0x0A 0x0D) in a row where the RFC allows them
//   - at most kJsonMaxDepth open containers (`{` and `[` reject at that depth)
//   - strings of bytes 0x20..0x7F other than `"` and `\`, the escapes \" \\ \/ \b \f \n \r \t and
//     \u + four hex digits (surrogate pairing unchecked), and well-formed UTF-8 (Unicode Table 3-7)
//   - numbers -?(0|[1-9][0-9]*)(\.[0-9]+)?([eE][+-]?[0-9]+)?, ended by the delimiter behind them
//   - the literals true, false and null; duplicate keys are allowed
// The state is 16 bytes per sequence; START is all zero bits.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DL_JSON_HD __host__ __device__ inline
#else
#define DL_JSON_HD inline
#endif

namespace dl {

constexpr int kJsonMaxWs = 8;
constexpr int kJsonMaxDepth = 64;

enum JsonLex : uint8_t {
    JL_START = 0,   // before the opening `{`
    JL_OBJ_OPEN,    // behind `{`: a key or `}`
    JL_KEY_NEXT,    // behind `,` in an object: a key
    JL_KEY,         // inside a key string
    JL_KEY_ESC,     // behind `\`
    JL_KEY_HEX,     // aux hex digits owed
    JL_KEY_UTF8,    // aux: continuation bytes owed | range of the next one << 2
    JL_COLON,       // behind a key: `:`
    JL_VALUE,       // behind `:` or behind `,` in an array: a value
    JL_ARR_OPEN,    // behind `[`: a value or `]`
    JL_STR,         // inside a value string (the four states as for keys)
    JL_STR_ESC,
    JL_STR_HEX,
    JL_STR_UTF8,
    JL_AFTER,       // behind a value: `,` or the closer of the innermost container
    JL_NUM_MINUS,   // behind `-`: a digit
    JL_NUM_ZERO,    // behind a leading 0
    JL_NUM_INT,     // inside the integer digits
    JL_NUM_DOT,     // behind `.`: a digit
    JL_NUM_FRAC,    // inside the fraction digits
    JL_NUM_E,       // behind e / E: a sign or a digit
    JL_NUM_ESIGN,   // behind the exponent's sign: a digit
    JL_NUM_EXP,     // inside the exponent digits
    JL_LIT,         // inside true / false / null: aux = literal << 4 | bytes seen
    JL_DONE,        // behind the top-level object's `}`
    JL_COUNT,
    JL_REJECT = 255
};

struct JsonState {
    uint8_t lex;    // JsonLex
    uint8_t aux;    // UTF-8 / hex digits owed, or the position inside a literal
    uint8_t ws;     // consecutive whitespace bytes
    uint8_t depth;  // open containers
    uint32_t pad;
    uint64_t stack;  // bit d: the container opened at depth d is an object (else an array)
};
static_assert(sizeof(JsonState) == 16, "JsonState is 16 bytes per sequence");

DL_JSON_HD JsonState jsonStart() { return JsonState{JL_START, 0, 0, 0, 0, 0}; }
DL_JSON_HD JsonState jsonReject() { return JsonState{JL_REJECT, 0, 0, 0, 0, 0}; }
DL_JSON_HD bool jsonRejected(const JsonState &s) { return s.lex == JL_REJECT; }
DL_JSON_HD bool jsonDone(const JsonState &s) { return s.lex == JL_DONE; }
DL_JSON_HD bool jsonSame(const JsonState &a, const JsonState &b) {
    return a.lex == b.lex && a.aux == b.aux && a.ws == b.ws && a.depth == b.depth && a.stack == b.stack;
}

DL_JSON_HD bool jsonIsWs(uint8_t c) { return c == 0x20 || c == 0x09 || c == 0x0A || c == 0x0D; }
DL_JSON_HD bool jsonIsDigit(uint8_t c) { return c >= '0' && c <= '9'; }
DL_JSON_HD bool jsonIsHex(uint8_t c) {
    return jsonIsDigit(c) || (c >= 'a' && c <= 'f') || (c >= 'A' && c <= 'F');
}

// the first byte of a value (not whitespace) in state s, whose lex and ws are already reset
DL_JSON_HD JsonState jsonValueStart(JsonState s, uint8_t c) {
    if (c == '"') {
        s.lex = JL_STR;
    } else if (c == '{' || c == '[') {
        if (s.depth >= kJsonMaxDepth) return jsonReject();
        const uint64_t bit = 1ull << s.depth;
        s.stack = c == '{' ? (s.stack | bit) : (s.stack & ~bit);
        s.depth++;
        s.lex = c == '{' ? JL_OBJ_OPEN : JL_ARR_OPEN;
    } else if (c == '-') {
        s.lex = JL_NUM_MINUS;
    } else if (c == '0') {
        s.lex = JL_NUM_ZERO;
    } else if (c >= '1' && c <= '9') {
        s.lex = JL_NUM_INT;
    } else if (c == 't' || c == 'f' || c == 'n') {
        s.lex = JL_LIT;
        s.aux = (uint8_t)((c == 't' ? 0 : c == 'f' ? 1 : 2) << 4 | 1);
    } else {
        return jsonReject();
    }
    return s;
}

// a byte behind a complete value (not whitespace): `,` or the closer of the innermost container
DL_JSON_HD JsonState jsonAfterValue(JsonState s, uint8_t c) {
    if (s.depth == 0) return jsonReject();
    const bool obj = (s.stack >> (s.depth - 1)) & 1ull;
    if (c == ',') {
        s.lex = obj ? JL_KEY_NEXT : JL_VALUE;
    } else if (c == (obj ? '}' : ']')) {
        s.depth--;
        s.lex = s.depth == 0 ? JL_DONE : JL_AFTER;
    } else {
        return jsonReject();
    }
    return s;
}

// a byte inside a string (the key's or the value's four states share their order)
DL_JSON_HD JsonState jsonStringByte(JsonState s, uint8_t c, bool key) {
    const uint8_t base = key ? JL_KEY : JL_STR;
    const int sub = s.lex - base;
    if (sub == 0) {  // plain
        if (c == '"') {
            s.lex = key ? JL_COLON : JL_AFTER;
        } else if (c == '\\') {
            s.lex = base + 1;
        } else if (c >= 0x20 && c <= 0x7F) {
        } else if (c >= 0xC2 && c <= 0xDF) {
            s.lex = base + 3, s.aux = 1;
        } else if (c >= 0xE0 && c <= 0xEF) {  // E0: A0..BF, ED: 80..9F
            s.lex = base + 3, s.aux = (uint8_t)(2 | (c == 0xE0 ? 1 : c == 0xED ? 2 : 0) << 2);
        } else if (c >= 0xF0 && c <= 0xF4) {  // F0: 90..BF, F4: 80..8F
            s.lex = base + 3, s.aux = (uint8_t)(3 | (c == 0xF0 ? 3 : c == 0xF4 ? 4 : 0) << 2);
        } else {
            return jsonReject();
        }
    } else if (sub == 1) {  // behind the backslash
        if (c == 'u') {
            s.lex = base + 2, s.aux = 4;
        } else if (c == '"' || c == '\\' || c == '/' || c == 'b' || c == 'f' || c == 'n' || c == 'r' || c == 't') {
            s.lex = base;
        } else {
            return jsonReject();
        }
    } else if (sub == 2) {  // hex digits
        if (!jsonIsHex(c)) return jsonReject();
        if (--s.aux == 0) s.lex = base;
    } else {  // continuation bytes
        const int range = s.aux >> 2;
        const uint8_t lo = range == 1 ? 0xA0 : range == 3 ? 0x90 : 0x80;
        const uint8_t hi = range == 2 ? 0x9F : range == 4 ? 0x8F : 0xBF;
        if (c < lo || c > hi) return jsonReject();
        s.aux = (uint8_t)((s.aux & 3) - 1);
        if (s.aux == 0) s.lex = base;
    }
    return s;
}

// byte `at` of true / false / null (their bytes packed little-endian), 0 behind the last one
DL_JSON_HD uint8_t jsonLiteralByte(int which, int at) {
    const uint64_t lit = which == 0 ? 0x65757274ull : which == 1 ? 0x65736c6166ull : 0x6c6c756eull;
    return (uint8_t)(lit >> (8 * at));
}

DL_JSON_HD JsonState jsonStep(JsonState s, uint8_t c) {
    const uint8_t lex = s.lex;
    if (lex >= JL_DONE) return jsonReject();  // DONE accepts nothing, REJECT stays
    if (lex >= JL_KEY && lex <= JL_KEY_UTF8) return jsonStringByte(s, c, true);
    if (lex >= JL_STR && lex <= JL_STR_UTF8) return jsonStringByte(s, c, false);
    if (lex == JL_LIT) {
        const int which = s.aux >> 4, at = s.aux & 15;
        if (c != jsonLiteralByte(which, at)) return jsonReject();
        if (jsonLiteralByte(which, at + 1) == 0)
            s.lex = JL_AFTER, s.aux = 0;
        else
            s.aux++;
        return s;
    }
    if (lex >= JL_NUM_MINUS && lex <= JL_NUM_EXP) {
        const bool d = jsonIsDigit(c);
        switch (lex) {
        case JL_NUM_MINUS:
            if (!d) return jsonReject();
            s.lex = c == '0' ? JL_NUM_ZERO : JL_NUM_INT;
            return s;
        case JL_NUM_DOT:
            if (!d) return jsonReject();
            s.lex = JL_NUM_FRAC;
            return s;
        case JL_NUM_E:
            if (c == '+' || c == '-') {
                s.lex = JL_NUM_ESIGN;
                return s;
            }
            // fall through
        case JL_NUM_ESIGN:
            if (!d) return jsonReject();
            s.lex = JL_NUM_EXP;
            return s;
        default:
            break;
        }
        // ZERO, INT, FRAC, EXP: a complete number
        if (d) return lex == JL_NUM_ZERO ? jsonReject() : s;
        if (c == '.' && (lex == JL_NUM_ZERO || lex == JL_NUM_INT)) {
            s.lex = JL_NUM_DOT;
            return s;
        }
        if ((c == 'e' || c == 'E') && lex != JL_NUM_EXP) {
            s.lex = JL_NUM_E;
            return s;
        }
        s.lex = JL_AFTER;  // the delimiter behind the number
        if (jsonIsWs(c)) {
            s.ws = 1;
            return s;
        }
        return jsonAfterValue(s, c);
    }
    // between tokens: whitespace is allowed, and counted
    if (jsonIsWs(c)) {
        if (s.ws >= kJsonMaxWs) return jsonReject();
        s.ws++;
        return s;
    }
    s.ws = 0;
    switch (lex) {
    case JL_START:
        if (c != '{') return jsonReject();
        return jsonValueStart(s, c);
    case JL_OBJ_OPEN:
        if (c == '}') {
            s.lex = JL_AFTER;  // (an empty object: close it as behind a value)
            return jsonAfterValue(s, c);
        }
        // fall through
    case JL_KEY_NEXT:
        if (c != '"') return jsonReject();
        s.lex = JL_KEY;
        return s;
    case JL_COLON:
        if (c != ':') return jsonReject();
        s.lex = JL_VALUE;
        return s;
    case JL_ARR_OPEN:
        if (c == ']') {
            s.lex = JL_AFTER;
            return jsonAfterValue(s, c);
        }
        // fall through
    case JL_VALUE:
        return jsonValueStart(s, c);
    case JL_AFTER:
        return jsonAfterValue(s, c);
    default:
        return jsonReject();
    }
}

// Token classes of the mask's table.
enum JsonTokenClass : uint32_t { JT_REGULAR = 0, JT_EOS = 1, JT_BANNED = 2 };

// A token's table entry: `off` is the index of its first 4-byte word in the table's words (the
// piece's bytes, little-endian, zero-padded to whole words), info = length in bytes | class << 16.
DL_JSON_HD uint32_t jsonTokenLen(uint32_t info) { return info & 0xffffu; }
DL_JSON_HD uint32_t jsonTokenClass(uint32_t info) { return info >> 16; }

// The state behind the token's bytes, REJECT when the token is not allowed in s: a regular piece of
// at least one byte none of whose bytes rejects (a byte behind DONE rejects), or an EOS in DONE
// (which stays DONE).
DL_JSON_HD JsonState jsonStepToken(JsonState s, const uint32_t *words, uint32_t off, uint32_t info) {
    const uint32_t cls = jsonTokenClass(info), len = jsonTokenLen(info);
    if (cls == JT_EOS) return s.lex == JL_DONE ? s : jsonReject();
    if (cls != JT_REGULAR || len == 0) return jsonReject();
    uint32_t w = 0;
    for (uint32_t i = 0; i < len; i++) {
        if ((i & 3u) == 0) w = words[off + (i >> 2)];
        s = jsonStep(s, (uint8_t)(w & 0xffu));
        if (s.lex == JL_REJECT) return s;
        w >>= 8;
    }
    return s;
}

}  // namespace dl
