// What a forward's graph is captured for, and the key the engine's graph cache files it under.
// Plain C++ (no HIP): the native unit tests include it.
#pragma once

#include <cstdint>

#include "../core/common.h"

namespace dl {
namespace engine_detail {

// What follows the layers of a forward:
//   LOGITS  the logits, for the host          ARGMAX  the rows' argmax
//   CHAIN   ARGMAX that feeds the token back  SAMPLE  the sampler's draw per row
//   EMBED   every row is a non-drawing row and one of them is pooled (Backend::setPooling): all the
//           layers, then launchPool on the root; no wcls, no logits exchange, no token pick on any rank
enum class GraphKind : unsigned { LOGITS = 0, ARGMAX = 1, CHAIN = 2, SAMPLE = 3, EMBED = 4 };
constexpr unsigned kGraphKinds = 5;

// The optional stages between the logits and the ids of a SAMPLE forward, a bit each (the root rank
// of a forward with an active LogitProc row; every other forward has none):
//   PROC     the logit processors ahead of the draw, the drawn tokens counted behind it
//   FILTER   the candidate filter (top_k / min_p) of a forward with a row whose filter is on
//   JSON     the JSON token mask and the automaton's advance (a drawn row in JSON mode)
//   GRAMMAR  the grammar token mask and advance (a drawn row that follows a compiled schema)
// FILTER, JSON and GRAMMAR work on the processed rows, so each implies PROC.
enum DrawStage : unsigned { PROC = 1, FILTER = 2, JSON = 4, GRAMMAR = 8 };
constexpr unsigned kDrawStageSets = 16;

// The fields a captured graph depends on, low bits first, each with its width.
struct GraphKeyFields {
    unsigned bucket = 0;     // index of the context bucket
    bool attnLong = false;   // decode attention runs the MFMA kernel
    bool prefillOk = false;  // the rows qualify for the MFMA prefill attention
    unsigned stages = 0;     // DrawStage bits
    GraphKind kind = GraphKind::LOGITS;
    unsigned rows = 0;
};
using GraphKey = uint32_t;
constexpr unsigned kKeyBucketBits = 4, kKeyStageBits = 4, kKeyKindBits = 3, kKeyRowBits = 14;
constexpr unsigned kKeyStageShift = kKeyBucketBits + 2, kKeyKindShift = kKeyStageShift + kKeyStageBits,
                   kKeyRowShift = kKeyKindShift + kKeyKindBits;
constexpr unsigned kKeyMaxBucket = (1u << kKeyBucketBits) - 1, kKeyMaxRows = (1u << kKeyRowBits) - 1;
static_assert(kKeyRowShift + kKeyRowBits <= 32, "the fields fit the key");
static_assert(kGraphKinds <= 1u << kKeyKindBits && kDrawStageSets == 1u << kKeyStageBits, "kinds and stage sets fit their fields");

// Throws when a value does not fit its field: a wider value would alias another forward's graph.
constexpr GraphKey graphKey(const GraphKeyFields &f) {
    DL_CHECK(f.bucket <= kKeyMaxBucket, "graph key: bucket index");
    DL_CHECK(f.stages < kDrawStageSets, "graph key: draw stages");
    DL_CHECK((unsigned)f.kind < kGraphKinds, "graph key: kind");
    DL_CHECK(f.rows <= kKeyMaxRows, "graph key: rows");
    return f.bucket | (f.attnLong ? 1u : 0u) << kKeyBucketBits | (f.prefillOk ? 1u : 0u) << (kKeyBucketBits + 1) |
           f.stages << kKeyStageShift | (unsigned)f.kind << kKeyKindShift | f.rows << kKeyRowShift;
}

constexpr GraphKeyFields graphKeyFields(GraphKey k) {
    GraphKeyFields f;
    f.bucket = k & kKeyMaxBucket;
    f.attnLong = (k >> kKeyBucketBits & 1u) != 0;
    f.prefillOk = (k >> (kKeyBucketBits + 1) & 1u) != 0;
    f.stages = k >> kKeyStageShift & (kDrawStageSets - 1);
    f.kind = (GraphKind)(k >> kKeyKindShift & ((1u << kKeyKindBits) - 1));
    f.rows = k >> kKeyRowShift;
    return f;
}

}  // namespace engine_detail
}  // namespace dl
