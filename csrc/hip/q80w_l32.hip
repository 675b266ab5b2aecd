// Q80-weight GEMV kernel instances with 32 lanes per weight row (see q80w_inst.h).
#include "q80w_inst.h"

namespace dl {
namespace hipk {
const void *gemvQ80wFnL32(int B, int pro, int epi) { return gemvQ80wFnB<32>(B, pro, epi); }
const void *gemvQ80wDepthFnL32(int depth) { return gemvQ80wDepthFn<32>(depth); }
}  // namespace hipk
}  // namespace dl
