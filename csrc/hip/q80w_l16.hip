// Q80-weight GEMV kernel instances with 16 lanes per weight row (see q80w_inst.h).
#include "q80w_inst.h"

namespace dl {
namespace hipk {
const void *gemvQ80wFnL16(int B, int pro, int epi) { return gemvQ80wFnB<16>(B, pro, epi); }
const void *gemvQ80wDepthFnL16(int depth) { return gemvQ80wDepthFn<16>(depth); }
}  // namespace hipk
}  // namespace dl
