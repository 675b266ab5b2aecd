// Q80-weight GEMV kernel instances with 64 lanes per weight row (see q80w_inst.h).
#include "q80w_inst.h"

namespace dl {
namespace hipk {
const void *gemvQ80wFnL64(int B, int pro, int epi) { return gemvQ80wFnB<64>(B, pro, epi); }
const void *gemvQ80wDepthFnL64(int depth) { return gemvQ80wDepthFn<64>(depth); }
}  // namespace hipk
}  // namespace dl
