// F16-weight GEMV kernel instances with 64 lanes per weight row (see f16w_inst.h).
#include "f16w_inst.h"

namespace dl {
namespace hipk {
const void *gemvF16wFnL64(int B, int pro, int epi) { return gemvF16wFnB<64>(B, pro, epi); }
}  // namespace hipk
}  // namespace dl
