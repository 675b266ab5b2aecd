// F16-weight GEMV kernel instances with 16 lanes per weight row (see f16w_inst.h).
#include "f16w_inst.h"

namespace dl {
namespace hipk {
const void *gemvF16wFnL16(int B, int pro, int epi) { return gemvF16wFnB<16>(B, pro, epi); }
}  // namespace hipk
}  // namespace dl
