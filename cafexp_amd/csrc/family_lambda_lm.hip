// cafe_score_per_family_lm: the per-family branch kernel under SEPARATE birth and death rates.  The body is the one of
// family_lambda_kernel.h, instantiated here on SlotParamLM (slot_param_lm(quantize(lambda), quantize(mu), quantize(t)); `zero`
// follows that function's rule); the host frame and the root kernel are family_lambda.hip's.  A translation unit of its own:
// the twelve widths of each rate model compile side by side, and `make check` reads the resources of each on its own.
#include "family_lambda_kernel.h"

namespace cafe {

template hipError_t launch_family_lambda<SlotParamLM>(const FamLamArgs<SlotParamLM>&, int, int64_t, int, hipStream_t);

}  // namespace cafe
