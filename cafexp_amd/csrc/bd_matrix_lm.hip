// K1 with separate birth and death rates: all transition matrices of one call under the linear birth-death process with
// birth rate lambda and death rate mu per lineage (cafe_set_death_rates and the _lm entries).  The body is K1's
// (bd_matrix_build.h; bd_matrix.hip has the derivation, the exchange identity of the k-major layout included), instantiated
// here on SlotParamLM: a translation unit of its own, so that the 36 kernels of each rate model compile side by side and
// `make check` reads the resources of each on its own.
#include "bd_matrix_build.h"

namespace cafe {

template hipError_t launch_bd_matrix_build<SlotParamLM>(const MatrixPool&, const SlotParamLM*, int, hipStream_t);
template hipError_t launch_bd_matrix_build_both<SlotParamLM>(const MatrixPool&, const MatrixPool&, const SlotParamLM*, const SlotParamLM*, int, int, hipStream_t);

}  // namespace cafe
