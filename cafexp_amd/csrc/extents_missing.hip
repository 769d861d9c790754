// node_level_kernel for a table with missing cells (CAFE_COUNT_MISSING): the MISSING = true instantiation of extents_level.h and
// its launcher.  A translation unit of its own, so that extents.hip holds the kernels it held and nothing else.
#include "extents_level.h"

namespace cafe {

hipError_t launch_node_level_missing(const ExtArgs& a, dim3 grid, int per_block, hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(node_level_kernel<true>, grid, dim3(kLevelThreads), 0, stream, a, per_block);
    return hipGetLastError();
}

}  // namespace cafe
