// The certified filter's upper-bound pass under a document mask: dense_split_kernel<true, true> (dense_split_kernel.h) in an object of
// its own.  dense_split.o keeps exactly the two unmasked instantiations it had, with the registers they had; this one is judged
// against <true, false> (tools/kernel_meta.sh on both objects).
#include "dense_split_kernel.h"

int launch_dense_split_masked(const DenseSplitArgs& a, unsigned grid, size_t lds, hipStream_t s) {
    SR_REQUIRE(a.upper_bound && a.mask && a.n_pairs == 1, "dense_split(masked): the upper-bound pass with a mask only");
    static DeviceOnce attr_once;
    SR_TRY(sr_allow_lds(attr_once, dense_split_kernel<true, true>, (int)lds));
    hipLaunchKernelGGL((dense_split_kernel<true, true>), dim3(grid), dim3(512), lds, s, a);
    SR_CHECK_LAUNCH();
    return SR_OK;
}
