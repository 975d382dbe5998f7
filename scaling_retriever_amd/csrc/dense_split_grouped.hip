// The certified filter's upper-bound pass under a document bitmap per query (sr_dense_search_grouped): dense_split_kernel<true, true, true>
// (dense_split_kernel.h) in an object of its own, as dense_split_masked.hip is.  dense_split.o and dense_split_masked.o keep the
// instantiations they had; this one is judged against <true, true> (tests/test_grouped_mask_host.py reads both objects' metadata).
#include "dense_split_kernel.h"

int launch_dense_split_grouped(const DenseSplitArgs& a, unsigned grid, size_t lds, hipStream_t s) {
    SR_REQUIRE(a.upper_bound && a.mask && a.mask_qoff && a.n_pairs == 1, "dense_split(grouped): the upper-bound pass with per-query masks only");
    static DeviceOnce attr_once;
    SR_TRY(sr_allow_lds(attr_once, dense_split_kernel<true, true, true>, (int)lds));
    hipLaunchKernelGGL((dense_split_kernel<true, true, true>), dim3(grid), dim3(512), lds, s, a);
    SR_CHECK_LAUNCH();
    return SR_OK;
}
