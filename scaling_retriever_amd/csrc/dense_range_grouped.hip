// Dense range search under a document bitmap per query (gfx950, sr_dense_range_count_grouped / _fill_grouped): the GROUPED
// instantiations of dense_range_kernel.h - an object of its own, as dense_range_masked.hip is, so that the unrestricted and the masked
// kernels stay the instantiations they were.  A 256-row tile runs no k-loop when the union of the bitmaps of the groups that have a
// query is clear there (the masked kernels' wave-uniform ballot, read from a.mask_union); in the epilogue, behind the k-loop, a lane
// loads the word offset of its own query column (a.mask_qoff) and tests its hits against that bitmap: for stride-1 segments the 32 bits
// of each of the wave's four 32-row blocks, two words joined by a funnel shift where id_base is not a multiple of 32; for other strides
// the bit of each hit row.  Host side and contract: dense_range.hip.
#include "dense_range_kernel.h"

int launch_dense_range_count_grouped(const DenseRangeArgs& a, int n_chunks_seg, hipStream_t s) {
    SR_REQUIRE(a.mask && a.mask_qoff && a.mask_union, "dense range (grouped): the bitmaps, the queries' word offsets and the union are all needed");
    return launch_dense_range_m<false, RangeFilter::grouped>(a, n_chunks_seg, s);
}
int launch_dense_range_fill_grouped(const DenseRangeArgs& a, int n_chunks_seg, hipStream_t s) {
    SR_REQUIRE(a.mask && a.mask_qoff && a.mask_union, "dense range (grouped): the bitmaps, the queries' word offsets and the union are all needed");
    return launch_dense_range_m<true, RangeFilter::grouped>(a, n_chunks_seg, s);
}
