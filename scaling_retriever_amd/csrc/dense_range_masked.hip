// Dense range search under a document bitmap (gfx950): the MASKED instantiations of dense_range_kernel.h - a hit also needs the bit of
// its document's global index, and a 256-row tile whose bits are all clear runs no k-loop.  Host side and contract: dense_range.hip.
#include "dense_range_kernel.h"

int launch_dense_range_count_masked(const DenseRangeArgs& a, int n_chunks_seg, hipStream_t s) { return launch_dense_range_m<false, RangeFilter::masked>(a, n_chunks_seg, s); }
int launch_dense_range_fill_masked(const DenseRangeArgs& a, int n_chunks_seg, hipStream_t s) { return launch_dense_range_m<true, RangeFilter::masked>(a, n_chunks_seg, s); }
