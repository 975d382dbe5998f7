// Exact fp32 MFMA scorer for batches of more than 64 queries, and for any batch in the batch-invariant mode (dense_score.hip).
#pragma once
#include "common.h"
struct DenseArgs {
    const void* D;        // segment base: rows of `dtype`
    const float* Q;
    int64_t row_begin;    // first doc row of this launch (within the segment)
    int64_t row_end;      // one past the last doc row of this launch
    int H;
    int nq;
    const float* tau;
    uint64_t* cand_keys;
    int* cand_count;
    int64_t cand_cap;
    uint32_t id_base, id_stride;
    int dtype;            // SR_DTYPE_F32 | SR_DTYPE_F16: how the rows are stored (the launch picks the instantiation)
};
// queries per workgroup of the kernel that serves a batch of nq (the 16-bit passes of dense_split.hip cut their batches the same way)
static inline int dense_query_tile(int64_t nq) { return nq > 128 ? 256 : (nq > 64 ? 128 : (nq > 32 ? 64 : 32)); }
// one launch over `rows` = a.row_end - a.row_begin docs, 256 per workgroup; plain: the double-buffered kernel where the pipelined one is the default
int launch_dense_exact(const DenseArgs& a, int64_t rows, bool plain, hipStream_t s);
