// The scan both range searches share (dense_range.hip holds the kernels): a [n_chunks, nq] table of 32-bit hit counts per (chunk of
// documents, query) becomes, in place, exclusive prefixes over the chunks, and the per-query totals become lims.  Any number of chunks
// (the dense head uses at most SR_RANGE_MAX_CHUNKS, the sparse head one per doc tile: 1 080 at 8.84 M documents) and any nq; a
// query's total is below 2^32.
#pragma once
#include "common.h"

// table[c][q] := sum of table[c'][q] over c' < c (in place); lims[0] = 0, lims[q + 1] = hits of queries 0..q
int launch_range_scan(uint32_t* table, int n_chunks, int64_t nq, int64_t* d_lims, hipStream_t s);
