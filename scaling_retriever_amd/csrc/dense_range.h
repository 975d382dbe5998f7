// Dense range search (dense_range.hip): every document whose exact score exceeds a per-query threshold, as CSR.
#pragma once
#include "common.h"
#include "range_scan.h"      // the (chunk, query) scan, shared with the sparse range search

#define SR_RANGE_MAX_CHUNKS 1024   // rows of the (chunk, query) table: 4 KiB per query at most

// One launch = one segment: grid (query tiles, chunks of the segment).  A chunk is chunk_rows consecutive rows (a multiple of 256; the
// segment's last chunk may be shorter), walked by ONE workgroup in ascending row order.
struct DenseRangeArgs {
    const void* D;            // segment base: rows of `dtype`
    const float* Q;           // [nq, H]
    const float* thr;         // [nq]
    int64_t seg_rows;         // rows of the segment
    int64_t chunk_rows;
    int chunk_base;           // table row of the segment's first chunk
    int H, nq;
    int dtype;                // SR_DTYPE_F32 | SR_DTYPE_F16
    int64_t id_base, id_stride;
    uint32_t* table;          // [n_chunks, nq]: count kernel writes the hits of (chunk, query); the scan turns them into exclusive prefixes over the chunks
    // fill only
    const int64_t* lims;      // [nq + 1]
    float* out_scores;
    int64_t* out_ids;
    int64_t capacity;
    // masked kernels only
    const uint32_t* mask;     // bitmap over global doc indices: bit (i & 31) of word i >> 5; read at id_base + row * id_stride of the segment's rows only
    // grouped kernels only: `mask` holds the groups' bitmaps stacked, mask_words words each
    const uint32_t* mask_qoff;    // [nq rounded up to 256] word offset of every query's own bitmap inside mask (0 past nq)
    const uint32_t* mask_union;   // [mask_words] the OR of the bitmaps of the groups that have a query: decides which tiles are skipped
    int64_t mask_words;           // words of one bitmap: nothing at or beyond them is read
};
// query tile: 256 wide for nq > 128, 128 wide below (as launch_dense_exact picks its pipelined kernels)
static inline int dense_range_query_tile(int64_t nq) { return nq > 128 ? 256 : 128; }
// a.mask null: the unrestricted kernels; else their masked twins (a hit needs its document's bit, a 256-row tile without a set bit is
// skipped); with a.mask_qoff too: the grouped twins (the bit of the query's own bitmap, a tile without a bit in the union is skipped)
int launch_dense_range_count(const DenseRangeArgs& a, int n_chunks_seg, hipStream_t s);
int launch_dense_range_fill(const DenseRangeArgs& a, int n_chunks_seg, hipStream_t s);
// the masked instantiations (dense_range_masked.hip); called by the two above, after their checks of the chunking
int launch_dense_range_count_masked(const DenseRangeArgs& a, int n_chunks_seg, hipStream_t s);
int launch_dense_range_fill_masked(const DenseRangeArgs& a, int n_chunks_seg, hipStream_t s);
// the grouped instantiations (dense_range_grouped.hip), likewise
int launch_dense_range_count_grouped(const DenseRangeArgs& a, int n_chunks_seg, hipStream_t s);
int launch_dense_range_fill_grouped(const DenseRangeArgs& a, int n_chunks_seg, hipStream_t s);
