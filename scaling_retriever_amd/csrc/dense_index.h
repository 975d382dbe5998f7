// The dense index handle and what its parts share (internal): dense_index.hip owns the handle and the segments' preparation,
// dense_search.hip the search pass and the certified filter's orchestration, dense_restrict.hip pair scoring and the subset / masked /
// grouped searches, dense_range.hip the range search.
#pragma once
#include "common.h"
#include "pair_score.h"
#include <mutex>
#include <vector>

struct DenseSegment {
    const void* rows;                   // caller's rows, fp32 or binary16 (sr_dense_index::row_dtype): never copied, never widened
    int64_t n;
    int64_t id_base, id_stride;
    DeviceBuf<unsigned short> pl[3];    // library-owned bf16 planes (bf16x3 / bf16x6 score modes only)
    int n_planes = 0;
    // certified filter (SR_PRECISION_FP32_FILTERED, dense_filter.hip): fp16 plane of the rows scaled by fsd (a power of two)
    // and the per-document error terms (x, y); f_state: 0 = not built, 1 = ready, -1 = cannot be filtered (non-finite or
    // out-of-range values, no memory)
    DeviceBuf<unsigned short> fpl;
    DeviceBuf<float> fxy;               // [n, 2], then [ceil(n / 128), 2]: the maxima of x and of y over every group of 128 documents
    float fsd = 1.f, fisd = 1.f;
    float fx_max = 0.f, fy_max = 0.f;   // the largest x and y of the segment (scaled domain): the second threshold's e_max (dense_filter.h)
    int f_state = 0;
};
// bytes of DenseSegment::fxy for a segment of n rows
static inline size_t filter_xy_bytes(int64_t n) { return (size_t)(n + ceil_div64(n, 128)) * 8; }

struct sr_dense_index {
    int dim = 0;
    std::vector<DenseSegment> segs;
    int64_t ntotal = 0;
    int64_t ws_limit = 4ll << 30;
    int precision = SR_PRECISION_FP32;
    int row_dtype = SR_DTYPE_F32;          // SR_DTYPE_F32 | SR_DTYPE_F16: decided by the first non-empty add, then fixed
    bool batch_invariant = false;          // sr_dense_index_set_batch_invariant: batches <= 64 run the tiled kernels (one k order)
    DeviceBuf<unsigned short> qpl[3];      // query planes for the split precisions, [nq, dim] each
    TopkWS ws;
    StreamOrder order;
    LaunchProfile prof;
    std::mutex mu;
    // SR_PRECISION_FP32_FILTERED (dense_filter.hip)
    TopkWS wsf;                       // the 16-bit passes (upper-bound pass, bf16x3 / bf16x6): segmented candidate slots - a workspace of
                                      // its own, so an index that alternates pass kinds does not free and re-allocate GBs per search
    TopkWS ws2;                       // exact top-k over the re-scored candidates
    TopkWS ws3;                       // exact re-do of the queries without a certificate
    DeviceBuf<float> qa;              // [fq_cap, 4] per query (A', B', sq, 1 / sq), then 3 x [fq_cap]: slack, tau2, tau_eff (dense_filter.h)
    DeviceBuf<float> a_scores;        // [fq_cap, fkp] the kp largest upper bounds U, sorted
    DeviceBuf<int64_t> a_ids;
    DeviceBuf<int> flags;             // [2 fq_cap + 2]: per-query flags, then the xmin scratch of the re-score
    int64_t fq_cap = 0;               // what the four lists above were sized for: queries, candidates per query
    int fkp = 0;
    DeviceBuf<unsigned int> f_scratch;    // [2]: absmax bits, bad flag (segment preparation)
    // queries the certificate could not be given for are re-done by the exact kernel, those alone
    DeviceBuf<float> redo_q, redo_scores;
    DeviceBuf<int64_t> redo_idx, redo_ids;
    int64_t redo_cap = 0; int redo_k = 0;     // what they were sized for: queries, k
    int64_t n_filtered = 0, n_fallback = 0;   // searches answered by the filter alone / with queries (or all) redone by the exact kernel
    int64_t nq_certified = 0, nq_redone = 0;  // queries answered by the filter / re-done by the exact kernel
    int64_t pend_nq = 0; int pend_k = 0; const float* pend_q = nullptr;   // sr_dense_search_begin ran for this batch
    // sr_dense_score_pairs (pair_score.hip): the segments as a device table (rebuilt when a segment was added), the call's status words
    DeviceBuf<PairSeg> pair_segs; size_t pair_segs_n = 0;
    PairStatus* pair_status = nullptr;
    // sr_dense_search_subset / _masked hold both forms of the filter (doc_mask.hip); allocated on first use, reused
    DeviceBuf<uint32_t> mask_words;        // the bitmap of a list: id_end / 8 bytes
    DeviceBuf<int64_t> mask_list;          // the list of a bitmap: 8 m bytes
    DeviceBuf<int64_t> mask_blocks;        // per-workgroup counts of the bitmap -> list scan, + 1: the count
    // sr_dense_search_grouped (dense_restrict.hip): allocated on first use, reused
    DeviceBuf<uint32_t> grp_valid;         // bitmap of the positions below id_end that name a document (only for layouts with gaps)
    size_t grp_valid_segs = 0;             // stamp of the segment list grp_valid was built from (segments are only ever added)
    DeviceBuf<uint32_t> grp_qoff;          // [nq rounded up to 256] word offset of every query's bitmap: the grouped pass reads it
    DeviceBuf<int64_t> grp_counts;         // [n_groups] set bits per group, + 1: the first (group, bit) that names no document
    // sr_dense_range_count / _fill (dense_range.hip): the (chunk, query) prefix table of the last count and what it was made for
    DeviceBuf<uint32_t> range_tab;                                   // [chunks of all segments, range_nq]
    int64_t range_nq = -1, range_total = 0, range_chunk_rows = 0;    // range_nq = -1: no count to fill from
    size_t range_segs = 0; int64_t range_ntotal = 0;                 // stamp of the segment list (segments are only ever added)
    int range_kind = 0;                                              // what the last count ran under (SR_RANGE_KIND_*): its fill must too
    // sr_dense_range_count_grouped: written by the count, read by its fill (buffers of their own: a grouped search in between leaves them)
    DeviceBuf<uint32_t> range_qoff;        // [range_nq rounded up to 256] word offset of every query's bitmap
    DeviceBuf<uint32_t> range_union;       // [W] the OR of the bitmaps of the groups that have a query: the tile skip reads it
    DeviceBuf<int32_t> range_used;         // the ids of those groups, ascending
    int64_t range_groups = 0;              // n_groups of the last grouped count
};
// the three kinds of a range search on a handle: a fill needs a preceding count of its own kind
enum { SR_RANGE_KIND_ALL = 0, SR_RANGE_KIND_MASKED = 1, SR_RANGE_KIND_GROUPED = 2 };
static inline const char* sr_range_kind_text(int kind) {
    return kind == SR_RANGE_KIND_GROUPED ? "under filter groups" : kind == SR_RANGE_KIND_MASKED ? "under a mask" : "without a mask";
}

// bf16 planes of every segment a score mode needs (the certified filter keeps its own fp16 plane, filter_prepare_segment)
static inline int planes_of(int precision) {
    return precision == SR_PRECISION_BF16X6 ? 3 : (precision == SR_PRECISION_BF16X3 ? 2 : 0);
}

// ---- dense_index.hip ----
int filter_prepare_segment(sr_dense_index* idx, DenseSegment& seg);
// the largest document index of any segment, plus one: the length of a document bitmap
int64_t dense_id_end(const sr_dense_index* idx);

// ---- dense_search.hip: every function below is called with idx->mu held ----
enum class DenseArith { exact, bf16x3, bf16x6, filter_upper_bound };
struct DensePassOpts {
    DenseArith arith = DenseArith::exact;   // filter_upper_bound: the certified filter's pass, one fp16 plane product + the per-pair error term
    bool tiled_only = false;                // the re-do of a few queries: the tiled kernels whatever the count (one k order), workspace ws3
    int k_inner = 0;                        // filter_upper_bound: the k of the search, where the pass's own k is the candidates per query
    const uint32_t* mask = nullptr;         // filter_upper_bound, nullable: the document bitmap of a masked search - only set bits become keys
    const uint32_t* mask_qoff = nullptr;    // with mask, nullable: per query the word offset of its own bitmap inside mask (grouped search)
};
// top-k of every query over all segments (16-bit arithmetic serves batches of more than 64 queries, the exact kernels the others)
int dense_search_pass(sr_dense_index* idx, const float* d_queries, int64_t nq, int k, float* d_out_scores, int64_t* d_out_ids,
                      const DensePassOpts& opts, hipStream_t s);
// whether the certified filter can serve this index and batch, and with how many candidates per query (*kp)
int dense_filter_applies(sr_dense_index* idx, int64_t nq, int k, int* kp, bool* applies, bool full_kp = false);
// The two halves of a filtered search.  First: the kp documents with the largest upper bounds per query (idx->a_scores / a_ids / qa), under
// the document bitmap d_mask over [0, id_end) if one is given - query q's own at d_mask + d_mask_qoff[q] words if offsets are given too;
// *done = false: the filter does not apply.
int dense_filtered_candidates(sr_dense_index* idx, const float* d_queries, int64_t nq, int k, hipStream_t s, bool* done,
                              const uint32_t* d_mask = nullptr, const uint32_t* d_mask_qoff = nullptr);
// Second: exact re-score, certificate, exact re-do of the queries without one.  d_thr (nullable, doc-sharded search): per query a value
// proven not to exceed the GLOBAL k-th exact score.  d_list / m (masked search; d_list null otherwise): the allowed documents, ascending.
// redo_out (grouped search; null otherwise): the queries without a certificate are counted and handed back, ascending, instead of re-done -
// the caller re-does each under its own group's list.
int dense_filtered_finish(sr_dense_index* idx, const float* d_queries, int64_t nq, int k, const float* d_thr, float* d_out_scores,
                          int64_t* d_out_ids, hipStream_t s, const int64_t* d_list = nullptr, int64_t m = 0,
                          std::vector<int64_t>* redo_out = nullptr);
// room in idx->redo_q / redo_idx / redo_scores / redo_ids for nf queries taken out of a batch and their [nf, k] results
int dense_redo_reserve(sr_dense_index* idx, int64_t nf, int k);

// ---- dense_restrict.hip (idx->mu held): idx->pair_segs := the segments as a device table; top-k within an ascending list by the gather kernel ----
int dense_pair_segs(sr_dense_index* idx, const char* who);
int dense_subset_gather(sr_dense_index* idx, const float* d_queries, int64_t nq, int k, const int64_t* d_subset, int64_t m,
                        float* d_out_scores, int64_t* d_out_ids, hipStream_t s, const char* who);
