// The host side every filtered entry point shares (document filters: subset, mask, masks with query_group - dense_restrict.hip,
// dense_range.hip, subset_search.hip, sparse_range.hip): argument checks, the group ids' read-back, and what an error that scores
// nothing leaves in the outputs.  The kernels the filters run under have their own owners (dense_split_kernel.h, dense_range_kernel.h,
// sparse_cert.hip, doc_mask.hip); the route rules and the crossover constants stay with their entry points.
#pragma once
#include "common.h"
#include "doc_mask.h"
#include <vector>

// ---- the head of a filtered top-k search: handle, nq, k in this order, then (after the caller's own checks and its nq == 0 return) the
// pointers.  An entry point whose checks come in another order keeps its own lines.
static inline int sr_search_sizes(const char* who, const void* idx, int64_t nq, int k, int k_max) {
    SR_REQUIRE(idx, "%s: null index", who);
    SR_REQUIRE(nq >= 0 && nq < (1ll << 30), "%s: bad nq=%lld", who, (long long)nq);
    SR_REQUIRE(k >= 1 && k <= k_max, "%s: k=%d outside [1, %d]", who, k, k_max);
    return SR_OK;
}
// filter_given: the filter's own pointers, or a filter that needs none.  dense_queries: fp32 rows, read 16 bytes at a time.
static inline int sr_search_pointers(const char* who, const void* d_queries, const void* d_out_scores, const void* d_out_ids, bool filter_given,
                                     bool dense_queries) {
    SR_REQUIRE(d_queries && d_out_scores && d_out_ids && filter_given, "%s: null pointer", who);
    SR_REQUIRE(!dense_queries || ((uintptr_t)d_queries & 15) == 0, "%s: queries must be 16-byte aligned", who);
    return SR_OK;
}

// ---- filter groups: n_groups bitmaps of n_bits bits and a group id per query ----
// The checks before any device work, one call each, so that an entry point whose checks come in another order calls them in its own.
static inline int sr_require_groups(const char* who, int64_t n_groups) {
    SR_REQUIRE(n_groups >= 1, "%s: n_groups=%lld, at least one group is needed", who, (long long)n_groups);
    return SR_OK;
}
// bits_fmt: the caller's wording, over (who, n_bits, index_bits)
static inline int sr_require_mask_bits(const char* who, const char* bits_fmt, int64_t n_bits, int64_t index_bits) {
    SR_REQUIRE(n_bits == index_bits, bits_fmt, who, (long long)n_bits, (long long)index_bits);
    return SR_OK;
}
// words: of one bitmap as the scorer walks it; and_union: the scorer keeps the OR of all groups as one more row
static inline int sr_require_group_words(const char* who, int64_t n_groups, int64_t words, bool and_union) {
    SR_REQUIRE(n_groups < (1ll << 32) && (n_groups + (and_union ? 1 : 0)) * words < (1ll << 32), "%s: %lld groups%s of %lld words exceed 2^32 words", who,
               (long long)n_groups, and_union ? " (and their union)" : "", (long long)words);
    return SR_OK;
}
// the common order: n_groups, n_bits, the word limit over the bitmaps as given
static inline int sr_group_mask_checks(const char* who, int64_t n_groups, int64_t n_bits, int64_t index_bits, const char* bits_fmt) {
    SR_TRY(sr_require_groups(who, n_groups));
    SR_TRY(sr_require_mask_bits(who, bits_fmt, n_bits, index_bits));
    return sr_require_group_words(who, n_groups, doc_mask_words(n_bits), false);
}
// the two halves of a grouped range search take the pointers on their own; a search checks them with its others (sr_search_pointers)
static inline int sr_require_group_pointers(const char* who, int64_t nq, const uint32_t* d_group_words, const int32_t* d_query_group, int64_t n_bits) {
    SR_REQUIRE(nq <= 0 || (d_query_group && (d_group_words || n_bits == 0)), "%s: null masks or query groups", who);
    return SR_OK;
}

// the first q with grp[q] outside [0, n_groups), -1 if there is none
static inline int64_t sr_first_bad_group(const int32_t* grp, int64_t nq, int64_t n_groups) {
    for (int64_t q = 0; q < nq; ++q)
        if (grp[q] < 0 || grp[q] >= n_groups) return q;
    return -1;
}
// grp := the nq group ids (one read-back of 4 nq bytes, one wait); *bad := sr_first_bad_group.  Between this and sr_bad_group_error the
// caller leaves its outputs as its contract says: padding rows, zeroed lims, or nothing.
static inline int sr_read_query_groups(const int32_t* d_query_group, int64_t nq, int64_t n_groups, hipStream_t s, std::vector<int32_t>* grp,
                                       int64_t* bad) {
    grp->resize((size_t)nq);
    SR_TRY(sr_read_back(grp->data(), d_query_group, (size_t)nq * 4, s));
    *bad = sr_first_bad_group(grp->data(), nq, n_groups);
    return SR_OK;
}
// tail: " (nothing was searched)", " (nothing was scored)" or ""
static inline int sr_bad_group_error(const char* who, int64_t q, int32_t g, int64_t n_groups, const char* tail) {
    sr_set_error("%s: query %lld is in group %d, outside [0, %lld)%s", who, (long long)q, (int)g, (long long)n_groups, tail);
    return SR_ERR_INVALID;
}

// The length of a per-query word-offset table: whole query tiles of the widest kernel that reads it (256), a lane beyond nq reads an
// offset of 0.  d_qoff [sr_query_offsets_len(nq)] := the word offset of every query's bitmap (launch_doc_mask_query_offsets).
static inline int64_t sr_query_offsets_len(int64_t nq) { return ceil_div64(nq, 256) * 256; }
static inline int sr_query_offsets(const int32_t* d_query_group, int64_t nq, int64_t n_bits, uint32_t* d_qoff, hipStream_t s) {
    return launch_doc_mask_query_offsets(d_query_group, nq, sr_query_offsets_len(nq), n_bits, d_qoff, s);
}

// ---- what an error that scores nothing leaves behind (filter_args.hip) ----
// every output row of a top-k search := (pad_score, -1) - what the selects write for a query without a candidate: -FLT_MAX dense, 0
// sparse - and every count (nullable) := 0; then the stream is waited for
#define SR_DENSE_PAD_SCORE (-3.402823466e38f)
int launch_pad_rows(float* d_scores, int64_t* d_ids, int32_t* d_counts, int64_t nq, int k, float pad_score, hipStream_t s);
// the lims of a range count without a hit: lims[0 .. nq] := 0, waited for, *total := 0
static inline int sr_zero_lims(int64_t* d_lims, int64_t nq, int64_t* total, hipStream_t s) {
    SR_CHECK_HIP(hipMemsetAsync(d_lims, 0, (size_t)(nq + 1) * 8, s));
    SR_CHECK_HIP(hipStreamSynchronize(s));
    *total = 0;
    return SR_OK;
}
