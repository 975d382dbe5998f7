// Dense scoring restricted to given documents: caller-supplied (query, document) pairs (pair_score.hip), and top-k within a subset
// given as an ascending list or as a bitmap - by the gather kernel (subset_search.hip) or by the certified filter's pass under the
// bitmap (dense_search.hip, doc_mask.hip); and the same under a bitmap per query (filter groups, at the end of the file).
#include "dense_index.h"
#include "dense_filter.h"
#include "subset_search.h"
#include "doc_mask.h"
#include "filter_args.h"
#include <algorithm>
#include <utility>

int dense_pair_segs(sr_dense_index* idx, const char* who) {
    if (idx->pair_segs_n != idx->segs.size()) {           // segments are only ever added, all of one row type
        std::vector<PairSeg> h;
        for (const DenseSegment& seg : idx->segs) h.push_back(PairSeg{seg.rows, seg.n, seg.id_base, seg.id_stride});
        idx->pair_segs_n = 0;
        if (idx->pair_segs.reserve((int64_t)h.size(), nullptr) != SR_OK) {
            sr_set_error("%s: out of device memory for the table of %zu segments", who, h.size());
            return SR_ERR_NOMEM;
        }
        SR_CHECK_HIP(hipMemcpy(idx->pair_segs.p, h.data(), sizeof(PairSeg) * h.size(), hipMemcpyHostToDevice));
        idx->pair_segs_n = h.size();
    }
    return SR_OK;
}

extern "C" int sr_dense_score_pairs(sr_dense_index* idx, const float* d_queries, int64_t nq, const int64_t* d_cand_indptr,
                                    const int64_t* d_cand_ids, float* d_out_scores, sr_stream stream) {
    SR_REQUIRE(idx, "sr_dense_score_pairs: null index");
    SR_REQUIRE(nq >= 0 && nq < (1ll << 30), "sr_dense_score_pairs: bad nq=%lld", (long long)nq);
    if (nq == 0) return SR_OK;
    SR_REQUIRE(d_queries && d_cand_indptr && d_cand_ids && d_out_scores, "sr_dense_score_pairs: null pointer");
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(idx->mu);
    StreamOrder::Scope in_order(idx->order, s);
    SR_TRY(dense_pair_segs(idx, "sr_dense_score_pairs"));
    SR_TRY(pair_status_begin(&idx->pair_status, d_cand_indptr, nq, s));
    SR_TRY(launch_dense_pairs(idx->pair_segs.p, (int)idx->pair_segs_n, idx->row_dtype, d_queries, nq, idx->dim, d_cand_indptr, d_cand_ids, d_out_scores,
                              idx->pair_status, s));
    return pair_status_end(idx->pair_status, d_cand_ids, "sr_dense_score_pairs", s);
}

// The gather route of a subset search (subset_search.hip): scores are the pair scorer's chains, the select is the searches' own.  The
// caller has run the check kernel on the list (idx->pair_status) and set up idx->pair_segs; nothing is scored once the check found an offender.
int dense_subset_gather(sr_dense_index* idx, const float* d_queries, int64_t nq, int k, const int64_t* d_subset, int64_t m,
                        float* d_out_scores, int64_t* d_out_ids, hipStream_t s, const char* who) {
    int64_t nq_batch = 0, slab = 0;
    SR_TRY(subset_plan(idx->ws_limit, nq, k, m, 64, &nq_batch, &slab, who));
    for (int64_t qb = 0; qb < nq; qb += nq_batch) {
        const int64_t nqb = nq - qb < nq_batch ? nq - qb : nq_batch;
        SR_TRY(idx->ws.ensure(nqb, k, slab));
        SR_TRY(topk_reset(idx->ws, nqb, s));
        // short first slabs, doubled: until k rows were seen every one is a candidate (as the searches' first launches)
        int64_t step = ceil_div64((int64_t)k + 1024, 64) * 64;
        for (int64_t j0 = 0; j0 < m;) {
            if (step > slab) step = slab;
            const int64_t n = m - j0 < step ? m - j0 : step;
            DenseSubsetArgs a;
            a.segs = idx->pair_segs.p; a.n_segs = (int)idx->pair_segs_n; a.dtype = idx->row_dtype;
            a.Q = d_queries + qb * idx->dim; a.nq = (int)nqb; a.H = idx->dim;
            a.subset = d_subset + j0; a.n_slab = n;
            a.tau = idx->ws.tau; a.cand_keys = idx->ws.cand_keys; a.cand_count = idx->ws.cand_count; a.cand_cap = idx->ws.cand_cap;
            a.st = idx->pair_status;
            SR_TRY(launch_dense_subset(a, s));
            SR_TRY(topk_compact(idx->ws, nqb, k, s));
            j0 += n;
            step *= 2;
        }
        SR_TRY(topk_finalize(idx->ws, nqb, k, -3.402823466e38f, d_out_scores + qb * k, d_out_ids + qb * k, nullptr, s));
    }
    return SR_OK;
}

// Route rule of the subset searches.  gather: one fmaf chain per (query, allowed row) on the vector ALU, cost ~ nq x m (2.0 ms per
// 1 000 rows at 6 980 queries).  mask: the certified filter's pass over ALL rows on the MFMA pipe with the bitmap in its epilogue, cost
// ~ nq x ntotal whatever m is (229 - 262 ms at 6 980 queries x 8.84 M rows).  auto takes the mask route where it applies and nq x m
// reaches SR_SUBSET_DENSE_CROSSOVER: measured with both routes forced at 6 980 queries (tools/bench_subset.py --legs dense_routes,
// profiles/subset_search.json) the two meet near m = 130 000 (gather 203 ms at 100 000 and 1 988 ms at 1 000 000, mask
// 262 and 245 ms) - one box, one collection size, an estimate.  The constant holds only near that point (nq = 6 980, ntotal = 8.84 M):
// by the cost model above the routes really meet at a FRACTION m / ntotal (about 1.5 % here) that does not depend on nq, so a batch
// ten times larger takes the mask route at a tenth of the m, where gather would still be the cheaper, and a collection ten times
// smaller keeps gather up to ten times the fraction.  The product form is the rule as specified; a rule in m / id_end is the next
// step once a second collection size has been measured.  Dev switch SR_SUBSET_DENSE_ROUTE=gather|mask forces one, read per call;
// `mask` where the filter does not apply is served by gather.
#define SR_SUBSET_DENSE_CROSSOVER (6980ll * 130000ll)
static bool subset_dense_wants_mask(int64_t nq, int64_t m) {
    if (const char* route = sr_dev_getenv("SR_SUBSET_DENSE_ROUTE")) {
        if (strcmp(route, "mask") == 0) return true;
        if (strcmp(route, "gather") == 0) return false;
    }
    return nq * m >= SR_SUBSET_DENSE_CROSSOVER;
}

// room for `want` elements of one of the handle's three filter buffers (mask_words, mask_list, mask_blocks)
template <typename T>
static int dense_mask_scratch(DeviceBuf<T>& buf, int64_t want, const char* who) {
    if (buf.reserve(want, nullptr) == SR_OK) return SR_OK;
    sr_set_error("%s: out of device memory for %lld bytes of filter scratch", who, (long long)(want * (int64_t)sizeof(T)));
    return SR_ERR_NOMEM;
}

// The mask route: both forms of the filter are at hand and d_list has passed the check kernel.  Caller holds idx->mu.
static int dense_search_restricted(sr_dense_index* idx, const float* d_queries, int64_t nq, int k, const int64_t* d_list, int64_t m,
                                   const uint32_t* d_words, float* d_out_scores, int64_t* d_out_ids, hipStream_t s, const char* who) {
    bool done = false;
    SR_TRY(dense_filtered_candidates(idx, d_queries, nq, k, s, &done, d_words));
    if (!done) return dense_subset_gather(idx, d_queries, nq, k, d_list, m, d_out_scores, d_out_ids, s, who);     // e.g. no room for the candidate lists
    return dense_filtered_finish(idx, d_queries, nq, k, nullptr, d_out_scores, d_out_ids, s, d_list, m);
}

// Top-k within a subset of the documents: the gather route (subset_search.hip), or - for large nq x m on an index the certified filter
// serves - the filter's pass under the list's bitmap (the mask route).  The same bits either way.
extern "C" int sr_dense_search_subset(sr_dense_index* idx, const float* d_queries, int64_t nq, int k, const int64_t* d_subset, int64_t m,
                                      float* d_out_scores, int64_t* d_out_ids, sr_stream stream) {
    SR_REQUIRE(idx, "sr_dense_search_subset: null index");
    SR_REQUIRE(nq >= 0 && nq < (1ll << 30), "sr_dense_search_subset: bad nq=%lld", (long long)nq);
    SR_REQUIRE(m >= 0 && m <= idx->ntotal, "sr_dense_search_subset: a strictly ascending subset of %lld documents holds at most that many, not m=%lld",
               (long long)idx->ntotal, (long long)m);
    SR_REQUIRE(k >= 1 && k <= SR_MAX_TOPK_LARGE, "sr_dense_search_subset: k=%d outside [1, %d]", k, SR_MAX_TOPK_LARGE);
    SR_REQUIRE(k <= SR_MAX_TOPK || (int64_t)k - SR_MAX_TOPK <= m, "sr_dense_search_subset: k=%d exceeds %d by more than the subset's %lld documents", k,
               SR_MAX_TOPK, (long long)m);
    if (nq == 0) return SR_OK;
    SR_TRY(sr_search_pointers("sr_dense_search_subset", d_queries, d_out_scores, d_out_ids, d_subset || m == 0, true));
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(idx->mu);
    StreamOrder::Scope in_order(idx->order, s);
    int64_t nq_batch = 0, slab = 0;
    SR_TRY(subset_plan(idx->ws_limit, nq, k, m, 64, &nq_batch, &slab, "sr_dense_search_subset"));       // a call that cannot run fails before any launch
    if (m > 0) SR_TRY(dense_pair_segs(idx, "sr_dense_search_subset"));
    SR_TRY(subset_status_begin(&idx->pair_status, s));
    SR_TRY(launch_subset_check_dense(idx->pair_segs.p, (int)idx->pair_segs_n, d_subset, m, idx->pair_status, s));
    int kp = 0;
    bool mask_route = idx->precision == SR_PRECISION_FP32_FILTERED && subset_dense_wants_mask(nq, m);
    if (mask_route) SR_TRY(dense_filter_applies(idx, nq, k, &kp, &mask_route, true));
    if (mask_route) {
        // the list gets its bitmap once the check kernel has accepted it: the mask route reads the call's status here, not at the end (a
        // bad list goes on to the gather route, which writes the padding rows and reports it)
        const int64_t n_bits = dense_id_end(idx);
        mask_route = subset_status_end(idx->pair_status, d_subset, "sr_dense_search_subset", "doc index", s) == SR_OK;
        if (mask_route) {
            SR_TRY(dense_mask_scratch(idx->mask_words, doc_mask_words(n_bits) > 0 ? doc_mask_words(n_bits) : 1, "sr_dense_search_subset"));
            SR_TRY(launch_doc_mask_from_list(d_subset, m, idx->mask_words.p, n_bits, idx->pair_status, nullptr, s));
            return dense_search_restricted(idx, d_queries, nq, k, d_subset, m, idx->mask_words.p, d_out_scores, d_out_ids, s, "sr_dense_search_subset");
        }
    }
    SR_TRY(dense_subset_gather(idx, d_queries, nq, k, d_subset, m, d_out_scores, d_out_ids, s, "sr_dense_search_subset"));
    return subset_status_end(idx->pair_status, d_subset, "sr_dense_search_subset", "doc index", s);
}

// The same search with the filter given as a bitmap.  The bitmap is expanded to the ascending list of its set bits, which goes through
// the check kernel of sr_dense_search_subset (a set bit that names no document is found there); then the same two routes.
extern "C" int sr_dense_search_masked(sr_dense_index* idx, const float* d_queries, int64_t nq, int k, const uint32_t* d_mask_words,
                                      int64_t n_bits, float* d_out_scores, int64_t* d_out_ids, sr_stream stream) {
    SR_TRY(sr_search_sizes("sr_dense_search_masked", idx, nq, k, SR_MAX_TOPK_LARGE));
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(idx->mu);
    const int64_t id_end = dense_id_end(idx);
    SR_REQUIRE(n_bits == id_end, "sr_dense_search_masked: the mask holds n_bits=%lld bits, the index's document indices end at %lld", (long long)n_bits,
               (long long)id_end);
    if (nq == 0) return SR_OK;
    SR_TRY(sr_search_pointers("sr_dense_search_masked", d_queries, d_out_scores, d_out_ids, d_mask_words || n_bits == 0, true));
    StreamOrder::Scope in_order(idx->order, s);
    // the list of the set bits: count (one 8-byte read-back: it sizes the list and the slabs), then expand
    SR_TRY(dense_mask_scratch(idx->mask_blocks, doc_mask_blocks(n_bits) + 1, "sr_dense_search_masked"));
    int64_t m = 0;
    SR_TRY(doc_mask_count_sync(d_mask_words, n_bits, idx->mask_blocks.p, s, &m));
    SR_TRY(dense_mask_scratch(idx->mask_list, m > 0 ? m : 1, "sr_dense_search_masked"));
    int64_t* const d_list = idx->mask_list.p;
    SR_TRY(launch_doc_mask_expand(d_mask_words, n_bits, idx->mask_blocks.p, d_list, m, s));
    if (m > 0) SR_TRY(dense_pair_segs(idx, "sr_dense_search_masked"));
    SR_TRY(subset_status_begin(&idx->pair_status, s));
    SR_TRY(launch_subset_check_dense(idx->pair_segs.p, (int)idx->pair_segs_n, d_list, m, idx->pair_status, s));
    // The list is ascending by construction: an offender is a bit in a gap of a strided segment or past a short segment's end.  The
    // call's one read of the status: the mask route needs it before its pass, and the limit on k needs a list that stands.
    PairStatus h;
    SR_CHECK_HIP(hipMemcpyAsync(&h, idx->pair_status, sizeof(h), hipMemcpyDeviceToHost, s));
    SR_CHECK_HIP(hipStreamSynchronize(s));
    const bool bad = h.first_bad != ~0ull;
    const bool k_fits = k <= SR_MAX_TOPK || (int64_t)k - SR_MAX_TOPK <= m;
    if (!bad) {
        SR_REQUIRE(k_fits, "sr_dense_search_masked: k=%d exceeds %d by more than the mask's %lld documents", k, SR_MAX_TOPK, (long long)m);
        int kp = 0;
        bool mask_route = idx->precision == SR_PRECISION_FP32_FILTERED && subset_dense_wants_mask(nq, m);
        if (mask_route) SR_TRY(dense_filter_applies(idx, nq, k, &kp, &mask_route, true));
        if (mask_route)
            return dense_search_restricted(idx, d_queries, nq, k, d_list, m, d_mask_words, d_out_scores, d_out_ids, s, "sr_dense_search_masked");
    }
    // the gather route; after an offender it scores nothing and every output row is padding
    if (k_fits) SR_TRY(dense_subset_gather(idx, d_queries, nq, k, d_list, m, d_out_scores, d_out_ids, s, "sr_dense_search_masked"));
    if (bad) {
        // a k no valid mask of this count could have: the rows are padded here
        if (!k_fits) SR_TRY(launch_pad_rows(d_out_scores, d_out_ids, nullptr, nq, k, SR_DENSE_PAD_SCORE, s));
        int64_t bit = -1;
        SR_CHECK_HIP(hipMemcpy(&bit, d_list + h.first_bad, sizeof(int64_t), hipMemcpyDeviceToHost));
        sr_set_error("sr_dense_search_masked: mask bit %lld is set but names no document of the index (nothing was searched)", (long long)bit);
        return SR_ERR_INVALID;
    }
    return SR_OK;
}

// ---- filter groups: a document bitmap per query (sr_dense_search_grouped) ------------------------------------------
// Route rule.  The grouped pass is the mask route with the bit read from the query's own bitmap: cost ~ nq x ntotal whatever the groups
// are.  The loop runs the gather route once per group: cost ~ sum_g nq_g x m_g pairs, plus a gather of the queries, a bitmap -> list
// expansion and a scatter per group.  auto takes the pass where it applies and the pairs reach SR_SUBSET_DENSE_CROSSOVER - a constant
// that was measured for ONE group (above).  The loop's per-group overhead moves the real crossover down as the groups multiply, and
// nobody has measured where.  Dev switch SR_GROUPED_DENSE_ROUTE=pass|loop forces one, read per call; `pass` where the filter does not
// apply is served by the loop.
static bool grouped_dense_wants_pass(int64_t pairs) {
    if (const char* route = sr_dev_getenv("SR_GROUPED_DENSE_ROUTE")) {
        if (strcmp(route, "pass") == 0) return true;
        if (strcmp(route, "loop") == 0) return false;
    }
    return pairs >= SR_SUBSET_DENSE_CROSSOVER;
}

// idx->grp_valid := the bitmap of the positions that name a document, or *d_valid = null where every position below id_end does (stride-1
// segments that cover [0, id_end): nothing to test).  Built from the segment table and kept until a segment is added.
static int grouped_valid_bitmap(sr_dense_index* idx, int64_t n_bits, const uint32_t** d_valid, hipStream_t s) {
    *d_valid = nullptr;
    std::vector<std::pair<int64_t, int64_t>> spans;       // (id_base, n) of the stride-1 segments
    bool dense_layout = true;
    for (const DenseSegment& seg : idx->segs) {
        if (seg.n > 1 && seg.id_stride != 1) dense_layout = false;
        spans.push_back({seg.id_base, seg.n});
    }
    if (dense_layout) {
        std::sort(spans.begin(), spans.end());
        int64_t end = 0;
        for (const auto& sp : spans) {
            if (sp.first > end) break;                    // a hole in front of this segment
            if (sp.first + sp.second > end) end = sp.first + sp.second;
        }
        if (end >= n_bits) return SR_OK;
    }
    if (idx->grp_valid_segs != idx->segs.size() || !idx->grp_valid.p) {
        idx->grp_valid_segs = 0;
        SR_TRY(dense_mask_scratch(idx->grp_valid, doc_mask_words(n_bits), "sr_dense_search_grouped"));
        SR_CHECK_HIP(hipMemsetAsync(idx->grp_valid.p, 0, (size_t)doc_mask_words(n_bits) * 4, s));
        for (const DenseSegment& seg : idx->segs) SR_TRY(launch_doc_mask_add_segment(idx->grp_valid.p, n_bits, seg.n, seg.id_base, seg.id_stride, s));
        idx->grp_valid_segs = idx->segs.size();
    }
    *d_valid = idx->grp_valid.p;
    return SR_OK;
}

// The queries h_members[0 .. n) of the call (ascending) searched under one group's bitmap of m set bits, by the gather route, and their
// rows written into the call's outputs.  h_members is the source of an asynchronous copy: it must outlive the caller's next wait.
static int grouped_gather_group(sr_dense_index* idx, const float* d_queries, int k, const uint32_t* d_words, int64_t n_bits, int64_t m,
                                const int64_t* h_members, int64_t n, float* d_out_scores, int64_t* d_out_ids, hipStream_t s) {
    if (n == 0) return SR_OK;
    SR_TRY(dense_redo_reserve(idx, n, k));
    SR_CHECK_HIP(hipMemcpyAsync(idx->redo_idx.p, h_members, (size_t)n * 8, hipMemcpyHostToDevice, s));
    SR_TRY(launch_filter_gather_rows(d_queries, idx->redo_idx.p, n, idx->dim, idx->redo_q.p, false, s));
    // the ascending list of the group's bits: the count is known, the scan only places the workgroups
    SR_TRY(dense_mask_scratch(idx->mask_blocks, doc_mask_blocks(n_bits) + 1, "sr_dense_search_grouped"));
    SR_TRY(dense_mask_scratch(idx->mask_list, m > 0 ? m : 1, "sr_dense_search_grouped"));
    SR_TRY(doc_mask_list(d_words, n_bits, m, idx->mask_blocks.p, idx->mask_list.p, s));
    SR_TRY(dense_subset_gather(idx, idx->redo_q.p, n, k, idx->mask_list.p, m, idx->redo_scores.p, idx->redo_ids.p, s, "sr_dense_search_grouped"));
    SR_TRY(launch_filter_gather_rows(idx->redo_scores.p, idx->redo_idx.p, n, k, d_out_scores, true, s));
    return launch_filter_gather_rows(idx->redo_ids.p, idx->redo_idx.p, n, 2 * (int64_t)k, d_out_ids, true, s);
}

// Top-k of every query within its own group's documents.  Two routes, the same bits: the certified filter's pass with the bit test reading
// the query's bitmap (dense_split_grouped.hip), its uncertified queries re-done by the gather route under their group's list; or the
// gather route group by group.
extern "C" int sr_dense_search_grouped(sr_dense_index* idx, const float* d_queries, int64_t nq, int k, const uint32_t* d_group_words,
                                       int64_t n_groups, int64_t n_bits, const int32_t* d_query_group, float* d_out_scores,
                                       int64_t* d_out_ids, sr_stream stream) {
    const char* const who = "sr_dense_search_grouped";
    SR_TRY(sr_search_sizes(who, idx, nq, k, SR_MAX_TOPK));
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(idx->mu);
    SR_TRY(sr_group_mask_checks(who, n_groups, n_bits, dense_id_end(idx), "%s: the masks hold n_bits=%lld bits each, the index's document indices end at %lld"));
    const int64_t n_words = doc_mask_words(n_bits);
    if (nq == 0) return SR_OK;
    SR_TRY(sr_search_pointers(who, d_queries, d_out_scores, d_out_ids, d_query_group && (d_group_words || n_bits == 0), true));
    StreamOrder::Scope in_order(idx->order, s);
    // 1. the group ids: one read-back of 4 nq bytes
    std::vector<int32_t> grp;
    int64_t bad = -1;
    SR_TRY(sr_read_query_groups(d_query_group, nq, n_groups, s, &grp, &bad));
    if (bad >= 0) {
        SR_TRY(launch_pad_rows(d_out_scores, d_out_ids, nullptr, nq, k, SR_DENSE_PAD_SCORE, s));
        return sr_bad_group_error(who, bad, grp[(size_t)bad], n_groups, " (nothing was searched)");
    }
    // 2. set bits per group, and the first set bit that names no document: one read-back of 8 (n_groups + 1) bytes
    const uint32_t* d_valid = nullptr;
    SR_TRY(grouped_valid_bitmap(idx, n_bits, &d_valid, s));
    SR_TRY(dense_mask_scratch(idx->grp_counts, n_groups + 1, "sr_dense_search_grouped"));
    SR_TRY(launch_doc_masks_check(d_group_words, n_groups, n_bits, d_valid, idx->grp_counts.p, s));
    std::vector<int64_t> counts((size_t)n_groups + 1);
    SR_CHECK_HIP(hipMemcpyAsync(counts.data(), idx->grp_counts.p, (size_t)(n_groups + 1) * 8, hipMemcpyDeviceToHost, s));
    SR_CHECK_HIP(hipStreamSynchronize(s));
    if (counts[(size_t)n_groups] != -1) {
        const uint64_t at = (uint64_t)counts[(size_t)n_groups];
        const int64_t word = (int64_t)(at >> 5);
        SR_TRY(launch_pad_rows(d_out_scores, d_out_ids, nullptr, nq, k, SR_DENSE_PAD_SCORE, s));
        sr_set_error("sr_dense_search_grouped: group %lld: mask bit %lld is set but names no document of the index (nothing was searched)",
                     (long long)(word / n_words), (long long)((word % n_words) * 32 + (int64_t)(at & 31)));
        return SR_ERR_INVALID;
    }
    // 3. the queries by group (a stable sort: ascending inside a group), the pairs a gather of everything would score
    std::vector<int64_t> order((size_t)nq);
    for (int64_t q = 0; q < nq; ++q) order[(size_t)q] = q;
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return grp[(size_t)a] < grp[(size_t)b]; });
    int64_t pairs = 0;
    for (int64_t q = 0; q < nq; ++q) pairs += counts[(size_t)grp[(size_t)q]];
    if (idx->ntotal > 0) SR_TRY(dense_pair_segs(idx, "sr_dense_search_grouped"));
    SR_TRY(subset_status_begin(&idx->pair_status, s));    // the gather kernel reads it; the bitmaps have passed their own check
    // runs of `sel` (positions of `order`, sorted by group) -> one gather search per group that has a query in it
    auto gather_groups = [&](const std::vector<int64_t>& sel) -> int {
        for (size_t i0 = 0; i0 < sel.size();) {
            const int64_t g = grp[(size_t)sel[i0]];
            size_t i1 = i0;
            while (i1 < sel.size() && grp[(size_t)sel[i1]] == g) ++i1;
            SR_TRY(grouped_gather_group(idx, d_queries, k, d_group_words + g * n_words, n_bits, counts[(size_t)g], sel.data() + i0, (int64_t)(i1 - i0),
                                        d_out_scores, d_out_ids, s));
            i0 = i1;
        }
        SR_CHECK_HIP(hipStreamSynchronize(s));            // `sel` (pageable host memory) is the source of asynchronous copies
        return SR_OK;
    };
    int kp = 0;
    bool pass_route = idx->precision == SR_PRECISION_FP32_FILTERED && grouped_dense_wants_pass(pairs);
    if (pass_route) SR_TRY(dense_filter_applies(idx, nq, k, &kp, &pass_route, true));
    if (pass_route) {
        SR_TRY(dense_mask_scratch(idx->grp_qoff, sr_query_offsets_len(nq), who));
        SR_TRY(sr_query_offsets(d_query_group, nq, n_bits, idx->grp_qoff.p, s));
        bool done = false;
        SR_TRY(dense_filtered_candidates(idx, d_queries, nq, k, s, &done, d_group_words, idx->grp_qoff.p));
        if (done) {
            std::vector<int64_t> redo;                     // the queries without a certificate, ascending
            SR_TRY(dense_filtered_finish(idx, d_queries, nq, k, nullptr, d_out_scores, d_out_ids, s, nullptr, 0, &redo));
            if (redo.empty()) return SR_OK;
            std::stable_sort(redo.begin(), redo.end(), [&](int64_t a, int64_t b) { return grp[(size_t)a] < grp[(size_t)b]; });
            return gather_groups(redo);
        }
    }
    return gather_groups(order);                          // the group loop (also: no room for the candidate lists)
}
