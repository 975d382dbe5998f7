// Dense scoring restricted to given documents: caller-supplied (query, document) pairs (pair_score.hip), and top-k within a subset
// given as an ascending list or as a bitmap - by the gather kernel (subset_search.hip) or by the certified filter's pass under the
// bitmap (dense_search.hip, doc_mask.hip).
#include "dense_index.h"
#include "subset_search.h"
#include "doc_mask.h"

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
    SR_REQUIRE(d_queries && d_out_scores && d_out_ids && (d_subset || m == 0), "sr_dense_search_subset: null pointer");
    SR_REQUIRE(((uintptr_t)d_queries & 15) == 0, "sr_dense_search_subset: queries must be 16-byte aligned");
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

// every output entry := (-FLT_MAX, -1): what the selects write for a query without a candidate
__global__ void dense_pad_rows_kernel(float* __restrict__ scores, int64_t* __restrict__ ids, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        scores[i] = -3.402823466e38f;
        ids[i] = -1;
    }
}

// The same search with the filter given as a bitmap.  The bitmap is expanded to the ascending list of its set bits, which goes through
// the check kernel of sr_dense_search_subset (a set bit that names no document is found there); then the same two routes.
extern "C" int sr_dense_search_masked(sr_dense_index* idx, const float* d_queries, int64_t nq, int k, const uint32_t* d_mask_words,
                                      int64_t n_bits, float* d_out_scores, int64_t* d_out_ids, sr_stream stream) {
    SR_REQUIRE(idx, "sr_dense_search_masked: null index");
    SR_REQUIRE(nq >= 0 && nq < (1ll << 30), "sr_dense_search_masked: bad nq=%lld", (long long)nq);
    SR_REQUIRE(k >= 1 && k <= SR_MAX_TOPK_LARGE, "sr_dense_search_masked: k=%d outside [1, %d]", k, SR_MAX_TOPK_LARGE);
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(idx->mu);
    const int64_t id_end = dense_id_end(idx);
    SR_REQUIRE(n_bits == id_end, "sr_dense_search_masked: the mask holds n_bits=%lld bits, the index's document indices end at %lld", (long long)n_bits,
               (long long)id_end);
    if (nq == 0) return SR_OK;
    SR_REQUIRE(d_queries && d_out_scores && d_out_ids && (d_mask_words || n_bits == 0), "sr_dense_search_masked: null pointer");
    SR_REQUIRE(((uintptr_t)d_queries & 15) == 0, "sr_dense_search_masked: queries must be 16-byte aligned");
    StreamOrder::Scope in_order(idx->order, s);
    // the list of the set bits: count (one 8-byte read-back: it sizes the list and the slabs), then expand
    const int64_t n_blocks = doc_mask_blocks(n_bits);
    SR_TRY(dense_mask_scratch(idx->mask_blocks, n_blocks + 1, "sr_dense_search_masked"));
    int64_t* d_count = idx->mask_blocks.p + n_blocks;
    SR_TRY(launch_doc_mask_count(d_mask_words, n_bits, idx->mask_blocks.p, d_count, s));
    int64_t m = 0;
    SR_CHECK_HIP(hipMemcpyAsync(&m, d_count, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    SR_CHECK_HIP(hipStreamSynchronize(s));
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
        if (!k_fits) {                                    // a k no valid mask of this count could have: the rows are padded here
            const int64_t n = nq * (int64_t)k;
            const int64_t blocks = ceil_div64(n, 256) < 65536 ? ceil_div64(n, 256) : 65536;
            hipLaunchKernelGGL(dense_pad_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, s, d_out_scores, d_out_ids, n);
            SR_CHECK_LAUNCH();
            SR_CHECK_HIP(hipStreamSynchronize(s));
        }
        int64_t bit = -1;
        SR_CHECK_HIP(hipMemcpy(&bit, d_list + h.first_bad, sizeof(int64_t), hipMemcpyDeviceToHost));
        sr_set_error("sr_dense_search_masked: mask bit %lld is set but names no document of the index (nothing was searched)", (long long)bit);
        return SR_ERR_INVALID;
    }
    return SR_OK;
}
