// Dense top-k search: the scan of all segments with fused top-k filtering, in exact fp32 or 16-bit arithmetic, and around it the
// certified filter (SR_PRECISION_FP32_FILTERED: exact results at 16-bit MFMA speed) and the doc-sharded begin / finish pair.
//
// A doc chunk = one launch; scores never go to HBM: survivors (score >= tau[q]) are appended as 64-bit keys to the per-query
// candidate buffer and merged into the running top-k between launches, which raises tau (topk.hip).
#include "dense_index.h"
#include "dense_score.h"
#include "dense_stream.h"
#include "dense_split.h"
#include "dense_filter.h"
#include <stdlib.h>

// The scan every arithmetic runs over a workspace that was reset: per segment, launches of `step` rows - the step doubling up to `cap`
// and carried across segments - each followed by after_launch() (the compaction); then the final select.  row_elem_bytes: what the
// launch profile counts per row element.
template <typename Launch, typename AfterLaunch>
static int dense_scan(sr_dense_index* idx, TopkWS& ws, int64_t nq, int k, int64_t step, int64_t cap, double row_elem_bytes, float* d_out_scores,
                      int64_t* d_out_ids, hipStream_t s, Launch launch, AfterLaunch after_launch) {
    for (const DenseSegment& seg : idx->segs) {
        for (int64_t r0 = 0; r0 < seg.n;) {
            const int64_t r1 = r0 + step < seg.n ? r0 + step : seg.n;
            step = step * 2 < cap ? step * 2 : cap;
            idx->prof.begin(s);
            SR_TRY(launch(seg, r0, r1));
            idx->prof.end(s, 2.0 * (double)nq * (double)(r1 - r0) * idx->dim, (double)(r1 - r0) * idx->dim * row_elem_bytes);
            SR_TRY(after_launch());
            r0 = r1;
        }
    }
    return topk_finalize(ws, nq, k, -3.402823466e38f, d_out_scores, d_out_ids, nullptr, s);
}

// Launch plan of the tiled kernels and the 16-bit passes.  *chunk = docs per launch (= candidate capacity per query): workgroups per
// launch = doc tiles x query tiles are a multiple of the 256 CUs (one workgroup per CU: no partially filled last round), at least
// default_wgs, within the candidate budget.  The first launches see no threshold yet (every doc is a candidate until k have been seen),
// so they are kept short and doubled - *step0 = 2048, then 4096, ... docs - until the regular chunk: each then appends about k survivors
// per query instead of a whole chunk's worth for the first one (32 768 keys per query, 1.8 GB at 6980 queries) ... but never shorter
// than one workgroup per CU.
static void dense_tiled_plan(int64_t nq, int k, int64_t cand_limit, int64_t default_wgs, int64_t* step0, int64_t* chunk) {
    const int64_t TM = 256, qtiles = ceil_div64(nq, dense_query_tile(nq));
    int64_t g = 256, t = qtiles;
    while (t) { const int64_t r = g % t; g = t; t = r; }     // g = gcd(256, qtiles)
    const int64_t unit = 256 / g;
    const char* env_wgs = sr_dev_getenv("SR_DENSE_LAUNCH_WGS");      // A/B switch: workgroups per launch
    const int64_t launch_wgs = env_wgs ? atoll(env_wgs) : default_wgs;
    *chunk = TM * unit * ceil_div64(launch_wgs, unit * qtiles);
    int64_t max_cap = cand_limit / (8 * nq);
    max_cap = (max_cap / TM) * TM;
    if (max_cap < TM) max_cap = TM;
    if (*chunk > max_cap) *chunk = max_cap;
    *step0 = ceil_div64((int64_t)k + 1024, TM) * TM;
    if (*step0 < TM * ceil_div64(256, qtiles)) *step0 = TM * ceil_div64(256, qtiles);
    if (*step0 > *chunk) *step0 = *chunk;
}

// scores on the 16-bit MFMA pipe (dense_split.hip): the same chunking and top-k machinery, a workspace of its own
static int dense_pass_16bit(sr_dense_index* idx, const float* d_queries, int64_t nq, int k, float* d_out_scores, int64_t* d_out_ids,
                            const DensePassOpts& opts, int64_t cand_limit, hipStream_t s) {
    TopkWS& ws = idx->wsf;
    const int np = opts.arith == DenseArith::filter_upper_bound ? 0 : (opts.arith == DenseArith::bf16x6 ? 3 : 2);   // bf16 planes per operand
    // twice the docs per launch of the exact kernels (28 rounds of tiles instead of 14 at 6 980 queries): half the launch ramps and
    // compactions, 0.7606 -> 0.7417 ms per 14 rounds, search -2 % (same results; tools/split_ab.py SR_DENSE_LAUNCH_WGS=...)
    int64_t step0, chunk;
    dense_tiled_plan(nq, k, cand_limit, 7168, &step0, &chunk);
    for (int p = 0; p < 3; ++p) SR_TRY(idx->qpl[p].reserve(nq * (int64_t)idx->dim, "dense search"));
    // the filter's second threshold (dense_filter.h): k_inner = the k of the search, `k` here = kp candidates
    bool two = np == 0 && opts.k_inner > 0 && opts.k_inner < k;
    if (const char* e = sr_dev_getenv("SR_FILTER_TAU2")) two = two && atoi(e) != 0;                  // A/B switch
    // with the second threshold the running set is cut back (and both thresholds refreshed) once it holds k + 1 024 keys instead of 2 k:
    // fresher thresholds save more in the pass than the extra selects cost (search 229.3 -> 224.4 ms at the MSMARCO shape)
    int select_over = two ? k + 1024 : 2 * k;
    if (const char* e = sr_dev_getenv("SR_FILTER_SELECT_OVER")) select_over = atoi(e);              // A/B switch
    float* f_slack = idx->qa.p + 4 * idx->fq_cap, *f_tau2 = f_slack + idx->fq_cap, *f_tau_eff = f_tau2 + idx->fq_cap;
    if (np == 0) SR_TRY(launch_filter_queries(d_queries, nq, idx->dim, idx->qpl[0].p, idx->qa.p, s));     // idx->qa: dense_filtered_candidates
    else SR_TRY(launch_split_bf16(d_queries, idx->qpl[0].p, idx->qpl[1].p, idx->qpl[2].p, nq * (int64_t)idx->dim, s));
    if (two) {
        FilterSegMax fm;
        fm.count = (int)idx->segs.size();
        for (int i = 0; i < fm.count; ++i) { fm.x[i] = idx->segs[i].fx_max; fm.y[i] = idx->segs[i].fy_max; fm.isd[i] = idx->segs[i].fisd; }
        SR_TRY(launch_filter_slack(idx->qa.p, nq, fm, f_slack, f_tau2, s));
    }
    // segmented candidate slots: one segment per (256-doc tile of a launch, producer lane group), see common.h
    bool use_seg = true;
    if (const char* e = sr_dev_getenv("SR_SPLIT_SEG")) use_seg = atoi(e) != 0;       // A/B switch: 0 = atomic appends only
    if (use_seg) SR_TRY(ws.ensure_segments(nq, k, chunk, (int)(chunk / 256) * SR_SEG_PROD));
    else SR_TRY(ws.ensure(nq, k, chunk));
    SR_TRY(topk_reset(ws, nq, s));
    if (two && idx->ntotal > 0) SR_TRY(launch_filter_tau(ws.tau, f_tau2, f_slack, f_tau_eff, nq, s));    // ahead of the first launch: both -inf
    return dense_scan(
        idx, ws, nq, k, step0, chunk, 4.0, d_out_scores, d_out_ids, s,
        [&](const DenseSegment& seg, int64_t r0, int64_t r1) {
            DenseSplitArgs a{};
            for (int p = 0; p < 3; ++p) { a.D[p] = seg.pl[p].p; a.Q[p] = idx->qpl[p].p; }
            if (np == 0) {            // the certified filter: one fp16 plane product + the per-pair error term
                a.n_pairs = 1;
                a.pair_d[0] = 0; a.pair_q[0] = 0;
                a.D[0] = seg.fpl.p;
                a.upper_bound = 1;
                a.dxy = seg.fxy.p; a.qa = idx->qa.p; a.sd = seg.fsd; a.isd = seg.fisd;
                a.dxy_gmax = seg.fxy.p + 2 * seg.n;
                a.mask = opts.mask;
                a.mask_qoff = opts.mask_qoff;
            } else {                  // (d plane, q plane), smallest products first: the last three are bf16x3's
                a.n_pairs = np == 2 ? 3 : 6;
                const int pd[6] = {2, 0, 1, 1, 0, 0}, pq[6] = {0, 2, 1, 0, 1, 0};
                for (int i = 0; i < a.n_pairs; ++i) { a.pair_d[i] = pd[6 - a.n_pairs + i]; a.pair_q[i] = pq[6 - a.n_pairs + i]; }
            }
            a.row_begin = r0; a.row_end = r1; a.H = idx->dim; a.nq = (int)nq;
            a.tau = two ? f_tau_eff : ws.tau; a.cand_keys = ws.cand_keys; a.cand_count = ws.cand_count;
            a.cand_cap = ws.cand_cap; a.id_base = (uint32_t)seg.id_base; a.id_stride = (uint32_t)seg.id_stride;
            a.seg_cnt = ws.seg_n > 0 ? ws.seg_cnt : nullptr; a.seg_n = ws.seg_n; a.seg_off = ws.seg_off;
            return launch_dense_split(a, s);
        },
        [&]() {
            if (!two) return topk_compact(ws, nq, k, s);
            SR_TRY(topk_compact2(ws, nq, k, opts.k_inner, f_tau2, select_over, s));
            return launch_filter_tau(ws.tau, f_tau2, f_slack, f_tau_eff, nq, s);
        });
}

// HBM-bound regime (<= 64 queries): D straight to registers, chunks grow geometrically (64 Ki docs, x2 per launch)
static int dense_pass_stream(sr_dense_index* idx, const float* d_queries, int64_t nq, int k, float* d_out_scores, int64_t* d_out_ids,
                             int64_t cand_limit, hipStream_t s) {
    TopkWS& ws = idx->ws;
    int64_t cap = cand_limit / (8 * nq);
    if (cap > (1ll << 22)) cap = 1ll << 22;
    cap = (cap / 128) * 128;
    if (cap < 128) cap = 128;
    SR_TRY(ws.ensure(nq, k, cap));
    SR_TRY(topk_reset(ws, nq, s));
    return dense_scan(
        idx, ws, nq, k, 65536 < cap ? 65536 : cap, cap, (double)sr_dtype_size(idx->row_dtype), d_out_scores, d_out_ids, s,
        [&](const DenseSegment& seg, int64_t r0, int64_t r1) {
            DenseStreamArgs a;
            a.D = seg.rows; a.Q = d_queries; a.row_begin = r0; a.row_end = r1; a.H = idx->dim; a.nq = (int)nq;
            a.tau = ws.tau; a.cand_keys = ws.cand_keys; a.cand_count = ws.cand_count;
            a.cand_cap = ws.cand_cap; a.id_base = (uint32_t)seg.id_base; a.id_stride = (uint32_t)seg.id_stride;
            a.dtype = idx->row_dtype;
            return launch_dense_stream(a, s);
        },
        [&]() { return topk_compact(ws, nq, k, s); });
}

// the exact MFMA kernels (dense_score.hip); the re-do of a few queries keeps its own (differently shaped) workspace
static int dense_pass_tiled(sr_dense_index* idx, const float* d_queries, int64_t nq, int k, float* d_out_scores, int64_t* d_out_ids,
                            bool redo, int64_t cand_limit, hipStream_t s) {
    TopkWS& ws = redo ? idx->ws3 : idx->ws;
    const char* env_variant = sr_dev_getenv("SR_DENSE_VARIANT");   // A/B switch, read per call: 1 = plain double buffer instead of the pipelined kernel
    const bool plain = env_variant && atoi(env_variant) == 1;
    int64_t step0, chunk;
    dense_tiled_plan(nq, k, cand_limit, 2048, &step0, &chunk);
    SR_TRY(ws.ensure(nq, k, chunk));
    SR_TRY(topk_reset(ws, nq, s));
    return dense_scan(
        idx, ws, nq, k, step0, chunk, (double)sr_dtype_size(idx->row_dtype), d_out_scores, d_out_ids, s,
        [&](const DenseSegment& seg, int64_t r0, int64_t r1) {
            DenseArgs a;
            a.D = seg.rows; a.Q = d_queries; a.row_begin = r0; a.row_end = r1; a.H = idx->dim; a.nq = (int)nq;
            a.tau = ws.tau; a.cand_keys = ws.cand_keys; a.cand_count = ws.cand_count;
            a.cand_cap = ws.cand_cap; a.id_base = (uint32_t)seg.id_base; a.id_stride = (uint32_t)seg.id_stride;
            a.dtype = idx->row_dtype;
            return launch_dense_exact(a, r1 - r0, plain, s);
        },
        [&]() { return topk_compact(ws, nq, k, s); });
}

// one batch whose workspace fits the limit
static int dense_pass_batch(sr_dense_index* idx, const float* d_queries, int64_t nq, int k, float* d_out_scores, int64_t* d_out_ids,
                            const DensePassOpts& opts, hipStream_t s) {
    const int64_t cand_limit = idx->ws_limit - nq * (k > SR_MAX_TOPK ? topk_large_bytes_per_query(k) : 0);   // candidate buffer budget
    if (opts.arith != DenseArith::exact && nq > 64) return dense_pass_16bit(idx, d_queries, nq, k, d_out_scores, d_out_ids, opts, cand_limit, s);
    if (!opts.tiled_only && !idx->batch_invariant && dense_stream_supports((int)nq, idx->dim))
        return dense_pass_stream(idx, d_queries, nq, k, d_out_scores, d_out_ids, cand_limit, s);
    return dense_pass_tiled(idx, d_queries, nq, k, d_out_scores, d_out_ids, opts.tiled_only, cand_limit, s);
}

// k > SR_MAX_TOPK: the running set (2k keys per query) and the select's buffers count against the workspace limit next to
// the candidate buffer (at least one 256-doc tile per query).  A call that does not fit runs in query sub-batches of more
// than 64 queries each, so that every query stays in the kernel family (and k order) of the unsplit call: the bits do not
// depend on the limit.
int dense_search_pass(sr_dense_index* idx, const float* d_queries, int64_t nq, int k, float* d_out_scores, int64_t* d_out_ids,
                      const DensePassOpts& opts, hipStream_t s) {
    if (k > SR_MAX_TOPK) {
        const int64_t per_q = topk_large_bytes_per_query(k) + 8 * 256;
        const int64_t b_max = idx->ws_limit / per_q;
        if (b_max < nq) {
            int64_t nb = b_max >= 1 ? ceil_div64(nq, b_max) : 0;
            if (nb == 0 || nq / nb <= 64) {
                const int64_t smallest = nq <= 128 ? nq : 65;
                sr_set_error("dense search: k = %d needs %lld bytes of workspace for a batch of %lld queries (limit %lld bytes)", k,
                             (long long)(smallest * per_q), (long long)smallest, (long long)idx->ws_limit);
                return SR_ERR_NOMEM;
            }
            for (int64_t b = 0, q0 = 0; b < nb; ++b) {            // balanced: every batch holds floor(nq / nb) or one more queries
                const int64_t nqb = nq / nb + (b < nq % nb ? 1 : 0);
                SR_TRY(dense_pass_batch(idx, d_queries + q0 * idx->dim, nqb, k, d_out_scores + q0 * k, d_out_ids + q0 * k, opts, s));
                q0 += nqb;
            }
            return SR_OK;
        }
    }
    return dense_pass_batch(idx, d_queries, nq, k, d_out_scores, d_out_ids, opts, s);
}

// ---- SR_PRECISION_FP32_FILTERED: exact results at 16-bit MFMA speed (dense_filter.hip) --------------------------------------------
static void filter_segs_of(const sr_dense_index* idx, FilterSegs& fs) {
    fs.count = (int)idx->segs.size();
    fs.dtype = idx->row_dtype;
    for (int i = 0; i < fs.count; ++i) {
        fs.rows[i] = idx->segs[i].rows; fs.n[i] = idx->segs[i].n;
        fs.xy[i] = idx->segs[i].fxy.p; fs.isd[i] = idx->segs[i].fisd;
        fs.id_base[i] = (uint32_t)idx->segs[i].id_base; fs.id_stride[i] = (uint32_t)idx->segs[i].id_stride;
    }
}

// full_kp: the mask route of the subset searches, where max(3k, k + 2048) candidates must fit SR_MAX_TOPK as they are (k <= 1 365) - the
// unrestricted search goes on with a list cut to SR_MAX_TOPK, there a k beyond that is served by the gather route.
int dense_filter_applies(sr_dense_index* idx, int64_t nq, int k, int* kp_out, bool* applies, bool full_kp) {
    *applies = false;
    if (k > SR_MAX_TOPK) return SR_OK;                         // no room for k + 64 candidates in the in-LDS top-k
    int kp = 3 * k > k + 2048 ? 3 * k : k + 2048;            // candidates per query: k = 1000 -> 3072
    if (const char* e = sr_dev_getenv("SR_FILTER_KP")) kp = atoi(e);
    if (full_kp && kp > SR_MAX_TOPK) return SR_OK;
    if (kp > SR_MAX_TOPK) kp = SR_MAX_TOPK;
    if (nq <= 64 || kp < k + 64 || idx->dim % 64 != 0 || idx->dim < 128 || (int)idx->segs.size() > SR_FILTER_MAX_SEGS) return SR_OK;
    for (DenseSegment& seg : idx->segs) {
        if (seg.f_state == 0) SR_TRY(filter_prepare_segment(idx, seg));
        if (seg.f_state != 1) return SR_OK;                   // not filterable / no room for the plane: exact kernel
    }
    *kp_out = kp;
    *applies = true;
    return SR_OK;
}

int dense_filtered_candidates(sr_dense_index* idx, const float* d_queries, int64_t nq, int k, hipStream_t s, bool* done,
                              const uint32_t* d_mask, const uint32_t* d_mask_qoff) {
    *done = false;
    int kp = 0;
    bool applies = false;
    SR_TRY(dense_filter_applies(idx, nq, k, &kp, &applies));
    if (!applies) return SR_OK;
    if (idx->fq_cap < nq || idx->fkp != kp) {
        idx->qa.release(); idx->a_scores.release(); idx->a_ids.release(); idx->flags.release();
        idx->fq_cap = 0;
        if (idx->qa.reserve(nq * 7, nullptr) != SR_OK || idx->a_scores.reserve(nq * kp, nullptr) != SR_OK ||
            idx->a_ids.reserve(nq * kp, nullptr) != SR_OK || idx->flags.reserve(2 * nq + 2, nullptr) != SR_OK)
            return SR_OK;                                     // no room for the candidate lists: exact kernel
        idx->fq_cap = nq;
        idx->fkp = kp;
    }
    SR_CHECK_HIP(hipMemsetAsync(idx->flags.p, 0, (size_t)nq * 4, s));
    // 1. the kp documents with the largest upper bounds U (the query planes and constants are made by the pass)
    const DensePassOpts opts{DenseArith::filter_upper_bound, /*tiled_only=*/false, /*k_inner=*/k, d_mask, d_mask_qoff};
    SR_TRY(dense_search_pass(idx, d_queries, nq, kp, idx->a_scores.p, idx->a_ids.p, opts, s));
    *done = true;
    return SR_OK;
}

// the re-do buffers, sized for nf queries at this k (kept until a call needs more)
int dense_redo_reserve(sr_dense_index* idx, int64_t nf, int k) {
    if (idx->redo_cap >= nf && idx->redo_k == k) return SR_OK;
    idx->redo_q.release(); idx->redo_idx.release(); idx->redo_scores.release(); idx->redo_ids.release();
    idx->redo_cap = 0;
    const int64_t cap = nf < 64 ? 64 : nf;
    SR_TRY(idx->redo_q.reserve(cap * idx->dim, "dense search (re-do)"));
    SR_TRY(idx->redo_idx.reserve(cap, "dense search (re-do)"));
    SR_TRY(idx->redo_scores.reserve(cap * k, "dense search (re-do)"));
    SR_TRY(idx->redo_ids.reserve(cap * k, "dense search (re-do)"));
    idx->redo_cap = cap;
    idx->redo_k = k;
    return SR_OK;
}

// d_list: queries without a certificate are re-done by the gather kernel over that list, whose chains are the exact kernel's
// (subset_search.hip): the same bits, no masked exact kernel.  redo_out: they are handed back instead (the grouped search re-does each
// under its own group's list).
int dense_filtered_finish(sr_dense_index* idx, const float* d_queries, int64_t nq, int k, const float* d_thr, float* d_out_scores,
                          int64_t* d_out_ids, hipStream_t s, const int64_t* d_list, int64_t m, std::vector<int64_t>* redo_out) {
    const int kp = idx->fkp;
    int* const flags = idx->flags.p;
    FilterSegs fs;
    filter_segs_of(idx, fs);
    // 2. exact scores of the candidates that can still be in the top-k -> exact top-k
    SR_TRY(idx->ws2.ensure(nq, k, kp));
    SR_TRY(topk_reset(idx->ws2, nq, s));
    SR_TRY(launch_filter_rescore(fs, d_queries, idx->a_scores.p, idx->a_ids.p, idx->qa.p, nq, k, kp, idx->dim, idx->ws2.cand_keys,
                                 idx->ws2.cand_count, idx->ws2.cand_cap, flags, reinterpret_cast<unsigned int*>(flags) + nq + 1, d_thr, s));
    SR_TRY(topk_compact(idx->ws2, nq, k, s));
    SR_TRY(topk_finalize(idx->ws2, nq, k, -3.402823466e38f, d_out_scores, d_out_ids, nullptr, s));
    // 3. certificate against the k-th exact score
    SR_TRY(launch_filter_certify(idx->a_scores.p, d_out_scores, idx->qa.p, nq, k, kp, flags, d_thr, s));
    // the queries that were not certified are re-done by the exact kernel - those alone (one small D2H per search)
    std::vector<int> h((size_t)nq);
    SR_CHECK_HIP(hipMemcpyAsync(h.data(), flags, (size_t)nq * 4, hipMemcpyDeviceToHost, s));
    SR_CHECK_HIP(hipStreamSynchronize(s));
    std::vector<int64_t> redo;
    for (int64_t q = 0; q < nq; ++q)
        if (h[(size_t)q] != 0) redo.push_back(q);
    const int64_t nf = (int64_t)redo.size();
    idx->nq_certified += nq - nf;
    idx->nq_redone += nf;
    if (nf == 0) { ++idx->n_filtered; return SR_OK; }
    ++idx->n_fallback;
    if (redo_out) { redo_out->swap(redo); return SR_OK; }     // grouped search: every query is re-done under its own group's list
    if (nf * 2 > nq) {                                         // most of the batch: redo all of it in place
        if (d_list) return dense_subset_gather(idx, d_queries, nq, k, d_list, m, d_out_scores, d_out_ids, s, "dense search (masked)");
        return dense_search_pass(idx, d_queries, nq, k, d_out_scores, d_out_ids, DensePassOpts{}, s);
    }
    SR_TRY(dense_redo_reserve(idx, nf, k));
    SR_CHECK_HIP(hipMemcpyAsync(idx->redo_idx.p, redo.data(), (size_t)nf * 8, hipMemcpyHostToDevice, s));
    SR_TRY(launch_filter_gather_rows(d_queries, idx->redo_idx.p, nf, idx->dim, idx->redo_q.p, false, s));
    // the tiled kernels whatever the count: one k order for the whole batch (the streaming kernel accumulates in another)
    if (d_list) SR_TRY(dense_subset_gather(idx, idx->redo_q.p, nf, k, d_list, m, idx->redo_scores.p, idx->redo_ids.p, s, "dense search (masked)"));
    else SR_TRY(dense_search_pass(idx, idx->redo_q.p, nf, k, idx->redo_scores.p, idx->redo_ids.p, DensePassOpts{DenseArith::exact, /*tiled_only=*/true}, s));
    SR_TRY(launch_filter_gather_rows(idx->redo_scores.p, idx->redo_idx.p, nf, k, d_out_scores, true, s));
    SR_TRY(launch_filter_gather_rows(idx->redo_ids.p, idx->redo_idx.p, nf, 2 * (int64_t)k, d_out_ids, true, s));
    SR_CHECK_HIP(hipStreamSynchronize(s));                    // `redo` (pageable host memory) is the source of an async copy
    return SR_OK;
}

// A k above SR_MAX_TOPK is served while the rows it asks for hold at most SR_MAX_TOPK entries of padding (k <= ntotal + SR_MAX_TOPK):
// a search of more rows than the index holds documents is still rejected there, as it was before the large-k path existed.
static bool dense_k_fits(const sr_dense_index* idx, int k) { return k <= SR_MAX_TOPK || (int64_t)k - SR_MAX_TOPK <= idx->ntotal; }

static DenseArith dense_arith_of(int precision) {
    return precision == SR_PRECISION_BF16X3 ? DenseArith::bf16x3 : (precision == SR_PRECISION_BF16X6 ? DenseArith::bf16x6 : DenseArith::exact);
}

extern "C" int sr_dense_search(sr_dense_index* idx, const float* d_queries, int64_t nq, int k, float* d_out_scores,
                               int64_t* d_out_ids, sr_stream stream) {
    SR_REQUIRE(idx, "sr_dense_search: null index");
    SR_REQUIRE(nq >= 0 && nq < (1ll << 30), "sr_dense_search: bad nq=%lld", (long long)nq);
    SR_REQUIRE(k >= 1 && k <= SR_MAX_TOPK_LARGE, "sr_dense_search: k=%d outside [1, %d]", k, SR_MAX_TOPK_LARGE);
    SR_REQUIRE(dense_k_fits(idx, k), "sr_dense_search: k=%d exceeds %d by more than the index's %lld documents", k, SR_MAX_TOPK,
               (long long)idx->ntotal);
    if (nq == 0) return SR_OK;
    SR_REQUIRE(d_queries && d_out_scores && d_out_ids, "sr_dense_search: null pointer");
    SR_REQUIRE(((uintptr_t)d_queries & 15) == 0, "sr_dense_search: queries must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(idx->mu);
    StreamOrder::Scope in_order(idx->order, s);
    if (idx->precision == SR_PRECISION_FP32_FILTERED) {
        bool done = false;
        SR_TRY(dense_filtered_candidates(idx, d_queries, nq, k, s, &done));
        if (done) return dense_filtered_finish(idx, d_queries, nq, k, nullptr, d_out_scores, d_out_ids, s);
        if (nq > 64 && k <= SR_MAX_TOPK) { ++idx->n_fallback; idx->nq_redone += nq; }   // a larger k was never eligible
    }
    return dense_search_pass(idx, d_queries, nq, k, d_out_scores, d_out_ids, DensePassOpts{dense_arith_of(idx->precision)}, s);
}

// Doc-sharded search in two halves (distributed.py ShardedDenseRetriever): every rank runs _begin on its shard, the ranks take
// the minimum of d_lower over the shards (nq floats, one small all-reduce), every rank runs _finish with it.  A shard then
// re-scores only the candidates that can reach the GLOBAL top-k - about k / W of them instead of k - and returns those (the
// rest of its [nq, k] output is padding, id -1): the merge of the shards' outputs is the global top-k, bit for bit what one
// index over all documents returns.  `share` = the number of shards W.  When the certified filter does not apply (exact
// precision mode, <= 64 queries, no room for the plane) d_lower is -inf and _finish is a plain sr_dense_search.  The pair must
// not be interleaved with other searches on the same handle.
extern "C" int sr_dense_search_begin(sr_dense_index* idx, const float* d_queries, int64_t nq, int k, int share, float* d_lower,
                                     sr_stream stream) {
    SR_REQUIRE(idx && d_lower, "sr_dense_search_begin: null argument");
    SR_REQUIRE(nq >= 0 && nq < (1ll << 30) && k >= 1 && k <= SR_MAX_TOPK_LARGE && share >= 1, "sr_dense_search_begin: bad argument");
    SR_REQUIRE(dense_k_fits(idx, k), "sr_dense_search_begin: k=%d exceeds %d by more than the index's %lld documents", k, SR_MAX_TOPK,
               (long long)idx->ntotal);
    if (nq == 0) return SR_OK;
    SR_REQUIRE(d_queries && ((uintptr_t)d_queries & 15) == 0, "sr_dense_search_begin: queries must be non-null and 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(idx->mu);
    StreamOrder::Scope in_order(idx->order, s);
    idx->pend_nq = 0;
    bool done = false;
    if (idx->precision == SR_PRECISION_FP32_FILTERED) SR_TRY(dense_filtered_candidates(idx, d_queries, nq, k, s, &done));
    if (!done) {
        std::vector<float> h((size_t)nq, -INFINITY);
        SR_CHECK_HIP(hipMemcpyAsync(d_lower, h.data(), (size_t)nq * 4, hipMemcpyHostToDevice, s));
        SR_CHECK_HIP(hipStreamSynchronize(s));
        return SR_OK;
    }
    FilterSegs fs;
    filter_segs_of(idx, fs);
    int j = (k + share - 1) / share;
    if (j > idx->fkp) j = idx->fkp;
    SR_TRY(launch_filter_lower_bound(fs, d_queries, idx->a_scores.p, idx->a_ids.p, idx->qa.p, nq, idx->fkp, j, idx->dim, idx->flags.p,
                                     reinterpret_cast<unsigned int*>(idx->flags.p) + nq + 1, d_lower, s));
    idx->pend_nq = nq; idx->pend_k = k; idx->pend_q = d_queries;
    return SR_OK;
}

extern "C" int sr_dense_search_finish(sr_dense_index* idx, const float* d_queries, int64_t nq, int k, const float* d_threshold,
                                      float* d_out_scores, int64_t* d_out_ids, sr_stream stream) {
    SR_REQUIRE(idx, "sr_dense_search_finish: null index");
    if (nq == 0) return SR_OK;
    SR_REQUIRE(d_queries && d_out_scores && d_out_ids, "sr_dense_search_finish: null pointer");
    bool pending;
    {
        std::lock_guard<std::mutex> lock(idx->mu);
        pending = idx->pend_nq == nq && idx->pend_k == k && idx->pend_q == d_queries && nq > 0;
        idx->pend_nq = 0;
        if (pending) {
            hipStream_t s = (hipStream_t)stream;
            StreamOrder::Scope in_order(idx->order, s);
            return dense_filtered_finish(idx, d_queries, nq, k, d_threshold, d_out_scores, d_out_ids, s);
        }
    }
    return sr_dense_search(idx, d_queries, nq, k, d_out_scores, d_out_ids, stream);
}
