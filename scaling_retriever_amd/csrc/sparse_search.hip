// sr_sparse_search (gfx950): which scorer serves a call - the certified two-stage scorer (sparse_cert.hip) where the index has one and
// k leaves room for its band of extra keys, else the exact kernels (sparse_score.hip) - and the re-do of the queries the certified
// scorer hands back.
#include "sparse_index.h"
#include <algorithm>
#include <vector>

// ---- queries the certified scorer hands back: their rows are gathered into a CSR of their own, scored by the exact kernels and
// scattered into the result rows
__global__ void sparse_sub_gather_kernel(const int64_t* __restrict__ q_indptr, const int32_t* __restrict__ q_cols, const float* __restrict__ q_vals,
                                         const int64_t* __restrict__ sel, const int64_t* __restrict__ sub_indptr, int32_t* __restrict__ sub_cols,
                                         float* __restrict__ sub_vals) {
    const int64_t j = blockIdx.x;
    const int64_t q = sel[j];
    const int64_t b = q_indptr[q], n = q_indptr[q + 1] - b, o = sub_indptr[j];
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
        sub_cols[o + i] = q_cols[b + i];
        sub_vals[o + i] = q_vals[b + i];
    }
}
__global__ void sparse_sub_scatter_kernel(const int64_t* __restrict__ sel, int k, const float* __restrict__ s_in, const int64_t* __restrict__ i_in,
                                          const int32_t* __restrict__ c_in, float* __restrict__ s_out, int64_t* __restrict__ i_out,
                                          int32_t* __restrict__ c_out) {
    const int64_t j = blockIdx.x;
    const int64_t q = sel[j];
    for (int i = threadIdx.x; i < k; i += blockDim.x) {
        s_out[q * k + i] = s_in[j * k + i];
        i_out[q * k + i] = i_in[j * k + i];
    }
    if (c_out && threadIdx.x == 0) c_out[q] = c_in[j];
}

// The queries of `call` that d_uncert flags, through the exact kernels.  wide_band > 0 (and at least SR_CERT_RETRY_MIN queries handed
// back): the sub-batch first goes through the certified scorer once more with that many keys beyond k - a certificate that failed for
// want of room is then usually given - and only what it hands back again reaches the exact kernels.  filt (null: the whole collection):
// the search runs under a document filter - the second pass under its bitmap, and the exact kernels are the list routes of
// sr_sparse_search_subset over its list, which rank the allowed documents only.
#define SR_CERT_RETRY_MIN 256
static int sparse_redo_exact(sr_sparse_index* idx, const SparseCall& call, const uint8_t* d_uncert, int wide_band, SparseDocFilter* filt,
                             hipStream_t s) {
    const int64_t nq = call.nq;
    std::vector<uint8_t> h_un((size_t)nq);
    std::vector<int64_t> h_ip((size_t)nq + 1);
    SR_CHECK_HIP(hipMemcpyAsync(h_un.data(), d_uncert, (size_t)nq, hipMemcpyDeviceToHost, s));
    SR_CHECK_HIP(hipMemcpyAsync(h_ip.data(), call.q_indptr, sizeof(int64_t) * ((size_t)nq + 1), hipMemcpyDeviceToHost, s));
    SR_CHECK_HIP(hipStreamSynchronize(s));
    std::vector<int64_t> sel, sub_ip(1, 0);
    for (int64_t q = 0; q < nq; ++q)
        if (h_un[(size_t)q]) {
            sel.push_back(q);
            sub_ip.push_back(sub_ip.back() + (h_ip[(size_t)q + 1] - h_ip[(size_t)q]));
        }
    const int64_t ns = (int64_t)sel.size();
    if (ns == 0) return SR_OK;
    if (filt) SR_TRY(sparse_filter_need_list(idx, filt, s));
    const int64_t nnz = sub_ip.back() > 0 ? sub_ip.back() : 1;
    CallBuf<int64_t> d_sel, d_sip, d_ids;
    CallBuf<int32_t> d_cols, d_cnt;
    CallBuf<float> d_vals, d_sc;
    CallBuf<uint8_t> d_un2;
    if (d_sel.reserve(ns, nullptr) != SR_OK || d_sip.reserve(ns + 1, nullptr) != SR_OK || d_cols.reserve(nnz, nullptr) != SR_OK ||
        d_vals.reserve(nnz, nullptr) != SR_OK || d_sc.reserve(ns * call.k, nullptr) != SR_OK || d_ids.reserve(ns * call.k, nullptr) != SR_OK ||
        d_cnt.reserve(ns, nullptr) != SR_OK) {
        sr_set_error("sr_sparse_search: out of device memory for %lld re-done queries", (long long)ns);
        return SR_ERR_NOMEM;
    }
    // the handed-back queries as a call of their own: a CSR gathered from the caller's, result rows scattered back below
    SparseCall sub = call;
    sub.q_indptr = d_sip.p; sub.q_cols = d_cols.p; sub.q_vals = d_vals.p; sub.nq = ns;
    sub.out_scores = d_sc.p; sub.out_ids = d_ids.p; sub.out_counts = d_cnt.p;
    int rc = SR_OK;
    if (hipMemcpyAsync(d_sel.p, sel.data(), 8 * (size_t)ns, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(d_sip.p, sub_ip.data(), 8 * ((size_t)ns + 1), hipMemcpyHostToDevice, s) != hipSuccess)
        rc = SR_ERR_HIP;
    if (rc == SR_OK) {
        hipLaunchKernelGGL(sparse_sub_gather_kernel, dim3((unsigned)ns), dim3(64), 0, s, call.q_indptr, call.q_cols, call.q_vals, d_sel.p, d_sip.p,
                           d_cols.p, d_vals.p);
        bool done = false;
        if (wide_band > 0 && ns >= SR_CERT_RETRY_MIN && idx->cert && d_un2.reserve(ns, nullptr) == SR_OK) {
            SparseCertOptions opt;
            opt.uncert = d_un2.p; opt.band_keys = wide_band; opt.mask_pad = filt ? filt->mask_pad : nullptr;
            SparseCertResult res;
            rc = sparse_cert_search(idx, sub, opt, &res, s);
            if (rc == SR_OK && !res.no_memory) {
                ++idx->n_cert_retries;
                sparse_cert_count_retry(idx->cert, ns);
                if (res.n_uncert > 0) rc = sparse_redo_exact(idx, sub, d_un2.p, 0, filt, s);
                done = true;
            }
            if (hipStreamSynchronize(s) != hipSuccess && rc == SR_OK) rc = SR_ERR_HIP;
        }
        if (rc == SR_OK && !done)
            rc = filt ? sparse_subset_lists(idx, sub, filt->list, filt->m, subset_sparse_use_array(filt->m, idx->n_docs), s, filt->who)
                      : sparse_exact_search(idx, sub, s);
    }
    if (rc == SR_OK) {
        hipLaunchKernelGGL(sparse_sub_scatter_kernel, dim3((unsigned)ns), dim3(256), 0, s, d_sel.p, call.k, d_sc.p, d_ids.p, d_cnt.p, call.out_scores,
                           call.out_ids, call.out_counts);
        if (hipGetLastError() != hipSuccess) rc = SR_ERR_HIP;
    }
    if (hipStreamSynchronize(s) != hipSuccess && rc == SR_OK) rc = SR_ERR_HIP;      // the temporaries go when this returns
    if (rc == SR_ERR_HIP) sr_set_error("sr_sparse_search: re-doing uncertified queries failed: %s", hipGetErrorString(hipGetLastError()));
    return rc;
}

// certified two-stage scorer (sparse_cert.hip) where the index has one and k leaves room for its band of extra keys.  Dev switch
// SR_SPARSE_CERT_SEARCH=0: exact kernels only (A/B)
bool sparse_cert_applies(const sr_sparse_index* idx, int k) {
    bool use_cert = idx->cert != nullptr && k + 1024 <= SR_MAX_TOPK;
    {
        const char* forced = sr_dev_getenv("SR_SPARSE_CERT");        // 1: also on collections too small for it to pay (tests)
        if (!(forced && atoi(forced) == 1)) use_cert = use_cert && idx->n_docs >= 8ll * (k + 1024);
    }
    if (const char* e = sr_dev_getenv("SR_SPARSE_CERT_SEARCH")) use_cert = use_cert && atoi(e) != 0;
    return use_cert;
}

// ---- a bitmap per query (sr_sparse_search_grouped): the queries of a call group by group, each group under its own bitmap
int sparse_grouped_each(sr_sparse_index* idx, const SparseCall& call, const SparseGroups& groups, const uint8_t* h_flags, bool lists_only, hipStream_t s) {
    const int64_t nq = call.nq;
    const int32_t* grp = groups.h_group + groups.q0;
    std::vector<int64_t> sel;                                // the chosen queries by group (a stable sort: ascending inside a group)
    for (int64_t q = 0; q < nq; ++q)
        if (!h_flags || h_flags[q]) sel.push_back(q);
    if (sel.empty()) return SR_OK;
    std::stable_sort(sel.begin(), sel.end(), [&](int64_t a, int64_t b) { return grp[a] < grp[b]; });
    std::vector<int64_t> h_ip((size_t)nq + 1);
    SR_CHECK_HIP(hipMemcpyAsync(h_ip.data(), call.q_indptr, sizeof(int64_t) * ((size_t)nq + 1), hipMemcpyDeviceToHost, s));
    SR_CHECK_HIP(hipStreamSynchronize(s));
    const int64_t ns_all = (int64_t)sel.size();
    std::vector<int64_t> sub_ip((size_t)ns_all + 1, 0);      // one CSR over all chosen queries in `sel` order; a group is a run of its rows
    for (int64_t j = 0; j < ns_all; ++j) sub_ip[(size_t)j + 1] = sub_ip[(size_t)j] + (h_ip[(size_t)sel[(size_t)j] + 1] - h_ip[(size_t)sel[(size_t)j]]);
    const int64_t nnz = sub_ip.back() > 0 ? sub_ip.back() : 1;
    CallBuf<int64_t> d_sel, d_sip, d_ids;
    CallBuf<int32_t> d_cols, d_cnt;
    CallBuf<float> d_vals, d_sc;
    if (d_sel.reserve(ns_all, nullptr) != SR_OK || d_sip.reserve(ns_all + 1, nullptr) != SR_OK || d_cols.reserve(nnz, nullptr) != SR_OK ||
        d_vals.reserve(nnz, nullptr) != SR_OK || d_sc.reserve(ns_all * call.k, nullptr) != SR_OK || d_ids.reserve(ns_all * call.k, nullptr) != SR_OK ||
        d_cnt.reserve(ns_all, nullptr) != SR_OK) {
        sr_set_error("%s: out of device memory for %lld queries searched group by group", groups.who, (long long)ns_all);
        return SR_ERR_NOMEM;
    }
    int rc = SR_OK;
    if (hipMemcpyAsync(d_sel.p, sel.data(), 8 * (size_t)ns_all, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(d_sip.p, sub_ip.data(), 8 * ((size_t)ns_all + 1), hipMemcpyHostToDevice, s) != hipSuccess)
        rc = SR_ERR_HIP;
    if (rc == SR_OK) {
        hipLaunchKernelGGL(sparse_sub_gather_kernel, dim3((unsigned)ns_all), dim3(64), 0, s, call.q_indptr, call.q_cols, call.q_vals, d_sel.p, d_sip.p,
                           d_cols.p, d_vals.p);
        if (hipGetLastError() != hipSuccess) rc = SR_ERR_HIP;
    }
    for (int64_t j0 = 0; rc == SR_OK && j0 < ns_all;) {
        const int64_t g = grp[sel[(size_t)j0]];
        int64_t j1 = j0;
        while (j1 < ns_all && grp[sel[(size_t)j1]] == g) ++j1;
        // rows [j0, j1) of the gathered CSR as a call of their own (SparseCall::rows: q_indptr moves, cols / vals stay)
        SparseCall sub = call;
        sub.q_indptr = d_sip.p + j0; sub.q_cols = d_cols.p; sub.q_vals = d_vals.p; sub.nq = j1 - j0;
        sub.out_scores = d_sc.p + j0 * call.k; sub.out_ids = d_ids.p + j0 * call.k; sub.out_counts = d_cnt.p + j0;
        const uint32_t* words = groups.words + g * groups.n_words;
        rc = lists_only ? sparse_masked_lists(idx, sub, words, groups.h_count[g], s, groups.who) : sparse_masked_body(idx, sub, words, s, groups.who);
        j0 = j1;
    }
    if (rc == SR_OK) {
        hipLaunchKernelGGL(sparse_sub_scatter_kernel, dim3((unsigned)ns_all), dim3(256), 0, s, d_sel.p, call.k, d_sc.p, d_ids.p, d_cnt.p, call.out_scores,
                           call.out_ids, call.out_counts);
        if (hipGetLastError() != hipSuccess) rc = SR_ERR_HIP;
    }
    if (hipStreamSynchronize(s) != hipSuccess && rc == SR_OK) rc = SR_ERR_HIP;      // the temporaries (and `sel`, a copy's source) go when this returns
    if (rc == SR_ERR_HIP) sr_set_error("%s: searching group by group failed: %s", groups.who, hipGetErrorString(hipGetLastError()));
    return rc;
}

int sparse_certified_search(sr_sparse_index* idx, const SparseCall& call, SparseDocFilter* filt, hipStream_t s, const SparseGroups* groups) {
    // The scorer's workspace is ~200 KB per query: the query set goes through in batches (a whole MSMARCO-Dev set is one batch), and
    // a batch whose buffers do not fit in device memory is served by the exact kernels instead of failing the call; the queries it
    // cannot certify are re-done by the exact kernels.
    int64_t batch = SR_CERT_QUERY_BATCH;
    if (const char* e = sr_dev_getenv("SR_SPARSE_CERT_BATCH")) batch = std::max<int64_t>(32, atoll(e) / 32 * 32);   // tests: several batches on small inputs
    SparseCertOptions opt;
    opt.uncert = sparse_cert_uncert_buffer(idx->cert, call.nq < batch ? call.nq : batch);
    opt.mask_pad = filt ? filt->mask_pad : nullptr;
    if (groups) { opt.mask_pad = groups->union_pad; opt.group_pad = groups->group_pad; }
    for (int64_t qb = 0; qb < call.nq; qb += batch) {
        const SparseCall part = call.rows(qb, call.nq - qb < batch ? call.nq - qb : batch);
        SparseCertResult res;
        res.no_memory = opt.uncert == nullptr || (filt && filt->mask_pad == nullptr) || (groups && groups->group_pad == nullptr);
        if (groups) {
            // a batch (a multiple of 32 queries) walks its own slice of the word offsets.  What it hands back - or all of it, if its buffers
            // do not fit - is re-done under each query's OWN group's list, group by group, and goes straight there: a second, wider-band pass
            // would need the gathered queries' offsets and a scorer call per retry, for the few queries a grouped pass hands back
            SparseGroups part_groups = *groups;
            part_groups.q0 = groups->q0 + qb;
            opt.qoff = groups->qoff ? groups->qoff + qb : nullptr;
            if (sr_dev_getenv("SR_SPARSE_CERT_FAKE_OOM")) res.no_memory = true;
            if (!res.no_memory) SR_TRY(sparse_cert_search(idx, part, opt, &res, s));
            if (res.no_memory) {
                ++idx->n_cert_no_memory;
                SR_TRY(sparse_grouped_each(idx, part, part_groups, nullptr, true, s));
            } else if (res.n_uncert > 0) {
                std::vector<uint8_t> h_un((size_t)part.nq);
                SR_CHECK_HIP(hipMemcpyAsync(h_un.data(), opt.uncert, (size_t)part.nq, hipMemcpyDeviceToHost, s));
                SR_CHECK_HIP(hipStreamSynchronize(s));
                SR_TRY(sparse_grouped_each(idx, part, part_groups, h_un.data(), true, s));
            }
            continue;
        }
        if (sr_dev_getenv("SR_SPARSE_CERT_FAKE_OOM")) res.no_memory = true;          // tests: the fallback below
        if (!res.no_memory) SR_TRY(sparse_cert_search(idx, part, opt, &res, s));
        if (res.no_memory) {
            ++idx->n_cert_no_memory;
            if (filt) {
                SR_TRY(sparse_filter_need_list(idx, filt, s));
                SR_TRY(sparse_subset_lists(idx, part, filt->list, filt->m, subset_sparse_use_array(filt->m, idx->n_docs), s, filt->who));
            } else {
                SR_TRY(sparse_exact_search(idx, part, s));
            }
        } else if (res.n_uncert > 0) {
            // many queries handed back under a band that could still grow: once more through the scorer with the widest band, then the exact kernels
            const int widest = SR_MAX_TOPK - call.k;           // worth a second pass only if it at least doubles the band
            SR_TRY(sparse_redo_exact(idx, part, opt.uncert, 2 * res.band_used <= widest ? widest : 0, filt, s));
        }
    }
    return SR_OK;
}

extern "C" int sr_sparse_search(sr_sparse_index* idx, const int64_t* d_q_indptr, const int32_t* d_q_cols,
                                const float* d_q_vals, int64_t nq, int k, float threshold, int64_t id_base,
                                int64_t id_stride, float* d_out_scores, int64_t* d_out_ids, int32_t* d_out_counts,
                                sr_stream stream) {
    SR_REQUIRE(idx, "sr_sparse_search: null index");
    SR_REQUIRE(nq >= 0 && nq < (1ll << 30), "sr_sparse_search: bad nq");
    SR_REQUIRE(k >= 1 && k <= SR_MAX_TOPK_LARGE, "sr_sparse_search: k=%d outside [1, %d]", k, SR_MAX_TOPK_LARGE);
    SR_REQUIRE(id_stride >= 1 && id_base >= 0 && id_base + (idx->n_docs - 1) * id_stride < 0xffffffffll,
               "sr_sparse_search: global doc index exceeds 32 bits");
    if (nq == 0) return SR_OK;
    SR_REQUIRE(d_q_indptr && d_out_scores && d_out_ids, "sr_sparse_search: null pointer");
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(idx->mu);
    StreamOrder::Scope in_order(idx->order, s);
    const SparseCall call{d_q_indptr, d_q_cols, d_q_vals, nq, k, threshold, id_base, id_stride, d_out_scores, d_out_ids, d_out_counts};
    return sparse_cert_applies(idx, k) ? sparse_certified_search(idx, call, nullptr, s) : sparse_exact_search(idx, call, s);
}
