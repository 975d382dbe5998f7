// The sparse index handle (gfx950): what sr_sparse_index_create builds for the exact scorer - validation, the skip table, the dense
// columns of the heavy terms - its destruction, and the statistics / measurement hooks.  The kernels that score are in
// sparse_score.hip, the certified scorer's side structures in sparse_cert_build.hip.
#include "sparse_index.h"
#include <algorithm>
#include <utility>
#include <vector>

#define SP_TILE SR_SPARSE_TILE_DOCS
#define SP_SUB SR_SPARSE_SKIP_DOCS

// dense column of a heavy term: column[slot][doc] = value (the buffer is zero-filled first)
__global__ void sparse_dense_fill_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ doc_ids,
                                         const float* __restrict__ vals, const int32_t* __restrict__ slot_term,
                                         int64_t stride, float* __restrict__ dense) {
    const int slot = blockIdx.y;
    const int64_t t = slot_term[slot];
    const int64_t b = indptr[t], e = indptr[t + 1];
    float* col = dense + (int64_t)slot * stride;
    for (int64_t pp = b + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; pp < e; pp += (int64_t)gridDim.x * blockDim.x)
        col[doc_ids[pp]] = vals[pp];
}

// ---- index build: skip table + validation -----------------------------------
// skip[t][b] = number of postings of term t with doc id < b * SP_SUB  (lower bound); n_sub entries + 1 per term
__global__ void sparse_skip_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ doc_ids,
                                   int64_t n_terms, int n_sub, int32_t* __restrict__ skip) {
    const int64_t t = blockIdx.x;
    const int64_t b = indptr[t], e = indptr[t + 1];
    const int64_t len = e - b;
    const int n_tiles = n_sub;
    for (int tile = threadIdx.x; tile <= n_tiles; tile += blockDim.x) {
        const int64_t bound = (int64_t)tile * SP_SUB;
        int64_t lo = 0, hi = len;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t)doc_ids[b + mid] < bound) lo = mid + 1; else hi = mid;
        }
        skip[t * (n_tiles + 1) + tile] = (int32_t)lo;
    }
}

// flags[0] |= 1 if a posting list is not strictly ascending, |= 2 if a doc id is out of range,
// |= 4 if indptr is not monotone
__global__ void sparse_validate_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ doc_ids,
                                       int64_t n_terms, int64_t n_docs, int* __restrict__ flags) {
    const int64_t t = blockIdx.x;
    const int64_t b = indptr[t], e = indptr[t + 1];
    if (e < b) { if (threadIdx.x == 0) atomicOr(flags, 4); return; }
    int bad = 0;
    for (int64_t p = b + threadIdx.x; p < e; p += blockDim.x) {
        const int32_t d = doc_ids[p];
        if (d < 0 || (int64_t)d >= n_docs) bad |= 2;
        if (p > b && doc_ids[p - 1] >= d) bad |= 1;
    }
    if (bad) atomicOr(flags, bad);
}

// Terms present in at least 1 / SP_DENSE_DIV of the docs get a dense column: the longest lists first, at most SP_DENSE_MAX of
// them and never more than a quarter of the free device memory (a column costs 4 B per doc, the list it shadows 8 B per
// posting; measured at MSMARCO shape, thresholds of 1/3 .. 1/8 of the docs are within 2 % of each other, 1/2 is 5 % slower).
// No such term: the query-block kernel is not used.
#define SP_DENSE_DIV 4
#define SP_DENSE_MAX 64
static int sparse_build_dense(sr_sparse_index* idx, hipStream_t s) {
    std::vector<int64_t> h_indptr((size_t)idx->n_terms + 1);
    SR_CHECK_HIP(hipMemcpyAsync(h_indptr.data(), idx->indptr, sizeof(int64_t) * h_indptr.size(), hipMemcpyDeviceToHost, s));
    SR_CHECK_HIP(hipStreamSynchronize(s));
    std::vector<std::pair<int64_t, int32_t>> heavy;   // (-length, term)
    for (int64_t t = 0; t < idx->n_terms; ++t) {
        const int64_t len = h_indptr[(size_t)t + 1] - h_indptr[(size_t)t];
        if (len > 0 && len * SP_DENSE_DIV >= idx->n_docs) heavy.emplace_back(-len, (int32_t)t);
    }
    if (heavy.empty()) return SR_OK;
    std::sort(heavy.begin(), heavy.end());
    const int64_t stride = (int64_t)idx->n_tiles * SP_TILE;
    size_t free_b = 0, total_b = 0;
    SR_CHECK_HIP(hipMemGetInfo(&free_b, &total_b));
    int64_t fit = (int64_t)(free_b / 4) / (stride * 4);       // at most a quarter of what is free
    int n = (int)heavy.size();
    if (n > SP_DENSE_MAX) n = SP_DENSE_MAX;
    if (n > fit) n = (int)fit;
    if (n <= 0) return SR_OK;
    std::vector<int32_t> h_slot((size_t)idx->n_terms, -1), h_terms((size_t)n);
    for (int i = 0; i < n; ++i) {
        h_slot[(size_t)heavy[(size_t)i].second] = i;
        h_terms[(size_t)i] = heavy[(size_t)i].second;
    }
    DeviceBuf<int32_t> d_terms;       // released on every path below
    if (idx->dense.reserve(stride * n, nullptr) != SR_OK || idx->dense_slot.reserve(idx->n_terms, nullptr) != SR_OK ||
        d_terms.reserve(n, nullptr) != SR_OK) {
        // columns are an optimisation: without them the per-query kernel serves every block
        idx->dense.release();
        idx->dense_slot.release();
        d_terms.release();
        return SR_OK;
    }
    int rc = SR_OK;
    if (hipMemsetAsync(idx->dense.p, 0, sizeof(float) * (size_t)stride * (size_t)n, s) != hipSuccess ||
        hipMemcpyAsync(idx->dense_slot.p, h_slot.data(), sizeof(int32_t) * h_slot.size(), hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(d_terms.p, h_terms.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s) != hipSuccess) {
        rc = SR_ERR_HIP;
    } else {
        hipLaunchKernelGGL(sparse_dense_fill_kernel, dim3(256, (unsigned)n), dim3(256), 0, s, idx->indptr, idx->doc_ids, idx->vals,
                           d_terms.p, stride, idx->dense.p);
        if (hipStreamSynchronize(s) != hipSuccess) rc = SR_ERR_HIP;
    }
    d_terms.release();
    if (rc != SR_OK) {
        sr_set_error("sr_sparse_index_create: building the dense columns failed: %s", hipGetErrorString(hipGetLastError()));
        return rc;
    }
    idx->n_dense = n;
    idx->dense_stride = stride;
    return SR_OK;
}

// validation and the skip table; *d_flags is the caller's to release
static int sparse_build_skip(sr_sparse_index* idx, DeviceBuf<int>* d_flags, hipStream_t s) {
    const int n_sub = idx->n_tiles * (SP_TILE / SP_SUB);
    if (idx->skip.reserve(idx->n_terms * (int64_t)(n_sub + 1), nullptr) != SR_OK || d_flags->reserve(1, nullptr) != SR_OK) {
        sr_set_error("sr_sparse_index_create: out of device memory for the skip table (%lld x %d)", (long long)idx->n_terms,
                     idx->n_tiles + 1);
        return SR_ERR_NOMEM;
    }
    int h_flags = 0;
    if (hipMemsetAsync(d_flags->p, 0, sizeof(int), s) != hipSuccess) return SR_ERR_HIP;
    hipLaunchKernelGGL(sparse_validate_kernel, dim3((unsigned)idx->n_terms), dim3(256), 0, s, idx->indptr, idx->doc_ids, idx->n_terms,
                       idx->n_docs, d_flags->p);
    hipLaunchKernelGGL(sparse_skip_kernel, dim3((unsigned)idx->n_terms), dim3(64), 0, s, idx->indptr, idx->doc_ids, idx->n_terms, n_sub,
                       idx->skip.p);
    if (hipMemcpyAsync(&h_flags, d_flags->p, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
        sr_set_error("sr_sparse_index_create: %s", hipGetErrorString(hipGetLastError()));
        return SR_ERR_HIP;
    }
    if (h_flags) {
        sr_set_error("sr_sparse_index_create: invalid index (%s%s%s)",
                     (h_flags & 1) ? "posting list not strictly ascending by doc id; " : "",
                     (h_flags & 2) ? "doc id out of [0, n_docs); " : "", (h_flags & 4) ? "indptr not monotone" : "");
        return SR_ERR_INVALID;
    }
    return SR_OK;
}

extern "C" int sr_sparse_index_create(sr_sparse_index** out, const int64_t* d_indptr, const int32_t* d_doc_ids,
                                      const float* d_vals, int64_t n_terms, int64_t n_docs, sr_stream stream) {
    SR_REQUIRE(out, "sr_sparse_index_create: null out");
    SR_REQUIRE(n_terms >= 1 && n_docs >= 1, "sr_sparse_index_create: need n_terms >= 1 and n_docs >= 1");
    SR_REQUIRE(n_docs < 0xffffffffll, "sr_sparse_index_create: n_docs exceeds 32 bits");
    SR_REQUIRE(d_indptr, "sr_sparse_index_create: null indptr");
    hipStream_t s = (hipStream_t)stream;
    sr_sparse_index* idx = new sr_sparse_index();
    idx->indptr = d_indptr;
    idx->doc_ids = d_doc_ids;
    idx->vals = d_vals;
    idx->n_terms = n_terms;
    idx->n_docs = n_docs;
    idx->n_tiles = (int)ceil_div64(n_docs, SP_TILE);
    DeviceBuf<int> d_flags;
    int rc = sparse_build_skip(idx, &d_flags, s);
    d_flags.release();
    if (rc == SR_OK) rc = sparse_build_dense(idx, s);
    if (rc == SR_OK) rc = sparse_cert_build(idx, s);
    if (rc != SR_OK) {
        (void)sr_sparse_index_destroy(idx);
        return rc;
    }
    *out = idx;
    return SR_OK;
}

extern "C" int sr_sparse_index_set_workspace_limit(sr_sparse_index* idx, int64_t bytes) {
    SR_REQUIRE(idx && bytes >= (1 << 20), "sr_sparse_index_set_workspace_limit: bad argument");
    idx->ws_limit = bytes;
    return SR_OK;
}

extern "C" int sr_sparse_index_destroy(sr_sparse_index* idx) {
    if (!idx) return SR_OK;
    idx->ws.release();
    idx->order.release();
    sparse_cert_destroy(idx->cert);
    idx->skip.release();
    idx->dense.release();
    idx->dense_slot.release();
    idx->plan_term.release();
    idx->plan_w.release();
    idx->plan_n.release();
    idx->plan_ok.release();
    idx->plan_off.release();
    idx->plan_perm.release();
    idx->q_done.release();
    idx->plan_bad.release();
    idx->d_counters.release();
    idx->d_postings.release();
    idx->seg_cnt.release();
    idx->pair_qflags.release();
    if (idx->pair_status) (void)hipFree(idx->pair_status);      // allocated by pair_status_begin / subset_status_begin
    idx->filt_words.release();
    idx->filt_blocks.release();
    idx->filt_list.release();
    idx->grp_counts.release();
    idx->range_tab.release();
    idx->range_qgroup.release();
    delete idx;
    return SR_OK;
}

extern "C" int sr_sparse_index_block_stats(sr_sparse_index* idx, int64_t* n_dense_terms, int64_t* n_block_calls,
                                           int64_t* n_fallback_calls) {
    SR_REQUIRE(idx && n_dense_terms && n_block_calls && n_fallback_calls, "sr_sparse_index_block_stats: null argument");
    std::lock_guard<std::mutex> lock(idx->mu);
    *n_dense_terms = idx->n_dense;
    *n_block_calls = idx->n_block_calls;
    *n_fallback_calls = idx->n_fallback_calls;
    return SR_OK;
}

// Work counters of the query-block kernel (measurement hook, like sr_sparse_index_profile): while enabled every workgroup adds
// what it loads and applies to 6 device counters; the call returns them and resets them.  out[0] dense columns loaded (one =
// 4096 floats), [1] (column, query) applications (one = 4096 unfused multiply-adds), [2] / [3] postings loaded by the one-step /
// grouped scatter runs (8 bytes each, one LDS read-modify-write each), [4] plan entries fetched, [5] workgroup-tiles.
extern "C" int sr_sparse_index_work_counters(sr_sparse_index* idx, int enable, uint64_t* out6) {
    SR_REQUIRE(idx, "sr_sparse_index_work_counters: null index");
    std::lock_guard<std::mutex> lock(idx->mu);
    if (!idx->d_counters.p) {
        if (idx->d_counters.reserve(6, "sr_sparse_index_work_counters") != SR_OK) return SR_ERR_HIP;
        SR_CHECK_HIP(hipMemset(idx->d_counters.p, 0, 6 * 8));
    }
    SR_CHECK_HIP(hipDeviceSynchronize());
    if (out6) SR_CHECK_HIP(hipMemcpy(out6, idx->d_counters.p, 6 * 8, hipMemcpyDeviceToHost));
    SR_CHECK_HIP(hipMemset(idx->d_counters.p, 0, 6 * 8));
    idx->count_work = enable != 0;
    return SR_OK;
}

extern "C" int sr_sparse_index_profile(sr_sparse_index* idx, int enable) {
    SR_REQUIRE(idx, "sr_sparse_index_profile: null index");
    std::lock_guard<std::mutex> lock(idx->mu);
    if (enable && !idx->d_postings.p) {
        if (idx->d_postings.reserve(1, "sr_sparse_index_profile") != SR_OK) return SR_ERR_HIP;
        SR_CHECK_HIP(hipMemset(idx->d_postings.p, 0, 8));
    }
    idx->prof.enabled = enable != 0;
    return SR_OK;
}

extern "C" int sr_sparse_index_profile_read(sr_sparse_index* idx, int64_t* n_launches, double* total_ms,
                                            double* total_posting_bytes) {
    SR_REQUIRE(idx && n_launches && total_ms && total_posting_bytes, "sr_sparse_index_profile_read: null argument");
    std::lock_guard<std::mutex> lock(idx->mu);
    *n_launches = idx->prof.read(total_ms);
    unsigned long long n = 0;
    if (idx->d_postings.p) {
        SR_CHECK_HIP(hipMemcpy(&n, idx->d_postings.p, 8, hipMemcpyDeviceToHost));
        SR_CHECK_HIP(hipMemset(idx->d_postings.p, 0, 8));
    }
    *total_posting_bytes = 8.0 * (double)n;
    return SR_OK;
}
