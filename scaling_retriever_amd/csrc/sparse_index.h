// State of a sparse (inverted) index handle, shared by the exact scorer (sparse_score.hip), the certified MFMA scorer
// (sparse_cert.hip) and the on-device index build (sparse_build.hip).
#pragma once
#include "common.h"
#include <mutex>

struct SparseCert;      // sparse_cert.hip
struct PairStatus;      // pair_score.h

// Geometry of sr_sparse_index::skip (built by sparse_score.hip, which checks these against its own tile constants): the exact scorer's
// doc tiles hold SR_SPARSE_TILE_DOCS documents (n_tiles of them), and skip[t * (n_sub + 1) + b] = number of postings of term t with
// doc id < b * SR_SPARSE_SKIP_DOCS for b = 0 .. n_sub, n_sub = n_tiles * (SR_SPARSE_TILE_DOCS / SR_SPARSE_SKIP_DOCS).
#define SR_SPARSE_TILE_DOCS 8192
#define SR_SPARSE_SKIP_DOCS 4096

struct sr_sparse_index {
    const int64_t* indptr = nullptr;
    const int32_t* doc_ids = nullptr;
    const float* vals = nullptr;
    int64_t n_terms = 0, n_docs = 0;
    int n_tiles = 0;
    int32_t* skip = nullptr;
    // heavy terms as dense columns (query-block kernel)
    int n_dense = 0;
    int64_t dense_stride = 0;
    float* dense = nullptr;
    int32_t* dense_slot = nullptr;
    // per-call plan of the query blocks
    int64_t plan_cap = 0, plan_blocks_cap = 0;
    int32_t* plan_term = nullptr;
    float* plan_w = nullptr;
    int32_t* plan_n = nullptr;
    uint8_t* plan_ok = nullptr;
    int64_t* plan_off = nullptr;
    unsigned long long* d_stamps = nullptr;   // dev switch SR_SPARSE_STAMPS
    unsigned long long* d_counters = nullptr; // sr_sparse_index_work_counters
    int* seg_cnt = nullptr;                   // wave-owned candidate regions of the query-block kernel: [q_batch][seg_cap]
    int64_t seg_q_cap = 0; int seg_cap = 0;
    bool count_work = false;
    int32_t* plan_perm = nullptr;     // every batch's queries in block order
    uint8_t* q_done = nullptr;
    int64_t plan_q_cap = 0;
    int* plan_bad = nullptr;
    int64_t n_block_calls = 0, n_fallback_calls = 0;
    int64_t ws_limit = 4ll << 30;
    TopkWS ws;
    StreamOrder order;
    LaunchProfile prof;
    unsigned long long* d_postings = nullptr;  // device counter of postings touched (profiling only)
    // certified two-stage scorer (null: the index or the device does not qualify; every search then runs the exact kernels)
    SparseCert* cert = nullptr;
    int64_t n_cert_no_memory = 0;       // query batches served by the exact kernels because the certified scorer's buffers did not fit
    int64_t n_cert_retries = 0;         // sub-batches of handed-back queries sent through the scorer again with the widest band
    uint8_t* pair_qflags = nullptr; int64_t pair_qflags_cap = 0;   // sr_sparse_score_pairs: per query, may the forward route serve it
    PairStatus* pair_status = nullptr;  // sr_sparse_score_pairs: the call's status words (pair_score.hip)
    // sr_sparse_search_subset / _masked (subset_search.hip): the form of the call's document filter that the caller did not give - the
    // bitmap of a list, or the ascending list of a bitmap with the per-workgroup counts of its expansion - kept and grown on demand
    uint32_t* filt_words = nullptr; int64_t filt_words_cap = 0;
    int64_t* filt_blocks = nullptr; int64_t filt_blocks_cap = 0;
    int64_t* filt_list = nullptr; int64_t filt_list_cap = 0;
    // sr_sparse_range_count / _fill (sparse_range.hip): the (chunk, query) table of the last count - hits per cell, turned into exclusive
    // prefixes over the chunks by the scan - and what it was made for.  A chunk is range_chunk_tiles consecutive doc tiles
    int32_t* range_tab = nullptr; int64_t range_tab_cap = 0;          // [range_chunks, range_nq] int32
    int64_t range_nq = -1, range_total = 0;                           // range_nq = -1: no count to fill from
    int range_chunk_tiles = 0, range_chunks = 0;
    std::mutex mu;
};

// ---- certified two-stage scorer (sparse_cert.hip) ----
// Builds the side structures (fp16 MFMA tiles of the heavy terms, packed postings, per-tile run table, doc-major forward index).
// SR_OK with idx->cert == nullptr when the index does not qualify (a negative or non-finite value, too few docs, no memory).
int sparse_cert_build(sr_sparse_index* idx, hipStream_t s);
void sparse_cert_destroy(SparseCert* c);
// the doc-major forward index (row d = postings [fwd_indptr[d], fwd_indptr[d + 1]) of fwd_tv, term << 32 | value bits, terms ascending);
// false (pointers untouched) when c is null or was built without it
bool sparse_cert_forward_index(const SparseCert* c, const int64_t** fwd_indptr, const uint64_t** fwd_tv);
// Scores every query; d_uncert[q] = 1 marks the queries whose result rows were NOT written and must be served by the exact
// kernels (query outside the fast path's preconditions, or its candidate set could not be certified).  *n_uncert = their number.
// The call synchronises the stream TWICE: after the plan (the largest rare-term count sizes the band) and at the end (*n_uncert).
// *no_memory = true (with SR_OK): the per-call buffers of this batch did not fit
// in device memory; they were released, nothing was computed, and the caller serves the batch with the exact kernels.
// d_mask_pad (null: every document): the bitmap of sparse_cert_mask_pad; a document whose bit is clear never becomes a stage-1 key, so
// the result is the top-k among the allowed documents and "fewer than k docs with a non-zero key" counts allowed documents only.
int sparse_cert_search(sr_sparse_index* idx, const int64_t* d_q_indptr, const int32_t* d_q_cols, const float* d_q_vals, int64_t nq,
                       int k, float threshold, int64_t id_base, int64_t id_stride, float* d_out_scores, int64_t* d_out_ids,
                       int32_t* d_out_counts, uint8_t* d_uncert, int64_t* n_uncert, bool* no_memory, int band_keys, int* band_used,
                       const uint32_t* d_mask_pad, hipStream_t s);
// band_keys: keys the running set keeps beyond k (the certificate's room); 0 = chosen from the batch's largest rare-term count (1 024 /
// 2 048 / 3 072, capped at SR_MAX_TOPK - k); *band_used returns it.
// The scorer's own copy of a caller's bitmap (d_words uint32 [ceil(n_docs / 32)]) in the length its kernel walks, n_tiles * 32 words: the
// caller's words, the bits of the last one at or beyond n_docs cleared, zeros behind.  Filled on the stream; *d_mask_pad = null (with
// SR_OK): no device memory for it.  _bytes: its size.
int sparse_cert_mask_pad(sr_sparse_index* idx, const uint32_t* d_words, const uint32_t** d_mask_pad, hipStream_t s);
int64_t sparse_cert_mask_pad_bytes(const SparseCert* c);
void sparse_cert_count_retry(SparseCert* c, int64_t ns);
// [nq] flag bytes kept with the scorer (grown on demand); nullptr = out of device memory
uint8_t* sparse_cert_uncert_buffer(SparseCert* c, int64_t nq);
// queries per call of sparse_cert_search: its per-query workspace is ~200 KB (candidate slots of a launch, running set, approximate lists)
#define SR_CERT_QUERY_BATCH 8192

// ---- search under a document filter (subset_search.hip, sparse_score.hip) ----
// Both forms of one call's filter.  `words` is always there; the list is expanded from it when a route or a hand-back needs its entries.
struct SparseDocFilter {
    const uint32_t* words = nullptr;     // uint32 [ceil(n_docs / 32)]
    const uint32_t* mask_pad = nullptr;  // sparse_cert_mask_pad of `words`
    const int64_t* list = nullptr;       // the set bits, ascending; valid once list_ready
    int64_t m = 0;                       // number of set bits
    bool list_ready = false;
    const char* who = "sr_sparse_search_masked";      // the entry point, for error messages
};
// expands f->words into the handle's list (launch_doc_mask_expand; needs the per-workgroup counts of the call's launch_doc_mask_count in
// idx->filt_blocks) unless the list is there already
int sparse_filter_need_list(sr_sparse_index* idx, SparseDocFilter* f, hipStream_t s);
// Which list route serves a filter of m documents, the default rule or the dev switch SR_SUBSET_SPARSE_ROUTE=pairs|array
bool subset_sparse_use_array(int64_t m, int64_t n_docs);
// The list routes of sr_sparse_search_subset for a query CSR: idx->mu held, the call's status begun (subset_status_begin) and d_subset
// known to be strictly ascending positions in [0, n_docs) - or its check kernel queued in front.  array: which of the two routes.
int sparse_subset_lists(sr_sparse_index* idx, const int64_t* d_q_indptr, const int32_t* d_q_cols, const float* d_q_vals, int64_t nq, int k,
                        float threshold, const int64_t* d_subset, int64_t m, bool array, int64_t id_base, int64_t id_stride, float* d_out_scores,
                        int64_t* d_out_ids, int32_t* d_out_counts, hipStream_t s, const char* who);
// May this call go through the certified scorer: the index has one, k + 1024 <= SR_MAX_TOPK, n_docs >= 8 (k + 1024) unless SR_SPARSE_CERT=1,
// and not SR_SPARSE_CERT_SEARCH=0 (dev switches)
bool sparse_cert_applies(const sr_sparse_index* idx, int k);
// The certified search of sr_sparse_search in query batches, with the exact re-do of what the scorer hands back.  filt (null: the whole
// collection): the pass runs under filt->mask_pad and handed-back queries, or a batch whose buffers do not fit, are served by
// sparse_subset_lists over the filter's list.  idx->mu held.
int sparse_certified_search(sr_sparse_index* idx, const int64_t* d_q_indptr, const int32_t* d_q_cols, const float* d_q_vals, int64_t nq, int k,
                            float threshold, int64_t id_base, int64_t id_stride, float* d_out_scores, int64_t* d_out_ids, int32_t* d_out_counts,
                            SparseDocFilter* filt, hipStream_t s);

// ---- device-wide exclusive scan of int64 counts (sparse_build.hip): out[i] = sum_{j < i} in[j], out[n] = total; in == out allowed
int sr_device_exclusive_scan_i64(const int64_t* d_in, int64_t* d_out, int64_t n, hipStream_t s);
