// State of a sparse (inverted) index handle and the internal calls its files share: the handle's create / destroy / hooks
// (sparse_index.hip), the exact scorer (sparse_score.hip), the certified MFMA scorer (sparse_cert_build.hip, sparse_cert.hip), the
// search entry point that chooses between them (sparse_search.hip) and the on-device index build (sparse_build.hip).
#pragma once
#include "common.h"
#include <mutex>

struct SparseCert;      // sparse_cert.h
struct PairStatus;      // pair_score.h
struct SparseGroups;    // below

// Geometry of sr_sparse_index::skip (built by sparse_index.hip; sparse_score.hip checks these against its own tile constants): the
// exact scorer's doc tiles hold SR_SPARSE_TILE_DOCS documents (n_tiles of them), and skip[t * (n_sub + 1) + b] = number of postings of
// term t with doc id < b * SR_SPARSE_SKIP_DOCS for b = 0 .. n_sub, n_sub = n_tiles * (SR_SPARSE_TILE_DOCS / SR_SPARSE_SKIP_DOCS).
#define SR_SPARSE_TILE_DOCS 8192
#define SR_SPARSE_SKIP_DOCS 4096
// queries per workgroup of the query-block kernel (sparse_score.hip: SPB_Q), i.e. weights per entry of plan_w
#define SR_SPARSE_BLOCK_QUERIES 4

// Every device buffer the library allocates for the handle is a DeviceBuf: reserve() where it is filled, release() in
// sr_sparse_index_destroy, nothing else.
struct sr_sparse_index {
    const int64_t* indptr = nullptr;
    const int32_t* doc_ids = nullptr;
    const float* vals = nullptr;
    int64_t n_terms = 0, n_docs = 0;
    int n_tiles = 0;
    DeviceBuf<int32_t> skip;
    // heavy terms as dense columns (query-block kernel); n_dense = 0: none, the per-query kernel serves every search
    int n_dense = 0;
    int64_t dense_stride = 0;
    DeviceBuf<float> dense;
    DeviceBuf<int32_t> dense_slot;
    // per-call plan of the query blocks
    DeviceBuf<int32_t> plan_term;        // [query terms of the call]
    DeviceBuf<float> plan_w;             // [query terms of the call][SR_SPARSE_BLOCK_QUERIES]
    DeviceBuf<int32_t> plan_n;           // [blocks]
    DeviceBuf<uint8_t> plan_ok;          // [blocks]
    DeviceBuf<int64_t> plan_off;         // [blocks]
    DeviceBuf<int32_t> plan_perm;        // [blocks][SR_SPARSE_BLOCK_QUERIES]: every batch's queries in block order
    DeviceBuf<uint8_t> q_done;           // [queries of the call]
    DeviceBuf<int> plan_bad;             // [1]
    DeviceBuf<unsigned long long> d_counters;  // [6] sr_sparse_index_work_counters
    DeviceBuf<unsigned long long> d_postings;  // [1] postings touched (sr_sparse_index_profile)
    DeviceBuf<int> seg_cnt;              // wave-owned candidate regions of the query-block kernel: [seg_q_cap][seg_cap]
    int64_t seg_q_cap = 0; int seg_cap = 0;
    bool count_work = false;
    int64_t n_block_calls = 0, n_fallback_calls = 0;
    int64_t ws_limit = 4ll << 30;
    TopkWS ws;
    StreamOrder order;
    LaunchProfile prof;
    // certified two-stage scorer (null: the index or the device does not qualify; every search then runs the exact kernels)
    SparseCert* cert = nullptr;
    int64_t n_cert_no_memory = 0;       // query batches served by the exact kernels because the certified scorer's buffers did not fit
    int64_t n_cert_retries = 0;         // sub-batches of handed-back queries sent through the scorer again with the widest band
    DeviceBuf<uint8_t> pair_qflags;     // sr_sparse_score_pairs: per query, may the forward route serve it
    PairStatus* pair_status = nullptr;  // the call's status words, allocated by pair_status_begin / subset_status_begin (pair_score.hip)
    // sr_sparse_search_subset / _masked (subset_search.hip): the form of the call's document filter that the caller did not give - the
    // bitmap of a list, or the ascending list of a bitmap with the per-workgroup counts of its expansion - kept and grown on demand
    DeviceBuf<uint32_t> filt_words;
    DeviceBuf<int64_t> filt_blocks;
    DeviceBuf<int64_t> filt_list;
    DeviceBuf<int64_t> grp_counts;       // sr_sparse_search_grouped: [n_groups + 1] set bits per group (+ the unused word of launch_doc_masks_check)
    // sr_sparse_range_count / _fill (sparse_range.hip): the (chunk, query) table of the last count - hits per cell, turned into exclusive
    // prefixes over the chunks by the scan - and what it was made for.  A chunk is range_chunk_tiles consecutive doc tiles
    DeviceBuf<int32_t> range_tab;                                     // [range_chunks, range_nq]
    int64_t range_nq = -1, range_total = 0;                           // range_nq = -1: no count to fill from
    int range_chunk_tiles = 0, range_chunks = 0;
    int range_kind = 0;                                              // what the last count ran under (0 none, 1 a bitmap, 2 filter groups): its fill must too
    DeviceBuf<int32_t> range_qgroup;                                  // grouped count: [range_nq] the checked group of every query, read by its fill
    int64_t range_groups = 0;                                         // n_groups of the last grouped count
    std::mutex mu;
};

// One search as the internal drivers hand it on: the query CSR, what is asked for, and where the result rows go.
struct SparseCall {
    const int64_t* q_indptr = nullptr;   // [nq + 1] offsets into q_cols / q_vals
    const int32_t* q_cols = nullptr;
    const float* q_vals = nullptr;
    int64_t nq = 0;
    int k = 0;
    float threshold = 0.f;
    int64_t id_base = 0, id_stride = 1;
    float* out_scores = nullptr;         // [nq, k]
    int64_t* out_ids = nullptr;          // [nq, k]
    int32_t* out_counts = nullptr;       // [nq] or null
    // the same call for the queries [qb, qb + nqb) alone.  q_indptr moves to row qb; its entries still index the whole q_cols / q_vals,
    // which therefore stay where they are
    SparseCall rows(int64_t qb, int64_t nqb) const {
        SparseCall c = *this;
        c.q_indptr = q_indptr + qb;
        c.nq = nqb;
        c.out_scores = out_scores + qb * k;
        c.out_ids = out_ids + qb * k;
        c.out_counts = out_counts ? out_counts + qb : nullptr;
        return c;
    }
};

// ---- exact scorer (sparse_score.hip) ----
// The exact kernels over all docs for the queries of one call (the caller holds idx->mu and the stream order).
int sparse_exact_search(sr_sparse_index* idx, const SparseCall& call, hipStream_t s);

// ---- certified two-stage scorer (sparse_cert_build.hip: the index-side structures; sparse_cert.hip: the search) ----
// Builds the side structures (fp16 MFMA tiles of the heavy terms, packed postings, per-tile run table, doc-major forward index).
// SR_OK with idx->cert == nullptr when the index does not qualify (a negative or non-finite value, too few docs, no memory).
int sparse_cert_build(sr_sparse_index* idx, hipStream_t s);
void sparse_cert_destroy(SparseCert* c);
// the doc-major forward index (row d = postings [fwd_indptr[d], fwd_indptr[d + 1]) of fwd_tv, term << 32 | value bits, terms ascending);
// false (pointers untouched) when c is null or was built without it
bool sparse_cert_forward_index(const SparseCert* c, const int64_t** fwd_indptr, const uint64_t** fwd_tv);
struct SparseCertOptions {
    uint8_t* uncert = nullptr;           // [nq] out: 1 marks a query whose result rows were NOT written (sparse_cert_uncert_buffer)
    // keys the running set keeps beyond k (the certificate's room); 0 = chosen from the batch's largest rare-term count (1 024 / 2 048 /
    // 3 072), capped at SR_MAX_TOPK - k
    int band_keys = 0;
    // null: every document; else the bitmap of sparse_cert_mask_pad: a document whose bit is clear never becomes a stage-1 key, so the
    // result is the top-k among the allowed documents and "fewer than k docs with a non-zero key" counts allowed documents only
    const uint32_t* mask_pad = nullptr;
    // a bitmap per query (sparse_cert_group_pad): group_pad = the groups' padded bitmaps, qoff [nq rounded up to 32] = the word offset of
    // each query's row in it, mask_pad = their union.  Null: one bitmap for all queries, or none
    const uint32_t* group_pad = nullptr;
    const uint32_t* qoff = nullptr;
};
struct SparseCertResult {
    int64_t n_uncert = 0;                // queries flagged in SparseCertOptions::uncert
    // (with SR_OK) the per-call buffers of this batch did not fit in device memory; they were released, nothing was computed, and the
    // caller serves the batch with the exact kernels
    bool no_memory = false;
    int band_used = 0;                   // the band the pass ran with
};
// Scores every query of the call; the flagged ones (query outside the fast path's preconditions, or its candidate set could not be
// certified) must be served by the exact kernels.  The call synchronises the stream TWICE: after the plan (the largest rare-term count
// sizes the band) and at the end (n_uncert).
int sparse_cert_search(sr_sparse_index* idx, const SparseCall& call, const SparseCertOptions& opt, SparseCertResult* res, hipStream_t s);
// The scorer's own copy of a caller's bitmap (d_words uint32 [ceil(n_docs / 32)]) in the length its kernel walks, n_tiles * 32 words: the
// caller's words, the bits of the last one at or beyond n_docs cleared, zeros behind.  Filled on the stream; *d_mask_pad = null (with
// SR_OK): no device memory for it.  _bytes: its size.
int sparse_cert_mask_pad(sr_sparse_index* idx, const uint32_t* d_words, const uint32_t** d_mask_pad, hipStream_t s);
int64_t sparse_cert_mask_pad_bytes(const SparseCert* c);
// The same for a grouped search: d_group_words uint32 [n_groups, ceil(n_docs / 32)] -> [n_groups + 1][n_tiles * 32] words on the handle, row
// n_groups = the union of the groups, and the queries' word offsets d_query_group[q] * n_tiles * 32, zero-padded to a multiple of 32
// queries.  (n_groups + 1) * n_tiles * 32 < 2^32 (SR_ERR_INVALID otherwise).  Pointers null (with SR_OK): no device memory.  _bytes: the
// size of the bitmaps.
int sparse_cert_group_pad(sr_sparse_index* idx, const uint32_t* d_group_words, int64_t n_groups, const int32_t* d_query_group, int64_t nq,
                          const uint32_t** d_group_pad, const uint32_t** d_union_pad, const uint32_t** d_qoff, hipStream_t s);
int64_t sparse_cert_group_pad_bytes(const SparseCert* c, int64_t n_groups);
void sparse_cert_count_retry(SparseCert* c, int64_t ns);
// [nq] flag bytes kept with the scorer (grown on demand); nullptr = out of device memory
uint8_t* sparse_cert_uncert_buffer(SparseCert* c, int64_t nq);
// queries per call of sparse_cert_search: its per-query workspace is ~200 KB (candidate slots of a launch, running set, approximate lists)
#define SR_CERT_QUERY_BATCH 8192

// ---- search under a document filter (subset_search.hip, sparse_search.hip) ----
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
// The list routes of sr_sparse_search_subset for one call: idx->mu held, the call's status begun (subset_status_begin) and d_subset
// known to be strictly ascending positions in [0, n_docs) - or its check kernel queued in front.  array: which of the two routes.
int sparse_subset_lists(sr_sparse_index* idx, const SparseCall& call, const int64_t* d_subset, int64_t m, bool array, hipStream_t s,
                        const char* who);
// May this call go through the certified scorer: the index has one, k + 1024 <= SR_MAX_TOPK, n_docs >= 8 (k + 1024) unless SR_SPARSE_CERT=1,
// and not SR_SPARSE_CERT_SEARCH=0 (dev switches)
bool sparse_cert_applies(const sr_sparse_index* idx, int k);
// The certified search of sr_sparse_search in query batches, with the exact re-do of what the scorer hands back.  filt (null: the whole
// collection): the pass runs under filt->mask_pad and handed-back queries, or a batch whose buffers do not fit, are served by
// sparse_subset_lists over the filter's list.  groups (with filt null): a bitmap per query - the pass runs the grouped twin of the score
// kernel, every batch with its slice of groups->qoff, and what a batch hands back is re-done by sparse_grouped_each under each query's
// own group's list (no second, wider-band pass).  idx->mu held.
int sparse_certified_search(sr_sparse_index* idx, const SparseCall& call, SparseDocFilter* filt, hipStream_t s, const SparseGroups* groups = nullptr);

// ---- search under a bitmap per query (sr_sparse_search_grouped: subset_search.hip, sparse_search.hip) ----
// What the drivers know of a grouped call.  The host arrays describe ALL queries of the entry's call; q0 = the first of them that the
// SparseCall handed along with this struct holds (a batch, a sub-call).
struct SparseGroups {
    const uint32_t* words = nullptr;     // the caller's bitmaps, uint32 [n_groups, n_words]
    int64_t n_groups = 0, n_words = 0;
    const int32_t* h_group = nullptr;    // host: group of every query, range-checked
    const int64_t* h_count = nullptr;    // host: set bits of every group
    int64_t q0 = 0;
    // sparse_cert_group_pad (all null: no device memory for them)
    const uint32_t* group_pad = nullptr;
    const uint32_t* union_pad = nullptr;
    const uint32_t* qoff = nullptr;      // of query 0 of the entry's call
    const char* who = "sr_sparse_search_grouped";
};
// The body of sr_sparse_search_masked behind its argument checks: count of the set bits (one read-back), workspace check, route rule, search.
int sparse_masked_body(sr_sparse_index* idx, const SparseCall& call, const uint32_t* d_mask_words, hipStream_t s, const char* who);
// The list routes (pairs / array by the rule) for one call under a bitmap of m set bits: the bitmap expanded into the handle's list
int sparse_masked_lists(sr_sparse_index* idx, const SparseCall& call, const uint32_t* d_mask_words, int64_t m, hipStream_t s, const char* who);
// The queries of `call` (h_flags null: all; else those with a non-zero flag, h_flags [call.nq] on the host) searched group by group, only
// groups that hold such a query: the group's queries gathered into a CSR of their own, searched under the group's bitmap - lists_only:
// by sparse_masked_lists, else by sparse_masked_body - and their rows scattered back.  Waits for the stream.
int sparse_grouped_each(sr_sparse_index* idx, const SparseCall& call, const SparseGroups& groups, const uint8_t* h_flags, bool lists_only, hipStream_t s);

// ---- device-wide exclusive scan of int64 counts (sparse_build.hip): out[i] = sum_{j < i} in[j], out[n] = total; in == out allowed
int sr_device_exclusive_scan_i64(const int64_t* d_in, int64_t* d_out, int64_t n, hipStream_t s);
