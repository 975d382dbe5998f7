// Search within a document subset (subset_search.hip): one strictly ascending allow-list shared by all queries of a call.
#pragma once
#include "common.h"
#include "pair_score.h"

// *d_status: the handle's PairStatus (allocated on first use; first_bad = ~0, the other word unused), reset on the stream
int subset_status_begin(PairStatus** d_status, hipStream_t s);
// the call's one read-back: waits for the stream; SR_ERR_INVALID with the first offending position named.  what_id = "doc index" (dense)
// or "position" (sparse): how an entry that is in order but not in the index is called in the message
int subset_status_end(PairStatus* d_status, const int64_t* d_subset, const char* who, const char* what_id, hipStream_t s);

// Queries per batch and subset entries per slab so that 8 bytes per (query, slab entry) - and for k > SR_MAX_TOPK the large
// select's buffers - fit ws_limit.  min_slab = the smallest slab the route can work with.  SR_ERR_NOMEM if one query does not fit.
int subset_plan(int64_t ws_limit, int64_t nq, int k, int64_t m, int64_t min_slab, int64_t* nq_batch, int64_t* slab, const char* who);

// first_bad = min(first_bad, j) for every j with subset[j] <= subset[j - 1] or subset[j] in no segment
int launch_subset_check_dense(const PairSeg* d_segs, int n_segs, const int64_t* d_subset, int64_t m, PairStatus* d_status, hipStream_t s);

struct DenseSubsetArgs {
    const PairSeg* segs; int n_segs;
    int dtype;                      // SR_DTYPE_F32 | SR_DTYPE_F16: row storage
    const float* Q; int nq; int H;  // the queries of this batch
    const int64_t* subset;          // the slab: n_slab entries
    int64_t n_slab;
    const float* tau; uint64_t* cand_keys; int* cand_count; int64_t cand_cap;     // TopkWS of the batch
    const PairStatus* st;           // nothing is scored once the check found an offender
};
// appends key(score, doc index) of every (query, slab entry) with score >= tau[query]; score = the fmaf chain of dense_pairs_kernel
int launch_dense_subset(const DenseSubsetArgs& a, hipStream_t s);
