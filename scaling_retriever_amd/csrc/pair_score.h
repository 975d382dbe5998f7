// Pair scoring on the resident indexes (pair_score.hip): exact scores of caller-supplied (query, document) pairs.
#pragma once
#include "common.h"

struct PairSeg {                    // one dense segment: global doc index = id_base + row * id_stride
    const void* rows;               // fp32 or binary16 rows: the index's row type, passed to launch_dense_pairs
    int64_t n;
    int64_t id_base, id_stride;
};
struct PairStatus {                 // device word pair of a call: what the kernels found wrong
    unsigned long long first_bad;   // smallest pair position whose candidate id is not in the index (~0: none)
    int indptr_bad;                 // cand_indptr does not start at 0 or decreases somewhere: nothing was scored
    int pad;
};

// the row of global doc index gid (element offset into its segment's rows), as dense_pairs_kernel finds it; false: in no segment
__device__ inline bool pair_row_of(const PairSeg* __restrict__ segs, int n_segs, int64_t gid, int H, int* seg, int64_t* elem) {
    for (int sgi = 0; sgi < n_segs; ++sgi) {
        const int64_t off = gid - segs[sgi].id_base, stride = segs[sgi].id_stride;
        int64_t r = off;                                  // stride 1 (every segment of DenseFlatIndexer): no 64-bit divide
        bool in_seg = off >= 0;
        if (stride != 1) {
            r = off / stride;
            in_seg = in_seg && r * stride == off;
        }
        if (in_seg && r < segs[sgi].n) {
            *seg = sgi;
            *elem = r * (int64_t)H;
            return true;
        }
    }
    return false;
}
// the valid prefix of row q of a [nq, n] id list: counts[q] cut to [0, n], n without counts
__device__ inline int list_count(const int32_t* __restrict__ counts, int64_t q, int n) {
    if (!counts) return n;
    const int c = counts[q];
    return c < 0 ? 0 : (c > n ? n : c);
}
// first_bad = min(first_bad, q * n + i) for every valid entry (i < list_count, id >= 0) of ids [nq, n] that is in no segment (dense_mmr.hip)
int launch_id_list_check(const PairSeg* d_segs, int n_segs, int H, const int64_t* d_ids, const int32_t* d_counts, int64_t nq, int n,
                         PairStatus* d_status, hipStream_t s);

// *d_status: the handle's PairStatus (allocated on first use), reset on the stream; then cand_indptr is checked
int pair_status_begin(PairStatus** d_status, const int64_t* d_cand_indptr, int64_t nq, hipStream_t s);
// the call's one read-back: waits for the stream; SR_ERR_INVALID with the first offender named (who = entry point)
int pair_status_end(PairStatus* d_status, const int64_t* d_cand_ids, const char* who, hipStream_t s);

// out[p] = fp32 fmaf chain of Q[q] . row(cand_ids[p]) in dense_score.hip's k order, for cand_indptr[q] <= p < cand_indptr[q + 1]
// dtype = SR_DTYPE_F32 | SR_DTYPE_F16: how the segments' rows are stored (fp16 rows are widened in registers: the same chain)
int launch_dense_pairs(const PairSeg* d_segs, int n_segs, int dtype, const float* Q, int64_t nq, int H, const int64_t* d_cand_indptr,
                       const int64_t* d_cand_ids, float* d_out, PairStatus* d_status, hipStream_t s);

// sparse pair route: idx->pair_qflags[q] := the terms of query q are valid and strictly ascending (the forward index may serve it), for the nq
// queries of a call; the buffer grows on demand (who = entry point, for the message of SR_ERR_NOMEM)
struct sr_sparse_index;
int sparse_pair_query_flags(sr_sparse_index* idx, const int64_t* d_q_indptr, const int32_t* d_q_cols, int64_t nq, const char* who,
                            hipStream_t s);
