// The exact score of ONE (query, document) pair of a sparse index, computed by one wave: the device function behind
// sparse_pairs_kernel (pair_score.hip) and the pair route of the subset search (subset_search.hip).  The routes and the ordered sum
// are described at sparse_pairs_kernel; both callers get the same bits from it.
#pragma once
#include "common.h"

struct SparseChainIndex {
    const int64_t* indptr; const int32_t* doc_ids; const float* vals;
    int64_t n_terms;
    const int64_t* fwd_indptr; const uint64_t* fwd_tv;      // null: postings route only
};

// scores[doc] of the reference's term-serial chain (scaling_retriever/indexer.py:324-340) for the query terms [tb, te) of q_cols /
// q_vals; `forward` (wave-uniform): the document's forward row serves the pair.  Every lane of the wave calls it and returns the sum.
__device__ inline float sparse_pair_chain(const SparseChainIndex& x, const int32_t* __restrict__ q_cols, const float* __restrict__ q_vals,
                                          int64_t tb, int64_t te, bool forward, int64_t doc, int lane) {
#pragma clang fp contract(off)
    float s = 0.f;
    auto ordered_add = [&](bool m, float prod) {
        uint64_t mm = __ballot(m);
        while (mm) {
            const int i = __builtin_ctzll(mm);
            mm &= mm - 1;
            s = s + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(prod), i));
        }
    };
    if (forward) {
        const int64_t b = x.fwd_indptr[doc], e = x.fwd_indptr[doc + 1];
        for (int64_t c = b; c < e; c += 64) {
            const int64_t i = c + lane;
            bool m = false;
            float prod = 0.f;
            if (i < e) {
                const uint64_t tv = x.fwd_tv[i];
                const int32_t t = (int32_t)(tv >> 32);
                int64_t lo = tb, hi = te;
                while (lo < hi) {
                    const int64_t mid = (lo + hi) >> 1;
                    if (q_cols[mid] < t) lo = mid + 1; else hi = mid;
                }
                if (lo < te && q_cols[lo] == t) {
                    m = true;
                    prod = q_vals[lo] * __uint_as_float((uint32_t)tv);
                }
            }
            ordered_add(m, prod);
        }
    } else {
        for (int64_t c = tb; c < te; c += 64) {
            const int64_t i = c + lane;
            bool m = false;
            float prod = 0.f;
            if (i < te) {
                const int32_t t = q_cols[i];
                if (t >= 0 && t < x.n_terms) {
                    const int64_t pe = x.indptr[t + 1];
                    int64_t lo = x.indptr[t], hi = pe;
                    while (lo < hi) {
                        const int64_t mid = (lo + hi) >> 1;
                        if ((int64_t)x.doc_ids[mid] < doc) lo = mid + 1; else hi = mid;
                    }
                    if (lo < pe && (int64_t)x.doc_ids[lo] == doc) {
                        m = true;
                        prod = q_vals[i] * x.vals[lo];
                    }
                }
            }
            ordered_add(m, prod);
        }
    }
    return s;
}
