// Pair scoring: exact scores of caller-supplied (query, document) pairs from the resident indexes - what the reference's
// rerank_forward (scaling_retriever/modeling/llm_encoder.py:593-615) computes by encoding both sides of every pair again, here
// read from the vectors the indexes already hold.  The candidate lists are ragged (CSR over queries) and only their offsets'
// last entry says how many pairs there are, on the device: both kernels run a fixed grid whose workgroups / waves stride over
// the pairs, so that no size has to come back to the host before the launch.
#include "pair_score.h"
#include "sparse_index.h"
#include "sparse_pair_chain.h"
#include <math.h>

// ---------------------------------------------------------------------------------------------------- status ---
__global__ void pair_check_indptr_kernel(const int64_t* __restrict__ cand_indptr, int64_t nq, PairStatus* __restrict__ st) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    if (cand_indptr[q + 1] < cand_indptr[q] || (q == 0 && cand_indptr[0] != 0)) atomicOr(&st->indptr_bad, 1);
}

int pair_status_begin(PairStatus** d_status, const int64_t* d_cand_indptr, int64_t nq, hipStream_t s) {
    if (!*d_status) {
        if (hipMalloc((void**)d_status, sizeof(PairStatus)) != hipSuccess) {
            (void)hipGetLastError();
            *d_status = nullptr;
            sr_set_error("pair scoring: out of device memory for %zu status bytes", sizeof(PairStatus));
            return SR_ERR_NOMEM;
        }
    }
    SR_CHECK_HIP(hipMemsetAsync(&(*d_status)->first_bad, 0xff, sizeof(unsigned long long), s));
    SR_CHECK_HIP(hipMemsetAsync(&(*d_status)->indptr_bad, 0, 2 * sizeof(int), s));
    hipLaunchKernelGGL(pair_check_indptr_kernel, dim3((unsigned)ceil_div64(nq, 256)), dim3(256), 0, s, d_cand_indptr, nq, *d_status);
    SR_CHECK_LAUNCH();
    return SR_OK;
}

int pair_status_end(PairStatus* d_status, const int64_t* d_cand_ids, const char* who, hipStream_t s) {
    PairStatus h;
    SR_CHECK_HIP(hipMemcpyAsync(&h, d_status, sizeof(h), hipMemcpyDeviceToHost, s));
    SR_CHECK_HIP(hipStreamSynchronize(s));
    SR_REQUIRE(h.indptr_bad == 0, "%s: cand_indptr must start at 0 and never decrease (nothing was scored)", who);
    if (h.first_bad != ~0ull) {
        int64_t id = 0;
        SR_CHECK_HIP(hipMemcpy(&id, d_cand_ids + h.first_bad, sizeof(id), hipMemcpyDeviceToHost));
        sr_set_error("%s: candidate id %lld (pair %llu) is not in the index", who, (long long)id, h.first_bad);
        return SR_ERR_INVALID;
    }
    return SR_OK;
}

// first i in [1, nq] with indptr[i] > p, minus 1: the (non-empty) list that holds pair p < indptr[nq]
__device__ inline int64_t pair_query_of(const int64_t* __restrict__ indptr, int64_t nq, int64_t p) {
    int64_t lo = 1, hi = nq;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (indptr[mid] > p) hi = mid; else lo = mid + 1;
    }
    return lo - 1;
}

// ----------------------------------------------------------------------------------------------------- dense ---
// A pure gather.  One wave per tile of 64 consecutive pairs, lane = pair: the 64 rows are fetched 64 columns at a time as
// coalesced 256-byte pieces (16 lanes per row, 4 rows per load instruction), transposed through a padded LDS tile, and every
// lane runs the fp32 fmaf chain of ITS pair in dense_score_kernel's k order (per 8 columns: k = 8s + j, then 8s + 4 + j) - the
// chain is serial in k, so a pair's sum cannot be spread over lanes.  All 16 loads of the next chunk are in flight while this
// one goes through LDS and the chain (the shape of filter_rescore_kernel, dense_filter.hip).  A list of 1 000 candidates is 16
// consecutive tiles, each reading its query chunk once (a broadcast LDS read in the chain); a tile that straddles lists runs one
// pass per list with the other lists' lanes idle (their rows are not fetched).  The workgroups stride over the tiles.
#define PS_KC 64
template <typename T>
__global__ __launch_bounds__(64) void dense_pairs_kernel(const PairSeg* __restrict__ segs, int n_segs, const float* __restrict__ Q,
                                                         int64_t nq, int H, const int64_t* __restrict__ cand_indptr,
                                                         const int64_t* __restrict__ cand_ids, float* __restrict__ out,
                                                         PairStatus* __restrict__ st) {
    __shared__ float tile[64][PS_KC + 1];
    __shared__ float qs[PS_KC];
    __shared__ const T* rowp[64];
    if (st->indptr_bad) return;
    const int lane = threadIdx.x;
    const int64_t total = cand_indptr[nq];
    const int nch = (H + PS_KC - 1) / PS_KC;
    for (int64_t t0 = (int64_t)blockIdx.x * 64; t0 < total; t0 += (int64_t)gridDim.x * 64) {
        const int64_t p = t0 + lane;
        const T* row = nullptr;
        if (p < total) {
            const int64_t gid = cand_ids[p];
            for (int sgi = 0; sgi < n_segs; ++sgi) {
                const int64_t off = gid - segs[sgi].id_base, stride = segs[sgi].id_stride;
                int64_t r = off;                              // stride 1 (every segment of DenseFlatIndexer): no 64-bit divide
                bool in_seg = off >= 0;
                if (stride != 1) {
                    r = off / stride;
                    in_seg = in_seg && r * stride == off;
                }
                if (in_seg && r < segs[sgi].n) {
                    row = static_cast<const T*>(segs[sgi].rows) + r * (int64_t)H;
                    break;
                }
            }
            if (!row) {
                atomicMin(&st->first_bad, (unsigned long long)p);
                out[p] = __builtin_nanf("");
            }
        }
        const int64_t tile_end = t0 + 64 < total ? t0 + 64 : total;
        int64_t q = pair_query_of(cand_indptr, nq, t0);
        for (int64_t seg_b = t0; seg_b < tile_end;) {
            while (cand_indptr[q + 1] <= seg_b) ++q;          // empty lists; ends: cand_indptr[nq] = total > seg_b
            const int64_t list_e = cand_indptr[q + 1];
            const int64_t seg_e = list_e < tile_end ? list_e : tile_end;
            const bool mine = p >= seg_b && p < seg_e;
            __syncthreads();                                  // the previous pass has read rowp
            rowp[lane] = mine ? row : nullptr;
            __syncthreads();
            const T* myp[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) myp[i] = rowp[i * 4 + (lane >> 4)];
            const float* qrow = Q + q * (int64_t)H;
            float acc = 0.f;
            auto fetch = [&](int k0, f32x4 (&v)[16], float& qv) {
                const int col = k0 + (lane & 15) * 4;         // H % 16 == 0: a 16-byte piece is inside the row or beyond it
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (myp[i] && col < H) v[i] = sr_load_row4<T>(myp[i] + col);
                }
                qv = k0 + lane < H ? qrow[k0 + lane] : 0.f;
            };
            auto chunk = [&](const f32x4 (&v)[16], float qv, int k0) {
                __syncthreads();                              // the previous chunk is consumed
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    float* t = &tile[i * 4 + (lane >> 4)][(lane & 15) * 4];
                    t[0] = v[i][0]; t[1] = v[i][1]; t[2] = v[i][2]; t[3] = v[i][3];
                }
                qs[lane] = qv;
                __syncthreads();
                if (H - k0 >= PS_KC) {
#pragma unroll
                    for (int s8 = 0; s8 < PS_KC; s8 += 8)
#pragma unroll
                        for (int jj = 0; jj < 4; ++jj) {
                            acc = __builtin_fmaf(qs[s8 + jj], tile[lane][s8 + jj], acc);
                            acc = __builtin_fmaf(qs[s8 + 4 + jj], tile[lane][s8 + 4 + jj], acc);
                        }
                } else {                                      // the last chunk of a dim that is not a multiple of 64: its columns only
                    for (int s8 = 0; s8 < H - k0; s8 += 8)
#pragma unroll
                        for (int jj = 0; jj < 4; ++jj) {
                            acc = __builtin_fmaf(qs[s8 + jj], tile[lane][s8 + jj], acc);
                            acc = __builtin_fmaf(qs[s8 + 4 + jj], tile[lane][s8 + 4 + jj], acc);
                        }
                }
            };
            f32x4 va[16], vb[16];
            float qva, qvb;
            fetch(0, va, qva);
            for (int c = 0; c < nch; c += 2) {
                if (c + 1 < nch) fetch((c + 1) * PS_KC, vb, qvb);
                chunk(va, qva, c * PS_KC);
                if (c + 1 >= nch) break;
                if (c + 2 < nch) fetch((c + 2) * PS_KC, va, qva);
                chunk(vb, qvb, (c + 1) * PS_KC);
            }
            if (mine && row) out[p] = acc;
            seg_b = seg_e;
        }
    }
}

int launch_dense_pairs(const PairSeg* d_segs, int n_segs, int dtype, const float* Q, int64_t nq, int H, const int64_t* d_cand_indptr,
                       const int64_t* d_cand_ids, float* d_out, PairStatus* d_status, hipStream_t s) {
    // 8 one-wave workgroups per compute unit: 8 x 16 KB of rows in flight per unit, LDS 17 KB each
    if (dtype == SR_DTYPE_F16)
        hipLaunchKernelGGL(dense_pairs_kernel<_Float16>, dim3((unsigned)(sr_cu_count() * 8)), dim3(64), 0, s, d_segs, n_segs, Q, nq, H,
                           d_cand_indptr, d_cand_ids, d_out, d_status);
    else
        hipLaunchKernelGGL(dense_pairs_kernel<float>, dim3((unsigned)(sr_cu_count() * 8)), dim3(64), 0, s, d_segs, n_segs, Q, nq, H,
                           d_cand_indptr, d_cand_ids, d_out, d_status);
    SR_CHECK_LAUNCH();
    return SR_OK;
}

// ---------------------------------------------------------------------------------------------------- sparse ---
// One wave per pair; out[p] = scores[doc] of the reference's term-serial chain (scaling_retriever/indexer.py:324-340): for each
// query term in the query's order, s = s + q_t * v, unfused, from +0.0f.  Two routes to the matching postings, the same bits:
//   forward  (the index has the certified scorer's doc-major forward index and the query's terms are valid and strictly
//            ascending): lane = posting of the document's row, its term looked up in the query's sorted terms; the row's
//            ascending term order IS the query's order.  Reads the row (8 bytes per posting) and the cache-resident query.
//   postings (every other case: unordered or repeated query terms, unknown term ids, no forward index): lane = query term,
//            binary search of the document in that term's doc-sorted posting list - all terms of a chunk search side by side.
// Then the ordered sum: the matching lanes' products are added one after the other, lowest lane first.  A lane without a match
// adds nothing (s is never -0.0f: it starts at +0.0f and a sum is -0.0f only when both operands are).
struct SparsePairArgs {
    const int64_t* indptr; const int32_t* doc_ids; const float* vals;
    int64_t n_terms, n_docs;
    const int64_t* fwd_indptr; const uint64_t* fwd_tv;      // null: postings route only
    const uint8_t* q_ascending;                             // [nq] (with a forward index): the query's terms are valid and strictly ascending
    const int64_t* q_indptr; const int32_t* q_cols; const float* q_vals;
    int64_t nq;
    const int64_t* cand_indptr; const int64_t* cand_ids;
    float* out;
    PairStatus* st;
};
// once per query, not per pair: may the forward route serve it?
__global__ void sparse_pairs_query_kernel(const int64_t* __restrict__ q_indptr, const int32_t* __restrict__ q_cols, int64_t nq,
                                          int64_t n_terms, uint8_t* __restrict__ q_ascending) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    bool ok = true;
    int64_t prev = -1;
    for (int64_t i = q_indptr[q]; ok && i < q_indptr[q + 1]; ++i) {
        const int64_t t = q_cols[i];
        ok = t > prev && t < n_terms;
        prev = t;
    }
    q_ascending[q] = ok ? 1 : 0;
}

// idx->pair_qflags[q] for the nq queries of a call (grown on demand): may the forward route serve query q
int sparse_pair_query_flags(sr_sparse_index* idx, const int64_t* d_q_indptr, const int32_t* d_q_cols, int64_t nq, const char* who,
                            hipStream_t s) {
    if (idx->pair_qflags.reserve(nq, nullptr) != SR_OK) {
        sr_set_error("%s: out of device memory for %lld query flags", who, (long long)nq);
        return SR_ERR_NOMEM;
    }
    hipLaunchKernelGGL(sparse_pairs_query_kernel, dim3((unsigned)ceil_div64(nq, 256)), dim3(256), 0, s, d_q_indptr, d_q_cols, nq,
                       idx->n_terms, idx->pair_qflags.p);
    SR_CHECK_LAUNCH();
    return SR_OK;
}

__global__ __launch_bounds__(256) void sparse_pairs_kernel(SparsePairArgs a) {
#pragma clang fp contract(off)
    if (a.st->indptr_bad) return;
    const int lane = threadIdx.x & 63;
    const int64_t total = a.cand_indptr[a.nq];
    const int64_t n_waves = (int64_t)gridDim.x * 4;
    for (int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); p < total; p += n_waves) {
        const int64_t doc = a.cand_ids[p];
        if (doc < 0 || doc >= a.n_docs) {
            if (lane == 0) {
                atomicMin(&a.st->first_bad, (unsigned long long)p);
                a.out[p] = __builtin_nanf("");
            }
            continue;
        }
        const int64_t q = pair_query_of(a.cand_indptr, a.nq, p);
        const int64_t tb = a.q_indptr[q], te = a.q_indptr[q + 1];
        const bool forward = a.fwd_indptr != nullptr && a.q_ascending[q] != 0;
        const SparseChainIndex x{a.indptr, a.doc_ids, a.vals, a.n_terms, a.fwd_indptr, a.fwd_tv};
        const float s = sparse_pair_chain(x, a.q_cols, a.q_vals, tb, te, forward, doc, lane);
        if (lane == 0) a.out[p] = s;
    }
}

extern "C" int sr_sparse_score_pairs(sr_sparse_index* idx, const int64_t* d_q_indptr, const int32_t* d_q_cols, const float* d_q_vals,
                                     int64_t nq, const int64_t* d_cand_indptr, const int64_t* d_cand_ids, float* d_out_scores,
                                     sr_stream stream) {
    SR_REQUIRE(idx, "sr_sparse_score_pairs: null index");
    SR_REQUIRE(nq >= 0 && nq < (1ll << 30), "sr_sparse_score_pairs: bad nq");
    if (nq == 0) return SR_OK;
    SR_REQUIRE(d_q_indptr && d_q_cols && d_q_vals && d_cand_indptr && d_cand_ids && d_out_scores, "sr_sparse_score_pairs: null pointer");
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(idx->mu);
    StreamOrder::Scope in_order(idx->order, s);
    SR_TRY(pair_status_begin(&idx->pair_status, d_cand_indptr, nq, s));
    SparsePairArgs a;
    a.indptr = idx->indptr; a.doc_ids = idx->doc_ids; a.vals = idx->vals;
    a.n_terms = idx->n_terms; a.n_docs = idx->n_docs;
    a.fwd_indptr = nullptr; a.fwd_tv = nullptr;
    // dev switch SR_PAIR_SPARSE_ROUTE=postings: every pair through the posting lists (tests compare the two routes)
    const char* route = sr_dev_getenv("SR_PAIR_SPARSE_ROUTE");
    if (!(route && strcmp(route, "postings") == 0)) sparse_cert_forward_index(idx->cert, &a.fwd_indptr, &a.fwd_tv);
    a.q_ascending = nullptr;
    if (a.fwd_indptr) {
        SR_TRY(sparse_pair_query_flags(idx, d_q_indptr, d_q_cols, nq, "sr_sparse_score_pairs", s));
        a.q_ascending = idx->pair_qflags.p;
    }
    a.q_indptr = d_q_indptr; a.q_cols = d_q_cols; a.q_vals = d_q_vals; a.nq = nq;
    a.cand_indptr = d_cand_indptr; a.cand_ids = d_cand_ids; a.out = d_out_scores; a.st = idx->pair_status;
    hipLaunchKernelGGL(sparse_pairs_kernel, dim3((unsigned)(sr_cu_count() * 8)), dim3(256), 0, s, a);
    SR_CHECK_LAUNCH();
    return pair_status_end(idx->pair_status, d_cand_ids, "sr_sparse_score_pairs", s);
}
