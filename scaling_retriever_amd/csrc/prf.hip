// Pseudo-relevance feedback: Rocchio's rebuilt query for both heads, w = alpha q + beta / p sum(positive documents) -
// gamma / g sum(negative documents), from the first p and the last g valid entries of a ranked list per query.  No reference
// counterpart: its retrievers (scaling_retriever/indexer.py:191-217, :310-430) search with the query as it was encoded.
//   sr_sparse_feedback  one workgroup per query.  The query row and the rows of the at most 128 documents used are staged as 64-bit
//                       words term << 33 | source << 25 | slot (source 0 = the query, then the positive documents in list order, then
//                       the negative ones; slot = the entry's place in a value array beside the words) and sorted ascending (bitonic), so
//                       the entries of one term are adjacent and in list order.  The thread that finds a run's head walks it: q_t, then
//                       P_t and N_t one rounded fp32 add at a time - that fixes the order of the sums - and leaves w_t (or 0: dropped) in
//                       the head's value slot.  The kept heads are compacted in term order by a workgroup scan; under a term budget their
//                       keys f2ord(w) << 32 | ~term are sorted descending, the first max_terms re-keyed by term and sorted back.  Terms are
//                       unique per key: a total order, no atomic decides an output byte.  The words and values live in LDS up to
//                       sr_prf_max_entries() entries; a query above that runs the SAME kernel on a global-memory workspace (a workgroup's
//                       barriers order its global stores as they order its LDS stores).  A CSR needs the row sizes first, so the kernel
//                       runs twice, as sr_sparse_compact's pair does: a count pass that stops after the run sums, the scan of the
//                       counts, the one read-back of the total (capacity), the fill pass.
//   sr_dense_feedback   one workgroup per query; a thread owns one 16-byte piece of the row (4 fp32 / 8 fp16 columns) and adds the
//                       documents' pieces in list order, every row piece loaded once.
// The coefficients f32(beta / f32(p)), f32(gamma / f32(g)) come from two host-computed tables in the kernel arguments: no division on
// the device.  All arithmetic under contract(off): alpha * q + cp * P must stay two products and a sum.
#include "block_primitives.h"
#include "dense_index.h"
#include "subset_search.h"
#include <float.h>
#include <math.h>
#include <vector>

#define PRF_THREADS 256                 // sr_block_scan's four waves
#define PRF_MAX_SET 64                  // n_pos, n_neg
#define PRF_MAX_DOCS (2 * PRF_MAX_SET)
#define PRF_LDS_ENTRIES 8192            // sr_prf_max_entries(): 12 bytes of LDS per entry
#define PRF_SLOT_BITS 25                // entries of one query on the workspace route: below 2^25
#define PRF_TERM_SHIFT 33
#define PRF_PAD (~0ull)                 // an unused slot: sorts behind every entry (an entry's source is <= 128)
#define PRF_HEAD_BYTES 2608             // s_doc, s_start, s_off, lw in front of the words: a multiple of 16
#define PRF_WS_BUDGET (1ll << 30)       // workspace of one batch of queries above the LDS cap

struct PrfStatus {                      // device words of a call: what the kernels found wrong (~0: nothing)
    unsigned long long first_bad;       // smallest flat position of fb_ids whose valid entry names no document
    unsigned long long bad_query;       // smallest query whose columns are not strictly ascending inside [0, n_terms)
};

struct PrfCoef {
    float alpha;
    float cp[PRF_MAX_SET], cn[PRF_MAX_SET];     // [p - 1], [g - 1]
};

// The feedback sets of one query, by the whole workgroup: v = the entries i < cnt with fb[i] >= 0 in list order; s_doc[0, p) := the
// first p = min(n_pos, |v|) of them, s_doc[p, p + g) := the last g = min(n_neg, |v| - p).  lw: 4 LDS words.  Ends with a barrier.
__device__ inline void prf_sets(const int64_t* __restrict__ fb, int cnt, int n_pos, int n_neg, int64_t* s_doc, int* lw, int& p, int& g) {
    const int tid = threadIdx.x;
    int nv = 0;
    for (int i0 = 0; i0 < cnt; i0 += PRF_THREADS) {
        const int i = i0 + tid;
        int tot;
        (void)sr_block_scan(i < cnt && fb[i] >= 0 ? 1 : 0, lw, tot);
        nv += tot;
    }
    p = n_pos < nv ? n_pos : nv;
    g = n_neg < nv - p ? n_neg : nv - p;
    const int neg0 = nv - g;
    int base = 0;
    for (int i0 = 0; i0 < cnt && (base < p || g > 0); i0 += PRF_THREADS) {
        const int i = i0 + tid;
        const int64_t id = i < cnt ? fb[i] : -1;
        int tot;
        const int r = base + sr_block_scan(id >= 0 ? 1 : 0, lw, tot);
        if (id >= 0) {
            if (r < p) s_doc[r] = id;
            if (r >= neg0) s_doc[p + r - neg0] = id;
        }
        base += tot;
    }
    __syncthreads();
}

// ------------------------------------------------------------------------------------------------------------------ sparse: plan
// Per query: every valid feedback entry names a document, the query's columns are strictly ascending inside [0, n_terms), and
// ent[q] := the query's terms plus all terms of the documents used.
struct PrfPlanArgs {
    const int64_t* q_indptr; const int32_t* q_cols;
    const int64_t* d_indptr;
    int64_t n_docs, n_terms;
    const int64_t* fb; const int32_t* counts;
    int depth, n_pos, n_neg;
    PrfStatus* st;
    int64_t* ent;
};

__global__ __launch_bounds__(PRF_THREADS) void prf_plan_kernel(PrfPlanArgs a) {
    __shared__ int64_t s_doc[PRF_MAX_DOCS];
    __shared__ int lw[4];
    const int tid = threadIdx.x;
    const int64_t q = blockIdx.x;
    const int64_t* fb = a.fb + q * a.depth;
    const int cnt = list_count(a.counts, q, a.depth);
    int bad = 0;
    for (int i = tid; i < cnt; i += PRF_THREADS)
        if (fb[i] >= a.n_docs) {
            atomicMin(&a.st->first_bad, (unsigned long long)(q * a.depth + i));
            bad = 1;
        }
    const int64_t q0 = a.q_indptr[q], q1 = a.q_indptr[q + 1];
    int unordered = q1 < q0 ? 1 : 0;
    for (int64_t i = q0 + tid; i < q1; i += PRF_THREADS) {
        const int32_t c = a.q_cols[i];
        if (c < 0 || c >= a.n_terms || (i > q0 && a.q_cols[i - 1] >= c)) unordered = 1;
    }
    int any_bad, any_unordered;
    (void)sr_block_scan(bad, lw, any_bad);
    (void)sr_block_scan(unordered, lw, any_unordered);
    if (any_unordered && tid == 0) atomicMin(&a.st->bad_query, (unsigned long long)q);
    if (any_bad || any_unordered) {                             // uniform: nothing of this query is read further
        if (tid == 0) a.ent[q] = 0;
        return;
    }
    int p, g;
    prf_sets(fb, cnt, a.n_pos, a.n_neg, s_doc, lw, p, g);
    // the row sizes as two 32-bit halves through the int scan: a document row holds fewer than 2^31 terms
    int64_t len = 0;
    if (tid < p + g) len = a.d_indptr[s_doc[tid] + 1] - a.d_indptr[s_doc[tid]];
    if (len < 0) len = 0;
    int lo, hi;
    (void)sr_block_scan((int)(len & 0xffff), lw, lo);
    (void)sr_block_scan((int)(len >> 16), lw, hi);
    if (tid == 0) a.ent[q] = (q1 - q0) + (int64_t)lo + ((int64_t)hi << 16);
}

// --------------------------------------------------------------------------------------------------------------- sparse: feedback
struct PrfArgs {
    const int64_t* q_indptr; const int32_t* q_cols; const float* q_vals;
    const int64_t* d_indptr; const int32_t* d_cols; const float* d_vals;
    const int64_t* fb; const int32_t* counts;
    int depth, n_pos, n_neg, max_terms;
    int lds_entries;                    // LDS route: the entries the launch's LDS holds
    PrfCoef coef;
    const int64_t* jobs;                // [n, 2] (query, byte offset of its workspace), or null: workgroup b serves query b in LDS
    unsigned char* ws;
    int64_t* row_cnt;                   // count pass: [nq]
    const int64_t* row_ptr;             // fill pass
    int32_t* out_cols; float* out_vals;
};

template <bool FILL, bool WS>
__global__ __launch_bounds__(PRF_THREADS) void prf_sparse_kernel(PrfArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    int64_t* s_doc = reinterpret_cast<int64_t*>(smem_raw);                      // [128] the documents used, by source - 1
    int64_t* s_start = s_doc + PRF_MAX_DOCS;                                    // [130] first posting of every source's row
    int* s_off = reinterpret_cast<int*>(s_start + PRF_MAX_DOCS + 2);            // [132] first slot of every source, then the total
    int* lw = s_off + PRF_MAX_DOCS + 4;                                         // [4]
    const int tid = threadIdx.x;
    const int64_t q = a.jobs ? a.jobs[2 * (int64_t)blockIdx.x] : (int64_t)blockIdx.x;

    int p, g;
    prf_sets(a.fb + q * a.depth, list_count(a.counts, q, a.depth), a.n_pos, a.n_neg, s_doc, lw, p, g);
    const int S = 1 + p + g;
    if (tid < S) {
        const int64_t r0 = tid == 0 ? a.q_indptr[q] : a.d_indptr[s_doc[tid - 1]];
        const int64_t r1 = tid == 0 ? a.q_indptr[q + 1] : a.d_indptr[s_doc[tid - 1] + 1];
        s_start[tid] = r0;
        s_off[tid + 1] = r1 > r0 ? (int)(r1 - r0) : 0;
    }
    __syncthreads();
    if (tid == 0) {
        s_off[0] = 0;
        for (int s = 0; s < S; ++s) s_off[s + 1] += s_off[s];
    }
    __syncthreads();
    const int ent = s_off[S];
    if (!WS && ent > a.lds_entries) {                           // never: the host sent this query to the workspace route
        if (!FILL && tid == 0) a.row_cnt[q] = 0;
        return;
    }
    const int P = sr_pow2_at_least(ent, 2);
    uint64_t* keys;
    float* vals;
    if (WS) {
        keys = reinterpret_cast<uint64_t*>(a.ws + a.jobs[2 * (int64_t)blockIdx.x + 1]);
        vals = reinterpret_cast<float*>(keys + P);
    } else {
        keys = reinterpret_cast<uint64_t*>(smem_raw + PRF_HEAD_BYTES);
        vals = reinterpret_cast<float*>(keys + P);
    }

    for (int e = tid; e < P; e += PRF_THREADS) {
        uint64_t key = PRF_PAD;
        if (e < ent) {
            int lo = 0, hi = S;                                 // the source of slot e: the last s with s_off[s] <= e
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (s_off[mid] <= e) lo = mid; else hi = mid;
            }
            const int64_t at = s_start[lo] + (e - s_off[lo]);
            const uint32_t term = (uint32_t)(lo == 0 ? a.q_cols[at] : a.d_cols[at]);
            vals[e] = lo == 0 ? a.q_vals[at] : a.d_vals[at];
            key = ((uint64_t)term << PRF_TERM_SHIFT) | ((uint64_t)lo << PRF_SLOT_BITS) | (uint64_t)e;
        }
        keys[e] = key;
    }
    __syncthreads();
    sr_block_sort<PRF_THREADS, false>(keys, P);

    // every run's head: w of its term into the head's slot (0: dropped), 0 into the other slots of the run - a slot is read and
    // written by its run's head alone
    const float cp = p > 0 ? a.coef.cp[p - 1] : 0.f, cn = g > 0 ? a.coef.cn[g - 1] : 0.f;
    const uint64_t slot_mask = (1ull << PRF_SLOT_BITS) - 1;
    int kept = 0;
    for (int i = tid; i < ent; i += PRF_THREADS) {
        const uint64_t e = keys[i];
        const uint32_t term = (uint32_t)(e >> PRF_TERM_SHIFT);
        if (i > 0 && (uint32_t)(keys[i - 1] >> PRF_TERM_SHIFT) == term) continue;
        float w = 0.0f, sp = 0.0f, sn = 0.0f;
        for (int j = i; j < ent; ++j) {
            const uint64_t x = keys[j];
            if ((uint32_t)(x >> PRF_TERM_SHIFT) != term) break;
            const int s = (int)((x >> PRF_SLOT_BITS) & 0xffu);
            const int slot = (int)(x & slot_mask);
            const float v = vals[slot];
            if (j > i) vals[slot] = 0.0f;
            if (s == 0) w = a.coef.alpha * v;
            else if (s <= p) sp = sp + v;
            else sn = sn + v;
        }
        if (p > 0) {
            const float t = cp * sp;
            w = w + t;
        }
        if (g > 0) {
            const float t = cn * sn;
            w = w - t;
        }
        const bool keep = w > 0.0f;
        vals[(int)(e & slot_mask)] = keep ? w : 0.0f;
        kept += keep ? 1 : 0;
    }
    int K;
    (void)sr_block_scan(kept, lw, K);                           // its barriers stand behind the stores of vals
    const bool cut = a.max_terms > 0 && K > a.max_terms;
    const int m = cut ? a.max_terms : K;
    if (!FILL) {
        if (tid == 0) a.row_cnt[q] = m;
        return;
    }

    // the kept heads in term order, compacted: straight into the row, or (budget) to the front of the words as f2ord(w) << 32 | ~term.
    // A chunk's words are read before the scan's barriers and written behind them, at or in front of their own place.
    const int64_t row = a.row_ptr[q];
    int base = 0;
    for (int i0 = 0; i0 < ent; i0 += PRF_THREADS) {
        const int i = i0 + tid;
        uint32_t term = 0;
        float w = 0.0f;
        if (i < ent) {
            const uint64_t e = keys[i];
            term = (uint32_t)(e >> PRF_TERM_SHIFT);
            w = vals[(int)(e & slot_mask)];
        }
        int tot;
        const int at = base + sr_block_scan(w > 0.0f ? 1 : 0, lw, tot);
        if (w > 0.0f) {
            if (cut) {
                keys[at] = ((uint64_t)sr_f2ord(w) << 32) | (uint64_t)(~term);
            } else {
                a.out_cols[row + at] = (int32_t)term;
                a.out_vals[row + at] = w;
            }
        }
        base += tot;
    }
    if (!cut) return;
    const int P2 = sr_pow2_at_least(K, 2);                     // K <= ent: inside the words
    for (int i = K + tid; i < P2; i += PRF_THREADS) keys[i] = 0ull;     // below every key: the high word of a kept w is never 0
    __syncthreads();
    sr_block_sort<PRF_THREADS, true>(keys, P2);
    const int P3 = sr_pow2_at_least(m, 2);
    for (int i = tid; i < P3; i += PRF_THREADS) {
        uint64_t key = PRF_PAD;
        if (i < m) {
            const uint64_t k2 = keys[i];
            const uint32_t term = ~(uint32_t)(k2 & 0xffffffffu);
            key = ((uint64_t)term << 32) | (uint64_t)__float_as_uint(sr_ord2f((uint32_t)(k2 >> 32)));      // w > 0: its bits come back
        }
        keys[i] = key;                                          // slot i is read and written by this thread alone
    }
    __syncthreads();
    sr_block_sort<PRF_THREADS, false>(keys, P3);
    for (int i = tid; i < m; i += PRF_THREADS) {
        const uint64_t key = keys[i];
        a.out_cols[row + i] = (int32_t)(uint32_t)(key >> 32);
        a.out_vals[row + i] = __uint_as_float((uint32_t)(key & 0xffffffffu));
    }
}

// row_ptr [n + 1] := exclusive prefix of cnt [n], by one workgroup
__global__ __launch_bounds__(PRF_THREADS) void prf_scan_kernel(const int64_t* __restrict__ cnt, int64_t n, int64_t* __restrict__ row_ptr) {
    __shared__ int lw[4];
    int64_t base = 0;
    for (int64_t i0 = 0; i0 < n; i0 += PRF_THREADS) {
        const int64_t i = i0 + threadIdx.x;
        const int c = i < n ? (int)cnt[i] : 0;                  // a row holds fewer than 2^25 terms
        int tot;
        const int at = sr_block_scan(c, lw, tot);
        if (i < n) row_ptr[i] = base + at;
        base += tot;
    }
    if (threadIdx.x == 0) row_ptr[n] = base;
}

static int prf_check_arguments(const char* who, int64_t nq, int64_t depth, int n_pos, int n_neg, float alpha, float beta, float gamma) {
    SR_REQUIRE(nq >= 0 && nq < (1ll << 28), "%s: bad nq=%lld", who, (long long)nq);
    SR_REQUIRE(n_pos >= 1 && n_pos <= PRF_MAX_SET, "%s: n_pos = %d, 1 to %d documents are the positive set", who, n_pos, PRF_MAX_SET);
    SR_REQUIRE(n_neg >= 0 && n_neg <= PRF_MAX_SET, "%s: n_neg = %d, 0 to %d documents are the negative set", who, n_neg, PRF_MAX_SET);
    SR_REQUIRE(depth >= 1 && depth <= SR_MAX_TOPK, "%s: depth = %lld, a feedback list holds 1 to %d (sr_max_topk) entries", who,
               (long long)depth, SR_MAX_TOPK);
    SR_REQUIRE(alpha >= 0.f && alpha < INFINITY && beta >= 0.f && beta < INFINITY && gamma >= 0.f && gamma < INFINITY,
               "%s: alpha, beta and gamma must be finite and >= 0 (got %g, %g, %g)", who, (double)alpha, (double)beta, (double)gamma);
    return SR_OK;
}

static void prf_coefficients(PrfCoef* c, float alpha, float beta, float gamma) {
    c->alpha = alpha;
    for (int i = 0; i < PRF_MAX_SET; ++i) {
        c->cp[i] = beta / (float)(i + 1);
        c->cn[i] = gamma / (float)(i + 1);
    }
}

static int prf_lds_cap() {
    int cap = PRF_LDS_ENTRIES;
    if (const char* e = sr_dev_getenv("SR_PRF_MAX_ENTRIES")) {          // dev switch, read per call: small tests reach the workspace route
        const int v = atoi(e);
        if (v >= 1 && v < cap) cap = v;
    }
    return cap;
}

extern "C" int sr_prf_max_entries(void) { return prf_lds_cap(); }

template <bool FILL, bool WS>
static int prf_launch(const PrfArgs& a, int64_t n, size_t lds, hipStream_t s) {
    static DeviceOnce lds_set;
    SR_TRY(sr_allow_lds(lds_set, prf_sparse_kernel<FILL, WS>, PRF_HEAD_BYTES + 12 * PRF_LDS_ENTRIES));
    hipLaunchKernelGGL((prf_sparse_kernel<FILL, WS>), dim3((unsigned)n), dim3(PRF_THREADS), lds, s, a);
    SR_CHECK_LAUNCH();
    return SR_OK;
}

extern "C" int sr_sparse_feedback(const int64_t* d_q_indptr, const int32_t* d_q_cols, const float* d_q_vals, int64_t nq,
                                  const int64_t* d_doc_indptr, const int32_t* d_doc_cols, const float* d_doc_vals, int64_t n_docs,
                                  int64_t n_terms, const int64_t* d_fb_ids, const int32_t* d_counts, int64_t depth, int n_pos, int n_neg,
                                  float alpha, float beta, float gamma, int64_t max_terms, int64_t* d_row_ptr, int32_t* d_cols,
                                  float* d_vals, int64_t capacity, int64_t* h_nnz, sr_stream stream) {
    SR_TRY(prf_check_arguments("sr_sparse_feedback", nq, depth, n_pos, n_neg, alpha, beta, gamma));
    SR_REQUIRE(max_terms >= 0 && max_terms <= 0x7fffffff, "sr_sparse_feedback: max_terms %lld is negative (0 = no limit)", (long long)max_terms);
    SR_REQUIRE(n_docs >= 0 && n_terms >= 1 && n_terms < (1ll << 31), "sr_sparse_feedback: bad n_docs=%lld or n_terms=%lld", (long long)n_docs,
               (long long)n_terms);
    SR_REQUIRE(h_nnz && d_row_ptr, "sr_sparse_feedback: null pointer");
    if (nq == 0) { *h_nnz = 0; return SR_OK; }
    SR_REQUIRE(d_q_indptr && d_q_cols && d_q_vals && d_doc_indptr && d_doc_cols && d_doc_vals && d_fb_ids, "sr_sparse_feedback: null pointer");
    hipStream_t s = (hipStream_t)stream;

    CallBuf<int64_t> d_plan, d_cnt, d_jobs;     // d_plan: the two status words, then ent [nq]
    CallBuf<unsigned char> d_ws;
    SR_TRY(d_plan.reserve(nq + 2, "sr_sparse_feedback"));
    SR_TRY(d_cnt.reserve(nq, "sr_sparse_feedback"));
    PrfStatus* st = reinterpret_cast<PrfStatus*>(d_plan.p);
    SR_CHECK_HIP(hipMemsetAsync(st, 0xff, sizeof(PrfStatus), s));
    PrfPlanArgs pa;
    pa.q_indptr = d_q_indptr; pa.q_cols = d_q_cols; pa.d_indptr = d_doc_indptr; pa.n_docs = n_docs; pa.n_terms = n_terms;
    pa.fb = d_fb_ids; pa.counts = d_counts; pa.depth = (int)depth; pa.n_pos = n_pos; pa.n_neg = n_neg;
    pa.st = st; pa.ent = d_plan.p + 2;
    hipLaunchKernelGGL(prf_plan_kernel, dim3((unsigned)nq), dim3(PRF_THREADS), 0, s, pa);
    SR_CHECK_LAUNCH();
    std::vector<int64_t> h_plan((size_t)nq + 2);
    SR_CHECK_HIP(hipMemcpyAsync(h_plan.data(), d_plan.p, (size_t)(nq + 2) * 8, hipMemcpyDeviceToHost, s));
    SR_CHECK_HIP(hipStreamSynchronize(s));
    const unsigned long long first_bad = (unsigned long long)h_plan[0], bad_query = (unsigned long long)h_plan[1];
    if (first_bad != ~0ull) {
        int64_t id = 0;
        SR_CHECK_HIP(hipMemcpy(&id, d_fb_ids + first_bad, sizeof(id), hipMemcpyDeviceToHost));
        sr_set_error("sr_sparse_feedback: feedback id %lld (query %llu, entry %llu) is not a position in [0, %lld) (nothing was written)",
                     (long long)id, first_bad / (unsigned long long)depth, first_bad % (unsigned long long)depth, (long long)n_docs);
        return SR_ERR_INVALID;
    }
    SR_REQUIRE(bad_query == ~0ull, "sr_sparse_feedback: the columns of query %llu are not strictly ascending inside [0, %lld) (nothing was written)",
               bad_query, (long long)n_terms);

    // queries by route: LDS up to the cap, a global workspace above it, in batches of PRF_WS_BUDGET
    const int64_t* ent = h_plan.data() + 2;
    const int cap = prf_lds_cap();
    std::vector<int64_t> jobs;                  // the LDS queries (offset 0), then the workspace queries
    std::vector<int64_t> big;
    int64_t max_small = 0;
    for (int64_t q = 0; q < nq; ++q) {
        if (ent[q] >= (1ll << PRF_SLOT_BITS)) {
            sr_set_error("sr_sparse_feedback: query %lld and its feedback documents hold %lld entries, at most %lld are merged", (long long)q,
                         (long long)ent[q], (1ll << PRF_SLOT_BITS) - 1);
            return SR_ERR_UNSUPPORTED;
        }
        if (ent[q] > cap) big.push_back(q);
        else if (ent[q] > max_small) max_small = ent[q];
    }
    const int64_t n_small = nq - (int64_t)big.size();
    auto ws_bytes = [&](int64_t q) { return (int64_t)sr_pow2_at_least(ent[q], 2) * 8 + (ent[q] + 3) / 4 * 16; };
    struct Batch { int64_t first, n, bytes; };
    std::vector<Batch> batches;
    int64_t ws_max = 0;
    if (!big.empty()) {
        for (int64_t q = 0; q < nq; ++q)
            if (ent[q] <= cap) { jobs.push_back(q); jobs.push_back(0); }
        Batch b{n_small, 0, 0};
        for (int64_t q : big) {
            const int64_t need = ws_bytes(q);
            if (b.n > 0 && b.bytes + need > PRF_WS_BUDGET) {
                batches.push_back(b);
                b = Batch{b.first + b.n, 0, 0};
            }
            jobs.push_back(q); jobs.push_back(b.bytes);
            b.n += 1;
            b.bytes += need;
        }
        batches.push_back(b);
        for (const Batch& x : batches) ws_max = x.bytes > ws_max ? x.bytes : ws_max;
        SR_TRY(d_jobs.reserve((int64_t)jobs.size(), "sr_sparse_feedback"));
        SR_TRY(d_ws.reserve(ws_max, "sr_sparse_feedback"));
        SR_CHECK_HIP(hipMemcpyAsync(d_jobs.p, jobs.data(), jobs.size() * 8, hipMemcpyHostToDevice, s));
    }

    PrfArgs a;
    a.q_indptr = d_q_indptr; a.q_cols = d_q_cols; a.q_vals = d_q_vals;
    a.d_indptr = d_doc_indptr; a.d_cols = d_doc_cols; a.d_vals = d_doc_vals;
    a.fb = d_fb_ids; a.counts = d_counts;
    a.depth = (int)depth; a.n_pos = n_pos; a.n_neg = n_neg; a.max_terms = (int)max_terms;
    a.lds_entries = (int)max_small;
    prf_coefficients(&a.coef, alpha, beta, gamma);
    a.ws = d_ws.p;
    a.row_cnt = d_cnt.p; a.row_ptr = d_row_ptr; a.out_cols = d_cols; a.out_vals = d_vals;
    const size_t lds = (size_t)PRF_HEAD_BYTES + (size_t)sr_pow2_at_least(max_small, 2) * 8 + (size_t)(max_small + 3) / 4 * 16;
    auto pass = [&](bool fill) -> int {
        if (n_small > 0) {
            a.jobs = big.empty() ? nullptr : d_jobs.p;
            if (fill) SR_TRY((prf_launch<true, false>(a, n_small, lds, s))); else SR_TRY((prf_launch<false, false>(a, n_small, lds, s)));
        }
        for (const Batch& b : batches) {        // one workspace: the stream runs the batches one after the other
            a.jobs = d_jobs.p + 2 * b.first;
            if (fill) SR_TRY((prf_launch<true, true>(a, b.n, PRF_HEAD_BYTES, s))); else SR_TRY((prf_launch<false, true>(a, b.n, PRF_HEAD_BYTES, s)));
        }
        return SR_OK;
    };
    int rc = pass(false);
    int64_t total = 0;
    if (rc == SR_OK) {
        hipLaunchKernelGGL(prf_scan_kernel, dim3(1), dim3(PRF_THREADS), 0, s, d_cnt.p, nq, d_row_ptr);
        if (hipMemcpyAsync(&total, d_row_ptr + nq, 8, hipMemcpyDeviceToHost, s) != hipSuccess) rc = SR_ERR_HIP;
    }
    if (hipStreamSynchronize(s) != hipSuccess && rc == SR_OK) rc = SR_ERR_HIP;      // the jobs' host copy is read until here
    if (rc == SR_ERR_HIP) sr_set_error("sr_sparse_feedback: %s", hipGetErrorString(hipGetLastError()));
    SR_TRY(rc);
    *h_nnz = total;
    if (total > capacity || (total > 0 && (!d_cols || !d_vals))) {
        sr_set_error("sr_sparse_feedback: %lld entries, capacity %lld", (long long)total, (long long)capacity);
        return SR_ERR_NOMEM;
    }
    if (total > 0) {
        rc = pass(true);
        if (rc != SR_OK || !batches.empty()) (void)hipStreamSynchronize(s);       // the workspace is freed when this call returns
        SR_TRY(rc);
    }
    return SR_OK;
}

// ---------------------------------------------------------------------------------------------------------------- dense: feedback
struct PrfDenseArgs {
    const PairSeg* segs; int n_segs;
    int H;
    const float* Q;
    const int64_t* fb; const int32_t* counts;
    int depth, n_pos, n_neg;
    PrfCoef coef;
    float* out;
    const PairStatus* st;
};

// a 16-byte piece of a stored row: 4 fp32 or 8 binary16 columns, widened exactly (common.h SrRow)
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
template <typename T> struct PrfPiece;
template <> struct PrfPiece<float> {
    typedef f32x4 V;
    static __device__ inline void widen(f32x4 v, f32x4* out) { out[0] = v; }
};
template <> struct PrfPiece<_Float16> {
    typedef f16x8 V;
    static __device__ inline void widen(f16x8 h, f32x4* out) {
        out[0] = f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
        out[1] = f32x4{(float)h[4], (float)h[5], (float)h[6], (float)h[7]};
    }
};

template <typename T>
__global__ __launch_bounds__(PRF_THREADS) void prf_dense_kernel(PrfDenseArgs a) {
#pragma clang fp contract(off)
    constexpr int PIECE = 16 / (int)sizeof(T);                  // columns of a 16-byte piece
    constexpr int NV = PIECE / 4;
    typedef typename PrfPiece<T>::V RowV;
    typedef const RowV __attribute__((address_space(1)))* GlobalRowV;   // a pointer out of LDS is generic to the compiler: the rows are global
    __shared__ int64_t s_doc[PRF_MAX_DOCS];
    __shared__ const T* s_row[PRF_MAX_DOCS];
    __shared__ int lw[4];
    const int tid = threadIdx.x, H = a.H;
    const int64_t q = blockIdx.x;
    if (a.st->first_bad != ~0ull) return;                       // the check ran before this launch on the same stream
    int p, g;
    prf_sets(a.fb + q * a.depth, list_count(a.counts, q, a.depth), a.n_pos, a.n_neg, s_doc, lw, p, g);
    if (tid < p + g) {
        int seg = 0;
        int64_t elem = 0;
        const bool held = pair_row_of(a.segs, a.n_segs, s_doc[tid], H, &seg, &elem);
        s_row[tid] = held ? static_cast<const T*>(a.segs[seg].rows) + elem : nullptr;
    }
    __syncthreads();
    const float cp = p > 0 ? a.coef.cp[p - 1] : 0.f, cn = g > 0 ? a.coef.cn[g - 1] : 0.f;
    for (int col = tid * PIECE; col < H; col += PRF_THREADS * PIECE) {
        f32x4 sp[NV], sn[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) sp[v] = sn[v] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int j = 0; j < p + g; ++j) {
            const T* r = s_row[j];
            if (!r) continue;                                   // never: the check kernel found every id
            const RowV x = *(GlobalRowV)(uintptr_t)(r + col);
            f32x4 y[NV];
            PrfPiece<T>::widen(x, y);
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                if (j < p) sp[v] = sp[v] + y[v]; else sn[v] = sn[v] + y[v];
            }
        }
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const f32x4 qv = *reinterpret_cast<const f32x4*>(a.Q + q * H + col + 4 * v);
            f32x4 w = a.coef.alpha * qv;
            if (p > 0) {
                const f32x4 t = cp * sp[v];
                w = w + t;
            }
            if (g > 0) {
                const f32x4 t = cn * sn[v];
                w = w - t;
            }
            *reinterpret_cast<f32x4*>(a.out + q * H + col + 4 * v) = w;
        }
    }
}

extern "C" int sr_dense_feedback(sr_dense_index* idx, const float* d_queries, int64_t nq, const int64_t* d_fb_ids, const int32_t* d_counts,
                                 int64_t depth, int n_pos, int n_neg, float alpha, float beta, float gamma, float* d_out, sr_stream stream) {
    SR_REQUIRE(idx, "sr_dense_feedback: null index");
    SR_TRY(prf_check_arguments("sr_dense_feedback", nq, depth, n_pos, n_neg, alpha, beta, gamma));
    if (nq == 0) return SR_OK;
    SR_REQUIRE(d_queries && d_fb_ids && d_out, "sr_dense_feedback: null pointer");
    SR_REQUIRE(((uintptr_t)d_queries & 15) == 0 && ((uintptr_t)d_out & 15) == 0, "sr_dense_feedback: queries and output must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(idx->mu);
    StreamOrder::Scope in_order(idx->order, s);
    SR_TRY(dense_pair_segs(idx, "sr_dense_feedback"));
    SR_TRY(subset_status_begin(&idx->pair_status, s));
    const int n_segs = (int)idx->pair_segs_n;
    SR_TRY(launch_id_list_check(idx->pair_segs.p, n_segs, idx->dim, d_fb_ids, d_counts, nq, (int)depth, idx->pair_status, s));
    PrfDenseArgs a;
    a.segs = idx->pair_segs.p; a.n_segs = n_segs; a.H = idx->dim; a.Q = d_queries;
    a.fb = d_fb_ids; a.counts = d_counts; a.depth = (int)depth; a.n_pos = n_pos; a.n_neg = n_neg;
    prf_coefficients(&a.coef, alpha, beta, gamma);
    a.out = d_out; a.st = idx->pair_status;
    if (idx->row_dtype == SR_DTYPE_F16)
        hipLaunchKernelGGL(prf_dense_kernel<_Float16>, dim3((unsigned)nq), dim3(PRF_THREADS), 0, s, a);
    else
        hipLaunchKernelGGL(prf_dense_kernel<float>, dim3((unsigned)nq), dim3(PRF_THREADS), 0, s, a);
    SR_CHECK_LAUNCH();
    PairStatus h;
    SR_CHECK_HIP(hipMemcpyAsync(&h, idx->pair_status, sizeof(h), hipMemcpyDeviceToHost, s));
    SR_CHECK_HIP(hipStreamSynchronize(s));
    if (h.first_bad != ~0ull) {
        int64_t id = 0;
        SR_CHECK_HIP(hipMemcpy(&id, d_fb_ids + h.first_bad, sizeof(id), hipMemcpyDeviceToHost));
        sr_set_error("sr_dense_feedback: feedback id %lld (query %llu, entry %llu) is not in the index (nothing was written)", (long long)id,
                     h.first_bad / (unsigned long long)depth, h.first_bad % (unsigned long long)depth);
        return SR_ERR_INVALID;
    }
    return SR_OK;
}
