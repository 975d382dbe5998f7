// Diversified sparse search: exact greedy Maximal Marginal Relevance over a candidate list per query, on the documents'
// forward rows (a doc-major CSR, terms ascending inside a row: SparseIndexHIP.forward_rows()).  No reference counterpart: it extends
// SparseRetrieval.retrieve (scaling_retriever/indexer.py:310-430), whose result nothing diversifies.
//   sr_sparse_mmr  stateless, one workgroup per query runs all k picks.  Set-up: every valid candidate keeps in LDS the 64-bit offset
//                  and the length of its row (length -1: "not a candidate (any more)"), its id, f32(lambda * rel), its running m = the
//                  largest similarity to a selected row, its norm (cosine) and the partial sum of its chain.  A pick: the row picked
//                  last is staged in LDS as (term, value) pairs, in chunks of ascending terms; one wave per live candidate runs
//                  sparse_pair_chain's forward route against the chunk - a lane takes one entry of the candidate's row per 64-entry
//                  step, binary searches the chunk for its term, and the products of the lanes that found theirs are added in lane
//                  order (ballot + readlane): ascending terms, one rounded fp32 add each, bit for bit sr_sparse_score_pairs' score of
//                  (row i as the query, document j).  A row longer than a chunk continues its chain from the saved partial sum: the
//                  chunks come in term order, so the order of the sum is the same.  Then m = sim > m ? sim : m,
//                  v = f32(f32(lambda * rel) - f32(mu * m)) with contraction off, and dense_mmr.hip's workgroup reduction picks the
//                  best by (v descending as floats, -0.0 == +0.0; id ascending; position ascending): no atomic decides an output byte.
// Row offsets, not row pointers, go through LDS: the loads of a row are global loads off the kernel's own arguments.  The next step
// of a row is loaded before the current one is searched, every lane, always (a lane beyond the row re-reads its last entry).  Inside a
// pick the barriers order LDS alone.  Every loop is bounded by k, n and the rows' lengths; workgroups never communicate.  The ids are
// checked by a kernel of their own first: once it found a position outside [0, n_docs), every query's outputs are padding and no row
// offset is ever read for it.
#include "mmr_select.h"
#include "pair_score.h"
#include <float.h>
#include <math.h>

#define SMMR_CHUNK 512                  // (term, value) pairs of the picked row staged at a time: 4 KB of LDS
#define SMMR_CAND_BYTES 36

struct SparseMmrArgs {
    const int64_t* indptr; const int32_t* cols; const float* vals;
    int64_t n_docs;
    int n, k, sim_mode, chunk;
    const int64_t* ids; const float* rel; const int32_t* counts;
    float lambda, mu;
    int64_t* out_ids; float* out_rel; float* out_mmr; int32_t* out_pos; int32_t* out_counts;
    const unsigned long long* first_bad;
};

// first_bad = min(first_bad, q * n + i) for every valid entry (i < list_count, id >= 0) of ids [nq, n] that is no position of the CSR
__global__ void sparse_mmr_check_kernel(const int64_t* __restrict__ ids, const int32_t* __restrict__ counts, int64_t nq, int n, int64_t n_docs,
                                        unsigned long long* __restrict__ first_bad) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nq * n) return;
    const int64_t q = p / n;
    const int i = (int)(p - q * n);
    if (i < list_count(counts, q, n) && ids[p] >= n_docs) atomicMin(first_bad, (unsigned long long)p);
}

// s := s + the products in lane order, of the lanes with m set (wave-uniform s)
__device__ inline float smmr_ordered_add(float s, bool m, float prod) {
#pragma clang fp contract(off)
    uint64_t mm = __ballot(m);
    while (mm) {
        const int i = __builtin_ctzll(mm);
        mm &= mm - 1;
        s = s + __int_as_float(__builtin_amdgcn_readlane(__float_as_int(prod), i));
    }
    return s;
}

// One wave: the chain of the row [b, b + len) continued from s over its terms that the staged chunk ct / cv [0, cn) holds (SELF: over
// all its terms, against itself - ip(i, i)).  len > 0.
template <bool SELF>
__device__ inline float smmr_chain(const SparseMmrArgs& a, int64_t b, int len, const int32_t* ct, const float* cv, int cn, float s, int lane) {
#pragma clang fp contract(off)
    const int32_t tlo = SELF ? 0 : ct[0], thi = SELF ? 0 : ct[cn - 1];
    int o = lane < len ? lane : len - 1;
    int32_t t = a.cols[b + o];
    float v = a.vals[b + o];
    for (int off = 0; off < len; off += 64) {
        o = off + 64 + lane < len ? off + 64 + lane : len - 1;  // the next step, in flight while this one is searched
        const int32_t t_next = a.cols[b + o];
        const float v_next = a.vals[b + o];
        bool m = off + lane < len;
        float prod = 0.f;
        if (SELF) {
            prod = v * v;
        } else {
            m = m && t >= tlo && t <= thi;
            if (m) {
                int lo = 0, hi = cn;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (ct[mid] < t) lo = mid + 1; else hi = mid;
                }
                m = lo < cn && ct[lo] == t;
                if (m) prod = cv[lo] * v;
            }
        }
        s = smmr_ordered_add(s, m, prod);
        t = t_next;
        v = v_next;
    }
    return s;
}

__global__ __launch_bounds__(64 * MMR_MAX_WAVES) void sparse_mmr_kernel(SparseMmrArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    __shared__ MmrKey red[MMR_MAX_WAVES];
    __shared__ float s_best_v;
    const int n = a.n, tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nw = blockDim.x >> 6, nt = blockDim.x;
    int64_t* s_beg = reinterpret_cast<int64_t*>(smem_raw);      // [n] first entry of the candidate's row
    int64_t* s_id = s_beg + n;                                  // [n]
    int* s_len = reinterpret_cast<int*>(s_id + n);              // [n] entries of the row; -1: padding, or selected
    float* s_lr = reinterpret_cast<float*>(s_len + n);          // [n] f32(lambda * rel)
    float* s_m = s_lr + n;                                      // [n] largest similarity to a selected row
    float* s_norm = s_m + n;                                    // [n] f32(sqrt(ip(i, i))), cosine only
    float* s_acc = s_norm + n;                                  // [n] the chain's sum after the chunks so far
    int32_t* s_ct = reinterpret_cast<int32_t*>(s_acc + n);      // [chunk] the picked row's terms
    float* s_cv = reinterpret_cast<float*>(s_ct + a.chunk);     // [chunk] and values
    const int64_t q = blockIdx.x;
    const int64_t* ids = a.ids + q * n;
    const float* rel = a.rel + q * n;
    const int kk = a.k < n ? a.k : n;
    const bool cosine = a.sim_mode == SR_MMR_SIM_COSINE;

    int picked = 0;
    if (*a.first_bad == ~0ull) {                                // the check ran before this launch on the same stream
        const int cnt = list_count(a.counts, q, n);
        MmrKey mine;
        mine.ord = 0; mine.pos = -1; mine.id = 0;
        for (int i = tid; i < n; i += nt) {
            const int64_t id = ids[i];
            const bool valid = i < cnt && id >= 0 && id < a.n_docs;
            int64_t b = 0, e = 0;
            if (valid) {
                b = a.indptr[id];
                e = a.indptr[id + 1];
            }
            const float r = rel[i];
            s_beg[i] = b;
            s_id[i] = id;
            s_len[i] = valid ? (e > b ? (int)(e - b) : 0) : -1;
            s_lr[i] = a.lambda * r;
            s_m[i] = -INFINITY;
            s_norm[i] = 0.f;
            if (valid) {
                MmrKey c;
                c.ord = sr_f2ord(r); c.pos = i; c.id = id;
                if (mmr_better(c, mine)) mine = c;
            }
        }
        __syncthreads();
        if (cosine)
            for (int i = w; i < n; i += nw) {                   // a wave per candidate: its chain against itself
                const int len = s_len[i];
                if (len <= 0) continue;                         // an empty row: norm = sqrt(+0.0) = 0
                const float s = smmr_chain<true>(a, s_beg[i], len, nullptr, nullptr, 0, 0.f, lane);
                if (lane == 0) s_norm[i] = sqrtf(s);
            }
        MmrKey best = mmr_block_best(mine, red, nw);            // pick 0: by (rel, id, position); its barriers stand behind s_norm
        float best_v = best.pos >= 0 ? s_lr[best.pos] : 0.f;
        while (best.pos >= 0) {
            const int64_t pb = s_beg[best.pos];
            const int pl = s_len[best.pos];
            const float pnorm = s_norm[best.pos];
            __syncthreads();                                    // every thread holds the picked row
            if (tid == 0) {
                const int64_t o = q * a.k + picked;
                a.out_ids[o] = best.id;
                a.out_rel[o] = rel[best.pos];
                a.out_mmr[o] = best_v;
                a.out_pos[o] = best.pos;
                s_len[best.pos] = -1;
            }
            ++picked;
            __syncthreads();
            if (picked >= kk) break;

            mine.ord = 0; mine.pos = -1; mine.id = 0;
            float mine_v = 0.f;
            const int nch = pl > 0 ? (pl + a.chunk - 1) / a.chunk : 1;  // an empty picked row: one round, every similarity +0.0
            for (int c = 0; c < nch; ++c) {
                const int c0 = c * a.chunk;
                const int cn = pl - c0 < a.chunk ? pl - c0 : a.chunk;
                if (c > 0) mmr_lds_barrier();                   // the previous chunk is consumed
                for (int j = tid; j < cn; j += nt) {
                    s_ct[j] = a.cols[pb + c0 + j];
                    s_cv[j] = a.vals[pb + c0 + j];
                }
                mmr_lds_barrier();
                const bool last = c + 1 == nch;
                for (int i = w; i < n; i += nw) {               // a wave per live candidate
                    const int len = s_len[i];
                    if (len < 0) continue;
                    float s = c == 0 ? 0.f : s_acc[i];
                    if (cn > 0 && len > 0) s = smmr_chain<false>(a, s_beg[i], len, s_ct, s_cv, cn, s, lane);
                    if (!last) {
                        if (lane == 0) s_acc[i] = s;            // read back by this wave alone, behind the next chunk's barriers
                        continue;
                    }
                    float sim = s;
                    if (cosine) {
                        const float den = s_norm[i] * pnorm;
                        sim = den > 0.f ? s / den : 0.f;
                    }
                    const float m_old = s_m[i];
                    const float m = sim > m_old ? sim : m_old;
                    if (lane == 0) s_m[i] = m;
                    const float pen = a.mu * m;
                    const float v = s_lr[i] - pen;
                    MmrKey cand;
                    cand.ord = sr_f2ord(v); cand.pos = i; cand.id = s_id[i];
                    if (mmr_better(cand, mine)) {
                        mine = cand;
                        mine_v = v;
                    }
                }
            }
            best = mmr_block_best(mine, red, nw);
            // the winner's v, bits untouched (its key folds -0.0 into +0.0): from the wave that owns it (every lane holds the same v)
            if (best.pos >= 0 && mine.pos == best.pos && lane == 0) s_best_v = mine_v;
            __syncthreads();
            best_v = s_best_v;
        }
    }
    for (int i = picked + tid; i < a.k; i += nt) {
        const int64_t o = q * a.k + i;
        a.out_ids[o] = -1;
        a.out_rel[o] = -FLT_MAX;
        a.out_mmr[o] = -FLT_MAX;
        a.out_pos[o] = -1;
    }
    if (tid == 0) a.out_counts[q] = picked;
}

static int smmr_chunk() {
    int chunk = SMMR_CHUNK;
    if (const char* e = sr_dev_getenv("SR_MMR_SPARSE_CHUNK")) {         // dev switch, read per call: short rows cross chunk boundaries
        const int v = atoi(e);
        if (v >= 1 && v < chunk) chunk = v;
    }
    return chunk;
}

extern "C" int sr_sparse_mmr(const int64_t* d_doc_indptr, const int32_t* d_doc_cols, const float* d_doc_vals, int64_t n_docs,
                             const int64_t* d_ids, const float* d_rel, const int32_t* d_counts, int64_t nq, int64_t n, int k, float lambda,
                             int sim_mode, int64_t* d_out_ids, float* d_out_rel, float* d_out_mmr, int32_t* d_out_pos,
                             int32_t* d_out_counts, sr_stream stream) {
    SR_REQUIRE(nq >= 0 && nq < (1ll << 28), "sr_sparse_mmr: bad nq=%lld", (long long)nq);
    SR_REQUIRE(n >= 1 && n <= MMR_MAX_N, "sr_sparse_mmr: %lld candidates per query: 1 to %d (sr_mmr_max_candidates) are held in LDS", (long long)n,
               MMR_MAX_N);
    SR_REQUIRE(k >= 1 && k <= n, "sr_sparse_mmr: k = %d, 1 to n = %lld are selected", k, (long long)n);
    SR_REQUIRE(lambda >= 0.f && lambda <= 1.f, "sr_sparse_mmr: lambda = %g is not in [0, 1]", (double)lambda);
    SR_REQUIRE(sim_mode == SR_MMR_SIM_IP || sim_mode == SR_MMR_SIM_COSINE, "sr_sparse_mmr: sim_mode = %d is neither SR_MMR_SIM_IP nor SR_MMR_SIM_COSINE",
               sim_mode);
    SR_REQUIRE(n_docs >= 0, "sr_sparse_mmr: bad n_docs=%lld", (long long)n_docs);
    if (nq == 0) return SR_OK;
    SR_REQUIRE(d_doc_indptr && d_doc_cols && d_doc_vals && d_ids && d_rel && d_out_ids && d_out_rel && d_out_mmr && d_out_pos && d_out_counts,
               "sr_sparse_mmr: null pointer");
    hipStream_t s = (hipStream_t)stream;

    CallStatus<unsigned long long> d_status;
    SR_TRY(d_status.begin("sr_sparse_mmr", s));
    hipLaunchKernelGGL(sparse_mmr_check_kernel, dim3((unsigned)ceil_div64(nq * n, 256)), dim3(256), 0, s, d_ids, d_counts, nq, (int)n, n_docs,
                       d_status.p);
    SR_CHECK_LAUNCH();

    SparseMmrArgs a;
    a.indptr = d_doc_indptr; a.cols = d_doc_cols; a.vals = d_doc_vals; a.n_docs = n_docs;
    a.n = (int)n; a.k = k; a.sim_mode = sim_mode; a.chunk = smmr_chunk();
    a.ids = d_ids; a.rel = d_rel; a.counts = d_counts;
    a.lambda = lambda; a.mu = 1.0f - lambda;
    a.out_ids = d_out_ids; a.out_rel = d_out_rel; a.out_mmr = d_out_mmr; a.out_pos = d_out_pos; a.out_counts = d_out_counts;
    a.first_bad = d_status.p;
    // a wave per candidate, up to 8; at the cap 36 KB of candidates and 4 KB of chunk: inside the 64 KB every launch may take
    const int nw = n < MMR_MAX_WAVES ? (int)n : MMR_MAX_WAVES;
    const size_t lds = (size_t)SMMR_CAND_BYTES * (size_t)n + 8 * (size_t)a.chunk;
    hipLaunchKernelGGL(sparse_mmr_kernel, dim3((unsigned)nq), dim3(64 * nw), lds, s, a);
    SR_CHECK_LAUNCH();

    unsigned long long first_bad = 0;
    SR_TRY(d_status.read(&first_bad, s));
    if (first_bad != ~0ull) {
        int64_t id = 0;
        SR_CHECK_HIP(hipMemcpy(&id, d_ids + first_bad, sizeof(id), hipMemcpyDeviceToHost));
        sr_set_error("sr_sparse_mmr: candidate id %lld (query %llu, entry %llu) is not a position in [0, %lld) (nothing was selected)", (long long)id,
                     first_bad / (unsigned long long)n, first_bad % (unsigned long long)n, (long long)n_docs);
        return SR_ERR_INVALID;
    }
    return SR_OK;
}
