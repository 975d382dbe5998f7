// Search within a document subset (gfx950): the top-k of sr_dense_search / sr_sparse_search restricted to ONE allow-list of documents
// shared by all queries of the call - what faiss offers as IDSelector on a flat index.  The reference has no counterpart: it extends
// DenseFlatIndexer.search_knn (scaling_retriever/indexer.py:191-217) and SparseRetrieval.numba_score_float + select_topk
// (scaling_retriever/indexer.py:315-344), which always rank the whole collection.
//
// Dense.  The pair scorer (pair_score.hip) fetches a document row once per pair: nq fetches of every row of a shared list.  Here a
// workgroup (one wave) gathers a tile of 64 subset rows ONCE for a block of SS_QB = 16 queries: every subset row is read from HBM at
// most ceil(nq / 16) times, not nq times.  Layout as dense_pairs_kernel: lane = row, the rows fetched 64 columns at a time as coalesced
// 256-byte pieces (16 lanes per row), transposed through a padded LDS tile, the next chunk's loads in flight while this one is
// processed; the query block's chunk [16][64] is staged in LDS next to it and read as broadcasts.  Every lane keeps 16 running fmaf
// chains, one per query of the block, each in the exact kernel's k order (per 8 columns k = 8s + j, then 8s + 4 + j): a (query,
// document) score is the bits of sr_dense_score_pairs and depends on nothing else in the call.  Scores never go to memory as an
// [nq, m] array: survivors of score >= tau[query] are appended as keys (score, doc index) to the handle's candidate buffer, one slab
// of the subset at a time, and folded into the running top-k by the select code every search uses (topk.hip, topk_large.hip) - the
// key holds the doc index of subset entry j itself, so ties fall as in sr_dense_search.
//
// Sparse.  Three routes, the same bits (the reference's term-serial unfused chain):
//   pairs  one wave per (query, subset document): sparse_pair_chain (sparse_pair_chain.h), the chain of sr_sparse_score_pairs.
//   array  one workgroup per (query, tile of 8 192 documents that holds a subset entry): the tile's slice of the reference's score
//          array in LDS, the query's terms applied one after the other with a barrier between them, then a gathered select over
//          scores[subset[j]] for the subset entries of the tile, compacted in ascending position order.
//   mask   the certified scorer's pass over the whole collection under the filter's bitmap (sparse_cert.hip): a document whose bit is
//          clear never becomes a stage-1 key; the re-score from the forward index returns the same chain.
// pairs and array keep score > threshold and score >= tau[query] and feed the same top-k.
//
// A bitmap per query (sr_sparse_search_grouped, at the end of this file): one pass of the certified scorer for all groups
// (cert_score_kernel<KS, true, true>), or the body of the masked search group by group.
#include "subset_search.h"
#include "doc_mask.h"
#include "filter_args.h"
#include "sparse_index.h"
#include "sparse_pair_chain.h"
#include <math.h>
#include <mutex>
#include <vector>

// ---------------------------------------------------------------------------------------------------- status ---
int subset_status_begin(PairStatus** d_status, hipStream_t s) {
    if (!*d_status) {
        if (hipMalloc((void**)d_status, sizeof(PairStatus)) != hipSuccess) {
            (void)hipGetLastError();
            *d_status = nullptr;
            sr_set_error("subset search: out of device memory for %zu status bytes", sizeof(PairStatus));
            return SR_ERR_NOMEM;
        }
    }
    SR_CHECK_HIP(hipMemsetAsync(&(*d_status)->first_bad, 0xff, sizeof(unsigned long long), s));
    SR_CHECK_HIP(hipMemsetAsync(&(*d_status)->indptr_bad, 0, 2 * sizeof(int), s));
    return SR_OK;
}

int subset_status_end(PairStatus* d_status, const int64_t* d_subset, const char* who, const char* what_id, hipStream_t s) {
    PairStatus h;
    SR_CHECK_HIP(hipMemcpyAsync(&h, d_status, sizeof(h), hipMemcpyDeviceToHost, s));
    SR_CHECK_HIP(hipStreamSynchronize(s));
    if (h.first_bad != ~0ull) {
        int64_t v[2] = {0, 0};
        const bool has_prev = h.first_bad > 0;
        SR_CHECK_HIP(hipMemcpy(v, d_subset + h.first_bad - (has_prev ? 1 : 0), sizeof(int64_t) * (has_prev ? 2 : 1), hipMemcpyDeviceToHost));
        if (has_prev && v[1] <= v[0])
            sr_set_error("%s: subset must be strictly ascending: position %llu holds %lld after %lld (nothing was searched)", who, h.first_bad,
                         (long long)v[1], (long long)v[0]);
        else
            sr_set_error("%s: subset position %llu: %s %lld is not in the index (nothing was searched)", who, h.first_bad, what_id,
                         (long long)v[has_prev ? 1 : 0]);
        return SR_ERR_INVALID;
    }
    return SR_OK;
}

int subset_plan(int64_t ws_limit, int64_t nq, int k, int64_t m, int64_t min_slab, int64_t* nq_batch, int64_t* slab, const char* who) {
    const int64_t large_bytes = k > SR_MAX_TOPK ? topk_large_bytes_per_query(k) : 0;
    const int64_t mm = m > 0 ? m : 1;
    const int64_t smallest = mm < min_slab ? mm : min_slab;
    const int64_t per_q = large_bytes + 8 * smallest;
    const int64_t b_max = ws_limit / per_q;
    if (b_max < 1) {
        sr_set_error("%s: k = %d and a slab of %lld subset entries need %lld bytes of workspace per query (limit %lld bytes)", who, k,
                     (long long)smallest, (long long)per_q, (long long)ws_limit);
        return SR_ERR_NOMEM;
    }
    int64_t b = nq < b_max ? nq : b_max;
    if (b < nq && b >= 16) b = b / 16 * 16;               // whole query blocks of the dense kernel
    int64_t sl = (ws_limit / b - large_bytes) / 8;
    if (sl >= 64) sl = sl / 64 * 64;                      // whole row tiles
    if (sl > (1ll << 20)) sl = 1ll << 20;
    if (const char* e = sr_dev_getenv("SR_SUBSET_MAX_SLAB")) {        // dev switch: several slabs on inputs far below any workspace limit (tests)
        const int64_t cap = atoll(e);
        if (cap >= 1 && sl > cap) sl = cap;
    }
    if (sl < smallest) sl = smallest;
    if (sl > mm) sl = mm;
    *nq_batch = b;
    *slab = sl;
    return SR_OK;
}

// ----------------------------------------------------------------------------------------------------- dense ---
// the segment row of global doc index gid, as dense_pairs_kernel finds it; false: in no segment
__device__ inline bool subset_dense_row(const PairSeg* __restrict__ segs, int n_segs, int64_t gid, int* seg, int64_t* row) {
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
            *row = r;
            return true;
        }
    }
    return false;
}

__global__ void subset_check_dense_kernel(const PairSeg* __restrict__ segs, int n_segs, const int64_t* __restrict__ subset, int64_t m,
                                          PairStatus* __restrict__ st) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const int64_t gid = subset[j];
    int seg;
    int64_t row;
    bool ok = subset_dense_row(segs, n_segs, gid, &seg, &row);
    if (j > 0 && subset[j - 1] >= gid) ok = false;
    if (!ok) atomicMin(&st->first_bad, (unsigned long long)j);
}

int launch_subset_check_dense(const PairSeg* d_segs, int n_segs, const int64_t* d_subset, int64_t m, PairStatus* d_status, hipStream_t s) {
    if (m == 0) return SR_OK;
    hipLaunchKernelGGL(subset_check_dense_kernel, dim3((unsigned)ceil_div64(m, 256)), dim3(256), 0, s, d_segs, n_segs, d_subset, m, d_status);
    SR_CHECK_LAUNCH();
    return SR_OK;
}

#define SS_QB 16        // queries per workgroup: a subset row is fetched ceil(nq / SS_QB) times
#define SS_KC 64        // columns per chunk
template <typename T>
__global__ __launch_bounds__(64) void dense_subset_kernel(DenseSubsetArgs a) {
    __shared__ float tile[64][SS_KC + 1];
    __shared__ __attribute__((aligned(16))) float qs[SS_QB][SS_KC];
    __shared__ const T* rowp[64];
    if (a.st->first_bad != ~0ull) return;                 // the check ran before this launch on the same stream
    const int lane = threadIdx.x;
    const int H = a.H;
    const int n_qblk = (a.nq + SS_QB - 1) / SS_QB;
    const int q0 = (int)(blockIdx.x % (unsigned)n_qblk) * SS_QB;      // the query blocks of one tile run side by side: its rows come from L2
    const int64_t j = (int64_t)(blockIdx.x / (unsigned)n_qblk) * 64 + lane;
    const T* row = nullptr;
    uint32_t gid = 0;
    if (j < a.n_slab) {
        const int64_t g = a.subset[j];
        int seg;
        int64_t r;
        if (subset_dense_row(a.segs, a.n_segs, g, &seg, &r)) {
            row = static_cast<const T*>(a.segs[seg].rows) + r * (int64_t)H;
            gid = (uint32_t)g;
        }
    }
    rowp[lane] = row;
    __syncthreads();
    const T* myp[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) myp[i] = rowp[i * 4 + (lane >> 4)];
    const int nch = (H + SS_KC - 1) / SS_KC;
    float acc[SS_QB];
#pragma unroll
    for (int qi = 0; qi < SS_QB; ++qi) acc[qi] = 0.f;
    auto fetch = [&](int k0, f32x4 (&v)[16], f32x4 (&qv)[SS_QB / 4]) {
        const int col = k0 + (lane & 15) * 4;             // H % 16 == 0: a 16-byte piece is inside the row or beyond it
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (myp[i] && col < H) v[i] = sr_load_row4<T>(myp[i] + col);
        }
#pragma unroll
        for (int i = 0; i < SS_QB / 4; ++i) {             // query i * 4 + (lane >> 4) of the block, the same 16-byte piece
            const int q = q0 + i * 4 + (lane >> 4);
            qv[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (q < a.nq && col < H) qv[i] = *reinterpret_cast<const f32x4*>(a.Q + (int64_t)q * H + col);
        }
    };
    auto chunk = [&](const f32x4 (&v)[16], const f32x4 (&qv)[SS_QB / 4], int k0) {
        __syncthreads();                                  // the previous chunk is consumed
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            float* t = &tile[i * 4 + (lane >> 4)][(lane & 15) * 4];
            t[0] = v[i][0]; t[1] = v[i][1]; t[2] = v[i][2]; t[3] = v[i][3];
        }
#pragma unroll
        for (int i = 0; i < SS_QB / 4; ++i) *reinterpret_cast<f32x4*>(&qs[i * 4 + (lane >> 4)][(lane & 15) * 4]) = qv[i];
        __syncthreads();
        const int ncol = H - k0 >= SS_KC ? SS_KC : H - k0;    // the last chunk of a dim that is not a multiple of 64: its columns only
        if (ncol == SS_KC) {
#pragma unroll
            for (int s8 = 0; s8 < SS_KC; s8 += 8)
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const float d0 = tile[lane][s8 + jj], d1 = tile[lane][s8 + 4 + jj];
#pragma unroll
                    for (int qi = 0; qi < SS_QB; ++qi) {
                        acc[qi] = __builtin_fmaf(qs[qi][s8 + jj], d0, acc[qi]);
                        acc[qi] = __builtin_fmaf(qs[qi][s8 + 4 + jj], d1, acc[qi]);
                    }
                }
        } else {
            for (int s8 = 0; s8 < ncol; s8 += 8)
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const float d0 = tile[lane][s8 + jj], d1 = tile[lane][s8 + 4 + jj];
#pragma unroll
                    for (int qi = 0; qi < SS_QB; ++qi) {
                        acc[qi] = __builtin_fmaf(qs[qi][s8 + jj], d0, acc[qi]);
                        acc[qi] = __builtin_fmaf(qs[qi][s8 + 4 + jj], d1, acc[qi]);
                    }
                }
        }
    };
    f32x4 va[16], vb[16], qa[SS_QB / 4], qb[SS_QB / 4];
    fetch(0, va, qa);
    for (int c = 0; c < nch; c += 2) {
        if (c + 1 < nch) fetch((c + 1) * SS_KC, vb, qb);
        chunk(va, qa, c * SS_KC);
        if (c + 1 >= nch) break;
        if (c + 2 < nch) fetch((c + 2) * SS_KC, va, qa);
        chunk(vb, qb, (c + 1) * SS_KC);
    }
    if (!row) return;
#pragma unroll
    for (int qi = 0; qi < SS_QB; ++qi) {
        const int q = q0 + qi;
        if (q < a.nq && acc[qi] >= a.tau[q]) {
            const int pos = atomicAdd(&a.cand_count[q], 1);
            if (pos < a.cand_cap) a.cand_keys[(int64_t)q * a.cand_cap + pos] = sr_make_key(acc[qi], gid);
        }
    }
}

int launch_dense_subset(const DenseSubsetArgs& a, hipStream_t s) {
    if (a.n_slab == 0 || a.nq == 0) return SR_OK;
    const int64_t blocks = ceil_div64(a.n_slab, 64) * ceil_div64(a.nq, SS_QB);
    SR_REQUIRE(blocks < (1ll << 31), "subset search: %lld workgroups in one launch", (long long)blocks);
    if (a.dtype == SR_DTYPE_F16) hipLaunchKernelGGL(dense_subset_kernel<_Float16>, dim3((unsigned)blocks), dim3(64), 0, s, a);
    else hipLaunchKernelGGL(dense_subset_kernel<float>, dim3((unsigned)blocks), dim3(64), 0, s, a);
    SR_CHECK_LAUNCH();
    return SR_OK;
}

// ---------------------------------------------------------------------------------------------------- sparse ---
__global__ void subset_check_sparse_kernel(const int64_t* __restrict__ subset, int64_t m, int64_t n_docs, PairStatus* __restrict__ st) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const int64_t d = subset[j];
    if (d < 0 || d >= n_docs || (j > 0 && subset[j - 1] >= d)) atomicMin(&st->first_bad, (unsigned long long)j);
}

struct SparseSubsetArgs {
    SparseChainIndex x;
    int64_t n_docs;
    const uint8_t* q_ascending;     // pairs route with a forward index: [nq of the call], indexed like q_indptr
    const int64_t* q_indptr; const int32_t* q_cols; const float* q_vals;      // q_indptr points at the batch's first query
    int64_t nq;                     // queries of the batch
    const int64_t* subset;          // pairs: the slab; array: the whole list
    int64_t n_sub;
    int tile_begin;                 // array: first tile of this launch
    const int32_t* skip; int skip_n;      // array: the index's skip table (sparse_index.h), skip_n + 1 entries per term
    float threshold;
    const float* tau; uint64_t* cand_keys; int* cand_count; int64_t cand_cap;
    uint32_t id_base, id_stride;
    const PairStatus* st;
};

__global__ __launch_bounds__(256) void sparse_subset_pairs_kernel(SparseSubsetArgs a) {
    if (a.st->first_bad != ~0ull) return;
    const int lane = threadIdx.x & 63;
    const int64_t total = a.nq * a.n_sub;
    const int64_t n_waves = (int64_t)gridDim.x * 4;
    for (int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); p < total; p += n_waves) {
        const int64_t j = p / a.nq, q = p - j * a.nq;     // the waves of a workgroup share a document's row
        const int64_t doc = a.subset[j];
        const int64_t tb = a.q_indptr[q], te = a.q_indptr[q + 1];
        const bool forward = a.x.fwd_indptr != nullptr && a.q_ascending[q] != 0;
        const float s = sparse_pair_chain(a.x, a.q_cols, a.q_vals, tb, te, forward, doc, lane);
        if (lane == 0 && s > a.threshold && s >= a.tau[q]) {
            const int pos = atomicAdd(&a.cand_count[q], 1);
            if (pos < a.cand_cap) a.cand_keys[q * a.cand_cap + pos] = sr_make_key(s, a.id_base + (uint32_t)doc * a.id_stride);
        }
    }
}

#define SS_TILE SR_SPARSE_TILE_DOCS      // the exact scorer's doc tiles: the index's skip table gives a term's run inside one
// first i in [lo, hi) with v[i] >= x (hi: none)
template <typename V>
__device__ inline int64_t subset_lower_bound(const V* __restrict__ v, int64_t lo, int64_t hi, int64_t x) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)v[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void sparse_subset_array_kernel(SparseSubsetArgs a) {
#pragma clang fp contract(off)
    __shared__ float sc[SS_TILE];
    __shared__ int wave_tot[4];
    __shared__ int s_base;
    if (a.st->first_bad != ~0ull) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t q = blockIdx.x;
    const int tile = a.tile_begin + (int)blockIdx.y;
    const int64_t doc0 = (int64_t)tile * SS_TILE;
    const int n_here = (int)((a.n_docs - doc0) < SS_TILE ? (a.n_docs - doc0) : SS_TILE);
    // the subset entries of this tile (the same in every thread)
    const int64_t jb = subset_lower_bound(a.subset, 0, a.n_sub, doc0);
    const int64_t je = subset_lower_bound(a.subset, jb, a.n_sub, doc0 + n_here);
    if (jb == je) return;
    for (int d = tid; d < SS_TILE; d += 256) sc[d] = 0.f;
    __syncthreads();
    // the reference's loop (scaling_retriever/indexer.py:324-340): for each query term in the query's order, scores[doc] += q_t * v
    for (int64_t i = a.q_indptr[q]; i < a.q_indptr[q + 1]; ++i) {
        const int64_t t = a.q_cols[i];
        if (t < 0 || t >= a.x.n_terms) continue;          // an unknown term is an empty posting list
        const float w = a.q_vals[i];
        const int32_t* sk = a.skip + t * (a.skip_n + 1) + (int64_t)tile * (SS_TILE / SR_SPARSE_SKIP_DOCS);
        const int64_t pb = a.x.indptr[t] + sk[0], pe = a.x.indptr[t] + sk[SS_TILE / SR_SPARSE_SKIP_DOCS];     // the term's run inside this tile
        for (int64_t p = pb + tid; p < pe; p += 256) {    // docs are unique inside one posting list
            const int d = (int)((int64_t)a.x.doc_ids[p] - doc0);
            const float prod = w * a.x.vals[p];
            sc[d] = sc[d] + prod;
        }
        __syncthreads();                                  // term-serial: the next term may touch the same docs
    }
    // gathered select: the tile's subset entries with score > threshold and score >= tau, in ascending position order
    const float tq = a.tau[q], thr = a.threshold;
    const int n_sub_here = (int)(je - jb);                // <= SS_TILE: the entries are distinct docs of the tile
    const int per_t = (n_sub_here + 255) / 256;           // thread tid owns entries [tid * per_t, + per_t)
    int cnt = 0;
    for (int e = tid * per_t; e < (tid + 1) * per_t && e < n_sub_here; ++e) {
        const int d = (int)(a.subset[jb + e] - doc0);
        const float s = sc[d];
        cnt += (s > thr && s >= tq) ? 1 : 0;
    }
    int incl = cnt;
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(incl, off);
        if (lane >= off) incl += o;
    }
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    int wbase = 0, total = 0;
    for (int w = 0; w < 4; ++w) {
        if (w < wave) wbase += wave_tot[w];
        total += wave_tot[w];
    }
    if (total == 0) return;
    if (tid == 0) s_base = atomicAdd(&a.cand_count[q], total);
    __syncthreads();
    int pos = s_base + wbase + incl - cnt;
    uint64_t* dst = a.cand_keys + q * a.cand_cap;
    for (int e = tid * per_t; e < (tid + 1) * per_t && e < n_sub_here; ++e) {
        const int64_t doc = a.subset[jb + e];
        const float s = sc[(int)(doc - doc0)];
        if (s > thr && s >= tq) {
            if (pos < a.cand_cap) dst[pos] = sr_make_key(s, a.id_base + (uint32_t)doc * a.id_stride);
            ++pos;
        }
    }
}

// Route rule.  The pair route costs one wave and a binary search per posting of every (query, subset document); the array route streams
// the postings of the query's terms once per tile whatever m is, and a streamed posting costs roughly a sixteenth of a searched one.  So
// between the two list routes the array route serves subsets of at least a sixteenth of the collection, the pair route smaller ones.
// The third route, mask, runs the certified scorer's pass over the whole collection under the filter's bitmap (sparse_cert.hip,
// cert_score_kernel<KS, true>) where sr_sparse_search would use the scorer; its cost hardly depends on m (41.5 - 71.9 ms for 6 980 queries
// at the config-3 shape).  Dev switch SR_SUBSET_SPARSE_ROUTE=pairs|array|mask forces one (tests compare the three); mask where the
// scorer does not apply is served by the list rule.
bool subset_sparse_use_array(int64_t m, int64_t n_docs) {
    if (const char* route = sr_dev_getenv("SR_SUBSET_SPARSE_ROUTE")) {
        if (strcmp(route, "array") == 0) return true;
        if (strcmp(route, "pairs") == 0) return false;
    }
    return m * 16 >= n_docs;
}
// Where the mask route takes over, as a product bound on nq x m like the dense one (dense_restrict.hip).  Measured on one MI355X at the config-3
// shape, 8.84 M documents, k = 1 000 (profiles/subset_search.json, key sparse_routes.rows): the smallest measured m at which the forced
// mask route beats both list routes, and does so at every larger measured m, is m = 10 000 for nq = 6 980 (mask 43.3 ms, pairs 55.6 ms;
// at m = 1 000 pairs wins with 7.06 against 41.5 ms) and m = 1 000 000 for nq = 64 (mask 7.72 ms, array 15.7 ms; at m = 100 000 pairs wins
// with 6.15 against 7.41 ms).  Both crossings lie at nq x m of 6.4e7 - 7.0e7; the constant is the smaller of the two products, so that the
// rule sends each measured nq to the mask route from its own crossing on.  One box, one collection size.
// sr_sparse_search_grouped compares sum_g nq_g * m_g with the same constant.  It was measured for ONE group: the group loop pays its
// per-group overhead once per group, so the real crossing moves down as groups multiply (64 queries in 8 groups of 10 %: the pass 8.5
// ms, the loop 45.0 ms at a product of 5.7e7, below the constant).  The constant stays where it is.
#define SR_SUBSET_SPARSE_MASK_CROSSOVER (64ll * 1000000ll)
// The one rule of sr_sparse_search_subset and sr_sparse_search_masked: does a call with nq queries, this k and m allowed documents take the mask route
static bool subset_sparse_use_mask(const sr_sparse_index* idx, int64_t nq, int k, int64_t m) {
    bool wants = nq * m >= SR_SUBSET_SPARSE_MASK_CROSSOVER;
    if (const char* route = sr_dev_getenv("SR_SUBSET_SPARSE_ROUTE")) {
        if (strcmp(route, "array") == 0 || strcmp(route, "pairs") == 0) wants = false;
        if (strcmp(route, "mask") == 0) wants = true;
    }
    // an empty filter has nothing to scan for; the scorer's copy of the bitmap counts against the workspace limit
    return wants && m > 0 && sparse_cert_applies(idx, k) && sparse_cert_mask_pad_bytes(idx->cert) <= idx->ws_limit;
}

int sparse_filter_need_list(sr_sparse_index* idx, SparseDocFilter* f, hipStream_t s) {
    if (f->list_ready) return SR_OK;
    SR_TRY(idx->filt_list.reserve(f->m > 0 ? f->m : 1, f->who));
    SR_TRY(launch_doc_mask_expand(f->words, idx->n_docs, idx->filt_blocks.p, idx->filt_list.p, f->m, s));
    f->list = idx->filt_list.p;
    f->list_ready = true;
    return SR_OK;
}

int sparse_subset_lists(sr_sparse_index* idx, const SparseCall& call, const int64_t* d_subset, int64_t m, bool array, hipStream_t s,
                        const char* who) {
    const int64_t nq = call.nq;
    const int k = call.k;
    int64_t nq_batch = 0, slab = 0;
    SR_TRY(subset_plan(idx->ws_limit, nq, k, m, array ? SS_TILE : 64, &nq_batch, &slab, who));
    SparseSubsetArgs a;
    a.x = SparseChainIndex{idx->indptr, idx->doc_ids, idx->vals, idx->n_terms, nullptr, nullptr};
    a.n_docs = idx->n_docs;
    a.q_ascending = nullptr;
    if (!array && m > 0) {
        // the pair route's own two ways to the postings, as in sr_sparse_score_pairs (dev switch SR_PAIR_SPARSE_ROUTE=postings)
        const char* route = sr_dev_getenv("SR_PAIR_SPARSE_ROUTE");
        if (!(route && strcmp(route, "postings") == 0)) sparse_cert_forward_index(idx->cert, &a.x.fwd_indptr, &a.x.fwd_tv);
        if (a.x.fwd_indptr) SR_TRY(sparse_pair_query_flags(idx, call.q_indptr, call.q_cols, nq, who, s));
    }
    a.q_cols = call.q_cols; a.q_vals = call.q_vals;
    a.skip = idx->skip.p; a.skip_n = idx->n_tiles * (SR_SPARSE_TILE_DOCS / SR_SPARSE_SKIP_DOCS);
    a.threshold = call.threshold;
    a.id_base = (uint32_t)call.id_base; a.id_stride = (uint32_t)call.id_stride;
    a.st = idx->pair_status;
    const int n_tiles = idx->n_tiles;
    // a launch appends at most min(m, its docs) keys per query; slab < m only with slab >= SS_TILE (subset_plan: min_slab)
    int tiles_per_launch = slab >= m || slab < SS_TILE ? n_tiles : (int)(slab / SS_TILE);
    if (tiles_per_launch > 65535) tiles_per_launch = 65535;                   // the grid's second dimension
    for (int64_t qb = 0; qb < nq; qb += nq_batch) {
        const int64_t nqb = nq - qb < nq_batch ? nq - qb : nq_batch;
        const SparseCall part = call.rows(qb, nqb);
        SR_TRY(idx->ws.ensure(nqb, k, slab));
        SR_TRY(topk_reset(idx->ws, nqb, s));
        a.q_indptr = part.q_indptr;
        a.q_ascending = a.x.fwd_indptr ? idx->pair_qflags.p + qb : nullptr;
        a.nq = nqb;
        a.tau = idx->ws.tau; a.cand_keys = idx->ws.cand_keys; a.cand_count = idx->ws.cand_count; a.cand_cap = idx->ws.cand_cap;
        if (m > 0 && array) {
            a.subset = d_subset; a.n_sub = m;
            for (int t0 = 0; t0 < n_tiles; t0 += tiles_per_launch) {
                const int nt = n_tiles - t0 < tiles_per_launch ? n_tiles - t0 : tiles_per_launch;
                a.tile_begin = t0;
                hipLaunchKernelGGL(sparse_subset_array_kernel, dim3((unsigned)nqb, (unsigned)nt), dim3(256), 0, s, a);
                SR_CHECK_LAUNCH();
                SR_TRY(topk_compact(idx->ws, nqb, k, s));
            }
        } else if (m > 0) {
            // short first slabs, doubled: until k entries were seen every one is a candidate (as the searches' first launches)
            int64_t step = ceil_div64((int64_t)k + 1024, 64) * 64;
            for (int64_t j0 = 0; j0 < m;) {
                if (step > slab) step = slab;
                const int64_t n = m - j0 < step ? m - j0 : step;
                a.subset = d_subset + j0; a.n_sub = n; a.tile_begin = 0;
                const int64_t waves = nqb * n;
                const int64_t grid = ceil_div64(waves, 4) < (int64_t)sr_cu_count() * 8 ? ceil_div64(waves, 4) : (int64_t)sr_cu_count() * 8;
                hipLaunchKernelGGL(sparse_subset_pairs_kernel, dim3((unsigned)grid), dim3(256), 0, s, a);
                SR_CHECK_LAUNCH();
                SR_TRY(topk_compact(idx->ws, nqb, k, s));
                j0 += n;
                step *= 2;
            }
        }
        SR_TRY(topk_finalize(idx->ws, nqb, k, 0.f, part.out_scores, part.out_ids, part.out_counts, s));
    }
    return SR_OK;
}

extern "C" int sr_sparse_search_subset(sr_sparse_index* idx, const int64_t* d_q_indptr, const int32_t* d_q_cols, const float* d_q_vals,
                                       int64_t nq, int k, float threshold, const int64_t* d_subset, int64_t m, int64_t id_base,
                                       int64_t id_stride, float* d_out_scores, int64_t* d_out_ids, int32_t* d_out_counts,
                                       sr_stream stream) {
    SR_TRY(sr_search_sizes("sr_sparse_search_subset", idx, nq, k, SR_MAX_TOPK_LARGE));
    SR_REQUIRE(m >= 0 && m <= idx->n_docs, "sr_sparse_search_subset: a strictly ascending subset of %lld documents holds at most that many, not m=%lld",
               (long long)idx->n_docs, (long long)m);
    SR_REQUIRE(id_stride >= 1 && id_base >= 0 && id_base + (idx->n_docs - 1) * id_stride < 0xffffffffll,
               "sr_sparse_search_subset: global doc index exceeds 32 bits");
    if (nq == 0) return SR_OK;
    SR_TRY(sr_search_pointers("sr_sparse_search_subset", d_q_indptr, d_out_scores, d_out_ids, d_subset || m == 0, false));
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(idx->mu);
    StreamOrder::Scope in_order(idx->order, s);
    const SparseCall call{d_q_indptr, d_q_cols, d_q_vals, nq, k, threshold, id_base, id_stride, d_out_scores, d_out_ids, d_out_counts};
    const bool array = subset_sparse_use_array(m, idx->n_docs);
    {   // a call that cannot run fails before any launch, whichever route serves it
        int64_t nq_batch = 0, slab = 0;
        SR_TRY(subset_plan(idx->ws_limit, nq, k, m, array ? SS_TILE : 64, &nq_batch, &slab, "sr_sparse_search_subset"));
    }
    SR_TRY(subset_status_begin(&idx->pair_status, s));
    if (m > 0) {
        hipLaunchKernelGGL(subset_check_sparse_kernel, dim3((unsigned)ceil_div64(m, 256)), dim3(256), 0, s, d_subset, m, idx->n_docs,
                           idx->pair_status);
        SR_CHECK_LAUNCH();
    }
    // The mask route reads the call's status here, not at the end: the list gets its bitmap once the check kernel has accepted it (a bad
    // list goes on to the list routes, which score nothing, write the padding rows and report it)
    if (subset_sparse_use_mask(idx, nq, k, m) && subset_status_end(idx->pair_status, d_subset, "sr_sparse_search_subset", "position", s) == SR_OK) {
        const int64_t n_words = doc_mask_words(idx->n_docs);
        SR_TRY(idx->filt_words.reserve(n_words > 0 ? n_words : 1, "sr_sparse_search_subset"));
        SR_TRY(launch_doc_mask_from_list(d_subset, m, idx->filt_words.p, idx->n_docs, idx->pair_status, nullptr, s));
        SparseDocFilter f;
        f.words = idx->filt_words.p; f.list = d_subset; f.m = m; f.list_ready = true; f.who = "sr_sparse_search_subset";
        SR_TRY(sparse_cert_mask_pad(idx, f.words, &f.mask_pad, s));
        return sparse_certified_search(idx, call, &f, s);
    }
    SR_TRY(sparse_subset_lists(idx, call, d_subset, m, array, s, "sr_sparse_search_subset"));
    return subset_status_end(idx->pair_status, d_subset, "sr_sparse_search_subset", "position", s);
}

// The same search with the filter given as a bitmap.  The count of the set bits (one 8-byte read-back) feeds the route rule; the ascending
// list is expanded only where a list route or a hand-back of the mask route needs its entries.  Every sparse position names a document,
// so a set bit below n_bits is never invalid and the list needs no check.
extern "C" int sr_sparse_search_masked(sr_sparse_index* idx, const int64_t* d_q_indptr, const int32_t* d_q_cols, const float* d_q_vals,
                                       int64_t nq, int k, float threshold, const uint32_t* d_mask_words, int64_t n_bits, int64_t id_base,
                                       int64_t id_stride, float* d_out_scores, int64_t* d_out_ids, int32_t* d_out_counts, sr_stream stream) {
    SR_TRY(sr_search_sizes("sr_sparse_search_masked", idx, nq, k, SR_MAX_TOPK_LARGE));
    SR_REQUIRE(n_bits == idx->n_docs, "sr_sparse_search_masked: the mask holds n_bits=%lld bits, the index %lld documents", (long long)n_bits,
               (long long)idx->n_docs);
    SR_REQUIRE(id_stride >= 1 && id_base >= 0 && id_base + (idx->n_docs - 1) * id_stride < 0xffffffffll,
               "sr_sparse_search_masked: global doc index exceeds 32 bits");
    if (nq == 0) return SR_OK;
    SR_TRY(sr_search_pointers("sr_sparse_search_masked", d_q_indptr, d_out_scores, d_out_ids, d_mask_words || n_bits == 0, false));
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(idx->mu);
    StreamOrder::Scope in_order(idx->order, s);
    const SparseCall call{d_q_indptr, d_q_cols, d_q_vals, nq, k, threshold, id_base, id_stride, d_out_scores, d_out_ids, d_out_counts};
    return sparse_masked_body(idx, call, d_mask_words, s, "sr_sparse_search_masked");
}

int sparse_masked_body(sr_sparse_index* idx, const SparseCall& call, const uint32_t* d_mask_words, hipStream_t s, const char* who) {
    const int64_t nq = call.nq, n_bits = idx->n_docs;
    const int k = call.k;
    SR_TRY(idx->filt_blocks.reserve(doc_mask_blocks(n_bits) + 1, who));
    SparseDocFilter f;
    f.words = d_mask_words;
    f.who = who;
    SR_TRY(doc_mask_count_sync(d_mask_words, n_bits, idx->filt_blocks.p, s, &f.m));
    const bool array = subset_sparse_use_array(f.m, idx->n_docs);
    {   // the workspace errors of sr_sparse_search_subset for a list of this length, before any scoring
        int64_t nq_batch = 0, slab = 0;
        SR_TRY(subset_plan(idx->ws_limit, nq, k, f.m, array ? SS_TILE : 64, &nq_batch, &slab, who));
    }
    SR_TRY(subset_status_begin(&idx->pair_status, s));        // the list kernels read it; nothing here can raise it
    if (subset_sparse_use_mask(idx, nq, k, f.m)) {
        SR_TRY(sparse_cert_mask_pad(idx, f.words, &f.mask_pad, s));
        return sparse_certified_search(idx, call, &f, s);
    }
    SR_TRY(sparse_filter_need_list(idx, &f, s));
    return sparse_subset_lists(idx, call, f.list, f.m, array, s, who);
}

int sparse_masked_lists(sr_sparse_index* idx, const SparseCall& call, const uint32_t* d_mask_words, int64_t m, hipStream_t s, const char* who) {
    SR_TRY(idx->filt_blocks.reserve(doc_mask_blocks(idx->n_docs) + 1, who));
    SR_TRY(idx->filt_list.reserve(m > 0 ? m : 1, who));
    SR_TRY(doc_mask_list(d_mask_words, idx->n_docs, m, idx->filt_blocks.p, idx->filt_list.p, s));
    SR_TRY(subset_status_begin(&idx->pair_status, s));
    return sparse_subset_lists(idx, call, idx->filt_list.p, m, subset_sparse_use_array(m, idx->n_docs), s, who);
}

// ---- filter groups: a document bitmap per query (sr_sparse_search_grouped) --------------------------------------------
// Route rule.  The grouped pass is the mask route with the bit read from the query's own bitmap: one pass of the certified scorer whatever
// the groups are.  The loop runs the body of sr_sparse_search_masked once per group that holds a query.  auto takes the pass where it
// applies and sum_g nq_g * m_g reaches SR_SUBSET_SPARSE_MASK_CROSSOVER - a constant that was measured for ONE group (above).  The loop's
// per-group overhead (a gather of the queries, the count's read-back, and for a group on the mask route a whole pass of its own) moves
// the real crossing down as the groups multiply; the constant is left where it is (DESIGN.md 4.20 has the measurements).  Dev switch
// SR_GROUPED_SPARSE_ROUTE=pass|loop forces one, read per call; `pass` where the pass does not apply is served by the loop.
static bool grouped_sparse_wants_pass(int64_t pairs) {
    if (const char* route = sr_dev_getenv("SR_GROUPED_SPARSE_ROUTE")) {
        if (strcmp(route, "pass") == 0) return true;
        if (strcmp(route, "loop") == 0) return false;
    }
    return pairs >= SR_SUBSET_SPARSE_MASK_CROSSOVER;
}

extern "C" int sr_sparse_search_grouped(sr_sparse_index* idx, const int64_t* d_q_indptr, const int32_t* d_q_cols, const float* d_q_vals,
                                        int64_t nq, int k, float threshold, const uint32_t* d_group_words, int64_t n_groups, int64_t n_bits,
                                        const int32_t* d_query_group, int64_t id_base, int64_t id_stride, float* d_out_scores,
                                        int64_t* d_out_ids, int32_t* d_out_counts, sr_stream stream) {
    const char* const who = "sr_sparse_search_grouped";
    SR_TRY(sr_search_sizes(who, idx, nq, k, SR_MAX_TOPK_LARGE));
    SR_TRY(sr_require_mask_bits(who, "%s: the masks hold n_bits=%lld bits each, the index %lld documents", n_bits, idx->n_docs));
    SR_TRY(sr_require_groups(who, n_groups));
    // the limit counts the bitmaps and their union in the score kernel's length: whole tiles of 1 024 documents
    SR_TRY(sr_require_group_words(who, n_groups, ceil_div64(n_bits, 1024) * 32, true));
    const int64_t n_words = doc_mask_words(n_bits);
    SR_REQUIRE(id_stride >= 1 && id_base >= 0 && id_base + (idx->n_docs - 1) * id_stride < 0xffffffffll,
               "sr_sparse_search_grouped: global doc index exceeds 32 bits");
    if (nq == 0) return SR_OK;
    SR_TRY(sr_search_pointers(who, d_q_indptr, d_out_scores, d_out_ids, d_query_group && (d_group_words || n_bits == 0), false));
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(idx->mu);
    StreamOrder::Scope in_order(idx->order, s);
    const SparseCall call{d_q_indptr, d_q_cols, d_q_vals, nq, k, threshold, id_base, id_stride, d_out_scores, d_out_ids, d_out_counts};
    // 1. the group ids: one read-back of 4 nq bytes
    std::vector<int32_t> grp;
    int64_t bad = -1;
    SR_TRY(sr_read_query_groups(d_query_group, nq, n_groups, s, &grp, &bad));
    if (bad >= 0) {
        SR_TRY(launch_pad_rows(d_out_scores, d_out_ids, d_out_counts, nq, k, 0.f, s));
        return sr_bad_group_error(who, bad, grp[(size_t)bad], n_groups, " (nothing was searched)");
    }
    // 2. set bits per group, one word-parallel pass over all bitmaps: one read-back of 8 n_groups bytes
    SR_TRY(idx->grp_counts.reserve(n_groups + 1, "sr_sparse_search_grouped"));
    SR_TRY(launch_doc_masks_check(d_group_words, n_groups, n_bits, nullptr, idx->grp_counts.p, s));
    std::vector<int64_t> counts((size_t)n_groups);
    SR_CHECK_HIP(hipMemcpyAsync(counts.data(), idx->grp_counts.p, (size_t)n_groups * 8, hipMemcpyDeviceToHost, s));
    SR_CHECK_HIP(hipStreamSynchronize(s));
    int64_t pairs = 0;
    bool any_bit = false;                                  // does a group with a query allow a document at all
    for (int64_t q = 0; q < nq; ++q) {
        pairs += counts[(size_t)grp[(size_t)q]];
        any_bit = any_bit || counts[(size_t)grp[(size_t)q]] > 0;
    }
    SparseGroups groups;
    groups.words = d_group_words; groups.n_groups = n_groups; groups.n_words = n_words;
    groups.h_group = grp.data(); groups.h_count = counts.data();
    // 3. the pass where the masked search's mask route would apply and the padded bitmaps fit the workspace limit; else the group loop
    if (grouped_sparse_wants_pass(pairs) && any_bit && sparse_cert_applies(idx, k) && sparse_cert_group_pad_bytes(idx->cert, n_groups) <= idx->ws_limit) {
        SR_TRY(sparse_cert_group_pad(idx, d_group_words, n_groups, d_query_group, nq, &groups.group_pad, &groups.union_pad, &groups.qoff, s));
        if (groups.group_pad) return sparse_certified_search(idx, call, nullptr, s, &groups);
    }
    return sparse_grouped_each(idx, call, groups, nullptr, false, s);
}
