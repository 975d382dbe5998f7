// Hybrid fusion: the two device steps of the exact hybrid search (scaling_retriever_amd/hybrid.py) that surround the
// pair scorers.  The reference's HybridRetriever (scaling_retriever/indexer.py:859-1019) only dumps the two heads' runs; this extends it.
//   sr_hybrid_union  per query the set union of a list of dense positions (A) and a list of sparse positions mapped through s2d (B),
//                    as an ascending duplicate-free CSR with spos / tie per entry.  One workgroup per query: B (and a rectangular A) is
//                    sorted in LDS; the union is placed by ranks - an entry's output slot is its own rank plus the number of entries
//                    of the OTHER list below it (a binary search) - so a long ascending A is only ever read, never staged.
//   sr_hybrid_rank   per query the top-k of a ragged candidate list by (fused score descending, tie ascending): an 8-pass radix select
//                    of the k-th largest 64-bit key, the kept keys sorted in LDS; plus the certificate flag and the range threshold.
#include "block_primitives.h"
#include "hybrid_fuse.h"
#include "sparse_index.h"
#include <float.h>
#include <math.h>

// a[0, P) ascending with HF_EMPTY slots at its end (P a power of two, <= 16 * 256) -> a[0, n) strictly ascending, in place; returns n.
// Thread t owns slots [t * per, (t + 1) * per): it reads them (and its predecessor) before the scan's barriers and writes behind them.
__device__ inline int hf_unique(uint32_t* a, int P, int* lw) {
    const int per = P >= HF_THREADS ? P / HF_THREADS : 1;
    const int b = (int)threadIdx.x * per;
    uint32_t v[16];
    uint32_t prev = (b > 0 && b < P) ? a[b - 1] : HF_EMPTY;
    int cnt = 0;
    unsigned keep = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        v[i] = (i < per && b + i < P) ? a[b + i] : HF_EMPTY;
        if (v[i] != HF_EMPTY && v[i] != prev) {
            keep |= 1u << i;
            ++cnt;
        }
        prev = v[i];
    }
    int total;
    int at = sr_block_scan(cnt, lw, total);
#pragma unroll
    for (int i = 0; i < 16; ++i)
        if (keep & (1u << i)) a[at++] = v[i];
    __syncthreads();
    return total;
}

struct UnionArgs {
    const int64_t* a_ids; const int64_t* a_indptr; int64_t kd;          // a_indptr null: A is [nq, kd] with negative padding
    const int64_t* b_spos; const int32_t* b_counts; int64_t ks;
    const int64_t* s2d; int64_t n_s2d; const int64_t* d2s; int64_t n_d2s;
    int64_t* counts;                                                    // count kernel: [nq] union lengths
    const int64_t* out_indptr; int64_t* out_dpos; int64_t* out_spos; int64_t* out_tie; int64_t capacity;
    HybridStatus* st;
    int Pa, Pb;
};

template <bool CSR>
__device__ inline int64_t hf_a_at(const UnionArgs& a, const uint32_t* sa, int64_t a0, int64_t i) {
    return CSR ? a.a_ids[a0 + i] : (int64_t)sa[i];
}
// first i in [0, n) with A[i] >= x, else n
template <bool CSR>
__device__ inline int64_t hf_lower_bound_a(const UnionArgs& a, const uint32_t* sa, int64_t a0, int64_t n, int64_t x) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (hf_a_at<CSR>(a, sa, a0, mid) < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__device__ inline int hf_lower_bound_b(const uint32_t* sb, int n, int64_t x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((int64_t)sb[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// grid (nq, Y).  FILL = false: counts[q] = |A u B| (Y = 1).  FILL = true: the union into out_indptr[q] .., the entries of A strided over
// the Y workgroups of the query (each prepares B on its own), the B-only entries by workgroup 0.
template <bool CSR, bool FILL>
__global__ __launch_bounds__(HF_THREADS) void hybrid_union_kernel(UnionArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    uint32_t* sb = reinterpret_cast<uint32_t*>(smem_raw);       // [Pb] the dense positions of B, then sorted and unique
    int* eb = reinterpret_cast<int*>(sb + a.Pb);                // [Pb + 1] eb[j] = entries of B below j that are not in A
    uint32_t* sa = reinterpret_cast<uint32_t*>(eb + a.Pb + 1);  // [Pa] a rectangular A, sorted and unique
    __shared__ int lw[4];
    const int tid = threadIdx.x;
    const int64_t q = blockIdx.x;

    int nb_raw = a.b_counts[q];
    nb_raw = nb_raw < 0 ? 0 : (nb_raw > a.ks ? (int)a.ks : nb_raw);
    for (int i = tid; i < a.Pb; i += HF_THREADS) {
        uint32_t v = HF_EMPTY;
        if (i < nb_raw) {
            const int64_t sp = a.b_spos[q * a.ks + i];
            const int64_t d = (sp >= 0 && sp < a.n_s2d) ? a.s2d[sp] : -1;
            if (d < 0 || d >= a.n_d2s) atomicMin(&a.st->first_bad_b, (unsigned long long)(q * a.ks + i));
            else v = (uint32_t)d;
        }
        sb[i] = v;
    }
    if (!CSR)
        for (int i = tid; i < a.Pa; i += HF_THREADS) {
            uint32_t v = HF_EMPTY;
            if (i < a.kd) {
                const int64_t id = a.a_ids[q * a.kd + i];
                if (id >= a.n_d2s) atomicMin(&a.st->first_bad_a, (unsigned long long)(q * a.kd + i));
                else if (id >= 0) v = (uint32_t)id;
            }
            sa[i] = v;
        }
    __syncthreads();
    sr_block_sort<HF_THREADS, false>(sb, a.Pb);
    const int nB = hf_unique(sb, a.Pb, lw);
    int64_t a0 = 0, nA;
    if (CSR) {
        a0 = a.a_indptr[q];
        nA = a.a_indptr[q + 1] - a0;
        nA = nA < 0 ? 0 : nA;
    } else {
        sr_block_sort<HF_THREADS, false>(sa, a.Pa);
        nA = hf_unique(sa, a.Pa, lw);
    }

    // eb: exclusive prefix over B of "not in A"
    const int perB = (nB + HF_THREADS - 1) / HF_THREADS;        // <= 16
    const int b0 = tid * perB;
    unsigned only = 0;
    int cnt = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int j = b0 + i;
        if (i < perB && j < nB) {
            const int64_t x = sb[j];
            const int64_t lb = hf_lower_bound_a<CSR>(a, sa, a0, nA, x);
            if (!(lb < nA && hf_a_at<CSR>(a, sa, a0, lb) == x)) {
                only |= 1u << i;
                ++cnt;
            }
        }
    }
    int n_only;
    int at = sr_block_scan(cnt, lw, n_only);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int j = b0 + i;
        if (i < perB && j < nB) {
            eb[j] = at;
            at += (only >> i) & 1u;
        }
    }
    if (tid == 0) eb[nB] = n_only;
    __syncthreads();

    if (!FILL) {
        if (tid == 0) a.counts[q] = nA + n_only;
        return;
    }
    const int64_t o0 = a.out_indptr[q];
    int64_t o1 = a.out_indptr[q + 1];
    o1 = o1 < a.capacity ? o1 : a.capacity;                     // no store outside the query's segment or the caller's buffers
    auto put = [&](int64_t p, int64_t d) {
        if (p < o0 || p >= o1) return;
        const bool ok = d >= 0 && d < a.n_d2s;
        const int64_t sp = ok ? a.d2s[d] : -1;
        a.out_dpos[p] = d;
        a.out_spos[p] = sp;
        a.out_tie[p] = sp >= 0 ? sp : a.n_s2d + d;
    };
    for (int64_t i = (int64_t)blockIdx.y * HF_THREADS + tid; i < nA; i += (int64_t)gridDim.y * HF_THREADS) {
        const int64_t d = hf_a_at<CSR>(a, sa, a0, i);
        if (CSR && (d < 0 || d >= a.n_d2s)) atomicMin(&a.st->first_bad_a, (unsigned long long)(a0 + i));
        put(o0 + i + eb[hf_lower_bound_b(sb, nB, d)], d);
    }
    if (blockIdx.y == 0)
        for (int j = tid; j < nB; j += HF_THREADS)
            if (eb[j + 1] != eb[j]) {
                const int64_t d = sb[j];
                put(o0 + hf_lower_bound_a<CSR>(a, sa, a0, nA, d) + eb[j], d);
            }
}

template <bool CSR, bool FILL>
static int launch_union(const UnionArgs& a, int64_t nq, int ny, hipStream_t s) {
    static DeviceOnce lds_set;
    SR_TRY(sr_allow_lds(lds_set, hybrid_union_kernel<CSR, FILL>, 64 * 1024 - 64));
    const size_t lds = sizeof(uint32_t) * ((size_t)a.Pb * 2 + 1 + (CSR ? 0 : (size_t)a.Pa));     // <= 48 KB + 4
    hipLaunchKernelGGL((hybrid_union_kernel<CSR, FILL>), dim3((unsigned)nq, (unsigned)ny), dim3(HF_THREADS), lds, s, a);
    SR_CHECK_LAUNCH();
    return SR_OK;
}

extern "C" int sr_hybrid_union(const int64_t* d_a_ids, const int64_t* d_a_indptr, int64_t kd, const int64_t* d_b_spos,
                               const int32_t* d_b_counts, int64_t ks, const int64_t* d_s2d, int64_t n_s2d, const int64_t* d_d2s,
                               int64_t n_d2s, int64_t nq, int64_t* d_out_indptr, int64_t* d_out_dpos, int64_t* d_out_spos,
                               int64_t* d_out_tie, int64_t capacity, int64_t* total, sr_stream stream) {
    SR_REQUIRE(nq >= 0 && nq < (1ll << 30), "sr_hybrid_union: bad nq");
    SR_REQUIRE(d_out_indptr && total, "sr_hybrid_union: null pointer");
    SR_REQUIRE(ks >= 0 && ks <= SR_MAX_TOPK, "sr_hybrid_union: list B holds %lld entries per query, at most %d are sorted in LDS", (long long)ks, SR_MAX_TOPK);
    SR_REQUIRE(d_a_indptr || (kd >= 0 && kd <= SR_MAX_TOPK),
               "sr_hybrid_union: a rectangular list A holds %lld entries per query, at most %d are sorted in LDS (pass a longer one as an ascending CSR)",
               (long long)kd, SR_MAX_TOPK);
    SR_REQUIRE(n_s2d >= 0 && n_d2s >= 0 && n_s2d + n_d2s < (1ll << 32), "sr_hybrid_union: len(s2d) + len(d2s) = %lld does not fit the 32-bit tie",
               (long long)(n_s2d + n_d2s));
    SR_REQUIRE(capacity >= 0, "sr_hybrid_union: bad capacity");
    hipStream_t s = (hipStream_t)stream;
    *total = 0;
    if (nq == 0) {
        SR_CHECK_HIP(hipMemsetAsync(d_out_indptr, 0, sizeof(int64_t), s));
        return SR_OK;
    }
    SR_REQUIRE(d_a_ids && d_b_spos && d_b_counts && d_s2d && d_d2s && d_out_dpos && d_out_spos && d_out_tie, "sr_hybrid_union: null pointer");
    // the call's scratch: nq counts and the status words, freed when it returns (it waits for the stream to read the status)
    CallBuf<int64_t> counts;
    if (counts.reserve(nq, nullptr) != SR_OK) {
        sr_set_error("sr_hybrid_union: out of device memory for %zu scratch bytes", sizeof(int64_t) * (size_t)nq);
        return SR_ERR_NOMEM;
    }
    CallStatus<HybridStatus> st;
    SR_TRY(st.begin("sr_hybrid_union", s));
    UnionArgs a;
    a.a_ids = d_a_ids; a.a_indptr = d_a_indptr; a.kd = d_a_indptr ? 0 : kd;
    a.b_spos = d_b_spos; a.b_counts = d_b_counts; a.ks = ks;
    a.s2d = d_s2d; a.n_s2d = n_s2d; a.d2s = d_d2s; a.n_d2s = n_d2s;
    a.counts = counts.p;
    a.out_indptr = d_out_indptr; a.out_dpos = d_out_dpos; a.out_spos = d_out_spos; a.out_tie = d_out_tie; a.capacity = capacity;
    a.st = st.p;
    a.Pa = sr_pow2_at_least(a.kd, 1); a.Pb = sr_pow2_at_least(ks, 1);
    if (d_a_indptr) SR_TRY((launch_union<true, false>(a, nq, 1, s))); else SR_TRY((launch_union<false, false>(a, nq, 1, s)));
    SR_TRY(sr_device_exclusive_scan_i64(a.counts, d_out_indptr, nq, s));
    if (d_a_indptr) {
        // a long A is spread over several workgroups per query when the queries alone do not fill the device
        int64_t ny = (int64_t)sr_cu_count() * 4 / nq;
        ny = ny < 1 ? 1 : (ny > 64 ? 64 : ny);
        SR_TRY((launch_union<true, true>(a, nq, (int)ny, s)));
    } else {
        SR_TRY((launch_union<false, true>(a, nq, 1, s)));
    }
    HybridStatus h;
    int64_t n_out = 0;
    SR_CHECK_HIP(hipMemcpyAsync(&n_out, d_out_indptr + nq, sizeof(n_out), hipMemcpyDeviceToHost, s));
    SR_TRY(st.read(&h, s));                                     // waits for both copies, also when it fails
    if (h.first_bad_b != ~0ull) {
        int64_t sp = 0;
        SR_CHECK_HIP(hipMemcpy(&sp, d_b_spos + h.first_bad_b, sizeof(sp), hipMemcpyDeviceToHost));
        sr_set_error("sr_hybrid_union: sparse position %lld (query %llu, entry %llu of list B) maps to no dense document", (long long)sp,
                     h.first_bad_b / (unsigned long long)ks, h.first_bad_b % (unsigned long long)ks);
        return SR_ERR_INVALID;
    }
    if (h.first_bad_a != ~0ull) {
        int64_t id = 0;
        SR_CHECK_HIP(hipMemcpy(&id, d_a_ids + h.first_bad_a, sizeof(id), hipMemcpyDeviceToHost));
        sr_set_error("sr_hybrid_union: dense position %lld (entry %llu of list A) is outside [0, %lld)", (long long)id, h.first_bad_a, (long long)n_d2s);
        return SR_ERR_INVALID;
    }
    *total = n_out;
    SR_REQUIRE(n_out <= capacity, "sr_hybrid_union: the union holds %lld entries, the outputs %lld (indptr is complete, the lists are cut)",
               (long long)n_out, (long long)capacity);
    return SR_OK;
}

// ------------------------------------------------------------------------------------------------------ rank ---
struct RankArgs {
    const int64_t* indptr; const int64_t* dpos; const int64_t* spos; const int64_t* tie;
    const float* dense; const float* sparse;
    float w_d, w_s;
    int k, P;                       // P = next power of two >= k: the slots of the kept keys
    int n_cache;                    // keys of a list of at most this many entries are computed once and kept in LDS
    const float* D; const float* S; const uint8_t* complete;
    unsigned long long tie_limit;
    float* out_scores; int64_t* out_ids; int32_t* out_counts; int32_t* out_cert; float* out_thr;
    HybridStatus* st;
};

// fused(p): two rounded products, one rounded sum - the element-wise torch ops of rerank.fused_scores.  NOT __fmul_rn / __fadd_rn: the
// compiler's headers define them as a plain `x * y` / `x + y` compiled under the default contraction mode, so hipcc fuses them into an
// fma even inside a contract(off) scope (one rounding instead of two: 0.3 * -8.833333 + 2 * 1.5 came out as 0.35 instead of 0.3499999,
// seen in the disassembly as v_fma_f32).  Plain operators under the pragma carry no contract flag and stay three instructions.
__device__ inline float hf_fuse(float w_d, float d, float w_s, float sp) {
#pragma clang fp contract(off)
    const float a = w_d * d;
    const float b = w_s * sp;
    return a + b;
}

__device__ inline float hf_fused_at(const RankArgs& a, int64_t p) {
    const float sp = a.spos[p] >= 0 ? a.sparse[p] : 0.0f;       // no posting: no common term
    return hf_fuse(a.w_d, a.dense[p], a.w_s, sp);
}
// larger key = better: order-preserving fused bits (-0.0f ranks as +0.0f: the order is by value, ties by tie), then the smaller tie
__device__ inline uint64_t hf_key(const RankArgs& a, int64_t p) {
    const int64_t t = a.tie[p];
    if ((unsigned long long)t >= a.tie_limit) atomicMin(&a.st->first_bad_a, (unsigned long long)p);
    return ((uint64_t)sr_f2ord(hf_fused_at(a, p) + 0.0f) << 32) | (uint64_t)(~(uint32_t)t);
}

__global__ __launch_bounds__(HF_THREADS) void hybrid_rank_kernel(RankArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    uint64_t* kept = reinterpret_cast<uint64_t*>(smem_raw);             // [P] keys of the result
    uint64_t* cache = kept + a.P;                                       // [n_cache]
    uint32_t* kept_at = reinterpret_cast<uint32_t*>(cache + a.n_cache); // [P] their places in the list
    __shared__ int hist[256], scan[4], ctrl[4];
    const int tid = threadIdx.x, k = a.k;
    const int64_t q = blockIdx.x;
    const int64_t a0 = a.indptr[q];
    int64_t n = a.indptr[q + 1] - a0;
    n = n < 0 ? 0 : n;
    const bool cached = n <= a.n_cache;
    if (cached) {
        for (int i = tid; i < (int)n; i += HF_THREADS) cache[i] = hf_key(a, a0 + i);
        __syncthreads();
    }
    auto key_at = [&](int64_t i) -> uint64_t { return cached ? cache[i] : hf_key(a, a0 + i); };

    // the k-th largest key by an MSB-first radix select, 8 bits per pass (topk.hip's, over a list of any length)
    uint64_t T = 0;                 // fewer than k candidates: all are kept
    const bool have_kth = n >= k;
    if (have_kth) {
        uint64_t prefix = 0;
        int64_t remaining = k;
        for (int pass = 7; pass >= 0; --pass) {
            const int shift = pass * 8;
            hist[tid] = 0;
            __syncthreads();
            for (int64_t i = tid; i < n; i += HF_THREADS) {
                const uint64_t key = key_at(i);
                if (pass == 7 || (key >> (shift + 8)) == prefix) {
                    // the leading bytes of a query's keys are mostly one value: a wave whose keys agree adds once
                    const int bin = (int)((key >> shift) & 255);
                    const int b0 = __builtin_amdgcn_readfirstlane(bin);
                    const unsigned long long act = __ballot(1), same = __ballot(bin == b0);
                    if (same == act) {
                        if ((tid & 63) == __ffsll((long long)act) - 1) atomicAdd(&hist[b0], __popcll(act));
                    } else {
                        atomicAdd(&hist[bin], 1);
                    }
                }
            }
            __syncthreads();
            const int c = hist[tid];
            int sfx = c;                                        // suffix sums of the bins: s = sum_{b >= tid} hist[b]
            for (int off = 1; off < 64; off <<= 1) {
                const int o = __shfl_down(sfx, off);
                if ((tid & 63) + off < 64) sfx += o;
            }
            if ((tid & 63) == 0) scan[tid >> 6] = sfx;
            __syncthreads();
            for (int w = (tid >> 6) + 1; w < 4; ++w) sfx += scan[w];
            const int above = sfx - c;
            if (sfx >= remaining && above < remaining) {        // exactly one bin
                ctrl[0] = tid;
                ctrl[1] = (int)remaining - above;
            }
            __syncthreads();
            prefix = (prefix << 8) | (uint64_t)ctrl[0];
            remaining = ctrl[1];
        }
        T = prefix;
    }
    if (tid == 0) ctrl[2] = 0;
    for (int i = tid; i < a.P; i += HF_THREADS) {               // an unused slot: below every key (a key's low word is never 0)
        kept[i] = 0ull;
        kept_at[i] = 0u;
    }
    __syncthreads();
    for (int64_t i = tid; i < n; i += HF_THREADS) {
        const uint64_t key = key_at(i);
        if (key >= T) {
            const int slot = atomicAdd(&ctrl[2], 1);
            if (slot < a.P) {                                   // keys are unique (ties are): exactly min(n, k) of them
                kept[slot] = key;
                kept_at[slot] = (uint32_t)i;
            }
        }
    }
    __syncthreads();
    int m = ctrl[2];
    m = m < k ? m : k;
    const int P = sr_pow2_at_least(m, 2);                       // m <= k: inside the a.P slots
    sr_block_sort_kv<HF_THREADS, true>(kept, kept_at, P);       // descending, the places carried along
    for (int i = tid; i < k; i += HF_THREADS) {
        const int64_t o = q * k + i;
        if (i < m) {
            a.out_scores[o] = hf_fused_at(a, a0 + kept_at[i]);  // the fused bits themselves (the key holds a -0.0f as +0.0f)
            a.out_ids[o] = a.dpos[a0 + kept_at[i]];
        } else {
            a.out_scores[o] = -FLT_MAX;
            a.out_ids[o] = -1;
        }
    }
    if (tid != 0) return;
    a.out_counts[q] = m;
    // the certificate and the range threshold: every document outside both lists has fused <= B
    const float w_d = a.w_d, w_s = a.w_s, S = a.S[q];
    const float Fk = have_kth ? sr_key_score(T) : -INFINITY;
    const float B = hf_fuse(w_d, a.D[q], w_s, S);
    a.out_cert[q] = (a.complete[q] != 0 || (have_kth && Fk > B)) ? 1 : 0;
    // pred(d*), d* the smallest float with g(d*) = fused(d*, S) >= Fk; g is monotone: bisection over the ordered image of the floats
    float thr;
    if (!have_kth || hf_fuse(w_d, -FLT_MAX, w_s, S) >= Fk) {
        thr = -INFINITY;
    } else if (!(hf_fuse(w_d, INFINITY, w_s, S) >= Fk)) {
        thr = INFINITY;                                         // no dense score reaches Fk with this S (never an uncertified query)
    } else {
        uint32_t lo = sr_f2ord(-FLT_MAX), hi = sr_f2ord(INFINITY);
        while (hi - lo > 1) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (hf_fuse(w_d, sr_ord2f(mid), w_s, S) >= Fk) hi = mid; else lo = mid;
        }
        thr = sr_ord2f(lo);
    }
    a.out_thr[q] = thr;
}

extern "C" int sr_hybrid_rank(const int64_t* d_cand_indptr, const int64_t* d_dpos, const int64_t* d_spos, const int64_t* d_tie,
                              const float* d_dense_scores, const float* d_sparse_scores, int64_t nq, float w_d, float w_s, int k,
                              const float* d_D, const float* d_S, const uint8_t* d_complete, int64_t n_s2d, int64_t id_end,
                              float* d_out_scores, int64_t* d_out_ids, int32_t* d_out_counts, int32_t* d_out_certified,
                              float* d_out_threshold, sr_stream stream) {
    SR_REQUIRE(nq >= 0 && nq < (1ll << 30), "sr_hybrid_rank: bad nq");
    SR_REQUIRE(k >= 1, "sr_hybrid_rank: bad k = %d", k);
    if (k > SR_MAX_TOPK) {
        sr_set_error("sr_hybrid_rank: k = %d, at most %d are selected and sorted in LDS", k, SR_MAX_TOPK);
        return SR_ERR_UNSUPPORTED;
    }
    SR_REQUIRE(w_d >= 0.f && w_s >= 0.f && w_d < INFINITY && w_s < INFINITY, "sr_hybrid_rank: the weights must be finite and >= 0");
    SR_REQUIRE(n_s2d >= 0 && id_end >= 0 && n_s2d + id_end < (1ll << 32),
               "sr_hybrid_rank: len(s2d) + id_end = %lld does not fit the 32-bit tie of the key", (long long)(n_s2d + id_end));
    if (nq == 0) return SR_OK;
    SR_REQUIRE(d_cand_indptr && d_dpos && d_spos && d_tie && d_dense_scores && d_sparse_scores && d_D && d_S && d_complete && d_out_scores &&
               d_out_ids && d_out_counts && d_out_certified && d_out_threshold, "sr_hybrid_rank: null pointer");
    hipStream_t s = (hipStream_t)stream;
    CallStatus<HybridStatus> st;
    SR_TRY(st.begin("sr_hybrid_rank", s));
    RankArgs a;
    a.indptr = d_cand_indptr; a.dpos = d_dpos; a.spos = d_spos; a.tie = d_tie; a.dense = d_dense_scores; a.sparse = d_sparse_scores;
    a.w_d = w_d; a.w_s = w_s; a.k = k; a.P = sr_pow2_at_least(k, 2);
    // 12 bytes per kept slot; the key cache takes what is left of 32 KB (3 - 4 workgroups per compute unit), nothing for a large k
    const size_t kept_bytes = (size_t)a.P * 12;
    a.n_cache = kept_bytes < 32 * 1024 ? (int)((32 * 1024 - kept_bytes) / 8) : 0;
    a.D = d_D; a.S = d_S; a.complete = d_complete; a.tie_limit = (unsigned long long)(n_s2d + id_end);
    a.out_scores = d_out_scores; a.out_ids = d_out_ids; a.out_counts = d_out_counts; a.out_cert = d_out_certified; a.out_thr = d_out_threshold;
    a.st = st.p;
    static DeviceOnce lds_set;
    SR_TRY(sr_allow_lds(lds_set, hybrid_rank_kernel, 60 * 1024));
    hipLaunchKernelGGL(hybrid_rank_kernel, dim3((unsigned)nq), dim3(HF_THREADS), kept_bytes + (size_t)a.n_cache * 8, s, a);
    SR_CHECK_LAUNCH();
    HybridStatus h;
    SR_TRY(st.read(&h, s));
    if (h.first_bad_a != ~0ull) {
        int64_t t = 0;
        SR_CHECK_HIP(hipMemcpy(&t, d_tie + h.first_bad_a, sizeof(t), hipMemcpyDeviceToHost));
        sr_set_error("sr_hybrid_rank: tie %lld (candidate %llu) is outside [0, %lld)", (long long)t, h.first_bad_a, (long long)(n_s2d + id_end));
        return SR_ERR_INVALID;
    }
    return SR_OK;
}
