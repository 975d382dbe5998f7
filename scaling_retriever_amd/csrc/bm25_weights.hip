// sr_bm25_weights: the term frequencies of a term-major CSR -> BM25 weights.  Contract: include/sr_hip.h, "lexical"; DESIGN.md 4.29.
//
// One thread per posting, a wave's 64 postings contiguous, so the three posting streams (document ids and frequencies in, weights out:
// 12 bytes per posting) move in full-width accesses; the document length is the one gathered read.  The posting's term is not stored.
// A wave owns one contiguous run of postings and walks it 64 at a time: it searches d_indptr once for the term of its first posting
// (17 dependent reads at 128 K terms, wave-uniform) and carries the term from piece to piece - inside a posting list longer than a wave,
// which is where nearly all postings of a collection are, a piece costs one read of d_indptr; a piece that crosses a list boundary
// searches above the carried term, and only then does a lane search between the piece's first and last term.  (A search per 64
// postings would be 34 dependent reads a piece; a rough estimate put that at several times the time of the streams, so it was not
// built and not measured.)  The scalars and the idf table come from the host; the kernel runs no logarithm.
#include "common.h"

#define BW_THREADS 256
#define BW_BLOCKS_PER_CU 8              // grid cap: above it a wave's run of postings is longer than one piece of 64

struct BwArgs {
    const int64_t* indptr; const int32_t* doc_ids; const float* tf;
    int64_t n_terms, nnz;
    int64_t per;                        // postings of one wave's run: a multiple of 64
    const int32_t* doc_len; int64_t n_docs;
    const float* idf;
    float numer, a, s;
    float* out;
    unsigned long long* first_bad;      // smallest posting whose document id is outside [0, n_docs)
};

// the term t in [lo, hi] with indptr[t] <= p < indptr[t + 1], given indptr[lo] <= p < indptr[hi + 1]
__device__ inline int64_t bw_term(const int64_t* __restrict__ indptr, int64_t lo, int64_t hi, int64_t p) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo + 1) >> 1);
        if (indptr[mid] <= p) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(BW_THREADS) void bm25_weights_kernel(BwArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    // wave-uniform from here to `p`: the wave's run of postings [r0, r1), a multiple of 64 long
    const int64_t wave = (int64_t)blockIdx.x * (BW_THREADS / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t r0 = wave * a.per, r1 = r0 + a.per < a.nnz ? r0 + a.per : a.nnz;
    if (r0 >= r1) return;
    int64_t t_lo = bw_term(a.indptr, 0, a.n_terms - 1, r0);               // once per wave; carried from piece to piece below
    for (int64_t w0 = r0; w0 < r1; w0 += 64) {
        const int64_t w1 = w0 + 63 < r1 ? w0 + 63 : r1 - 1;
        // the term of the piece's last posting: t_lo itself inside a long list (one read), else a search above t_lo
        const int64_t t_hi = a.indptr[t_lo + 1] > w1 ? t_lo : bw_term(a.indptr, t_lo, a.n_terms - 1, w1);
        const int64_t first = t_lo;
        t_lo = t_hi;                                                        // indptr[t_hi] <= w1 < the next piece's postings
        const int64_t p = w0 + lane;
        if (p > w1) continue;
        const int64_t t = first == t_hi ? first : bw_term(a.indptr, first, t_hi, p);
        const int32_t d = a.doc_ids[p];
        const float tf = a.tf[p];
        if (d < 0 || d >= a.n_docs) {
            atomicMin(a.first_bad, (unsigned long long)p);
            continue;
        }
        const float dl = (float)a.doc_len[d];
        const float sl = a.s * dl;
        const float K = a.a + sl;
        const float num = tf * a.numer;
        const float den = tf + K;
        const float q = num / den;
        a.out[p] = a.idf[t] * q;
    }
}

extern "C" int sr_bm25_weights(const int64_t* d_indptr, const int32_t* d_doc_ids, const float* d_tf, int64_t n_terms, int64_t nnz,
                               const int32_t* d_doc_len, int64_t n_docs, const float* d_idf, float numer, float a, float s, float* d_out_vals,
                               sr_stream stream) {
    SR_REQUIRE(n_terms >= 0 && nnz >= 0 && n_docs >= 0 && n_terms < (1ll << 31) && n_docs < (1ll << 31),
               "sr_bm25_weights: bad sizes (n_terms %lld, nnz %lld, n_docs %lld)", (long long)n_terms, (long long)nnz, (long long)n_docs);
    SR_REQUIRE(nnz == 0 || (n_terms >= 1 && d_indptr && d_doc_ids && d_tf && d_doc_len && d_idf && d_out_vals), "sr_bm25_weights: null pointer");
    if (nnz == 0) return SR_OK;
    hipStream_t st = (hipStream_t)stream;
    CallStatus<unsigned long long> status;
    SR_TRY(status.begin("sr_bm25_weights", st));
    BwArgs k;
    k.indptr = d_indptr; k.doc_ids = d_doc_ids; k.tf = d_tf; k.n_terms = n_terms; k.nnz = nnz; k.doc_len = d_doc_len; k.n_docs = n_docs;
    k.idf = d_idf; k.numer = numer; k.a = a; k.s = s; k.out = d_out_vals; k.first_bad = status.p;
    const int64_t cap = (int64_t)sr_cu_count() * BW_BLOCKS_PER_CU;
    const int64_t need = ceil_div64(nnz, BW_THREADS);
    const int64_t grid = need < cap ? need : cap;
    k.per = ceil_div64(ceil_div64(nnz, 64), grid * (BW_THREADS / 64)) * 64;
    hipLaunchKernelGGL(bm25_weights_kernel, dim3((unsigned)grid), dim3(BW_THREADS), 0, st, k);
    SR_CHECK_LAUNCH();
    unsigned long long first_bad = ~0ull;
    SR_TRY(status.read(&first_bad, st));
    if (first_bad != ~0ull) {
        int32_t d = 0;
        SR_CHECK_HIP(hipMemcpy(&d, d_doc_ids + first_bad, sizeof(d), hipMemcpyDeviceToHost));
        sr_set_error("sr_bm25_weights: document id %d (posting %llu) is outside [0, %lld) (the outputs are not to be used)", (int)d, first_bad,
                     (long long)n_docs);
        return SR_ERR_INVALID;
    }
    return SR_OK;
}
