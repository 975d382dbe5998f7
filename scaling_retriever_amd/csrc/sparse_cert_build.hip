// The certified sparse scorer's index side (gfx950): the structures built once per index - fp16 MFMA tiles of the heavy terms, packed
// postings, the per-tile run tables and the doc-major forward index - their release, and the statistics / debug hooks.  What they are
// for and the search over them: sparse_cert.hip.
#include "sparse_cert.h"
#include <algorithm>
#include <math.h>
#include <vector>

#define SC_FWD_MAX 1024               // postings per doc the forward-index sort handles

// per term: largest value; flags |= 1 for a negative or non-finite value
__global__ __launch_bounds__(256) void cert_term_stats_kernel(const int64_t* __restrict__ indptr, const float* __restrict__ vals,
                                                              float* __restrict__ vmax, int* __restrict__ flags) {
    __shared__ float red[4];
    const int64_t t = blockIdx.x;
    const int64_t b = indptr[t], e = indptr[t + 1];
    float mx = 0.f;
    int bad = 0;
    for (int64_t p = b + threadIdx.x; p < e; p += 256) {
        const float v = vals[p];
        if (!(v >= 0.f) || !(v < 3.0e38f)) bad = 1;
        mx = fmaxf(mx, v);
    }
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    if (bad) atomicOr(flags, 1);
    __syncthreads();
    if (threadIdx.x == 0) vmax[t] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

__global__ void cert_fill_d16_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ doc_ids,
                                     const float* __restrict__ vals, const int32_t* __restrict__ slot_term, int KS, float vscale,
                                     _Float16* __restrict__ d16) {
    const int sl = blockIdx.y;
    const int64_t t = slot_term[sl];
    const int64_t b = indptr[t], e = indptr[t + 1];
    const int s = sl >> 4, kk = sl & 15;
    for (int64_t p = b + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < e; p += (int64_t)gridDim.x * blockDim.x) {
        const int64_t doc = doc_ids[p];
        const int64_t tile = doc / SC_DT;
        const int dl = (int)(doc - tile * SC_DT);
        const int mb = dl >> 5, r = dl & 31;
        const int lane = r + 32 * (kk >> 3);
        d16[((((tile * SC_MB + mb) * KS + s) * 64 + lane) << 3) + (kk & 7)] = (_Float16)(vals[p] * vscale);
    }
}

__global__ void cert_pack_postings_kernel(const int32_t* __restrict__ doc_ids, const float* __restrict__ vals, int64_t nnz, float vscale,
                                          uint32_t* __restrict__ P) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nnz) return;
    const _Float16 h = (_Float16)(vals[p] * vscale);
    const uint32_t dl = (uint32_t)doc_ids[p] & (SC_DT - 1);
    P[p] = ((dl >> 1) << 2) | (dl & 1u) | ((uint32_t)__builtin_bit_cast(unsigned short, h) << 16);
}

// S[t][i] = indptr[t] + #{postings of t with doc < i * SC_DT}, i = 0 .. n_tiles.  The thread of posting p (doc d, predecessor d')
// fills the tiles in (tile(d'), tile(d)]; the thread "behind the last posting" fills the rest.
__global__ __launch_bounds__(256) void cert_s_table_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ doc_ids, int n_tiles,
                                                           uint32_t* __restrict__ S) {
    const int64_t t = blockIdx.x;
    const int64_t b = indptr[t], e = indptr[t + 1];
    uint32_t* row = S + t * (int64_t)(n_tiles + 1);
    for (int64_t p = b + threadIdx.x; p <= e; p += 256) {
        const int prev = p > b ? (int)(doc_ids[p - 1] / SC_DT) : -1;
        const int cur = p < e ? (int)(doc_ids[p] / SC_DT) : n_tiles;
        for (int i = prev + 1; i <= cur; ++i) row[i] = (uint32_t)p;
    }
}

// E[t][i] from the table of starts and the packed postings (see SparseCert::E)
__global__ __launch_bounds__(256) void cert_e_table_kernel(const uint32_t* __restrict__ S, const uint32_t* __restrict__ P, int n_tiles, int e_stride,
                                                           uint32_t* __restrict__ E) {
    const int64_t t = blockIdx.x;
    const uint32_t* srow = S + t * (int64_t)(n_tiles + 1);
    uint32_t* erow = E + t * (int64_t)e_stride;
    for (int i = threadIdx.x; i < e_stride; i += 256) {
        uint32_t e = 0u;
        if (i < n_tiles) {
            const uint32_t b = srow[i], n = srow[i + 1] - b;
            if (n == 1u) e = P[b] | 2u;
            else if (n >= 2u) e = 0xffff0000u | (n < 0xffffu ? n : 0xffffu);
        }
        erow[i] = e;
    }
}

__global__ void cert_fwd_count_kernel(const int32_t* __restrict__ doc_ids, int64_t nnz, int32_t* __restrict__ cnt) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < nnz) atomicAdd(&cnt[doc_ids[p]], 1);
}
__global__ void cert_i32_to_i64_kernel(const int32_t* __restrict__ in, int64_t n, int64_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = in[i];
}
__global__ __launch_bounds__(256) void cert_fwd_fill_kernel(const int64_t* __restrict__ indptr, const int32_t* __restrict__ doc_ids,
                                                            const float* __restrict__ vals, const int64_t* __restrict__ fwd_indptr,
                                                            int32_t* __restrict__ cursor, uint64_t* __restrict__ fwd_tv) {
    const int64_t t = blockIdx.y;
    const int64_t b = indptr[t], e = indptr[t + 1];
    for (int64_t p = b + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < e; p += (int64_t)gridDim.x * blockDim.x) {
        const int32_t d = doc_ids[p];
        const int64_t pos = fwd_indptr[d] + atomicAdd(&cursor[d], 1);
        fwd_tv[pos] = ((uint64_t)(uint32_t)t << 32) | (uint64_t)__float_as_uint(vals[p]);
    }
}
// one wave per doc: bitonic sort of its (term, value) pairs by term in LDS; flags |= 2 for a doc with more than SC_FWD_MAX postings
__global__ __launch_bounds__(256) void cert_fwd_sort_kernel(const int64_t* __restrict__ fwd_indptr, int64_t n_docs, uint64_t* __restrict__ fwd_tv,
                                                            int* __restrict__ flags) {
    __shared__ uint64_t keys_all[4][SC_FWD_MAX];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t d = (int64_t)blockIdx.x * 4 + wave;
    if (d >= n_docs) return;
    const int64_t b = fwd_indptr[d];
    const int n = (int)(fwd_indptr[d + 1] - b);
    if (n <= 1) return;
    if (n > SC_FWD_MAX) {
        if (lane == 0) atomicOr(flags, 2);
        return;
    }
    uint64_t* keys = keys_all[wave];
    int P = 64;
    while (P < n) P <<= 1;
    for (int i = lane; i < P; i += 64)
        keys[i] = i < n ? fwd_tv[b + i] : ~0ull;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    // not sr_block_sort (block_primitives.h): a wave sorts its own row, four rows per workgroup, behind a wavefront fence - no barrier
    for (int size = 2; size <= P; size <<= 1)
        for (int j = size >> 1; j > 0; j >>= 1) {
            for (int i = lane; i < P; i += 64) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const bool up = (i & size) == 0;
                    const uint64_t x = keys[i], y = keys[ixj];
                    if (up ? (x > y) : (x < y)) { keys[i] = y; keys[ixj] = x; }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        }
    for (int i = lane; i < n; i += 64) fwd_tv[b + i] = keys[i];
}

bool sparse_cert_forward_index(const SparseCert* c, const int64_t** fwd_indptr, const uint64_t** fwd_tv) {
    if (!c || !c->fwd_indptr.p || !c->fwd_tv.p) return false;
    *fwd_indptr = c->fwd_indptr.p;
    *fwd_tv = c->fwd_tv.p;
    return true;
}

// diagnostic (-DSC_STAMPS=1 builds): mean cycles per tile step of the sampled waves
static void cert_print_stamps(const unsigned long long* d_stamps) {
    unsigned long long h[80] = {0};
    if (hipMemcpy(h, d_stamps, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess || !h[0]) return;
    const double n = (double)h[0];
    fprintf(stderr, "[cert stamps] %llu sampled tile steps of %.0f cycles: last matrix wave at the barrier after %.0f, last scatter wave after %.0f (scatter last in %.0f %% of the steps); first blocks of wave 1 with a candidate: %.0f %%\n",
            h[0], (double)h[1] / n, (double)h[2] / n, (double)h[3] / n, 100.0 * (double)h[4] / n, 100.0 * (double)h[5] / n);
    fprintf(stderr, "[cert stamps]   matrix waves  : barrier arrival");
    for (int w = 0; w < 8; ++w) fprintf(stderr, " %.0f", (double)h[16 + w] / n);
    fprintf(stderr, " | end of the last MFMA chain");
    for (int w = 0; w < 8; ++w) fprintf(stderr, " %.0f", (double)h[32 + w] / n);
    fprintf(stderr, " | keys of the first block done");
    for (int w = 0; w < 8; ++w) fprintf(stderr, " %.0f", (double)h[48 + w] / n);
    fprintf(stderr, " | end of the first filter");
    for (int w = 0; w < 8; ++w) fprintf(stderr, " %.0f", (double)h[64 + w] / n);
    fprintf(stderr, "\n[cert stamps]   scatter waves : barrier arrival");
    for (int w = 8; w < 16; ++w) fprintf(stderr, " %.0f", (double)h[16 + w] / n);
    fprintf(stderr, " | end of the adds");
    for (int w = 8; w < 16; ++w) fprintf(stderr, " %.0f", (double)h[32 + w] / n);
    fprintf(stderr, "\n");
}

void sparse_cert_destroy(SparseCert* c) {
    if (!c) return;
    if (c->d_stamps.p) cert_print_stamps(c->d_stamps.p);
    c->d_stamps.release();
    c->dslot.release();
    c->vmax.release();
    c->d16.release();
    c->P.release();
    c->S.release();
    c->E.release();
    c->fwd_indptr.release();
    c->fwd_tv.release();
    c->bfrag.release();
    c->rare_term.release();
    c->rare_w.release();
    c->cq.release();
    c->sq.release();
    c->n_rare.release();
    c->n_qt.release();
    c->n_drop.release();
    c->tau2.release();
    c->elig.release();
    c->overflow.release();
    c->m_count.release();
    c->ap_ids.release();
    c->d_n_uncert.release();
    c->d_uncert.release();
    c->dump.release();
    c->mask_pad.release();
    c->group_pad.release();
    c->group_qoff.release();
    c->ws.release();
    delete c;
}

// the build's own temporaries
struct CertBuildScratch {
    DeviceBuf<int> flags;
    DeviceBuf<int32_t> terms, cnt;
    DeviceBuf<int64_t> cnt64;
    void release() { flags.release(); terms.release(); cnt.release(); cnt64.release(); }
};

// *ok = false (with SR_OK): the index does not qualify, or there is no memory for the structures - not an error
static int cert_build_structures(sr_sparse_index* idx, SparseCert* c, const std::vector<int64_t>& h_indptr, int64_t nnz, bool log,
                                 CertBuildScratch& t, bool* ok, hipStream_t s) {
    const int64_t V = idx->n_terms, N = idx->n_docs;
    *ok = false;
    if (c->vmax.reserve(V, nullptr) != SR_OK || t.flags.reserve(1, nullptr) != SR_OK) return SR_OK;
    if (hipMemsetAsync(t.flags.p, 0, sizeof(int), s) != hipSuccess) return SR_ERR_HIP;
    hipLaunchKernelGGL(cert_term_stats_kernel, dim3((unsigned)V), dim3(256), 0, s, idx->indptr, idx->vals, c->vmax.p, t.flags.p);
    std::vector<float> h_vmax((size_t)V);
    int h_flags = 0;
    if (hipMemcpyAsync(h_vmax.data(), c->vmax.p, sizeof(float) * (size_t)V, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(&h_flags, t.flags.p, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return SR_ERR_HIP;
    if (h_flags & 1) return SR_OK;                // a negative / non-finite value: exact kernels only
    float vmax_all = 0.f;
    for (float v : h_vmax) vmax_all = std::max(vmax_all, v);
    if (!(vmax_all > 0.f)) return SR_OK;
    {   // largest value lands in [2^13, 2^14): far from fp16's subnormals and from its maximum
        int ex;
        (void)frexpf(vmax_all, &ex);          // vmax_all = m * 2^ex, m in [0.5, 1)
        c->vscale = ldexpf(1.0f, 14 - ex);
    }
    // dense terms: the longest lists, those present in at least 1 / 1024 of the docs, at most T_max, a multiple of 16
    int t_max = 128;
    if (const char* e = sr_dev_getenv("SR_SPARSE_CERT_T")) t_max = atoi(e);
    t_max = std::max(16, std::min(SC_TMAX, t_max / 16 * 16));
    std::vector<std::pair<int64_t, int32_t>> heavy;
    for (int64_t tm = 0; tm < V; ++tm) {
        const int64_t len = h_indptr[(size_t)tm + 1] - h_indptr[(size_t)tm];
        if (len > 0 && len * 1024 >= N) heavy.emplace_back(-len, (int32_t)tm);
    }
    std::sort(heavy.begin(), heavy.end());
    int n_heavy = (int)std::min<size_t>(heavy.size(), (size_t)t_max);
    c->T = std::max(16, (n_heavy + 15) / 16 * 16);
    c->KS = c->T / 16;
    if (c->KS == 3) { c->KS = 4; c->T = 64; }                         // instantiated k-step counts: 1, 2, 4 .. 8
    std::vector<int32_t> h_slot((size_t)V, -1), h_terms((size_t)std::max(1, n_heavy));
    for (int i = 0; i < n_heavy; ++i) {
        h_slot[(size_t)heavy[(size_t)i].second] = i;
        h_terms[(size_t)i] = heavy[(size_t)i].second;
    }
    const size_t d16_halves = (size_t)c->n_tiles * (size_t)c->T * SC_DT;
    const size_t s_words = (size_t)V * (size_t)(c->n_tiles + 1);
    c->e_stride = (c->n_tiles + 3) / 4 * 4 + 4;
    const size_t e_words = (size_t)V * (size_t)c->e_stride;
    if (e_words >= 0xffffffffull) return SR_OK;   // the kernel addresses table E with 32-bit word offsets
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return SR_ERR_HIP;
    const size_t need = d16_halves * 2 + (size_t)nnz * 12 + (s_words + e_words) * 4 + (size_t)N * 16 + (64u << 20);
    if (need > free_b / 2) {                  // side structures may take at most half of what is free
        if (log) fprintf(stderr, "[sr_hip] sparse index: the certified scorer needs %.2f GB, more than half of the %.2f GB free: exact kernels only\n",
                         (double)need / 1e9, (double)free_b / 1e9);
        return SR_OK;
    }
    if (log) fprintf(stderr, "[sr_hip] sparse index of %lld docs, %lld postings: certified scorer with %d heavy terms, %.2f GB of side structures "
                             "(SR_SPARSE_SCORER=exact to do without)\n", (long long)N, (long long)nnz, c->T, (double)need / 1e9);
    if (c->dslot.reserve(V, nullptr) != SR_OK || c->d16.reserve((int64_t)d16_halves, nullptr) != SR_OK || c->P.reserve(nnz + 4, nullptr) != SR_OK ||
        c->S.reserve((int64_t)s_words, nullptr) != SR_OK || c->E.reserve((int64_t)e_words, nullptr) != SR_OK ||
        c->fwd_indptr.reserve(N + 1, nullptr) != SR_OK || c->fwd_tv.reserve(nnz + 2, nullptr) != SR_OK ||
        t.terms.reserve((int64_t)h_terms.size(), nullptr) != SR_OK || t.cnt.reserve(N, nullptr) != SR_OK || t.cnt64.reserve(N, nullptr) != SR_OK)
        return SR_OK;
    if (hipMemcpyAsync(c->dslot.p, h_slot.data(), sizeof(int32_t) * (size_t)V, hipMemcpyHostToDevice, s) != hipSuccess) return SR_ERR_HIP;
    if (hipMemcpyAsync(t.terms.p, h_terms.data(), sizeof(int32_t) * h_terms.size(), hipMemcpyHostToDevice, s) != hipSuccess) return SR_ERR_HIP;
    if (hipMemsetAsync(c->d16.p, 0, d16_halves * 2, s) != hipSuccess) return SR_ERR_HIP;
    if (hipMemsetAsync(t.cnt.p, 0, sizeof(int32_t) * (size_t)N, s) != hipSuccess) return SR_ERR_HIP;
    if (n_heavy > 0)
        hipLaunchKernelGGL(cert_fill_d16_kernel, dim3(256, (unsigned)n_heavy), dim3(256), 0, s, idx->indptr, idx->doc_ids, idx->vals, t.terms.p,
                           c->KS, c->vscale, c->d16.p);
    hipLaunchKernelGGL(cert_pack_postings_kernel, dim3((unsigned)ceil_div64(nnz, 256)), dim3(256), 0, s, idx->doc_ids, idx->vals, nnz,
                       c->vscale, c->P.p);
    hipLaunchKernelGGL(cert_s_table_kernel, dim3((unsigned)V), dim3(256), 0, s, idx->indptr, idx->doc_ids, c->n_tiles, c->S.p);
    if (hipMemsetAsync(c->P.p + nnz, 0, 4 * sizeof(uint32_t), s) != hipSuccess) return SR_ERR_HIP;       // an 8-byte read of the last posting stays inside
    hipLaunchKernelGGL(cert_e_table_kernel, dim3((unsigned)V), dim3(256), 0, s, c->S.p, c->P.p, c->n_tiles, c->e_stride, c->E.p);
    hipLaunchKernelGGL(cert_fwd_count_kernel, dim3((unsigned)ceil_div64(nnz, 256)), dim3(256), 0, s, idx->doc_ids, nnz, t.cnt.p);
    hipLaunchKernelGGL(cert_i32_to_i64_kernel, dim3((unsigned)ceil_div64(N, 256)), dim3(256), 0, s, t.cnt.p, N, t.cnt64.p);
    if (hipGetLastError() != hipSuccess) return SR_ERR_HIP;
    if (sr_device_exclusive_scan_i64(t.cnt64.p, c->fwd_indptr.p, N, s) != SR_OK) return SR_ERR_HIP;
    if (hipMemsetAsync(t.cnt.p, 0, sizeof(int32_t) * (size_t)N, s) != hipSuccess) return SR_ERR_HIP;
    hipLaunchKernelGGL(cert_fwd_fill_kernel, dim3(64, (unsigned)V), dim3(256), 0, s, idx->indptr, idx->doc_ids, idx->vals, c->fwd_indptr.p, t.cnt.p,
                       c->fwd_tv.p);
    hipLaunchKernelGGL(cert_fwd_sort_kernel, dim3((unsigned)ceil_div64(N, 4)), dim3(256), 0, s, c->fwd_indptr.p, N, c->fwd_tv.p, t.flags.p);
    if (hipGetLastError() != hipSuccess) return SR_ERR_HIP;
    if (hipMemcpyAsync(&h_flags, t.flags.p, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return SR_ERR_HIP;
    *ok = !(h_flags & 2);                     // a doc with more postings than the forward sort handles: exact kernels only
    return SR_OK;
}

int sparse_cert_build(sr_sparse_index* idx, hipStream_t s) {
    // dev switch SR_SPARSE_CERT: 0 = never, 1 = whenever the index qualifies structurally (tests on small indexes);
    // default: collections of at least 64 tiles
    int mode = -1;
    if (const char* e = sr_dev_getenv("SR_SPARSE_CERT")) mode = atoi(e);
    // public switches (include/sr_hip.h): SR_SPARSE_SCORER=exact keeps the index without the scorer's side structures (they take up to half
    // of the free device memory: ~22 bytes per posting + 8 bytes per (term, doc tile)); SR_LOG=1 says on stderr what was built or why not
    const char* scorer = getenv("SR_SPARSE_SCORER");
    const bool log = getenv("SR_LOG") && atoi(getenv("SR_LOG")) != 0;
    if (scorer && strcmp(scorer, "exact") == 0) mode = 0;
    if (mode == 0 || (mode < 0 && idx->n_docs < 64 * SC_DT)) {
        if (log) fprintf(stderr, "[sr_hip] sparse index of %lld docs: exact kernels only (%s)\n", (long long)idx->n_docs,
                         mode == 0 ? "certified scorer switched off" : "fewer than 65 536 docs");
        return SR_OK;
    }
    std::vector<int64_t> h_indptr((size_t)idx->n_terms + 1);
    SR_CHECK_HIP(hipMemcpyAsync(h_indptr.data(), idx->indptr, sizeof(int64_t) * h_indptr.size(), hipMemcpyDeviceToHost, s));
    SR_CHECK_HIP(hipStreamSynchronize(s));
    const int64_t nnz = h_indptr.back() - h_indptr.front();
    if (nnz <= 0 || nnz >= 0xffffffffll || h_indptr.front() != 0) return SR_OK;
    SparseCert* c = new SparseCert();
    c->nnz = nnz;
    c->n_tiles = (int)ceil_div64(idx->n_docs, SC_DT);
    CertBuildScratch scratch;
    bool ok = false;
    const int rc = cert_build_structures(idx, c, h_indptr, nnz, log, scratch, &ok, s);
    scratch.release();
    if (rc != SR_OK) {
        sr_set_error("sr_sparse_index_create: building the certified scorer's structures failed: %s", hipGetErrorString(hipGetLastError()));
        sparse_cert_destroy(c);
        return rc;
    }
    if (!ok) {
        (void)hipGetLastError();
        sparse_cert_destroy(c);
        return SR_OK;
    }
    idx->cert = c;
    return SR_OK;
}

// Which path served the searches so far.  out[0] = 1 if the certified scorer exists for this index, [1] dense terms (MFMA K),
// [2] searches it ran, [3] queries it was given, [4] queries it handed to the exact kernels (uncertified), [5] doc tiles, [6] candidates
// re-scored, [7] query batches served by the exact kernels because the scorer's per-call buffers did not fit in device memory
extern "C" int sr_sparse_index_cert_stats(sr_sparse_index* idx, int64_t* out8) {
    SR_REQUIRE(idx && out8, "sr_sparse_index_cert_stats: null argument");
    std::lock_guard<std::mutex> lock(idx->mu);
    for (int i = 0; i < 8; ++i) out8[i] = 0;
    if (SparseCert* c = idx->cert) {
        out8[0] = 1; out8[1] = c->T; out8[2] = c->n_calls; out8[3] = c->n_queries; out8[4] = c->n_uncert; out8[5] = c->n_tiles; out8[6] = c->n_rescored;
    }
    out8[7] = idx->n_cert_no_memory;
    return SR_OK;
}

// Debug / test hook: after enable = 1 every search keeps the stage-1 keys of all (query, doc) pairs; enable = 2 copies the keys of
// the last search to h_keys [nq_pad][n_tiles * 1024] (uint16) and returns the per-query constants the bound needs:
// h_consts [nq_pad][6] = {cq (0: the query is outside the fast path), s_q, rare terms in stage 1, query terms, rare terms left out, the
// k-th best key the last select of the scan saw}.  *vscale / *T: the index-side constants.
extern "C" int sr_sparse_index_cert_debug(sr_sparse_index* idx, int enable, uint16_t* h_keys, int64_t keys_capacity, float* h_consts,
                                          int64_t nq_pad, float* vscale, int32_t* T) {
    SR_REQUIRE(idx, "sr_sparse_index_cert_debug: null index");
    std::lock_guard<std::mutex> lock(idx->mu);
    SparseCert* c = idx->cert;
    SR_REQUIRE(c, "sr_sparse_index_cert_debug: this index has no certified scorer");
    if (enable != 2) {
        c->want_dump = enable != 0;
        return SR_OK;
    }
    const int64_t stride = (int64_t)c->n_tiles * SC_DT;
    SR_REQUIRE(c->dump.p && h_keys && h_consts && nq_pad * stride <= c->dump.cap, "sr_sparse_index_cert_debug: nothing recorded");
    SR_REQUIRE(keys_capacity >= nq_pad * stride, "sr_sparse_index_cert_debug: key buffer too small");
    SR_CHECK_HIP(hipDeviceSynchronize());
    SR_CHECK_HIP(hipMemcpy(h_keys, c->dump.p, sizeof(uint16_t) * (size_t)(nq_pad * stride), hipMemcpyDeviceToHost));
    std::vector<float> cqv((size_t)nq_pad), sqv((size_t)nq_pad);
    std::vector<int32_t> nr((size_t)nq_pad), nt((size_t)nq_pad), nd((size_t)nq_pad);
    SR_CHECK_HIP(hipMemcpy(cqv.data(), c->cq.p, sizeof(float) * (size_t)nq_pad, hipMemcpyDeviceToHost));
    SR_CHECK_HIP(hipMemcpy(sqv.data(), c->sq.p, sizeof(float) * (size_t)nq_pad, hipMemcpyDeviceToHost));
    SR_CHECK_HIP(hipMemcpy(nr.data(), c->n_rare.p, sizeof(int32_t) * (size_t)nq_pad, hipMemcpyDeviceToHost));
    SR_CHECK_HIP(hipMemcpy(nt.data(), c->n_qt.p, sizeof(int32_t) * (size_t)nq_pad, hipMemcpyDeviceToHost));
    SR_CHECK_HIP(hipMemcpy(nd.data(), c->n_drop.p, sizeof(int32_t) * (size_t)nq_pad, hipMemcpyDeviceToHost));
    std::vector<float> t2((size_t)nq_pad);
    SR_CHECK_HIP(hipMemcpy(t2.data(), c->tau2.p, sizeof(float) * (size_t)nq_pad, hipMemcpyDeviceToHost));
    for (int64_t q = 0; q < nq_pad; ++q) {
        h_consts[6 * q] = cqv[(size_t)q];
        h_consts[6 * q + 1] = sqv[(size_t)q];
        h_consts[6 * q + 2] = (float)nr[(size_t)q];
        h_consts[6 * q + 3] = (float)nt[(size_t)q];
        h_consts[6 * q + 4] = (float)nd[(size_t)q];
        h_consts[6 * q + 5] = t2[(size_t)q];
    }
    if (vscale) *vscale = c->vscale;
    if (T) *T = c->T;
    return SR_OK;
}

// Test-only read-out of the scorer's buffers (include/sr_hip.h): no kernel, one device-to-host copy per call.
extern "C" int sr_sparse_index_cert_readout(sr_sparse_index* idx, int what, void* h_dst, int64_t capacity_bytes, int64_t* n_bytes) {
    SR_REQUIRE(idx && n_bytes, "sr_sparse_index_cert_readout: null argument");
    std::lock_guard<std::mutex> lock(idx->mu);
    SparseCert* c = idx->cert;
    SR_REQUIRE(c, "sr_sparse_index_cert_readout: this index has no certified scorer");
    const int64_t V = idx->n_terms, N = idx->n_docs, nqp = c->last_nq_pad;
    const void* src = nullptr;
    int64_t bytes = 0;
    bool host = false;
    int64_t info[12];
    uint32_t vs_bits;
    memcpy(&vs_bits, &c->vscale, 4);
    auto plan_ok = [&](const void* p) { return p != nullptr && nqp > 0; };
    switch (what) {
        case 0:
            info[0] = c->T; info[1] = c->KS; info[2] = c->n_tiles; info[3] = c->e_stride; info[4] = V; info[5] = N; info[6] = c->nnz;
            info[7] = c->last_nq; info[8] = nqp; info[9] = c->last_k; info[10] = c->last_k_eff; info[11] = (int64_t)vs_bits;
            src = info; bytes = (int64_t)sizeof(info); host = true; break;
        case 1: src = c->dslot.p; bytes = 4 * V; break;
        case 2: src = c->vmax.p; bytes = 4 * V; break;
        case 3: src = c->d16.p; bytes = 2 * (int64_t)c->n_tiles * c->T * SC_DT; break;
        case 4: src = c->P.p; bytes = 4 * (c->nnz + 4); break;
        case 5: src = c->S.p; bytes = 4 * V * (int64_t)(c->n_tiles + 1); break;
        case 6: src = c->E.p; bytes = 4 * V * (int64_t)c->e_stride; break;
        case 7: src = c->fwd_indptr.p; bytes = 8 * (N + 1); break;
        case 8: src = c->fwd_tv.p; bytes = 8 * c->nnz; break;
        case 9: src = c->bfrag.p; bytes = 2 * nqp * c->T; break;
        case 10: src = c->rare_term.p; bytes = 4 * nqp * 256; break;
        case 11: src = c->rare_w.p; bytes = 4 * nqp * 256; break;
        case 12: src = c->elig.p; bytes = nqp; break;
        case 13: src = c->cq.p; bytes = 4 * nqp; break;
        case 14: src = c->sq.p; bytes = 4 * nqp; break;
        case 15: src = c->n_rare.p; bytes = 4 * nqp; break;
        case 16: src = c->n_qt.p; bytes = 4 * nqp; break;
        case 17: src = c->n_drop.p; bytes = 4 * nqp; break;
        case 18: src = c->m_count.p; bytes = 4 * nqp; break;
        case 19: src = c->ap_ids.p; bytes = 8 * nqp * 2 * (int64_t)c->last_k_eff; break;
        case 20: src = c->h_uncert.data(); bytes = (int64_t)c->h_uncert.size(); host = true; break;
        default: sr_set_error("sr_sparse_index_cert_readout: unknown buffer %d", what); return SR_ERR_INVALID;
    }
    if (what >= 9 && what <= 19) SR_REQUIRE(plan_ok(src), "sr_sparse_index_cert_readout: no search has run");
    if (what == 19) SR_REQUIRE(c->last_k_eff > 0, "sr_sparse_index_cert_readout: the last search ran no certificate");
    if (what == 20) SR_REQUIRE(!c->h_uncert.empty(), "sr_sparse_index_cert_readout: no flags recorded (enable sr_sparse_index_cert_debug first)");
    *n_bytes = bytes;
    if (!h_dst) return SR_OK;                                // size query
    SR_REQUIRE(capacity_bytes >= bytes, "sr_sparse_index_cert_readout: buffer too small");
    if (bytes == 0) return SR_OK;
    if (host) { memcpy(h_dst, src, (size_t)bytes); return SR_OK; }
    SR_CHECK_HIP(hipDeviceSynchronize());
    SR_CHECK_HIP(hipMemcpy(h_dst, src, (size_t)bytes, hipMemcpyDeviceToHost));
    return SR_OK;
}
