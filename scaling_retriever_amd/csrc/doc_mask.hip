// Document bitmaps (gfx950): list -> bitmap by an atomic-or scatter, bitmap -> ascending list by popcount per word, a scan and an
// ordered expand.  The reference has no counterpart (DenseFlatIndexer.search_knn, scaling_retriever/indexer.py:191-217, always ranks
// the whole index); the bitmap is the form faiss offers as IDSelectorBitmap.  sr_dense_search_masked / _subset (dense_restrict.hip) hold
// both forms of a filter: the bitmap feeds the certified filter's masked pass (dense_split_kernel.h), the list the gather kernel.
// At the end of the file: the kernels of the grouped search (sr_dense_search_grouped) - stacked bitmaps checked and counted in one pass -
// and the union of the present groups' bitmaps that the grouped range search skips tiles by (sr_dense_range_count_grouped).
#include "doc_mask.h"

#define DM_THREADS 256

__global__ __launch_bounds__(DM_THREADS) void doc_mask_scatter_kernel(const int64_t* __restrict__ list, int64_t m, uint32_t* __restrict__ words,
                                                                       int64_t n_bits, const PairStatus* __restrict__ st, int* __restrict__ bad) {
    const int64_t j = (int64_t)blockIdx.x * DM_THREADS + threadIdx.x;
    if (j >= m) return;
    if (st && st->first_bad != ~0ull) return;             // the check ran before this launch on the same stream
    const int64_t id = list[j];
    if (id < 0 || id >= n_bits) {                         // never a write outside the words
        if (bad) atomicOr(bad, 1);
        return;
    }
    atomicOr(&words[id >> 5], 1u << (unsigned)(id & 31));
}

int launch_doc_mask_from_list(const int64_t* d_list, int64_t m, uint32_t* d_words, int64_t n_bits, const PairStatus* st, int* d_bad,
                              hipStream_t s) {
    if (n_bits > 0) SR_CHECK_HIP(hipMemsetAsync(d_words, 0, (size_t)doc_mask_words(n_bits) * 4, s));
    if (m == 0) return SR_OK;
    hipLaunchKernelGGL(doc_mask_scatter_kernel, dim3((unsigned)ceil_div64(m, DM_THREADS)), dim3(DM_THREADS), 0, s, d_list, m, d_words, n_bits,
                       st, d_bad);
    SR_CHECK_LAUNCH();
    return SR_OK;
}

// word w of the bitmap with the bits at or beyond n_bits cleared; 0 beyond the last word
__device__ __forceinline__ uint32_t doc_mask_word(const uint32_t* __restrict__ words, int64_t w, int64_t n_words, int64_t n_bits) {
    if (w >= n_words) return 0u;
    uint32_t v = words[w];
    const unsigned tail = (unsigned)(n_bits & 31);
    if (w == n_words - 1 && tail != 0) v &= (1u << tail) - 1u;
    return v;
}

// inclusive scan of one int per thread over the workgroup's DM_THREADS threads; *total = the sum (the same in every thread)
__device__ __forceinline__ int doc_mask_block_scan(int v, int* wave_tot, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(incl, off);
        if (lane >= off) incl += o;
    }
    __syncthreads();                                      // wave_tot of a previous call is consumed
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    int base = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < DM_THREADS / 64; ++w) {
        if (w < wave) base += wave_tot[w];
        sum += wave_tot[w];
    }
    *total = sum;
    return incl + base;
}

__global__ __launch_bounds__(DM_THREADS) void doc_mask_count_kernel(const uint32_t* __restrict__ words, int64_t n_words, int64_t n_bits,
                                                                     int64_t* __restrict__ blocks) {
    __shared__ int wave_tot[DM_THREADS / 64];
    const int64_t w = (int64_t)blockIdx.x * DM_THREADS + threadIdx.x;
    int total;
    (void)doc_mask_block_scan(__popc(doc_mask_word(words, w, n_words, n_bits)), wave_tot, &total);
    if (threadIdx.x == 0) blocks[blockIdx.x] = total;
}

// one workgroup: blocks[b] := sum of blocks[0 .. b), *count = the sum of all
__global__ __launch_bounds__(DM_THREADS) void doc_mask_scan_kernel(int64_t* __restrict__ blocks, int64_t n_blocks, int64_t* __restrict__ count) {
    __shared__ int wave_tot[DM_THREADS / 64];
    int64_t carry = 0;
    for (int64_t b0 = 0; b0 < n_blocks; b0 += DM_THREADS) {
        const int64_t b = b0 + threadIdx.x;
        const int v = b < n_blocks ? (int)blocks[b] : 0;      // <= 8 192 each, <= 2^21 per round
        int total;
        const int incl = doc_mask_block_scan(v, wave_tot, &total);
        if (b < n_blocks) blocks[b] = carry + (incl - v);
        carry += total;
    }
    if (threadIdx.x == 0) *count = carry;
}

__global__ __launch_bounds__(DM_THREADS) void doc_mask_expand_kernel(const uint32_t* __restrict__ words, int64_t n_words, int64_t n_bits,
                                                                      const int64_t* __restrict__ blocks, int64_t* __restrict__ list,
                                                                      int64_t capacity) {
    __shared__ int wave_tot[DM_THREADS / 64];
    const int64_t w = (int64_t)blockIdx.x * DM_THREADS + threadIdx.x;
    uint32_t v = doc_mask_word(words, w, n_words, n_bits);
    const int c = __popc(v);
    int total;
    const int incl = doc_mask_block_scan(c, wave_tot, &total);
    int64_t pos = blocks[blockIdx.x] + (incl - c);
    while (v) {
        const int b = __ffs((int)v) - 1;
        if (pos < capacity) list[pos] = w * 32 + b;
        ++pos;
        v &= v - 1u;
    }
}

int launch_doc_mask_count(const uint32_t* d_words, int64_t n_bits, int64_t* d_blocks, int64_t* d_count, hipStream_t s) {
    if (n_bits == 0) {
        SR_CHECK_HIP(hipMemsetAsync(d_count, 0, sizeof(int64_t), s));
        return SR_OK;
    }
    const int64_t n_blocks = doc_mask_blocks(n_bits);
    SR_REQUIRE(n_blocks < (1ll << 31), "doc mask: %lld bits are too many for one launch", (long long)n_bits);
    hipLaunchKernelGGL(doc_mask_count_kernel, dim3((unsigned)n_blocks), dim3(DM_THREADS), 0, s, d_words, doc_mask_words(n_bits), n_bits, d_blocks);
    SR_CHECK_LAUNCH();
    hipLaunchKernelGGL(doc_mask_scan_kernel, dim3(1), dim3(DM_THREADS), 0, s, d_blocks, n_blocks, d_count);
    SR_CHECK_LAUNCH();
    return SR_OK;
}

int launch_doc_mask_expand(const uint32_t* d_words, int64_t n_bits, const int64_t* d_blocks, int64_t* d_list, int64_t capacity, hipStream_t s) {
    if (n_bits == 0 || capacity == 0) return SR_OK;
    hipLaunchKernelGGL(doc_mask_expand_kernel, dim3((unsigned)doc_mask_blocks(n_bits)), dim3(DM_THREADS), 0, s, d_words, doc_mask_words(n_bits),
                       n_bits, d_blocks, d_list, capacity);
    SR_CHECK_LAUNCH();
    return SR_OK;
}

int doc_mask_count_sync(const uint32_t* d_words, int64_t n_bits, int64_t* d_blocks, hipStream_t s, int64_t* m) {
    int64_t* d_count = d_blocks + doc_mask_blocks(n_bits);
    SR_TRY(launch_doc_mask_count(d_words, n_bits, d_blocks, d_count, s));
    SR_CHECK_HIP(hipMemcpyAsync(m, d_count, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    SR_CHECK_HIP(hipStreamSynchronize(s));
    return SR_OK;
}

int doc_mask_list(const uint32_t* d_words, int64_t n_bits, int64_t m, int64_t* d_blocks, int64_t* d_list, hipStream_t s) {
    SR_TRY(launch_doc_mask_count(d_words, n_bits, d_blocks, d_blocks + doc_mask_blocks(n_bits), s));
    return launch_doc_mask_expand(d_words, n_bits, d_blocks, d_list, m, s);
}

extern "C" int sr_doc_mask_from_list(const int64_t* d_list, int64_t m, uint32_t* d_words, int64_t n_bits, sr_stream stream) {
    SR_REQUIRE(m >= 0 && n_bits >= 0 && n_bits <= (1ll << 32), "sr_doc_mask_from_list: bad sizes m=%lld n_bits=%lld", (long long)m, (long long)n_bits);
    SR_REQUIRE((d_list || m == 0) && (d_words || n_bits == 0), "sr_doc_mask_from_list: null pointer");
    hipStream_t s = (hipStream_t)stream;
    CallBuf<int> d_bad;
    SR_TRY(d_bad.reserve(1, "sr_doc_mask_from_list"));
    SR_CHECK_HIP(hipMemsetAsync(d_bad.p, 0, sizeof(int), s));
    SR_TRY(launch_doc_mask_from_list(d_list, m, d_words, n_bits, nullptr, d_bad.p, s));
    int h_bad = 0;
    if (sr_read_back(&h_bad, d_bad.p, sizeof(int), s) != SR_OK) {
        sr_set_error("sr_doc_mask_from_list: reading the status back failed");
        return SR_ERR_HIP;
    }
    SR_REQUIRE(h_bad == 0, "sr_doc_mask_from_list: the list holds an entry outside [0, %lld) (the other entries were set)", (long long)n_bits);
    return SR_OK;
}

extern "C" int sr_doc_list_from_mask(const uint32_t* d_words, int64_t n_bits, int64_t* d_list, int64_t capacity, int64_t* d_count,
                                     sr_stream stream) {
    SR_REQUIRE(n_bits >= 0 && n_bits <= (1ll << 32) && capacity >= 0, "sr_doc_list_from_mask: bad sizes n_bits=%lld capacity=%lld",
               (long long)n_bits, (long long)capacity);
    SR_REQUIRE((d_words || n_bits == 0) && (d_list || capacity == 0) && d_count, "sr_doc_list_from_mask: null pointer");
    hipStream_t s = (hipStream_t)stream;
    CallBuf<int64_t> d_blocks;                            // the per-workgroup counts: scratch of this call
    if (n_bits > 0) SR_TRY(d_blocks.reserve(doc_mask_blocks(n_bits), "sr_doc_list_from_mask"));
    SR_TRY(launch_doc_mask_count(d_words, n_bits, d_blocks.p, d_count, s));
    SR_TRY(launch_doc_mask_expand(d_words, n_bits, d_blocks.p, d_list, capacity, s));
    if (d_blocks.p && hipStreamSynchronize(s) != hipSuccess) {
        sr_set_error("sr_doc_list_from_mask: the stream failed");
        return SR_ERR_HIP;
    }
    return SR_OK;
}

// one thread per destination word: bit i of dst = bit map[i] of src where map[i] names a source bit, else 0
__global__ __launch_bounds__(DM_THREADS) void doc_mask_remap_kernel(const uint32_t* __restrict__ src, int64_t n_src_bits,
                                                                     const int64_t* __restrict__ map, int64_t n_dst_bits,
                                                                     uint32_t* __restrict__ dst) {
    const int64_t w = (int64_t)blockIdx.x * DM_THREADS + threadIdx.x;
    if (w >= (n_dst_bits + 31) >> 5) return;
    uint32_t v = 0;
#pragma unroll 8
    for (int b = 0; b < 32; ++b) {
        const int64_t i = w * 32 + b;
        if (i >= n_dst_bits) break;
        const int64_t j = map[i];
        if (j >= 0 && j < n_src_bits) v |= ((src[j >> 5] >> (unsigned)(j & 31)) & 1u) << b;
    }
    dst[w] = v;
}

extern "C" int sr_doc_mask_remap(const uint32_t* d_src_words, int64_t n_src_bits, const int64_t* d_map, int64_t n_dst_bits,
                                 uint32_t* d_dst_words, sr_stream stream) {
    SR_REQUIRE(n_src_bits >= 0 && n_src_bits <= (1ll << 32) && n_dst_bits >= 0 && n_dst_bits <= (1ll << 32),
               "sr_doc_mask_remap: bad sizes n_src_bits=%lld n_dst_bits=%lld", (long long)n_src_bits, (long long)n_dst_bits);
    SR_REQUIRE((d_src_words || n_src_bits == 0) && ((d_map && d_dst_words) || n_dst_bits == 0), "sr_doc_mask_remap: null pointer");
    if (n_dst_bits == 0) return SR_OK;
    hipLaunchKernelGGL(doc_mask_remap_kernel, dim3((unsigned)ceil_div64(doc_mask_words(n_dst_bits), DM_THREADS)), dim3(DM_THREADS), 0,
                       (hipStream_t)stream, d_src_words, n_src_bits, d_map, n_dst_bits, d_dst_words);
    SR_CHECK_LAUNCH();
    return SR_OK;
}

// ---- filter groups (sr_dense_search_grouped) ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(DM_THREADS) void doc_mask_add_segment_kernel(uint32_t* __restrict__ valid, int64_t n_bits, int64_t n, int64_t id_base,
                                                                           int64_t id_stride) {
    for (int64_t r = (int64_t)blockIdx.x * DM_THREADS + threadIdx.x; r < n; r += (int64_t)gridDim.x * DM_THREADS) {
        const int64_t id = id_base + r * id_stride;
        if (id >= 0 && id < n_bits) atomicOr(&valid[id >> 5], 1u << (unsigned)(id & 31));     // never a write outside the words
    }
}

int launch_doc_mask_add_segment(uint32_t* d_valid, int64_t n_bits, int64_t n, int64_t id_base, int64_t id_stride, hipStream_t s) {
    if (n <= 0 || n_bits <= 0) return SR_OK;
    int64_t blocks = ceil_div64(n, DM_THREADS);
    if (blocks > (1 << 20)) blocks = 1 << 20;             // the rest by the grid stride
    hipLaunchKernelGGL(doc_mask_add_segment_kernel, dim3((unsigned)blocks), dim3(DM_THREADS), 0, s, d_valid, n_bits, n, id_base, id_stride);
    SR_CHECK_LAUNCH();
    return SR_OK;
}

// blockIdx.x: 256 words of a bitmap; blockIdx.y, strided: the groups.  counts[g] += the workgroup's set bits; counts[n_groups] = the
// smallest (g * n_words + w) * 32 + bit among the set bits that `valid` does not have
__global__ __launch_bounds__(DM_THREADS) void doc_masks_check_kernel(const uint32_t* __restrict__ words, int64_t n_groups, int64_t n_words,
                                                                      int64_t n_bits, const uint32_t* __restrict__ valid,
                                                                      unsigned long long* __restrict__ counts) {
    __shared__ int wave_tot[DM_THREADS / 64];
    const int64_t w = (int64_t)blockIdx.x * DM_THREADS + threadIdx.x;
    const uint32_t ok = (valid && w < n_words) ? valid[w] : ~0u;
    for (int64_t g = blockIdx.y; g < n_groups; g += gridDim.y) {
        const uint32_t v = doc_mask_word(words + g * n_words, w, n_words, n_bits);
        int total;
        (void)doc_mask_block_scan(__popc(v), wave_tot, &total);
        if (threadIdx.x == 0 && total) atomicAdd(&counts[g], (unsigned long long)total);
        const uint32_t off = v & ~ok;
        if (off) atomicMin(&counts[n_groups], ((unsigned long long)(g * n_words + w) << 5) + (unsigned)(__ffs((int)off) - 1));
    }
}

int launch_doc_masks_check(const uint32_t* d_group_words, int64_t n_groups, int64_t n_bits, const uint32_t* d_valid, int64_t* d_counts,
                           hipStream_t s) {
    SR_CHECK_HIP(hipMemsetAsync(d_counts, 0, (size_t)n_groups * 8, s));
    SR_CHECK_HIP(hipMemsetAsync(d_counts + n_groups, 0xff, 8, s));
    if (n_bits == 0) return SR_OK;
    const int64_t n_words = doc_mask_words(n_bits), gx = ceil_div64(n_words, DM_THREADS);
    int64_t gy = n_groups < 65535 ? n_groups : 65535;     // a launch carries fewer than 2^31 threads; the other groups by the stride
    if (gy > (1ll << 31) / (gx * DM_THREADS)) gy = (1ll << 31) / (gx * DM_THREADS);
    if (gy < 1) gy = 1;
    hipLaunchKernelGGL(doc_masks_check_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(DM_THREADS), 0, s, d_group_words, n_groups, n_words, n_bits,
                       d_valid, reinterpret_cast<unsigned long long*>(d_counts));
    SR_CHECK_LAUNCH();
    return SR_OK;
}

// one thread per word: the OR of that word over the bitmaps of the listed groups
__global__ __launch_bounds__(DM_THREADS) void doc_masks_union_kernel(const uint32_t* __restrict__ words, const int32_t* __restrict__ used,
                                                                      int64_t n_used, int64_t n_words, uint32_t* __restrict__ out) {
    const int64_t w = (int64_t)blockIdx.x * DM_THREADS + threadIdx.x;
    if (w >= n_words) return;
    uint32_t v = 0;
    for (int64_t j = 0; j < n_used; ++j) v |= words[(int64_t)used[j] * n_words + w];
    out[w] = v;
}

int launch_doc_masks_union(const uint32_t* d_group_words, const int32_t* d_used, int64_t n_used, int64_t n_bits, uint32_t* d_union,
                           hipStream_t s) {
    const int64_t n_words = doc_mask_words(n_bits);
    if (n_words == 0) return SR_OK;
    hipLaunchKernelGGL(doc_masks_union_kernel, dim3((unsigned)ceil_div64(n_words, DM_THREADS)), dim3(DM_THREADS), 0, s, d_group_words, d_used,
                       n_used, n_words, d_union);
    SR_CHECK_LAUNCH();
    return SR_OK;
}

__global__ void doc_mask_query_offsets_kernel(const int32_t* __restrict__ query_group, int64_t nq, int64_t nq_pad, uint32_t n_words,
                                              uint32_t* __restrict__ qoff) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < nq_pad) qoff[q] = q < nq ? (uint32_t)query_group[q] * n_words : 0u;
}

int launch_doc_mask_query_offsets(const int32_t* d_query_group, int64_t nq, int64_t nq_pad, int64_t n_bits, uint32_t* d_qoff, hipStream_t s) {
    if (nq_pad == 0) return SR_OK;
    hipLaunchKernelGGL(doc_mask_query_offsets_kernel, dim3((unsigned)ceil_div64(nq_pad, DM_THREADS)), dim3(DM_THREADS), 0, s, d_query_group, nq,
                       nq_pad, (uint32_t)doc_mask_words(n_bits), d_qoff);
    SR_CHECK_LAUNCH();
    return SR_OK;
}
