// Collapsed search (scaling_retriever_amd/collapse.py): the device step that turns a ranked row into its
// first-occurrence-per-group row ("MaxP", field collapsing) and says whether that row is provably the top-k groups of the full ranking.
// No reference counterpart: the reference ranks passages only.
//   sr_topk_collapse  one 256-thread workgroup per query streams its row in chunks of TC_CHUNK ranks.  The group keys met so far sit in
//                     an LDS hash table (open addressing, linear probing) of (key, first position) slots: every entry of a chunk claims
//                     or finds its key's slot (an LDS compare-and-swap) and lowers the slot's position to its own (an LDS minimum), so
//                     after one barrier an entry is a first occurrence iff the slot holds its own position.  Positions only grow along
//                     the row, hence a key accepted in chunk 0 suppresses its reappearance in chunk 2 with no reset in between, and the
//                     minimum makes the outcome independent of the order in which lanes arrive: the outputs are the same bytes on every
//                     run.  First occurrences are appended in rank order behind a block scan; the loop ends at k groups or at the row's
//                     end.  No sort: a chunk costs O(TC_CHUNK) LDS operations and five barriers.
#include "block_primitives.h"
#include <float.h>
#include <limits.h>

#define TC_THREADS 256                      // the four waves of sr_block_scan
#define TC_CHUNK 1024                       // ranks per chunk
#define TC_PER (TC_CHUNK / TC_THREADS)      // consecutive ranks per thread: the block scan then appends in rank order
#define TC_NONE INT_MAX

struct CollapseArgs {
    const float* scores; const int64_t* ids; const int32_t* counts; int64_t row_len; int exhaustive;
    const int32_t* keys; int64_t n_keys; int k;
    int slots;                              // of the hash table: >= 1.5 (k + TC_CHUNK), so it is never more than 2/3 full
    float* out_scores; int64_t* out_ids; int32_t* out_keys; int32_t* out_counts; int32_t* out_complete;
    int32_t* status;                        // [nq] the first position of the row whose id or key is invalid, -1: none
};

// slots in [0, slots): the high word of a multiplicative hash scaled to the table (slots need not be a power of two)
__device__ inline int tc_home(int32_t key, int slots) {
    return (int)(((uint64_t)((uint32_t)key * 2654435761u) * (uint64_t)(uint32_t)slots) >> 32);
}

__global__ __launch_bounds__(TC_THREADS) void topk_collapse_kernel(CollapseArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    int32_t* tkey = reinterpret_cast<int32_t*>(smem_raw);       // [slots] the key of a slot, -1: free
    int32_t* tpos = tkey + a.slots;                             // [slots] the smallest position of the row that holds it
    __shared__ int lw[4], ctrl[2];                              // ctrl: the first negative id (no counts), the first invalid entry
    const int tid = threadIdx.x, k = a.k;
    const int64_t q = blockIdx.x;
    const float* scores = a.scores + q * a.row_len;
    const int64_t* ids = a.ids + q * a.row_len;
    int64_t end = a.row_len;                                    // the valid prefix as far as it is known
    if (a.counts) {
        const int64_t c = a.counts[q];
        end = c < 0 ? 0 : (c < end ? c : end);
    }
    for (int i = tid; i < a.slots; i += TC_THREADS) {
        tkey[i] = -1;
        tpos[i] = TC_NONE;
    }
    if (tid < 2) ctrl[tid] = TC_NONE;
    __syncthreads();

    int n_out = 0;
    bool bad = false;
    for (int64_t base = 0; base < end && n_out < k; base += TC_CHUNK) {
        const int64_t p0 = base + (int64_t)tid * TC_PER;
        int64_t id[TC_PER];
#pragma unroll
        for (int j = 0; j < TC_PER; ++j) {
            id[j] = p0 + j < end ? ids[p0 + j] : 0;
            if (!a.counts && id[j] < 0) atomicMin(&ctrl[0], (int)(p0 + j));
        }
        if (!a.counts) {                                        // the dense searches' padding ends the row
            __syncthreads();
            const int64_t neg = ctrl[0];
            end = neg < end ? neg : end;
        }
        int slot[TC_PER];
        int32_t key[TC_PER];
#pragma unroll
        for (int j = 0; j < TC_PER; ++j) {
            slot[j] = -1;
            key[j] = -1;
            if (p0 + j < end) {
                const int64_t d = id[j];
                const int32_t g = (d >= 0 && d < a.n_keys) ? a.keys[d] : -1;
                if (g < 0) {
                    atomicMin(&ctrl[1], (int)(p0 + j));
                } else {
                    int s = tc_home(g, a.slots);
                    for (;;) {                                  // ends: the table always has a free slot
                        const int32_t cur = atomicCAS(&tkey[s], -1, g);
                        if (cur == -1 || cur == g) break;
                        s = s + 1 == a.slots ? 0 : s + 1;
                    }
                    atomicMin(&tpos[s], (int)(p0 + j));
                    slot[j] = s;
                    key[j] = g;
                }
            }
        }
        __syncthreads();
        if (ctrl[1] != TC_NONE) {                               // the same for every thread
            bad = true;
            break;
        }
        unsigned keep = 0;
        int cnt = 0;
#pragma unroll
        for (int j = 0; j < TC_PER; ++j)
            if (slot[j] >= 0 && tpos[slot[j]] == (int)(p0 + j)) {
                keep |= 1u << j;
                ++cnt;
            }
        int total;
        int at = n_out + sr_block_scan(cnt, lw, total);
#pragma unroll
        for (int j = 0; j < TC_PER; ++j)
            if (keep & (1u << j)) {
                if (at < k) {
                    const int64_t o = q * k + at;
                    a.out_scores[o] = scores[p0 + j];
                    a.out_ids[o] = id[j];
                    a.out_keys[o] = key[j];
                }
                ++at;
            }
        n_out = total >= k - n_out ? k : n_out + total;
    }
    if (bad) {
        if (tid == 0) a.status[q] = ctrl[1];
        return;
    }
    for (int i = n_out + tid; i < k; i += TC_THREADS) {
        const int64_t o = q * k + i;
        a.out_scores[o] = -FLT_MAX;
        a.out_ids[o] = -1;
        a.out_keys[o] = -1;
    }
    if (tid == 0) {
        a.out_counts[q] = n_out;
        a.out_complete[q] = (n_out == k || end < a.row_len || a.exhaustive) ? 1 : 0;
        a.status[q] = -1;
    }
}

// out[0] = the first query whose status is set, out[1] = its status; -1, -1: none.  One workgroup.
__global__ __launch_bounds__(TC_THREADS) void collapse_status_kernel(const int32_t* status, int64_t nq, long long* out) {
    __shared__ unsigned long long first;
    if (threadIdx.x == 0) first = ~0ull;
    __syncthreads();
    for (int64_t q = threadIdx.x; q < nq; q += TC_THREADS)
        if (status[q] >= 0) {
            atomicMin(&first, (unsigned long long)q);
            break;
        }
    __syncthreads();
    if (threadIdx.x == 0) {
        out[0] = first == ~0ull ? -1 : (long long)first;
        out[1] = first == ~0ull ? -1 : (long long)status[first];
    }
}

extern "C" int sr_topk_collapse(const float* d_scores, const int64_t* d_ids, const int32_t* d_counts, int64_t nq, int64_t row_len,
                                int exhaustive, const int32_t* d_keys, int64_t n_keys, int k, float* d_out_scores, int64_t* d_out_ids,
                                int32_t* d_out_keys, int32_t* d_out_counts, int32_t* d_out_complete, sr_stream stream) {
    SR_REQUIRE(nq >= 0 && nq < (1ll << 30), "sr_topk_collapse: bad nq");
    SR_REQUIRE(row_len >= 0 && row_len < (1ll << 31), "sr_topk_collapse: row_len = %lld is outside [0, 2^31)", (long long)row_len);
    SR_REQUIRE(n_keys >= 0, "sr_topk_collapse: bad n_keys");
    SR_REQUIRE(k >= 1, "sr_topk_collapse: bad k = %d", k);
    if (k > SR_MAX_TOPK) {
        sr_set_error("sr_topk_collapse: k = %d, at most %d groups are kept in LDS", k, SR_MAX_TOPK);
        return SR_ERR_UNSUPPORTED;
    }
    SR_REQUIRE(d_scores && d_ids && d_keys && d_out_scores && d_out_ids && d_out_keys && d_out_counts && d_out_complete,
               "sr_topk_collapse: null pointer");
    if (nq == 0) return SR_OK;
    hipStream_t s = (hipStream_t)stream;
    // the call's scratch: a status word per query and the two words read back, freed when it returns
    const size_t status_bytes = (sizeof(int32_t) * (size_t)nq + 7) & ~(size_t)7;
    CallBuf<unsigned char> scratch;
    if (scratch.reserve((int64_t)(status_bytes + 2 * sizeof(long long)), nullptr) != SR_OK) {
        sr_set_error("sr_topk_collapse: out of device memory for %zu scratch bytes", status_bytes + 2 * sizeof(long long));
        return SR_ERR_NOMEM;
    }
    CollapseArgs a;
    a.scores = d_scores; a.ids = d_ids; a.counts = d_counts; a.row_len = row_len; a.exhaustive = exhaustive;
    a.keys = d_keys; a.n_keys = n_keys; a.k = k;
    a.slots = ((k + TC_CHUNK) * 3 / 2 + 255) / 256 * 256;      // <= 7680: 60 KB at k = 4096, 24 KB at k = 1000
    a.out_scores = d_out_scores; a.out_ids = d_out_ids; a.out_keys = d_out_keys; a.out_counts = d_out_counts; a.out_complete = d_out_complete;
    a.status = reinterpret_cast<int32_t*>(scratch.p);
    long long* d_first = reinterpret_cast<long long*>(scratch.p + status_bytes);
    static DeviceOnce lds_set;
    SR_TRY(sr_allow_lds(lds_set, topk_collapse_kernel, 64 * 1024 - 64));
    hipLaunchKernelGGL(topk_collapse_kernel, dim3((unsigned)nq), dim3(TC_THREADS), sizeof(int32_t) * 2 * (size_t)a.slots, s, a);
    SR_CHECK_LAUNCH();
    hipLaunchKernelGGL(collapse_status_kernel, dim3(1), dim3(TC_THREADS), 0, s, a.status, nq, d_first);
    SR_CHECK_LAUNCH();
    long long h[2] = {-1, -1};
    SR_TRY(sr_read_back(h, d_first, sizeof(h), s));
    if (h[0] >= 0) {
        long long id = 0;
        SR_CHECK_HIP(hipMemcpy(&id, d_ids + h[0] * row_len + h[1], sizeof(id), hipMemcpyDeviceToHost));
        if (id < 0 || id >= n_keys) {
            sr_set_error("sr_topk_collapse: query %lld, position %lld: id %lld is outside the key table [0, %lld)", h[0], h[1], id, (long long)n_keys);
        } else {
            int32_t g = 0;
            SR_CHECK_HIP(hipMemcpy(&g, d_keys + id, sizeof(g), hipMemcpyDeviceToHost));
            sr_set_error("sr_topk_collapse: query %lld, position %lld: id %lld has the negative group key %d", h[0], h[1], id, (int)g);
        }
        return SR_ERR_INVALID;
    }
    return SR_OK;
}
