// Top-k in global memory for k > SR_MAX_TOPK (gfx950): the same TopkWS protocol as topk.hip, without an LDS array sized by k.
//
// The score kernels append survivors (keys >= tau) to the candidate buffer exactly as for a small k.  topk_compact2 with
// k > SR_MAX_TOPK then runs, per query, either an append (the set stays a superset of the top-k while its 2k slots hold
// everything) or a radix select of the k-th largest key of run set + candidates:
//   plan    one thread per query: append, select or nothing; resets the per-query select state
//   append  (query, slice) workgroups copy the candidates behind the running set (and find the smallest key when n == k)
//   hist/pick, per 8-bit digit from the top: (query, slice) workgroups count the keys that match the digits chosen so far in LDS
//           and add the counts to the query's 256 global bins; one workgroup per query then picks the digit of the k-th key.
//           The four score digits always run (tau = the exact score of the k-th key, as the LDS select sets it); the four
//           index digits only for queries whose boundary score still holds more keys than the rank left to place
//   holes   slots of run[0, k) that are empty or hold a key below the k-th key T are listed (global, k words per query)
//   fill    the kept keys of run[k, nr) and of the candidates move into the listed slots
//   finish  run_count = k, tau = score(T), cand_count = 0
// Keys are unique, so the kept set (and everything downstream) does not depend on the order the atomic appends left it in.
// topk_finalize cuts the set to k the same way, sorts run[0, next_pow2(k)) descending in place (bitonic: 4096-key tiles in LDS,
// the wider merge steps in global memory; the slots past the kept keys hold zeros, which sort last) and writes [nq, k] outputs.
// A query's keys are spread over several workgroups (slices) when the launch has few queries: one query with k close to N
// still fills the chip.  No kernel here uses scratch (tests/test_large_k_gpu.py reads the code object's metadata).
#include "common.h"

struct TopkLargeState {
    uint64_t prefix;               // digits chosen so far; the k-th key T once mode == 3
    uint64_t minkey;               // append with n == k: smallest key of the set (atomicMin)
    int64_t remaining;             // rank of the k-th key inside the keys that match prefix
    int64_t nr, nc;                // running set / candidates at the start of this compaction
    unsigned long long n_holes;    // listed holes, then placed fillers
    unsigned long long n_filled;
    int mode;                      // 0 nothing to do, 1 append, 2 select running, 3 select done (prefix = T)
    int pad_;
};

#define TL_THREADS 256
#define TL_UNROLL 4                // independent key loads in flight per thread
#define TL_TILE 4096               // keys per LDS tile of the sort (32 KB)

int64_t topk_large_bytes_per_query(int k) {
    return 2 * (int64_t)k * 8 + (int64_t)k * 4 + 256 * 8 + (int64_t)sizeof(TopkLargeState) + 16;
}

// ------------------------------------------------------------- workspace ---
int topk_large_alloc(TopkWS& ws, int64_t nq, int k) {
    if (hipMalloc(&ws.l_holes, sizeof(uint32_t) * (size_t)nq * (size_t)k) != hipSuccess ||
        hipMalloc(&ws.l_hist, sizeof(unsigned long long) * 256 * (size_t)nq) != hipSuccess ||
        hipMalloc(&ws.l_state, sizeof(TopkLargeState) * (size_t)nq) != hipSuccess) {
        (void)hipGetLastError();
        return SR_ERR_NOMEM;
    }
    // the pick kernel clears the bins it read: they are zero at the start of every pass
    SR_CHECK_HIP(hipMemset(ws.l_hist, 0, sizeof(unsigned long long) * 256 * (size_t)nq));
    return SR_OK;
}

// ----------------------------------------------------------------- device ---
__device__ inline uint64_t tl_key(const uint64_t* run, const uint64_t* cand, int64_t nr, int64_t i) {
    return i < nr ? run[i] : cand[i - nr];
}

// wave-aggregated slot reservation: every active lane with `want` gets a distinct index from *ctr
__device__ inline unsigned long long tl_reserve(unsigned long long* ctr, bool want) {
    const unsigned long long m = __ballot(want);
    if (m == 0) return 0;
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((long long)m) - 1;
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(ctr, (unsigned long long)__popcll(m));
    base = __shfl(base, leader);
    const unsigned long long below = lane == 0 ? 0ull : (m & (~0ull >> (64 - lane)));
    return base + (unsigned long long)__popcll(below);
}

__global__ __launch_bounds__(TL_THREADS) void topk_large_plan_kernel(const int* __restrict__ run_count, const int* __restrict__ cand_count,
                                                                    TopkLargeState* __restrict__ st, int64_t nq, int k,
                                                                    int64_t select_over, int cut_only) {
    const int64_t q = (int64_t)blockIdx.x * TL_THREADS + threadIdx.x;
    if (q >= nq) return;
    const int64_t nr = (int64_t)(uint32_t)run_count[q];        // up to 2k = 2^31
    const int64_t nc = cut_only ? 0 : (int64_t)cand_count[q];
    const int64_t n = nr + nc;
    TopkLargeState t;
    t.prefix = 0;
    t.minkey = ~0ull;
    t.remaining = k;
    t.nr = nr;
    t.nc = nc;
    t.n_holes = 0;
    t.n_filled = 0;
    t.pad_ = 0;
    if (cut_only) t.mode = nr > k ? 2 : 0;                       // topk_finalize: cut the set to k
    else if (nc == 0) t.mode = 0;
    else if (n <= k || (nr >= k && n <= select_over)) t.mode = 1;
    else t.mode = 2;
    st[q] = t;
}

__global__ __launch_bounds__(TL_THREADS) void topk_large_append_kernel(uint64_t* __restrict__ run_keys, const uint64_t* __restrict__ cand_keys,
                                                                      TopkLargeState* __restrict__ st, int k, int64_t cand_cap, int S) {
    const int64_t q = blockIdx.x / S;
    const int64_t sl = blockIdx.x % S;
    if (st[q].mode != 1) return;                                 // workgroup-uniform
    const int64_t nr = st[q].nr, nc = st[q].nc, n = nr + nc;
    uint64_t* run = run_keys + q * 2 * (int64_t)k;
    const uint64_t* cand = cand_keys + q * cand_cap;
    const int64_t stride = (int64_t)S * TL_THREADS;
    for (int64_t i = sl * TL_THREADS + threadIdx.x; i < nc; i += stride) run[nr + i] = cand[i];
    if (n == k) {
        // tau = smallest kept score (read from the sources: the copies above are not visible to other workgroups)
        uint64_t mn = ~0ull;
        for (int64_t i = sl * TL_THREADS + threadIdx.x; i < n; i += stride) {
            const uint64_t key = tl_key(run, cand, nr, i);
            mn = key < mn ? key : mn;
        }
        for (int off = 32; off > 0; off >>= 1) {
            const uint64_t o = __shfl_xor(mn, off);
            mn = o < mn ? o : mn;
        }
        if ((threadIdx.x & 63) == 0 && mn != ~0ull) atomicMin(reinterpret_cast<unsigned long long*>(&st[q].minkey), (unsigned long long)mn);
    }
}

// one 8-bit digit (bits [shift, shift + 8)) of the keys that match the digits chosen so far
__global__ __launch_bounds__(TL_THREADS) void topk_large_hist_kernel(const uint64_t* __restrict__ run_keys, const uint64_t* __restrict__ cand_keys,
                                                                    const TopkLargeState* __restrict__ st, unsigned long long* __restrict__ hist_g,
                                                                    int k, int64_t cand_cap, int S, int shift) {
    __shared__ unsigned int hist[256];
    const int64_t q = blockIdx.x / S;
    const int64_t sl = blockIdx.x % S;
    if (st[q].mode != 2) return;                                 // workgroup-uniform
    const int tid = threadIdx.x;
    const int64_t nr = st[q].nr, n = nr + st[q].nc;
    const uint64_t prefix = st[q].prefix;
    const uint64_t* run = run_keys + q * 2 * (int64_t)k;
    const uint64_t* cand = cand_keys + q * cand_cap;
    hist[tid] = 0;
    __syncthreads();
    const int64_t stride = (int64_t)S * TL_THREADS;
    for (int64_t i0 = sl * TL_THREADS + tid; i0 < n; i0 += stride * TL_UNROLL) {
        uint64_t keys[TL_UNROLL];
#pragma unroll
        for (int u = 0; u < TL_UNROLL; ++u) {
            const int64_t i = i0 + u * stride;
            keys[u] = i < n ? tl_key(run, cand, nr, i) : 0ull;
        }
#pragma unroll
        for (int u = 0; u < TL_UNROLL; ++u) {
            const bool in = i0 + u * stride < n && (shift == 56 || (keys[u] >> (shift + 8)) == prefix);
            const int bin = (int)((keys[u] >> shift) & 255);
            // the leading digits of a query's keys are mostly ONE value: a wave whose lanes agree adds once
            const unsigned long long act = __ballot(in);
            if (act) {
                const int b0 = __shfl(bin, __ffsll((long long)act) - 1);
                if (__ballot(in && bin == b0) == act) {
                    if ((tid & 63) == __ffsll((long long)act) - 1) atomicAdd(&hist[b0], (unsigned int)__popcll(act));
                } else if (in) {
                    atomicAdd(&hist[bin], 1u);
                }
            }
        }
    }
    __syncthreads();
    const unsigned int c = hist[tid];
    if (c) atomicAdd(&hist_g[q * 256 + tid], (unsigned long long)c);
}

// one workgroup per query: the bin that holds the key of rank `remaining`; clears the bins for the next pass
__global__ __launch_bounds__(TL_THREADS) void topk_large_pick_kernel(TopkLargeState* __restrict__ st, unsigned long long* __restrict__ hist_g,
                                                                    int shift) {
    __shared__ unsigned long long part[4];
    const int64_t q = blockIdx.x;
    if (st[q].mode != 2) return;                                 // workgroup-uniform; its bins are all zero
    const int tid = threadIdx.x;
    const int64_t remaining = st[q].remaining;
    const uint64_t prefix = st[q].prefix;
    const unsigned long long c = hist_g[q * 256 + tid];
    hist_g[q * 256 + tid] = 0;
    // suffix sums s = sum_{b >= tid} hist[b]: in the wave by shuffles, across the four waves through LDS
    unsigned long long sfx = c;
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long o = __shfl_down(sfx, off);
        if ((tid & 63) + off < 64) sfx += o;
    }
    if ((tid & 63) == 0) part[tid >> 6] = sfx;
    __syncthreads();
    for (int w = (tid >> 6) + 1; w < 4; ++w) sfx += part[w];
    const int64_t above = (int64_t)(sfx - c);
    if ((int64_t)sfx >= remaining && above < remaining) {      // exactly one bin: an empty bin has sfx == above
        const uint64_t p = (prefix << 8) | (uint64_t)tid;
        const int64_t r = remaining - above;
        if (shift == 0) {
            st[q].prefix = p;
            st[q].mode = 3;
        } else if (shift <= 32 && r == (int64_t)c) {
            // the score is complete and every key of this prefix is kept: T = the smallest key with this prefix
            st[q].prefix = p << shift;
            st[q].mode = 3;
        } else {
            st[q].prefix = p;
            st[q].remaining = r;
        }
    }
}

// slots of run[0, k) that are empty or hold a key below T
__global__ __launch_bounds__(TL_THREADS) void topk_large_holes_kernel(const uint64_t* __restrict__ run_keys, TopkLargeState* __restrict__ st,
                                                                     uint32_t* __restrict__ holes, int k, int S) {
    const int64_t q = blockIdx.x / S;
    const int64_t sl = blockIdx.x % S;
    if (st[q].mode != 3) return;
    const int64_t nr = st[q].nr;
    const uint64_t T = st[q].prefix;
    const uint64_t* run = run_keys + q * 2 * (int64_t)k;
    uint32_t* hq = holes + q * (int64_t)k;
    const int64_t stride = (int64_t)S * TL_THREADS;
    for (int64_t i0 = sl * TL_THREADS + threadIdx.x; i0 - (int64_t)threadIdx.x < k; i0 += stride) {   // wave-uniform trip count
        const bool hole = i0 < k && (i0 >= nr || run[i0] < T);
        const unsigned long long j = tl_reserve(&st[q].n_holes, hole);
        if (hole && j < (unsigned long long)k) hq[j] = (uint32_t)i0;
    }
}

// the kept keys of run[k, nr) and of the candidates into the listed holes
__global__ __launch_bounds__(TL_THREADS) void topk_large_fill_kernel(uint64_t* __restrict__ run_keys, const uint64_t* __restrict__ cand_keys,
                                                                    TopkLargeState* __restrict__ st, const uint32_t* __restrict__ holes,
                                                                    int k, int64_t cand_cap, int S) {
    const int64_t q = blockIdx.x / S;
    const int64_t sl = blockIdx.x % S;
    if (st[q].mode != 3) return;
    const int64_t nr = st[q].nr, nc = st[q].nc;
    const int64_t extra = nr > k ? nr - k : 0;
    const int64_t nf = extra + nc;
    const unsigned long long n_holes = st[q].n_holes;           // final: written by the previous launch
    const uint64_t T = st[q].prefix;
    uint64_t* run = run_keys + q * 2 * (int64_t)k;
    const uint64_t* cand = cand_keys + q * cand_cap;
    const uint32_t* hq = holes + q * (int64_t)k;
    const int64_t stride = (int64_t)S * TL_THREADS;
    for (int64_t f0 = sl * TL_THREADS + threadIdx.x; f0 - (int64_t)threadIdx.x < nf; f0 += stride) {
        const uint64_t key = f0 < nf ? (f0 < extra ? run[k + f0] : cand[f0 - extra]) : 0ull;
        const bool keep = f0 < nf && key >= T;
        const unsigned long long j = tl_reserve(&st[q].n_filled, keep);
        if (keep && j < n_holes) run[hq[j]] = key;               // sources at or above slot k, holes below it
    }
}

__global__ __launch_bounds__(TL_THREADS) void topk_large_finish_kernel(const TopkLargeState* __restrict__ st, int* __restrict__ run_count,
                                                                      int* __restrict__ cand_count, float* __restrict__ tau, int64_t nq, int k) {
    const int64_t q = (int64_t)blockIdx.x * TL_THREADS + threadIdx.x;
    if (q >= nq) return;
    const TopkLargeState t = st[q];
    if (t.mode == 1) {
        run_count[q] = (int)(uint32_t)(t.nr + t.nc);
        cand_count[q] = 0;
        if (t.nr + t.nc == k) tau[q] = sr_key_score(t.minkey);
    } else if (t.mode == 3) {
        run_count[q] = k;
        cand_count[q] = 0;
        tau[q] = sr_key_score(t.prefix);
    }
}

// ------------------------------------------------------------------- sort ---
// Bitonic sort, descending, of run[0, Pq) per query, Pq = next_pow2(kept keys) <= next_pow2(k) <= 2k slots.  A stage `size`
// wider than Pq leaves a query as it is (already sorted), so the launches are shaped by P = next_pow2(k) and every query skips
// what lies beyond its own Pq.
__host__ __device__ inline int64_t tl_pow2_at_least(int64_t v) {
    int64_t p = 2;
    while (p < v) p <<= 1;
    return p;
}

// stages size_lo .. size_hi (powers of two), steps j < min(size, TL_TILE) inside one LDS tile; `first`: load zeros past the
// query's kept keys (and store them back)
__global__ __launch_bounds__(TL_THREADS) void topk_large_sort_tile_kernel(uint64_t* __restrict__ run_keys, const int* __restrict__ run_count,
                                                                         int k, int64_t tiles, int64_t size_lo, int64_t size_hi, int first) {
    __shared__ uint64_t keys[TL_TILE];
    const int64_t q = blockIdx.x / tiles;
    const int64_t t = blockIdx.x % tiles;
    const int64_t cnt = (int64_t)(uint32_t)run_count[q];
    const int64_t Pq = tl_pow2_at_least(cnt);
    const int64_t base = t * TL_TILE;
    if (base >= Pq || size_lo > Pq) return;                    // workgroup-uniform
    const int L = (int)(Pq - base < TL_TILE ? Pq - base : TL_TILE);
    uint64_t* run = run_keys + q * 2 * (int64_t)k + base;
    for (int i = threadIdx.x; i < L; i += TL_THREADS) keys[i] = (!first || base + i < cnt) ? run[i] : 0ull;
    __syncthreads();
    const int64_t hi = size_hi < Pq ? size_hi : Pq;
    for (int64_t size = size_lo; size <= hi; size <<= 1) {
        for (int j = (int)((size >> 1) < TL_TILE ? (size >> 1) : TL_TILE / 2); j > 0; j >>= 1) {
            for (int p = threadIdx.x; p < L / 2; p += TL_THREADS) {
                const int i = (p / j) * 2 * j + (p % j);
                const bool desc = ((base + i) & size) == 0;
                const uint64_t a = keys[i], b = keys[i + j];
                if (desc ? (a < b) : (a > b)) {
                    keys[i] = b;
                    keys[i + j] = a;
                }
            }
            __syncthreads();
        }
    }
    for (int i = threadIdx.x; i < L; i += TL_THREADS) run[i] = keys[i];
}

// one step j >= TL_TILE of stage `size` in global memory: TL_UNROLL pairs per thread
__global__ __launch_bounds__(TL_THREADS) void topk_large_sort_step_kernel(uint64_t* __restrict__ run_keys, const int* __restrict__ run_count,
                                                                         int k, int64_t blocks, int64_t size, int64_t j) {
    const int64_t q = blockIdx.x / blocks;
    const int64_t b = blockIdx.x % blocks;
    const int64_t Pq = tl_pow2_at_least((int64_t)(uint32_t)run_count[q]);
    if (size > Pq) return;
    uint64_t* run = run_keys + q * 2 * (int64_t)k;
    const int64_t half = Pq >> 1;
#pragma unroll
    for (int u = 0; u < TL_UNROLL; ++u) {
        const int64_t p = (b * TL_UNROLL + u) * TL_THREADS + threadIdx.x;
        if (p < half) {
            const int64_t i = (p / j) * 2 * j + (p % j);
            const bool desc = (i & size) == 0;
            const uint64_t a = run[i], c = run[i + j];
            if (desc ? (a < c) : (a > c)) {
                run[i] = c;
                run[i + j] = a;
            }
        }
    }
}

__global__ __launch_bounds__(TL_THREADS) void topk_large_emit_kernel(const uint64_t* __restrict__ run_keys, const int* __restrict__ run_count,
                                                                    int k, int64_t blocks, float pad_score, float* __restrict__ out_scores,
                                                                    int64_t* __restrict__ out_ids, int32_t* __restrict__ out_counts) {
    const int64_t q = blockIdx.x / blocks;
    const int64_t b = blockIdx.x % blocks;
    const int64_t held = (int64_t)(uint32_t)run_count[q];
    const int64_t cnt = held < k ? held : k;
    const uint64_t* run = run_keys + q * 2 * (int64_t)k;
#pragma unroll
    for (int u = 0; u < TL_UNROLL; ++u) {
        const int64_t i = (b * TL_UNROLL + u) * TL_THREADS + threadIdx.x;
        if (i < k) {
            const int64_t o = q * (int64_t)k + i;
            if (i < cnt) {
                const uint64_t key = run[i];
                out_scores[o] = sr_key_score(key);
                out_ids[o] = (int64_t)sr_key_gid(key);
            } else {
                out_scores[o] = pad_score;
                out_ids[o] = -1;
            }
        }
    }
    if (out_counts && b == 0 && threadIdx.x == 0) out_counts[q] = (int32_t)cnt;
}

// ------------------------------------------------------------------- host ---
// slices per query: enough workgroups to fill the chip when there are few queries, at least 4096 keys each
static int slices_for(int64_t nq, int64_t n_max) {
    int64_t S = ceil_div64(2048, nq);
    const int64_t by_keys = ceil_div64(n_max, 4096);
    if (S > by_keys) S = by_keys;
    return S < 1 ? 1 : (int)S;
}

// append or select (cut_only: cut the running set to k, candidates ignored)
static int topk_large_select(TopkWS& ws, int64_t nq, int k, int64_t select_over, bool cut_only, hipStream_t s) {
    const int64_t cand_cap = ws.cand_cap;
    const int S = slices_for(nq, 2 * (int64_t)k + (cut_only ? 0 : cand_cap));
    TopkLargeState* st = reinterpret_cast<TopkLargeState*>(ws.l_state);
    const dim3 per_q((unsigned)ceil_div64(nq, TL_THREADS)), sliced((unsigned)(nq * S)), blk(TL_THREADS);
    hipLaunchKernelGGL(topk_large_plan_kernel, per_q, blk, 0, s, ws.run_count, ws.cand_count, st, nq, k, select_over, cut_only ? 1 : 0);
    SR_CHECK_LAUNCH();
    if (!cut_only) {
        hipLaunchKernelGGL(topk_large_append_kernel, sliced, blk, 0, s, ws.run_keys, ws.cand_keys, st, k, cand_cap, S);
        SR_CHECK_LAUNCH();
    }
    for (int shift = 56; shift >= 0; shift -= 8) {
        hipLaunchKernelGGL(topk_large_hist_kernel, sliced, blk, 0, s, ws.run_keys, ws.cand_keys, st, ws.l_hist, k, cand_cap, S, shift);
        SR_CHECK_LAUNCH();
        hipLaunchKernelGGL(topk_large_pick_kernel, dim3((unsigned)nq), blk, 0, s, st, ws.l_hist, shift);
        SR_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(topk_large_holes_kernel, sliced, blk, 0, s, ws.run_keys, st, ws.l_holes, k, S);
    SR_CHECK_LAUNCH();
    hipLaunchKernelGGL(topk_large_fill_kernel, sliced, blk, 0, s, ws.run_keys, ws.cand_keys, st, ws.l_holes, k, cand_cap, S);
    SR_CHECK_LAUNCH();
    hipLaunchKernelGGL(topk_large_finish_kernel, per_q, blk, 0, s, st, ws.run_count, ws.cand_count, ws.tau, nq, k);
    SR_CHECK_LAUNCH();
    return SR_OK;
}

int topk_large_compact(TopkWS& ws, int64_t nq, int k, int64_t select_over, hipStream_t s) {
    return topk_large_select(ws, nq, k, select_over, false, s);
}

int topk_large_finalize(TopkWS& ws, int64_t nq, int k, float pad_score, float* d_out_scores, int64_t* d_out_ids,
                        int32_t* d_out_counts, hipStream_t s) {
    SR_TRY(topk_large_select(ws, nq, k, 2 * (int64_t)k, true, s));
    const int64_t P = tl_pow2_at_least(k);                       // <= 2k slots
    const int64_t tiles = ceil_div64(P, TL_TILE);
    const dim3 blk(TL_THREADS);
    hipLaunchKernelGGL(topk_large_sort_tile_kernel, dim3((unsigned)(nq * tiles)), blk, 0, s, ws.run_keys, ws.run_count, k, tiles,
                       (int64_t)2, (int64_t)TL_TILE, 1);
    SR_CHECK_LAUNCH();
    const int64_t step_blocks = ceil_div64(P / 2, (int64_t)TL_THREADS * TL_UNROLL);
    for (int64_t size = 2 * TL_TILE; size <= P; size <<= 1) {
        for (int64_t j = size >> 1; j >= TL_TILE; j >>= 1) {
            hipLaunchKernelGGL(topk_large_sort_step_kernel, dim3((unsigned)(nq * step_blocks)), blk, 0, s, ws.run_keys, ws.run_count, k,
                               step_blocks, size, j);
            SR_CHECK_LAUNCH();
        }
        hipLaunchKernelGGL(topk_large_sort_tile_kernel, dim3((unsigned)(nq * tiles)), blk, 0, s, ws.run_keys, ws.run_count, k, tiles,
                           size, size, 0);
        SR_CHECK_LAUNCH();
    }
    const int64_t emit_blocks = ceil_div64(k, (int64_t)TL_THREADS * TL_UNROLL);
    hipLaunchKernelGGL(topk_large_emit_kernel, dim3((unsigned)(nq * emit_blocks)), blk, 0, s, ws.run_keys, ws.run_count, k, emit_blocks,
                       pad_score, d_out_scores, d_out_ids, d_out_counts);
    SR_CHECK_LAUNCH();
    return SR_OK;
}
