// Rank fusion: per query the top-k distinct documents of up to 8 ranked lists by a fused score that is defined on the
// lists alone - reciprocal rank fusion, sum_l w_l / (c + rank_l), or CombSUM over per-list min-max normalised scores.  No reference
// counterpart: its HybridRetriever (scaling_retriever/indexer.py:859-1019) dumps the two heads' runs and fuses nothing.
//   sr_rank_fuse  one workgroup per query.  The valid entries are staged in LDS as 64-bit words id << 32 | list << 16 | rank0 and sorted
//                 ascending (bitonic), so the entries of one document are adjacent and in list order; the thread that finds a run's head
//                 walks it and adds the contributions one rounded fp32 add at a time - that fixes the order of the sum.  Every slot then
//                 holds the key f2ord(fused) << 32 | ~id of the run it heads (0: no head), the keys are sorted descending, the first k
//                 leave.  The id-sorted words stay resident: a binary search finds a result's run again for its per-list ranks.
#include "block_primitives.h"
#include "hybrid_fuse.h"
#include <float.h>
#include <math.h>

#define RF_MAX_LISTS 8
#define RF_PAD (~0ull)                  // an unused slot: sorts behind every entry (an entry's list field is < 8)

struct FuseArgs {
    const int64_t* ids; const int32_t* counts; const float* scores;
    int n_lists, depth, P, k;           // P = next power of two >= n_lists * depth: the slots of both sorts
    int64_t nq;
    float w[RF_MAX_LISTS];
    float c;
    float* out_scores; int64_t* out_ids; int32_t* out_counts; int32_t* out_ranks;
    HybridStatus* st;                   // first_bad_a: an id >= 2^32; first_bad_b: an id twice in one row (flat positions of ids)
};

// The fused score of the run of one document that starts at ent[i]: +0.0f plus the contribution of every list that holds it, in
// ascending list order, one rounded add each.  Plain operators under contract(off) (see hf_fuse in hybrid_fuse.hip): prev + w * norm
// must stay a product and a sum.  The division is the correctly rounded one (v_div_scale / v_div_fmas / v_div_fixup; the Makefile
// asks for it by name).  A list that occurs twice in the run is an id twice in one row: reported, its second entry adds nothing.
template <int METHOD>
__device__ inline float rf_run_sum(const FuseArgs& a, const uint64_t* ent, int i, uint32_t id, int64_t q, const float* s_w,
                                   const float* s_mn, const float* s_span) {
#pragma clang fp contract(off)
    float sum = 0.0f;
    int prev_l = -1;
    for (int j = i; j < a.P; ++j) {
        const uint64_t x = ent[j];
        if (x == RF_PAD || (uint32_t)(x >> 32) != id) break;
        const int l = (int)((x >> 16) & 0xffffu), r0 = (int)(x & 0xffffu);
        if (l == prev_l) {
            atomicMin(&a.st->first_bad_b, (unsigned long long)(((int64_t)l * a.nq + q) * a.depth + r0));
            continue;
        }
        prev_l = l;
        float contrib;
        if (METHOD == SR_FUSE_RRF) {
            const float den = a.c + (float)(r0 + 1);
            contrib = s_w[l] / den;
        } else {
            const float span = s_span[l];
            float norm = 1.0f;
            if (span > 0.0f) {
                const float d = a.scores[((int64_t)l * a.nq + q) * a.depth + r0] - s_mn[l];
                norm = d / span;
            }
            contrib = s_w[l] * norm;
        }
        sum = sum + contrib;
    }
    return sum;
}

template <int METHOD>
__global__ __launch_bounds__(HF_THREADS) void rank_fuse_kernel(FuseArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    uint64_t* ent = reinterpret_cast<uint64_t*>(smem_raw);      // [P] the entries, ascending by (id, list, rank0)
    uint64_t* keys = ent + a.P;                                 // [P] the result keys, descending
    __shared__ int lw[4], s_cnt[RF_MAX_LISTS];
    __shared__ float s_w[RF_MAX_LISTS], s_mn[RF_MAX_LISTS], s_span[RF_MAX_LISTS], s_red[2][RF_MAX_LISTS][4];
    const int tid = threadIdx.x, L = a.n_lists, depth = a.depth, P = a.P, k = a.k;
    const int64_t q = blockIdx.x;

#pragma unroll
    for (int l = 0; l < RF_MAX_LISTS; ++l)
        if (tid == l) {
            s_w[l] = a.w[l];
            int cnt = depth;
            if (l < L && a.counts) {
                cnt = a.counts[(int64_t)l * a.nq + q];
                cnt = cnt < 0 ? 0 : (cnt > depth ? depth : cnt);
            }
            s_cnt[l] = l < L ? cnt : 0;
        }
    __syncthreads();

    const int n_in = L * depth;
    for (int i = tid; i < P; i += HF_THREADS) {
        uint64_t e = RF_PAD;
        if (i < n_in) {
            const int l = i / depth, r = i - l * depth;
            if (r < s_cnt[l]) {
                const int64_t pos = ((int64_t)l * a.nq + q) * depth + r;
                const int64_t id = a.ids[pos];
                if (id >= (1ll << 32)) atomicMin(&a.st->first_bad_a, (unsigned long long)pos);
                else if (id >= 0) e = ((uint64_t)id << 32) | ((uint64_t)l << 16) | (uint64_t)r;
            }
        }
        ent[i] = e;
    }
    if (METHOD == SR_FUSE_MINMAX) {
        // smallest and largest score over the valid entries of every list: min / max are exact, so the order of the reduction is free
        for (int l = 0; l < L; ++l) {
            float mn = INFINITY, mx = -INFINITY;
            const int64_t row = ((int64_t)l * a.nq + q) * depth;
            for (int r = tid; r < s_cnt[l]; r += HF_THREADS)
                if (a.ids[row + r] >= 0) {
                    const float s = a.scores[row + r];
                    mn = fminf(mn, s);
                    mx = fmaxf(mx, s);
                }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                mn = fminf(mn, __shfl_xor(mn, off));
                mx = fmaxf(mx, __shfl_xor(mx, off));
            }
            if ((tid & 63) == 0) {
                s_red[0][l][tid >> 6] = mn;
                s_red[1][l][tid >> 6] = mx;
            }
        }
        __syncthreads();
        if (tid < L) {
#pragma clang fp contract(off)
            const float mn = fminf(fminf(s_red[0][tid][0], s_red[0][tid][1]), fminf(s_red[0][tid][2], s_red[0][tid][3]));
            const float mx = fmaxf(fmaxf(s_red[1][tid][0], s_red[1][tid][1]), fmaxf(s_red[1][tid][2], s_red[1][tid][3]));
            s_mn[tid] = mn;
            s_span[tid] = mx - mn;                              // an empty list: -inf, never read
        }
    }
    __syncthreads();
    sr_block_sort<HF_THREADS, false>(ent, P);

    // every slot: the key of the run it heads, else 0 (below every key: the high word of a key is never 0)
    int heads = 0;
    for (int i = tid; i < P; i += HF_THREADS) {
        uint64_t key = 0ull;
        const uint64_t e = ent[i];
        if (e != RF_PAD) {
            const uint32_t id = (uint32_t)(e >> 32);
            if (i == 0 || (uint32_t)(ent[i - 1] >> 32) != id) {     // pads sort last: ent[i - 1] is an entry
                const float fused = rf_run_sum<METHOD>(a, ent, i, id, q, s_w, s_mn, s_span);
                key = ((uint64_t)sr_f2ord(fused) << 32) | (uint64_t)(~id);
                ++heads;
            }
        }
        keys[i] = key;
    }
    int distinct;
    (void)sr_block_scan(heads, lw, distinct);                   // its barriers stand behind the stores of keys
    sr_block_sort<HF_THREADS, true>(keys, P);

    const int m = distinct < k ? distinct : k;
    for (int i = tid; i < k; i += HF_THREADS) {
        const int64_t o = q * k + i;
        uint32_t id = 0;
        if (i < m) {
            const uint64_t key = keys[i];
            id = ~(uint32_t)(key & 0xffffffffu);
            a.out_scores[o] = sr_ord2f((uint32_t)(key >> 32));  // the fused bits: a sum that starts at +0.0f is never -0.0f
            a.out_ids[o] = (int64_t)id;
        } else {
            a.out_scores[o] = -FLT_MAX;
            a.out_ids[o] = -1;
        }
        if (a.out_ranks) {
            int32_t* rk = a.out_ranks + o * L;
            for (int l = 0; l < L; ++l) rk[l] = 0;
            if (i < m) {
                const uint64_t x = (uint64_t)id << 32;          // first entry of the run: lower bound in the id-sorted words
                int lo = 0, hi = P;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (ent[mid] < x) lo = mid + 1; else hi = mid;
                }
                for (int j = lo; j < P; ++j) {
                    const uint64_t e = ent[j];
                    if (e == RF_PAD || (uint32_t)(e >> 32) != id) break;
                    const int l = (int)((e >> 16) & 0xffffu);
                    if (l < L && rk[l] == 0) rk[l] = (int32_t)(e & 0xffffu) + 1;
                }
            }
        }
    }
    if (tid == 0) a.out_counts[q] = m;
}

template <int METHOD>
static int launch_fuse(const FuseArgs& a, hipStream_t s) {
    static DeviceOnce lds_set;
    SR_TRY(sr_allow_lds(lds_set, rank_fuse_kernel<METHOD>, 16 * 2 * SR_MAX_TOPK));
    const size_t lds = (size_t)a.P * 16;                        // 32 KB for 2 x 1000, 128 KB at the limit
    hipLaunchKernelGGL((rank_fuse_kernel<METHOD>), dim3((unsigned)a.nq), dim3(HF_THREADS), lds, s, a);
    SR_CHECK_LAUNCH();
    return SR_OK;
}

extern "C" int sr_rank_fuse(const int64_t* d_ids, const int32_t* d_counts, const float* d_scores, int n_lists, int64_t nq, int64_t depth,
                            int method, const float* h_weights, float c, int k, float* d_out_scores, int64_t* d_out_ids,
                            int32_t* d_out_counts, int32_t* d_out_ranks, sr_stream stream) {
    SR_REQUIRE(nq >= 0 && nq < (1ll << 30), "sr_rank_fuse: bad nq");
    if (n_lists < 1 || n_lists > RF_MAX_LISTS || depth < 1 || depth > SR_MAX_TOPK || (int64_t)n_lists * depth > 2 * SR_MAX_TOPK) {
        sr_set_error("sr_rank_fuse: %d lists of %lld entries: 1 to %d lists of 1 to %d entries, at most %d entries together, are sorted in LDS",
                     n_lists, (long long)depth, RF_MAX_LISTS, SR_MAX_TOPK, 2 * SR_MAX_TOPK);
        return SR_ERR_UNSUPPORTED;
    }
    if (k < 1 || k > SR_MAX_TOPK) {
        sr_set_error("sr_rank_fuse: k = %d, 1 to %d are returned", k, SR_MAX_TOPK);
        return SR_ERR_UNSUPPORTED;
    }
    SR_REQUIRE(method == SR_FUSE_RRF || method == SR_FUSE_MINMAX, "sr_rank_fuse: bad method %d", method);
    SR_REQUIRE(h_weights, "sr_rank_fuse: null pointer (weights)");
    for (int l = 0; l < n_lists; ++l)
        SR_REQUIRE(h_weights[l] >= 0.f && h_weights[l] < INFINITY, "sr_rank_fuse: the weights must be finite and >= 0 (list %d)", l);
    SR_REQUIRE(method != SR_FUSE_RRF || (c > -1.f && c < INFINITY), "sr_rank_fuse: c must be finite and > -1");
    SR_REQUIRE(method != SR_FUSE_MINMAX || d_scores, "sr_rank_fuse: min-max fusion reads the scores, got a null pointer");
    SR_REQUIRE(d_ids && d_out_scores && d_out_ids && d_out_counts, "sr_rank_fuse: null pointer");
    if (nq == 0) return SR_OK;
    hipStream_t s = (hipStream_t)stream;
    CallStatus<HybridStatus> st;
    SR_TRY(st.begin("sr_rank_fuse", s));
    FuseArgs a;
    a.ids = d_ids; a.counts = d_counts; a.scores = d_scores;
    a.n_lists = n_lists; a.depth = (int)depth; a.P = sr_pow2_at_least((int64_t)n_lists * depth, 2); a.k = k; a.nq = nq;
    for (int l = 0; l < RF_MAX_LISTS; ++l) a.w[l] = l < n_lists ? h_weights[l] : 0.f;
    a.c = c;
    a.out_scores = d_out_scores; a.out_ids = d_out_ids; a.out_counts = d_out_counts; a.out_ranks = d_out_ranks;
    a.st = st.p;
    if (method == SR_FUSE_RRF) SR_TRY(launch_fuse<SR_FUSE_RRF>(a, s)); else SR_TRY(launch_fuse<SR_FUSE_MINMAX>(a, s));
    HybridStatus h;
    SR_TRY(st.read(&h, s));
    const unsigned long long bad = h.first_bad_a != ~0ull ? h.first_bad_a : h.first_bad_b;
    if (bad != ~0ull) {
        int64_t id = 0;
        SR_CHECK_HIP(hipMemcpy(&id, d_ids + bad, sizeof(id), hipMemcpyDeviceToHost));
        const unsigned long long row = bad / (unsigned long long)depth;
        if (h.first_bad_a != ~0ull)
            sr_set_error("sr_rank_fuse: id %lld (list %llu, query %llu, entry %llu) does not fit the 32 id bits of a key", (long long)id,
                         row / (unsigned long long)nq, row % (unsigned long long)nq, bad % (unsigned long long)depth);
        else
            sr_set_error("sr_rank_fuse: id %lld (list %llu, query %llu, entry %llu) occurs twice among the valid entries of its row",
                         (long long)id, row / (unsigned long long)nq, row % (unsigned long long)nq, bad % (unsigned long long)depth);
        return SR_ERR_INVALID;
    }
    return SR_OK;
}
