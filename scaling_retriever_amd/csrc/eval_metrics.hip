// Evaluation on the device: the ranking metrics of a result list against graded judgements, and the paired
// randomization test over two runs' per-query values.  No reference counterpart: its utils/metrics.py hands {qid: {docid: score}}
// dicts to pytrec_eval.
//   sr_eval_ranked         one workgroup per query.  Every valid entry finds its place in the query's judgement row by binary search
//                          (its index there, kept per slot in LDS).  The judged entries are compacted and sorted by that index, so a
//                          judged document that occurs twice stands beside itself.  The valid entries are then compacted as one 64-bit
//                          word each, f2ord(score) << 32 | tie_key << 16 | (0xFFFF - slot), sorted descending (bitonic) in score order,
//                          and the relevant ones are compacted in rank order with a block scan as rank << 32 | grade.  One lane runs
//                          the serial sums over those few words and writes every cut as it passes it.  eval_means_kernel then sums
//                          every column over the evaluated queries in ascending q, one lane per column, the rows staged through LDS.
//   sr_eval_randomization  one thread per permutation walks the queries in order; the differences are staged through LDS in chunks and
//                          read as a broadcast; one splitmix64 word gives the signs of 64 queries.  Per-workgroup counts are summed
//                          by a last pass (integer sums: the bytes do not depend on the order).
// All arithmetic on the result path is fp64 with contraction off; `/` is the correctly rounded division.  The kernels compute no
// logarithm: log2(i + 2) and the ideal DCGs come from the host.
#include "block_primitives.h"
#include <limits.h>

#define EV_MAX_CUTS 16
#define EV_MAX_COLS 8
#define EV_THREADS 256                  // the four waves of sr_block_scan and sr_block_min
#define EV_MEAN_ROWS 32                 // queries per LDS tile of the means kernel
#define EV_CHUNK 256                    // queries per LDS tile of the randomization kernel (a multiple of 64)
#define EV_MAX_PERM_BLOCKS 4096

struct EvalStatus {                     // device words of a call: what the kernels found wrong (~0: nothing)
    unsigned long long bad_qrel;        // smallest query whose judgement row is not strictly ascending (or lies outside the arrays)
    unsigned long long bad_tie;         // smallest flat position of a valid entry whose tie_key is outside [0, 65536)
    unsigned long long bad_dup;         // smallest flat position of a valid entry whose judged document stands earlier in its row
};

struct EvalArgs {
    const float* scores; const int64_t* ids; const int32_t* counts; const int32_t* tie; const int64_t* exclude;
    const int64_t* indptr; const int64_t* qrel_ids; const int32_t* grades;
    int64_t n_qrel;
    const int32_t* n_rel; const double* idcg; const double* log2t;
    int cuts[EV_MAX_CUTS];
    int n_cuts, order, depth, pmax;     // pmax = next power of two >= depth: the slots of the sorts
    int64_t rr_depth, nq;
    double* out; int32_t* flags;
    EvalStatus* st;
};

__global__ __launch_bounds__(EV_THREADS) void eval_ranked_kernel(EvalArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    uint64_t* keys = reinterpret_cast<uint64_t*>(smem_raw);     // [pmax] the judged entries, then the ranking, then the relevant entries
    int32_t* jw = reinterpret_cast<int32_t*>(keys + a.pmax);    // [depth] per slot: the entry's index in the judgement row, -1 = not judged, -2 = not valid
    __shared__ int lw[4], red[4], s_rr_end;
    const int tid = threadIdx.x, depth = a.depth, n_cuts = a.n_cuts, ncol = 1 + 4 * a.n_cuts;
    const int64_t q = blockIdx.x;

    // ---- the judgement row: inside the arrays, strictly ascending
    int64_t lo = a.indptr[q], hi = a.indptr[q + 1];
    if (lo < 0 || hi < lo || hi > a.n_qrel) {
        if (tid == 0) atomicMin(&a.st->bad_qrel, (unsigned long long)q);
        lo = hi = 0;
    }
    for (int64_t i = lo + 1 + tid; i < hi; i += EV_THREADS)
        if (a.qrel_ids[i - 1] >= a.qrel_ids[i]) atomicMin(&a.st->bad_qrel, (unsigned long long)q);
    int cnt = depth;
    if (a.counts) {
        cnt = a.counts[q];
        cnt = cnt < 0 ? 0 : (cnt > depth ? depth : cnt);
    }
    const int64_t excl = a.exclude ? a.exclude[q] : -1;         // an id < 0 is padding already: any negative value excludes nothing
    if (tid == 0) s_rr_end = depth;

    // ---- pass A: every valid entry's index in the judgement row; the judged ones compacted as index << 32 | slot
    int njud = 0;
    for (int base = 0; base < depth; base += EV_THREADS) {
        const int r = base + tid;
        int j = -2;
        if (r < cnt) {
            const int64_t id = a.ids[q * depth + r];
            if (id >= 0 && id != excl) {
                int64_t l = lo, h = hi;
                while (l < h) {                                 // lower bound of id in the row
                    const int64_t mid = (l + h) >> 1;
                    if (a.qrel_ids[mid] < id) l = mid + 1; else h = mid;
                }
                j = (l < hi && a.qrel_ids[l] == id) ? (int)(l - lo) : -1;
            }
        }
        if (r < depth) jw[r] = j;
        int tot;
        const int ex = sr_block_scan(j >= 0 ? 1 : 0, lw, tot);
        if (j >= 0) keys[njud + ex] = ((uint64_t)(uint32_t)j << 32) | (uint64_t)r;
        njud += tot;
    }
    if (njud >= 2) {                                            // uniform: njud is the scan's total
        const int P = sr_pow2_at_least(njud, 2);
        for (int i = njud + tid; i < P; i += EV_THREADS) keys[i] = 0ull;
        __syncthreads();
        sr_block_sort<EV_THREADS, true>(keys, P);
        // equal indexes stand together, the later slot first: the entry in front of an equal one is a repeat
        for (int i = tid; i + 1 < njud; i += EV_THREADS) {
            const uint64_t x = keys[i];
            if ((uint32_t)(x >> 32) == (uint32_t)(keys[i + 1] >> 32))
                atomicMin(&a.st->bad_dup, (unsigned long long)(q * depth + (int64_t)(x & 0xffffffffu)));
        }
    }
    __syncthreads();

    // ---- pass B: the valid entries compacted in list order, one key each
    int nv = 0;
    for (int base = 0; base < depth; base += EV_THREADS) {
        const int r = base + tid;
        const bool valid = r < depth && jw[r] >= -1;
        int tot;
        const int ex = sr_block_scan(valid ? 1 : 0, lw, tot);
        if (valid) {
            const int v = nv + ex;
            uint64_t key = (uint64_t)(0xFFFF - r);
            if (a.tie) {
                const int32_t t = a.tie[q * depth + r];
                if (t < 0 || t > 0xFFFF) atomicMin(&a.st->bad_tie, (unsigned long long)(q * depth + r));
                key |= (uint64_t)((uint32_t)t & 0xFFFFu) << 16;
            }
            if (a.order == SR_EVAL_ORDER_SCORE) key |= (uint64_t)sr_f2ord(a.scores[q * depth + r]) << 32;
            keys[v] = key;
            if (a.rr_depth > 0 && (int64_t)v == a.rr_depth) s_rr_end = r;  // the first entry behind recip_rank's cut
        }
        nv += tot;
    }
    if (a.order == SR_EVAL_ORDER_SCORE && nv >= 2) {
        const int P = sr_pow2_at_least(nv, 2);
        for (int i = nv + tid; i < P; i += EV_THREADS) keys[i] = 0ull;  // below every key: the high word of a key is never 0
        __syncthreads();
        sr_block_sort<EV_THREADS, true>(keys, P);
    } else {
        __syncthreads();
    }

    // ---- pass C: the relevant entries compacted in rank order as rank << 32 | grade; recip_rank's rank among the entries in front of its cut
    const int rr_end = s_rr_end;
    int nrel = 0, nflag = 0, rr_rank = INT_MAX;
    for (int base = 0; base < nv; base += EV_THREADS) {
        const int p = base + tid;
        int g = 0;
        bool flag = false;
        if (p < nv) {
            const int r = 0xFFFF - (int)(keys[p] & 0xFFFFu);
            const int j = jw[r];
            if (j >= 0) g = a.grades[lo + j];
            flag = r < rr_end;
        }
        const bool rel = g > 0;
        int tot, frank = p + 1;
        if (rr_end < depth) {                                   // uniform
            int ftot;
            frank = nflag + sr_block_scan(flag ? 1 : 0, lw, ftot) + 1;
            nflag += ftot;
        }
        const int ex = sr_block_scan(rel ? 1 : 0, lw, tot);     // its barriers stand behind the loads of keys
        if (rel) {
            keys[nrel + ex] = ((uint64_t)(uint32_t)(p + 1) << 32) | (uint64_t)(uint32_t)g;    // nrel + ex <= p: a slot already read
            if (flag && frank < rr_rank) rr_rank = frank;
        }
        nrel += tot;
    }
    rr_rank = sr_block_min(rr_rank, red);                       // its barriers stand behind the stores of keys

    const bool evaluated = hi > lo && nv > 0;
    const int n_rel = a.n_rel[q];
    double* out = a.out + q * (int64_t)ncol;
    if (tid == 0) a.flags[q] = (evaluated ? 1 : 0) | (n_rel <= 0 ? 2 : 0);
    if (!evaluated) {
        for (int c = tid; c < ncol; c += EV_THREADS) out[c] = 0.0;
        return;
    }
    if (tid != 0) return;
    {
#pragma clang fp contract(off)
        out[0] = rr_rank != INT_MAX ? 1.0 / (double)rr_rank : 0.0;
        int h = 0, i = 0;
        double dcg = 0.0, ap = 0.0;
        for (int c = 0; c < n_cuts; ++c) {
            const int cut = a.cuts[c];
            while (i < nrel) {
                const uint64_t w = keys[i];
                const int rank = (int)(w >> 32);
                if (rank > cut) break;
                ++h;
                dcg = dcg + (double)(int32_t)(uint32_t)w / a.log2t[rank - 1];
                ap = ap + (double)h / (double)rank;
                ++i;
            }
            const double idcg = a.idcg[q * n_cuts + c];
            out[1 + c] = n_rel > 0 ? (double)h / (double)n_rel : 0.0;
            out[1 + n_cuts + c] = idcg > 0.0 ? dcg / idcg : 0.0;
            out[1 + 2 * n_cuts + c] = n_rel > 0 ? (double)h / (double)(n_rel < cut ? n_rel : cut) : 0.0;
            out[1 + 3 * n_cuts + c] = n_rel > 0 ? ap / (double)n_rel : 0.0;
        }
    }
}

// Column means over the evaluated queries: every column is summed in ascending q from 0.0, one rounded add each, by ONE lane - the order
// the contract asks for.  The rows come through LDS EV_MEAN_ROWS at a time so that the serial lane never waits for HBM.
__global__ __launch_bounds__(EV_THREADS) void eval_means_kernel(const double* out, const int32_t* flags, int64_t nq, int ncol, double* mean,
                                                              int64_t* n_eval) {
    __shared__ double tile[EV_MEAN_ROWS * (1 + 4 * EV_MAX_CUTS)];
    __shared__ int32_t fl[EV_MEAN_ROWS];
    const int tid = threadIdx.x;
    double sum = 0.0;
    int64_t n = 0;
    for (int64_t q0 = 0; q0 < nq; q0 += EV_MEAN_ROWS) {
        const int rows = (int)(nq - q0 < EV_MEAN_ROWS ? nq - q0 : EV_MEAN_ROWS);
        for (int i = tid; i < rows * ncol; i += EV_THREADS) tile[i] = out[q0 * ncol + i];
        if (tid < rows) fl[tid] = flags[q0 + tid];
        __syncthreads();
        if (tid < ncol) {
#pragma clang fp contract(off)
            for (int r = 0; r < rows; ++r)
                if (fl[r] & 1) {
                    sum = sum + tile[r * ncol + tid];
                    ++n;
                }
        }
        __syncthreads();
    }
    if (tid < ncol) mean[tid] = n > 0 ? sum / (double)n : 0.0;
    if (tid == 0) *n_eval = n;
}

extern "C" int sr_eval_max_cuts(void) { return EV_MAX_CUTS; }

extern "C" int sr_eval_ranked(const float* d_scores, const int64_t* d_ids, const int32_t* d_counts, const int32_t* d_tie_key,
                              const int64_t* d_exclude, int64_t nq, int64_t depth, const int64_t* d_qrel_indptr, const int64_t* d_qrel_ids,
                              const int32_t* d_qrel_grades, int64_t n_qrel, const int32_t* d_n_rel, const double* d_idcg,
                              const double* d_log2, const int32_t* h_cuts, int n_cuts, int order, int64_t rr_depth, double* d_out,
                              int32_t* d_out_flags, double* d_out_mean, int64_t* d_out_n, sr_stream stream) {
    SR_REQUIRE(nq >= 0 && nq < (1ll << 30) && n_qrel >= 0, "sr_eval_ranked: bad sizes (nq %lld, n_qrel %lld)", (long long)nq, (long long)n_qrel);
    SR_REQUIRE(depth >= 1, "sr_eval_ranked: depth = %lld, a list holds at least one entry", (long long)depth);
    if (depth > SR_MAX_TOPK) {
        sr_set_error("sr_eval_ranked: depth = %lld, lists of 1 to %d entries are ranked in LDS", (long long)depth, SR_MAX_TOPK);
        return SR_ERR_UNSUPPORTED;
    }
    SR_REQUIRE(n_cuts >= 0 && n_cuts <= EV_MAX_CUTS, "sr_eval_ranked: n_cuts = %d, 0 to %d cuts are evaluated", n_cuts, EV_MAX_CUTS);
    SR_REQUIRE(n_cuts == 0 || h_cuts, "sr_eval_ranked: null pointer (cuts)");
    for (int c = 0; c < n_cuts; ++c)
        SR_REQUIRE(h_cuts[c] >= 1 && (c == 0 || h_cuts[c] > h_cuts[c - 1]), "sr_eval_ranked: the cuts must be >= 1 and strictly ascending (cut %d)", c);
    SR_REQUIRE(order == SR_EVAL_ORDER_SCORE || order == SR_EVAL_ORDER_LIST, "sr_eval_ranked: bad order %d", order);
    SR_REQUIRE(rr_depth >= 0, "sr_eval_ranked: rr_depth = %lld must be >= 0", (long long)rr_depth);
    SR_REQUIRE(order != SR_EVAL_ORDER_SCORE || d_scores, "sr_eval_ranked: the score order reads the scores, got a null pointer");
    SR_REQUIRE(d_ids && d_qrel_indptr && d_n_rel && d_log2 && d_out && d_out_flags && d_out_mean && d_out_n, "sr_eval_ranked: null pointer");
    SR_REQUIRE(n_qrel == 0 || (d_qrel_ids && d_qrel_grades), "sr_eval_ranked: null pointer (judgements)");
    SR_REQUIRE(n_cuts == 0 || d_idcg, "sr_eval_ranked: null pointer (idcg)");
    hipStream_t s = (hipStream_t)stream;
    const int ncol = 1 + 4 * n_cuts;
    CallStatus<EvalStatus> st;
    SR_TRY(st.begin("sr_eval_ranked", s));
    EvalArgs a;
    a.scores = d_scores; a.ids = d_ids; a.counts = d_counts; a.tie = d_tie_key; a.exclude = d_exclude;
    a.indptr = d_qrel_indptr; a.qrel_ids = d_qrel_ids; a.grades = d_qrel_grades; a.n_qrel = n_qrel;
    a.n_rel = d_n_rel; a.idcg = d_idcg; a.log2t = d_log2;
    for (int c = 0; c < EV_MAX_CUTS; ++c) a.cuts[c] = c < n_cuts ? h_cuts[c] : 0;
    a.n_cuts = n_cuts; a.order = order; a.depth = (int)depth; a.pmax = sr_pow2_at_least(depth, 2);
    a.rr_depth = rr_depth; a.nq = nq;
    a.out = d_out; a.flags = d_out_flags; a.st = st.p;
    if (nq > 0) {
        const size_t lds = (size_t)a.pmax * 8 + (size_t)depth * 4;      // 48 KB at the cap
        hipLaunchKernelGGL(eval_ranked_kernel, dim3((unsigned)nq), dim3(EV_THREADS), lds, s, a);
        SR_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(eval_means_kernel, dim3(1), dim3(EV_THREADS), 0, s, (const double*)d_out, (const int32_t*)d_out_flags, nq, ncol,
                       d_out_mean, d_out_n);
    SR_CHECK_LAUNCH();
    EvalStatus h;
    SR_TRY(st.read(&h, s));
    if (h.bad_qrel != ~0ull) {
        sr_set_error("sr_eval_ranked: the judged ids of query %llu are not strictly ascending inside the judgement arrays", h.bad_qrel);
        return SR_ERR_INVALID;
    }
    if (h.bad_tie != ~0ull) {
        int32_t t = 0;
        SR_CHECK_HIP(hipMemcpy(&t, d_tie_key + h.bad_tie, sizeof(t), hipMemcpyDeviceToHost));
        sr_set_error("sr_eval_ranked: tie_key %d (query %llu, entry %llu) is outside [0, 65536)", (int)t, h.bad_tie / (unsigned long long)depth,
                     h.bad_tie % (unsigned long long)depth);
        return SR_ERR_INVALID;
    }
    if (h.bad_dup != ~0ull) {
        int64_t id = 0;
        SR_CHECK_HIP(hipMemcpy(&id, d_ids + h.bad_dup, sizeof(id), hipMemcpyDeviceToHost));
        sr_set_error("sr_eval_ranked: judged id %lld (query %llu, entry %llu) occurs twice among the valid entries of its list", (long long)id,
                     h.bad_dup / (unsigned long long)depth, h.bad_dup % (unsigned long long)depth);
        return SR_ERR_INVALID;
    }
    return SR_OK;
}

// ------------------------------------------------------------------------------------------------ randomization test ---
__device__ inline uint64_t ev_mix(uint64_t z) {                 // the splitmix64 step
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// T_obs[c]: the sum of diff[c, q] over q ascending from +0.0, one lane per column
__global__ void eval_tobs_kernel(const double* diff, int n_cols, int64_t n, double* t_obs) {
#pragma clang fp contract(off)
    const int c = threadIdx.x;
    if (c >= n_cols) return;
    double t = 0.0;
    for (int64_t q = 0; q < n; ++q) t = t + diff[c * n + q];
    t_obs[c] = t;
}

// One thread per permutation; a workgroup takes EV_THREADS permutations at a time and strides over the rest.  part[block, c] = the
// number of its permutations with |T_b[c]| >= |T_obs[c]|.
template <int NC>
__global__ __launch_bounds__(EV_THREADS) void eval_perm_kernel(const double* diff, int64_t n, int64_t n_perm, uint64_t seed, uint64_t W,
                                                             const double* t_obs, int64_t* part) {
    __shared__ double sd[NC][EV_CHUNK];
    __shared__ int lw[4];
    const int tid = threadIdx.x;
    double aobs[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) aobs[c] = fabs(t_obs[c]);
    int64_t cnt[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) cnt[c] = 0;
    for (int64_t b0 = (int64_t)blockIdx.x * EV_THREADS; b0 < n_perm; b0 += (int64_t)gridDim.x * EV_THREADS) {
        const int64_t b = b0 + tid;
        const uint64_t wbase = seed + (uint64_t)b * W;
        double t[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) t[c] = 0.0;
        for (int64_t q0 = 0; q0 < n; q0 += EV_CHUNK) {
            const int len = (int)(n - q0 < EV_CHUNK ? n - q0 : EV_CHUNK);
            __syncthreads();                                    // the previous tile has been read
            for (int i = tid; i < NC * EV_CHUNK; i += EV_THREADS) {
                const int c = i / EV_CHUNK, j = i - c * EV_CHUNK;
                if (j < len) sd[c][j] = diff[c * n + q0 + j];
            }
            __syncthreads();
            {
#pragma clang fp contract(off)
                for (int j0 = 0; j0 < len; j0 += 64) {
                    const uint64_t word = ev_mix(wbase + (uint64_t)((q0 + j0) >> 6));
                    const int m = len - j0 < 64 ? len - j0 : 64;
                    for (int j = 0; j < m; ++j) {
                        const bool flip = (word >> j) & 1ull;
#pragma unroll
                        for (int c = 0; c < NC; ++c) {
                            const double d = sd[c][j0 + j];     // one address for the whole wave: a broadcast
                            t[c] = t[c] + (flip ? -d : d);
                        }
                    }
                }
            }
        }
        if (b < n_perm) {
#pragma unroll
            for (int c = 0; c < NC; ++c) cnt[c] += fabs(t[c]) >= aobs[c] ? 1 : 0;
        }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        int tot;
        (void)sr_block_scan((int)cnt[c], lw, tot);              // at most 2^31 / gridDim.x permutations per thread: fits an int
        if (tid == 0) part[(int64_t)blockIdx.x * NC + c] = tot;
    }
}

__global__ void eval_count_kernel(const int64_t* part, int n_blocks, int n_cols, int64_t* count_ge) {
    const int c = threadIdx.x;
    if (c >= n_cols) return;
    int64_t sum = 0;
    for (int b = 0; b < n_blocks; ++b) sum += part[(int64_t)b * n_cols + c];
    count_ge[c] = sum;
}

template <int NC>
static int launch_perm(const double* diff, int64_t n, int64_t n_perm, uint64_t seed, const double* t_obs, int64_t* part, int blocks,
                       hipStream_t s) {
    hipLaunchKernelGGL((eval_perm_kernel<NC>), dim3((unsigned)blocks), dim3(EV_THREADS), 0, s, diff, n, n_perm, seed,
                       (uint64_t)((n + 63) >> 6), t_obs, part);
    SR_CHECK_LAUNCH();
    return SR_OK;
}

extern "C" int sr_eval_randomization(const double* d_diff, int n_cols, int64_t n, int64_t n_perm, uint64_t seed, double* d_t_obs,
                                     int64_t* d_count_ge, sr_stream stream) {
    SR_REQUIRE(n_cols >= 1 && n_cols <= EV_MAX_COLS, "sr_eval_randomization: n_cols = %d, 1 to %d columns share the signs", n_cols, EV_MAX_COLS);
    SR_REQUIRE(n >= 0 && n < (1ll << 40), "sr_eval_randomization: bad n %lld", (long long)n);
    SR_REQUIRE(n_perm >= 1 && n_perm < (1ll << 31), "sr_eval_randomization: n_perm = %lld, 1 to 2^31 - 1 permutations are drawn", (long long)n_perm);
    SR_REQUIRE((n == 0 || d_diff) && d_t_obs && d_count_ge, "sr_eval_randomization: null pointer");
    hipStream_t s = (hipStream_t)stream;
    // every thread's count must fit the int of the block sum: at most 2^31 / (blocks * EV_THREADS) + 1 rounds, each adds 0 or 1
    int64_t blocks = ceil_div64(n_perm, EV_THREADS);
    if (blocks > EV_MAX_PERM_BLOCKS) blocks = EV_MAX_PERM_BLOCKS;
    CallBuf<int64_t> part;
    SR_TRY(part.reserve(blocks * n_cols, "sr_eval_randomization"));
    hipLaunchKernelGGL(eval_tobs_kernel, dim3(1), dim3(64), 0, s, d_diff, n_cols, n, d_t_obs);
    SR_CHECK_LAUNCH();
    switch (n_cols) {
        case 1: SR_TRY(launch_perm<1>(d_diff, n, n_perm, seed, d_t_obs, part.p, (int)blocks, s)); break;
        case 2: SR_TRY(launch_perm<2>(d_diff, n, n_perm, seed, d_t_obs, part.p, (int)blocks, s)); break;
        case 3: SR_TRY(launch_perm<3>(d_diff, n, n_perm, seed, d_t_obs, part.p, (int)blocks, s)); break;
        case 4: SR_TRY(launch_perm<4>(d_diff, n, n_perm, seed, d_t_obs, part.p, (int)blocks, s)); break;
        case 5: SR_TRY(launch_perm<5>(d_diff, n, n_perm, seed, d_t_obs, part.p, (int)blocks, s)); break;
        case 6: SR_TRY(launch_perm<6>(d_diff, n, n_perm, seed, d_t_obs, part.p, (int)blocks, s)); break;
        case 7: SR_TRY(launch_perm<7>(d_diff, n, n_perm, seed, d_t_obs, part.p, (int)blocks, s)); break;
        default: SR_TRY(launch_perm<8>(d_diff, n, n_perm, seed, d_t_obs, part.p, (int)blocks, s)); break;
    }
    hipLaunchKernelGGL(eval_count_kernel, dim3(1), dim3(64), 0, s, (const int64_t*)part.p, (int)blocks, n_cols, d_count_ge);
    SR_CHECK_LAUNCH();
    SR_CHECK_HIP(hipStreamSynchronize(s));                  // the partial counts are freed when the call returns
    return SR_OK;
}
