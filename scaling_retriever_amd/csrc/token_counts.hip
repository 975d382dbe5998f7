// sr_token_counts: token rows [B, L] (a loader's input_ids / attention_mask) -> a term-frequency CSR: per row the distinct counted ids
// ascending with their number of occurrences, and the row's number of counted slots (BM25's document length).  Contract: include/sr_hip.h,
// "lexical"; DESIGN.md 4.29.
//
// A row's slots become 32-bit keys - the id, TC_SKIP for a slot that does not count (masked, or one of the skip ids) - sorted ascending,
// so that the occurrences of an id form a run and the slots that do not count sit behind all runs.  The first slot of a run is its head;
// a head's frequency is the distance to the end of its run; a head's place in the row is the number of heads before it.  The sort runs
// twice: the count launch keeps the number of heads per row, the row offsets come from the scan the range searches share
// (launch_range_scan with one chunk), and the fill launch sorts again and writes.  Two instantiations:
//   tc_wave_kernel<R>   rows of at most 64 R slots (R = 1, 2, 4): one wave per row, four rows per workgroup, the keys in R registers per
//                       lane in the order slot = r * 64 + lane.  A bitonic step at distance >= 64 exchanges two registers of a lane, one
//                       below 64 is a cross-lane exchange; heads and run ends are ballots.  No LDS, no barrier.
//   tc_block_kernel     longer rows up to TC_MAX_LEN: one workgroup per row, the keys in LDS, sr_block_sort, heads appended through
//                       sr_block_scan 256 slots at a time, the end of a run found by a binary search of the sorted keys.
#include "block_primitives.h"
#include "range_scan.h"

#define TC_MAX_LEN 8192                 // sr_token_counts_max_len(): 32 KB of keys, and f32(count) is exact
#define TC_MAX_SKIP 16
#define TC_THREADS 256                  // the four waves of sr_block_scan
#define TC_WAVE_MAX_LEN 256             // rows up to here take the wave kernel: the longest it is instantiated for (R = 4).  No crossing below
                                        // it: at 16 384 rows it takes 0.34 - 0.45 of the workgroup kernel's time at every L <= 256 (profiles/bm25.json)
#define TC_SKIP 0xFFFFFFFFu             // key of a slot that does not count: behind every id (ids are below 2^31)

struct TcArgs {
    const int64_t* ids; const int64_t* mask;
    int64_t B; int L;
    int64_t n_terms;
    int n_skip; int32_t skip[TC_MAX_SKIP];
    unsigned long long* first_bad;      // count launch: smallest b * L + position of a counted id outside [0, n_terms)
    uint32_t* row_heads;                // count launch: distinct counted ids per row
    const int64_t* row_ptr;             // fill launch
    int32_t* cols; float* vals; int32_t* len;
    int64_t capacity;
};

// the key of slot i of row b; a counted id out of range is recorded (count launch) and does not count
template <bool FILL>
__device__ inline uint32_t tc_key(const TcArgs& a, int64_t b, int i) {
    if (i >= a.L) return TC_SKIP;
    const int64_t at = b * a.L + i;
    if (a.mask && a.mask[at] == 0) return TC_SKIP;
    const int64_t id = a.ids[at];
    for (int j = 0; j < a.n_skip; ++j)
        if (id == (int64_t)a.skip[j]) return TC_SKIP;
    if (id < 0 || id >= a.n_terms) {
        if (!FILL) atomicMin(a.first_bad, (unsigned long long)at);
        return TC_SKIP;
    }
    return (uint32_t)id;
}

template <int R, bool FILL>
__global__ __launch_bounds__(TC_THREADS) void tc_wave_kernel(TcArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * (TC_THREADS / 64) + (threadIdx.x >> 6);
    if (b >= a.B) return;                                               // whole waves: no barrier below
    constexpr int N = 64 * R;
    uint32_t key[R];
#pragma unroll
    for (int r = 0; r < R; ++r) key[r] = tc_key<FILL>(a, b, r * 64 + lane);
    // bitonic sort, ascending, of slot e = r * 64 + lane
#pragma unroll
    for (int size = 2; size <= N; size <<= 1) {
#pragma unroll
        for (int j = size >> 1; j > 0; j >>= 1) {
            if (j >= 64) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int jr = j >> 6;
                    if ((r & jr) == 0) {
                        const bool up = (((r * 64) & size) == 0);       // size > j >= 64: the lane bits do not enter
                        const uint32_t x = key[r], y = key[r | jr];
                        const bool sw = up ? (x > y) : (x < y);
                        key[r] = sw ? y : x;
                        key[r | jr] = sw ? x : y;
                    }
                }
            } else {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const int e = r * 64 + lane;
                    const uint32_t o = __shfl_xor(key[r], j);
                    const bool keep_min = ((lane & j) == 0) == ((e & size) == 0);
                    const uint32_t lo = key[r] < o ? key[r] : o, hi = key[r] < o ? o : key[r];
                    key[r] = keep_min ? lo : hi;
                }
            }
        }
    }
    // heads and run ends as ballots, register by register
    unsigned long long H[R], T[R];
    int n_heads = 0, n_counted = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        uint32_t prev = __shfl_up(key[r], 1), next = __shfl_down(key[r], 1);
        const uint32_t prev_reg = r > 0 ? __shfl(key[r > 0 ? r - 1 : 0], 63) : TC_SKIP;     // slot 0 has no slot before it: TC_SKIP differs from a counted key
        const uint32_t next_reg = r + 1 < R ? __shfl(key[r + 1 < R ? r + 1 : r], 0) : TC_SKIP;
        if (lane == 0) prev = prev_reg;
        if (lane == 63) next = next_reg;
        const bool counted = key[r] != TC_SKIP;
        H[r] = __ballot(counted && prev != key[r]);
        T[r] = __ballot(counted && next != key[r]);
        n_heads += __popcll(H[r]);
        n_counted += __popcll(__ballot(counted));
    }
    if (!FILL) {
        if (lane == 0) a.row_heads[b] = (uint32_t)n_heads;
        return;
    }
    const int64_t base = a.row_ptr[b];
    int before = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if ((H[r] >> lane) & 1ull) {
            const int rank = before + __popcll(H[r] & ((1ull << lane) - 1ull));
            int end = -1;                                               // slot of the run's last key: the first run end at or behind this head
#pragma unroll
            for (int rr = r; rr < R; ++rr) {
                const unsigned long long m = rr == r ? (T[rr] >> lane) << lane : T[rr];
                if (end < 0 && m != 0ull) end = rr * 64 + __builtin_ctzll(m);
            }
            const int64_t p = base + rank;
            if (p < a.capacity) {
                a.cols[p] = (int32_t)key[r];
                a.vals[p] = (float)(end - (r * 64 + lane) + 1);
            }
        }
        before += __popcll(H[r]);
    }
    if (lane == 0) a.len[b] = n_counted;
}

// first slot of keys[0, P) whose key is above k (P a power of two; the keys are sorted)
__device__ inline int tc_upper(const uint32_t* keys, int P, uint32_t k) {
    int lo = 0, n = P;
    while (n > 0) {
        const int half = n >> 1;
        if (keys[lo + half] <= k) { lo += half + 1; n -= half + 1; } else n = half;
    }
    return lo;
}

template <bool FILL>
__global__ __launch_bounds__(TC_THREADS) void tc_block_kernel(TcArgs a, int P) {
    extern __shared__ __attribute__((aligned(16))) uint32_t tc_keys[];      // [P]
    __shared__ int lw[4];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    for (int i = tid; i < P; i += TC_THREADS) tc_keys[i] = tc_key<FILL>(a, b, i);
    __syncthreads();
    sr_block_sort<TC_THREADS, false>(tc_keys, P);
    const int64_t base = FILL ? a.row_ptr[b] : 0;
    int before = 0;
    for (int i0 = 0; i0 < P; i0 += TC_THREADS) {                            // uniform trip count: the scan's barriers
        const int i = i0 + tid;
        const uint32_t k = tc_keys[i];
        const int head = k != TC_SKIP && (i == 0 || tc_keys[i - 1] != k) ? 1 : 0;
        int tot;
        const int rank = before + sr_block_scan(head, lw, tot);
        if (FILL && head) {
            const int64_t p = base + rank;
            if (p < a.capacity) {
                a.cols[p] = (int32_t)k;
                a.vals[p] = (float)(tc_upper(tc_keys, P, k) - i);
            }
        }
        before += tot;
    }
    if (tid == 0) {
        if (FILL) a.len[b] = tc_upper(tc_keys, P, TC_SKIP - 1u);          // the counted keys sit in front of the first TC_SKIP
        else a.row_heads[b] = (uint32_t)before;
    }
}

// rows up to this length take the wave kernel; the dev switch SR_TC_WAVE_MAX_LEN (0 .. 256) moves it for tools/bench_bm25.py's sweep
static int tc_wave_max_len() {
    const char* e = sr_dev_getenv("SR_TC_WAVE_MAX_LEN");
    if (!e) return TC_WAVE_MAX_LEN;
    const int v = atoi(e);
    return v < 0 ? 0 : (v > TC_WAVE_MAX_LEN ? TC_WAVE_MAX_LEN : v);
}

template <bool FILL>
static int tc_launch(const TcArgs& a, hipStream_t s) {
    const unsigned wave_grid = (unsigned)ceil_div64(a.B, TC_THREADS / 64);
    if (a.L <= tc_wave_max_len()) {
        if (a.L <= 64) hipLaunchKernelGGL((tc_wave_kernel<1, FILL>), dim3(wave_grid), dim3(TC_THREADS), 0, s, a);
        else if (a.L <= 128) hipLaunchKernelGGL((tc_wave_kernel<2, FILL>), dim3(wave_grid), dim3(TC_THREADS), 0, s, a);
        else hipLaunchKernelGGL((tc_wave_kernel<4, FILL>), dim3(wave_grid), dim3(TC_THREADS), 0, s, a);
    } else {
        const int P = sr_pow2_at_least(a.L, 2 * TC_THREADS);                // at least one slot per thread in every scan step
        hipLaunchKernelGGL((tc_block_kernel<FILL>), dim3((unsigned)a.B), dim3(TC_THREADS), (size_t)P * sizeof(uint32_t), s, a, P);
    }
    SR_CHECK_LAUNCH();
    return SR_OK;
}

extern "C" int sr_token_counts_max_len(void) { return TC_MAX_LEN; }

extern "C" int sr_token_counts(const int64_t* d_ids, const int64_t* d_mask, int64_t B, int64_t L, const int32_t* h_skip, int n_skip,
                               int64_t n_terms, int64_t* d_row_ptr, int32_t* d_cols, float* d_vals, int32_t* d_len, int64_t capacity,
                               int64_t* h_nnz, sr_stream stream) {
    SR_REQUIRE(B >= 0 && L >= 0 && capacity >= 0, "sr_token_counts: bad sizes (B %lld, L %lld, capacity %lld)", (long long)B, (long long)L,
               (long long)capacity);
    SR_REQUIRE(L <= TC_MAX_LEN, "sr_token_counts: rows of %lld slots, at most %d", (long long)L, TC_MAX_LEN);
    SR_REQUIRE(B < (1ll << 24), "sr_token_counts: %lld rows, at most 2^24 - 1 a call (one workgroup of 256 threads per row: the launch limit)", (long long)B);
    SR_REQUIRE(n_skip >= 0 && n_skip <= TC_MAX_SKIP && (n_skip == 0 || h_skip), "sr_token_counts: n_skip = %d, expected 0 .. %d ids in h_skip", n_skip,
               TC_MAX_SKIP);
    SR_REQUIRE(n_terms >= 1 && n_terms < (1ll << 31), "sr_token_counts: n_terms = %lld is outside [1, 2^31)", (long long)n_terms);
    SR_REQUIRE(d_row_ptr && h_nnz && (B == 0 || (d_len && (L == 0 || d_ids))), "sr_token_counts: null pointer");
    hipStream_t s = (hipStream_t)stream;
    *h_nnz = 0;
    if (B == 0 || L == 0) {
        SR_CHECK_HIP(hipMemsetAsync(d_row_ptr, 0, (size_t)(B + 1) * sizeof(int64_t), s));
        if (B > 0) SR_CHECK_HIP(hipMemsetAsync(d_len, 0, (size_t)B * sizeof(int32_t), s));
        SR_CHECK_HIP(hipStreamSynchronize(s));
        return SR_OK;
    }
    TcArgs a;
    a.ids = d_ids; a.mask = d_mask; a.B = B; a.L = (int)L; a.n_terms = n_terms; a.n_skip = n_skip;
    for (int j = 0; j < TC_MAX_SKIP; ++j) a.skip[j] = j < n_skip ? h_skip[j] : 0;
    a.row_ptr = d_row_ptr; a.cols = d_cols; a.vals = d_vals; a.len = d_len; a.capacity = capacity;
    CallBuf<uint32_t> d_heads;          // per-row head counts, zeroed by the scan that turns them into d_row_ptr
    SR_TRY(d_heads.reserve(B, "sr_token_counts"));
    CallStatus<unsigned long long> st;
    SR_TRY(st.begin("sr_token_counts", s));
    a.first_bad = st.p; a.row_heads = d_heads.p;
    SR_TRY(tc_launch<false>(a, s));
    SR_TRY(launch_range_scan(d_heads.p, 1, B, d_row_ptr, s));
    int64_t total = 0;
    unsigned long long first_bad = ~0ull;
    const hipError_t copied = hipMemcpyAsync(&total, d_row_ptr + B, sizeof(total), hipMemcpyDeviceToHost, s);
    SR_TRY(st.read(&first_bad, s));                                         // waits for the stream, after a failed copy too
    SR_CHECK_HIP(copied);
    if (first_bad != ~0ull) {
        int64_t id = 0;
        SR_CHECK_HIP(hipMemcpy(&id, d_ids + first_bad, sizeof(id), hipMemcpyDeviceToHost));
        sr_set_error("sr_token_counts: token id %lld (row %llu, position %llu) is outside [0, %lld) (only the row offsets were written)", (long long)id,
                     first_bad / (unsigned long long)L, first_bad % (unsigned long long)L, (long long)n_terms);
        return SR_ERR_INVALID;
    }
    *h_nnz = total;
    if (total > capacity || (total > 0 && (!d_cols || !d_vals))) {
        sr_set_error("sr_token_counts: %lld entries, capacity %lld", (long long)total, (long long)capacity);
        return SR_ERR_NOMEM;
    }
    return tc_launch<true>(a, s);
}
