// Test-only hook: the top-k protocol of topk.hip / topk_large.hip on a caller-supplied key stream (tests/test_topk_replay_gpu.py,
// tests/topk_cases.py).  topk_reset -> per step (a producer appends the step's entries as every score kernel does -> topk_compact2 ->
// the thresholds, counts and the running set are copied out) -> topk_finalize.  The workspace lives for one call; nothing here is
// reached by a search, and no existing kernel or launch function is touched.
#include "common.h"

// one workgroup per query; plain appends behind one atomic reservation per entry (seg_n == 0)
__global__ __launch_bounds__(256) void replay_append_kernel(const float* __restrict__ scores, const int64_t* __restrict__ ids,
                                                            int64_t n_stream, int64_t begin, int64_t end, int filter,
                                                            const float* __restrict__ tau, uint64_t* __restrict__ cand_keys,
                                                            int* __restrict__ cand_count, int64_t cand_cap) {
    const int64_t q = blockIdx.x;
    const float t = tau[q];
    uint64_t* dst = cand_keys + q * cand_cap;
    for (int64_t i = begin + threadIdx.x; i < end; i += 256) {
        const int64_t id = ids[q * n_stream + i];
        const float sc = scores[q * n_stream + i];
        if (id >= 0 && (!filter || sc >= t)) {
            const int p = atomicAdd(&cand_count[q], 1);
            if (p < cand_cap) dst[p] = sr_make_key(sc, (uint32_t)id);
        }
    }
}

// segmented slots, the contract of dense_split_kernel.h: producer p takes the step's entries [p seg_group, (p + 1) seg_group) and owns
// segment p.  1..SR_SEG_P survivors go to its segment and their count to seg_cnt; more, or a producer beyond seg_n, take one atomic
// reservation in the head of the buffer, which ends at seg_off.  One thread per producer.
__global__ __launch_bounds__(256) void replay_append_segments_kernel(const float* __restrict__ scores, const int64_t* __restrict__ ids,
                                                                     int64_t n_stream, int64_t begin, int64_t end, int filter,
                                                                     const float* __restrict__ tau, uint64_t* __restrict__ cand_keys,
                                                                     int* __restrict__ cand_count, int64_t cand_cap,
                                                                     unsigned char* __restrict__ seg_cnt, int seg_n, int64_t seg_off,
                                                                     int seg_group) {
    const int64_t q = blockIdx.x;
    const float t = tau[q];
    uint64_t* dst = cand_keys + q * cand_cap;
    const float* sq = scores + q * n_stream;
    const int64_t* iq = ids + q * n_stream;
    const int64_t n_prod = (end - begin + seg_group - 1) / seg_group;
    for (int64_t p = threadIdx.x; p < n_prod; p += 256) {
        const int64_t lo = begin + p * seg_group, hi = lo + seg_group < end ? lo + seg_group : end;
        const bool seg_ok = p < seg_n;
        uint64_t* seg_dst = dst + seg_off + p * SR_SEG_P;          // only dereferenced when seg_ok
        int n = 0;
        for (int64_t i = lo; i < hi; ++i)
            if (iq[i] >= 0 && (!filter || sq[i] >= t)) {
                if (seg_ok && n < SR_SEG_P) seg_dst[n] = sr_make_key(sq[i], (uint32_t)iq[i]);
                ++n;
            }
        if (n == 0) continue;
        if (seg_ok && n <= SR_SEG_P) {
            seg_cnt[q * seg_n + p] = (unsigned char)n;
            continue;
        }
        int at = atomicAdd(&cand_count[q], n);
        for (int64_t i = lo; i < hi; ++i)
            if (iq[i] >= 0 && (!filter || sq[i] >= t)) {
                if (at < seg_off) dst[at] = sr_make_key(sq[i], (uint32_t)iq[i]);
                ++at;
            }
    }
}

// what the compaction is about to see: the appended candidates plus the segment counts, at most the head's seg_off slots
__global__ void replay_count_kernel(const int* __restrict__ cand_count, const unsigned char* __restrict__ seg_cnt, int seg_n,
                                    int64_t seg_off, int64_t nq, int32_t* __restrict__ out) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    int64_t n = cand_count[q];
    for (int i = 0; i < seg_n; ++i) n += seg_cnt[q * seg_n + i];
    if (seg_n > 0 && n > seg_off) n = seg_off;
    out[q] = (int32_t)n;
}

__global__ void replay_fill_kernel(float* __restrict__ dst, float v, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = v;
}

namespace {
// the call's workspace: released on every exit path, after the stream has finished with it
struct ReplayWS {
    TopkWS ws;
    hipStream_t s;
    explicit ReplayWS(hipStream_t s_) : s(s_) {}
    ReplayWS(const ReplayWS&) = delete;
    ~ReplayWS() {
        (void)hipStreamSynchronize(s);
        ws.release();
    }
};
}  // namespace

extern "C" int sr_topk_replay(const float* d_scores, const int64_t* d_ids, int64_t nq, int64_t n_stream, const int64_t* h_steps,
                              int n_steps, int k, int k2, int64_t select_over, int filter, int seg_n, int seg_group, float tau2_init,
                              float pad_score, float* d_out_scores, int64_t* d_out_ids, int32_t* d_out_counts, float* d_trace_tau,
                              float* d_trace_tau2, int32_t* d_trace_cand, int32_t* d_trace_run, uint64_t* d_trace_keys,
                              sr_stream stream) {
    SR_REQUIRE(d_scores && d_ids && h_steps && d_out_scores && d_out_ids && d_out_counts && d_trace_tau && d_trace_tau2 && d_trace_cand &&
                   d_trace_run,
               "sr_topk_replay: null pointer");
    SR_REQUIRE(nq >= 0 && nq <= (1 << 20) && n_stream >= 0 && n_stream <= (1ll << 32) && n_steps >= 0 && n_steps <= (1 << 16),
               "sr_topk_replay: bad sizes (nq=%lld n_stream=%lld n_steps=%d)", (long long)nq, (long long)n_stream, n_steps);
    SR_REQUIRE(k >= 1 && k <= (1 << 20), "sr_topk_replay: k = %d outside [1, 2^20]", k);
    SR_REQUIRE(k2 >= 0 && k2 < k && (k2 == 0 || k <= SR_MAX_TOPK), "sr_topk_replay: k2 = %d needs 0 <= k2 < k = %d and k <= %d", k2, k,
               SR_MAX_TOPK);
    SR_REQUIRE(filter == 0 || filter == 1, "sr_topk_replay: filter %d is neither 0 nor 1", filter);
    SR_REQUIRE(seg_n >= 0 && seg_n <= (1 << 20) && seg_n % 4 == 0 && (seg_n == 0 || k <= SR_MAX_TOPK),
               "sr_topk_replay: seg_n = %d must be a multiple of 4 in [0, 2^20], and 0 for k > %d", seg_n, SR_MAX_TOPK);
    SR_REQUIRE(seg_n == 0 || (seg_group >= 1 && seg_group <= (1 << 16)), "sr_topk_replay: seg_group = %d outside [1, 2^16]", seg_group);
    int64_t longest = 0;
    for (int i = 0; i < n_steps; ++i) {
        const int64_t len = h_steps[i + 1] - h_steps[i];
        SR_REQUIRE(h_steps[i] >= 0 && len >= 0 && h_steps[i + 1] <= n_stream, "sr_topk_replay: steps must ascend inside [0, n_stream] (step %d: %lld..%lld)",
                   i, (long long)h_steps[i], (long long)h_steps[i + 1]);
        SR_REQUIRE(len <= (1ll << 22), "sr_topk_replay: step %d has %lld entries, more than 2^22", i, (long long)len);
        longest = len > longest ? len : longest;
    }
    if (nq == 0) return SR_OK;
    hipStream_t s = (hipStream_t)stream;
    ReplayWS r(s);
    TopkWS& ws = r.ws;
    const int64_t head = longest > 0 ? longest : 1;               // every entry of the longest step may survive
    if (seg_n > 0) SR_TRY(ws.ensure_segments(nq, k, head, seg_n));
    else SR_TRY(ws.ensure(nq, k, head));
    CallBuf<float> tau2;
    SR_TRY(tau2.reserve(nq, "sr_topk_replay"));
    const dim3 per_q((unsigned)ceil_div64(nq, 256)), blk(256);
    SR_TRY(topk_reset(ws, nq, s));
    hipLaunchKernelGGL(replay_fill_kernel, per_q, blk, 0, s, tau2.p, tau2_init, nq);
    SR_CHECK_LAUNCH();
    for (int i = 0; i < n_steps; ++i) {
        const int64_t begin = h_steps[i], end = h_steps[i + 1];
        if (end > begin) {
            if (seg_n > 0)
                hipLaunchKernelGGL(replay_append_segments_kernel, dim3((unsigned)nq), blk, 0, s, d_scores, d_ids, n_stream, begin, end, filter,
                                   ws.tau, ws.cand_keys, ws.cand_count, ws.cand_cap, ws.seg_cnt, ws.seg_n, ws.seg_off, seg_group);
            else
                hipLaunchKernelGGL(replay_append_kernel, dim3((unsigned)nq), blk, 0, s, d_scores, d_ids, n_stream, begin, end, filter, ws.tau,
                                   ws.cand_keys, ws.cand_count, ws.cand_cap);
            SR_CHECK_LAUNCH();
        }
        hipLaunchKernelGGL(replay_count_kernel, per_q, blk, 0, s, ws.cand_count, ws.seg_cnt, ws.seg_n, ws.seg_off, nq, d_trace_cand + (int64_t)i * nq);
        SR_CHECK_LAUNCH();
        SR_TRY(topk_compact2(ws, nq, k, k2, tau2.p, select_over, s));
        SR_CHECK_HIP(hipMemcpyAsync(d_trace_tau + (int64_t)i * nq, ws.tau, sizeof(float) * (size_t)nq, hipMemcpyDeviceToDevice, s));
        SR_CHECK_HIP(hipMemcpyAsync(d_trace_tau2 + (int64_t)i * nq, tau2.p, sizeof(float) * (size_t)nq, hipMemcpyDeviceToDevice, s));
        SR_CHECK_HIP(hipMemcpyAsync(d_trace_run + (int64_t)i * nq, ws.run_count, sizeof(int32_t) * (size_t)nq, hipMemcpyDeviceToDevice, s));
        if (d_trace_keys)        // the fresh workspace holds exactly [nq, 2k] keys
            SR_CHECK_HIP(hipMemcpyAsync(d_trace_keys + (int64_t)i * nq * 2 * k, ws.run_keys, sizeof(uint64_t) * (size_t)nq * 2 * (size_t)k,
                                        hipMemcpyDeviceToDevice, s));
    }
    SR_TRY(topk_finalize(ws, nq, k, pad_score, d_out_scores, d_out_ids, d_out_counts, s));
    SR_CHECK_HIP(hipStreamSynchronize(s));
    return SR_OK;
}
