// Internal launch interface of the encoder kernels (gfx950).
#pragma once
#include "common.h"

typedef unsigned short bf16_t;  // raw bf16 bits

enum GemmEpilogue {
    EPI_STORE_BF16 = 0,  // C[M,N] bf16 = acc
    EPI_RESID_F32 = 1,   // X[M,N] fp32 += acc            (o_proj / down_proj + residual)
    EPI_SWIGLU = 2,      // C[M,N/2] bf16 = silu(gate) * up, W rows interleaved gate/up in 16-row blocks
    EPI_SEGMAX = 3,      // out[seq_of[m], n] = max(out, acc) over the tokens of each sequence (sparse head)
    EPI_STORE_F32 = 4,   // C[M,N] fp32 = acc (tests)
    EPI_QKV_ROPE = 5,    // C[M,N] bf16 = acc with RoPE applied (fp32) to features n < n_rope (q and k heads)
    EPI_QKV_ROPE_F32 = 6,   // same, C[M,N] fp32 (fp32 regime: the attention reads fp32 operands)
    EPI_SWIGLU_SPLIT = 7,   // fp32 regime: silu(gate) * up in fp32, stored as split-bf16 plane segments (out_map)
    EPI_SWIGLU_F32 = 8,     // C[M,N/2] fp32 = silu(gate) * up (accurate exp, true division)
    // fp32 regime on fp16 planes: operands are [rows, 3K] fp16 plane segments of rows scaled by a power of two, the MFMA is
    // v_mfma_f32_16x16x32_f16 and the accumulators are multiplied by a_scale[m] * w_scale[n] (the inverse scales) before the
    // epilogue of the base behaviour runs
    EPI_H_FIRST = 9,
    EPI_QKV_ROPE_F32_H = 9, EPI_RESID_F32_H = 10, EPI_SWIGLU_F32_H = 11, EPI_SEGMAX_H = 12,
    // silu(gate) * up in fp32, multiplied by out_scale[m] (a power of two from a rigorous row bound, so that no value can
    // overflow fp16) and stored directly as the [f1 | f0 | f0] fp16 plane segments the down_proj GEMM consumes: C [M, 3 N/2]
    // (out_nseg = 3), or [f1 | f0], C [M, 2 N/2] (out_nseg = 2)
    EPI_SWIGLU_SPLIT_H = 13,
    EPI_SWIGLU_SPLITH_BASE = 14,    // internal: the base behaviour of EPI_SWIGLU_SPLIT_H
};

// ---- fp32 regime: fp32 operands as sums of bf16 planes ---------------------------------------------------
// x = p0 + p1 + p2, each plane the bf16 rounding of what the previous ones left (the subtractions are exact in fp32),
// so three planes carry the whole 24-bit significand.  A fp32-class product a.w is the sum of plane products
// a_i . w_j; laid out along K as segments it is ONE bf16 GEMM with K' = n_seg * K (fp32 accumulate in the MFMA):
//   A' = [a_{pa[0]} | a_{pa[1]} | ...]   W' = [w_{pw[0]} | w_{pw[1]} | ...]      (smallest terms first)
//   3 planes, 6 products (error below fp32 epsilon):  pa = 2 0 1 1 0 0   pw = 0 2 1 0 1 0
//   2 planes, 3 products (~2^-17 relative):           pa = 1 0 0         pw = 0 1 0
#define SR_MAX_SEG 6
struct SplitMap {
    int n_seg;
    int plane[SR_MAX_SEG];
};
//   fp16 planes (SR_FP32_PLANES_F16 = 16): two fp16 planes of power-of-two scaled rows, the same 3-product maps; 11 + 11
//   significand bits: truncation 3 * 2^-22, below the fp32 accumulation's own rounding - an fp32 GEMM's error at half the work
#define SR_FP32_PLANES_F16 16
inline SplitMap split_map_a(int planes) {
    if (planes == 3) return SplitMap{6, {2, 0, 1, 1, 0, 0}};
    return SplitMap{3, {1, 0, 0, 0, 0, 0}};
}
inline SplitMap split_map_w(int planes) {
    if (planes == 3) return SplitMap{6, {0, 2, 1, 0, 1, 0}};
    return SplitMap{3, {0, 1, 0, 0, 0, 0}};
}

struct GemmArgs {
    const bf16_t* A;   // activations [M, K] row-major
    const bf16_t* W;   // weights [N, K] row-major (nn.Linear layout)
    int M, N, K;
    void* C;           // output (bf16 or fp32 by epilogue); ldc = N (or N/2 for SWIGLU)
    const int* seq_of; // EPI_SEGMAX: sequence id of each token row
    int64_t out_ld;    // EPI_SEGMAX: leading dimension of out (= N)
    // EPI_QKV_ROPE
    const int* pos;         // [M] rope position of each token
    const float* rope_cos;  // [max_pos, head_dim / 2]
    const float* rope_sin;
    int n_rope;             // features [0, n_rope) are rotated (q heads then k heads), the rest (v) stored as is
    int head_dim;           // 64 or 128
    const float* bias;      // QKV + RoPE epilogues only: [N] fp32 bias of the q, k and v rows (the order of W), added to the fp32 accumulator
                            // before the rotation (Qwen2: nn.Linear(bias=True) on q_proj / k_proj / v_proj); null = no bias (Llama)
    unsigned long long* stamps;  // diagnostics only (tools/micro): 4 s_memrealtime stamps (100 MHz) per workgroup-tile, else null
    const float* a_scale;   // _H epilogues: [M] inverse scale of each activation row (a power of two)
    const float* w_scale;   // _H epilogues: [N] inverse scale of each weight row
    const float* out_scale; // EPI_SWIGLU_SPLIT_H: [M] forward scale of each output row
    int a_nseg;             // _H epilogues: plane segments of A and W per row (K = a_nseg x features), 2 or 3; 0 = not stated.  launch_big
                            // picks the 256 x 256 loop by it (gemm_bf16.hip)
    int out_nseg;           // EPI_SWIGLU_SPLIT_H: 3 = C [M, 3 N/2] = [f1 | f0 | f0], 2 = [f1 | f0] (down_proj weights without a g1 plane)
    SplitMap out_map;  // EPI_SWIGLU_SPLIT: plane of each output segment; C is [M, n_seg * N/2] bf16
    int m_fastest;     // tile order, chosen by launch_gemm_bf16: 1 = token tiles fastest (W far larger than the caches)
    int xcd_order;     // 1: the workgroups of one XCD (blockIdx % 8) work on a compact block of tiles, so that its L2 serves
                       // most operand rows (see gemm_bf16.hip); ignored with m_fastest
};

// y = A @ W^T with fused epilogue. Requirements: K % 64 == 0, N % 16 == 0 (N % 32 for SWIGLU),
// A/W/C 16-byte aligned.
int launch_gemm_bf16(GemmEpilogue epi, const GemmArgs& g, hipStream_t s);

// fp16-plane regime (encoder_f16_planes.hip), called by the layer loop of encoder.hip and by the test hooks of api.hip: norm + split of
// fp32 rows [T, K] (T >= 1) into [f1 | f0 | f0] / [f1 | f0] plane segments + inverse row scales, and the gate/up bound
// max_j |w_gate_j||w_up_j| (cmax is zeroed first); launch_gu_pair_samples: that product for ns evenly spaced single pairs (sr_model_finalize)
int launch_rows_split_f16(float* x, const float* embed, const int* tok, const float* w, bf16_t* xs, float* inv, int T, int K, float eps,
                          int nseg, const float* gu_cmax, float* act_sc, float* act_inv, hipStream_t s);
int launch_gu_cmax(const bf16_t* wgu_s, const float* wgu_i, int I, int K, int nseg, float* cmax, hipStream_t s);
int launch_gu_pair_samples(const bf16_t* wgu_s, const float* wgu_i, int I, int K, int nseg, int ns, float* p, hipStream_t s);

// bf16 regime and heads (encoder_kernels.hip), called by encoder.hip and by the test hooks of api.hip: RMSNorm with its optional
// embedding gather / pending bf16 residual / "residual add only" exit, the plan's launches (spans + cu_seqlens, then the per-token
// arrays), the dense head's two launches (stats: [T] float2 scratch) and the sparse head's finish; launch_rmsnorm_split: the RMSNorm of
// the bf16-plane fp32 regimes, output as plane segments [T, n_seg * H]
int launch_rmsnorm_split(float* x, const float* embed, const int* tok_id, const float* w, bf16_t* xs, int T, int H, float eps,
                         const SplitMap& map, hipStream_t s);
int launch_rmsnorm(float* x, const float* embed, const int* tok_id, const bf16_t* delta, const float* w, bf16_t* xn, float* xn_f32, int T,
                   int H, float eps, hipStream_t s);
int launch_plan_rows(const int64_t* mask, int B, int L, int mode, int* span_start, int* span_len, int* pool_start, int* row_len,
                     const int* row_shift, int* cu, hipStream_t s);
int launch_plan_tokens(const int64_t* ids, const int64_t* mask, int B, int L, const int* span_start, const int* cu, int* tok_id, int* pos,
                       unsigned char* key_valid, int* seq_of, int vocab, int mode, const int* row_shift, hipStream_t s);
int launch_dense_head(const float* x, const float* w, float2* stats, const int* cu, const int* pos, const int* pool_start, float* out,
                      int B, int T, int H, float eps, hipStream_t s);
int launch_sparse_finish(float* out, int64_t n, float scale, int round_bf16, hipStream_t s);

struct AttnArgs {
    const bf16_t* qkv;      // [T, (nh + 2*nkv) * hd] packed tokens, q heads then k heads then v heads
    bf16_t* out;            // [T, nh * hd]
    const int* cu_seqlens;  // [B + 1]
    const int* pos;         // [T] rope position of each token (apply_rope only)
    const unsigned char* key_valid;  // [T] 1 = attend to this token as a key
    const float* rope_cos;  // [max_pos, hd/2]
    const float* rope_sin;
    int B, nh, nkv, hd;
    float scale;            // 1/sqrt(hd)
    int apply_rope;         // 1: rotate q/k while loading (qkv holds raw projections); 0: qkv is already rotated
    int max_seqlen;         // longest sequence of the batch (host side); <= 256 enables the fast path.  0 = unknown is for apply_rope = 1
                            // only: max_seqlen = 0 with apply_rope = 0 does not occur for a batch with a non-empty sequence (every
                            // caller knows the lengths); there it means that all sequences are empty and nothing is launched
};
// Bidirectional (non-causal) GQA attention over packed var-len sequences.
int launch_attention(const AttnArgs& a, hipStream_t s);

// fp32 regime (the reference encodes dense queries without autocast, eval_dense.py:94-106): fp32 q/k/v (already
// rotated), fp32 scores, softmax and P.V; the output is written as split-bf16 plane segments for the o_proj GEMM.
struct AttnF32Args {
    const float* qkv;       // [T, (nh + 2*nkv) * hd]
    float* out_f32;         // if set: plain fp32 output [T, nh * hd] (the fp16-plane regime splits whole rows afterwards)
    bf16_t* out;            // else [T, n_seg * nh * hd] bf16 plane segments
    const int* cu_seqlens;  // [B + 1]
    const unsigned char* key_valid;  // [T]
    int B, nh, nkv, hd;
    float scale;
    int max_seqlen;         // longest sequence of the batch (grid sizing)
    SplitMap out_map;
    // set by launch_attention_f32: a kernel serves the sequences with only_gt < S and (only_le == 0 or S <= only_le), so the kernel
    // - and with it the bits - of a sequence depends on ITS length, never on what else shares the batch
    int only_le = 0, only_gt = 0;
    // launch plan of the <= 64-token kernel (attention_f32.hip): class_seqs[n - 1] = sequences of the batch with ceil(S / 16) = n key
    // blocks, n = 1..4, counted by a caller that holds cu_seqlens on the host (have_classes = 1: classes without a sequence are not
    // launched).  have_classes = 0: not known, one launch sized by max_seqlen serves every class.  nkb_only is set per launch
    // (0 = every class the launch has room for).
    int have_classes = 0, class_seqs[4] = {0, 0, 0, 0};
    int nkb_only = 0;
};
int launch_attention_f32(const AttnF32Args& a, hipStream_t s);
