// LlamaBiDense / LlamaBiSparse encode on gfx950: packing plan, the layer loop of each precision regime and the pooling heads.
// Model handle and weights: model_weights.hip; small kernels: encoder_kernels.hip, encoder_f16_planes.hip; GEMMs: gemm_bf16.hip;
// attention: attention.hip, attention_f32.hip.
//
// Reference semantics reproduced (file:line into HansiZeng/scaling-retriever):
//  * backbone   LlamaBiModel over HF LlamaModel.forward, bidirectional mask on padded
//               KEYS only, position_ids = arange(L)     modeling/bidirectional_llama.py:67-188
//  * dense head per-token L2 normalise, mean of the LAST `len` positions (literal
//               `[-length:]` slice, so left padding is assumed)  modeling/llm_encoder.py:424-443
//  * sparse head log(1 + relu(max_L(logits * H^-0.25 + (1-mask) * -1e6)))
//                                                           modeling/llm_encoder.py:186-196
//  * precision  bf16 GEMM inputs / fp32 accumulate, fp32 residual stream, norms, rope
//               tables, softmax and heads - the torch.autocast(bf16) regime of
//               indexer.py:46-52,255-256 (fp32 master weights are rounded to bf16 once).
//
// Packing: a row keeps the contiguous span of positions it needs - the keys (mask == 1)
// and, for the dense head, the last `len` positions - so a left-padded batch (the
// reference's eval setting) is computed with ZERO pad tokens, while right-padded or
// holed masks stay literal (pad query rows are computed, masked as keys).
#include "encoder_model.h"
#include <math.h>

// one encode call: what the plan found out about the batch, handed to every layer
struct Pass {
    sr_model* m;
    hipStream_t s;
    int B, T;                // sequences, packed tokens
    int max_len;             // longest packed sequence
    int attn_class[4];       // fp32 attention's launch plan: sequences of at most 64 tokens by key-block count ceil(S / 16) (attention_f32.hip)
    bool fused_on, fused_all;   // fp16 planes: dev switch SR_FP32_FUSED_ACT, see model_forward
};

// fp32-regime workspace: allocated by the first fp32 call; a failed allocation frees all of it, so that a later call can try again
static int ensure_fp32_workspace(sr_model* m) {
    if (m->xs) return SR_OK;
    const sr_model_config& c = m->cfg;
    SR_REQUIRE(c.fp32_planes > 0, "encode(fp32): the model was created with fp32_planes = 0 (bf16 regime only)");
    const int64_t Tm = m->Tm, nsg = split_map_a(c.fp32_planes).n_seg;
    const ModelDims& d = m->d;
    DeviceArena& mem = m->mem_fp32;
    auto allocate = [&]() -> int {
        SR_TRY(mem.alloc(m->xs, Tm * d.H * nsg, true));
        SR_TRY(mem.alloc(m->qkv_f, Tm * d.n_qkv, true));
        SR_TRY(mem.alloc(m->attn_s, Tm * d.nq * nsg, true));
        SR_TRY(mem.alloc(m->act_s, Tm * d.I * nsg, true));
        if (c.fp32_planes != SR_FP32_PLANES_F16) return SR_OK;
        SR_TRY(mem.alloc(m->attn_f, Tm * d.nq, true));
        SR_TRY(mem.alloc(m->act_f, Tm * d.I, true));
        SR_TRY(mem.alloc(m->xs_i, Tm, true));
        SR_TRY(mem.alloc(m->attn_i, Tm, true));
        SR_TRY(mem.alloc(m->act_i, Tm, true));
        SR_TRY(mem.alloc(m->act_sc, Tm, true));
        return SR_OK;
    };
    if (allocate() != SR_OK) {
        mem.release();
        sr_set_error("encode(fp32): hipMalloc of the fp32-regime workspace failed (%lld tokens)", (long long)Tm);
        return SR_ERR_NOMEM;
    }
    return SR_OK;
}

// ---- argument builders ----------------------------------------------------------------------------------------
// C = A @ W^T; the call sites that need more (rope, bias, scales, segment counts, sequence ids) set it afterwards
static GemmArgs gemm(const bf16_t* A, const bf16_t* W, int M, int N, int K, void* C) {
    GemmArgs g{};
    g.A = A; g.W = W; g.M = M; g.N = N; g.K = K; g.C = C;
    return g;
}
// fp16 planes: A and W hold nseg segments of K features per row, with the inverse row scales a_inv / w_inv
static GemmArgs gemm_f16(const bf16_t* A, const float* a_inv, const bf16_t* W, const float* w_inv, int nseg, int M, int N, int K, void* C) {
    GemmArgs g = gemm(A, W, M, N, nseg * K, C);
    g.a_nseg = nseg; g.a_scale = a_inv; g.w_scale = w_inv;
    return g;
}
// QKV epilogues: rotate the q and k heads by the token's position, after adding the bias (null: none)
static void set_rope(GemmArgs& g, const sr_model* m, const float* bias) {
    g.pos = m->pos; g.rope_cos = m->rope_cos; g.rope_sin = m->rope_sin; g.n_rope = m->d.nq + m->d.nkv; g.head_dim = m->d.hd;
    g.bias = bias;
}
// fp32 attention over the rotated q/k/v in qkv_f; the caller sets the output (out_f32, or out + out_map)
static AttnF32Args attn_f32_args(const Pass& p) {
    const sr_model* m = p.m;
    AttnF32Args a{};
    a.qkv = m->qkv_f; a.cu_seqlens = m->cu; a.key_valid = m->key_valid;
    a.B = p.B; a.nh = m->cfg.num_heads; a.nkv = m->cfg.num_kv_heads; a.hd = m->d.hd;
    a.scale = 1.0f / sqrtf((float)m->d.hd); a.max_seqlen = p.max_len;
    a.have_classes = 1;
    for (int n = 0; n < 4; ++n) a.class_seqs[n] = p.attn_class[n];
    return a;
}
// fp16 planes: rows of fp32 src [T, K] -> nseg plane segments + inverse row scales; with w the RMSNorm of the row first
static int split_rows(const Pass& p, float* src, const float* w, bf16_t* dst, float* inv, int K, int nseg) {
    return launch_rows_split_f16(src, nullptr, nullptr, w, dst, inv, p.T, K, p.m->cfg.rms_norm_eps, nseg, nullptr, nullptr, nullptr, p.s);
}

// ---- one layer in each regime: norm -> QKV + RoPE -> attention -> o_proj -> norm -> gate-up + SwiGLU -> down_proj ------------
// bf16 regime.  o_proj and down_proj return bf16 (delta), as an nn.Linear does under autocast; the NEXT norm kernel adds it to the
// fp32 residual stream x, so the last down_proj output is still pending when the layer returns (model_forward folds the final one)
static int layer_bf16(const Pass& p, int li) {
    sr_model* m = p.m;
    const ModelDims& d = m->d;
    const LayerW& l = m->layers[li];
    const float eps = m->cfg.rms_norm_eps;
    const int T = p.T;
    hipStream_t s = p.s;
    // input_layernorm: fused with the embedding gather in the first layer, with the previous layer's down_proj output in the others
    if (li == 0) SR_TRY(launch_rmsnorm(m->x, m->embed, m->tok_id, nullptr, l.ln1, m->xn, nullptr, T, d.H, eps, s));
    else SR_TRY(launch_rmsnorm(m->x, nullptr, nullptr, m->delta, l.ln1, m->xn, nullptr, T, d.H, eps, s));
    GemmArgs g = gemm(m->xn, l.wqkv, T, d.n_qkv, d.H, m->qkv);
    set_rope(g, m, l.bqkv_r);
    SR_TRY(launch_gemm_bf16(EPI_QKV_ROPE, g, s));
    AttnArgs a{};
    a.qkv = m->qkv; a.out = m->attn; a.cu_seqlens = m->cu; a.pos = m->pos; a.key_valid = m->key_valid;
    a.rope_cos = m->rope_cos; a.rope_sin = m->rope_sin; a.B = p.B; a.nh = m->cfg.num_heads; a.nkv = m->cfg.num_kv_heads;
    a.hd = d.hd; a.scale = 1.0f / sqrtf((float)d.hd);
    a.apply_rope = 0; a.max_seqlen = p.max_len;
    SR_TRY(launch_attention(a, s));
    SR_TRY(launch_gemm_bf16(EPI_STORE_BF16, gemm(m->attn, l.wo, T, d.H, d.nq, m->delta), s));
    // x += o_proj output, then post_attention_layernorm
    SR_TRY(launch_rmsnorm(m->x, nullptr, nullptr, m->delta, l.ln2, m->xn, nullptr, T, d.H, eps, s));
    SR_TRY(launch_gemm_bf16(EPI_SWIGLU, gemm(m->xn, l.wgu, T, 2 * d.I, d.H, m->act), s));
    return launch_gemm_bf16(EPI_STORE_BF16, gemm(m->act, l.wdown, T, d.H, d.I, m->delta), s);
}

// fp32 regime on bf16 planes (fp32_planes 2 or 3): every producer writes its output as the plane segments of split_map_a, o_proj and
// down_proj add straight into x
static int layer_f32_planes(const Pass& p, int li) {
    sr_model* m = p.m;
    const ModelDims& d = m->d;
    const LayerW& l = m->layers[li];
    const float eps = m->cfg.rms_norm_eps;
    const SplitMap ma = split_map_a(m->cfg.fp32_planes);
    const int T = p.T, nsg = ma.n_seg;
    hipStream_t s = p.s;
    // input_layernorm (the embedding gather is fused into the first one)
    SR_TRY(launch_rmsnorm_split(m->x, li == 0 ? m->embed : nullptr, li == 0 ? m->tok_id : nullptr, l.ln1, m->xs, T, d.H, eps, ma, s));
    GemmArgs g = gemm(m->xs, l.wqkv_s, T, d.n_qkv, nsg * d.H, m->qkv_f);
    set_rope(g, m, l.bqkv);
    SR_TRY(launch_gemm_bf16(EPI_QKV_ROPE_F32, g, s));
    AttnF32Args a = attn_f32_args(p);
    a.out = m->attn_s; a.out_map = ma;
    SR_TRY(launch_attention_f32(a, s));
    SR_TRY(launch_gemm_bf16(EPI_RESID_F32, gemm(m->attn_s, l.wo_s, T, d.H, nsg * d.nq, m->x), s));
    SR_TRY(launch_rmsnorm_split(m->x, nullptr, nullptr, l.ln2, m->xs, T, d.H, eps, ma, s));
    g = gemm(m->xs, l.wgu_s, T, 2 * d.I, nsg * d.H, m->act_s);
    g.out_map = ma;
    SR_TRY(launch_gemm_bf16(EPI_SWIGLU_SPLIT, g, s));
    return launch_gemm_bf16(EPI_RESID_F32, gemm(m->act_s, l.wdown_s, T, d.H, nsg * d.I, m->x), s);
}

// fp32 regime on fp16 planes (fp32_planes 16): every GEMM input is split by ONE kernel that sees whole rows (norm + split, or split of
// an fp32 buffer), because the power-of-two scale is per row; 3 plane products per GEMM, 2 where the weights' g1 plane is zero (the
// split writes the segment count of its consumer's weights, K' = nseg K)
static int layer_f16_planes(const Pass& p, int li) {
    sr_model* m = p.m;
    const ModelDims& d = m->d;
    const LayerW& l = m->layers[li];
    const float eps = m->cfg.rms_norm_eps;
    const int T = p.T;
    hipStream_t s = p.s;
    // input_layernorm (the embedding gather is fused into the first one)
    SR_TRY(launch_rows_split_f16(m->x, li == 0 ? m->embed : nullptr, li == 0 ? m->tok_id : nullptr, l.ln1, m->xs, m->xs_i, T, d.H, eps,
                                 l.qkv_seg, nullptr, nullptr, nullptr, s));
    GemmArgs g = gemm_f16(m->xs, m->xs_i, l.wqkv_s, l.wqkv_i, l.qkv_seg, T, d.n_qkv, d.H, m->qkv_f);
    set_rope(g, m, l.bqkv);
    SR_TRY(launch_gemm_bf16(EPI_QKV_ROPE_F32_H, g, s));
    AttnF32Args a = attn_f32_args(p);
    a.out_f32 = m->attn_f;
    SR_TRY(launch_attention_f32(a, s));
    SR_TRY(split_rows(p, m->attn_f, nullptr, m->attn_s, m->attn_i, d.nq, l.o_seg));
    SR_TRY(launch_gemm_bf16(EPI_RESID_F32_H, gemm_f16(m->attn_s, m->attn_i, l.wo_s, l.wo_i, l.o_seg, T, d.H, d.nq, m->x), s));
    if (p.fused_on && (l.fused_act || p.fused_all)) {       // per layer: sr_model_finalize
        // the norm kernel also fixes the scale of the row's SwiGLU output (a rigorous bound, no overflow), so the
        // gate-up GEMM writes the down_proj's fp16 plane segments itself: no fp32 intermediate, no split pass
        SR_TRY(launch_rows_split_f16(m->x, nullptr, nullptr, l.ln2, m->xs, m->xs_i, T, d.H, eps, l.gu_seg, m->gu_cmax + li, m->act_sc,
                                     m->act_i, s));
        g = gemm_f16(m->xs, m->xs_i, l.wgu_s, l.wgu_i, l.gu_seg, T, 2 * d.I, d.H, m->act_s);
        g.out_scale = m->act_sc; g.out_nseg = l.down_seg;
        SR_TRY(launch_gemm_bf16(EPI_SWIGLU_SPLIT_H, g, s));
    } else {
        SR_TRY(split_rows(p, m->x, l.ln2, m->xs, m->xs_i, d.H, l.gu_seg));
        SR_TRY(launch_gemm_bf16(EPI_SWIGLU_F32_H, gemm_f16(m->xs, m->xs_i, l.wgu_s, l.wgu_i, l.gu_seg, T, 2 * d.I, d.H, m->act_f), s));
        SR_TRY(split_rows(p, m->act_f, nullptr, m->act_s, m->act_i, d.I, l.down_seg));
    }
    return launch_gemm_bf16(EPI_RESID_F32_H, gemm_f16(m->act_s, m->act_i, l.wdown_s, l.wdown_i, l.down_seg, T, d.H, d.I, m->x), s);
}

// ---- forward: validate, plan, layers ------------------------------------------------------------------------------
// the packing plan: spans and cu_seqlens on the device, the lengths on the host (one sync), then the per-token arrays
static int plan_batch(sr_model* m, const int64_t* d_ids, const int64_t* d_mask, int B, int L, int mode, const int32_t* d_shift, Pass& p) {
    hipStream_t s = p.s;
    SR_TRY(launch_plan_rows(d_mask, B, L, mode, m->span_start, m->span_len, m->pool_start, m->row_len, d_shift, m->cu, s));
    SR_CHECK_HIP(hipMemcpyAsync(m->h_cu, m->cu, (size_t)(B + 1) * 4, hipMemcpyDeviceToHost, s));
    SR_CHECK_HIP(hipStreamSynchronize(s));
    p.B = B;
    p.T = m->h_cu[B];
    p.max_len = 0;
    // a row whose attention_mask is all zero packs to zero tokens: every kernel skips it and both heads return the
    // zero vector for it (the reference's sparse head gives exactly that; its dense head would average garbage)
    for (int n = 0; n < 4; ++n) p.attn_class[n] = 0;
    for (int b = 0; b < B; ++b) {
        const int len = m->h_cu[b + 1] - m->h_cu[b];
        p.max_len = len > p.max_len ? len : p.max_len;
        if (len >= 1 && len <= 64) ++p.attn_class[(len - 1) >> 4];
    }
    SR_REQUIRE(p.T <= m->Tm, "encode: batch packs to %d tokens, workspace holds %d (raise max_batch_tokens or split the batch)", p.T, m->Tm);
    m->last_T = p.T;
    if (p.T == 0) return SR_OK;
    return launch_plan_tokens(d_ids, d_mask, B, L, m->span_start, m->cu, m->tok_id, m->pos, m->key_valid, m->seq_of, m->d.V, mode, d_shift, s);
}

static int model_forward(sr_model* m, const int64_t* d_ids, const int64_t* d_mask, int B, int L, int mode, int prec, const int32_t* d_shift,
                         Pass& p) {
    const sr_model_config& c = m->cfg;
    SR_REQUIRE(m->finalized, "encode: sr_model_finalize was not called");
    SR_REQUIRE(B >= 1 && L >= 1, "encode: bad batch shape [%d, %d]", B, L);
    SR_REQUIRE(B <= m->Bm, "encode: batch of %d sequences exceeds max_batch_seqs %d", B, m->Bm);
    SR_REQUIRE(L <= m->max_pos, "encode: sequence length %d exceeds %d", L, m->max_pos);
    SR_REQUIRE(d_ids && d_mask, "encode: null input");
    if (prec == PREC_FP32) SR_TRY(ensure_fp32_workspace(m));
    SR_TRY(plan_batch(m, d_ids, d_mask, B, L, mode, d_shift, p));
    if (p.T == 0) return SR_OK;
    const bool f16p = prec == PREC_FP32 && c.fp32_planes == SR_FP32_PLANES_F16;
    if (f16p) {
        // dev switch SR_FP32_FUSED_ACT=0: SwiGLU output as fp32 + a separate row-split pass (A/B, and the reference of the test)
        // (= 1: the fused route in every layer, whatever sr_model_finalize decided - to measure what the fallback rule avoids)
        const char* env_fa = sr_dev_getenv("SR_FP32_FUSED_ACT");
        p.fused_on = !(env_fa && *env_fa == '0');
        p.fused_all = env_fa && *env_fa == '1';
    }
    for (int li = 0; li < c.num_layers; ++li)
        SR_TRY(prec == PREC_BF16 ? layer_bf16(p, li) : (f16p ? layer_f16_planes(p, li) : layer_f32_planes(p, li)));
    // bf16 regime: fold the last down_proj output into the residual stream so that the heads see the complete hidden state
    if (prec == PREC_BF16)
        SR_TRY(launch_rmsnorm(m->x, nullptr, nullptr, m->delta, nullptr, nullptr, nullptr, p.T, m->d.H, c.rms_norm_eps, p.s));
    return SR_OK;
}

static int head_dense(const Pass& p, int prec, float* d_out) {
    sr_model* m = p.m;
    const int H = m->d.H;
    if (p.T == 0) {
        SR_CHECK_HIP(hipMemsetAsync(d_out, 0, (size_t)p.B * H * 4, p.s));
        return SR_OK;
    }
    // a [T] float2 scratch: xn (bf16 [Tm, H]) is free after the last layer in the bf16 regime, xs in the fp32 regime
    float2* stats = reinterpret_cast<float2*>(prec == PREC_FP32 ? (void*)m->xs : (void*)m->xn);
    return launch_dense_head(m->x, m->norm_w, stats, m->cu, m->pos, m->pool_start, d_out, p.B, p.T, H, m->cfg.rms_norm_eps, p.s);
}

static int head_sparse(const Pass& p, int prec, float* d_out) {
    sr_model* m = p.m;
    const int H = m->d.H, V = m->d.V, T = p.T;
    const float eps = m->cfg.rms_norm_eps;
    hipStream_t s = p.s;
    SR_CHECK_HIP(hipMemsetAsync(d_out, 0, (size_t)p.B * V * 4, s));
    if (T == 0) return SR_OK;       // log(1 + relu(max over no tokens)) = 0
    // final norm -> GEMM input of the regime
    GemmArgs g;
    GemmEpilogue epi = EPI_SEGMAX;
    if (prec == PREC_FP32 && m->cfg.fp32_planes == SR_FP32_PLANES_F16) {
        SR_TRY(split_rows(p, m->x, m->norm_w, m->xs, m->xs_i, H, m->lm_head_seg));
        g = gemm_f16(m->xs, m->xs_i, m->lm_head_s, m->lm_head_i, m->lm_head_seg, T, V, H, d_out);
        epi = EPI_SEGMAX_H;
    } else if (prec == PREC_FP32) {
        const SplitMap ma = split_map_a(m->cfg.fp32_planes);
        SR_TRY(launch_rmsnorm_split(m->x, nullptr, nullptr, m->norm_w, m->xs, T, H, eps, ma, s));
        g = gemm(m->xs, m->lm_head_s, T, V, ma.n_seg * H, d_out);
    } else {
        SR_TRY(launch_rmsnorm(m->x, nullptr, nullptr, nullptr, m->norm_w, m->xn, nullptr, T, H, eps, s));
        g = gemm(m->xn, m->lm_head, T, V, H, d_out);
    }
    // rows with seq_of == -2 (mask == 0 inside the span) are skipped by the segmented max
    g.seq_of = m->seq_of; g.out_ld = V;
    SR_TRY(launch_gemm_bf16(epi, g, s));
    // under autocast the lm_head output is bf16 (rounded before the fp32 upcast, llm_encoder.py:187-188); in fp32 it is not
    return launch_sparse_finish(d_out, (int64_t)p.B * V, powf((float)H, -0.25f), prec == PREC_FP32 ? 0 : 1, s);
}

// mode 0: dense head, 1: sparse head, 2: both from ONE backbone pass (the hybrid model)
static int encode_any(sr_model* m, const int64_t* d_input_ids, const int64_t* d_attention_mask, int32_t B, int32_t L, int mode,
                      int prec, float* d_dense, float* d_sparse, hipStream_t s, const int32_t* d_shift = nullptr) {
    std::lock_guard<std::mutex> lock(m->mu);
    StreamOrder::Scope in_order(m->order, s);
    Pass p{};
    p.m = m; p.s = s; p.B = B;
    SR_TRY(model_forward(m, d_input_ids, d_attention_mask, B, L, mode, prec, d_shift, p));
    if (mode != 1) SR_TRY(head_dense(p, prec, d_dense));     // first: its scratch is the sparse head's GEMM input
    if (mode != 0) SR_TRY(head_sparse(p, prec, d_sparse));
    return SR_OK;
}

extern "C" int sr_encode_dense(sr_model* m, const int64_t* d_input_ids, const int64_t* d_attention_mask, int32_t B, int32_t L,
                               float* d_out, sr_stream stream) {
    SR_REQUIRE(m && d_out, "sr_encode_dense: null argument");
    return encode_any(m, d_input_ids, d_attention_mask, B, L, 0, PREC_BF16, d_out, nullptr, (hipStream_t)stream);
}

extern "C" int sr_encode_dense_fp32(sr_model* m, const int64_t* d_input_ids, const int64_t* d_attention_mask, int32_t B, int32_t L,
                                    float* d_out, sr_stream stream) {
    SR_REQUIRE(m && d_out, "sr_encode_dense_fp32: null argument");
    return encode_any(m, d_input_ids, d_attention_mask, B, L, 0, PREC_FP32, d_out, nullptr, (hipStream_t)stream);
}

extern "C" int sr_encode_sparse(sr_model* m, const int64_t* d_input_ids, const int64_t* d_attention_mask, int32_t B, int32_t L,
                                float* d_out, sr_stream stream) {
    SR_REQUIRE(m && d_out, "sr_encode_sparse: null argument");
    SR_REQUIRE(m->cfg.has_lm_head, "sr_encode_sparse: model was created without an lm_head (LlamaBiModel)");
    return encode_any(m, d_input_ids, d_attention_mask, B, L, 1, PREC_BF16, nullptr, d_out, (hipStream_t)stream);
}

extern "C" int sr_encode_sparse_fp32(sr_model* m, const int64_t* d_input_ids, const int64_t* d_attention_mask, int32_t B, int32_t L,
                                     float* d_out, sr_stream stream) {
    SR_REQUIRE(m && d_out, "sr_encode_sparse_fp32: null argument");
    SR_REQUIRE(m->cfg.has_lm_head, "sr_encode_sparse_fp32: model was created without an lm_head (LlamaBiModel)");
    return encode_any(m, d_input_ids, d_attention_mask, B, L, 1, PREC_FP32, nullptr, d_out, (hipStream_t)stream);
}

extern "C" int sr_encode_both(sr_model* m, const int64_t* d_input_ids, const int64_t* d_attention_mask, int32_t B, int32_t L,
                              int32_t fp32, float* d_out_sparse, float* d_out_dense, sr_stream stream) {
    SR_REQUIRE(m && d_out_sparse && d_out_dense, "sr_encode_both: null argument");
    SR_REQUIRE(m->cfg.has_lm_head, "sr_encode_both: model was created without an lm_head (LlamaBiModel)");
    return encode_any(m, d_input_ids, d_attention_mask, B, L, 2, fp32 ? PREC_FP32 : PREC_BF16, d_out_dense, d_out_sparse,
                      (hipStream_t)stream);
}

// Rows of SEVERAL left-padded batches in one call (the drop-in drivers hand the encoder eval_batch_size rows at a time,
// eval_dense.py:94-106 / indexer.py:382-403; 128 queries are ~1 100 tokens - far too few rows for 256-row GEMM tiles): the caller
// lays the batches into one [B, L] matrix (L = the widest batch, narrower batches get extra left padding) and passes, per row, how far
// it moved right.  Positions are counted from there, so every row is computed with the position_ids it had in its own batch and its
// output is bit-identical to encoding that batch alone (the kernels do not depend on batch composition).
extern "C" int sr_encode_rows(sr_model* m, const int64_t* d_input_ids, const int64_t* d_attention_mask, int32_t B, int32_t L,
                              const int32_t* d_row_shift, int32_t mode, int32_t fp32, float* d_out_sparse, float* d_out_dense,
                              sr_stream stream) {
    SR_REQUIRE(m, "sr_encode_rows: null model");
    SR_REQUIRE(mode >= 0 && mode <= 2, "sr_encode_rows: mode %d (0 dense, 1 sparse, 2 both)", mode);
    SR_REQUIRE(mode == 1 || d_out_dense, "sr_encode_rows: null dense output");
    SR_REQUIRE(mode == 0 || d_out_sparse, "sr_encode_rows: null sparse output");
    SR_REQUIRE(mode == 0 || m->cfg.has_lm_head, "sr_encode_rows: model was created without an lm_head (LlamaBiModel)");
    return encode_any(m, d_input_ids, d_attention_mask, B, L, mode, fp32 ? PREC_FP32 : PREC_BF16, d_out_dense, d_out_sparse,
                      (hipStream_t)stream, d_row_shift);
}

extern "C" int sr_model_last_hidden(sr_model* m, float* d_out, int64_t capacity_rows, int64_t* n_tokens, sr_stream stream) {
    SR_REQUIRE(m && d_out && n_tokens, "sr_model_last_hidden: null argument");
    hipStream_t s = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(m->mu);
    StreamOrder::Scope in_order(m->order, s);
    const int T = m->last_T;
    *n_tokens = T;
    SR_REQUIRE(capacity_rows >= T, "sr_model_last_hidden: capacity %lld < %d tokens", (long long)capacity_rows, T);
    if (T == 0) return SR_OK;
    SR_TRY(launch_rmsnorm(m->x, (const float*)nullptr,
                       (const int*)nullptr, (const bf16_t*)nullptr, m->norm_w, (bf16_t*)nullptr, d_out, T, m->cfg.hidden_size, m->cfg.rms_norm_eps, s));
    return SR_OK;
}
