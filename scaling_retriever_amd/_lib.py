"""ctypes binding of libsr_hip.so (C ABI in include/sr_hip.h).

The product path has NO fallback: if the HIP library is missing or a call fails,
this module raises.  Build it with `python -c "import __graft_entry__ as g; g.build()"`
or `make -C scaling_retriever_amd/csrc`.
"""
import contextlib
import ctypes
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SR_HIP_LIB") or os.path.join(_HERE, "libsr_hip.so")     # SR_HIP_LIB: diagnostic builds (tools/micro)

SR_OK, SR_ERR_INVALID, SR_ERR_HIP, SR_ERR_NOMEM, SR_ERR_UNSUPPORTED = 0, 1, 2, 3, 4
SR_DTYPE_F32, SR_DTYPE_BF16, SR_DTYPE_F16 = 0, 1, 2
SR_FUSE_RRF, SR_FUSE_MINMAX = 0, 1              # sr_rank_fuse's methods
SR_MMR_SIM_IP, SR_MMR_SIM_COSINE = 0, 1         # sr_sparse_mmr's similarities
SR_EVAL_ORDER_SCORE, SR_EVAL_ORDER_LIST = 0, 1  # sr_eval_ranked's rankings

c_void_p, c_int, c_int32, c_int64, c_float, c_char_p = (ctypes.c_void_p, ctypes.c_int, ctypes.c_int32,
                                                         ctypes.c_int64, ctypes.c_float, ctypes.c_char_p)


class SrModelConfig(ctypes.Structure):
    _fields_ = [
        ("vocab_size", c_int32), ("hidden_size", c_int32), ("intermediate_size", c_int32), ("num_layers", c_int32),
        ("num_heads", c_int32), ("num_kv_heads", c_int32), ("head_dim", c_int32),
        ("rms_norm_eps", c_float), ("rope_theta", c_float), ("rope_llama3", c_int32),
        ("rope_factor", c_float), ("rope_low_freq_factor", c_float), ("rope_high_freq_factor", c_float),
        ("rope_original_max_pos", c_int32), ("tie_word_embeddings", c_int32), ("has_lm_head", c_int32),
        ("max_batch_tokens", c_int32), ("max_batch_seqs", c_int32), ("fp32_planes", c_int32),
        ("attention_bias", c_int32),      # 1: q / k / v projections carry a bias (Qwen2); ctypes zero-fills it when not given
    ]


# name -> (restype, argtypes); every function declared in include/sr_hip.h
SIGNATURES = {
    "sr_last_error": (c_char_p, []),
    "sr_version": (c_int, []),
    "sr_max_topk": (c_int, []),
    "sr_dense_index_create": (c_int, [ctypes.POINTER(c_void_p), c_int]),
    "sr_dense_index_add": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64]),
    "sr_dense_index_add_f16": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_int64]),
    "sr_dense_index_row_dtype": (c_int, [c_void_p]),
    "sr_dense_index_owned_bytes": (c_int, [c_void_p, ctypes.POINTER(c_int64)]),
    "sr_dense_index_ntotal": (c_int64, [c_void_p]),
    "sr_dense_search": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p]),
    "sr_dense_index_set_workspace_limit": (c_int, [c_void_p, c_int64]),
    "sr_dense_index_set_batch_invariant": (c_int, [c_void_p, c_int]),
    "sr_dense_score_pairs": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sr_dense_search_subset": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "sr_dense_index_id_end": (c_int64, [c_void_p]),
    "sr_doc_mask_from_list": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p]),
    "sr_doc_list_from_mask": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p]),
    "sr_dense_search_masked": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "sr_dense_search_grouped": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
                                        c_void_p]),
    "sr_dense_range_count": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, ctypes.POINTER(c_int64), c_void_p]),
    "sr_dense_range_fill": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "sr_dense_range_count_masked": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, ctypes.POINTER(c_int64),
                                            c_void_p]),
    "sr_dense_range_fill_masked": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64,
                                           c_void_p]),
    "sr_dense_range_count_grouped": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p,
                                             ctypes.POINTER(c_int64), c_void_p]),
    "sr_dense_range_fill_grouped": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p,
                                            c_void_p, c_int64, c_void_p]),
    "sr_doc_mask_remap": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p]),
    "sr_dense_index_set_precision": (c_int, [c_void_p, c_int]),
    "sr_dense_search_begin": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_int, c_void_p, c_void_p]),
    "sr_dense_search_finish": (c_int, [c_void_p, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sr_dense_index_filter_stats": (c_int, [c_void_p, ctypes.POINTER(c_int64), ctypes.POINTER(c_int64)]),
    "sr_dense_index_filter_query_stats": (c_int, [c_void_p, ctypes.POINTER(c_int64), ctypes.POINTER(c_int64)]),
    "sr_dense_index_destroy": (c_int, [c_void_p]),
    "sr_dense_index_profile": (c_int, [c_void_p, c_int]),
    "sr_dense_index_profile_read": (c_int, [c_void_p, ctypes.POINTER(c_int64), ctypes.POINTER(ctypes.c_double),
                                            ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    "sr_sparse_index_work_counters": (c_int, [c_void_p, c_int, ctypes.POINTER(ctypes.c_uint64)]),
    "sr_sparse_index_profile": (c_int, [c_void_p, c_int]),
    "sr_sparse_index_profile_read": (c_int, [c_void_p, ctypes.POINTER(c_int64), ctypes.POINTER(ctypes.c_double),
                                             ctypes.POINTER(ctypes.c_double)]),
    "sr_sparse_index_create": (c_int, [ctypes.POINTER(c_void_p), c_void_p, c_void_p, c_void_p, c_int64, c_int64,
                                       c_void_p]),
    "sr_sparse_search": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_float, c_int64, c_int64,
                                 c_void_p, c_void_p, c_void_p, c_void_p]),
    "sr_sparse_index_set_workspace_limit": (c_int, [c_void_p, c_int64]),
    "sr_sparse_score_pairs": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sr_sparse_search_subset": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_float, c_void_p, c_int64, c_int64,
                                        c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sr_sparse_search_masked": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_float, c_void_p, c_int64, c_int64,
                                        c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sr_sparse_search_grouped": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_float, c_void_p, c_int64, c_int64,
                                         c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sr_sparse_range_count": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, ctypes.POINTER(c_int64), c_void_p]),
    "sr_sparse_range_fill": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_void_p,
                                     c_void_p, c_int64, c_void_p]),
    "sr_sparse_range_count_masked": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p,
                                             ctypes.POINTER(c_int64), c_void_p]),
    "sr_sparse_range_fill_masked": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int64,
                                            c_int64, c_void_p, c_void_p, c_int64, c_void_p]),
    "sr_sparse_range_count_grouped": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_void_p,
                                              c_void_p, ctypes.POINTER(c_int64), c_void_p]),
    "sr_sparse_range_fill_grouped": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int64, c_void_p,
                                             c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_int64, c_void_p]),
    "sr_sparse_index_block_stats": (c_int, [c_void_p, ctypes.POINTER(c_int64), ctypes.POINTER(c_int64),
                                            ctypes.POINTER(c_int64)]),
    "sr_sparse_index_destroy": (c_int, [c_void_p]),
    "sr_sparse_index_cert_stats": (c_int, [c_void_p, ctypes.POINTER(c_int64)]),
    "sr_sparse_index_cert_debug": (c_int, [c_void_p, c_int, c_void_p, c_int64, c_void_p, c_int64,
                                           ctypes.POINTER(c_float), ctypes.POINTER(ctypes.c_int32)]),
    "sr_sparse_index_cert_readout": (c_int, [c_void_p, c_int, c_void_p, c_int64, ctypes.POINTER(c_int64)]),
    "sr_sparse_csr_expand_terms": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p]),
    "sr_sparse_csr_build": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int, c_void_p, c_void_p,
                                    c_void_p, c_void_p]),
    "sr_topk_merge": (c_int, [c_void_p, c_void_p, c_int, c_int64, c_int, c_float, c_void_p, c_void_p, c_void_p]),
    "sr_topk_replay": (c_int, [c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int, c_int, c_int, c_int64, c_int, c_int, c_int, c_float,
                               c_float, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sr_hybrid_union": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int64,
                                c_void_p, c_void_p, c_void_p, c_void_p, c_int64, ctypes.POINTER(c_int64), c_void_p]),
    "sr_hybrid_rank": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, c_int, c_void_p,
                               c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sr_rank_fuse": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int64, c_int64, c_int, ctypes.POINTER(c_float), c_float, c_int, c_void_p,
                             c_void_p, c_void_p, c_void_p, c_void_p]),
    "sr_eval_max_cuts": (c_int, []),
    "sr_eval_ranked": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int64,
                               c_void_p, c_void_p, c_void_p, ctypes.POINTER(c_int32), c_int, c_int, c_int64, c_void_p, c_void_p, c_void_p,
                               c_void_p, c_void_p]),
    "sr_eval_randomization": (c_int, [c_void_p, c_int, c_int64, c_int64, ctypes.c_uint64, c_void_p, c_void_p, c_void_p]),
    "sr_mmr_max_candidates": (c_int, []),
    "sr_dense_mmr": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int, c_float, c_void_p, c_void_p, c_void_p, c_void_p,
                             c_void_p, c_void_p]),
    "sr_sparse_mmr": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int, c_float, c_int,
                              c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sr_prf_max_entries": (c_int, []),
    "sr_sparse_feedback": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_void_p,
                                   c_int64, c_int, c_int, c_float, c_float, c_float, c_int64, c_void_p, c_void_p, c_void_p, c_int64,
                                   ctypes.POINTER(c_int64), c_void_p]),
    "sr_dense_feedback": (c_int, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int, c_int, c_float, c_float, c_float, c_void_p,
                                  c_void_p]),
    "sr_topk_collapse": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int, c_void_p, c_int64, c_int, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_void_p]),
    "sr_group_members_count": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64,
                                       c_void_p, c_void_p, ctypes.POINTER(c_int64), c_void_p]),
    "sr_group_members_fill": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int64,
                                      c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "sr_segment_topm": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_float, c_float, c_void_p, c_void_p, c_void_p,
                                c_void_p]),
    "sr_model_create": (c_int, [ctypes.POINTER(c_void_p), ctypes.POINTER(SrModelConfig)]),
    "sr_model_set_weight": (c_int, [c_void_p, c_char_p, c_void_p, c_int, c_int64, c_int64, c_void_p]),
    "sr_model_finalize": (c_int, [c_void_p]),
    "sr_model_readout": (c_int, [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_int64, ctypes.POINTER(c_int64), ctypes.POINTER(c_int64),
                                 ctypes.POINTER(c_int64)]),
    "sr_model_weight_segments": (c_int, [c_void_p, ctypes.POINTER(ctypes.c_int32), c_int64, ctypes.POINTER(c_int64)]),
    "sr_model_fused_act_layers": (c_int, [c_void_p, ctypes.POINTER(ctypes.c_int32), c_int64, ctypes.POINTER(c_int64)]),
    "sr_encode_dense": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "sr_encode_sparse": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "sr_encode_dense_fp32": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "sr_encode_sparse_fp32": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p]),
    "sr_encode_both": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "sr_encode_rows": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "sr_model_last_hidden": (c_int, [c_void_p, c_void_p, c_int64, ctypes.POINTER(c_int64), c_void_p]),
    "sr_model_destroy": (c_int, [c_void_p]),
    "sr_lora_merge": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int32, c_float, c_void_p]),
    "sr_run_writer_mapped_rounds": (c_int64, []),
    "sr_write_run_json": (c_int, [c_char_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                  c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int32, ctypes.POINTER(c_int64)]),
    "sr_write_run_json_part": (c_int, [c_char_p, c_int32, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64,
                                       c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int32, ctypes.POINTER(c_int64)]),
    "sr_gemm_bf16": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p]),
    "sr_gemm_f16_scaled": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sr_rows_split_f16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                                  c_void_p, c_void_p, c_void_p]),
    "sr_gu_cmax_f16": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p]),
    "sr_gemm_f16_planes": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_void_p]),
    "sr_rmsnorm_bf16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int32, c_int32, c_void_p]),
    "sr_dense_head_pool": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int32, c_int32, c_int32, c_void_p, c_void_p,
                                   c_void_p]),
    "sr_sparse_finish": (c_int, [c_void_p, c_int64, c_float, c_int32, c_void_p]),
    "sr_encode_plan": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                               c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, ctypes.POINTER(c_int64), c_void_p]),
    "sr_split_bf16": (c_int, [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "sr_gemm_qkv_rope": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_int32, c_int32, c_void_p]),
    "sr_gemm_qkv_rope_bias": (c_int, [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_int32, c_int32, c_void_p, c_int32, c_void_p]),
    "sr_attention_varlen": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32,
                                    c_int32, c_int32, c_int32, c_void_p]),
    "sr_attention_varlen_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_int32,
                                        c_int32, c_int32, c_void_p]),
    "sr_sparse_compact": (c_int, [c_void_p, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int64,
                                  ctypes.POINTER(c_int64), c_void_p]),
    "sr_sparse_compact_topm": (c_int, [c_void_p, c_int64, c_int64, c_int64, c_void_p, c_void_p, c_void_p, c_int64,
                                       ctypes.POINTER(c_int64), c_void_p]),
    "sr_token_counts_max_len": (c_int, []),
    "sr_token_counts": (c_int, [c_void_p, c_void_p, c_int64, c_int64, ctypes.POINTER(c_int32), c_int, c_int64, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_int64, ctypes.POINTER(c_int64), c_void_p]),
    "sr_bm25_weights": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_void_p, c_int64, c_void_p, c_float, c_float, c_float,
                                c_void_p, c_void_p]),
}

_lib = None
_lock = threading.Lock()


class SrHipError(RuntimeError):
    pass


def _bind(path):
    if not os.path.exists(path):
        raise SrHipError(
            f"{path} not found: the HIP extension is not built. There is no CPU fallback; "
            "run `make -C scaling_retriever_amd/csrc` (needs hipcc, targets gfx950).")
    # torch first: it ships its own libamdhip64; were the system runtime pulled in by our DT_NEEDED before torch's, the
    # process would hold two HIP runtimes and the second would find "no ROCm-capable device"
    import torch  # noqa: F401
    lib = ctypes.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    return lib


def load():
    """Load libsr_hip.so and bind every entry point.  Raises if the library is missing."""
    global _lib
    with _lock:
        if _lib is None:
            _lib = _bind(LIB_PATH)
        return _lib


@contextlib.contextmanager
def library(path):
    """Development aid (same-process A/B of two builds, tools/quick_query_encode.py --ab-lib): inside the block load() returns the
    build at `path`; an object created there keeps that build (a backbone holds the handle it was created with), and the
    process-wide library is restored on exit."""
    global _lib
    other = _bind(os.path.abspath(path))
    with _lock:
        keep, _lib = _lib, other
    try:
        yield other
    finally:
        with _lock:
            _lib = keep


def check(rc, what=""):
    """Map a C-ABI status to the Python exception the reference would raise for the same condition."""
    if rc == SR_OK:
        return
    msg = load().sr_last_error().decode("utf-8", "replace")
    if rc == SR_ERR_INVALID:
        raise ValueError(f"{what}: {msg}" if what else msg)
    if rc == SR_ERR_NOMEM:
        raise MemoryError(f"{what}: {msg}" if what else msg)
    raise SrHipError(f"{what}: [{rc}] {msg}" if what else f"[{rc}] {msg}")


def stream_ptr():
    """hipStream_t of torch's current stream (so C-ABI work is ordered with torch ops)."""
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def require_gpu():
    import torch
    if not torch.cuda.is_available():
        raise SrHipError("no ROCm device visible: scaling_retriever_amd runs its hot path on MI355X only "
                         "(there is no CPU fallback)")
