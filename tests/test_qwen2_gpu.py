"""GPU: the Qwen2 family - Qwen2BiDense / Qwen2BiSparse / Qwen2BiHybrid
(/root/reference/scaling_retriever/modeling/llm_encoder.py:204-209,528-533 over modeling/bidrectional_qwen2.py:68-101): a Llama
layer whose q_proj / k_proj / v_proj carry a bias, added in the QKV + RoPE epilogues of csrc/gemm_bf16.hip.  Goldens from the
reference's own heads (tests/golden/make_golden_qwen2.py), production widths against the numpy oracle with a bias hook
(tests/qwen2_common.py), the per-kernel entry point against plain torch, and the Python surface."""
import ctypes
import os

import numpy as np
import pytest
import torch

from golden_weights import make_weights
from oracle import llama_bi as LB
from qwen2_common import CASES, BiasHooks, load_case, random_biases, rel

pytestmark = pytest.mark.gpu

FP32_TOL = 2e-5          # the project's fp32-regime bar


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _encode(model, ids, mask):
    return model.doc_encode(input_ids=_t(ids), attention_mask=_t(mask)).cpu().numpy()


def _bf16_bar():
    """max(1.5e-2, 2.5 r): r = the largest relative L2 between the reference's own autocast and fp32 outputs over the new cases."""
    r = max(float(load_case(n)[0]["r_autocast"]) for n in CASES)
    return max(1.5e-2, 2.5 * r), r


@pytest.mark.parametrize("planes", [16, 3])
@pytest.mark.parametrize("name", CASES)
def test_golden_parity_fp32_regime(name, planes):
    from scaling_retriever_amd.modeling.llm_encoder import Qwen2BiDense, Qwen2BiSparse
    z, cfg, w = load_case(name)
    for cls, key in ((Qwen2BiDense, "dense"), (Qwen2BiSparse, "sparse")):
        model = cls.from_weights(cfg, w, precision="fp32", fp32_planes=planes).to("cuda").eval()
        for side in ("left", "right"):
            out = _encode(model, z[f"{side}:input_ids"], z[f"{side}:attention_mask"])
            e = rel(out, z[f"{side}:{key}"])
            print(f"qwen2 fp32 regime {name} planes={planes} {key} {side}: rel L2 {e:.3e}")
            assert e <= FP32_TOL, (name, planes, key, side, e)


@pytest.mark.parametrize("name", CASES)
def test_golden_parity_bf16_regime(name):
    from scaling_retriever_amd.modeling.llm_encoder import Qwen2BiDense, Qwen2BiSparse
    z, cfg, w = load_case(name)
    bar, r = _bf16_bar()
    for cls, key in ((Qwen2BiDense, "dense"), (Qwen2BiSparse, "sparse")):
        model = cls.from_weights(cfg, w, precision="bf16").to("cuda").eval()
        for side in ("left", "right"):
            out = _encode(model, z[f"{side}:input_ids"], z[f"{side}:attention_mask"])
            e = rel(out, z[f"{side}:{key}"])
            print(f"qwen2 bf16 regime {name} {key} {side}: rel L2 {e:.3e} (reference autocast r {r:.3e}, bar {bar:.3e})")
            assert e <= bar, (name, key, side, e, bar)


def test_dropped_or_misplaced_bias_is_caught():
    from scaling_retriever_amd.modeling.llm_encoder import Qwen2BiDense
    z, cfg, w = load_case("enc_qwen2_hd64")
    ids, mask, gold = z["left:input_ids"], z["left:attention_mask"], z["left:dense"]
    zeroed = {k: (np.zeros_like(v) if k.endswith(".bias") else v) for k, v in w.items()}
    out0 = _encode(Qwen2BiDense.from_weights(cfg, zeroed, precision="fp32").to("cuda").eval(), ids, mask)
    assert rel(out0, gold) > 0.1
    # q / k / v segments permuted: k and v have the same length and swap; the q bias goes in rolled by half a head
    perm = dict(w)
    for i in range(cfg["num_hidden_layers"]):
        p = f"model.layers.{i}.self_attn."
        perm[p + "k_proj.bias"], perm[p + "v_proj.bias"] = w[p + "v_proj.bias"], w[p + "k_proj.bias"]
    outp = _encode(Qwen2BiDense.from_weights(cfg, perm, precision="fp32").to("cuda").eval(), ids, mask)
    assert rel(outp, gold) > 100 * FP32_TOL
    roll = dict(w)
    for i in range(cfg["num_hidden_layers"]):
        p = f"model.layers.{i}.self_attn.q_proj.bias"
        roll[p] = np.roll(w[p], 32)
    outr = _encode(Qwen2BiDense.from_weights(cfg, roll, precision="fp32").to("cuda").eval(), ids, mask)
    assert rel(outr, gold) > 100 * FP32_TOL
    good = _encode(Qwen2BiDense.from_weights(cfg, w, precision="fp32").to("cuda").eval(), ids, mask)
    assert rel(good, gold) <= FP32_TOL


# ---- production width: the 256^2 four- and eight-wave loops and their staged epilogues ---------------------------------
WIDTH = {
    "1.5b": {"hidden_size": 1536, "intermediate_size": 8960, "num_attention_heads": 12, "num_key_value_heads": 2, "head_dim": 128,
             "num_hidden_layers": 2, "vocab_size": 4096, "rms_norm_eps": 1e-6, "rope_theta": 1000000.0,
             "tie_word_embeddings": True, "max_position_embeddings": 512, "model_type": "qwen2"},
    "0.5b": {"hidden_size": 896, "intermediate_size": 4864, "num_attention_heads": 14, "num_key_value_heads": 2, "head_dim": 64,
             "num_hidden_layers": 2, "vocab_size": 4096, "rms_norm_eps": 1e-6, "rope_theta": 1000000.0,
             "tie_word_embeddings": True, "max_position_embeddings": 512, "model_type": "qwen2"},
}


def _wide_batch(cfg, n=128, lo=1, hi=192, seed=11):
    rng = np.random.default_rng(seed)
    lens = rng.integers(lo, hi + 1, size=n)
    lens[0], lens[1] = hi, lo
    ids = rng.integers(3, cfg["vocab_size"], size=(n, hi)).astype(np.int64)
    mask = np.zeros((n, hi), dtype=np.int64)
    for i, l in enumerate(lens):
        mask[i, hi - l:] = 1
    ids[mask == 0] = 0
    return ids, mask


@pytest.mark.parametrize("size", ["1.5b", "0.5b"])
def test_production_width_against_oracle_and_across_tile_plans(size, monkeypatch):
    from scaling_retriever_amd.modeling.llm_encoder import Qwen2BiDense
    cfg = WIDTH[size]
    w = make_weights(cfg, 4321, embed_std=0.05)
    w.update(random_biases(cfg, 99))
    ids, mask = _wide_batch(cfg)
    ref = LB.dense_encode(w, cfg, ids, mask, BiasHooks(w))
    emu = rel(LB.dense_encode(w, cfg, ids, mask, BiasHooks(w, bf16=True)), ref)
    nobias = rel(LB.dense_encode(w, cfg, ids, mask), ref)
    assert nobias > 0.1, nobias                                    # the biases matter at this width too
    t_ids, t_mask = _t(ids), _t(mask)
    for prec in ("fp32", "bf16"):
        model = Qwen2BiDense.from_weights(cfg, w, precision=prec).to("cuda").eval()
        want = model.doc_encode(input_ids=t_ids, attention_mask=t_mask).clone()
        e = rel(want.cpu().numpy(), ref)
        bar = FP32_TOL if prec == "fp32" else 3.0 * emu           # bf16: the rule of tests/test_encoder_depth_gpu.py
        print(f"qwen2 width {size} {prec}: rel L2 {e:.3e} (bar {bar:.3e}, oracle bf16 emulation {emu:.3e})")
        assert e <= bar, (size, prec, e, bar)
        # every tile plan adds the same bias: same bits as the default
        for var, val in (("SR_GEMM_BIG", "8w"), ("SR_GEMM_BIG", "4w"), ("SR_GEMM_TILE", "128"), ("SR_GEMM_TILE", "256")):
            monkeypatch.setenv(var, val)
            got = model.doc_encode(input_ids=t_ids, attention_mask=t_mask)
            monkeypatch.delenv(var)
            assert torch.equal(got, want), (size, prec, var, val)
        # a handful of tokens runs the single-wave streaming tiles (16 / 32 / 64 token rows); SR_GEMM_SKINNY=0 sends the same rows
        # through the 128-wide tiles: the same bits, and the oracle's values
        for rows in (slice(1, 2), slice(1, 3), slice(1, 4)):          # 1, 1 + l2, 1 + l2 + l3 tokens
            sm_ids, sm_mask = t_ids[rows, -24:].contiguous(), (t_mask[rows, -24:]).contiguous()
            small = model.doc_encode(input_ids=sm_ids, attention_mask=sm_mask).clone()
            monkeypatch.setenv("SR_GEMM_SKINNY", "0")
            got = model.doc_encode(input_ids=sm_ids, attention_mask=sm_mask)
            monkeypatch.delenv("SR_GEMM_SKINNY")
            assert torch.equal(got, small), (size, prec, rows)
            sref = LB.dense_encode(w, cfg, sm_ids.cpu().numpy(), sm_mask.cpu().numpy(), BiasHooks(w))
            assert rel(small.cpu().numpy(), sref) <= (FP32_TOL if prec == "fp32" else 3.0 * emu), (size, prec, rows)
        del model
        torch.cuda.empty_cache()


# ---- per-kernel: sr_gemm_qkv_rope_bias against plain torch ------------------------------------------------------------------
def _rope_tables(hd, max_pos, theta=1000000.0):
    inv = 1.0 / (theta ** (torch.arange(0, hd, 2, dtype=torch.float64) / hd))
    ang = torch.arange(max_pos, dtype=torch.float32)[:, None] * inv.float()[None, :]
    return torch.cos(ang).cuda().contiguous(), torch.sin(ang).cuda().contiguous()


def _rotate(x, pos, cos, sin, hd):
    c = torch.cat([cos[pos.long()], cos[pos.long()]], -1)[:, None, :]
    s = torch.cat([sin[pos.long()], sin[pos.long()]], -1)[:, None, :]
    rot = torch.cat([-x[..., hd // 2:], x[..., :hd // 2]], -1)
    return x * c + rot * s


@pytest.mark.parametrize("fp32_out", [0, 1])
@pytest.mark.parametrize("nh,nkv,hd,K", [(14, 2, 64, 896), (12, 2, 128, 512)])
@pytest.mark.parametrize("M", [1, 77, 256, 3497])
def test_qkv_gemm_with_bias_and_fused_rope(M, nh, nkv, hd, K, fp32_out):
    from scaling_retriever_amd import _lib as L
    lib = L.load()
    g = torch.Generator(device="cuda").manual_seed(nh * hd + M)
    N = (nh + 2 * nkv) * hd
    A = torch.randn((M, K), device="cuda", generator=g).bfloat16()
    W = (torch.randn((N, K), device="cuda", generator=g) / K ** 0.5).bfloat16()
    bias = torch.randn((N,), device="cuda", generator=g)
    pos = torch.randint(0, 500, (M,), device="cuda", generator=g).int()
    cos, sin = _rope_tables(hd, 512)
    out = torch.empty((M, N), dtype=torch.float32 if fp32_out else torch.bfloat16, device="cuda")
    L.check(lib.sr_gemm_qkv_rope_bias(A.data_ptr(), W.data_ptr(), M, N, K, out.data_ptr(), pos.data_ptr(), cos.data_ptr(),
                                      sin.data_ptr(), (nh + nkv) * hd, hd, bias.data_ptr(), fp32_out, L.stream_ptr()),
            "sr_gemm_qkv_rope_bias")
    torch.cuda.synchronize()
    y = A.float() @ W.float().T + bias
    qk = _rotate(y[:, :(nh + nkv) * hd].reshape(M, nh + nkv, hd), pos, cos, sin, hd).reshape(M, -1)
    ref = torch.cat([qk, y[:, (nh + nkv) * hd:]], dim=1)
    # the tolerance of the sr_gemm_qkv_rope test in tests/test_rope_attention_gpu.py
    torch.testing.assert_close(out.float(), ref, rtol=1e-2, atol=1e-2)
    assert (out.float() - ref).abs().max() <= 0.01 * ref.abs().max() + 1e-3
    # the bias is there (a zero bias would be ~1 off), on every segment
    nob = y - bias
    assert (out.float()[:, (nh + nkv) * hd:] - nob[:, (nh + nkv) * hd:]).abs().max() > 0.5
    if not fp32_out:
        # without a bias: the bits of sr_gemm_qkv_rope
        a = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")
        b = torch.empty((M, N), dtype=torch.bfloat16, device="cuda")
        L.check(lib.sr_gemm_qkv_rope_bias(A.data_ptr(), W.data_ptr(), M, N, K, a.data_ptr(), pos.data_ptr(), cos.data_ptr(),
                                          sin.data_ptr(), (nh + nkv) * hd, hd, None, 0, L.stream_ptr()), "sr_gemm_qkv_rope_bias")
        L.check(lib.sr_gemm_qkv_rope(A.data_ptr(), W.data_ptr(), M, N, K, b.data_ptr(), pos.data_ptr(), cos.data_ptr(),
                                     sin.data_ptr(), (nh + nkv) * hd, hd, L.stream_ptr()), "sr_gemm_qkv_rope")
        torch.cuda.synchronize()
        assert torch.equal(a, b)


# ---- surface ---------------------------------------------------------------------------------------------------------------
def test_hybrid_and_encode_batches_bit_for_bit():
    from scaling_retriever_amd.modeling.llm_encoder import Qwen2BiDense, Qwen2BiHybrid, Qwen2BiSparse
    z, cfg, w = load_case("enc_qwen2_hd128")
    ids, mask = _t(z["left:input_ids"]), _t(z["left:attention_mask"])
    for prec in ("bf16", "fp32"):
        hy = Qwen2BiHybrid.from_weights(cfg, w, precision=prec).to("cuda").eval()
        de = Qwen2BiDense.from_weights(cfg, w, precision=prec).to("cuda").eval()
        sp = Qwen2BiSparse.from_weights(cfg, w, precision=prec).to("cuda").eval()
        s, d = hy.encode(input_ids=ids, attention_mask=mask)
        assert torch.equal(d, de.encode(input_ids=ids, attention_mask=mask)), prec
        assert torch.equal(s, sp.encode(input_ids=ids, attention_mask=mask)), prec
        # a second, narrower left-padded batch (the collators pad left): the last 66 columns of the three long rows.  Both batches'
        # longest rows are above 64 tokens: at head_dim 128 the bf16 attention picks its kernel by the call's longest sequence
        # (csrc/attention.hip: chunked online softmax above 64), for Llama as for Qwen2, and the bits follow the kernel
        b2 = {"input_ids": _t(z["left:input_ids"][[0, 2, 3], -66:]), "attention_mask": _t(z["left:attention_mask"][[0, 2, 3], -66:])}
        b1 = {"input_ids": ids, "attention_mask": mask}
        both = de.encode_batches([b1, b2])
        assert torch.equal(both, torch.cat([de.encode(**b1), de.encode(**b2)])), prec
        del hy, de, sp
    # head_dim 64, short rows, all three heads
    z, cfg, w = load_case("enc_qwen2_hd64")
    b1 = {"input_ids": _t(z["left:input_ids"]), "attention_mask": _t(z["left:attention_mask"])}
    b2 = {"input_ids": _t(z["left:input_ids"][1:4, -12:]), "attention_mask": _t(z["left:attention_mask"][1:4, -12:])}
    for prec in ("bf16", "fp32"):
        for cls in (Qwen2BiDense, Qwen2BiSparse, Qwen2BiHybrid):
            m = cls.from_weights(cfg, w, precision=prec).to("cuda").eval()
            both, one, two = m.encode_batches([b1, b2]), m.encode(**b1), m.encode(**b2)
            if isinstance(both, tuple):
                for h in range(2):
                    assert torch.equal(both[h], torch.cat([one[h], two[h]])), (prec, cls.__name__, h)
            else:
                assert torch.equal(both, torch.cat([one, two])), (prec, cls.__name__)


def test_store_embs_index_search_round_trip(tmp_path):
    from scaling_retriever_amd.indexer import DenseFlatIndexer, store_embs
    from scaling_retriever_amd.modeling.llm_encoder import Qwen2BiDense
    from scaling_retriever_amd.utils.utils import obtain_doc_vec_dir_files
    z, cfg, w = load_case("enc_qwen2_hd64")
    model = Qwen2BiDense.from_weights(cfg, w).to("cuda").eval()
    rng = np.random.default_rng(5)
    n, L = 300, 20
    lens = rng.integers(4, L + 1, size=n)
    ids = rng.integers(0, cfg["vocab_size"] - 1, size=(n, L)).astype(np.int64)
    mask = np.zeros((n, L), np.int64)
    for i, l in enumerate(lens):
        mask[i, L - l:] = 1

    class Loader:
        batch_size = 32

        def __len__(self):
            return (n + 31) // 32

        def __iter__(self):
            for b0 in range(0, n, 32):
                yield {"input_ids": torch.from_numpy(ids[b0:b0 + 32]), "attention_mask": torch.from_numpy(mask[b0:b0 + 32]),
                       "ids": list(range(b0, min(n, b0 + 32)))}
    d = str(tmp_path / "embs")
    store_embs(model, Loader(), 0, d, "cuda", chunk_size=128)
    vec_files, id_files = obtain_doc_vec_dir_files(d)
    index = DenseFlatIndexer()
    index.init_index(model.hidden_size)
    for vf, idf in zip(vec_files, id_files):
        index.index_data(np.load(vf), np.load(idf).tolist())
    pick = rng.choice(n, size=24, replace=False)
    q = model.query_encode(input_ids=_t(ids[pick]), attention_mask=_t(mask[pick]))        # fp32 regime, as eval_dense.py:94-106
    top_ids, scores = index.search_knn(q, 5)
    assert [int(t[0]) for t in top_ids] == [int(p) for p in pick]


def test_bias_names_need_attention_bias_and_finalize_needs_the_biases():
    from scaling_retriever_amd import _lib as L
    lib = L.load()
    base = dict(vocab_size=64, hidden_size=128, intermediate_size=128, num_layers=1, num_heads=2, num_kv_heads=1, head_dim=64,
                rms_norm_eps=1e-6, rope_theta=1e6, max_batch_tokens=256, max_batch_seqs=8, fp32_planes=0)
    b = torch.zeros(128, device="cuda")
    for ab in (0, 1):
        cfg = L.SrModelConfig(attention_bias=ab, **base)
        h = ctypes.c_void_p()
        L.check(lib.sr_model_create(ctypes.byref(h), ctypes.byref(cfg)), "sr_model_create")
        try:
            rc = lib.sr_model_set_weight(h, b"model.layers.0.self_attn.q_proj.bias", b.data_ptr(), L.SR_DTYPE_F32, 128, 1, L.stream_ptr())
            msg = lib.sr_last_error().decode()
            if ab == 0:
                assert rc == L.SR_ERR_INVALID and "unknown tensor name 'model.layers.0.self_attn.q_proj.bias'" in msg, (rc, msg)
                continue
            assert rc == L.SR_OK, msg
            rc = lib.sr_model_set_weight(h, b"model.layers.0.self_attn.k_proj.bias", b.data_ptr(), L.SR_DTYPE_F32, 128, 1, L.stream_ptr())
            assert rc == L.SR_ERR_INVALID and "expected [64, 1]" in lib.sr_last_error().decode()
            shapes = {"model.embed_tokens.weight": (64, 128), "model.norm.weight": (128, 1),
                      "model.layers.0.self_attn.q_proj.weight": (128, 128), "model.layers.0.self_attn.k_proj.weight": (64, 128),
                      "model.layers.0.self_attn.v_proj.weight": (64, 128), "model.layers.0.self_attn.o_proj.weight": (128, 128),
                      "model.layers.0.mlp.gate_proj.weight": (128, 128), "model.layers.0.mlp.up_proj.weight": (128, 128),
                      "model.layers.0.mlp.down_proj.weight": (128, 128), "model.layers.0.input_layernorm.weight": (128, 1),
                      "model.layers.0.post_attention_layernorm.weight": (128, 1)}
            for nm, (r, c) in shapes.items():
                t = torch.ones((r, c), device="cuda")
                L.check(lib.sr_model_set_weight(h, nm.encode(), t.data_ptr(), L.SR_DTYPE_F32, r, c, L.stream_ptr()), nm)
            torch.cuda.synchronize()
            rc = lib.sr_model_finalize(h)
            msg = lib.sr_last_error().decode()
            assert rc == L.SR_ERR_INVALID and "layer 0 is missing self_attn.{q,k,v}_proj.bias" in msg, (rc, msg)
        finally:
            lib.sr_model_destroy(h)
