"""GPU parity of the encoder's fp32 regime.

The reference encodes DENSE QUERIES without autocast (/root/reference/eval_dense.py:94-106, no autocast at :101-102)
and examples/quick_start.py runs both heads that way: every nn.Linear is an fp32 GEMM, SDPA runs on fp32 operands.
The HIP encoder reproduces that regime with split-bf16 planes of both GEMM operands (3 planes = the whole fp32
significand, 6 plane products, fp32 accumulation in the MFMA) and an fp32 attention kernel; which regime a call runs in
follows torch.autocast, as it does for the reference's nn.Linear.

Tolerance (floating point): relative L2 <= 2e-4 against the fp32 golden vectors of the reference's own head classes
(tests/golden/enc_*.npz; the bf16 regime sits at 3-6e-3).  Measured values are printed; with the default fp16 planes (and
with three bf16 planes) they are below 1e-6, i.e. the size of an fp32 summation-order change.
"""
import json
import os

import numpy as np
import pytest
import torch

from golden_weights import make_weights
from oracle import llama_bi as LB

pytestmark = [pytest.mark.gpu, pytest.mark.fp32_regime]

FP32_TOL = 2e-4          # the bar
FP32_TOL_3PLANES = 2e-5  # what three planes are expected to hold with a wide margin


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def _case(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name + ".npz"))
    cfg = json.loads(str(z["config_json"]))
    return z, cfg, make_weights(cfg, int(z["weight_seed"]))


def _t(z, side):
    return (torch.from_numpy(z[f"{side}:input_ids"]).cuda(), torch.from_numpy(z[f"{side}:attention_mask"]).cuda())


# ---------------------------------------------------------------- split-plane GEMM
def _planes(x, n):
    """fp32 tensor -> n bf16 planes (torch restatement of split_bf16x3, csrc/common.h)."""
    out, r = [], x.float()
    for _ in range(n):
        p = r.bfloat16()
        out.append(p)
        r = r - p.float()
    return out


@pytest.mark.parametrize("planes,tol", [(3, 5e-7), (2, 3e-5)])
def test_split_gemm_is_fp32_class(planes, tol):
    """A' = plane segments of A, W' of W (kernels.h SplitMap order) through sr_gemm_bf16 == A @ W^T in fp32 class."""
    from scaling_retriever_amd import _lib as L
    lib = L.load()
    g = torch.Generator(device="cuda").manual_seed(5)
    M, N, K = 700, 384, 1024
    A = torch.randn((M, K), device="cuda", generator=g) * 3.0
    W = torch.randn((N, K), device="cuda", generator=g) / K ** 0.5
    pa, pw = ([2, 0, 1, 1, 0, 0], [0, 2, 1, 0, 1, 0]) if planes == 3 else ([1, 0, 0], [0, 1, 0])
    ap, wp = _planes(A, planes), _planes(W, planes)
    A2 = torch.cat([ap[i] for i in pa], dim=1).contiguous()
    W2 = torch.cat([wp[i] for i in pw], dim=1).contiguous()
    C = torch.empty((M, N), dtype=torch.float32, device="cuda")
    L.check(lib.sr_gemm_bf16(A2.data_ptr(), W2.data_ptr(), M, N, K * len(pa), 4, C.data_ptr(), None, L.stream_ptr()))
    torch.cuda.synchronize()
    ref = A.double() @ W.double().T
    err = ((C.double() - ref).norm() / ref.norm()).item()
    err_fp32 = (((A @ W.T).double() - ref).norm() / ref.norm()).item()
    err_bf16 = (((A.bfloat16().float() @ W.bfloat16().float().T).double() - ref).norm() / ref.norm()).item()
    print(f"split GEMM ({planes} planes): rel err {err:.2e}; torch fp32 matmul {err_fp32:.2e}; bf16 inputs {err_bf16:.2e}")
    assert err < tol
    if planes == 3:
        assert err < 4 * err_fp32 + 1e-7      # the error class of an fp32 GEMM


def test_fp16_plane_gemm_has_the_error_of_an_fp32_gemm():
    """The default representation of the fp32 regime: rows scaled by a power of two, two fp16 planes (22 significand bits), three
    plane products, the MFMA's fp32 accumulation, inverse scales applied in the epilogue (sr_gemm_f16_scaled) - vs float64, next
    to torch's own fp32 matmul.  Includes outlier columns (x50) and rows of very different magnitude."""
    from scaling_retriever_amd import _lib as L
    lib = L.load()
    g = torch.Generator(device="cuda").manual_seed(9)
    M, N, K = 900, 640, 2048
    A = torch.randn((M, K), device="cuda", generator=g) * 3.0
    A[:, :5] *= 50.0
    A *= torch.exp(torch.empty((M, 1), device="cuda").uniform_(-6, 6, generator=g))
    W = torch.randn((N, K), device="cuda", generator=g) / K ** 0.5
    W *= torch.exp(torch.empty((N, 1), device="cuda").uniform_(-6, 6, generator=g))

    def planes(x):
        mx = x.abs().amax(1, keepdim=True)
        sc = torch.pow(2.0, 15 - torch.frexp(mx).exponent.float())            # row_scale_pow2 (csrc/common.h)
        xs = x * sc
        f0 = xs.half()
        f1 = (xs - f0.float()).half()
        return f0, f1, (1.0 / sc).reshape(-1).contiguous()
    a0, a1, ai = planes(A)
    w0, w1, wi = planes(W)
    A2 = torch.cat([a1, a0, a0], dim=1).contiguous()
    W2 = torch.cat([w0, w1, w0], dim=1).contiguous()
    C = torch.zeros((M, N), dtype=torch.float32, device="cuda")
    L.check(lib.sr_gemm_f16_scaled(A2.data_ptr(), W2.data_ptr(), M, N, 3 * K, ai.data_ptr(), wi.data_ptr(), C.data_ptr(), L.stream_ptr()))
    torch.cuda.synchronize()
    ref = A.double() @ W.double().T
    rowwise = lambda X: float(((X.double() - ref).norm(dim=1) / ref.norm(dim=1)).max())     # noqa: E731
    err, err_fp32 = rowwise(C), rowwise(A @ W.T)
    print(f"fp16-plane GEMM: worst row rel err {err:.2e}; torch fp32 matmul {err_fp32:.2e}")
    assert err < 2e-6 and err < 3 * err_fp32 + 2e-7


# ---------------------------------------------------------------- heads vs the fp32 golden
@pytest.mark.parametrize("planes", [16, 3])
@pytest.mark.parametrize("name", ["enc_tiny_a", "enc_hd64", "enc_hd128", "enc_toy_q", "enc_toy_d"])
@pytest.mark.parametrize("side", ["left", "right"])
def test_dense_fp32_matches_reference_fp32_golden(golden_dir, name, side, planes):
    from scaling_retriever_amd.modeling.llm_encoder import LlamaBiDense
    z, cfg, w = _case(golden_dir, name)
    model = LlamaBiDense.from_weights(cfg, w, fp32_planes=planes).to("cuda").eval()
    ids, mask = _t(z, side)
    assert model.base_model.resolve_precision() == "fp32"          # no autocast active: the reference's query regime
    with torch.no_grad():                                           # eval_dense.py:101
        out = model.query_encode(input_ids=ids, attention_mask=mask).cpu().numpy()
    e = rel(out, z[f"{side}:dense"])
    print(f"{name}/{side}/planes {planes}: fp32-regime dense rel L2 {e:.2e} (reference's own bf16-autocast: "
          f"{rel(z[f'{side}:dense_bf16autocast'], z[f'{side}:dense']):.2e})")
    assert e < FP32_TOL_3PLANES < FP32_TOL
    hs = model.base_model.last_hidden_state_packed().cpu().numpy()
    m = z[f"{side}:attention_mask"].astype(bool)
    if side == "left":                                              # packed tokens = exactly the unmasked positions
        assert rel(hs, z[f"{side}:last_hidden_state"][m]) < FP32_TOL_3PLANES


@pytest.mark.parametrize("planes", [16, 3])
@pytest.mark.parametrize("name", ["enc_tiny_a", "enc_hd64", "enc_hd128"])
@pytest.mark.parametrize("side", ["left", "right"])
def test_sparse_fp32_matches_reference_fp32_golden(golden_dir, name, side, planes):
    from scaling_retriever_amd.modeling.llm_encoder import LlamaBiSparse
    z, cfg, w = _case(golden_dir, name)
    model = LlamaBiSparse.from_weights(cfg, w, fp32_planes=planes).to("cuda").eval()
    ids, mask = _t(z, side)
    out = model.encode(input_ids=ids, attention_mask=mask).cpu().numpy()
    gold = z[f"{side}:sparse"]
    e = rel(out, gold)
    print(f"{name}/{side}/planes {planes}: fp32-regime sparse rel L2 {e:.2e}")
    assert e < FP32_TOL_3PLANES
    # the support (which terms are non-zero) must agree except where the max logit is within rounding of zero
    flip = (out > 0) != (gold > 0)
    assert np.all(np.maximum(out, gold)[flip] < 1e-5)


def test_two_planes_mode(golden_dir):
    from scaling_retriever_amd.modeling.llm_encoder import LlamaBiDense
    z, cfg, w = _case(golden_dir, "enc_hd64")
    model = LlamaBiDense.from_weights(cfg, w, fp32_planes=2).to("cuda").eval()
    ids, mask = _t(z, "left")
    e = rel(model.query_encode(input_ids=ids, attention_mask=mask).cpu().numpy(), z["left:dense"])
    print(f"2 planes / 3 products: rel L2 {e:.2e}")
    assert e < FP32_TOL


# ---------------------------------------------------------------- fused SwiGLU split, its fallback, and the unfused route
def _with_outlier_pair(w, s, j=7):
    """Layer 0: gate/up pair j scaled by s, its down_proj column by 1 / s^2, so that the hidden state keeps its range."""
    w = dict(w)
    for n in ("gate_proj", "up_proj"):
        a = w[f"model.layers.0.mlp.{n}.weight"].copy()
        a[j] *= np.float32(s)
        w[f"model.layers.0.mlp.{n}.weight"] = a
    d = w["model.layers.0.mlp.down_proj.weight"].copy()
    d[:, j] /= np.float32(s * s)
    w["model.layers.0.mlp.down_proj.weight"] = d
    return w


FUSED_VS_UNFUSED = 2.0


@pytest.mark.parametrize("s", [1, 32, 1024])
def test_fused_act_against_the_unfused_route_and_three_planes(golden_dir, s, monkeypatch):
    """enc_hd64 as it is (s = 1) and with one gate/up pair of layer 0 scaled by s = 32 / 1024: the fp32 regime's default route
    against the oracle, next to SR_FP32_FUSED_ACT=0 (fp32 SwiGLU output + row split in every layer) and fp32_planes = 3.

    The fused SwiGLU split scales a row by a bound B that one large pair sets for every row; its low plane's floor is 2^-39 B
    (tests/fp32_plane_cases.py), 2^-13 of the row's largest element at s = 1024.  sr_model_finalize therefore decides per layer
    (DESIGN 4.4): hidden max_j p_j < 2^16 median_j p_j keeps the fused route, else the layer runs unfused.  Required: which layers
    fell back; the default within FP32_TOL_3PLANES; and the default within FUSED_VS_UNFUSED = 2 x the error of the
    SR_FP32_FUSED_ACT=0 route on the same inputs.  The factor was measured once against the unfused route, not against the code
    under test: default / unfused on MI355X is 6.95e-07 / 6.94e-07 (s = 1), 6.31e-07 / 6.31e-07 (32), 6.99e-07 / 6.99e-07 (1024),
    three planes 6.2 - 6.8e-07 - all of it the fp32 oracle's own summation noise.  The ratio is 1.00; 2 leaves room for a
    power-of-two scale one step apart and nothing seen asks for more.  SR_FP32_FUSED_ACT=1 (fused in every layer, the behaviour
    before the rule) is printed for the record: 6.55e-07 at s = 32, 1.90e-04 at s = 1024 - what the rule avoids."""
    from scaling_retriever_amd.modeling.llm_encoder import LlamaBiDense
    z, cfg, w = _case(golden_dir, "enc_hd64")
    if s != 1:
        w = _with_outlier_pair(w, s)
    ids, mask = _t(z, "left")
    ref = LB.dense_encode(w, cfg, z["left:input_ids"], z["left:attention_mask"])
    monkeypatch.delenv("SR_FP32_FUSED_ACT", raising=False)
    model = LlamaBiDense.from_weights(cfg, w).to("cuda").eval()
    assert model.base_model.fused_act_layers() == [s == 1, True, True]
    e = {}
    e["default"] = rel(model.query_encode(input_ids=ids, attention_mask=mask).cpu().numpy(), ref)
    monkeypatch.setenv("SR_FP32_FUSED_ACT", "0")
    e["unfused"] = rel(model.query_encode(input_ids=ids, attention_mask=mask).cpu().numpy(), ref)
    monkeypatch.setenv("SR_FP32_FUSED_ACT", "1")
    e["fused everywhere"] = rel(model.query_encode(input_ids=ids, attention_mask=mask).cpu().numpy(), ref)
    monkeypatch.delenv("SR_FP32_FUSED_ACT", raising=False)
    three = LlamaBiDense.from_weights(cfg, w, fp32_planes=3).to("cuda").eval()
    assert three.base_model.fused_act_layers() == []
    e["3 planes"] = rel(three.query_encode(input_ids=ids, attention_mask=mask).cpu().numpy(), ref)
    print(f"enc_hd64, outlier factor {s}: rel L2 vs the oracle " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert e["default"] < FP32_TOL_3PLANES and e["unfused"] < FP32_TOL_3PLANES and e["3 planes"] < FP32_TOL_3PLANES
    assert e["default"] <= FUSED_VS_UNFUSED * e["unfused"]


# ---------------------------------------------------------------- the regime follows torch.autocast
def test_regime_follows_autocast(golden_dir):
    from scaling_retriever_amd import _lib
    from scaling_retriever_amd.modeling.llm_encoder import LlamaBiDense
    z, cfg, w = _case(golden_dir, "enc_hd64")
    ids, mask = _t(z, "left")
    auto = LlamaBiDense.from_weights(cfg, w).to("cuda").eval()
    bf16 = LlamaBiDense.from_weights(cfg, w, precision="bf16").to("cuda").eval()
    fp32 = LlamaBiDense.from_weights(cfg, w, precision="fp32").to("cuda").eval()
    with torch.autocast("cuda", dtype=torch.bfloat16):              # indexer.py:46-52
        assert auto.base_model.resolve_precision() == "bf16"
        a_doc = auto.doc_encode(input_ids=ids, attention_mask=mask)
        f_in_autocast = fp32.doc_encode(input_ids=ids, attention_mask=mask)     # forced regimes ignore the context
    a_query = auto.query_encode(input_ids=ids, attention_mask=mask)
    assert torch.equal(a_doc, bf16.doc_encode(input_ids=ids, attention_mask=mask))
    assert torch.equal(a_query, fp32.query_encode(input_ids=ids, attention_mask=mask))
    assert torch.equal(a_query, f_in_autocast)
    assert not torch.equal(a_doc, a_query)
    assert a_query.dtype == torch.float32 and a_doc.dtype == torch.float32
    with torch.autocast("cuda", dtype=torch.float16):
        with pytest.raises(NotImplementedError):
            auto.doc_encode(input_ids=ids, attention_mask=mask)
    none = LlamaBiDense.from_weights(cfg, w, fp32_planes=0).to("cuda").eval()
    with pytest.raises(_lib.SrHipError):
        none.query_encode(input_ids=ids, attention_mask=mask)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert torch.equal(none.doc_encode(input_ids=ids, attention_mask=mask), a_doc)


def test_eval_dense_query_vecs_run_in_fp32(golden_dir):
    """eval_dense.generate_query_vecs (the mirror of eval_dense.py:94-106) must hit the fp32 regime, store_embs the bf16 one."""
    import eval_dense
    from scaling_retriever_amd.modeling.llm_encoder import LlamaBiDense
    z, cfg, w = _case(golden_dir, "enc_hd64")
    model = LlamaBiDense.from_weights(cfg, w).to("cuda").eval()
    batch = {"input_ids": torch.from_numpy(z["left:input_ids"]), "attention_mask": torch.from_numpy(z["left:attention_mask"]),
             "ids": list(range(len(z["left:input_ids"])))}
    reps, qids = eval_dense.generate_query_vecs(model, [batch], "cuda")
    assert qids == batch["ids"]
    assert rel(reps.cpu().numpy(), z["left:dense"]) < FP32_TOL_3PLANES


# ---------------------------------------------------------------- fp32 attention kernel, longer and ragged sequences
@pytest.mark.parametrize("hd,heads,kv", [(64, 4, 2), (128, 2, 1), (64, 4, 1), (128, 4, 1)])
def test_fp32_regime_long_ragged_sequences(hd, heads, kv):
    """Sequences beyond one 64-key chunk (online softmax across chunks) and beyond one 16-row q block, right padding
    with masked keys inside the batch, vs the numpy oracle in fp32.  The 4:1 configurations run the kernels the product
    uses (fp32 MFMA up to 64 tokens, the grouped FMA kernel above: the batch crosses that border), the 2:1 ones the
    per-head FMA kernel."""
    from scaling_retriever_amd.modeling.llm_encoder import LlamaBiDense, LlamaBiSparse
    cfg = dict(vocab_size=320, hidden_size=heads * hd, intermediate_size=384, num_hidden_layers=2, num_attention_heads=heads,
               num_key_value_heads=kv, head_dim=hd, rms_norm_eps=1e-5, rope_theta=500000.0, tie_word_embeddings=False)
    w = make_weights(cfg, 11)
    rng = np.random.default_rng(3)
    lens = [1, 17, 64, 65, 130, 200]
    L = max(lens)
    for side in ("left", "right"):
        ids = rng.integers(0, cfg["vocab_size"], size=(len(lens), L))
        mask = np.zeros((len(lens), L), np.int64)
        for r, n in enumerate(lens):
            if side == "left":
                mask[r, L - n:] = 1
            else:
                mask[r, :n] = 1
        t_ids, t_mask = torch.from_numpy(ids).cuda(), torch.from_numpy(mask).cuda()
        d = LlamaBiDense.from_weights(cfg, w).to("cuda").encode(input_ids=t_ids, attention_mask=t_mask).cpu().numpy()
        s = LlamaBiSparse.from_weights(cfg, w).to("cuda").encode(input_ids=t_ids, attention_mask=t_mask).cpu().numpy()
        ed, es = rel(d, LB.dense_encode(w, cfg, ids, mask)), rel(s, LB.sparse_encode(w, cfg, ids, mask))
        print(f"hd {hd} {side}: dense {ed:.2e} sparse {es:.2e}")
        assert ed < FP32_TOL_3PLANES and es < FP32_TOL_3PLANES


def test_fp32_regime_reproducible_and_batch_invariant(golden_dir):
    from scaling_retriever_amd.modeling.llm_encoder import LlamaBiDense
    z, cfg, w = _case(golden_dir, "enc_hd64")
    model = LlamaBiDense.from_weights(cfg, w).to("cuda").eval()
    ids, mask = _t(z, "left")
    a = model.query_encode(input_ids=ids, attention_mask=mask)
    b = model.query_encode(input_ids=ids, attention_mask=mask)
    assert torch.equal(a, b)
    n = int(mask[3].sum())
    alone = model.query_encode(input_ids=ids[3:4, -n:].contiguous(), attention_mask=mask[3:4, -n:].contiguous())
    assert rel(alone.cpu().numpy(), a[3:4].cpu().numpy()) < 1e-5
