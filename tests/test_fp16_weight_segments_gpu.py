"""fp32 regime on fp16 planes: weight matrices whose low plane g1 is all zero run on 2 K segments instead of 3.

sr_model_finalize re-packs such a matrix from [g0 | g1 | g0] to [g0 | g0] and the activations feeding its GEMM are split to
[f1 | f0]: the dropped product f0 . g1 only added exact zeros, so the outputs must be bit-identical (torch.equal) to a model
forced to 3 segments (dev switch SR_F16_WEIGHT_SEGS=3) on the same weights.  bf16-valued weights always qualify: 8 significand
bits fit the fp16 plane g0 of a power-of-two scaled row, and a value too small for g0 leaves a remainder below half of fp16's
smallest subnormal, which g1 rounds to zero as well.  fp32-valued weights keep 3 segments.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from golden_weights import make_weights
from oracle import llama_bi as LB

pytestmark = [pytest.mark.gpu, pytest.mark.fp32_regime]

CFG_1B_2L = dict(vocab_size=2048, hidden_size=2048, intermediate_size=8192, num_hidden_layers=2, num_attention_heads=32,
                 num_key_value_heads=8, head_dim=64, rms_norm_eps=1e-5, rope_theta=500000.0, tie_word_embeddings=False)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def bf16_valued(w):
    """The weights rounded to bf16, kept as fp32 arrays (a bf16 checkpoint promoted to fp32)."""
    return {k: torch.from_numpy(v).bfloat16().float().numpy() for k, v in w.items()}


def golden_case(golden_dir, name):
    z = np.load(os.path.join(golden_dir, name + ".npz"))
    cfg = json.loads(str(z["config_json"]))
    return z, cfg, make_weights(cfg, int(z["weight_seed"]))


def build(cls, cfg, w, monkeypatch, force3=False):
    with monkeypatch.context() as mp:
        if force3:                      # read by sr_model_finalize, inside .to()
            mp.setenv("SR_DEV_SWITCHES", "1")
            mp.setenv("SR_F16_WEIGHT_SEGS", "3")
        return cls.from_weights(cfg, w).to("cuda").eval()


def batch(cfg, lens, side, seed=0):
    rng = np.random.default_rng(seed)
    L = max(lens)
    ids = rng.integers(0, cfg["vocab_size"], size=(len(lens), L))
    mask = np.zeros((len(lens), L), np.int64)
    for r, n in enumerate(lens):
        if side == "left":
            mask[r, L - n:] = 1
        else:
            mask[r, :n] = 1
    return ids, mask


def encode(model, ids, mask):
    with torch.no_grad():
        return model.encode(input_ids=torch.from_numpy(ids).cuda(), attention_mask=torch.from_numpy(mask).cuda())


def n_matrices(cfg, sparse):
    return 4 * cfg["num_hidden_layers"] + (1 if sparse else 0)


@pytest.mark.parametrize("name", ["enc_tiny_a", "enc_hd64", "enc_hd128"])
def test_golden_cases_rounded_to_bf16(golden_dir, name, monkeypatch):
    from scaling_retriever_amd.modeling.llm_encoder import LlamaBiDense, LlamaBiSparse
    z, cfg, w = golden_case(golden_dir, name)
    w = bf16_valued(w)
    for cls, sparse in ((LlamaBiDense, False), (LlamaBiSparse, True)):
        two = build(cls, cfg, w, monkeypatch)
        three = build(cls, cfg, w, monkeypatch, force3=True)
        assert two.base_model.weight_segments() == [2] * n_matrices(cfg, sparse)
        assert three.base_model.weight_segments() == [3] * n_matrices(cfg, sparse)
        for side in ("left", "right"):
            ids, mask = z[f"{side}:input_ids"], z[f"{side}:attention_mask"]
            a, b = encode(two, ids, mask), encode(three, ids, mask)
            assert torch.equal(a, b), f"{name}/{side}/{cls.__name__}"
            ref = (LB.sparse_encode if sparse else LB.dense_encode)(w, cfg, ids, mask)
            e = rel(a.cpu().numpy(), ref)
            print(f"{name}/{side}/{cls.__name__}: 2 segments vs oracle rel L2 {e:.2e}")
            assert e < 2e-5


def test_fp32_weights_keep_three_segments(golden_dir):
    from scaling_retriever_amd.modeling.llm_encoder import LlamaBiSparse
    _, cfg, w = golden_case(golden_dir, "enc_hd64")
    model = LlamaBiSparse.from_weights(cfg, w).to("cuda").eval()
    assert model.base_model.weight_segments() == [3] * n_matrices(cfg, True)


@pytest.fixture(scope="module")
def wide_weights():
    return bf16_valued(make_weights(CFG_1B_2L, 21))


@pytest.mark.parametrize("side", ["left", "right"])
def test_1b_widths_bit_identical(wide_weights, side, monkeypatch):
    """1B widths, 2 layers: lengths 1-64 (2 080 tokens: 256^2 tiles plus a ragged tail), a skinny batch (M <= 64) and a
    single token, dense and sparse heads, vs the forced-3-segment model; the skinny batch also vs the oracle."""
    from scaling_retriever_amd.modeling.llm_encoder import LlamaBiDense, LlamaBiSparse
    cfg, w = CFG_1B_2L, wide_weights
    cases = [list(range(1, 65)), [5, 17, 33, 2], [1]]
    for cls, sparse in ((LlamaBiDense, False), (LlamaBiSparse, True)):
        two = build(cls, cfg, w, monkeypatch)
        three = build(cls, cfg, w, monkeypatch, force3=True)
        assert two.base_model.weight_segments() == [2] * n_matrices(cfg, sparse)
        for lens in cases:
            ids, mask = batch(cfg, lens, side, seed=len(lens))
            a, b = encode(two, ids, mask), encode(three, ids, mask)
            assert torch.equal(a, b), f"{cls.__name__}/{side}/{len(lens)} rows"
        ids, mask = batch(cfg, cases[1], side, seed=4)
        ref = (LB.sparse_encode if sparse else LB.dense_encode)(w, cfg, ids, mask)
        e = rel(encode(two, ids, mask).cpu().numpy(), ref)
        print(f"1B widths/{side}/{cls.__name__}: 2 segments vs oracle rel L2 {e:.2e}")
        assert e < 2e-5
        del two, three
        torch.cuda.empty_cache()


def test_one_fp32_entry_falls_back_for_its_matrix_only(wide_weights, monkeypatch):
    """An entry with more significand bits than fp16 holds gives its matrix (layer 1 down_proj) a nonzero g1 plane: that
    matrix alone keeps 3 segments, and the outputs still equal the forced-3 run."""
    from scaling_retriever_amd.modeling.llm_encoder import LlamaBiSparse
    cfg = CFG_1B_2L
    w = dict(wide_weights)
    d = w["model.layers.1.mlp.down_proj.weight"].copy()
    d[7, 100] = d[7, 100] * np.float32(1.0 + 2.0 ** -20)
    w["model.layers.1.mlp.down_proj.weight"] = d
    two = build(LlamaBiSparse, cfg, w, monkeypatch)
    three = build(LlamaBiSparse, cfg, w, monkeypatch, force3=True)
    expect = [2] * n_matrices(cfg, True)
    expect[4 * 1 + 3] = 3
    assert two.base_model.weight_segments() == expect
    for lens in (list(range(1, 65)), [9, 3]):
        ids, mask = batch(cfg, lens, "left", seed=7)
        assert torch.equal(encode(two, ids, mask), encode(three, ids, mask))


def test_set_weight_after_finalize_is_rejected(golden_dir):
    from scaling_retriever_amd import _lib
    from scaling_retriever_amd.modeling.llm_encoder import LlamaBiDense
    _, cfg, w = golden_case(golden_dir, "enc_hd64")
    bm = LlamaBiDense.from_weights(cfg, bf16_valued(w)).to("cuda").eval().base_model
    H = cfg["hidden_size"]
    t = torch.ones(H, dtype=torch.float32, device="cuda")
    rc = bm._lib.sr_model_set_weight(bm._h, b"model.norm.weight", t.data_ptr(), _lib.SR_DTYPE_F32, H, 1, _lib.stream_ptr())
    assert rc == _lib.SR_ERR_INVALID
    assert b"finalized" in bm._lib.sr_last_error()
    n = ctypes.c_int64(0)
    assert bm._lib.sr_model_weight_segments(bm._h, None, 0, ctypes.byref(n)) == _lib.SR_OK
    assert n.value == 4 * cfg["num_hidden_layers"]
