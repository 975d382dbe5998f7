"""GPU: the 256 x 256 GEMM loop of the fp32 regime's fp16-plane GEMMs is chosen by the operands' plane-segment count
(GemmArgs::a_nseg, csrc/gemm_bf16.hip launch_big): four-wave at 2 segments for the epilogues that measured faster on it (the
SwiGLU-split epilogue of the gate-up GEMM; EpiTraits::FOUR_WAVE_AT_2SEG), eight-wave at 3.  Both loops run the same k-ordered MFMA chain per output element, so the default dispatch must give the bits of
SR_GEMM_BIG=8w (the eight-wave loop everywhere).

2-layer model at 1B widths with bf16-rounded weights (every matrix at 2 segments), 300 tokens (128 x 128 tiles only) and
8 192 + 169 tokens (whole rounds of 256 x 256 tiles plus a ragged tail), dense and sparse heads; and the same model with one
fp32-valued entry, whose matrix alone runs at 3 segments."""
import numpy as np
import pytest
import torch

from golden_weights import make_weights
from test_fp16_weight_segments_gpu import CFG_1B_2L, batch, bf16_valued, build, encode, n_matrices

pytestmark = [pytest.mark.gpu, pytest.mark.fp32_regime]

# sequences of at most 64 tokens that pack to the token counts
TOKENS = {300: [64, 64, 64, 64, 44], 8192 + 169: [64] * 130 + [41]}
assert all(sum(v) == k for k, v in TOKENS.items())


@pytest.fixture(scope="module")
def wide_weights():
    return bf16_valued(make_weights(CFG_1B_2L, 21))


def _default_vs_eight_wave(model, lens, monkeypatch, what):
    ids, mask = batch(CFG_1B_2L, lens, "left", seed=len(lens))
    monkeypatch.delenv("SR_GEMM_BIG", raising=False)
    a = encode(model, ids, mask)
    monkeypatch.setenv("SR_GEMM_BIG", "8w")
    b = encode(model, ids, mask)
    monkeypatch.setenv("SR_GEMM_BIG", "4w")      # every staged fp16-plane GEMM on the four-wave loop: the default's choice lies between
    c = encode(model, ids, mask)
    monkeypatch.delenv("SR_GEMM_BIG", raising=False)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b), f"{what}, {sum(lens)} tokens: default dispatch != SR_GEMM_BIG=8w"
    assert torch.equal(a, c), f"{what}, {sum(lens)} tokens: default dispatch != SR_GEMM_BIG=4w"


@pytest.mark.parametrize("head", ["dense", "sparse"])
def test_two_segment_model_equals_the_eight_wave_loop(wide_weights, head, monkeypatch):
    from scaling_retriever_amd.modeling.llm_encoder import LlamaBiDense, LlamaBiSparse
    cls = LlamaBiDense if head == "dense" else LlamaBiSparse
    model = build(cls, CFG_1B_2L, wide_weights, monkeypatch)
    assert model.base_model.weight_segments() == [2] * n_matrices(CFG_1B_2L, head == "sparse")
    for lens in TOKENS.values():
        _default_vs_eight_wave(model, lens, monkeypatch, head)


@pytest.mark.parametrize("head", ["dense", "sparse"])
def test_a_three_segment_matrix_among_two_segment_ones(wide_weights, head, monkeypatch):
    """Layer 1 down_proj has one fp32-valued entry and keeps 3 segments (eight-wave loop), every other matrix runs at 2."""
    from scaling_retriever_amd.modeling.llm_encoder import LlamaBiDense, LlamaBiSparse
    cls = LlamaBiDense if head == "dense" else LlamaBiSparse
    w = dict(wide_weights)
    d = w["model.layers.1.mlp.down_proj.weight"].copy()
    d[7, 100] = d[7, 100] * np.float32(1.0 + 2.0 ** -20)
    w["model.layers.1.mlp.down_proj.weight"] = d
    model = build(cls, CFG_1B_2L, w, monkeypatch)
    expect = [2] * n_matrices(CFG_1B_2L, head == "sparse")
    expect[4 * 1 + 3] = 3
    assert model.base_model.weight_segments() == expect
    for lens in TOKENS.values():
        _default_vs_eight_wave(model, lens, monkeypatch, head + ", one 3-segment matrix")
