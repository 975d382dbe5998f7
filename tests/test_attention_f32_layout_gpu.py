"""GPU: the launch plan and data path of attention_f32_mfma_kernel (csrc/attention_f32.hip, sequences of at most 64 tokens).

The kernel is launched per key-block class ceil(S / 16) = 1..4 with LDS for that class only, takes q from global memory straight
into the MFMA operand registers and stores 16 bytes (fp32 form) / 8 bytes per segment (plane form) per lane.  None of that touches
an arithmetic chain, so every route must give the same bits:

  SR_ATTN_F32_LAYOUT   route of a call through sr_attention_varlen_f32 (no class counts: the caller has no host copy of cu_seqlens)
  unset                ONE launch of the new form, sized by the batch's longest sequence, serving every class
  0                    the form before the plan: one launch, LDS by the batch's longest sequence, q through LDS, element stores
  2                    one launch of the new form PER CLASS up to the longest sequence's; a workgroup of another class leaves

model_forward knows the class counts and skips the launches of empty classes; that route is taken by the encoder tests at the
end (a batch with every class, a batch of one class, a batch of one sequence) against SR_ATTN_F32_LAYOUT=0.

fp32 output is also held to the float64 bound of tests/test_attention_f32_gpu.py (4 x the error of torch's fp32 SDPA on the CPU
over that file's randn cases, computed there from seeded inputs: it never depends on what a kernel returns)."""
import functools

import pytest
import torch

from test_attention_f32_gpu import _bits, _bound, _reference_f64, _rows_with_a_valid_key, _run, _sequences

pytestmark = [pytest.mark.gpu, pytest.mark.fp32_regime]

# the class edges (16 n, 16 n + 1), an empty sequence and one sequence of the long path (FMA kernel, untouched by the switch)
LENGTHS = [1, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 0, 65]
CONFIGS = [(8, 2, 64), (4, 1, 128)]
configs = pytest.mark.parametrize("nh,nkv,hd", CONFIGS, ids=[f"{a}x{b}-hd{c}" for a, b, c in CONFIGS])
LAYOUTS = {"plan": None, "old": "0", "classes": "2"}
FORMS = [None, 2, 3]
BATCHES = ["ordered", "shuffled", "masked"]


@functools.lru_cache(maxsize=None)
def _batch(kind, nh, nkv, hd):
    """(qkv [T, (nh + 2 nkv) hd] fp32, lens, key_valid uint8 [T]) on the CPU, seeded."""
    g = torch.Generator().manual_seed(7000 + 100 * nh + hd + BATCHES.index(kind))
    lens = list(LENGTHS)
    if kind == "shuffled":
        lens = [lens[i] for i in torch.randperm(len(lens), generator=g).tolist()]
    T = sum(lens)
    qkv = torch.randn((T, (nh + 2 * nkv) * hd), generator=g)
    key_valid = torch.ones(T, dtype=torch.uint8)
    if kind == "masked":
        for t0, n in _sequences(lens):
            if n == 17:
                key_valid[t0:t0 + n] = 0                                   # a fully masked sequence: rows written as zeros
            elif n == 33:
                key_valid[t0 + 32] = 0                                     # the one key of the third block
            elif n == 64:
                key_valid[t0:t0 + 40] = 0                                  # masked prefix (left padding)
            elif n > 1:
                key_valid[t0:t0 + n] = (torch.rand(n, generator=g) < 0.7).to(torch.uint8)
                key_valid[t0 + n - 1] = 1
    return qkv, lens, key_valid


def _set_layout(monkeypatch, layout):
    for name in ("SR_ATTN_F32_LAYOUT", "SR_ATTN_F32_MFMA", "SR_ATTN_F32_GQA"):
        monkeypatch.delenv(name, raising=False)
    if LAYOUTS[layout] is not None:
        monkeypatch.setenv("SR_ATTN_F32_LAYOUT", LAYOUTS[layout])


@configs
@pytest.mark.parametrize("kind", BATCHES)
def test_every_route_gives_the_same_bits(kind, nh, nkv, hd, monkeypatch):
    """fp32 form and plane segments 2 / 3: the plan's single launch == the form before the plan == a launch per class; two runs of
    the plan are equal; the fp32 form meets the float64 bound and rows without a valid key are zeros."""
    qkv, lens, key_valid = _batch(kind, nh, nkv, hd)
    for planes in FORMS:
        out = {}
        for layout in LAYOUTS:
            _set_layout(monkeypatch, layout)
            out[layout] = _run(qkv, lens, key_valid, nh, nkv, hd, planes)
        assert not torch.isnan(out["old"].float()).any(), "the form before the plan left rows unwritten"
        for layout in ("plan", "classes"):
            assert torch.equal(_bits(out[layout]), _bits(out["old"])), f"{kind} planes {planes}: {layout} != SR_ATTN_F32_LAYOUT=0"
        _set_layout(monkeypatch, "plan")
        again = _run(qkv, lens, key_valid, nh, nkv, hd, planes)
        assert torch.equal(_bits(again), _bits(out["plan"])), f"{kind} planes {planes}: two runs differ"
        if planes is None:
            ref = _reference_f64(qkv.cuda(), lens, key_valid.cuda(), nh, nkv, hd).cpu()
            keep = _rows_with_a_valid_key(lens, key_valid)
            worst, bound = float((out["plan"].double() - ref).abs().max()), _bound("lengths", hd)
            print(f"{kind} {nh}x{nkv} hd{hd}: max |err| against float64 {worst:.3e}, bound {bound:.3e}")
            assert torch.equal(out["plan"][~keep], torch.zeros_like(out["plan"][~keep]))
            assert worst <= bound, (worst, bound)


@configs
@pytest.mark.parametrize("kind", ["ordered", "masked"])
@pytest.mark.parametrize("planes", [None, 2, 3])
def test_a_sequence_alone_equals_its_rows_in_the_batch(planes, kind, nh, nkv, hd, monkeypatch):
    """Alone, a sequence runs in a launch sized for ITS class; in the batch, in one sized for the longest - and with
    SR_ATTN_F32_LAYOUT=2 in its class's launch among workgroups that leave.  Same bits."""
    qkv, lens, key_valid = _batch(kind, nh, nkv, hd)
    _set_layout(monkeypatch, "plan")
    batch = _run(qkv, lens, key_valid, nh, nkv, hd, planes)
    for t0, n in _sequences(lens):
        if n == 0:
            continue
        for layout in ("plan", "classes"):
            _set_layout(monkeypatch, layout)
            alone = _run(qkv[t0:t0 + n].contiguous(), [n], key_valid[t0:t0 + n].contiguous(), nh, nkv, hd, planes)
            assert torch.equal(_bits(alone), _bits(batch[t0:t0 + n])), f"length {n} alone ({layout}) != in the batch"


@configs
def test_one_class_batches_and_a_batch_of_one(nh, nkv, hd, monkeypatch):
    """Batches whose sequences share one class (the launch is sized for it and no other class exists), with an empty sequence
    inside, and a batch of one sequence: all routes equal, every row written."""
    g = torch.Generator().manual_seed(99 + hd)
    for lens in ([3, 16, 0, 9, 1, 12], [33, 48, 40, 0, 47], [49, 64], [7], [64]):
        T = sum(lens)
        qkv = torch.randn((T, (nh + 2 * nkv) * hd), generator=g)
        key_valid = torch.ones(T, dtype=torch.uint8)
        for planes in (None, 2):
            out = {}
            for layout in LAYOUTS:
                _set_layout(monkeypatch, layout)
                out[layout] = _run(qkv, lens, key_valid, nh, nkv, hd, planes)
            assert not torch.isnan(out["plan"].float()).any()
            assert torch.equal(_bits(out["plan"]), _bits(out["old"])) and torch.equal(_bits(out["classes"]), _bits(out["old"])), (lens, planes)


# ------------------------------------------------------------------------------------------------------ through the encoder
@pytest.mark.parametrize("fp32_planes", [16, 3])
def test_encoder_with_class_counts_equals_the_old_form(golden_dir, fp32_planes, monkeypatch):
    """model_forward counts the classes on the host and launches only the ones that have a sequence (fp32_planes 16: fp32 output
    form, 3: plane segments).  A batch with every class, batches of one class (the other launches are skipped) and a batch of one
    sequence == the same encode with SR_ATTN_F32_LAYOUT=0."""
    from scaling_retriever_amd.modeling.llm_encoder import LlamaBiDense
    from test_fp16_weight_segments_gpu import batch, encode, golden_case
    _, cfg, w = golden_case(golden_dir, "enc_hd64")
    model = LlamaBiDense.from_weights(cfg, w, fp32_planes=fp32_planes).to("cuda").eval()
    for lens in (list(range(1, 65)), [35, 40, 48, 33], [16, 2, 9], [49], [7]):
        ids, mask = batch(cfg, lens, "left", seed=len(lens))
        _set_layout(monkeypatch, "plan")
        new = encode(model, ids, mask)
        _set_layout(monkeypatch, "old")
        old = encode(model, ids, mask)
        assert torch.isfinite(new).all()
        assert torch.equal(new, old), (fp32_planes, lens)
