"""GPU: the fp32 attention of the encoder's fp32 regime (csrc/attention_f32.hip) through sr_attention_varlen_f32, kernel by kernel,
element-wise against a float64 restatement of the same operation (per sequence, per head: softmax(q k^T / sqrt(hd) + mask) v,
masked keys -inf, a row without a valid key = zeros) on the same fp32 inputs.

Which kernel a parametrisation runs (launch_attention_f32; SR_ATTN_F32_MFMA / SR_ATTN_F32_GQA are its development switches):

  variant     switches                     nh / nkv == 4                                          any other group size
  mfma_gqa    none (the product's path)    attention_f32_mfma_kernel<hd> for sequences <= 64,     -
                                           attention_f32_gqa_kernel<hd, 4> for longer ones
  gqa         SR_ATTN_F32_MFMA=0           attention_f32_gqa_kernel<hd, 4> for every length       -
  fma         both = 0 / none needed       attention_f32_kernel<hd>                               attention_f32_kernel<hd>

with hd in {64, 128}: all six instantiations.

Tolerance.  The yardstick is the arithmetic the reference's no-autocast pass runs, not the kernel: torch's
scaled_dot_product_attention on the CPU on fp32 tensors with a float mask (finfo.min on masked keys), against the same float64
restatement, as the largest absolute error of an output element over every case of a family (rows without a valid key excluded:
the float mask gives them a mean of v, the kernels zeros).  A kernel's bound is that error times MARGIN = 4 (serial fmaf chains
and a 64-key online rescale against torch's blocked sums: a small constant between two correct fp32 implementations).  The
yardstick is recomputed by the test on the CPU from the same seeded inputs, so the bound never depends on what a kernel returns.

Measured (largest |error| against float64 of any output element over the family's cases; family = input kind x head dim over
the six head geometries; randn = the `lengths` and `masks` batches, large = the large-logit `lengths` batch):

  family        torch fp32 SDPA (CPU)   bound = 4 x   mfma_gqa     gqa          fma
  randn hd 64   1.298e-06               5.192e-06     1.431e-06    1.417e-06    1.417e-06
  randn hd 128  2.265e-06               9.059e-06     2.265e-06    2.384e-06    2.384e-06
  large hd 64   9.987e-05               3.995e-04     9.987e-05    9.987e-05    9.987e-05
  large hd 128  1.118e-04               4.471e-04     1.118e-04    1.118e-04    1.118e-04

Every kernel is within 1.1 x the yardstick; the margin of 4 was never needed.  The MFMA kernel and the FMA kernels differ from
each other by at most 8.3e-07 (randn) / 4.8e-07 (large).  Known-answer case: largest error 3.7e-28 (bound 1.2e-04).

Two exact statements failed when this file was written, both because the result depended on what hipcc chose to contract, and
were fixed in attention_f32.hip (explicit fmaf; the output value rounded once): attention_f32_kernel built the last four
products of every score with unfused multiplies and adds, so it was NOT bit-identical to attention_f32_gqa_kernel (all 36 cases
differed); and the FMA kernels' plane segments were the split of the unrounded o * inv (fma(o, inv, -p0)), not of the fp32
output (all 144 cases differed in planes 1 and 2).

The known-answer case has its own bound, derived in test_known_answer_names_key_and_kv_head."""
import functools
import itertools
import math

import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.fp32_regime]

MARGIN = 4.0
LENGTHS = [1, 2, 9, 15, 16, 17, 31, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81, 127, 128, 129, 200, 513]
# the packed batch: every length once, in an order that mixes the kernels' sides of the 64 / 65 border, and an empty sequence
# (cu[b] == cu[b + 1]) between two others
BATCH_LENGTHS = [65, 1, 513, 16, 64, 129, 2, 47, 80, 0, 9, 200, 63, 17, 128, 48, 31, 81, 15, 127, 49, 33, 79]
assert sorted(n for n in BATCH_LENGTHS if n) == LENGTHS

GEOMETRIES_G4 = [(4, 1), (8, 2), (32, 8)]
GEOMETRIES_OTHER = [(2, 2), (2, 1), (8, 1)]
HEAD_DIMS = [64, 128]
SWITCHES = {"mfma_gqa": {}, "gqa": {"SR_ATTN_F32_MFMA": "0"}, "fma": {"SR_ATTN_F32_MFMA": "0", "SR_ATTN_F32_GQA": "0"}}
# (nh, nkv, hd, variant): group 4 runs all three variants, the other group sizes only have attention_f32_kernel
COMBOS = [(nh, nkv, hd, v) for hd in HEAD_DIMS for nh, nkv in GEOMETRIES_G4 for v in ("mfma_gqa", "gqa", "fma")] + \
         [(nh, nkv, hd, "fma") for hd in HEAD_DIMS for nh, nkv in GEOMETRIES_OTHER]
COMBOS_G4 = [(nh, nkv, hd) for hd in HEAD_DIMS for nh, nkv in GEOMETRIES_G4]
combos = pytest.mark.parametrize("nh,nkv,hd,variant", COMBOS, ids=[f"{a}x{b}-hd{c}-{v}" for a, b, c, v in COMBOS])
combos_g4 = pytest.mark.parametrize("nh,nkv,hd", COMBOS_G4, ids=[f"{a}x{b}-hd{c}" for a, b, c in COMBOS_G4])
# split_map_a of csrc/kernels.h: plane (0 = leading bf16 plane) of each output segment
SEGMENT_PLANES = {3: [2, 0, 1, 1, 0, 0], 2: [1, 0, 0]}


# ------------------------------------------------------------------------------------------------------ cases (built on the CPU)
def _mask_batch():
    """(lengths, key_valid) of the `masks` batch; every sequence says what it is for."""
    seqs = []

    def add(n, masked):
        kv = torch.ones(n, dtype=torch.uint8)
        for a, b in masked:
            kv[a:b] = 0
        seqs.append(kv)

    add(200, [(64, 128)])            # a whole 64-key chunk masked in the middle
    add(200, [(0, 64)])              # the FIRST chunk masked, later ones valid
    add(200, [(77, 78)])             # one masked key
    add(64, [(0, 40)])               # masked prefix (left padding)
    add(65, [(35, 65)])              # masked suffix (right padding), across the 64 / 65 border
    add(17, [(0, 17)])               # every key masked (short-sequence kernel at group 4)
    add(130, [(0, 130)])             # every key masked (FMA kernels): rows must be WRITTEN as zeros
    add(0, [])                       # empty sequence between two others
    add(48, [(16, 17), (0, 3)])      # a masked key on a 16-key block edge + a short prefix
    add(129, [(0, 70)])              # prefix over the whole first chunk and part of the second; the last chunk holds one key
    add(513, [(500, 513), (128, 192), (3, 4)])   # suffix + a whole middle chunk + one key
    add(33, [(32, 33)])              # only the one key of the third 16-key block masked
    add(16, [(0, 15)])               # one valid key
    add(1, [])
    return [len(s) for s in seqs], torch.cat(seqs)


@functools.lru_cache(maxsize=None)
def _case(kind, nh, nkv, hd):
    """kind: 'lengths' (randn, all valid) | 'masks' (randn) | 'large' (large logits, all valid) | 'known' (known answer).
    Returns dict(qkv fp32 [T, (nh + 2 nkv) hd], lens, key_valid uint8 [T]) on the CPU, seeded."""
    g = torch.Generator().manual_seed(1000 * nh + 10 * nkv + hd + {"lengths": 1, "masks": 2, "large": 3, "known": 4}[kind])
    if kind == "masks":
        lens, key_valid = _mask_batch()
    else:
        lens = list(BATCH_LENGTHS)
        key_valid = torch.ones(sum(lens), dtype=torch.uint8)
    T, G = sum(lens), nh // nkv
    q = torch.randn((T, nh, hd), generator=g)
    k = torch.randn((T, nkv, hd), generator=g)
    v = torch.randn((T, nkv, hd), generator=g)
    extra = {}
    if kind == "large":
        # keys of norm sqrt(hd); q row r of head h = c (k[t] + 0.99 k[u]) + noise with c sqrt(hd) = 300: the scaled scores of keys t
        # and u are ~300 and ~297 (raw q.k: 2400 / 3400), every other key tens to hundreds below - exp() of a score that is
        # not reduced by the row maximum overflows, and a running maximum that is corrected wrongly when the dominant key
        # sits in a later chunk than the first gives a visibly wrong row
        k = k / k.norm(dim=-1, keepdim=True) * math.sqrt(hd)
        c = 300.0 / math.sqrt(hd)
        t0 = 0
        for n in lens:
            r = torch.arange(n)
            for h in range(nh):
                t, u = (7 * r + 3 * h + 3) % max(n, 1), (7 * r + 3 * h + 4) % max(n, 1)
                q[t0 + r, h] = c * (k[t0 + t, h // G] + 0.99 * k[t0 + u, h // G]) + 0.1 * q[t0 + r, h]
            t0 += n
    if kind == "known":
        # k of (key j, kv head g) = a random sign vector (norm^2 = hd, distinct per (g, j)); q of (row r, head h) = 16 x the
        # sign vector of ITS key t(r, h) in ITS kv head: scaled score 16 sqrt(hd) for that key, far less for every other.
        # v of (key j, kv head g) = [j, g, 0 ... 1 at 2 + j % (hd - 2) ... 0]: the output row names the key and the kv head.
        k = torch.where(torch.rand((T, nkv, hd), generator=g) < 0.5, -1.0, 1.0)
        v = torch.zeros((T, nkv, hd))
        target = torch.zeros((T, nh), dtype=torch.int64)
        t0 = 0
        for n in lens:
            j = torch.arange(n)
            for gk in range(nkv):
                v[t0 + j, gk, 0] = j.float()
                v[t0 + j, gk, 1] = float(gk)
                v[t0 + j, gk, 2 + j % (hd - 2)] = 1.0
            for h in range(nh):
                t = (5 * j + 3 * h + 1) % max(n, 1)
                target[t0 + j, h] = t
                q[t0 + j, h] = 16.0 * k[t0 + t, h // G]
            t0 += n
        extra["target"] = target
    qkv = torch.cat([q.reshape(T, -1), k.reshape(T, -1), v.reshape(T, -1)], dim=1).contiguous()
    return dict(qkv=qkv, lens=lens, key_valid=key_valid, **extra)


def _reference_f64(qkv, lens, key_valid, nh, nkv, hd, largest_weight=None):
    """The operation, plainly, in float64 on qkv's device: [T, nh * hd].  largest_weight: a [T, nh] float64 tensor that
    receives the largest softmax weight of each (row, head)."""
    T, G = qkv.shape[0], nh // nkv
    x = qkv.double()
    q = x[:, :nh * hd].reshape(T, nh, hd)
    k = x[:, nh * hd:(nh + nkv) * hd].reshape(T, nkv, hd)
    v = x[:, (nh + nkv) * hd:].reshape(T, nkv, hd)
    out = torch.zeros((T, nh, hd), dtype=torch.float64, device=qkv.device)
    t0 = 0
    for n in lens:
        sl = slice(t0, t0 + n)
        t0 += n
        valid = key_valid[sl].bool()
        if n == 0 or not bool(valid.any()):
            continue                                       # no valid key: zeros
        kk, vv = k[sl].repeat_interleave(G, dim=1), v[sl].repeat_interleave(G, dim=1)
        sc = torch.einsum("qhd,khd->hqk", q[sl], kk) / math.sqrt(hd)
        sc = sc.masked_fill(~valid[None, None, :], float("-inf"))
        p = torch.softmax(sc, dim=-1)
        out[sl] = torch.einsum("hqk,khd->qhd", p, vv)
        if largest_weight is not None:
            largest_weight[sl] = p.max(dim=-1).values.transpose(0, 1)
    return out.reshape(T, nh * hd)


def _rows_with_a_valid_key(lens, key_valid):
    keep = torch.zeros(sum(lens), dtype=torch.bool)
    t0 = 0
    for n in lens:
        if n and bool(key_valid[t0:t0 + n].any()):
            keep[t0:t0 + n] = True
        t0 += n
    return keep


def _yardstick_sdpa_fp32_cpu(qkv, lens, key_valid, nh, nkv, hd):
    """What the reference's no-autocast pass runs: torch SDPA on fp32 CPU tensors with a float mask (finfo.min on masked keys)."""
    T, G = qkv.shape[0], nh // nkv
    q = qkv[:, :nh * hd].reshape(T, nh, hd)
    k = qkv[:, nh * hd:(nh + nkv) * hd].reshape(T, nkv, hd)
    v = qkv[:, (nh + nkv) * hd:].reshape(T, nkv, hd)
    out = torch.zeros((T, nh, hd))
    t0 = 0
    for n in lens:
        sl = slice(t0, t0 + n)
        t0 += n
        if n == 0:
            continue
        mask = torch.zeros((1, 1, n, n))
        mask.masked_fill_(~key_valid[sl].bool()[None, None, None, :], torch.finfo(torch.float32).min)
        kk, vv = k[sl].repeat_interleave(G, dim=1), v[sl].repeat_interleave(G, dim=1)
        o = torch.nn.functional.scaled_dot_product_attention(q[sl].transpose(0, 1)[None], kk.transpose(0, 1)[None],
                                                             vv.transpose(0, 1)[None], attn_mask=mask)
        out[sl] = o[0].transpose(0, 1)
    return out.reshape(T, nh * hd)


def _kind_family(kind):
    return "large" if kind == "large" else "randn"


@functools.lru_cache(maxsize=None)
def _reference(kind, nh, nkv, hd):
    """float64 reference of a case, on the CPU (computed on the GPU when there is one: the same plain float64 code)."""
    c = _case(kind, nh, nkv, hd)
    dev = "cuda" if torch.cuda.is_available() else "cpu"
    return _reference_f64(c["qkv"].to(dev), c["lens"], c["key_valid"].to(dev), nh, nkv, hd).cpu()


@functools.lru_cache(maxsize=None)
def _yardstick_error(family, hd):
    """Largest |torch fp32 SDPA (CPU) - float64| of any output element over the family's cases and the six geometries."""
    worst = 0.0
    for kind in (("lengths", "masks") if family == "randn" else ("large",)):
        for nh, nkv in GEOMETRIES_G4 + GEOMETRIES_OTHER:
            c = _case(kind, nh, nkv, hd)
            keep = _rows_with_a_valid_key(c["lens"], c["key_valid"])
            y = _yardstick_sdpa_fp32_cpu(c["qkv"], c["lens"], c["key_valid"], nh, nkv, hd)
            worst = max(worst, float((y.double() - _reference(kind, nh, nkv, hd))[keep].abs().max()))
    return worst


def _bound(kind, hd):
    return MARGIN * _yardstick_error(_kind_family(kind), hd)


# ------------------------------------------------------------------------------------------------------ running the kernels
def _lib():
    from scaling_retriever_amd import _lib as L
    return L, L.load()


def _set_variant(monkeypatch, variant):
    for name in ("SR_ATTN_F32_MFMA", "SR_ATTN_F32_GQA"):
        monkeypatch.delenv(name, raising=False)
    for name, value in SWITCHES[variant].items():
        monkeypatch.setenv(name, value)


def _run(qkv, lens, key_valid, nh, nkv, hd, planes=None):
    """One call on CPU inputs; returns the fp32 output [T, nh hd] (planes None) or the bf16 segments [T, n_seg, nh hd], on the
    CPU.  The output is pre-filled with NaN: a row the kernels do not write stays visible.  max_seqlen is the true maximum."""
    L, lib = _lib()
    T = sum(lens)
    assert qkv.shape == (T, (nh + 2 * nkv) * hd) and key_valid.shape == (T,) and qkv.dtype == torch.float32
    d_qkv, d_kv = qkv.cuda().contiguous(), key_valid.cuda().contiguous()
    cu = torch.tensor([0] + list(itertools.accumulate(lens)), dtype=torch.int32, device="cuda")
    if planes is None:
        out = torch.full((T, nh * hd), float("nan"), dtype=torch.float32, device="cuda")
        args = (out.data_ptr(), None, 0)
    else:
        out = torch.full((T, len(SEGMENT_PLANES[planes]), nh * hd), float("nan"), dtype=torch.bfloat16, device="cuda")
        args = (None, out.data_ptr(), planes)
    L.check(lib.sr_attention_varlen_f32(d_qkv.data_ptr(), *args, cu.data_ptr(), d_kv.data_ptr(), len(lens), nh, nkv, hd, max(lens),
                                        L.stream_ptr()), "sr_attention_varlen_f32")
    torch.cuda.synchronize()
    return out.cpu()


def _run_case(kind, nh, nkv, hd, planes=None):
    c = _case(kind, nh, nkv, hd)
    return _run(c["qkv"], c["lens"], c["key_valid"], nh, nkv, hd, planes)


def _sequences(lens):
    t0 = 0
    for n in lens:
        yield t0, n
        t0 += n


def _check_against_f64(out, kind, nh, nkv, hd, what):
    """Element-wise: every output element within the family's bound of float64; rows without a valid key exactly zero."""
    c, ref = _case(kind, nh, nkv, hd), _reference(kind, nh, nkv, hd)
    assert torch.isfinite(out).all(), f"{what}: {int((~torch.isfinite(out)).sum())} non-finite output elements (unwritten rows or inf / NaN)"
    keep = _rows_with_a_valid_key(c["lens"], c["key_valid"])
    err = (out.double() - ref).abs()
    bound = _bound(kind, hd)
    worst = float(err.max())
    print(f"{what} {kind} {nh}x{nkv} hd{hd}: max |err| {worst:.3e}  bound {bound:.3e} (= {MARGIN:g} x {_yardstick_error(_kind_family(kind), hd):.3e})")
    assert torch.equal(out[~keep], torch.zeros_like(out[~keep])), f"{what}: rows without a valid key are not zeros"
    if worst > bound:
        row = int(err.max(dim=1).values.argmax())
        b = [i for i, (t0, n) in enumerate(_sequences(c["lens"])) if t0 <= row < t0 + n][0]
        raise AssertionError(f"{what} {kind} {nh}x{nkv} hd{hd}: max |err| {worst:.3e} > {bound:.3e} at token row {row} "
                             f"(sequence {b}, length {c['lens'][b]}), column {int(err[row].argmax())}")
    return worst


# ------------------------------------------------------------------------------------------------------ against float64
@combos
@pytest.mark.parametrize("kind", ["lengths", "masks", "large"])
def test_kernel_against_float64(kind, nh, nkv, hd, variant, monkeypatch):
    """Every instantiation, every length around the kernels' block edges in one packed batch, every mask form, randn and
    large-logit inputs: each output element within MARGIN x the error of torch's own fp32 SDPA."""
    _set_variant(monkeypatch, variant)
    _check_against_f64(_run_case(kind, nh, nkv, hd), kind, nh, nkv, hd, variant)


@combos
def test_known_answer_names_key_and_kv_head(nh, nkv, hd, variant, monkeypatch):
    """Row r of head h attends to key t(r, h) of kv head h // G alone; v spells (key, kv head), so a permutation of rows, heads,
    kv heads or keys shows in the output.  Bound: delta = the float64 softmax weight of all other keys together (asserted
    below 1e-12: scaled scores 16 sqrt(hd) against at most about half of it).  In fp32 the weight of key t is exp(0) = 1
    exactly and the other weights sum to at most 2 delta whatever the rounding of their scores (scores below 200, each with
    a relative error below hd 2^-24); the row is v[t] (entries j, g, 1: exact in fp32) plus at most 2 delta max|v|, times
    1 / (1 + that sum), formed with at most a product, a division and an accumulation rounding per element:
    |out - v[t]| <= max|v| (4 delta + 4 * 2^-24)."""
    _set_variant(monkeypatch, variant)
    c = _case("known", nh, nkv, hd)
    T, G = sum(c["lens"]), nh // nkv
    seq_start = torch.cat([torch.full((n,), t0) for t0, n in _sequences(c["lens"])])
    v = c["qkv"][:, (nh + nkv) * hd:].reshape(T, nkv, hd)
    expect = torch.stack([v[seq_start + c["target"][:, h], h // G] for h in range(nh)], dim=1)          # [T, nh, hd]
    pmax = torch.zeros((T, nh), dtype=torch.float64)
    ref = _reference_f64(c["qkv"], c["lens"], c["key_valid"], nh, nkv, hd, largest_weight=pmax).reshape(T, nh, hd)
    delta = float((1.0 - pmax).max())
    assert delta < 1e-12, delta                                                                          # the construction holds:
    assert float((ref - expect.double()).abs().max()) <= 2 * delta * float(v.max()) + 1e-12             # float64 says v[t] too
    out = _run_case("known", nh, nkv, hd).reshape(T, nh, hd)
    assert torch.isfinite(out).all()
    bound = float(v.max()) * (4 * delta + 4 * 2.0 ** -24)
    err = float((out.double() - expect.double()).abs().max())
    print(f"{variant} known {nh}x{nkv} hd{hd}: max |err| {err:.3e} bound {bound:.3e}")
    assert torch.equal(out[:, :, 0].round().long(), c["target"]), "an output row names another key than the one it attends to"
    assert torch.equal(out[:, :, 1].round().long(), (torch.arange(nh) // G)[None, :].expand(T, nh)), "wrong kv head"
    assert torch.equal(out[:, :, 2:].argmax(dim=-1), c["target"] % (hd - 2))
    assert err <= bound, (err, bound)


@combos_g4
@pytest.mark.parametrize("kind", ["lengths", "masks", "large"])
def test_mfma_and_fma_kernels_differ_within_both_bounds(kind, nh, nkv, hd, monkeypatch):
    """The MFMA kernel and the FMA kernels contract in different orders: not expected to be equal.  Both meet the float64 bound
    (test_kernel_against_float64), so they are within twice the bound of each other; the difference is printed."""
    _set_variant(monkeypatch, "mfma_gqa")
    a = _run_case(kind, nh, nkv, hd)
    _set_variant(monkeypatch, "fma")
    b = _run_case(kind, nh, nkv, hd)
    diff = float((a.double() - b.double()).abs().max())
    print(f"mfma vs fma {kind} {nh}x{nkv} hd{hd}: max |difference| {diff:.3e}, equal: {torch.equal(a, b)}")
    assert diff <= 2 * _bound(kind, hd)


# ------------------------------------------------------------------------------------------------------ exact statements
@combos_g4
@pytest.mark.parametrize("kind", ["lengths", "masks", "large", "known"])
@pytest.mark.parametrize("planes", [None, 3])
def test_gqa_kernel_is_bit_identical_to_the_per_head_kernel(kind, planes, nh, nkv, hd, monkeypatch):
    """attention_f32_gqa_kernel: 'same arithmetic per (row, head) ... bit-identical outputs' to attention_f32_kernel."""
    _set_variant(monkeypatch, "gqa")
    a = _run_case(kind, nh, nkv, hd, planes)
    _set_variant(monkeypatch, "fma")
    b = _run_case(kind, nh, nkv, hd, planes)
    assert torch.isfinite(a.float()).all()
    assert torch.equal(_bits(a), _bits(b))


def _bits(x):
    return x.view(torch.int32) if x.dtype == torch.float32 else x.view(torch.int16)


@combos_g4
def test_the_kernels_change_at_64_tokens(nh, nkv, hd, monkeypatch):
    """launch_attention_f32 at 4 q heads per kv head: sequences of at most 64 tokens run the MFMA kernel, longer ones the grouped
    FMA kernel.  With SR_ATTN_F32_MFMA=0 every sequence runs the grouped FMA kernel, so in the product's batch a sequence
    above 64 tokens has exactly those bits, and a sequence of 9 to 64 tokens does not (another kernel ran: the MFMA kernel
    normalises the weights before P V and contracts the keys in another order, which cannot give the same bits in every one
    of the at least 9 * 4 * 64 randn elements of a sequence; 1 and 2 tokens are left out, a one-key softmax is exact in
    both).  64 must differ and 65 must be equal: the border is where the code says it is."""
    c = _case("lengths", nh, nkv, hd)
    _set_variant(monkeypatch, "mfma_gqa")
    product = _run_case("lengths", nh, nkv, hd)
    _set_variant(monkeypatch, "gqa")
    grouped = _run_case("lengths", nh, nkv, hd)
    seen = set()
    for t0, n in _sequences(c["lens"]):
        same = torch.equal(_bits(product[t0:t0 + n]), _bits(grouped[t0:t0 + n]))
        if n > 64:
            assert same, f"length {n}: not the grouped FMA kernel's bits"
        elif n >= 9:
            assert not same, f"length {n}: the grouped FMA kernel's bits, so the MFMA kernel did not run"
        seen.add(n)
    assert {9, 48, 49, 63, 64, 65} <= seen


@combos
@pytest.mark.parametrize("kind", ["lengths", "masks"])
def test_a_sequence_alone_equals_the_sequence_in_the_batch(kind, nh, nkv, hd, variant, monkeypatch):
    """The kernel is chosen per sequence, so the bits of a sequence never depend on what else shares the batch: every length
    (both sides of the 64 / 65 border) run alone == its rows of the mixed batch; and alone it meets the float64 bound too."""
    _set_variant(monkeypatch, variant)
    c, ref = _case(kind, nh, nkv, hd), _reference(kind, nh, nkv, hd)
    batch = _run_case(kind, nh, nkv, hd)
    bound = _bound(kind, hd)
    for t0, n in _sequences(c["lens"]):
        if n == 0:
            continue
        alone = _run(c["qkv"][t0:t0 + n].contiguous(), [n], c["key_valid"][t0:t0 + n].contiguous(), nh, nkv, hd)
        assert torch.isfinite(alone).all(), n
        assert torch.equal(_bits(alone), _bits(batch[t0:t0 + n])), f"length {n}: alone != in the batch"
        assert float((alone.double() - ref[t0:t0 + n]).abs().max()) <= bound, n


def _split_bf16x3(x):
    """csrc/common.h split_bf16x3: plane i = the round-to-nearest-even bf16 of what the planes before it left."""
    p0 = x.bfloat16()
    r1 = x - p0.float()
    p1 = r1.bfloat16()
    p2 = (r1 - p1.float()).bfloat16()
    return [p0, p1, p2]


@combos
@pytest.mark.parametrize("kind", ["lengths", "masks", "large"])
@pytest.mark.parametrize("planes", [3, 2])
def test_plane_segments_are_the_split_of_the_fp32_output(planes, kind, nh, nkv, hd, variant, monkeypatch):
    """bf16 plane segments (fp32_planes 3: planes 2 0 1 1 0 0; 2: planes 1 0 0) == split_bf16x3 of the fp32 output form,
    segment by segment, bit for bit; rows without a valid key are written as zeros in every segment."""
    _set_variant(monkeypatch, variant)
    f32 = _run_case(kind, nh, nkv, hd)
    seg = _run_case(kind, nh, nkv, hd, planes)
    assert torch.isfinite(f32).all() and not torch.isnan(seg.float()).any()
    split = _split_bf16x3(f32)
    assert seg.shape[1] == len(SEGMENT_PLANES[planes])
    for sg, plane in enumerate(SEGMENT_PLANES[planes]):
        assert torch.equal(_bits(seg[:, sg]), _bits(split[plane])), f"segment {sg} is not plane {plane}"
    # the three planes carry the value: the split is the one of common.h only if they add up to it again
    assert float((split[0].double() + split[1].double() + split[2].double() - f32.double()).abs().max()) <= 2.0 ** -24 * float(f32.abs().max())


@combos
@pytest.mark.parametrize("planes", [None, 3])
def test_two_runs_are_bit_identical(planes, nh, nkv, hd, variant, monkeypatch):
    _set_variant(monkeypatch, variant)
    for kind in ("lengths", "masks"):
        a, b = _run_case(kind, nh, nkv, hd, planes), _run_case(kind, nh, nkv, hd, planes)
        assert torch.equal(_bits(a), _bits(b)), kind


# ------------------------------------------------------------------------------------------------------ status checks
@pytest.mark.parametrize("nh,nkv", [(4, 1), (2, 1)])
@pytest.mark.parametrize("variant", ["mfma_gqa", "gqa", "fma"])
def test_unsupported_head_dim_is_an_error_and_launches_nothing(nh, nkv, variant, monkeypatch):
    """head_dim 96: SR_ERR_UNSUPPORTED with a message; the buffers are sized for head_dim 96 and the output stays untouched."""
    _set_variant(monkeypatch, variant)
    L, lib = _lib()
    hd, n = 96, 5
    qkv = torch.randn((n, (nh + 2 * nkv) * hd), device="cuda")
    key_valid = torch.ones(n, dtype=torch.uint8, device="cuda")
    cu = torch.tensor([0, n], dtype=torch.int32, device="cuda")
    out = torch.full((n, nh * hd), float("nan"), device="cuda")
    rc = lib.sr_attention_varlen_f32(qkv.data_ptr(), out.data_ptr(), None, 0, cu.data_ptr(), key_valid.data_ptr(), 1, nh, nkv, hd, n,
                                     L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == L.SR_ERR_UNSUPPORTED
    assert b"head_dim 96" in lib.sr_last_error()
    assert torch.isnan(out).all()
    with pytest.raises(L.SrHipError):
        L.check(rc, "sr_attention_varlen_f32")
