"""GPU: the bf16 attention kernels (csrc/attention.hip) through sr_attention_varlen, instantiation by instantiation, every output
element against the float64 reference and the derived bound of tests/attention_cases.py (its docstring has the derivation).

Which kernel a row runs (launch_hd; SR_ATTN_CKB is its development switch, set per test):

  head dim  SR_ATTN_CKB  longest sequence of the batch       kernel                                      row
  64        -            <= 64 / <= 128 / <= 192 / <= 256    attention_small_kernel<64, 2 / 4 / 6 / 8>   small<64,2|4|6|8>
  64        -            > 256 (257, 511, 512, 513, 700)     attention_long_kernel<64, 8>                long<64,8>
  128       -            <= 64                               attention_small_kernel<128, 2>              small<128,2>
  128       -            > 64 (64 65 128 129 192 257 513)    attention_long_kernel<128, 2>               long<128,2>
  128       3            > 64 (96 97 192 193 288 289)        attention_long_kernel<128, 3>               long<128,3>
  128       8            65-128 / 129-192 / 193-256          attention_small_kernel<128, 4 / 6 / 8>      small<128,4|6|8>
  128       8            > 256                               attention_long_kernel<128, 8>               long<128,8>
  64, 128   -            rope tables passed, any length      attention_kernel<HD, true>                  rope<64>, rope<128>

Fourteen instantiations: all that launch_hd can reach.  Every row runs with the five head geometries (nh, nkv) = (4, 1), (32, 8),
(2, 2), (2, 1), (8, 1) and the case kinds lengths / masks / large / known.  With (8, 1) a 100-token sequence has 32 work items:
several blockIdx.z groups of the small and long kernels, several rounds of the rope kernel.

The rope rows pass quarter-turn tables ((cos, sin) in {(1,0), (0,1), (-1,0), (0,-1)} per (position, frequency), positions
not monotone): the rotation is exact, the float64 reference rotates with the same tables and the bound applies unchanged; a
wrong partner, sign, position index or table stride moves whole elements.  The loose tests with real tables
(test_encoder_gpu.py, test_rope_attention_gpu.py) stay as they are.

Every run writes into a buffer pre-filled with a NaN pattern, with guard rows before row 0 and after row T: every row of a
non-empty sequence must be written, rows of a fully masked sequence must be +0 bit for bit, guard rows keep their bits.

Measured (one MI355X run; largest |error| / bound over every element of the five geometries; torch = torch's CPU
scaled_dot_product_attention on the same bf16 tensors, the arithmetic of the reference's autocast pass, from
`python tests/attention_cases.py`; rows of fully masked sequences, NaN in torch, left out of its column):

  row            lengths: kernel  torch    masks: kernel  torch    large: kernel  torch
  small<64,2>             0.806  0.837            0.710  0.642            0.622  0.597
  small<64,4>             0.648  0.528            0.733  0.589            0.634  0.667
  small<64,6>             0.584  0.473            0.742  0.593            0.683  0.656
  small<64,8>             0.701  0.602            0.739  0.628            0.662  0.642
  long<64,8>              0.707  0.707            0.473  0.473            0.662  0.666
  small<128,2>            0.829  0.862            0.758  0.630            0.490  0.469
  long<128,2>             0.467  0.467            0.591  0.591            0.541  0.541
  long<128,3>             0.501  0.468            0.547  0.547            0.541  0.516
  small<128,4>            0.694  0.556            0.794  0.633            0.559  0.555
  small<128,6>            0.613  0.487            0.743  0.653            0.529  0.567
  small<128,8>            0.712  0.562            0.770  0.647            0.539  0.551
  long<128,8>             0.708  0.708            0.448  0.448            0.531  0.539
  rope<64>                0.721  0.600            0.573  0.458            0.640  0.668
  rope<128>               0.685  0.581            0.568  0.452            0.518  0.537

Every kernel ratio is below 1 (largest 0.829).  The kernels are looser than the torch yardstick, by up to 0.16 of the bound,
in the lengths and masks columns of the small and rope rows (they round the normalised weight to bf16 for the P V MFMA; torch's
CPU path keeps the weights in fp32 there); in the long rows the two agree to the digit shown (the output rounding decides the
worst element).  Known-answer cases: largest error 1.4e-21 (bound 1.2e-04).

Across instantiations (printed by test_the_same_sequence_under_other_instantiations, compared through the bound only):
small<64,4> and small<64,8> gave the same bits in all 15 (geometry, kind) batches; long<128,2>, <128,3> and <128,8> never did
(they rescale and sum the keys in chunks of 64 / 96 / 256): 16-22 % of the elements differ on randn inputs, under 0.02 % on the
large-logit batch, all within the bound."""
import functools
import itertools

import pytest
import torch

import attention_cases as AC

pytestmark = pytest.mark.gpu

GUARD = 3                  # guard rows on each side of the output
NAN_BITS = 0x7FC1          # a quiet NaN no arithmetic produces

COMBOS = [(row, nh, nkv) for row in AC.ROWS for nh, nkv in AC.GEOMETRIES]


@pytest.fixture(scope="module", params=COMBOS, ids=[f"{r}-{a}x{b}" for r, a, b in COMBOS])
def combo(request):
    """(row, nh, nkv); module-scoped so that pytest runs all tests of one combination together and the small caches below hit."""
    return request.param


@functools.lru_cache(maxsize=6)
def _reference(row, kind, nh, nkv):
    return AC.reference(AC.case(row, kind, nh, nkv), device="cuda")


@functools.lru_cache(maxsize=6)
def _device_inputs(row, kind, nh, nkv):
    c = AC.case(row, kind, nh, nkv)
    d = dict(qkv=c["qkv"].cuda(), key_valid=c["key_valid"].cuda())
    if "pos" in c:
        d.update(pos=c["pos"].cuda(), cos=c["cos"].cuda(), sin=c["sin"].cuda())
    return d


def _lib():
    from scaling_retriever_amd import _lib as L
    return L, L.load()


def _bits(x):
    return x.view(torch.int16)


def _run(monkeypatch, row, nh, nkv, lens, d):
    """One sr_attention_varlen call of the row's kernel on device inputs d (qkv, key_valid [, pos, cos, sin]) packed as `lens`.
    Returns the bf16 output [T, nh hd] on the CPU, after checking the guard rows."""
    L, lib = _lib()
    r = AC.ROWS[row]
    hd, T = r["hd"], sum(lens)
    longest = max(lens)
    assert r["rope"] or (r["lo"] <= longest and (r["hi"] is None or longest <= r["hi"])), (row, longest)     # the row's kernel runs
    if r["ckb"] is None:
        monkeypatch.delenv("SR_ATTN_CKB", raising=False)
    else:
        monkeypatch.setenv("SR_ATTN_CKB", r["ckb"])
    qkv, key_valid = d["qkv"].contiguous(), d["key_valid"].contiguous()
    assert qkv.shape == (T, (nh + 2 * nkv) * hd) and qkv.dtype == torch.bfloat16 and key_valid.shape == (T,)
    cu = torch.tensor([0] + list(itertools.accumulate(lens)), dtype=torch.int32, device="cuda")
    buf = torch.full((T + 2 * GUARD, nh * hd), NAN_BITS, dtype=torch.int16, device="cuda")
    out_ptr = buf.data_ptr() + GUARD * nh * hd * 2
    if r["rope"]:
        pos, cos, sin = d["pos"].contiguous(), d["cos"], d["sin"]
        assert pos.shape == (T,) and pos.dtype == torch.int32 and cos.shape == (AC.MAX_POS, hd // 2) and cos.dtype == torch.float32
        rope = (pos.data_ptr(), cos.data_ptr(), sin.data_ptr())
    else:
        rope = (None, None, None)
    L.check(lib.sr_attention_varlen(qkv.data_ptr(), out_ptr, cu.data_ptr(), rope[0], key_valid.data_ptr(), rope[1], rope[2],
                                    len(lens), nh, nkv, hd, L.stream_ptr()), "sr_attention_varlen")
    torch.cuda.synchronize()
    buf = buf.cpu()
    assert bool((buf[:GUARD] == torch.tensor(NAN_BITS, dtype=torch.int16)).all()), "rows before row 0 were written"
    assert bool((buf[GUARD + T:] == torch.tensor(NAN_BITS, dtype=torch.int16)).all()), "rows after row T were written"
    return buf[GUARD:GUARD + T].view(torch.bfloat16)


def _run_case(monkeypatch, row, kind, nh, nkv):
    return _run(monkeypatch, row, nh, nkv, AC.case(row, kind, nh, nkv)["lens"], _device_inputs(row, kind, nh, nkv))


def _sub_batch(d, pieces):
    """Device inputs of the token ranges `pieces` [(t0, n)] packed one after the other (the rope tables stay whole)."""
    out = {k: torch.cat([d[k][t0:t0 + n] for t0, n in pieces]) for k in ("qkv", "key_valid", "pos") if k in d}
    out.update({k: d[k] for k in ("cos", "sin") if k in d})
    return out


def _check(out, c, ref, bound, what):
    """Every element within the bound; every row written; fully masked rows +0 bit for bit.  Returns the largest |err| / bound."""
    written = _bits(out) != NAN_BITS
    assert bool(written.all()), f"{what}: {int((~written).any(dim=1).sum())} rows with unwritten elements"
    assert not bool(torch.isnan(out.float()).any()) and bool(torch.isfinite(out.float()).all()), f"{what}: non-finite output"
    dead = AC.fully_masked_rows(c)
    assert bool((_bits(out[dead]) == 0).all()), f"{what}: rows of a fully masked sequence are not +0"
    err = (out.double() - ref).abs()
    ratio = AC.worst_ratio(out, ref, bound)
    print(f"{what}: max |err| {float(err.max()):.3e}  max |err| / bound {ratio:.3f}")
    bad = err > bound
    if bool(bad.any()):
        t = int(bad.any(dim=1).nonzero()[0])
        b = [i for i, (t0, n) in enumerate(AC.sequences(c["lens"])) if t0 <= t < t0 + n][0]
        col = int(bad[t].nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} elements outside the bound, first at token row {t} (sequence {b}, length "
                             f"{c['lens'][b]}), column {col}: |err| {float(err[t, col]):.3e} > {float(bound[t, col]):.3e}")
    return ratio


@pytest.mark.parametrize("kind", ["lengths", "masks", "large"])
def test_every_element_is_within_the_bound(kind, combo, monkeypatch):
    row, nh, nkv = combo
    ref, bound = _reference(row, kind, nh, nkv)
    _check(_run_case(monkeypatch, row, kind, nh, nkv), AC.case(row, kind, nh, nkv), ref, bound, f"RATIO {row} {kind} {nh}x{nkv}")


def test_known_answer_names_key_and_kv_head(combo, monkeypatch):
    """Row r of head h attends to key t(r, h) of kv head h // G alone; v spells (key, kv head), so a permutation of rows, heads, kv
    heads or keys shows in the output.  Bound: delta = the float64 softmax weight of all other keys together (asserted below
    1e-12: scaled score 16 sqrt(hd) against at most about half of it).  In fp32 the weight of key t is exp2(0) = 1 exactly,
    which bf16 keeps, and the other weights sum to at most 2 delta whatever the rounding of their scores; the fp32 value
    before the output rounding is v[t] plus at most 2 delta max|v|, times 1 / (1 + that sum), formed with at most a product, a
    division and an accumulation rounding: within max|v| (4 delta + 4 * 2^-24) of v[t].  v[t] is a bf16 number, so rounding to
    the nearest bf16 at most doubles the distance: |out - v[t]| <= 2 max|v| (4 delta + 4 * 2^-24)."""
    row, nh, nkv = combo
    c = AC.case(row, "known", nh, nkv)
    hd, T, G = c["hd"], sum(c["lens"]), nh // nkv
    seq_start = torch.cat([torch.full((n,), t0) for t0, n in AC.sequences(c["lens"])])
    v = c["qkv"][:, (nh + nkv) * hd:].double().reshape(T, nkv, hd)
    expect = torch.stack([v[seq_start + c["target"][:, h], h // G] for h in range(nh)], dim=1)          # [T, nh, hd]
    delta = AC.weight_of_the_other_keys(c, device="cuda")
    assert delta < 1e-12, delta
    ref, _ = _reference(row, "known", nh, nkv)
    assert float((ref.reshape(T, nh, hd) - expect).abs().max()) <= 2 * delta * float(v.max()) + 1e-12    # float64 says v[t] too
    out = _run_case(monkeypatch, row, "known", nh, nkv)
    assert bool((_bits(out) != NAN_BITS).all()) and bool(torch.isfinite(out.float()).all())
    out = out.double().reshape(T, nh, hd)
    bound = 2 * float(v.max()) * (4 * delta + 4 * 2.0 ** -24)
    err = float((out - expect).abs().max())
    print(f"KNOWN {row} {nh}x{nkv}: max |err| {err:.3e} bound {bound:.3e}")
    assert torch.equal((out[:, :, 0] + 256 * out[:, :, 1]).round().long(), c["target"]), "an output row names another key than the one it attends to"
    assert torch.equal(out[:, :, 2].round().long(), (torch.arange(nh) // G)[None, :].expand(T, nh)), "wrong kv head"
    assert torch.equal(out[:, :, 3:].argmax(dim=-1), c["target"] % (hd - 3))
    assert err <= bound, (err, bound)


@pytest.mark.parametrize("kind", ["lengths", "masks"])
def test_a_sequence_alone_equals_the_sequence_in_the_batch(kind, combo, monkeypatch):
    """A workgroup reads one sequence only, so a sequence's bits cannot depend on what shares the batch.  The instantiation
    follows from the batch's longest sequence: a sequence inside the row's bracket runs truly alone; a shorter one runs behind
    a single companion, the batch's longest sequence, which keeps the row's kernel (another batch index, another token
    offset, other neighbours than in the packed batch)."""
    row, nh, nkv = combo
    c, d = AC.case(row, kind, nh, nkv), _device_inputs(row, kind, nh, nkv)
    r = AC.ROWS[row]
    batch = _run_case(monkeypatch, row, kind, nh, nkv)
    seqs = list(AC.sequences(c["lens"]))
    longest = max(seqs, key=lambda s: s[1])
    for t0, n in seqs:
        if n == 0:
            continue
        if r["rope"] or n >= r["lo"]:
            alone = _run(monkeypatch, row, nh, nkv, [n], _sub_batch(d, [(t0, n)]))
        else:
            alone = _run(monkeypatch, row, nh, nkv, [longest[1], n], _sub_batch(d, [longest, (t0, n)]))[longest[1]:]
        assert torch.equal(_bits(alone), _bits(batch[t0:t0 + n])), f"length {n} at row {t0}: alone != in the batch"


def test_two_runs_are_bit_identical(combo, monkeypatch):
    row, nh, nkv = combo
    for kind in ("lengths", "masks"):
        a, b = _run_case(monkeypatch, row, kind, nh, nkv), _run_case(monkeypatch, row, kind, nh, nkv)
        assert torch.equal(_bits(a), _bits(b)), kind


# the same sequences under several instantiations: (rows, the row whose batches are used); a companion sequence appended to the
# batch moves it into the other rows' brackets
ACROSS = [(("small<64,4>", "small<64,8>"), "small<64,4>", 256), (("long<128,2>", "long<128,3>", "long<128,8>"), "long<128,2>", 300)]


@pytest.mark.parametrize("rows,source,companion", ACROSS, ids=["small64_4_vs_8", "long128_2_vs_3_vs_8"])
@pytest.mark.parametrize("nh,nkv", AC.GEOMETRIES)
@pytest.mark.parametrize("kind", ["lengths", "masks", "large"])
def test_the_same_sequence_under_other_instantiations(kind, nh, nkv, rows, source, companion, monkeypatch):
    """Compared through the bound only: each instantiation is within the bound of float64 on the shared sequences.  Whether the
    bits agree is printed, not asserted (the instantiations sum the keys in other groupings)."""
    c, d = AC.case(source, kind, nh, nkv), _device_inputs(source, kind, nh, nkv)
    ref, bound = _reference(source, kind, nh, nkv)
    T = sum(c["lens"])
    outs = []
    for row in rows:
        lens, dd = list(c["lens"]), d
        if not (AC.ROWS[row]["lo"] <= max(lens) and (AC.ROWS[row]["hi"] is None or max(lens) <= AC.ROWS[row]["hi"])):
            # the companion: the batch's first sequence repeated to the length asked for, every key valid, appended last
            reps = [(0, c["lens"][0])] * (companion // c["lens"][0] + 1)
            extra = _sub_batch(d, reps)
            dd = {k: (torch.cat([d[k], extra[k][:companion]]) if k in ("qkv", "key_valid", "pos") else d[k]) for k in d}
            dd["key_valid"][T:] = 1
            lens = lens + [companion]
        out = _run(monkeypatch, row, nh, nkv, lens, dd)[:T]
        _check(out, c, ref, bound, f"ACROSS {row} on the batch of {source} {kind} {nh}x{nkv}")
        outs.append(out)
    for row, out in zip(rows[1:], outs[1:]):
        same = torch.equal(_bits(out), _bits(outs[0]))
        print(f"BITS {rows[0]} vs {row} {kind} {nh}x{nkv}: equal {same}, elements that differ {int((_bits(out) != _bits(outs[0])).sum())} of {out.numel()}")
