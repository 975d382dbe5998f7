"""CPU: the error bound of tests/attention_cases.py, which test_attention_bf16_gpu.py holds every kernel of csrc/attention.hip to,
is checked against itself here, without a kernel:

  * it holds for ideal arithmetic - the float64 reference with P rounded to bf16 (round to nearest even) and the output
    rounded to bf16, P rounded normalised (small and rope kernels) and unnormalised-then-divided (long kernel) - on every
    element of every case of every kernel row, nothing excluded;
  * it discriminates - each of a list of kernel defects, applied to that rounded reference, puts at least one element of
    every batch that contains the defect's feature outside the bound."""
import pytest
import torch

import attention_cases as AC

COMBOS = [(row, nh, nkv) for row in AC.ROWS for nh, nkv in AC.GEOMETRIES]
combos = pytest.mark.parametrize("row,nh,nkv", COMBOS, ids=[f"{r}-{a}x{b}" for r, a, b in COMBOS])


def test_rne_bf16_is_the_format_rounding():
    """rne_bf16 (float64 in, one rounding) against torch's fp32 -> bf16 conversion on fp32 numbers, ties included."""
    g = torch.Generator().manual_seed(1)
    x = torch.cat([torch.randn(100000, generator=g), torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 0.0, -0.0, 255.5, 2.0 ** -30])])
    assert torch.equal(AC.rne_bf16(x.double()), x.bfloat16().double())
    assert float(AC.rne_bf16(torch.tensor(1.0 + 2.0 ** -8, dtype=torch.float64))) == 1.0          # the tie that gives u = 2^-8


def test_the_cases_are_what_they_say():
    for row, r in AC.ROWS.items():
        for kind in ("lengths", "masks"):
            c = AC.case(row, kind, 2, 1)
            longest = max(c["lens"])
            assert c["lens"][0] != longest and 0 in c["lens"][1:-1] and r["lo"] <= longest and (r["hi"] is None or longest <= r["hi"])
        c = AC.case(row, "masks", 2, 1)
        v = c["qkv"][:, 3 * r["hd"]:].float()
        assert bool((v[c["key_valid"] == 0] == AC.MASKED_V).all()) and int((c["key_valid"] == 0).sum()) > 0
        assert bool(AC.fully_masked_rows(c).any())
        if r["rope"]:
            assert set(c["cos"].unique().tolist()) == {-1.0, 0.0, 1.0} and bool((c["cos"].abs() + c["sin"].abs() == 1).all())
            assert bool((c["pos"][1:] < c["pos"][:-1]).any())


@combos
@pytest.mark.parametrize("kind", AC.KINDS)
def test_the_bound_holds_for_ideally_rounded_arithmetic(kind, row, nh, nkv):
    c = AC.case(row, kind, nh, nkv)
    forms = (None, "normalised", "unnormalised")
    T = sum(c["lens"])
    ref, bound = torch.zeros((T, nh * c["hd"]), dtype=torch.float64), torch.zeros((T, nh * c["hd"]), dtype=torch.float64)
    outs = {f: torch.full_like(ref, float("nan")) for f in forms[1:]}
    for t0, n, os_, b in AC.compute(c, forms=forms, want_bound=True):
        ref[t0:t0 + n], bound[t0:t0 + n] = os_[0], b
        for f, o in zip(forms[1:], os_[1:]):
            outs[f][t0:t0 + n] = o
    dead = AC.fully_masked_rows(c)
    assert bool((bound[dead] == 0).all()) and (kind == "known" or bool((bound[~dead] > 0).all()))     # `known`: v has zeros
    for f in forms[1:]:
        assert bool(((outs[f] - ref).abs() <= bound).all()), (f, AC.worst_ratio(outs[f], ref, bound))  # NaN (unwritten) fails too


def _leaves_the_bound(c, form, defect):
    """None when no sequence of the batch contains the defect's feature; else whether an element of one leaves the bound."""
    found = None
    for t0, n, o, _ in AC.compute(c, form=form, defect=defect):
        found = False
        (_, _, ref, bound), = AC.compute(c, want_bound=True, only_t0=t0)
        if bool(((o - ref).abs() > bound).any()):
            return True
    return found


@combos
@pytest.mark.parametrize("kind", ["lengths", "masks", "large"])
def test_the_bound_rejects_each_defect(kind, row, nh, nkv):
    c = AC.case(row, kind, nh, nkv)
    form = "unnormalised" if row.startswith("long") else "normalised"
    must = {"drop_last_key", "exp2_of_ln", "swap_key_blocks"}
    if nkv > 1:
        must.add("kv_head_off_by_one")
    if kind == "masks":
        must |= {"unmask_first", "unmask_edge", "unmask_last", "masked_row_is_mean_v"}
    if AC.ROWS[row]["rope"]:
        must.add("rope_partner_next")
    for defect in AC.DEFECTS:
        if defect in ("kv_head_off_by_one", "rope_partner_next") and defect not in must:
            continue
        got = _leaves_the_bound(c, form, defect)
        assert (got is not None) == (defect in must), f"{defect}: the batch {'lacks' if got is None else 'has'} the feature"
        assert got is None or got, f"{defect} stays within the bound"
