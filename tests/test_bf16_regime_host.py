"""CPU: the bounds of tests/bf16_regime_cases.py hold for ideally rounded arithmetic (float64 products rounded once, then numpy fp32
with exactly the kernel's roundings, bf16 by round to nearest even) on every case test_bf16_regime_gpu.py runs, and each of a list
of kernel defects leaves them on at least one element of at least one case.  So a GPU failure means the kernel, not the bound -
and the checks can see the defects they are there for."""
import numpy as np
import pytest

import bf16_regime_cases as C

F32 = np.float32


# ------------------------------------------------------------------------------------------ format arithmetic
def test_bf16_rounding_restatement_and_its_half_spacing():
    """Round to nearest even on ties, the spacing h of (B) is reached (2^-8 relative at the bottom of a binade) and never passed;
    truncation passes it."""
    one = F32(1)
    assert C.bf16_round(np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20], F32)).tolist() == [1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7]
    assert C.half_spacing(1.0) == 2.0 ** -8 and C.half_spacing(1.999) == 2.0 ** -8 and C.half_spacing(2.0) == 2.0 ** -7
    assert C.half_spacing(2.0 ** -140) == 2.0 ** -134 and C.half_spacing(0.0) == 0.0
    tie = F32(1 + 2.0 ** -8)                            # correct rounding errs by 2^-8 |v| here: more than 2^-9 |v|
    assert abs(float(C.bf16_round(tie).item()) - float(tie)) == 2.0 ** -8 > 2.0 ** -9 * float(tie)
    rng = np.random.default_rng(0)
    v = (rng.standard_normal(20000) * np.exp(rng.uniform(-30, 30, 20000))).astype(F32)
    v[:4] = [2.0 ** -133, 3 * 2.0 ** -135, -2.0 ** -134, 2.0 ** -127]
    err = np.abs(C.bf16_round(v).astype(np.float64) - v)
    assert np.all(err <= C.half_spacing(v))
    assert C.ratio(C.bf16_round(v), v.astype(np.float64), C.half_spacing(v)) <= 1.0
    assert C.ratio(C.bf16_trunc(v), v.astype(np.float64), C.half_spacing(v)) > 1.9
    assert np.array_equal(C.bf16_value(C.bf16_bits(C.bf16_round(v))), C.bf16_round(v)) and one == C.bf16_value(np.array([0x3f80], np.uint16))[0]


# ------------------------------------------------------------------------------------------ RMSNorm
def _norm_outputs(c, combo, defect=None):
    src, d, _ = C.norm_inputs(c, combo)
    back, y, yb = C.norm_ideal(src, d, c["w"], c["eps"], defect=defect, x_before=c["x"])
    return back, yb, y


@pytest.mark.parametrize("H", C.NORM_H)
def test_norm_ideal_arithmetic_is_inside_the_bound(H):
    worst = 0.0
    for T in C.NORM_T:
        c = C.norm_case(H, T)
        for combo in C.NORM_COMBOS:
            back, yb, y = _norm_outputs(c, combo)
            assert C.check_norm(c, combo, back, xn=yb, xn_f32=y) == [], (H, T, combo)
            worst = max(worst, C.norm_ratio(c, combo, xn=yb, xn_f32=y))
    print(f"H {H}: ideal arithmetic reaches {worst:.3f} of the bound")
    assert worst <= 1.0


def test_norm_edges_are_what_they_claim():
    c = C.norm_case(320, 9)
    assert c["edge_names"] == ["eps_row", "cancel", "zero"] and C.norm_case(64, 1)["edge_names"] == ["eps_row"]
    x, d = c["x"], c["delta"]
    assert 0.3 < float((x[0].astype(np.float64) ** 2).mean()) / c["eps"] < 3              # mean(x^2) comparable with eps
    xw = (x[1] + d[1]).astype(F32)
    assert np.abs(xw).max() <= 4 * 2.0 ** -23 * np.abs(x[1]).max() and np.abs(xw).max() > 0   # cancels to a few ulps
    assert not x[2].any() and not d[2].any() and np.signbit(x[2]).any()
    assert not np.all(np.diff(c["tok"]) > 0)                                             # token ids out of order
    assert all(C.NORM_NCH[H] in (0, 1, 2, 4, 8, 12, 16) for H in C.NORM_H) and sorted(set(C.NORM_NCH.values())) == [0, 1, 2, 4, 8, 12, 16]
    assert not (d.view(np.uint32) & 0xFFFF).any()                                        # delta is bf16


@pytest.mark.parametrize("defect,combos", [("eps_outside_root", ["head", "layer"]), ("delta_after_bf16", ["layer", "fold"]),
                                            ("x_not_written_back", ["first_layer", "layer", "fold"]), ("weight_on_bf16_row", ["head", "layer"])])
def test_norm_defects_are_seen(defect, combos):
    for H in (64, 2048):
        c = C.norm_case(H, 9)
        for combo in combos:
            back, yb, y = _norm_outputs(c, combo, defect=defect)
            assert C.check_norm(c, combo, back, xn=yb, xn_f32=y) != [], (defect, H, combo)
    # truncation at the bf16 output
    c = C.norm_case(320, 5)
    back, _, y = _norm_outputs(c, "head")
    assert C.check_norm(c, "head", back, xn=C.bf16_trunc(y)) != []


# ------------------------------------------------------------------------------------------ GEMM epilogues
@pytest.mark.parametrize("name", list(C.EPILOGUES))
def test_gemm_ideal_arithmetic_is_inside_every_bound(name):
    worst = 0.0
    for c in C.epilogue_cases(C.EPILOGUES[name]):
        out = C.gemm_ideal(c)
        assert out.shape == C.out_shape(c)
        assert C.check_gemm(c, out) == [], {k: c[k] for k in ("epi", "M", "N", "K")}
        worst = max(worst, C.worst_ratio(c, out))
    print(f"{name}: ideal arithmetic reaches {worst:.3f} of the bound")
    assert worst <= 1.0


@pytest.mark.parametrize("defect,name", [(d, n) for d, epis in C.GEMM_DEFECTS.items() for n, e in C.EPILOGUES.items() if e in epis])
def test_gemm_defects_leave_the_bound(defect, name):
    """Every defect leaves the bound on at least one element of at least one case - in fact in most cases that can show it."""
    epi = C.EPILOGUES[name]
    seen = tried = 0
    for c in C.epilogue_cases(epi):
        if defect == "bias_after_rotation" and c.get("bias") is None:
            continue
        if defect == "rotation_reaches_v" and c["n_rope"] == c["N"]:
            continue
        tried += 1
        seen += C.check_gemm(c, C.gemm_ideal(c, defect=defect)) != []
    print(f"{defect} on {name}: outside the bound in {seen} of {tried} cases")
    assert seen >= 1
    if defect != "max_not_clamped":      # (that one shows only where a sequence has rows and a column is negative in all of them)
        assert seen >= tried // 2        # not marginal: M = 1 has no neighbour row and no masked row, the other cases show it


def test_segmax_case_has_what_the_kernel_can_get_wrong():
    c = C.gemm_case(C.EPI_SEGMAX, 300, 320, 192)
    ids = c["seq_of"]
    live = ids[ids >= 0]
    assert np.all(np.diff(live) >= 0) and (ids == -2).sum() > 10
    assert (ids == 0).sum() == 1 and (ids == 1).sum() > 150            # a sequence of 1 token next to a long one
    assert ids[15] == ids[16] == 1 and ids[127] == ids[128] == 1 and ids[254] == ids[257] == 2
    zero = C.gemm_reference(c)[2]
    assert zero[:3, 5].all() and zero[3].all() and not zero[:3].all()
    T, _ = C._products(c)
    assert np.abs(T[ids == -2]).max() > 8 * np.abs(T[ids >= 0]).max()   # the masked rows carry the largest values


def test_swiglu_case_reaches_large_gates_of_both_signs():
    c = C.gemm_case(C.EPI_SWIGLU, 17, 128, 192)
    T, _ = C._products(c)
    G, _ = C.P._deinterleave(T)
    assert G.max() > 95 and G.min() < -95            # __expf(-g) overflows fp32 below -88.7: the kernel's -0 is inside the bound
    # the fast path's own term: the restatement against float64, relative to silu, stays inside rel_s
    g = np.linspace(-87, 100, 4001).astype(F32)
    s = C.P._silu(g.astype(np.float64))
    rel = ((2 * np.abs(g) + 2) / (1 + np.exp(g.astype(np.float64))) + 4) * C.E
    assert np.all(np.abs(C.fast_silu(g) - s) <= rel * np.abs(s) + 2.0 ** -119)


# ------------------------------------------------------------------------------------------ dense head
@pytest.mark.parametrize("H", C.HEAD_H)
def test_head_ideal_arithmetic_is_inside_the_bound(H):
    for layout in C.HEAD_LAYOUTS:
        c = C.head_case(H, layout)
        out = C.head_ideal(c)
        assert C.check_head(c, out) == [], (H, layout)
        ref, bound, _ = C.head_reference(c)
        assert C.ratio(out, ref, bound) <= 1.0


def test_head_layouts_are_what_they_claim():
    c = C.head_case(64, "three")
    assert c["span_len"].tolist() == [2, 0, 70] and C.head_reference(c)[2].tolist() == [False, True, False]
    c = C.head_case(64, "three_shifted")
    assert C.head_reference(c)[2].tolist() == [False, False, True] and c["pos"][1] == 0          # shifted positions start at 0
    assert C.head_case(64, "one_empty")["T"] == 0
    assert sorted({len(v) for v in C.HEAD_LAYOUTS.values()}) == [1, 3]
    assert {n for v in C.HEAD_LAYOUTS.values() for _, n, _, _ in v} == {0, 1, 2, 70}


@pytest.mark.parametrize("defect", ["pool_by_span_len", "pool_before_start"])
def test_head_defects_are_seen(defect):
    for H in C.HEAD_H:
        c = C.head_case(H, "three")
        assert C.check_head(c, C.head_ideal(c, defect=defect)) != [], (defect, H)


# ------------------------------------------------------------------------------------------ sparse finish
@pytest.mark.parametrize("n", C.FINISH_N)
def test_finish_ideal_arithmetic_is_inside_the_bound(n):
    c = C.finish_case(n)
    for rb in (0, 1):
        assert C.check_finish(c, rb, C.finish_ideal(c, rb)) == [], (n, rb)


def test_finish_defects_are_seen():
    c = C.finish_case(1000)
    assert (c["v"] == 0).sum() >= 2 and (c["v"] < 0).any() and np.signbit(c["v"]).sum() >= 2
    assert C.check_finish(c, 1, C.finish_ideal(c, 1, defect="no_bf16_rounding")) != []
    assert C.check_finish(c, 0, C.finish_ideal(c, 1)) != []                 # ... and rounding when not asked
    for rb in (0, 1):
        assert C.check_finish(c, rb, C.finish_ideal(c, rb, defect="log_before_scale")) != []
    out = C.finish_ideal(c, 1)
    out[c["v"] <= 0] = -0.0
    assert C.check_finish(c, 1, out) != []                                  # -0 is not +0


# ------------------------------------------------------------------------------------------ plan
def test_plan_reference_on_cases_written_out_by_hand():
    c = dict(B=3, L=5, vocab=10, row_shift=None,
             ids=np.array([[11, 1, 2, 3, -4], [5, 6, 7, 8, 9], [1, 1, 1, 1, 1]], np.int64),
             mask=np.array([[0, 1, 0, 1, 0], [0, 0, 0, 0, 0], [0, 0, 0, 1, 1]], np.int64))
    r = C.plan_reference(c, 0)           # dense: row 0 has 2 keys, pools the last 2 positions, keeps [1, 5)
    assert r["span_start"].tolist() == [1, 0, 3] and r["span_len"].tolist() == [4, 0, 2] and r["pool_start"].tolist() == [3, 0, 3]
    assert r["row_len"].tolist() == [2, 0, 2] and r["cu"].tolist() == [0, 4, 4, 6]
    assert r["tok_id"].tolist() == [1, 2, 3, 0, 1, 1] and r["pos"].tolist() == [1, 2, 3, 4, 3, 4]
    assert r["key_valid"].tolist() == [1, 0, 1, 0, 1, 1] and r["seq_of"].tolist() == [0, 0, 0, 0, 2, 2]
    r = C.plan_reference(c, 1)           # sparse: [first key, last key]
    assert r["span_start"].tolist() == [1, 0, 3] and r["span_len"].tolist() == [3, 0, 2] and r["pool_start"].tolist() == [1, 0, 3]
    assert r["seq_of"].tolist() == [0, -2, 0, 2, 2]
    assert C.plan_reference(c, 2)["seq_of"].tolist() == [0, -2, 0, -2, 2, 2]
    c["row_shift"] = np.array([2, 0, 1], np.int32)
    r = C.plan_reference(c, 0)
    assert r["pool_start"].tolist() == [1, 0, 2] and r["pos"].tolist() == [0, 0, 1, 2, 2, 3]
    c["ids"][0, 1] = 10
    assert C.plan_reference(c, 0)["tok_id"][0] == 9


def test_plan_cases_have_what_the_kernels_can_get_wrong():
    for B in C.PLAN_B:
        c = C.plan_case(B, 65, "zero_rows", True)
        assert not c["mask"][0].any() and not c["mask"][-1].any() and not c["mask"][B // 2].any()
        assert (c["ids"] < 0).any() and (c["ids"] >= c["vocab"]).any()
    c = C.plan_case(5, 130, "left", True)
    first = (c["mask"] != 0).argmax(axis=1)
    assert c["row_shift"][0] > first[0] and np.all(c["row_shift"][1:] <= first[1:])
    c = C.plan_case(5, 130, "holes", False)
    r = C.plan_reference(c, 2)
    assert (r["seq_of"] == -2).any() and c["row_shift"] is None
    # the checks see a wrong cu behind the scan's 256 partitions and an unclamped id
    c = C.plan_case(257, 63, "right", False)
    r = C.plan_reference(c, 1)
    bad = dict(r, cu=r["cu"].copy())
    bad["cu"][-1] -= 1
    assert C.check_plan(c, 1, r) == [] and C.check_plan(c, 1, bad) != []
