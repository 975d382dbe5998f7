"""CPU: the bounds of tests/fp32_plane_cases.py hold for ideally rounded arithmetic (float64 products rounded once, then numpy
fp32 with exactly the kernel's roundings) on every case test_fp32_planes_gpu.py runs, and each of a list of kernel defects
leaves them.  So a GPU failure means the kernel, not the bound - and the checks can see the defects they are there for."""
import numpy as np
import pytest

import fp32_plane_cases as C


# ------------------------------------------------------------------------------------------ row split
@pytest.mark.parametrize("K", C.SPLIT_K)
def test_split_restatement_holds_its_own_properties(K):
    for T in C.SPLIT_T:
        c = C.split_case(K, T)
        for nseg in (2, 3):
            planes, inv = C.act_planes(c["x"], nseg)
            assert C.check_split_exact(c["x"], nseg, planes, inv) == [], (K, T, nseg)
            y = C.norm_ideal(c["x"], c["w"], c["eps"])
            planes, inv = C.act_planes(y, nseg)
            assert C.check_split_norm(c["x"], c["w"], c["eps"], nseg, planes, inv) == [], (K, T, nseg)
            g = C.norm_ideal(c["embed"][c["tok"]], c["w"], c["eps"])
            planes, inv = C.act_planes(g, nseg)
            assert C.check_split_norm(c["embed"][c["tok"]], c["w"], c["eps"], nseg, planes, inv) == [], (K, T, nseg)


def test_split_edges_are_what_they_claim():
    c = C.split_case(320, 9)
    x, names = c["x"], c["edge_names"]
    assert sorted(names) == ["below_pow2", "denormal", "outlier", "pow2_in_tail", "zero"]
    r = {n: x[i] for i, n in enumerate(names)}
    assert not r["zero"].any()
    assert np.abs(r["pow2_in_tail"]).argmax() == 319 and np.abs(r["pow2_in_tail"]).max() == 4.0       # in the last K % 256 tail
    assert np.abs(r["below_pow2"]).max() == np.nextafter(np.float32(4), np.float32(0))
    assert 0 < np.abs(r["denormal"]).max() < np.finfo(np.float32).tiny
    o = np.sort(np.abs(r["outlier"]))
    assert o[-1] >= 2.0 ** 18 * o[-2]
    # an exact power of two lands on 2^14, one ulp below it just under 2^15
    _, inv = C.act_planes(np.stack([r["pow2_in_tail"], r["below_pow2"]]), 2)
    assert inv[0] == 2.0 ** -12 and inv[1] == 2.0 ** -13
    assert C.split_case(64, 1)["edge_names"] == ["pow2_in_tail"]


@pytest.mark.parametrize("defect", ["low_dropped", "third_from_low", "scale_off_at_pow2"])
def test_split_defects_are_seen(defect):
    c = C.split_case(320, 9)
    planes, inv = C.act_planes(c["x"], 3, defect=defect)
    assert C.check_split_exact(c["x"], 3, planes, inv) != []
    if defect != "scale_off_at_pow2":         # with a norm the kernel's own maximum may sit either side of a power of two: no claim
        y = C.norm_ideal(c["x"], c["w"], c["eps"])
        planes, inv = C.act_planes(y, 3, defect=defect)
        assert C.check_split_norm(c["x"], c["w"], c["eps"], 3, planes, inv) != []


def test_cmax_and_act_scale_checks():
    c = C.loose_case(32)
    true, p = C.cmax_reference(c["W"], c["w_inv"], 3)
    assert p.argmax() == 7 and len(p) == c["I"]
    ideal = np.float32(true * 1.001)
    assert C.check_cmax(ideal, c["W"], c["w_inv"], 3) == []
    assert C.check_cmax(np.float32(true * 0.999), c["W"], c["w_inv"], 3) != []            # not a bound
    assert C.check_cmax(np.float32(np.sort(p)[-2] * 1.001), c["W"], c["w_inv"], 3) != []  # a pair missed
    y, _ = C.norm_reference(c["x"], c["wn"], c["eps"])
    B = ((y * y).sum(axis=1) * float(ideal) * 1.02).astype(np.float32)
    sc = C.row_scale_pow2(B)
    assert C.check_act_scale(c["x"], c["wn"], c["eps"], ideal, sc, np.float32(1) / sc) == []
    assert C.check_act_scale(c["x"], c["wn"], c["eps"], ideal, sc * np.float32(2), np.float32(0.5) / sc) != []
    assert C.check_act_scale(c["x"], c["wn"], c["eps"], ideal, sc, np.float32(0.5) / sc) != []


# ------------------------------------------------------------------------------------------ GEMM epilogues
def _cases(epi):
    return C.epilogue_cases(epi)


@pytest.mark.parametrize("name", list(C.EPILOGUES))
def test_ideal_arithmetic_is_inside_every_bound(name):
    worst = 0.0
    for c in _cases(C.EPILOGUES[name]):
        out = C.gemm_ideal(c)
        assert C.check_gemm(c, out) == [], {k: c[k] for k in ("epi", "M", "N", "nseg", "K0")}
        worst = max(worst, C.worst_ratio(c, out))
    print(f"{name}: ideal arithmetic reaches {worst:.3f} of the bound")
    assert worst <= 1.0


@pytest.mark.parametrize("defect,name", [(d, n) for d, epis in C.GEMM_DEFECTS.items() for n, e in C.EPILOGUES.items() if e in epis])
def test_gemm_defects_leave_the_bound(defect, name):
    epi = C.EPILOGUES[name]
    seen = 0
    for c in _cases(epi):
        if defect.startswith("row0") and c["M"] <= 256:
            continue
        if defect == "bias_after_rotation" and c.get("bias") is None:
            continue
        if defect == "third_from_low" and c["out_nseg"] != 3:
            continue
        if defect == "masked_row_in_max" and not (c["seq_of"] == -2).any():
            continue
        # (G) is a worst-case bound, K' e sum |a w|, and grows with K' against a sum that cancels: beyond 5 k-steps it is wider than
        # the 2^-12 a dropped low plane costs, so that defect is asked of the short chains only (every shape has them)
        if defect == "low_plane_dropped" and c["K"] > 320:
            continue
        assert C.check_gemm(c, C.gemm_ideal(c, defect=defect)) != [], (defect, {k: c[k] for k in ("epi", "M", "N", "nseg", "K0")})
        seen += 1
    assert seen >= 1


def test_segmax_case_has_what_the_kernel_can_get_wrong():
    c = C.gemm_case(C.EPI_SEGMAX, 300, 320, 3, 64)
    ids = c["seq_of"]
    live = ids[ids >= 0]
    assert np.all(np.diff(live) >= 0) and (ids == -2).sum() > 10
    assert (ids == 0).sum() == 1 and (ids == 1).sum() > 150            # a sequence of 1 token next to a long one
    # sequence 1 crosses the 16-row slabs, the 64- / 128-row tiles and row 256 lies inside sequence 2
    assert ids[15] == ids[16] == 1 and ids[127] == ids[128] == 1 and ids[254] == ids[257] == 2
    ref, bound, zero = C.gemm_reference(c)
    assert zero[:3, 5].all() and zero[3].all() and not zero[:3].all()
    T, _ = C._products(c)
    assert np.abs(T[ids == -2]).max() > 8 * np.abs(T[ids >= 0]).max()   # the masked rows carry the largest values


def test_swiglu_case_reaches_large_gates_of_both_signs():
    c = C.gemm_case(C.EPI_SWIGLU, 17, 128, 3, 64)
    T, _ = C._products(c)
    G, _ = C._deinterleave(T)
    assert G.max() > 95 and G.min() < -95            # expf(-g) overflows fp32 below -88.7: the kernel's -0 is inside the bound


def test_two_segments_equal_three_with_a_zero_low_plane():
    c2 = C.gemm_case(C.EPI_RESID, 33, 128, 2, 128)
    K0 = c2["K0"]
    hi = c2["W"][:, :K0]
    W3 = np.concatenate([hi, np.zeros_like(hi), hi], axis=1)
    A3 = np.concatenate([c2["A"], c2["A"][:, K0:]], axis=1)
    t2 = c2["A"].astype(np.float64) @ c2["W"].astype(np.float64).T
    assert np.array_equal(t2, A3.astype(np.float64) @ W3.astype(np.float64).T)


# ------------------------------------------------------------------------------------------ the loose bound
@pytest.mark.parametrize("factor", [32, 1024])
def test_loose_case_is_loose(factor):
    """The inputs of the GPU loose-bound test: in the rows whose outlier gate is negative (silu silences the pair that sets the
    bound) B / r is the factor squared times what Gaussian weights give, about 2^5.7: 2^15.7 and 2^25.7."""
    r = C.loose_reference(C.loose_case(factor))
    l2 = np.log2(r["B"] / r["rmax"])
    loose = l2 > C.LOOSE_LOG2[factor]
    print(f"factor {factor}: log2(B / r) = {np.round(np.sort(l2), 1).tolist()}; derived floor 2^{np.median(l2[loose]) - 39:.1f} of the row maximum")
    assert loose.sum() >= len(l2) // 4


def test_fallback_criterion_keeps_the_goldens_and_random_weights_fused(golden_dir):
    """sr_model_finalize's rule in float64 (fused_looseness): every layer of every golden model and Gaussian weights at the 1B / 8B
    widths stay fused, the outlier pair of the model test falls back."""
    import json
    import os

    from golden_weights import make_weights
    for name in ("enc_tiny_a", "enc_hd64", "enc_hd128", "enc_toy_q", "enc_qwen2_hd64", "enc_qwen2_hd128"):
        z = np.load(os.path.join(golden_dir, name + ".npz"))
        cfg = json.loads(str(z["config_json"]))
        w = make_weights(cfg, int(z["weight_seed"]))
        for li in range(cfg["num_hidden_layers"]):
            loose = C.fused_looseness(w[f"model.layers.{li}.mlp.gate_proj.weight"], w[f"model.layers.{li}.mlp.up_proj.weight"], cfg["hidden_size"])
            assert loose < 2.0 ** 15, (name, li, loose)            # a factor of two away from the threshold
    rng = np.random.default_rng(0)
    for H in (2048, 4096):
        wg, wu = rng.standard_normal((512, H)) * 0.02, rng.standard_normal((512, H)) * 0.02
        assert C.fused_looseness(wg, wu, H) < 2.0 ** 13.5
        wg[7] *= 32
        wu[7] *= 32
        assert C.fused_looseness(wg, wu, H) > 2.0 ** 20
