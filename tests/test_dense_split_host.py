"""CPU: the plane split restated in tests/dense_split_cases.py does what its docstring proves, the two tiers of bounds hold for
ideally rounded arithmetic on every data kind, the closed form of tier B is reached to within a factor of two (so it is not slack
by orders of magnitude), the fitted tolerance it replaces as documentation is exceeded by the arithmetic itself, and the defects the
GPU tests are there for leave tier A.  So a GPU failure means the kernel, not the bound."""
import numpy as np
import pytest
import torch

import dense_split_cases as C

F32 = np.float32
NQ, N = 9, 40


def _f64(*a):
    return [np.asarray(x, np.float64) for x in a]


# ------------------------------------------------------------------------------------------ the split (S)
def test_three_planes_reproduce_v_exactly_where_the_docstring_says():
    v = np.concatenate([C.specials(), C.split_vector(1 << 16)])
    p0, p1, p2 = C.split_planes(v)
    for p in (p0, p1, p2):
        assert np.isfinite(p).all() and not (p.view(np.uint32) & 0xFFFF).any()          # finite bf16 numbers, the top binade included
    x, s = v.astype(np.float64), sum(_f64(p0, p1, p2))
    exact = (np.abs(x) >= 2.0 ** -110) | (x == 0) | (np.ldexp(x, 133) == np.rint(np.ldexp(x, 133)))
    assert exact.sum() > 0.5 * v.size and (~exact).sum() > 100
    assert np.array_equal(s[exact], x[exact])
    assert (np.abs(s - x) <= C.F134).all() and (s != x).any()                           # the floor: what lies under 2^-133 is lost
    # a bf16 number is its own first plane, the others are +0; +-0 keep their sign in p0
    b = C.G.bf16_round(v[np.isfinite(C.G.bf16_round(v))])
    q0, q1, q2 = C.split_planes(b)
    assert np.array_equal(q0.view(np.uint32), b.view(np.uint32)) and not q1.view(np.uint32).any() and not q2.view(np.uint32).any()
    z = C.split_planes(np.array([0.0, -0.0], F32))
    assert [p.view(np.uint32).tolist() for p in z] == [[0, 0x80000000], [0, 0], [0, 0]]


def test_top_binade_saturates_and_the_unsaturated_split_does_not_survive_it():
    top = np.array([0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF], np.uint32).view(F32)          # below the boundary, on it (a tie: to even = inf), FLT_MAX
    assert np.isinf(C.G.bf16_round(top)).tolist() == [False, True, True]
    assert np.isinf(torch.from_numpy(top).to(torch.bfloat16).float().numpy()).tolist() == [False, True, True]       # torch's cast agrees
    raw = C.split_planes(top, saturate=False)
    assert np.isinf(raw[0][1:]).all() and np.isinf(raw[1][1:]).all() and np.isnan(raw[2][1:]).all()
    p = C.split_planes(np.concatenate([top, -top]))
    assert (p[0] == np.concatenate([np.full(3, C.BF16_MAX), np.full(3, -C.BF16_MAX)])).all()
    assert np.array_equal(sum(_f64(*p)), np.concatenate([top, -top]).astype(np.float64))
    assert (np.abs(p[1][1:3]) < 2.0 ** 120).all() or p[1][2] == 2.0 ** 120          # r1 < 2^120; FLT_MAX's rounds up to 2^120, finite
    assert C.plane_words(p[0]).tolist()[:3] == [0x7F7F] * 3


def test_residual_subtractions_are_exact_with_float64_as_witness():
    v = np.concatenate([C.specials(), C.split_vector(1 << 16)])
    p0, p1, _ = C.split_planes(v)
    r1 = (v - p0).astype(F32)
    r2 = (r1 - p1).astype(F32)
    assert np.array_equal(r1.astype(np.float64), v.astype(np.float64) - p0.astype(np.float64))
    assert np.array_equal(r2.astype(np.float64), r1.astype(np.float64) - p1.astype(np.float64))


def test_residual_bounds_of_the_split():
    v = np.concatenate([C.specials(), C.split_vector(1 << 16)])
    a = np.abs(v.astype(np.float64))
    r1, r2, r3 = C.residuals(v)
    p0, p1, _ = (np.abs(p.astype(np.float64)) for p in C.split_planes(v))
    assert (r1 <= np.maximum(2.0 ** -8 * a, C.F134)).all()
    assert (r2 <= np.maximum(2.0 ** -17 * (1 + 2.0 ** -8) * a, C.F134)).all()
    assert (r3 <= C.F134).all() and not r3[a >= 2.0 ** -110].any()
    assert (p0 <= (1 + 2.0 ** -8) * a + C.F134).all() and (p1 <= 2.0 ** -8 * (1 + 2.0 ** -8) * a + 2 * C.F134).all()
    # the bounds are reached: rho1 at a tie, rho2 by the `aligned` element (half of 2^-16 |v|, not more)
    assert C.residuals(np.array([1 + 2.0 ** -8], F32))[0][0] == 2.0 ** -8
    al = C.residuals(np.array([1 + 0.998 * 2.0 ** -8], F32))
    assert 0.99 * 2.0 ** -8 < al[0][0] and 0.95 * 2.0 ** -17 < al[1][0] <= 2.0 ** -17


# ------------------------------------------------------------------------------------------ tier B
def _planes(Q, D):
    return C.split_planes(Q), C.split_planes(D)


@pytest.mark.parametrize("H", C.HOST_H)
@pytest.mark.parametrize("kind", C.KINDS)
def test_tier_b_residual_and_closed_form_hold(kind, H):
    Q, D = C.case(kind, H, N, NQ)
    qp, dp = _planes(Q, D)
    qd, aqd = C.exact_product(Q, D)
    for mode in C.MODES:
        T, dA = C.tier_a(qp, dp, mode)
        K = len(C.PAIRS[mode]) * H
        f64 = 4 * K * 2.0 ** -53 * aqd                  # float64's own summation error, in T and in q.d
        err = np.abs(T - qd)
        res, closed = C.tier_b_residual(Q, D, mode), C.tier_b_closed(Q, D, mode)
        assert (err <= res + f64).all(), (kind, H, mode, float((err / (res + f64 + 1e-300)).max()))
        assert (res <= closed * (1 + 1e-12)).all(), (kind, H, mode)
        assert (dA <= K * C.E * (1 + 2.0 ** -5) * aqd + K * C.E * C.tier_b_floor(Q, D)).all()       # the header's form of dA
        if kind == "bf16_exact":                         # T is the exact product, tier B is 0, the modes agree
            assert not res.any() and not any(p.any() for p in qp[1:] + dp[1:])
            assert (err <= f64).all()
        if kind == "zeros":
            zp = C.zero_pairs(Q, D)
            assert zp.sum() > NQ and not T[zp].any() and not dA[zp].any()
        if kind == "tiny":                               # lo planes bf16-subnormal or gone, products still exact in fp32
            assert (np.abs(dp[1]) < 2.0 ** -126).any() and (dp[2] == 0).mean() > 0.3 and (np.abs(dp[0]) < 2.0 ** -126).any()
            A, W, _ = C.plane_operands(qp, dp, mode)
            pr = A[:, None, :].astype(np.float64) * W[None, :, :].astype(np.float64)
            assert np.array_equal(pr.astype(F32).astype(np.float64), pr)


@pytest.mark.parametrize("H", C.HOST_H + (256,))
def test_aligned_reaches_the_closed_form_and_passes_the_fitted_tolerance(H):
    """The closed form is not slack: `aligned` reaches more than half of it in both modes (0.96 of cB sum |q d|).  And the 2.5e-6 |q| |d|
    that tests/test_dense_bf16x3_gpu.py asserts on Gaussian data is not a property of the arithmetic: the restated plane sum itself is
    8 times that away from the true product here."""
    Q, D = C.case("aligned", H, N, NQ)
    qp, dp = _planes(Q, D)
    qd, aqd = C.exact_product(Q, D)
    nq, nd = np.linalg.norm(Q.astype(np.float64), axis=1), np.linalg.norm(D.astype(np.float64), axis=1)
    for mode in C.MODES:
        err = np.abs(C.tier_a(qp, dp, mode)[0] - qd)
        reach = float((err / C.tier_b_closed(Q, D, mode)).max())
        unit = 16 if mode == "bf16x3" else 24
        print(f"aligned H {H} {mode}: |T - q.d| reaches {reach:.3f} of the closed form, {float((err / aqd).max()) * 2.0 ** unit:.3f} x 2^-{unit} "
              f"sum |q d|, {float((err / (nq[:, None] * nd[None, :])).max()):.3g} |q||d|")
        assert 0.5 <= reach <= 1.0
    err3 = np.abs(C.tier_a(qp, dp, "bf16x3")[0] - qd)
    assert (err3 > C.FITTED_TOL["bf16x3"] * nq[:, None] * nd.max()).any()
    assert float((err3 / (nq[:, None] * nd[None, :])).max()) > 4 * C.FITTED_TOL["bf16x3"]
    # Gaussian data stays far inside it: why the fitted figure passes on the inputs it was fitted to
    Qg, Dg = C.case("gauss", H, N, NQ)
    eg = np.abs(C.tier_a(*_planes(Qg, Dg), "bf16x3")[0] - C.exact_product(Qg, Dg)[0])
    ng = np.linalg.norm(Qg.astype(np.float64), axis=1)[:, None] * np.linalg.norm(Dg.astype(np.float64), axis=1)[None, :]
    assert float((eg / ng).max()) < C.FITTED_TOL["bf16x3"]


# ------------------------------------------------------------------------------------------ tier A
def _fp32_chain(A, W, order):
    """The plane products summed in fp32, one rounding per addition, in the given order of the K terms."""
    pr = (A[:, None, :] * W[None, :, :]).astype(F32)              # exact
    acc = np.zeros(pr.shape[:2], F32)
    for k in order:
        acc = (acc + pr[:, :, k]).astype(F32)
    return acc


@pytest.mark.parametrize("kind", C.KINDS)
def test_fp32_summation_in_any_order_stays_inside_tier_a(kind):
    rng = np.random.default_rng(3)
    for H in (64, 192):
        Q, D = C.case(kind, H, N, NQ)
        qp, dp = _planes(Q, D)
        for mode in C.MODES:
            A, W, K = C.plane_operands(qp, dp, mode)
            T, dA = C.tier_a(qp, dp, mode)
            worst = 0.0
            for order in (np.arange(K), rng.permutation(K), np.argsort(-np.abs(A[0] * W[0]), kind="stable")):
                s = _fp32_chain(A, W, order)
                assert (np.abs(s.astype(np.float64) - T) <= dA).all(), (kind, H, mode)
                worst = max(worst, C.ratio(s, T, dA))
                if kind == "zeros":
                    assert not s[C.zero_pairs(Q, D)].view(np.uint32).any()        # exactly +0
            assert worst <= 1.0
            pw = (A[:, None, :] * W[None, :, :]).astype(F32).sum(axis=2, dtype=F32)          # numpy's pairwise sum
            assert (np.abs(pw.astype(np.float64) - T) <= dA).all()


def _mutant(qp, dp, mode, H, what):
    """The plane sum of a defective kernel, float64: the defects test_dense_split_gpu.py is there for."""
    pairs = list(C.PAIRS[mode])
    if what == "wrong_pairing":                   # two query planes of the pair list exchanged: (d0,q2) (d1,q1) -> (d0,q1) (d1,q2) / (d1,q0) (d0,q1) -> (d1,q1) (d0,q0)
        i, j = (1, 2) if mode == "bf16x6" else (0, 1)
        pairs[i], pairs[j] = (pairs[i][0], pairs[j][1]), (pairs[j][0], pairs[i][1])
    T = 0.0
    for n, (b, a) in enumerate(pairs):
        q, d = qp[a].astype(np.float64), dp[b].astype(np.float64).copy()
        if what == "dropped_slice" and n == len(pairs) - 1:
            d[:, H - 64:] = 0                       # the last k-step of the last pair never added
        if what == "doubled_slice" and n == len(pairs) - 1:
            d[:, :64] *= 2
        if what == "switch_early" and n + 1 < len(pairs):
            d[:, H - 64:] = dp[pairs[n + 1][0]][:, H - 64:]         # the last k-step of a pair already reads the next pair's planes
            q = q.copy()
            q[:, H - 64:] = qp[pairs[n + 1][1]][:, H - 64:]
        if what == "neighbour_row":
            d = np.roll(d, 1, axis=0)
        T = T + q @ d.T
    return T


@pytest.mark.parametrize("what", ["wrong_pairing", "dropped_slice", "doubled_slice", "switch_early", "neighbour_row"])
def test_kernel_defects_leave_tier_a(what):
    for mode in C.MODES:
        seen = []
        for kind in ("gauss", "aligned", "wide", "tiny"):
            for H in (64, 192):
                Q, D = C.case(kind, H, N, NQ)
                qp, dp = _planes(Q, D)
                T, dA = C.tier_a(qp, dp, mode)
                bad = np.abs(_mutant(qp, dp, mode, H, what) - T) > dA
                seen.append(float(bad.mean()))
        assert max(seen) > 0.9, (what, mode, seen)                 # at least one kind sees it on nearly every pair
        assert sum(s > 0.5 for s in seen) >= 2, (what, mode, seen)


def test_reordering_two_pairs_is_not_a_defect():
    """Exchanging the query planes of bf16x6's products 2 and 3, (d1,q1) and (d1,q0), only reorders the list: they share the document
    plane.  The sum is the same, and no bound on the value can or should tell the two orders apart."""
    pd, pq = [b for b, _ in C.PAIRS["bf16x6"]], [a for _, a in C.PAIRS["bf16x6"]]
    assert pd[2] == pd[3]
    pq[2], pq[3] = pq[3], pq[2]
    assert sorted(zip(pd, pq)) == sorted(C.PAIRS["bf16x6"])


# ------------------------------------------------------------------------------------------ the two routes of the references
def test_torch_route_of_the_references_equals_the_numpy_route():
    for kind in ("gauss", "wide", "tiny"):
        Q, D = C.case(kind, 192, N, NQ)
        qp, dp = _planes(Q, D)
        tq, td = [torch.from_numpy(p) for p in qp], [torch.from_numpy(p) for p in dp]
        for mode in C.MODES:
            T, dA = C.tier_a(qp, dp, mode)
            Tt, dAt = C.tier_a(tq, td, mode)
            K = len(C.PAIRS[mode]) * 192
            assert (np.abs(Tt.numpy() - T) <= 4 * K * 2.0 ** -53 * (dA / (K * C.E))).all()
            np.testing.assert_allclose(dAt.numpy(), dA, rtol=1e-12, atol=0)
            np.testing.assert_allclose(C.tier_b_closed(torch.from_numpy(Q), torch.from_numpy(D), mode).numpy(), C.tier_b_closed(Q, D, mode),
                                       rtol=1e-12, atol=0)
            assert C.ratio(Tt, Tt + dAt / 2, dAt) == pytest.approx(0.5) and C.ratio(T, T + dA / 2, dA) == pytest.approx(0.5)
