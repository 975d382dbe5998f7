"""CPU: the stage-1 key model of the certified sparse scorer (tests/sparse_cert_cases.py) against the documented bound, the
certificate's cut against the oracle's top-k, and seeded kernel defects against the model-vs-kernel tolerance (K) - on the adversarial
cases the GPU tests run (test_sparse_cert_kernels_gpu.py).  No kernel runs here: this file shows that the bound holds where it is
tight and that (K) is narrow enough to see a defect, so that a GPU failure of (K) means the kernel and not the bound."""
import numpy as np
import pytest

import sparse_cert_cases as C
from oracle import scoring as O

CASES = {c["name"]: c for c in C.host_cases()}


@pytest.fixture(scope="module")
def modelled():
    """name -> (case, index model, plan model, {q: (R, y)}), computed once and left unchanged."""
    out = {}
    for name, case in CASES.items():
        ix, plan = C.models(case)
        out[name] = (case, ix, plan, {q: C.key_model(ix, plan, q) for q in range(case["nq"]) if plan["elig"][q]})
    return out


def _key_range(R, y, T):
    tol = C.key_tolerance(y, T)
    return np.ceil(R + y - tol), np.floor(R + y + tol)              # the integers (K) admits


@pytest.mark.parametrize("name", list(CASES))
def test_key_model_lies_inside_the_documented_bound(modelled, name):
    case, ix, plan, keys = modelled[name]
    assert len(keys) >= 1
    for q, (R, y) in keys.items():
        tf = C.true_fix(ix, plan, case["qi"], case["qc"], case["qv"], q)
        lo, hi = C.bound(tf, ix["T"], int(plan["n_rare"][q]), int(plan["n_drop"][q]))
        k_lo, k_hi = _key_range(R, y, ix["T"])
        assert (k_lo >= lo).all(), (name, q, float((lo - k_lo).max()))
        assert (k_hi <= hi).all(), (name, q, float((k_hi - hi).max()))
        assert k_hi.max() <= C.saturation_limit(ix["T"], int(plan["n_rare"][q])) < 65535
        assert (R[case["N"]:] == 0).all() and (y[case["N"]:] == 0).all()         # the last tile's padding


@pytest.mark.parametrize("name", list(CASES))
def test_cut_from_the_kth_key_excludes_no_document_of_the_oracles_top_k(modelled, name):
    """Worst case inside (K): the k-th key as high as (K) lets it be, every document's key as low.  Ties at the oracle's k-th score
    count as top-k."""
    case, ix, plan, keys = modelled[name]
    k, N = case["k"], case["N"]
    checked = 0
    for q, (R, y) in keys.items():
        cols, v = case["qc"][case["qi"][q]:case["qi"][q + 1]], case["qv"][case["qi"][q]:case["qi"][q + 1]]
        fi, neg = O.numba_score_float(case["indptr"], case["ids"], case["vals"], cols, v, 0.0, N)
        if len(fi) < k:
            continue
        _, es = O.select_topk(fi, neg, k)
        top = fi[-neg >= es[-1]]
        k_lo, k_hi = _key_range(R[:N], y[:N], ix["T"])
        kth = np.sort(k_hi)[-k]
        cut = C.cut_from_kth(kth, ix["T"], int(plan["n_rare"][q]), int(plan["n_qt"][q]), int(plan["n_drop"][q]))
        assert cut <= kth
        if cut >= 1.0:
            assert (k_lo[top] >= cut).all(), (name, q, cut, float(k_lo[top].min()))
            checked += 1
    assert checked >= 1


def test_cut_mirror_is_monotone_and_below_its_argument():
    for T, nr, nq, nd in [(16, 0, 1, 0), (64, 64, 80, 3), (128, 256, 256, 17)]:
        cuts = [C.cut_from_kth(K, T, nr, nq, nd) for K in range(0, 65536, 97)]
        assert all(b >= a for a, b in zip(cuts, cuts[1:])) and all(c < K for c, K in zip(cuts, range(0, 65536, 97)))


def test_saturated_document_stays_in_its_half_word():
    case, ix, plan = C.saturation_case(), *C.models(C.saturation_case())
    star = case["star"]
    for q in range(3):
        R, y = C.key_model(ix, plan, q)
        top = R[star] + y[star]
        limit = C.saturation_limit(ix["T"], int(plan["n_rare"][q]))
        assert 0.975 * 65535 <= top and top + C.key_tolerance(y[star], ix["T"]) <= limit < 65535 - 900, (q, top, limit)
        assert (R + y).argmax() == star
    # query 0 (rare terms only): the even neighbour in the same LDS word holds one posting of one term - its key is that posting alone
    R, y = C.key_model(ix, plan, 0)
    j = list(plan["rare_term"][0]).index(16)
    v16 = np.float16(np.float32(0.37) * ix["vscale"]).astype(np.float32)
    assert y[star - 1] == 0 and R[star - 1] == int(np.uint32(v16 * plan["rare_w"][0, j] + np.float32(1.0)))


def test_drop_boundary_plan():
    case = C.drop_boundary_case()
    ix, plan = C.models(case)
    for q, want in enumerate(case["expect_drop"]):
        if want is None:
            assert plan["elig"][q] == 0 and plan["reason"][q] == case["expect_reason"][q]
        else:
            assert plan["elig"][q] == 1 and plan["n_drop"][q] == want, (q, plan["reason"][q], plan["n_drop"][q])
    w = plan["rare_w"][7, :2]                                       # the rare-only query just under 6e4
    assert plan["n_rare"][7] == 2 and 5.85e4 < w.max() < 6.0e4
    near = plan["rare_w"][[1, 2, 3, 4]][:, :4]
    assert (near[:2] == 0).all() and (near[2:] >= C.W_DROP).all() and near[2:].max() < 6.6e-5


def test_plan_model_names_every_way_off_the_fast_path():
    case = C.off_path_case()
    ix, plan = C.models(case)
    assert plan["reason"][:case["nq"]] == case["expect_reason"]
    assert plan["n_qt"][8] == 2 and plan["n_rare"][8] + (plan["B"][8] != 0).sum() == 1
    too_many = C.plan_model(ix, *C._queries([(np.arange(130, 130 + 250), np.ones(250))]))
    assert too_many["reason"][0] == "" and too_many["n_rare"][0] == 250            # 256 is the limit of a query's length as well


def test_subnormal_budget_turns_a_query_down():
    case = C.subnormal_case()
    ix, plan = C.models(case)
    assert plan["reason"][:4] == ["", "", "", "subnormal budget"] and plan["cq"][0] == np.float32(2.0 ** -24)
    assert float(ix["vscale"]) == 2.0 ** 13 and np.float16(C.SUB_MAX * 2.0 ** 13) == np.float16(2.0 ** -14) - np.float16(2.0 ** -24)


def test_uncertifiable_queries_fail_the_certificates_conditions():
    case = C.uncertifiable_case()
    ix, plan = C.models(case)
    R, y = C.key_model(ix, plan, 0)
    assert len(np.unique((R + y)[:case["N"]])) == 1                                  # one key for every doc: nothing separates k from k + band
    R, y = C.key_model(ix, plan, 1)
    assert ((R + y)[:case["N"]] > 0).sum() == 3 < case["k"]


def test_dense_slot_count_rounds_as_the_build_does():
    assert [C.round_T(130, cap)[1] for cap in C.KS_CAPS] == [C.EXPECTED_T[cap] for cap in C.KS_CAPS]
    assert C.round_T(130, 48) == (48, 64) and C.round_T(0, 128) == (0, 16) and C.round_T(33, 128) == (33, 64) and C.round_T(200, 1000) == (128, 128)
    assert C.round_T(130, 47) == (32, 32) and C.round_T(130, 5) == (16, 16)


@pytest.mark.parametrize("name", ["runs[9 tiles,integer]", "forward rows[1024]", "KS[T cap 48]"])
def test_index_model_structures_describe_the_index(modelled, name):
    """The tables decoded back: every (term, tile) run of P that S and E point at is the term's postings inside the tile; d16 holds the
    dense terms' values at the MFMA fragment position of (doc, slot); the forward rows are the docs' postings by ascending term."""
    case, ix, plan, _ = modelled[name]
    P, S, E = ix["P"], ix["S"], ix["E"]
    for t in range(ix["V"]):
        b, e = ix["indptr"][t], ix["indptr"][t + 1]
        assert S[t, 0] == b and S[t, -1] == e
        for i in range(ix["n_tiles"]):
            docs = ix["ids"][S[t, i]:S[t, i + 1]]
            assert ((docs >= i * C.DT) & (docs < (i + 1) * C.DT)).all()
            w = int(E[t, i])
            n = len(docs)
            assert (w == 0) if n == 0 else (w == int(P[S[t, i]]) | 2 and w >> 16 != 0xffff) if n == 1 else (w == (0xffff0000 | n))
        assert (E[t, ix["n_tiles"]:] == 0).all()
    dl = (P[:ix["nnz"]] & 0xfffc) // 2 + (P[:ix["nnz"]] & 1)
    assert np.array_equal(dl, ix["ids"] % C.DT) and np.array_equal((P[:ix["nnz"]] >> 16).astype(np.uint16).view(np.float16), ix["v16"])
    back = ix["d16"].reshape(ix["n_tiles"], 32, ix["KS"], 2, 32, 8).transpose(0, 1, 4, 2, 3, 5).reshape(ix["n_tiles"] * C.DT, ix["T"])
    assert np.array_equal(back, ix["A"]) and (ix["A"][:, ix["n_heavy"]:] == 0).all()
    for d in range(0, case["N"], 97):
        row = ix["fwd_tv"][ix["fwd_indptr"][d]:ix["fwd_indptr"][d + 1]]
        terms = (row >> np.uint64(32)).astype(np.int64)
        assert (np.diff(terms) > 0).all() and np.array_equal(terms, np.flatnonzero([d in ix["ids"][ix["indptr"][t]:ix["indptr"][t + 1]] for t in range(ix["V"])]))


DEFECTS = [("drop_tail_posting", "runs[9 tiles,integer]"), ("drop_tail_posting", "runs[10 tiles,real]"), ("drop_tail_posting", "groups[real]"),
           ("other_half", "runs[9 tiles,integer]"), ("other_half", "saturation"),
           ("e_one_tile_late", "runs[10 tiles,real]"), ("e_one_tile_late", "midpoints"),
           ("ring_fragment_ahead", "runs[9 tiles,integer]"), ("ring_fragment_ahead", "KS[T cap 48]"), ("ring_fragment_ahead", "KS[T cap 128]"),
           ("skip_group1_term", "groups[integer]"), ("skip_group1_term", "groups[real]")]


@pytest.mark.parametrize("defect,name", DEFECTS)
def test_seeded_kernel_defects_leave_the_key_tolerance(modelled, defect, name):
    """A kernel with the defect returns keys within (K) of the DEFECTIVE model; they are told from the sound model's keys wherever the two
    models differ by more than both tolerances together."""
    case, ix, plan, keys = modelled[name]
    seen = 0
    for q, (R, y) in keys.items():
        Rd, yd = C.key_model(ix, plan, q, defect=defect)
        seen += int((np.abs((Rd + yd) - (R + y)) > C.key_tolerance(y, ix["T"]) + C.key_tolerance(yd, ix["T"])).sum())
    assert seen >= 1, (defect, name)
