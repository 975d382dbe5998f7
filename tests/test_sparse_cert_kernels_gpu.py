"""GPU: the kernels of the certified sparse scorer one by one against the numpy model of tests/sparse_cert_cases.py (its docstring
carries the derivation of every tolerance used here; test_sparse_cert_host.py shows on the CPU that the tolerance sees the seeded
defects).  The stage-1 keys of EVERY (query, doc) pair come from sr_sparse_index_cert_debug, every other buffer from
sr_sparse_index_cert_readout; the rows of every search are compared bit for bit with the oracle's term-serial fp32 chain.

Instantiations of cert_score_kernel<KS, MASKED> and the test that runs each with its T asserted (cert_stats()["dense_terms"]):

    KS  T    unmasked                                   masked (sr_sparse_search_masked, mask route)
    1   16   test_every_instantiation[16-plain]         test_every_instantiation[16-masked]         + every *runs* / *groups* test below
    2   32   test_every_instantiation[32-plain]         test_every_instantiation[32-masked]
    4   64   test_every_instantiation[48-plain] (48 dense slots + 16 zero columns), [64-plain]      [48-masked], [64-masked]
    5   80   test_every_instantiation[80-plain]         test_every_instantiation[80-masked]
    6   96   test_every_instantiation[96-plain]         test_every_instantiation[96-masked]
    7   112  test_every_instantiation[112-plain]        test_every_instantiation[112-masked]
    8   128  test_every_instantiation[128-plain]        test_every_instantiation[128-masked]

Paths inside the kernel and where they run:
    staged quads, every tail code 1 - 3 and 0, full tiles          runs_case (runs of 0, 1, 2, 3, 4, 5, 8, 9, 1 024 postings per (term, tile))
    single postings (E word = the posting)                         runs_case, ks_case
    runs across a tile boundary, a term in the partial last tile   runs_case
    n_tiles % 4 = 0 .. 3 (E rows' padding), odd tile0, odd launch   runs_case(0 .. 3); runs_case(0) searches with k + band >= 2 048
    cert_overflow_windows (> 512 quads per wave and tile)          groups_case
    cert_extra_groups (65 - 256 rare terms)                        groups_case
    keys near 65 535, both halves of an LDS word                   saturation_case
    fp16 ties, subnormal values, dropped / too large rare weights  midpoints_case, subnormal_case, drop_boundary_case
cert_plan_kernel: test_plan_equals_the_model;  the nine build kernels: test_structures_equal_the_index_model;
cert_select_kernel: test_certificate_candidates_are_the_docs_above_the_cut, test_uncertifiable_queries_are_flagged_and_come_back_identical;
cert_rescore_kernel (LDS lists <= 64 terms, scalar loop above): test_rescore_of_the_forward_rows."""
import contextlib
import os

import numpy as np
import pytest
import torch

import sparse_cert_cases as C
from oracle import scoring as O

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    os.environ.update({k: str(v) for k, v in kw.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _mask_of(N):
    i = np.arange(N)
    rng = np.random.default_rng(5)
    return ((i // 32) % 3 != 1) & (rng.random(N) < 0.7)             # whole 32-doc blocks off, and single docs


class Run:
    """One index and one recorded search of a case (and one masked search on demand), shared by the tests of this module."""

    def __init__(self, case):
        from scaling_retriever_amd.scoring import SparseIndexHIP
        self.case = case
        self.env = dict(SR_SPARSE_CERT=1, SR_SPARSE_CERT_T=case["t_cap"], SR_SUBSET_SPARSE_ROUTE="mask")
        with _env(**self.env):
            self.idx = SparseIndexHIP(case["indptr"], case["ids"], case["vals"], case["N"])
        self.present = self.idx.cert_stats()["present"] == 1
        self.full = None
        self.searches = {}

    def oracle(self, flags=None):
        c = self.case
        if self.full is None:
            known = (c["qc"] >= 0) & (c["qc"] < len(c["indptr"]) - 1)      # the C oracle indexes the lists with every term it is given
            qi = np.concatenate([[0], np.cumsum(known)])[c["qi"]].astype(np.int64)
            self.full = O.sparse_retrieve_c(c["indptr"], c["ids"], c["vals"], qi, c["qc"][known], c["qv"][known], c["N"], 0.0, c["N"], q_threads=4)
        fi, fs, fc = self.full
        k, nq = c["k"], c["nq"]
        es, ei, ec = np.zeros((nq, k), np.float32), np.full((nq, k), -1, np.int64), np.zeros(nq, np.int32)
        for q in range(nq):
            row = fi[q, :int(fc[q])]
            keep = np.arange(len(row)) if flags is None else np.flatnonzero(flags[row])
            keep = keep[:k]
            ec[q] = len(keep)
            ei[q, :len(keep)], es[q, :len(keep)] = row[keep], fs[q, keep]
        return es, ei, ec

    def search(self, masked=False):
        """Search, compare the rows with the oracle bit for bit, return everything the hooks read out."""
        if masked in self.searches:
            return self.searches[masked]
        c, idx = self.case, self.idx
        flags = _mask_of(c["N"]) if masked else None
        with _env(**self.env):
            idx.cert_record_keys(True)
            before = idx.cert_stats()
            s, i, n = idx.search(c["qi"], c["qc"], c["qv"], c["k"], mask=flags)
            torch.cuda.synchronize()
            after = idx.cert_stats()
            keys, consts, vscale, T = idx.cert_recorded_keys(c["nq"])
            out = {name: idx.cert_readout(name) for name in ("bfrag", "rare_term", "rare_w", "elig", "cq", "sq", "n_rare", "n_qt", "n_drop",
                                                              "m_count", "ap_ids", "uncert")}
            out["info"] = idx.cert_readout("info")
            idx.cert_record_keys(False)
        assert after["searches"] - before["searches"] == 1 and after["queries"] - before["queries"] == c["nq"]
        es, ei, ec = self.oracle(flags)
        s, i, n = s.cpu().numpy(), i.cpu().numpy(), n.cpu().numpy()
        assert np.array_equal(n, ec), (c["name"], "counts")
        bad = [q for q in range(c["nq"]) if not (np.array_equal(i[q], ei[q]) and np.array_equal(s[q].view(np.uint32), es[q].view(np.uint32)))]
        assert not bad, f"{c['name']}: queries with different rows: {bad[:10]} ({len(bad)} of {c['nq']})"
        out.update(keys=keys, T=T, vscale=vscale, flags=flags, rows=(s, i, n), redone=after["redone_exact"] - before["redone_exact"],
                   rescored=after["candidates_rescored"] - before["candidates_rescored"])
        ix = C.index_model(c["indptr"], c["ids"], c["vals"], c["N"], c["t_cap"])
        out["ix"], out["plan"] = ix, C.plan_model(ix, c["qi"], c["qc"], c["qv"], sq_from_gpu=out["sq"])
        self.searches[masked] = out
        return out


_RUNS = {}


def _run(case):
    if case["name"] not in _RUNS:
        _RUNS[case["name"]] = Run(case)
    return _RUNS[case["name"]]


def _check_plan(case, r):
    """The plan read back against the model: decisions and counts equal, s_q within 1 ulp of the model's own, B entries and rare
    weights (computed from the GPU's s_q) bit for bit."""
    plan, nq, T, KS = r["plan"], case["nq"], r["ix"]["T"], r["ix"]["KS"]
    assert np.array_equal(r["elig"][:nq], plan["elig"][:nq]), (case["name"], [(q, plan["reason"][q]) for q in np.flatnonzero(r["elig"][:nq] != plan["elig"][:nq])])
    on = np.flatnonzero(plan["elig"][:nq])
    ulp = np.abs(r["sq"][on].view(np.int32).astype(np.int64) - plan["sq_model"][on].view(np.int32).astype(np.int64))
    assert (ulp <= 1).all(), (case["name"], ulp.max())
    assert np.array_equal(r["cq"][:nq], plan["cq"][:nq])
    for name in ("n_rare", "n_qt", "n_drop"):
        assert np.array_equal(r[name][:nq], plan[name][:nq]), (case["name"], name)
    got_B = r["bfrag"].reshape(-1, KS, 2, 32, 8).transpose(0, 3, 1, 2, 4).reshape(-1, T)       # [block][k-step][k / 8][query][k % 8] -> [query][slot]
    rt, rw = r["rare_term"].reshape(-1, C.MAXRT), r["rare_w"].reshape(-1, C.MAXRT)
    assert np.array_equal(got_B[on].view(np.uint16), plan["B"][on].view(np.uint16)), case["name"]
    assert np.array_equal(rt[on], plan["rare_term"][on]) and np.array_equal(rw[on].view(np.uint32), plan["rare_w"][on].view(np.uint32)), case["name"]
    return int(ulp.max()) if len(on) else 0


def _check_keys(case, r, exact=False):
    """(K) for every (query, doc); exact: integer data, key = R + rint(y) wherever y is not within 2^-6 of a tie.  Returns the largest
    |key - (R + y)| and the tolerance at that pair."""
    ix, plan, N = r["ix"], r["plan"], case["N"]
    worst = (0.0, 0.0)
    for q in np.flatnonzero(plan["elig"][:case["nq"]]):
        R, y = C.key_model(ix, plan, q, flush_subnormals=bool(C.MFMA_FLUSHES_F16_SUBNORMALS))
        key = r["keys"][q].astype(np.float64)
        err = np.abs(key - (R + y))
        tol = C.key_tolerance(y, ix["T"])
        j = int(np.argmax(err - tol))
        assert (err <= tol).all(), (case["name"], int(q), j, float(key[j]), int(R[j]), float(y[j]), float(tol[j]))
        if err.max() > worst[0]:
            worst = (float(err.max()), float(tol[np.argmax(err)]))
        assert (key[N:] == 0).all()
        if exact:
            clear = np.abs(y - np.floor(y) - 0.5) > 2.0 ** -6
            assert np.array_equal(key[clear], (R + np.rint(y))[clear]), (case["name"], int(q))
    print(f"[keys] {case['name']}: largest |key - model| {worst[0]:.4f} (tolerance there {worst[1]:.4f})")
    return worst


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("cap", C.KS_CAPS)
def test_every_instantiation(cap, masked):
    case = C.ks_case(cap)
    run = _run(case)
    assert run.present and run.idx.cert_stats()["dense_terms"] == C.EXPECTED_T[cap]
    r = run.search(masked)
    assert r["T"] == C.EXPECTED_T[cap] and r["info"]["KS"] == C.EXPECTED_T[cap] // 16
    assert r["redone"] <= case["nq"] // 8                            # the scorer's own pass carried the call
    _check_plan(case, r)
    _check_keys(case, r)


@pytest.mark.parametrize("name", ["runs1", "runs2real", "forward"])
def test_structures_equal_the_index_model(name):
    case = {"runs1": C.runs_case(1, True), "runs2real": C.runs_case(2, False), "forward": C.forward_rows_case(1024)}[name]
    run = _run(case)
    assert run.present
    ix = C.index_model(case["indptr"], case["ids"], case["vals"], case["N"], case["t_cap"])
    with _env(**run.env):
        info = run.idx.cert_readout("info")
        got = {n: run.idx.cert_readout(n) for n in ("dslot", "vmax", "d16", "P", "S", "E", "fwd_indptr", "fwd_tv")}
    for key in ("T", "KS", "n_tiles", "e_stride", "V", "N", "nnz"):
        assert info[key] == ix[key], key
    assert info["vscale"] == float(ix["vscale"])
    assert np.array_equal(got["dslot"], ix["dslot"])
    assert np.array_equal(got["vmax"].view(np.uint32), ix["vmax"].view(np.uint32))
    assert np.array_equal(got["d16"].view(np.uint16), ix["d16"].reshape(-1).view(np.uint16))
    assert np.array_equal(got["P"], ix["P"])
    assert np.array_equal(got["S"], ix["S"].reshape(-1))
    assert np.array_equal(got["E"], ix["E"].reshape(-1))
    assert np.array_equal(got["fwd_indptr"], ix["fwd_indptr"])
    assert np.array_equal(got["fwd_tv"], ix["fwd_tv"])


def test_a_document_of_1025_postings_turns_the_scorer_down():
    assert _run(C.forward_rows_case(1024)).present
    big = Run(C.forward_rows_case(1025))
    assert not big.present and big.idx.cert_stats()["present"] == 0


@pytest.mark.parametrize("name", ["drop", "off_path", "groups", "midpoints", "subnormal", "saturation"])
def test_plan_equals_the_model(name):
    case = {"drop": C.drop_boundary_case(), "off_path": C.off_path_case(), "groups": C.groups_case(False), "midpoints": C.midpoints_case(),
            "subnormal": C.subnormal_case(), "saturation": C.saturation_case()}[name]
    r = _run(case).search()
    ulp = _check_plan(case, r)
    print(f"[plan] {case['name']}: s_q within {ulp} ulp of the model")
    if "expect_reason" in case:
        for q, why in enumerate(case["expect_reason"]) if isinstance(case["expect_reason"], list) else case["expect_reason"].items():
            assert bool(r["elig"][q]) == (why == ""), (q, why)
            assert bool(r["uncert"][q]) or why == ""                 # what the plan turns down is handed to the exact kernels


@pytest.mark.parametrize("name", ["saturation", "midpoints", "subnormal", "drop", "runs2real", "groups_real", "forward"])
def test_keys_equal_the_model_within_the_derived_tolerance(name):
    case = {"saturation": C.saturation_case(), "midpoints": C.midpoints_case(), "subnormal": C.subnormal_case(), "drop": C.drop_boundary_case(),
            "runs2real": C.runs_case(2, False), "groups_real": C.groups_case(False), "forward": C.forward_rows_case(1024)}[name]
    r = _run(case).search()
    _check_keys(case, r)
    if name == "saturation":
        star, keys = case["star"], r["keys"]
        for q in range(3):
            assert keys[q].argmax() == star and 0.975 * 65535 <= keys[q, star] <= C.saturation_limit(16, int(r["n_rare"][q]))
        R, y = C.key_model(r["ix"], r["plan"], 0)
        assert keys[0, star - 1] == R[star - 1] and y[star - 1] == 0          # the other half of the saturated word: its own posting, nothing else


@pytest.mark.parametrize("name,masked", [("runs0", False), ("runs1", False), ("runs1", True), ("runs2", False), ("runs3", False),
                                         ("groups", False), ("groups", True)])
def test_integer_cases_have_exactly_one_key(name, masked):
    case = C.groups_case(True) if name == "groups" else C.runs_case(int(name[-1]), True)
    run = _run(case)
    assert run.idx.cert_stats()["dense_terms"] == 16
    r = run.search(masked)
    assert r["redone"] <= case["nq"] // 8
    if name == "runs0":
        assert r["info"]["k_eff"] >= 2048                            # launches of 3, 6 .. tiles: tile_begin 3 and 9 are odd
    _check_keys(case, r, exact=True)


def test_conversion_rounding_and_subnormal_operands():
    """r of (K), measured where y is exact (integer cases: every partial sum of the MFMA is exact in fp32, R has one value), and what the
    MFMA does with fp16 subnormal A operands, on the docs of the subnormal case whose key tells: y with the 15 subnormal products
    rounds to another integer than y without them, both at least 0.008 from the tie."""
    r_max = 0.0
    for case in (C.runs_case(1, True), C.groups_case(True)):
        r = _run(case).search()
        for q in np.flatnonzero(r["plan"]["elig"][:case["nq"]]):
            R, y = C.key_model(r["ix"], r["plan"], q)
            r_max = max(r_max, float(np.abs(r["keys"][q].astype(np.float64) - R - y).max()))
    print(f"[measured] conversion rounding r = {r_max:.6f} key units")
    assert r_max <= C.R_CVT
    case = C.subnormal_case()
    r = _run(case).search()
    assert r["plan"]["elig"][0] and r["plan"]["cq"][0] == np.float32(2.0 ** -24)
    _, y_keep = C.key_model(r["ix"], r["plan"], 0)
    _, y_flush = C.key_model(r["ix"], r["plan"], 0, flush_subnormals=True)
    frac = lambda v: np.abs(v - np.floor(v) - 0.5)
    tell = (np.rint(y_keep) != np.rint(y_flush)) & (frac(y_keep) > 0.008) & (frac(y_flush) > 0.008)
    tell[case["N"]:] = False
    key = r["keys"][0].astype(np.float64)
    kept, flushed = int((key[tell] == np.rint(y_keep)[tell]).sum()), int((key[tell] == np.rint(y_flush)[tell]).sum())
    print(f"[measured] fp16 subnormal A operands of the MFMA: {int(tell.sum())} telling docs, {kept} keys as if kept, {flushed} as if flushed")
    assert tell.sum() >= 5 and kept + flushed == tell.sum() and (kept == 0 or flushed == 0)
    assert (flushed > 0) == bool(C.MFMA_FLUSHES_F16_SUBNORMALS)


@pytest.mark.parametrize("name,masked", [("ks128", False), ("ks48", True), ("groups_real", False), ("runs2real", False), ("runs1", True),
                                         ("midpoints", False), ("forward", False)])
def test_certificate_candidates_are_the_docs_above_the_cut(name, masked):
    case = {"ks128": C.ks_case(128), "ks48": C.ks_case(48), "groups_real": C.groups_case(False), "runs2real": C.runs_case(2, False),
            "runs1": C.runs_case(1, True), "midpoints": C.midpoints_case(), "forward": C.forward_rows_case(1024)}[name]
    r = _run(case).search(masked)
    N, k, T = case["N"], case["k"], r["T"]
    allowed = np.ones(N, bool) if r["flags"] is None else r["flags"]
    ap = r["ap_ids"].reshape(-1, 2 * r["info"]["k_eff"])
    es, ei, ec = _run(case).oracle(r["flags"])
    certified = 0
    for q in range(case["nq"]):
        if r["uncert"][q]:
            assert r["m_count"][q] == 0
            continue
        keys = np.where(allowed, r["keys"][q, :N], 0).astype(np.int64)
        kth = np.sort(keys)[-k]
        cut = C.cut_from_kth(kth, T, int(r["n_rare"][q]), int(r["n_qt"][q]), int(r["n_drop"][q]))
        assert cut >= 1.0
        want = np.flatnonzero(keys >= int(cut))
        got = np.sort(ap[q, :r["m_count"][q]])
        assert np.array_equal(got, want), (case["name"], q, len(got), len(want))
        assert np.isin(ei[q, :ec[q]], got).all()
        certified += 1
    assert certified >= case["nq"] - case["nq"] // 8 - sum(1 for why in r["plan"]["reason"][:case["nq"]] if why)


def test_uncertifiable_queries_are_flagged_and_come_back_identical():
    case = C.uncertifiable_case()
    r = _run(case).search()                                          # the rows are compared with the oracle's inside
    assert list(r["elig"][:3]) == [1, 1, 1]
    assert list(r["uncert"]) == case["expect_uncert"] and r["redone"] == 2
    assert list(r["m_count"][:3] > 0) == [False, False, True]
    assert len(np.unique(r["keys"][0, :case["N"]])) == 1 and (r["keys"][1, :case["N"]] > 0).sum() == 3


def test_rescore_of_the_forward_rows():
    """Docs of 1, 2, 3 and 1 024 postings at odd and even offsets of fwd_tv as candidates of 64-term (LDS lists) and 65-term (scalar
    loop) queries: certified, re-scored, and rows of the result with the oracle's bits (compared inside search())."""
    case = C.forward_rows_case(1024)
    r = _run(case).search()
    assert r["redone"] == 0 and r["rescored"] > 0 and not r["uncert"].any()
    lens = np.diff(case["qi"])
    assert {64, 65} <= set(lens.tolist())
    ap = r["ap_ids"].reshape(-1, 2 * r["info"]["k_eff"])
    special = np.array([d for d, n in case["n_post"].items() if n > 0])
    s, i, n = r["rows"]
    for q in range(case["nq"]):
        cand = ap[q, :r["m_count"][q]]
        assert np.isin(special, cand).all(), (q, special[~np.isin(special, cand)])
        assert np.isin(special, i[q, :n[q]]).all(), q               # ... and they are among the k best: their exact scores were compared
