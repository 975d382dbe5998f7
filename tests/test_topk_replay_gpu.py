"""GPU: the top-k machine of csrc/topk.hip and csrc/topk_large.hip, path by path, against the numpy model of its protocol.

sr_topk_replay runs reset -> (producer append -> topk_compact2 -> read-out) per step -> topk_finalize on the streams of
tests/topk_cases.py; every threshold, count, running set and output must equal the model's - there is no tolerance here.  Which path a
(step, query) takes is the model's label (tests/test_topk_replay_host.py asserts that the list reaches them all).  The direct
sr_topk_merge tests at the end use np.lexsort as their reference."""
import ctypes

import numpy as np
import pytest

import topk_cases as TC

pytestmark = pytest.mark.gpu


def _hook(c, keys=True):
    """One sr_topk_replay call on a case -> its outputs and traces as numpy arrays."""
    import torch
    from scaling_retriever_amd import _lib
    lib = _lib.load()
    r = TC.expected(c)
    nq, k, S = c["nq"], c["k"], len(c["steps"]) - 1
    dev = "cuda:0"
    sc, ids = torch.from_numpy(r["scores"]).to(dev), torch.from_numpy(r["ids"]).to(dev)
    out = dict(out_scores=torch.full((nq, k), float("nan"), device=dev), out_ids=torch.full((nq, k), -7, dtype=torch.int64, device=dev),
               out_counts=torch.full((nq,), -7, dtype=torch.int32, device=dev), tau=torch.full((S, nq), float("nan"), device=dev),
               tau2=torch.full((S, nq), float("nan"), device=dev), cand=torch.full((S, nq), -7, dtype=torch.int32, device=dev),
               run=torch.full((S, nq), -7, dtype=torch.int32, device=dev))
    if keys:
        out["keys"] = torch.zeros((S, nq, 2 * k), dtype=torch.int64, device=dev)
    steps = (ctypes.c_int64 * (S + 1))(*c["steps"])
    p = {name: ctypes.c_void_p(t.data_ptr()) for name, t in out.items()}
    with torch.cuda.device(0):
        _lib.check(lib.sr_topk_replay(ctypes.c_void_p(sc.data_ptr()), ctypes.c_void_p(ids.data_ptr()), nq, r["scores"].shape[1], steps, S,
                                      k, c["k2"], c["select_over"], c["filter"], c["seg_n"], c["seg_group"], c["tau2_init"], c["pad_score"],
                                      p["out_scores"], p["out_ids"], p["out_counts"], p["tau"], p["tau2"], p["cand"], p["run"],
                                      p.get("keys"), _lib.stream_ptr()), "sr_topk_replay")
        torch.cuda.synchronize()
    return {name: t.cpu().numpy() for name, t in out.items()}


def _decode(keys):
    """uint64 keys (as int64 words) -> (scores fp32, ids int64), both sorted by id: the set they stand for."""
    u = keys.view(np.uint64)
    o = (u >> np.uint64(32)).astype(np.uint32)
    bits = np.where(o & np.uint32(0x80000000), o & np.uint32(0x7FFFFFFF), ~o)
    ids = (~u & np.uint64(0xFFFFFFFF)).astype(np.int64)
    by_id = np.argsort(ids)
    return bits.astype(np.uint32).view(np.float32)[by_id], ids[by_id]


def _check(c, g):
    """Everything the hook returned against the model."""
    r = TC.expected(c)
    name, k, S = c["name"], c["k"], len(c["steps"]) - 1
    assert np.array_equal(g["cand"], r["cand"]), (name, "cand", np.argwhere(g["cand"] != r["cand"])[:4])
    assert np.array_equal(g["run"], r["run"]), (name, "run", np.argwhere(g["run"] != r["run"])[:4])
    assert np.array_equal(g["tau"], r["tau"]), (name, "tau", np.argwhere(g["tau"] != r["tau"])[:4])
    # tau2: refreshed to the exact k2-th best score of the union by every select from registers, maybe by one from memory, never
    # by anything else, never lowered
    prev = np.full(c["nq"], c["tau2_init"], np.float32)
    for st in range(S):
        t2, exact = g["tau2"][st], r["kth2"][st]
        for q, lab in enumerate(r["label"][st]):
            where = (name, "tau2", st, q, lab, float(t2[q]), float(prev[q]), float(exact[q]))
            if c["k2"] > 0 and lab.endswith("regs"):
                assert t2[q] == exact[q], where
            elif c["k2"] > 0 and lab.startswith("select"):
                assert t2[q] == exact[q] or t2[q] == prev[q], where
            else:
                assert t2[q] == prev[q], where
            assert t2[q] >= prev[q], where
        prev = t2
    if "keys" in g:
        for st in range(S):
            for q in range(c["nq"]):
                e_ids, e_scores = r["run_set"][st][q]
                s, i = _decode(g["keys"][st, q, :g["run"][st, q]])
                assert np.array_equal(i, e_ids) and np.array_equal(s, e_scores), (name, "run set", st, q, r["label"][st][q])
    assert np.array_equal(g["out_counts"], r["out_counts"]), (name, "counts")
    assert np.array_equal(g["out_ids"], r["out_ids"]), (name, "ids", np.argwhere(g["out_ids"] != r["out_ids"])[:4])
    assert np.array_equal(g["out_scores"], r["out_scores"]), (name, "scores", np.argwhere(g["out_scores"] != r["out_scores"])[:4])


@pytest.mark.parametrize("c", TC.CASES, ids=lambda c: c["name"])
def test_replay_equals_model(c):
    _check(c, _hook(c))


def _same(a, b):
    for key in a:
        if key == "keys":       # the appends land in the order the atomics gave them: equal as sets
            for st in range(a["run"].shape[0]):
                for q in range(a["run"].shape[1]):
                    n = a["run"][st, q]
                    assert np.array_equal(np.sort(a["keys"][st, q, :n]), np.sort(b["keys"][st, q, :n])), (st, q)
        else:
            assert np.array_equal(a[key].view(np.int32) if a[key].dtype == np.float32 else a[key],
                                  b[key].view(np.int32) if b[key].dtype == np.float32 else b[key]), key


@pytest.mark.parametrize("name", ["k257_random", "r20_n5121_nrge", "l_plateau_straddle", "seg_two_rounds_g8"])
def test_replay_twice_is_identical(name):
    """A fresh workspace per call: the second call returns the bits of the first."""
    c = TC.BY_NAME[name]
    _same(_hook(c), _hook(c))


def test_replay_alternating_cases_keep_no_state():
    """Two cases with different k, segment geometry and path, in turn: each call gives its own result (nothing leaks through a
    static)."""
    a, b = TC.BY_NAME["seg_random_k2"], TC.BY_NAME["large_nrlt"]
    c = TC.BY_NAME["seg_g1"]
    for case in (a, b, c, a, b, c):
        _check(case, _hook(case, keys=False))


@pytest.mark.parametrize("nq", [9, 70])
def test_dense_search_orders_signed_zeros_by_doc_index(nq):
    """The rule holds where a score kernel builds the keys, not only in the hook: every document scores zero - all-zero rows give +0.0,
    rows whose products underflow from the negative side give -0.0 in a fused chain (even and odd rows here) - so the top-k is the k
    lowest doc indices, with scores that compare equal to 0.  nq = 9 and 70: the small-batch kernel and the MFMA kernel."""
    import torch
    from scaling_retriever_amd.scoring import DenseIndexHIP
    dim, n, k = 64, 640, 24
    rows = np.zeros((n, dim), np.float32)
    rows[1::2] = np.float32(-1e-30)
    q = np.full((nq, dim), 1e-30, np.float32)
    idx = DenseIndexHIP(dim)
    idx.add_host_rows(rows)
    s, i = idx.search(torch.from_numpy(q).cuda(), k)
    s, i = s.cpu().numpy(), i.cpu().numpy()
    assert np.array_equal(i, np.tile(np.arange(k), (nq, 1))), i[0]
    assert (s == 0).all()


# ------------------------------------------------------------------------------------------------------------ sr_topk_merge ---
def _merge_case(W, k, nq, seed, pad_score=-TC.FLT_MAX, zeros=False, big_ids=False):
    """[W, nq, k] lists with unique ids per query.  Query 1 (if there) is all padding, query 2 holds fewer than k entries in all, the
    others are full.  zeros: a block of +-0.0 straddles rank k under half of the entries.  -> scores, ids, expected [nq, k] pair."""
    rng = np.random.default_rng(seed)
    n = W * k
    scores, ids = np.empty((W, nq, k), np.float32), np.empty((W, nq, k), np.int64)
    e_s, e_i = np.full((nq, k), pad_score, np.float32), np.full((nq, k), -1, np.int64)
    for q in range(nq):
        s = rng.standard_normal(n).astype(np.float32)
        if zeros:                                       # k // 2 better entries, then zeros of both signs past rank k, the rest worse
            a, p = k // 2, min(n - k // 2, k)
            s[:a] = 1 + np.abs(s[:a])
            s[a:a + p] = np.where(rng.integers(0, 2, p) == 1, np.float32(-0.0), np.float32(0.0))
            s[a + p:] = -1 - np.abs(s[a + p:])
            s = s[rng.permutation(n)]
        i = rng.permutation(n).astype(np.int64)
        if big_ids:                                     # spread over [0, 2^32 - 1], both ends included
            i *= (2 ** 32 - 1) // max(1, n - 1)
            i[np.argmax(i)] = 2 ** 32 - 1
        if q == 1:
            i[:] = -1
        elif q == 2:
            i[rng.permutation(n)[max(1, k // 2):]] = -1
        v = i >= 0
        o = np.lexsort((i[v], -s[v].astype(np.float64)))[:k]
        e_s[q, :len(o)], e_i[q, :len(o)] = s[v][o], i[v][o]
        scores[:, q, :], ids[:, q, :] = s.reshape(W, k), i.reshape(W, k)
    return scores, ids, e_s, e_i


@pytest.mark.parametrize("W,k,nq,kw", [
    (7, 1024, 5, {}),                                   # W k = 7168: the last union the select holds in registers
    (8, 897, 5, {}),                                    # 7176: the first one it re-reads from memory
    (2, 4096, 4, {}),                                   # the memory select from an empty running set, the 64 KB sort
    (2, 4097, 4, {}),                                   # the global-memory path
    (5, 1, 9, {}),
    (3, 40, 9, dict(pad_score=-1.5)),
    (4, 25, 9, dict(zeros=True)),
    (2, 4097, 3, dict(zeros=True)),
    (4, 300, 5, dict(big_ids=True)),
    (1, 1, 1, dict(big_ids=True)),
], ids=lambda v: str(v) if not isinstance(v, dict) else "-".join(v) or "plain")
def test_topk_merge_direct(W, k, nq, kw):
    import torch
    from scaling_retriever_amd.scoring import topk_merge
    scores, ids, e_s, e_i = _merge_case(W, k, nq, seed=W * 100003 + k, **kw)
    s, i = topk_merge(torch.from_numpy(scores).cuda(), torch.from_numpy(ids).cuda(), **({"pad_score": kw["pad_score"]} if "pad_score" in kw else {}))
    s, i = s.cpu().numpy(), i.cpu().numpy()
    assert np.array_equal(i, e_i), np.argwhere(i != e_i)[:4]
    assert np.array_equal(s, e_s), np.argwhere(s != e_s)[:4]
