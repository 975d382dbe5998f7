"""The launch plan of a sparse search: how many scoring launches a search makes and how many posting bytes they cover.

Results are exact whatever the chunking, so a driver that cuts the doc tiles or the query batches differently passes every result
test and shows only as a speed change.  The handle counts its scoring launches (sr_sparse_index_profile / _profile_read); here one
search per case is compared with a restatement of the schedule:

  exact kernels (sparse_exact_search, doc tiles of 8 192): queries in batches of q_batch = min(nq, 1 024);
      max_tiles = clamp(limit / (8 q_batch 8 192), 1, min(64, n_tiles)) for k <= 4 096; per batch the launches cover 1, 2, 4, ...
      tiles, each at most max_tiles, until n_tiles are covered; one profiled launch per step, whether the query-block kernel, the
      per-query kernel or both ran in it;
  certified scorer (sparse_cert_search, doc tiles of 1 024): queries in batches of 8 192 (dev switch SR_SPARSE_CERT_BATCH);
      band = 1 024 keys while no query has more than 96 rare terms, capped at 4 096 - k; k_eff = k + band; the first launch covers
      k_eff // 1 024 + 1 tiles, then the step doubles, at most 512 tiles per launch; queries handed back would add the exact
      kernels' launches for that sub-batch - the certified cases assert that nothing is handed back.

A tile covered twice or skipped can leave the launch count as it is, so on the exact path total_posting_bytes must equal 8 x the
summed posting-list lengths of all valid query terms over all queries, and block_stats() / cert_stats() must match the route."""
import ctypes

import numpy as np
import pytest
import torch

from test_sparse_cert_gpu import _zipf_index, _zipf_queries

pytestmark = pytest.mark.gpu

WS_DEFAULT = 4 << 30
N_EXACT = 9 * 8192 + 1          # 10 doc tiles of the exact kernels
N_CERT = 40 * 1024 + 3          # 41 doc tiles of the certified scorer
V_EXACT = 40
HEAVY_TERM = 3


def _exact_launches(nq, n_docs, limit):
    n_tiles = -(-n_docs // 8192)
    q_batch = min(nq, 1024)
    max_tiles = max(1, min(limit // (8 * q_batch * 8192), 64, n_tiles))
    per_batch, t0, step = [], 0, 1
    while t0 < n_tiles:
        nt = min(step, max_tiles, n_tiles - t0)
        per_batch.append(nt)
        t0 += nt
        step *= 2
    return per_batch, -(-nq // q_batch)


def _cert_launches(nq, k, n_docs, batch=8192):
    n_tiles = -(-n_docs // 1024)
    k_eff = k + min(1024, 4096 - k)
    per_batch, t0, step = [], 0, k_eff // 1024 + 1
    while t0 < n_tiles:
        nt = min(step, 512, n_tiles - t0)
        per_batch.append(nt)
        t0 += nt
        step *= 2
    return per_batch, -(-nq // batch)


def _profiled_search(idx, q, k):
    from scaling_retriever_amd import _lib
    lib = _lib.load()
    _lib.check(lib.sr_sparse_index_profile(idx._h, 1))
    idx.search(*q, k)
    torch.cuda.synchronize()
    _lib.check(lib.sr_sparse_index_profile(idx._h, 0))
    n_l, ms, by = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
    _lib.check(lib.sr_sparse_index_profile_read(idx._h, ctypes.byref(n_l), ctypes.byref(ms), ctypes.byref(by)))
    return n_l.value, by.value


@pytest.fixture(scope="module")
def exact_lists():
    """40 posting lists of 200 .. 3 000 docs (none reaches n_docs / 4: no dense column), and the list of a term in every doc."""
    rng = np.random.default_rng(11)
    lists = [np.sort(rng.choice(N_EXACT, size=int(rng.integers(200, 3000)), replace=False)).astype(np.int32) for _ in range(V_EXACT)]
    return lists, np.arange(N_EXACT, dtype=np.int32)


def _exact_index(exact_lists, heavy, monkeypatch):
    from scaling_retriever_amd.scoring import SparseIndexHIP
    monkeypatch.setenv("SR_SPARSE_SCORER", "exact")          # no certified scorer: every search runs the exact kernels
    lists, everywhere = exact_lists
    lists = list(lists)
    if heavy:
        lists[HEAVY_TERM] = everywhere
    lens = np.array([len(l) for l in lists], np.int64)
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ids = np.concatenate(lists)
    vals = np.random.default_rng(12).uniform(0.1, 3.0, size=len(ids)).astype(np.float32)
    idx = SparseIndexHIP(indptr, ids, vals, N_EXACT)
    st = idx.cert_stats()
    assert st["present"] == 0
    assert idx.block_stats()["dense_terms"] == (1 if heavy else 0)
    return idx, lens


def _exact_queries(nq, descending=()):
    """Ascending terms, the heavy one in every second query, and a term the index does not know (no postings) in every third."""
    rng = np.random.default_rng(100 + nq)
    qi, qc = [0], []
    for q in range(nq):
        cols = set(rng.choice(V_EXACT, size=int(rng.integers(2, 7)), replace=False).tolist())
        if q % 2 == 0:
            cols.add(HEAVY_TERM)
        cols = sorted(cols)
        if q % 3 == 0:
            cols.append(V_EXACT + 5)
        if q in descending:
            cols = cols[::-1]
        qc.extend(cols)
        qi.append(len(qc))
    qc = np.array(qc, np.int32)
    return np.array(qi, np.int64), qc, np.random.default_rng(7).uniform(0.5, 2.0, size=len(qc)).astype(np.float32)


def _posting_bytes(q, lens):
    cols = q[1]
    return 8 * int(lens[cols[(cols >= 0) & (cols < len(lens))]].sum())


def _check_exact(idx, lens, q, k, limit, block_calls, fallback_calls, want_steps, want_batches):
    nq = len(q[0]) - 1
    n_l, by = _profiled_search(idx, q, k)
    steps, batches = _exact_launches(nq, N_EXACT, limit)
    bs, cs = idx.block_stats(), idx.cert_stats()
    print(f"exact nq={nq} limit={limit}: n_launches={n_l} expected={batches} x {steps} posting_bytes={by:.0f} "
          f"expected={_posting_bytes(q, lens)} {bs} {cs}")
    assert (steps, batches) == (want_steps, want_batches)
    assert n_l == batches * len(steps)
    assert by == _posting_bytes(q, lens)
    assert (bs["block_calls"], bs["fallback_calls"]) == (block_calls, fallback_calls)
    assert (cs["searches"], cs["queries"], cs["redone_exact"], cs["batches_without_memory"]) == (0, 0, 0, 0)


@pytest.mark.parametrize("heavy", [False, True])
def test_exact_launch_plan_default_limit(exact_lists, monkeypatch, heavy):
    """No heavy term: the per-query kernel alone; a heavy term: the query-block kernel alone.  10 tiles in launches of 1, 2, 4, 3."""
    idx, lens = _exact_index(exact_lists, heavy, monkeypatch)
    _check_exact(idx, lens, _exact_queries(5), 10, WS_DEFAULT, 1 if heavy else 0, 0, [1, 2, 4, 3], 1)


@pytest.mark.parametrize("heavy", [False, True])
def test_exact_launch_plan_small_limit(exact_lists, monkeypatch, heavy):
    """1 MiB of workspace for 8 queries: two tiles of candidate slots per query, so max_tiles = 2 decides."""
    idx, lens = _exact_index(exact_lists, heavy, monkeypatch)
    idx.set_workspace_limit(1 << 20)
    _check_exact(idx, lens, _exact_queries(8), 10, 1 << 20, 1 if heavy else 0, 0, [1, 2, 2, 2, 2, 1], 1)


@pytest.mark.parametrize("heavy", [False, True])
def test_exact_launch_plan_two_query_batches(exact_lists, monkeypatch, heavy):
    """1 030 queries: batches of 1 024 and 6, each with the schedule of the first."""
    idx, lens = _exact_index(exact_lists, heavy, monkeypatch)
    _check_exact(idx, lens, _exact_queries(1030), 10, WS_DEFAULT, 1 if heavy else 0, 0, [1, 2, 4, 3], 2)


def test_exact_launch_plan_mixed_launch(exact_lists, monkeypatch):
    """One query whose terms do not ascend: its block goes through the per-query kernel, the others through the query-block kernel, both
    in every step - still one profiled launch per step."""
    idx, lens = _exact_index(exact_lists, True, monkeypatch)
    _check_exact(idx, lens, _exact_queries(9, descending=(4,)), 10, WS_DEFAULT, 1, 1, [1, 2, 4, 3], 1)


@pytest.fixture(scope="module")
def cert_case():
    """The shape of the small fixtures of test_sparse_cert_gpu.py (Zipf index of 800 terms, 30 postings per doc; queries of up to 16 terms)."""
    rng = np.random.default_rng(800 + N_CERT)
    V = 800
    index = _zipf_index(rng, V, N_CERT, 30)
    return index, {nq: _zipf_queries(rng, V, nq, 16) for nq in (33, 70)}


def _check_cert(cert_case, monkeypatch, nq, k, batch, want_steps, want_batches):
    from scaling_retriever_amd.scoring import SparseIndexHIP
    monkeypatch.setenv("SR_DEV_SWITCHES", "1")
    monkeypatch.setenv("SR_SPARSE_CERT", "1")               # build + use the certified scorer below its size threshold as well
    if batch != 8192:
        monkeypatch.setenv("SR_SPARSE_CERT_BATCH", str(batch))
    (indptr, ids, vals), queries = cert_case
    q = queries[nq]
    assert np.diff(q[0]).max() <= 96                        # band = 1 024
    idx = SparseIndexHIP(indptr, ids, vals, N_CERT)
    assert idx.cert_stats()["present"] == 1 and idx.cert_stats()["doc_tiles"] == 41
    n_l, by = _profiled_search(idx, q, k)
    steps, batches = _cert_launches(nq, k, N_CERT, batch)
    bs, cs = idx.block_stats(), idx.cert_stats()
    print(f"certified nq={nq} batch={batch}: n_launches={n_l} expected={batches} x {steps} posting_bytes={by:.0f} {bs} {cs}")
    assert (steps, batches) == (want_steps, want_batches)
    assert cs["redone_exact"] == 0                          # nothing handed back: the count is the scorer's launches alone
    assert n_l == batches * len(steps)
    assert (cs["searches"], cs["queries"], cs["batches_without_memory"]) == (batches, nq, 0)
    assert (bs["block_calls"], bs["fallback_calls"]) == (0, 0)


def test_certified_launch_plan(cert_case, monkeypatch):
    """k_eff = 1 034: the first launch covers 2 tiles, then 4, 8, 16 and the last 11 of the 41."""
    _check_cert(cert_case, monkeypatch, 33, 10, 8192, [2, 4, 8, 16, 11], 1)


def test_certified_launch_plan_three_batches(cert_case, monkeypatch):
    """70 queries in batches of 32: 32, 32 and 6, each with the schedule of the first."""
    _check_cert(cert_case, monkeypatch, 70, 10, 32, [2, 4, 8, 16, 11], 3)
