"""Per-row term budget of the sparse head (sr_sparse_compact_topm, sparse_reps_to_csr(max_terms=), --doc_max_terms /
--query_max_terms): what can be checked without a device.  The numpy statement of the contract (topm_row_reference; tests/test_sparse_prune_gpu.py
carries the same lines) is checked here against a pick-by-pick loop."""
import ctypes
import inspect

import numpy as np


def topm_row_reference(row, m):
    """Columns kept for one fp32 row under budget m (0 = no limit), ascending: the min(m, nnz) non-zeros that come first by value
    descending, ties to the lower column.  -0.0 is zero."""
    nz = np.flatnonzero(row != 0)
    order = np.lexsort((nz, -row[nz]))        # value descending, then column ascending
    return np.sort(nz[order[:m]]) if m else nz


def _brute_force_row(row, m):
    """The contract one pick at a time: m times take the largest remaining non-zero, the lowest column among equals."""
    cand = [c for c in range(len(row)) if row[c] != 0]
    if m == 0:
        return cand
    kept = []
    for _ in range(min(m, len(cand))):
        best = cand[0]
        for c in cand[1:]:
            if row[c] > row[best]:          # strict: an equal value at a higher column never replaces a lower one
                best = c
        kept.append(best)
        cand.remove(best)
    return sorted(kept)


def test_numpy_reference_agrees_with_brute_force():
    rng = np.random.default_rng(7)
    levels = np.array([-1.0, -0.5, -0.0, 0.0, 0.0, 0.0, 0.5, 1.0, 1.0, 2.0], np.float32)
    n_cut_in_tie = 0
    for trial in range(200):
        V = int(rng.integers(1, 40))
        row = levels[rng.integers(0, len(levels), V)] if trial % 2 else \
            (rng.standard_normal(V) * (rng.random(V) < 0.5)).astype(np.float32)
        for m in (0, 1, 2, 3, 7, V, V + 3):
            got = topm_row_reference(row, m)
            assert got.tolist() == _brute_force_row(row, m), (row, m)
            dropped = np.setdiff1d(np.flatnonzero(row != 0), got)
            if len(dropped) and len(got) and row[dropped].max() == row[got].min():
                n_cut_in_tie += 1
                tied_kept = got[row[got] == row[got].min()]
                assert tied_kept.max() < dropped[row[dropped] == row[got].min()].min()     # the lower columns won the tie
    assert n_cut_in_tie > 20        # the tie rule was exercised


def test_entry_point_rejects_negative_budget_without_a_device():
    from scaling_retriever_amd import _lib
    lib = _lib.load()
    assert "sr_sparse_compact_topm" in _lib.SIGNATURES and hasattr(lib, "sr_sparse_compact_topm")
    n = ctypes.c_int64(-7)
    rc = lib.sr_sparse_compact_topm(None, 1, 8, -1, None, None, None, 0, ctypes.byref(n), None)
    assert rc == _lib.SR_ERR_INVALID
    assert "max_terms" in lib.sr_last_error().decode()
    assert n.value == -7            # nothing was written


def test_eval_sparse_flags_default_to_zero():
    import eval_sparse
    a = eval_sparse.parse_args(["--task_name", "indexing"])
    assert a.doc_max_terms == 0 and a.query_max_terms == 0
    a = eval_sparse.parse_args(["--task_name", "retrieval", "--doc_max_terms", "128", "--query_max_terms", "32"])
    assert a.doc_max_terms == 128 and a.query_max_terms == 32


def test_python_signatures_carry_the_budgets():
    from scaling_retriever_amd import indexer
    assert inspect.signature(indexer.sparse_reps_to_csr).parameters["max_terms"].default == 0
    assert inspect.signature(indexer.SparseIndexer.__init__).parameters["doc_max_terms"].default == 0
    assert inspect.signature(indexer.HybridIndexer.__init__).parameters["doc_max_terms"].default == 0
    assert inspect.signature(indexer.SparseRetrieval.__init__).parameters["query_max_terms"].default == 0
    assert inspect.signature(indexer.HybridRetriever.__init__).parameters["query_max_terms"].default == 0
