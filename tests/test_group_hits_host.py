"""CPU: the hits inside a collapsed search's groups - what needs no device.  The member table against numpy, the argument rules of the
new entry points and front ends (each rejected before anything touches a device), and the models' own invariant on the shared cases:
the first hit of every returned group is the group's representative."""
import ctypes

import numpy as np
import pytest
import torch

import collapse_cases as C
import group_hits_cases as H


def _table_equal(got, want):
    assert got[0].dtype == torch.int32 and got[1].dtype == torch.int64 and got[2].dtype == torch.int64
    for g, w in zip(got, want):
        assert np.array_equal(g.numpy(), w), (g, w)


@pytest.mark.parametrize("keys", [
    np.array([1 << 20, 3, 1 << 20, 0, 3, (1 << 31) - 1, 3], np.int32),          # sparse keys: never an array index
    np.full(17, 42, np.int32),                                                  # a single group
    np.arange(50, dtype=np.int32)[::-1].copy(),                                 # all groups distinct, keys descending along the index
    np.array([5, -1, 5, -1, 2], np.int32),                                      # indices without a document belong to no group
    np.zeros(0, np.int32),
], ids=["sparse-keys", "one-group", "all-distinct", "holes", "empty"])
def test_member_table_on_cpu_tensors(keys):
    from scaling_retriever_amd.collapse import member_table
    want = H.member_table_model(keys)
    _table_equal(member_table(keys), want)
    _table_equal(member_table(torch.from_numpy(keys), device="cpu"), want)
    uniq, indptr, ids = want
    assert (np.diff(uniq) > 0).all() and indptr[0] == 0 and indptr[-1] == len(ids) == int((keys >= 0).sum())
    for g in range(len(uniq)):
        members = ids[indptr[g]:indptr[g + 1]]
        assert (np.diff(members) > 0).all() and (keys[members] == uniq[g]).all()


def test_member_table_of_the_shared_case_is_the_models():
    from scaling_retriever_amd.collapse import member_table
    keys = C.dense_case()[2]
    _table_equal(member_table(keys), H.member_table_model(keys))
    with pytest.raises(ValueError, match="int32"):
        member_table(keys.astype(np.int64))


def test_segment_topm_validates_before_anything_touches_a_device():
    """sr_segment_topm through the ABI: m outside [1, 64], null pointers and a negative n_segs are SR_ERR_INVALID; the pointers below are
    never dereferenced.  The content of an indptr is device data: the front end checks one that still lives on the host."""
    from scaling_retriever_amd import _lib
    from scaling_retriever_amd.scoring import segment_topm
    lib = _lib.load()
    p = ctypes.c_void_p(4096)

    def topm(**kw):
        a = dict(dict(sc=p, ids=p, ptr=p, n=3, m=3, os=p, oi=p, oc=p), **kw)
        return lib.sr_segment_topm(a["sc"], a["ids"], a["ptr"], a["n"], a["m"], 0, 0.0, 0.0, a["os"], a["oi"], a["oc"], None)
    for change, text in [(dict(m=0), b"m = 0"), (dict(m=65), b"m = 65"), (dict(m=-1), b"m = -1"), (dict(sc=None), b"null pointer"),
                         (dict(ids=None), b"null pointer"), (dict(ptr=None), b"null pointer"), (dict(os=None), b"null pointer"),
                         (dict(oi=None), b"null pointer"), (dict(oc=None), b"null pointer"), (dict(n=-1), b"bad n_segs")]:
        rc = topm(**change)
        assert rc == _lib.SR_ERR_INVALID and text in lib.sr_last_error(), (change, rc, lib.sr_last_error())
    assert topm(n=0) == _lib.SR_OK
    s, i = np.zeros(6, np.float32), np.arange(6, dtype=np.int64)
    for m in (0, 65, 2.5, None):
        with pytest.raises(ValueError, match=r"integer in \[1, 64\]"):
            segment_topm(s, i, np.array([0, 6]), m)
    for indptr, text in [(np.array([1, 6]), "must start at 0"), (np.array([0, 4, 3, 6]), "decreases behind segment 1"),
                         (torch.tensor([0, 5, 2, 6]), "decreases behind segment 1"), (np.array([0, 5]), "ends at 5"),
                         (np.zeros((2, 2), np.int64), "1-D"), (np.array([0.0, 6.0]), "integers")]:
        with pytest.raises(ValueError, match=text):
            segment_topm(s, i, indptr, 2)
    with pytest.raises(ValueError, match="one length"):
        segment_topm(s, i[:5], np.array([0, 6]), 2)


def test_group_members_validate_before_anything_touches_a_device():
    """sr_group_members_count / _fill: null pointers, negative sizes and a mask without its words are SR_ERR_INVALID before any device
    work; the pointers below are never dereferenced."""
    from scaling_retriever_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(4096)
    total = ctypes.c_int64(-1)

    def count(**kw):
        a = dict(dict(keys=p, nq=2, kg=3, uniq=p, G=4, mptr=p, mids=p, n=9, words=None, n_masks=0, n_bits=0, qg=None, out=p,
                      total=ctypes.byref(total)), **kw)
        return lib.sr_group_members_count(a["keys"], a["nq"], a["kg"], a["uniq"], a["G"], a["mptr"], a["mids"], a["n"], a["words"], a["n_masks"],
                                          a["n_bits"], a["qg"], a["out"], a["total"], None)

    def fill(**kw):
        a = dict(dict(keys=p, nq=2, kg=3, uniq=p, G=4, mptr=p, mids=p, n=9, words=None, n_masks=0, n_bits=0, qg=None, ptr=p, out=p, cap=9), **kw)
        return lib.sr_group_members_fill(a["keys"], a["nq"], a["kg"], a["uniq"], a["G"], a["mptr"], a["mids"], a["n"], a["words"], a["n_masks"],
                                         a["n_bits"], a["qg"], a["ptr"], a["out"], a["cap"], None)
    shared = [(dict(keys=None), b"null pointer"), (dict(uniq=None), b"null pointer"), (dict(mptr=None), b"null pointer"),
              (dict(mids=None), b"null pointer"), (dict(out=None), b"null pointer"), (dict(nq=-1), b"bad sizes"), (dict(kg=-1), b"bad sizes"),
              (dict(G=-1), b"bad member table"), (dict(n=-1), b"bad member table"), (dict(n=1 << 31), b"bad member table"),
              (dict(n_masks=-1), b"bad mask sizes"), (dict(n_masks=1, n_bits=-1, words=p), b"bad mask sizes"),
              (dict(n_masks=1, n_bits=64), b"without d_mask_words"), (dict(n_masks=3, n_bits=64, words=p), b"need d_query_group")]
    for change, text in shared + [(dict(total=None), b"null pointer")]:
        rc = count(**change)
        assert rc == _lib.SR_ERR_INVALID and text in lib.sr_last_error(), (change, rc, lib.sr_last_error())
    for change, text in shared + [(dict(ptr=None), b"null pointer"), (dict(cap=-1), b"bad capacity")]:
        rc = fill(**change)
        assert rc == _lib.SR_ERR_INVALID and text in lib.sr_last_error(), (change, rc, lib.sr_last_error())
    assert total.value == -1
    assert fill(nq=0) == _lib.SR_OK and fill(kg=0) == _lib.SR_OK


def test_front_ends_check_their_arguments_on_the_host():
    from scaling_retriever_amd.scoring import group_members_count, member_table_argument
    table = tuple(torch.from_numpy(t) for t in H.member_table_model(np.array([3, 1, 3], np.int32)))
    assert member_table_argument(table) is not None
    for bad, text in [((table[0], table[1]), "member_table returns"), ((table[0].long(), table[1], table[2]), "int32, int64, int64"),
                      ((table[0], table[1][:-1], table[2]), "one offset more")]:
        with pytest.raises(ValueError, match=text):
            group_members_count(torch.zeros((1, 1), dtype=torch.int32), bad)
    for bad in (torch.zeros((1, 1), dtype=torch.int64), torch.zeros(3, dtype=torch.int32), np.zeros((1, 1), np.int32)):
        with pytest.raises(ValueError, match=r"int32 \[nq, kg\]"):
            group_members_count(bad, table)


def test_hits_without_collapse_is_an_error():
    """hits= asks for the passages inside a collapsed search's groups: retrieve(hits=) without collapse= raises before anything else is
    looked at (the objects below are not even initialised), and so does --collapse_hits without --collapse_file."""
    from scaling_retriever_amd.indexer import HybridRetriever, SparseRetrieval
    with pytest.raises(ValueError, match="pass collapse= as well"):
        SparseRetrieval.retrieve(object.__new__(SparseRetrieval), None, 5, hits=2)
    with pytest.raises(ValueError, match="pass collapse= as well"):
        HybridRetriever.retrieve(object.__new__(HybridRetriever), None, 5, hits=2)
    import eval_dense
    import eval_sparse
    for mod in (eval_dense, eval_sparse):
        assert mod.parse_args([]).collapse_hits == 0
        assert mod.parse_args(["--collapse_file", "groups.tsv", "--collapse_hits", "3"]).collapse_hits == 3
        with pytest.raises(SystemExit):
            mod.parse_args(["--collapse_hits", "3"])
        with pytest.raises(SystemExit):
            mod.parse_args(["--collapse_file", "groups.tsv", "--collapse_hits", "65"])


def test_hits_argument_of_the_index_classes():
    from scaling_retriever_amd.scoring import hits_argument
    assert hits_argument("x", 1) == 1 and hits_argument("x", np.int64(64)) == 64
    for m in (0, 65, -3, 1.5, "3", True):
        with pytest.raises(ValueError, match=r"x: the number of hits must be an integer in \[1, 64\]"):
            hits_argument("x", m)


def test_pack_hits_on_cpu_tensors():
    from scaling_retriever_amd.collapse import pack_hits
    s = torch.arange(24, dtype=torch.float32).reshape(2, 4, 3)
    i = torch.arange(100, 124).reshape(2, 4, 3)
    c = torch.tensor([[2, 0, 7, 1], [0, 0, 0, 0]], dtype=torch.int32)          # 7: more hits than m = 3 - three of them are held
    ps, pi, pc = pack_hits(s, i, c)
    assert pc.tolist() == [6, 0]
    assert pi[0].tolist() == [100, 101, 106, 107, 108, 109] + [-1] * 6 and ps[0, :6].tolist() == [0, 1, 6, 7, 8, 9]
    assert (pi[1] == -1).all() and (ps[1] == 0).all()


def _first_hit_is_the_representative(S, keys, keep, threshold, k, m):
    ranking = C.full_ranking(S, keep=keep if threshold is None else (S > threshold if keep is None else keep & (S > threshold)))
    want = C.collapsed_ranking(ranking, keys, k)
    hs, hi, hc = H.hits_model(S, keys, want[2], keep, threshold, m, pad_score=np.float32(0.0) if threshold is not None else -H.FLT_MAX)
    valid = want[2] >= 0
    assert valid.sum() > 0 and (hc[valid] >= 1).all() and (hc[~valid] == 0).all()
    assert np.array_equal(hi[..., 0], want[1])
    assert np.array_equal(hs[..., 0][valid].view(np.uint32), want[0][valid].view(np.uint32))
    return int(valid.sum())


def test_models_first_hit_is_the_representative():
    """The invariant of the definition, on the models alone: 200 queries x 50 slots of dense_case() (10 000 slots), under a mask too, and
    sparse_case() at both thresholds."""
    D, Q, keys, S = C.dense_case()
    assert _first_hit_is_the_representative(S, keys, None, None, 50, 3) == 200 * 50
    flags = np.random.default_rng(11).random(C.N_DOCS) < 0.5
    _first_hit_is_the_representative(S[:40], keys, flags, None, 50, 2)
    *_, skeys, SS = C.sparse_case()
    for threshold in (0.0, -1.0):
        _first_hit_is_the_representative(SS, skeys, None, np.float32(threshold), 50, 3)


def test_segment_topm_model_on_a_hand_made_case():
    scores = np.array([1, 5, 5, -0.0, 0.0, 3, 3, 3], np.float32)
    ids = np.array([9, 8, 2, 7, 4, 30, 10, 20], np.int64)
    indptr = np.array([0, 3, 3, 5, 8])
    s, i, c = H.segment_topm_model(scores, ids, indptr, 2)
    assert i.tolist() == [[2, 8], [-1, -1], [4, 7], [10, 20]] and c.tolist() == [3, 0, 2, 3]
    assert s[0].tolist() == [5, 5] and s[1].tolist() == [-H.FLT_MAX] * 2 and not np.signbit(s[2]).any()
    s, i, c = H.segment_topm_model(scores, ids, indptr, 2, threshold=3.0, pad_score=0.0)
    assert i.tolist() == [[2, 8], [-1, -1], [-1, -1], [-1, -1]] and c.tolist() == [2, 0, 0, 0]
