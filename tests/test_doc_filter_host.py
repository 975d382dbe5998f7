"""CPU: scaling_retriever_amd/doc_filter.py - the one resolver of a `mask=` / `masks=` argument (its host step and its device step, run
here with device="cpu"), the order "filter checks before any device work" on every filtered entry point of the two index classes, and
the one home of the "only one filter" rule."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

from scaling_retriever_amd import doc_filter
from scaling_retriever_amd.scoring import pack_doc_mask, pack_doc_masks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [0, 1, 31, 32, 33, 95]


def _resolve(given, n_bits, ndim=1):
    return doc_filter.mask_on_device(*doc_filter.mask_argument(given, lambda: n_bits, "n_bits", ndim), "cpu")


def _check(words, n_bits, want, n):
    """words: what the resolver returned for flags of n bits (per row); want: the packed words of the definition."""
    assert n_bits == n and torch.is_tensor(words) and words.dtype == torch.int32 and words.device.type == "cpu"
    assert words.data_ptr() != 0 and words.numel() >= 1                     # a valid pointer, also for an empty bitmap
    if n == 0:
        assert want.size == 0 and not bool(words.any())
        return
    got = words.numpy().view(np.uint32)
    assert got.shape == want.shape and np.array_equal(got, want)
    if n % 32:
        assert not (got[..., -1] >> np.uint32(n % 32)).any()                   # the unused bits of the last word


@pytest.mark.parametrize("n", SIZES)
def test_four_forms_of_a_mask_resolve_to_the_same_words(n):
    flags = np.random.default_rng(n).random(n) < 0.5
    want = pack_doc_mask(flags)
    assert want.dtype == np.uint32 and want.shape == ((n + 31) // 32,)
    packed_t = torch.from_numpy(want.view(np.int32).copy())
    for given in (flags, torch.from_numpy(flags), want, packed_t):
        words, n_bits = _resolve(given, n)
        _check(words, n_bits, want, n)
    if n:                                                                      # packed words that are already where they go are not copied
        assert _resolve(packed_t, n)[0].data_ptr() == packed_t.data_ptr()


@pytest.mark.parametrize("n_groups", [1, 3])
@pytest.mark.parametrize("n", SIZES)
def test_four_forms_of_stacked_masks_resolve_to_the_same_words(n, n_groups):
    flags = np.random.default_rng(100 * n_groups + n).random((n_groups, n)) < 0.5
    want_t = pack_doc_masks(flags)
    want = want_t.numpy().view(np.uint32)
    assert want.shape == (n_groups, (n + 31) // 32)
    for g in range(n_groups):
        assert np.array_equal(want[g], pack_doc_mask(flags[g]))
    for given in (flags, torch.from_numpy(flags), want.copy(), want_t.clone()):
        words, n_bits = _resolve(given, n, ndim=2)
        _check(words, n_bits, want, n)


def test_no_bits_give_a_valid_pointer():
    for given in (np.zeros(0, bool), torch.zeros(0, dtype=torch.bool), np.zeros(0, np.uint32), torch.zeros(0, dtype=torch.int32)):
        words, n_bits = _resolve(given, 0)
        assert n_bits == 0 and words.numel() == 1 and words.data_ptr() != 0 and int(words[0]) == 0
    words, n_bits = _resolve(np.zeros((2, 0), bool), 0, ndim=2)
    assert n_bits == 0 and words.numel() >= 1 and words.data_ptr() != 0


def test_n_bits_is_asked_only_for_packed_input():
    def never():
        raise AssertionError("the index was asked for its size")
    assert doc_filter.mask_argument(np.ones(40, bool), never, "n_bits")[1] is None
    assert doc_filter.mask_argument(torch.ones((2, 40), dtype=torch.bool), never, "n_bits", 2)[1] is None
    assert doc_filter.mask_argument(np.zeros(2, np.uint32), lambda: 40, "n_bits")[1] == 40


# the bad arguments of the issue's table, for a `mask=` of 100 bits (4 words) and for `masks=` of an empty dense index (0 words)
BAD_MASK = {"float dtype": np.ones(100, np.float32), "int64 dtype": np.ones(100, np.int64), "wrong rank": np.ones((4, 25), bool),
            "nested list of the wrong rank": [[True, False]], "wrong packed word count": np.zeros(5, np.uint32)}
BAD_MASKS = {"float dtype": np.ones((2, 4), np.float32), "int64 dtype": np.ones((2, 4), np.int64), "wrong rank": np.ones(4, bool),
             "nested list of the wrong rank": [True, False], "wrong packed word count": np.zeros((2, 1), np.uint32),
             "zero groups": np.zeros((0, 4), bool)}


@pytest.fixture
def handleless(monkeypatch):
    """(dense, sparse) index objects behind which no device work is possible: the dense one holds the handle of an empty index (made
    without a device; id_end = 0, asked for packed input), the sparse one holds nothing but n_docs."""
    from scaling_retriever_amd import _lib
    from scaling_retriever_amd.scoring import DenseIndexHIP, SparseIndexHIP
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.sr_dense_index_create(ctypes.byref(h), 64) == 0

    def no_device(*a, **k):
        raise AssertionError("the library was asked for a device")
    monkeypatch.setattr(_lib, "require_gpu", no_device)
    monkeypatch.setattr(_lib, "load", no_device)
    dense = object.__new__(DenseIndexHIP)
    dense.lib, dense._h, dense.dim = lib, h, 64                             # no `device`: nothing may get that far
    sparse = object.__new__(SparseIndexHIP)
    sparse.n_docs = 100
    yield dense, sparse
    dense.close()


@pytest.mark.parametrize("what", sorted(BAD_MASK))
def test_a_bad_mask_is_refused_before_any_device_work(handleless, what):
    dense, sparse = handleless
    bad = BAD_MASK[what]
    if what == "wrong packed word count":
        bad_dense = np.zeros(1, np.uint32)                                  # the empty index: a packed mask holds no word
    else:
        bad_dense = bad
    calls = [lambda: dense.search(None, 10, mask=bad_dense),
             lambda: dense.range_search(None, 0.0, mask=bad_dense),
             lambda: dense.range_count(None, 0.0, mask=bad_dense),
             lambda: dense.range_fill(None, None, None, 0, mask=bad_dense),
             lambda: sparse.search(None, None, None, 10, mask=bad),
             lambda: sparse.range_search(None, None, None, 0.0, mask=bad)]
    for call in calls:
        with pytest.raises(ValueError):
            call()


@pytest.mark.parametrize("what", sorted(BAD_MASKS))
def test_bad_stacked_masks_are_refused_before_any_device_work(handleless, what):
    dense, _ = handleless
    with pytest.raises(ValueError):
        dense.search_grouped(None, 10, BAD_MASKS[what], np.zeros(5, np.int64))


def test_one_filter_rule():
    doc_filter.one_filter("f", subset=None, mask=None)
    doc_filter.one_filter("f", subset=[1], mask=None)
    doc_filter.one_filter("f", np.ones((2, 4), bool), np.zeros(3, np.int64), allowed_ids=None, allowed_mask=None)
    with pytest.raises(ValueError, match="f: pass subset or mask, not both"):
        doc_filter.one_filter("f", subset=[1], mask=np.ones(4, bool))
    with pytest.raises(ValueError, match="g: pass allowed_ids or allowed_mask, not both"):
        doc_filter.one_filter("g", allowed_ids=["a"], allowed_mask=np.ones(4, bool))
    with pytest.raises(ValueError, match="not both"):
        doc_filter.one_filter("g", np.ones((2, 4), bool), np.zeros(3, np.int64), allowed_ids=["a"], allowed_mask=None)
    for pair in ((np.ones((2, 4), bool), None), (None, np.zeros(3, np.int64))):
        with pytest.raises(ValueError, match="go together"):
            doc_filter.one_filter("g", *pair, allowed_ids=None, allowed_mask=None)


def test_the_rule_is_spelled_out_in_one_module_only():
    package = os.path.join(ROOT, "scaling_retriever_amd")
    holders = sorted(os.path.relpath(p, package) for p in glob.glob(os.path.join(package, "**", "*.py"), recursive=True)
                     if "not both" in open(p).read())
    assert holders == ["doc_filter.py"], holders
