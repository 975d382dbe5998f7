"""GPU: sr_token_counts (csrc/token_counts.hip) against the numpy model of tests/bm25_cases.py, torch.equal on all four outputs.

The table: every L below with every B and every padding, alternating 0 and 16 skip ids.
  L        1, 63, 64 (one register per lane) | 65, 128 (two) | 192, 256 (four: the last wave-per-row length) | 257, 1 024, 1 025, 8 192 =
           sr_token_counts_max_len() (a workgroup per row, 512 to 8 192 LDS slots)
  B        0, 1, 3, 257 (the wave kernel's last workgroup holds one row of four)
  padding  left, right (attention_mask; the masked slots hold ids with a non-zero upper half), none (NULL mask)
  rows     row 0: all ids distinct, with ids 0 and n_terms - 1 among them; row 1 (B >= 3, with a mask or skip ids): only padding or only
           skip ids - an empty row of length 0; row 2: one id L times; the rest: random lengths, ids from a small range so that they repeat.
Every case also runs twice (same bytes) and through bm25.token_counts_by_steps (same bytes)."""
import ctypes

import numpy as np
import pytest
import torch

import bm25_cases as bc

pytestmark = pytest.mark.gpu

N_TERMS = 20000
SKIP16 = list(range(100, 116))
LENGTHS = [1, 63, 64, 65, 128, 192, 256, 257, 1024, 1025, 8192]


def make_rows(B, L, pad, n_skip, seed):
    rng = np.random.default_rng(seed)
    skip = SKIP16[:n_skip]
    ids = rng.integers(0, 300, (B, L)).astype(np.int64)            # the skip ids 100 .. 115 occur among them
    mask = None
    if pad != "none":
        n_real = rng.integers(0, L + 1, B)
        n_real[:1] = L
        slot = np.arange(L)[None, :]
        mask = (slot >= L - n_real[:, None]) if pad == "left" else (slot < n_real[:, None])
        mask = mask.astype(np.int64)
    if B >= 1:
        row = rng.permutation(np.setdiff1d(np.arange(1, N_TERMS - 1), skip))[:L]
        row[0] = 0
        if L > 1:
            row[-1] = N_TERMS - 1
        ids[0] = row
    if B >= 3:
        if mask is not None:
            mask[1] = 0
        elif n_skip:
            ids[1] = rng.choice(skip, L)
        ids[2] = 777
        if mask is not None:
            mask[2] = 1
    if mask is not None:
        ids = np.where(mask != 0, ids, ids | (np.int64(1) << 40))     # never read as ids: outside int32, outside [0, n_terms)
    return ids, mask, skip


def check_case(ids, mask, skip):
    from scaling_retriever_amd import bm25
    from scaling_retriever_amd.scoring import token_counts
    want = bc.model_token_counts(ids, mask, skip, N_TERMS)
    t_ids = torch.from_numpy(ids).cuda()
    t_mask = None if mask is None else torch.from_numpy(mask).cuda()
    got = token_counts(t_ids, t_mask, skip, N_TERMS)
    for g, w, dt in zip(got, want, (torch.int64, torch.int32, torch.float32, torch.int32)):
        assert g.dtype == dt and torch.equal(g.cpu(), torch.from_numpy(w)), (ids.shape, g.dtype)
    again = token_counts(t_ids, t_mask, skip, N_TERMS)
    steps = bm25.token_counts_by_steps(t_ids, t_mask, skip, N_TERMS)
    for g, a, s in zip(got, again, steps):
        assert torch.equal(g, a) and g.dtype == s.dtype and torch.equal(g, s), ids.shape
    return got


@pytest.mark.parametrize("L", LENGTHS)
def test_token_counts_equal_the_model(L):
    case = 0
    for B in (0, 1, 3, 257):
        for pad in ("left", "right", "none"):
            ids, mask, skip = make_rows(B, L, pad, 16 if case % 2 else 0, seed=1000 * L + case)
            row_ptr, cols, vals, lens = check_case(ids, mask, skip)
            if B >= 3:
                assert int(vals[row_ptr[2]]) == L and int(lens[2]) == L and int(row_ptr[3] - row_ptr[2]) == 1      # one id, L times
                assert int(row_ptr[1] - row_ptr[0]) == L                                                          # all distinct
                if mask is not None or skip:
                    assert int(lens[1]) == 0 and int(row_ptr[2]) == int(row_ptr[1])                                # the empty row
            case += 1


def test_empty_shapes():
    from scaling_retriever_amd.scoring import token_counts
    row_ptr, cols, vals, lens = token_counts(torch.zeros((5, 0), dtype=torch.int64, device="cuda"), None, (), N_TERMS)
    assert row_ptr.tolist() == [0] * 6 and cols.numel() == 0 and vals.numel() == 0 and lens.tolist() == [0] * 5
    row_ptr, cols, vals, lens = token_counts(torch.zeros((0, 7), dtype=torch.int64, device="cuda"), None, (), N_TERMS)
    assert row_ptr.tolist() == [0] and cols.numel() == 0 and lens.numel() == 0
    with pytest.raises(ValueError, match="at most 8192"):
        token_counts(torch.zeros((1, 8193), dtype=torch.int64, device="cuda"), None, (), N_TERMS)
    with pytest.raises(ValueError, match="n_skip = 17"):
        token_counts(torch.zeros((1, 8), dtype=torch.int64, device="cuda"), None, range(17), N_TERMS)


def _raw_call(ids, mask, skip, cols, vals, lens, row_ptr, cap):
    from scaling_retriever_amd import _lib
    lib = _lib.load()
    n = ctypes.c_int64(-1)
    h_skip = (ctypes.c_int32 * 16)(*skip)
    rc = lib.sr_token_counts(ids.data_ptr(), None if mask is None else mask.data_ptr(), ids.shape[0], ids.shape[1], h_skip, len(skip), N_TERMS,
                             row_ptr.data_ptr(), cols.data_ptr(), vals.data_ptr(), lens.data_ptr(), cap, ctypes.byref(n), _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc, n.value, lib.sr_last_error().decode()


@pytest.mark.parametrize("L", [40, 600])
def test_capacity_one_short_then_a_second_call(L):
    from scaling_retriever_amd import _lib
    ids, mask, skip = make_rows(9, L, "left", 16, seed=3)
    want = bc.model_token_counts(ids, mask, skip, N_TERMS)
    nnz = int(want[0][-1])
    t_ids, t_mask = torch.from_numpy(ids).cuda(), torch.from_numpy(mask).cuda()
    cols = torch.full((nnz,), -5, dtype=torch.int32, device="cuda")
    vals = torch.full((nnz,), -5.0, dtype=torch.float32, device="cuda")
    lens = torch.full((9,), -5, dtype=torch.int32, device="cuda")
    row_ptr = torch.empty(10, dtype=torch.int64, device="cuda")
    rc, n, msg = _raw_call(t_ids, t_mask, skip, cols, vals, lens, row_ptr, nnz - 1)
    assert rc == _lib.SR_ERR_NOMEM and n == nnz and f"{nnz} entries, capacity {nnz - 1}" in msg
    assert bool((cols == -5).all()) and bool((vals == -5.0).all()) and bool((lens == -5).all())
    assert torch.equal(row_ptr.cpu(), torch.from_numpy(want[0]))
    rc, n, _ = _raw_call(t_ids, t_mask, skip, cols, vals, lens, row_ptr, nnz)
    assert rc == _lib.SR_OK and n == nnz
    for g, w in zip((row_ptr, cols, vals, lens), want):
        assert torch.equal(g.cpu(), torch.from_numpy(w))


@pytest.mark.parametrize("L", [50, 300])
def test_out_of_range_id_names_the_smallest_row_and_position(L):
    from scaling_retriever_amd import _lib
    from scaling_retriever_amd.scoring import token_counts
    ids, mask, skip = make_rows(7, L, "right", 16, seed=4)
    mask[:] = 1
    ids &= (1 << 40) - 1
    ids[5, L - 2] = -3
    ids[3, 9] = N_TERMS                    # the smallest (row, position)
    ids[3, 30] = N_TERMS + 7
    ids[4, 2] = 1 << 33                    # skipped below: no error by itself
    mask[4, 2] = 0
    t_ids, t_mask = torch.from_numpy(ids).cuda(), torch.from_numpy(mask).cuda()
    with pytest.raises(ValueError, match=rf"token id {N_TERMS} \(row 3, position 9\)"):
        token_counts(t_ids, t_mask, skip, N_TERMS)
    cols = torch.full((7 * L,), -5, dtype=torch.int32, device="cuda")
    vals = torch.full((7 * L,), -5.0, dtype=torch.float32, device="cuda")
    lens = torch.full((7,), -5, dtype=torch.int32, device="cuda")
    row_ptr = torch.empty(8, dtype=torch.int64, device="cuda")
    rc, _, msg = _raw_call(t_ids, t_mask, skip, cols, vals, lens, row_ptr, 7 * L)
    assert rc == _lib.SR_ERR_INVALID and "row 3, position 9" in msg
    assert bool((cols == -5).all()) and bool((vals == -5.0).all()) and bool((lens == -5).all())
    with pytest.raises(ValueError, match="row 3, position 9"):
        bc.model_token_counts(ids, mask, skip, N_TERMS)
