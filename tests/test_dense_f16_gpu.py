"""A dense index of fp16-stored rows (sr_dense_index_add_f16, DenseIndexHIP(row_dtype="fp16")).

The contract: every entry point returns, BIT FOR BIT, what the same call returns on "the twin" - an fp32 index whose rows are
the fp16 values widened to fp32 (widening is exact).  The reference of every comparison here is therefore the existing fp32
path on the same GPU, itself pinned to the oracle by the other suites.  The only loss of information is the one rounding at
ingest, checked against float64 below.

Shapes are the smallest that reach every kernel family: N = 863 = 3 * 256 + 95 (last tile in [1, 128]) and 129; H = 256 / 512
(streaming kernel, one / two query slabs) and 320 (a multiple of 64 but not of 256: tiled kernels for every nq, and the filter)."""
import ctypes
import json
import math
import os
import shutil
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}


def _data(N, H, nq_max=200):
    """(rows32, rows16, twin, queries) on the device, made once per shape and never modified."""
    key = (N, H)
    if key not in _CACHE:
        g = torch.Generator(device="cpu").manual_seed(1000 * N + H)
        rows32 = (torch.randn((N, H), generator=g) * (0.5 / math.sqrt(H))).cuda()
        rows16 = rows32.half()
        q = (torch.randn((nq_max, H), generator=g) / math.sqrt(H)).cuda()
        _CACHE[key] = (rows32, rows16, rows16.float(), q)
    return _CACHE[key]


def _pair(H, parts16, precision="fp32", batch_invariant=False, ids=None):
    """(fp16 index, twin) over the same segments: parts16 = list of float16 cuda tensors; ids = [(id_base, id_stride)] per part."""
    from scaling_retriever_amd.scoring import DenseIndexHIP
    f16, twin = DenseIndexHIP(H), DenseIndexHIP(H)
    for idx in (f16, twin):
        if precision != "fp32":
            idx.set_precision(precision)
        if batch_invariant:
            idx.set_batch_invariant(True)
    for i, part in enumerate(parts16):
        kw = {} if ids is None else {"id_base": ids[i][0], "id_stride": ids[i][1]}
        f16.add_device_rows(part, **kw)
        twin.add_device_rows(part.float(), **kw)
    assert f16.stored_dtype() == "fp16" and twin.stored_dtype() == "fp32"
    return f16, twin


def _same_search(f16, twin, q, k):
    s16, i16 = f16.search(q, k)
    s32, i32 = twin.search(q, k)
    assert torch.equal(i16, i32), "ids differ from the twin"
    assert torch.equal(s16.view(torch.int32), s32.view(torch.int32)), "score bits differ from the twin"
    return s16, i16


# (N, H, nq, k, precision, batch-invariant): every kernel family at least once, every value of every parameter at least once.
#   streaming kernel (H % 256 == 0, nq <= 64, not batch-invariant): 1, 2, 3 and 4 query blocks, one and two query slabs
#   tiled kernels for nq <= 32 / <= 64 (H = 320, or batch-invariant), pipelined kernel for 65..128 and > 128 queries
#   certified filter (fp32_filtered, nq > 64): plane built from the fp16 rows, upper-bound pass, exact re-score of fp16 rows
SEARCH_CASES = [
    (863, 256, 1, 1, "fp32", False),
    (863, 256, 16, 10, "fp32", False),
    (863, 256, 17, 100, "fp32", False),
    (863, 512, 33, 10, "fp32", False),
    (863, 512, 64, 868, "fp32", False),
    (129, 256, 64, 10, "fp32", True),
    (863, 256, 16, 10, "fp32", True),
    (863, 320, 1, 10, "fp32", False),
    (863, 320, 17, 100, "fp32_filtered", False),
    (863, 320, 33, 1, "fp32", False),
    (863, 320, 65, 10, "fp32", False),
    (129, 320, 129, 100, "fp32", False),
    (863, 320, 200, 868, "fp32", False),
    (863, 320, 65, 10, "fp32_filtered", False),
    (863, 320, 129, 100, "fp32_filtered", False),
    (863, 512, 200, 10, "fp32_filtered", True),
    (129, 256, 200, 1, "fp32_filtered", False),
    (129, 512, 65, 134, "fp32_filtered", False),
]


@pytest.mark.parametrize("N,H,nq,k,precision,bi", SEARCH_CASES)
def test_twin_identity_search(N, H, nq, k, precision, bi):
    _, rows16, _, q = _data(N, H)
    f16, twin = _pair(H, [rows16], precision, bi)
    _same_search(f16, twin, q[:nq].contiguous(), k)


def test_twin_identity_two_strided_segments():
    _, rows16, _, q = _data(863, 320)
    parts, ids = [rows16[1::2].contiguous(), rows16[0::2].contiguous()], [(1, 2), (0, 2)]
    for precision, nq in (("fp32", 16), ("fp32", 129), ("fp32_filtered", 129)):
        f16, twin = _pair(320, parts, precision, False, ids)
        s, i = _same_search(f16, twin, q[:nq].contiguous(), 100)
        assert bool((i % 2 == 0).any()) and bool((i % 2 == 1).any())       # documents of both segments are among the results
    _, rows16, _, q = _data(863, 256)
    f16, twin = _pair(256, [rows16[1::2].contiguous(), rows16[0::2].contiguous()], "fp32", False, ids)
    _same_search(f16, twin, q[:16].contiguous(), 100)           # streaming kernel


def test_twin_identity_k_above_the_in_lds_top_k():
    _, rows16, _, q = _data(6000, 256)
    f16, twin = _pair(256, [rows16])
    assert 5000 > f16.lib.sr_max_topk()
    _same_search(f16, twin, q[:70].contiguous(), 5000)


def test_twin_identity_begin_finish():
    _, rows16, _, q = _data(863, 320)
    f16, twin = _pair(320, [rows16], "fp32_filtered")
    q = q[:129].contiguous()
    out = []
    for idx in (f16, twin):
        lower = idx.search_begin(q, 100, 2)
        s, i = idx.search_finish(q, 100, lower)
        out.append((lower, s, i))
    assert torch.isfinite(out[1][0]).any()                      # the filter applied: real thresholds, not -inf throughout
    for a, b in zip(out[0], out[1]):
        assert torch.equal(a, b)


def test_twin_identity_score_pairs():
    _, rows16, _, q = _data(863, 320)
    parts, ids = [rows16[1::2].contiguous(), rows16[0::2].contiguous()], [(1, 2), (0, 2)]
    f16, twin = _pair(320, parts, "fp32", False, ids)
    rng = np.random.default_rng(5)
    for nq in (1, 200):
        lens = rng.integers(0, 90, size=nq)
        lens[0] = 70                                            # more than one 64-pair tile
        if nq > 3:
            lens[1] = lens[3] = 0                               # empty lists
        indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        cand = rng.integers(0, 863, size=int(indptr[-1])).astype(np.int64)      # both segments
        cand[1] = cand[0]                                       # a repeated candidate
        a = f16.score_pairs(q[:nq].contiguous(), indptr, cand)
        b = twin.score_pairs(q[:nq].contiguous(), indptr, cand)
        assert a.numel() == int(indptr[-1]) and torch.equal(a.view(torch.int32), b.view(torch.int32))
    # the pair scores are the search's scores (more than 64 queries: the same k order)
    s, i = f16.search(q[:129].contiguous(), 5)
    p = f16.score_pairs(q[:129].contiguous(), np.arange(130, dtype=np.int64) * 5, i.reshape(-1))
    assert torch.equal(p, s.reshape(-1))
    msgs = []
    for idx in (f16, twin):
        with pytest.raises(ValueError) as e:
            idx.score_pairs(q[:2].contiguous(), np.array([0, 1, 3], np.int64), np.array([5, 7, 4000], np.int64))
        msgs.append(str(e.value))
    assert msgs[0] == msgs[1] and "4000" in msgs[0]


def _special_rows(H, N=300):
    """Normal rows with a block of 32 rows of fp16 specials: whole rows of subnormals (a flushed denormal would score 0), rows
    mixing subnormals, +-0 and +-65504, and one row of the largest finite value."""
    _, rows16, _, q = _data(863, H)
    rows = rows16[:N].clone()
    rng = np.random.default_rng(77 + H)
    bits = rng.integers(1, 1024, (32, H)).astype(np.uint16) | (rng.integers(0, 2, (32, H)).astype(np.uint16) << 15)   # subnormals, either sign
    specials = np.array([0x0000, 0x8000, 0x7BFF, 0xFBFF, 0x0001, 0x8001], dtype=np.uint16)           # +-0, +-65504, +-2^-24
    assert specials.view(np.float16)[2] == 65504 and specials.view(np.float16)[3] == -65504
    bits[8:24] = specials[rng.integers(0, 6, (16, H))]
    normal = rows[:8].cpu().numpy().view(np.uint16)
    bits[24:32] = np.where(rng.random((8, H)) < 0.5, bits[24:32], normal)                             # specials among normal values
    bits[23] = specials[2]
    block = torch.from_numpy(bits.view(np.float16))
    rows[100:132] = block.cuda()
    return rows, q


@pytest.mark.parametrize("H,nq,precision", [(256, 16, "fp32"), (320, 16, "fp32"), (320, 129, "fp32"), (320, 129, "fp32_filtered")])
def test_special_values_equal_the_twin(H, nq, precision):
    rows, q = _special_rows(H)
    f16, twin = _pair(H, [rows], precision)
    s, i = _same_search(f16, twin, q[:nq].contiguous(), rows.shape[0] + 5)     # every row's score is compared
    # the all-subnormal rows (100..107) score like the float64 product of their exact values: nothing was flushed to zero
    ref = q[:nq].double() @ rows[100:108].double().T
    got = torch.zeros_like(ref)
    for r in range(100, 108):
        got[:, r - 100] = s[i == r].double()
    # (fp32 chain of H products of magnitude <= |q_i| 2^-14: its error is far below 1e-3 of the largest score; a flush gives 0)
    assert float(ref.abs().max()) > 0 and float((got - ref).abs().max()) <= 1e-3 * float(ref.abs().max())


def test_filter_runs_on_an_fp16_index():
    _, rows16, _, q = _data(863, 320)
    f16, twin = _pair(320, [rows16], "fp32_filtered")
    _same_search(f16, twin, q[:200].contiguous(), 10)
    c16, c32 = f16.filter_query_stats()[0], twin.filter_query_stats()[0]
    assert c16 >= 1 and c16 >= c32, (c16, c32)


def test_memory_no_fp32_copy_anywhere():
    from scaling_retriever_amd.scoring import DenseIndexHIP
    N, H = 863, 320
    _, rows16, _, q = _data(N, H)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    idx = DenseIndexHIP(H)
    idx.add_device_rows(rows16)
    assert torch.cuda.memory_allocated() - before < N * H * 2      # the tensor is kept as it is: no fp32 (4 N H) copy, no copy at all
    for nq in (16, 200):
        idx.search(q[:nq].contiguous(), 10)
    idx.score_pairs(q[:4].contiguous(), np.array([0, 1, 2, 3, 4], np.int64), np.arange(4, dtype=np.int64))
    assert idx.owned_bytes() == 0                                  # fp32 mode: the library holds nothing per segment
    idx.set_precision("fp32_filtered")
    idx.search(q[:200].contiguous(), 10)
    assert idx.filter_query_stats()[0] >= 1
    # sr_dense_index_owned_bytes counts the bytes the library asked for: one fp16 plane and 8 bytes per document and per group of
    # 128 documents.  The device allocator then rounds each of those two allocations up to its own granularity (whole pages), which
    # this figure does not contain - so the bound holds without any rounding term.
    owned = idx.owned_bytes()
    assert 0 < owned <= 2 * N * H + 8 * (N + -(-N // 128)), owned
    twin = DenseIndexHIP(H)
    twin.set_precision("fp32_filtered")
    twin.add_device_rows(rows16.float())
    assert twin.owned_bytes() == owned                             # resident: 2 + 2 bytes per element instead of 4 + 2


def test_rounding_at_ingest(tmp_path):
    from scaling_retriever_amd.scoring import DenseIndexHIP
    N, H, nq, k = 863, 256, 65, 50
    rows32, rows16, _, q = _data(N, H)
    q = q[:nq].contiguous()
    base = DenseIndexHIP(H)
    base.add_device_rows(rows16)
    want_s, want_i = base.search(q, k)
    np.save(tmp_path / "embs16.npy", rows16.cpu().numpy())
    a, b, c, d = (DenseIndexHIP(H, row_dtype="fp16") for _ in range(4))
    a.add_device_rows(rows32)
    b.add_host_rows(rows32.cpu().numpy(), piece_bytes=100 * H * 4)           # several staged pieces, each rounded on the device
    c.add_npy_file(str(tmp_path / "embs16.npy"), piece_bytes=100 * H * 2)
    d.add_host_rows(rows16.cpu().numpy())
    for idx in (a, b, c, d):
        assert idx.stored_dtype() == "fp16" and idx._segments[0].dtype == torch.float16
        s, i = idx.search(q, k)
        assert torch.equal(i, want_i) and torch.equal(s, want_s)
    # against float64 with the UNROUNDED rows: one rounding to 11 significant bits per element, then the fp32 chain of H terms
    exact = q.double() @ rows32.double().T
    qn, dn = q.double().norm(dim=1), rows32.double().norm(dim=1)
    bound = (2.0 ** -11 * (1 + 2.0 ** -10) + 4 * H * 2.0 ** -24) * qn[:, None] * dn[None, :]
    err = (want_s.double() - torch.gather(exact, 1, want_i)).abs()
    lim = torch.gather(bound, 1, want_i)
    print("rounding at ingest: max error / bound =", float((err / lim).max()))
    assert bool((err <= lim).all())
    bad = rows32[:40].clone()
    bad[17, 3] = 1e5
    with pytest.raises(ValueError, match="row 17"):
        DenseIndexHIP(H, row_dtype="fp16").add_device_rows(bad)
    with pytest.raises(ValueError, match="row 17"):
        DenseIndexHIP(H, row_dtype="fp16").add_host_rows(bad.cpu().numpy())


def test_staging_ring_is_one_for_both_entry_points(tmp_path):
    """add_host_rows (array, memory-mapped view) and add_npy_file share one pinned ring: 1 000 rows in pieces of 96 make 11 pieces with a
    ragged last one, through 3 buffers and 2 threads, so every buffer is used again.  Each way produces, bit for bit, the segment
    add_device_rows makes of the same data, in all three staging modes."""
    from scaling_retriever_amd.scoring import DenseIndexHIP
    N, H = 1000, 64
    g = torch.Generator(device="cpu").manual_seed(7)
    rows32 = torch.randn((N, H), generator=g).numpy()
    rows16 = rows32.astype(np.float16)
    ring = dict(n_buffers=3, n_threads=2)

    def segments(src, row_dtype):
        """The segment each of the three ways makes of `src`, and the one add_device_rows makes."""
        path = str(tmp_path / f"rows_{src.dtype}_{len(src)}.npy")
        np.save(path, src)
        piece = 96 * H * src.dtype.itemsize
        made = []
        for add in (lambda i: i.add_host_rows(src, piece_bytes=piece, **ring),
                    lambda i: i.add_host_rows(np.load(path, mmap_mode="r"), piece_bytes=piece, **ring),
                    lambda i: i.add_npy_file(path, piece_bytes=piece, **ring),
                    lambda i: i.add_device_rows(torch.from_numpy(src).cuda())):
            idx = DenseIndexHIP(H, row_dtype=row_dtype)
            add(idx)
            assert len(idx._segments) == 1 and idx.ntotal == len(src)
            made.append(idx._segments[0])
        return made[:3], made[3]

    for src, row_dtype, want in ((rows32, "fp32", torch.from_numpy(rows32)),                 # fp32 source into an fp32 index
                                 (rows16, "fp32", torch.from_numpy(rows16)),                 # fp16 source: stored as it is, either index
                                 (rows16, "fp16", torch.from_numpy(rows16)),
                                 (rows32, "fp16", torch.from_numpy(rows32).half())):         # fp32 source, rounded on the device
        staged, direct = segments(src, row_dtype)
        assert direct.dtype == want.dtype and torch.equal(direct.cpu(), want)
        for seg in staged:
            assert seg.dtype == direct.dtype and seg.shape == direct.shape and seg.device == direct.device
            assert torch.equal(seg.view(torch.int16 if seg.dtype == torch.float16 else torch.int32),
                               direct.view(torch.int16 if seg.dtype == torch.float16 else torch.int32))
    # a value float16 cannot hold, in the tenth piece: both entry points name the row
    bad = rows32.copy()
    bad[917, 5] = 70000.0
    np.save(tmp_path / "bad.npy", bad)
    with pytest.raises(ValueError, match="row 917"):
        DenseIndexHIP(H, row_dtype="fp16").add_host_rows(bad, piece_bytes=96 * H * 4, **ring)
    with pytest.raises(ValueError, match="row 917"):
        DenseIndexHIP(H, row_dtype="fp16").add_npy_file(str(tmp_path / "bad.npy"), piece_bytes=96 * H * 4, **ring)
    # no rows: an empty segment
    staged, direct = segments(rows32[:0], "fp32")
    assert all(seg.shape == (0, H) and seg.dtype == torch.float32 for seg in staged + [direct])


def test_errors():
    from scaling_retriever_amd import _lib
    lib = _lib.load()
    H = 256
    _, rows16, twin_rows, _ = _data(863, H)
    p16, p32 = ctypes.c_void_p(rows16.data_ptr()), ctypes.c_void_p(twin_rows.data_ptr())

    def new():
        h = ctypes.c_void_p()
        assert lib.sr_dense_index_create(ctypes.byref(h), H) == 0
        return h
    h = new()
    assert lib.sr_dense_index_row_dtype(h) == _lib.SR_DTYPE_F32                     # empty
    assert lib.sr_dense_index_add_f16(h, p16, 100, 0, 1) == 0
    assert lib.sr_dense_index_row_dtype(h) == _lib.SR_DTYPE_F16
    assert lib.sr_dense_index_add(h, p32, 100, 100, 1) == _lib.SR_ERR_INVALID and b"fp16" in lib.sr_last_error()
    assert lib.sr_dense_index_ntotal(h) == 100 and lib.sr_dense_index_row_dtype(h) == _lib.SR_DTYPE_F16
    assert lib.sr_dense_index_add_f16(h, None, 5, 100, 1) == _lib.SR_ERR_INVALID
    assert lib.sr_dense_index_ntotal(h) == 100
    for mode in (1, 2):                                                             # bf16x3, bf16x6
        assert lib.sr_dense_index_set_precision(h, mode) == _lib.SR_ERR_UNSUPPORTED
    assert lib.sr_dense_index_set_precision(h, 3) == 0
    assert lib.sr_dense_index_destroy(h) == 0
    h = new()
    assert lib.sr_dense_index_add(h, p32, 100, 0, 1) == 0
    assert lib.sr_dense_index_add_f16(h, p16, 100, 100, 1) == _lib.SR_ERR_INVALID and b"fp32" in lib.sr_last_error()
    assert lib.sr_dense_index_ntotal(h) == 100 and lib.sr_dense_index_row_dtype(h) == _lib.SR_DTYPE_F32
    assert lib.sr_dense_index_destroy(h) == 0
    for mode in (1, 2):                     # an empty index already in a split mode refuses fp16 rows
        h = new()
        assert lib.sr_dense_index_set_precision(h, mode) == 0
        assert lib.sr_dense_index_add_f16(h, p16, 100, 0, 1) == _lib.SR_ERR_UNSUPPORTED
        assert lib.sr_dense_index_ntotal(h) == 0 and lib.sr_dense_index_row_dtype(h) == _lib.SR_DTYPE_F32
        assert lib.sr_dense_index_destroy(h) == 0
    from scaling_retriever_amd.scoring import DenseIndexHIP
    idx = DenseIndexHIP(H)
    idx.add_device_rows(rows16)
    with pytest.raises(_lib.SrHipError):
        idx.set_precision("bf16x3")
    with pytest.raises(ValueError):
        idx.add_device_rows(twin_rows)
    with pytest.raises(ValueError):
        DenseIndexHIP(H, row_dtype="bf16")


def test_flat_indexer_with_fp16_storage(tmp_path):
    from scaling_retriever_amd.indexer import DenseFlatIndexer
    N, H = 863, 320
    rows32, rows16, twin_rows, q = _data(N, H)
    ids = [f"d{i}" for i in range(N)]
    a, b = DenseFlatIndexer(), DenseFlatIndexer()
    a.init_index(H, storage="fp16")
    b.init_index(H)
    a.index_data(rows32.cpu().numpy(), ids)
    b.index_data(twin_rows.cpu().numpy(), ids)
    assert a.index.stored_dtype() == "fp16" and b.index.stored_dtype() == "fp32"
    qh = q[:129].cpu().numpy()

    def same(x, y):
        ids_x, s_x = x.search_knn(qh, 10)
        ids_y, s_y = y.search_knn(qh, 10)
        assert ids_x == ids_y and np.array_equal(s_x, s_y)
        for u, v in zip(x.search_arrays(qh[:7], 20), y.search_arrays(qh[:7], 20)):
            assert np.array_equal(u, v)
        lists = [[f"d{(7 * r + j) % N}" for j in range(r % 5)] for r in range(20)]
        ru, rv = x.score_candidates(qh[:20], lists), y.score_candidates(qh[:20], lists)
        assert np.array_equal(ru.scores, rv.scores) and np.array_equal(ru.positions, rv.positions) and np.array_equal(ru.counts, rv.counts)
    same(a, b)
    os.makedirs(tmp_path / "ix")
    a.serialize(str(tmp_path / "ix"))
    assert np.load(tmp_path / "ix" / "index.dpr").dtype == np.float16          # the dtype is kept: half the file
    c = DenseFlatIndexer()
    c.deserialize(str(tmp_path / "ix"))
    assert c.index.stored_dtype() == "fp16" and c.storage == "fp16"
    same(c, b)


def test_eval_dense_index_dtype_fp16(golden_dir, tmp_path):
    """eval_dense.py --index_dtype fp16 on the drivers' tiny collection: the run.json is byte for byte the one an fp32 index writes
    from shard files that were rounded to fp16 and widened again beforehand."""
    sys.path.insert(0, ROOT)
    import eval_dense
    from golden_weights import make_weights
    from test_eval_drivers import _texts, _write_model
    z = np.load(os.path.join(golden_dir, "enc_tiny_a.npz"))
    cfg = json.loads(str(z["config_json"]))
    rng = np.random.default_rng(3)
    lora, _ = _write_model(str(tmp_path), cfg, make_weights(cfg, int(z["weight_seed"])), rng)["dense"]
    with open(tmp_path / "corpus.tsv", "w") as f:
        for i, t in enumerate(_texts(rng, 60, 3, 20)):
            f.write(f"d{i}\t{t}\n")
    with open(tmp_path / "queries.tsv", "w") as f:
        for i, t in enumerate(_texts(rng, 6, 2, 6)):
            f.write(f"q{i}\t{t}\n")
    emb, emb_r = str(tmp_path / "embs"), str(tmp_path / "embs_rounded")
    eval_dense.main(["--task_name", "write_doc_embeds", "--model_name_or_path", lora, "--corpus_path", str(tmp_path / "corpus.tsv"),
                     "--doc_embed_dir", emb, "--eval_batch_size", "16", "--doc_max_length", "16", "--chunk_size", "32", "--token_budget", "0"])
    shutil.copytree(emb, emb_r)
    n_shards = 0
    for name in os.listdir(emb_r):
        if name.startswith("embs_") and name.endswith(".npy"):
            x = np.load(os.path.join(emb, name))
            assert x.dtype == np.float32                      # the artefacts stay fp32: rounding happens at ingest
            np.save(os.path.join(emb_r, name), x.astype(np.float16).astype(np.float32))
            n_shards += 1
    assert n_shards == 2
    runs = []
    for d, out, extra in ((emb, "out16", ["--index_dtype", "fp16"]), (emb_r, "out32", [])):
        eval_dense.main(["--task_name", "retrieval", "--model_name_or_path", lora, "--query_path", str(tmp_path / "queries.tsv"),
                         "--doc_embed_dir", d, "--out_dir", str(tmp_path / out), "--top_k", "10", "--query_max_length", "8"] + extra)
        runs.append(open(tmp_path / out / "run.json", "rb").read())
    assert len(json.loads(runs[0])) == 6 and runs[0] == runs[1]
