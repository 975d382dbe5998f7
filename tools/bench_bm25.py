#!/usr/bin/env python3
"""BM25 on the device, measured: sr_token_counts and sr_bm25_weights against the compositions of torch calls a caller
has without them (scaling_retriever_amd.bm25.token_counts_by_steps, bm25_weights_by_steps), the whole indexing pipeline, and the search
of a BM25-weighted index through the unchanged sr_sparse_search.

Legs (--legs, default all but `parent`, which needs --parent-lib):
  counts    token rows over V = 128 256 (log-uniform ids: Zipf with exponent 1; left padding, row lengths between L / 4 and L) at the
            shapes of --shapes: equal bytes first, then HIP events around each call, the variants alternating inside a round, median of
            --reps rounds; the composition is timed twice per round, the difference of its two medians is the spread.  Then the sweep of
            the row length at which the wave-per-row and the workgroup-per-row kernels cross (dev switch SR_TC_WAVE_MAX_LEN = 0 sends
            every row to the workgroup kernel).
  weights   a term-major index of n_docs x --l0-d postings (MS MARCO at about 50 distinct tokens per passage: 4.4e8) and a tenth of it.
  pipeline  Bm25Indexer.index from pre-tokenised chunks at --passages passages: passages per second, and the milliseconds inside
            sr_token_counts, sr_sparse_csr_build and (when the index is opened) sr_bm25_weights.
  search    --nq queries of 6 - 8 tokens at k = --k on the weighted full-size index (median of --reps calls after one warm-up call):
            queries per second and the share of queries the certified scorer handed back to the exact kernels.
  parent    sr_sparse_search at BASELINE.json configs[2]'s shape (L0_d = 128, L0_q = 32 learned-style weights) on this build, on the
            parent commit's library (--parent-lib) and on the parent's again: this build must be within the spread of the two parent
            runs plus one percent.
Writes one JSON document (default profiles/bm25.json) and prints it.

  python tools/bench_bm25.py                                  # full size, one MI355X
  python tools/bench_bm25.py --scale 0.02 --passages 32768    # a quick look
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ["SR_DEV_SWITCHES"] = "1"

from synth import build_index, build_queries  # noqa: E402

SHAPES = "2048:64,16384:192,256:192,4096:512,64:8192"
SKIP = (1, 2)
TC_WAVE_MAX_LEN = 256     # csrc/token_counts.hip: the sweep covers the lengths the wave kernel exists for
HBM_GBPS = 8000.0          # MI355X: 8 TB/s of HBM3E, the figure the rates below are set against


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b)


def alternating(variants, reps, warmup=1):
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    ms = {name: [] for name in variants}
    for _ in range(reps):
        for name, fn in variants.items():
            ms[name].append(once(fn)[1])
    return ms


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "runs": len(ms)}


def same_bytes(a, b):
    return all(x.shape == y.shape and x.dtype == y.dtype and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))
               for x, y in zip(a, b))


def compared(kernel, composition, reps, what):
    got, want = kernel(), composition()
    got, want = (got, want) if isinstance(got, tuple) else ((got,), (want,))
    assert same_bytes(got, want), f"kernel and composition differ: {what}; nothing was timed"
    del got, want
    ms = alternating({"kernel": kernel, "composition": composition, "composition_again": composition}, reps)
    kern, comp, comp2 = summary(ms["kernel"]), summary(ms["composition"]), summary(ms["composition_again"])
    spread = abs(comp["median_ms"] - comp2["median_ms"])
    return {"outputs_equal_bytes": True, "kernel": kern, "composition": comp, "composition_again": comp2, "composition_spread_ms": round(spread, 4),
            "kernel_speedup_over_composition": round(min(comp["median_ms"], comp2["median_ms"]) / kern["median_ms"], 2),
            "kernel_not_slower_beyond_the_spread": bool(kern["median_ms"] <= min(comp["median_ms"], comp2["median_ms"]) + spread)}


def token_rows(B, L, V, dev, seed):
    """(ids int64 [B, L], mask int64 [B, L]): log-uniform ids (Zipf, exponent 1), left padding, between L / 4 and L real slots a row."""
    g = torch.Generator(device=dev).manual_seed(seed)
    ids = (torch.exp(torch.rand((B, L), device=dev, generator=g) * float(np.log(V - 3))).to(torch.int64) + 2).clamp_(max=V - 1)
    real = torch.randint(max(1, L // 4), L + 1, (B,), device=dev, generator=g)
    mask = (torch.arange(L, device=dev)[None, :] >= (L - real)[:, None]).to(torch.int64)
    return ids, mask


def counts_leg(a, dev):
    from scaling_retriever_amd.bm25 import token_counts_by_steps
    from scaling_retriever_amd.scoring import token_counts
    out = {"vocab": a.vocab, "shapes": [], "sweep": []}
    for B, L in [tuple(int(x) for x in s.split(":")) for s in a.shapes.split(",")]:
        ids, mask = token_rows(B, L, a.vocab, dev, 7)
        leg = {"B": B, "L": L}
        leg.update(compared(lambda: token_counts(ids, mask, SKIP, a.vocab), lambda: token_counts_by_steps(ids, mask, SKIP, a.vocab), a.reps, leg))
        read = 2 * B * L * 16                                    # ids and mask, once for the count and once for the fill
        leg["bytes_read"] = read
        leg["read_GBps"] = round(read / (leg["kernel"]["median_ms"] * 1e-3) / 1e9, 1)
        leg["share_of_hbm"] = round(leg["read_GBps"] / HBM_GBPS, 4)
        out["shapes"].append(leg)
        print("[counts]", json.dumps(leg), file=sys.stderr, flush=True)
    for L in (16, 32, 64, 96, 128, 160, 192, 224, 256):
        ids, mask = token_rows(a.sweep_rows, L, a.vocab, dev, 8)

        def block():
            os.environ["SR_TC_WAVE_MAX_LEN"] = "0"
            try:
                return token_counts(ids, mask, SKIP, a.vocab)
            finally:
                del os.environ["SR_TC_WAVE_MAX_LEN"]
        assert same_bytes(token_counts(ids, mask, SKIP, a.vocab), block())
        ms = alternating({"wave": lambda: token_counts(ids, mask, SKIP, a.vocab), "block": block}, a.reps)
        row = {"B": a.sweep_rows, "L": L, "wave_per_row": summary(ms["wave"]), "workgroup_per_row": summary(ms["block"])}
        row["wave_over_workgroup"] = round(row["wave_per_row"]["median_ms"] / row["workgroup_per_row"]["median_ms"], 3)
        out["sweep"].append(row)
        print("[sweep]", json.dumps(row), file=sys.stderr, flush=True)
    # the library's switch (TC_WAVE_MAX_LEN, csrc/token_counts.hip) is the longest row the wave kernel is instantiated for; the sweep
    # says whether the wave kernel should serve every length up to it
    out["library_switch_rows_up_to"] = TC_WAVE_MAX_LEN
    wins = [r["L"] for r in out["sweep"] if r["wave_over_workgroup"] < 1.0]
    out["wave_kernel_wins_at"] = wins
    out["switch_agrees_with_sweep"] = wins == [r["L"] for r in out["sweep"] if r["L"] <= TC_WAVE_MAX_LEN]
    return out


def tf_index(V, N, l0_d, dev, seed):
    """(indptr, doc_ids, tf, doc_len): the synthetic index of tools/synth.py with small integer frequencies as values, and the document
    lengths they imply."""
    indptr, doc_ids, vals, _ = build_index(V, N, l0_d, dev, seed)
    del vals
    g = torch.Generator(device=dev).manual_seed(seed + 1)
    tf = torch.randint(1, 5, (doc_ids.numel(),), device=dev, generator=g).to(torch.float32)
    doc_len = torch.zeros(N, dtype=torch.float32, device=dev).index_add_(0, doc_ids.long(), tf).to(torch.int32)
    return indptr, doc_ids, tf, doc_len


def weights_leg(a, N, dev):
    from scaling_retriever_amd import bm25
    from scaling_retriever_amd.scoring import bm25_weights
    out = []
    keep = None
    for n in (max(4096, N // 10), N):
        indptr, doc_ids, tf, doc_len = tf_index(a.vocab, n, a.l0_d, dev, 3)
        nnz = int(tf.numel())
        avgdl = bm25.average_length(int(doc_len.sum(dtype=torch.int64)), n)
        scal = bm25.bm25_scalars(0.9, 0.4, avgdl)
        idf = torch.from_numpy(bm25.idf_table((indptr[1:] - indptr[:-1]).cpu().numpy(), n)).to(dev)
        leg = {"n_docs": n, "postings": nnz}
        leg.update(compared(lambda: bm25_weights(indptr, doc_ids, tf, doc_len, idf, *scal),
                            lambda: bm25.bm25_weights_by_steps(indptr, doc_ids, tf, doc_len, idf, *scal), a.reps, leg))
        moved = 16 * nnz                                         # 12 bytes of streams and the 4 gathered bytes per posting
        leg["bytes_moved"] = moved
        leg["GBps"] = round(moved / (leg["kernel"]["median_ms"] * 1e-3) / 1e9, 1)
        leg["share_of_hbm"] = round(leg["GBps"] / HBM_GBPS, 4)
        out.append(leg)
        print("[weights]", json.dumps(leg), file=sys.stderr, flush=True)
        keep = (indptr, doc_ids, bm25_weights(indptr, doc_ids, tf, doc_len, idf, *scal), n)
        del tf, doc_len, idf
        torch.cuda.empty_cache()
    return out, keep


def pipeline_leg(a, dev):
    from scaling_retriever_amd import bm25
    from scaling_retriever_amd.dataset.pipeline import TokenBudgetCollectionLoader
    rng = np.random.default_rng(5)
    chunks, n = [], 0
    while n < a.passages:
        c = min(32768, a.passages - n)
        lens = rng.integers(30, 121, c).astype(np.int32)
        flat = (np.exp(rng.random(int(lens.sum())) * np.log(a.vocab - 3)).astype(np.int64) + 2).clip(max=a.vocab - 1).astype(np.int32)
        chunks.append((list(range(n, n + c)), flat, lens))
        n += c
    spent = {"sr_token_counts": 0.0, "sr_sparse_csr_build": 0.0, "sr_bm25_weights": 0.0}

    def timed(name, fn):
        def call(*args, **kw):
            out, ms = once(lambda: fn(*args, **kw))
            spent[name] += ms
            return out
        return call
    real = (bm25.token_counts, bm25.sparse_csr_build, bm25.bm25_weights)
    bm25.token_counts, bm25.sparse_csr_build, bm25.bm25_weights = (timed(k_, f) for k_, f in zip(spent, real))
    try:
        def loader(cs):
            return TokenBudgetCollectionLoader(tokenized=cs, max_length=192, max_tokens=a.token_budget, max_seqs=4096, window=32768,
                                               pad_token_id=0, padding_side="left")
        bm25.Bm25Indexer(None, dev, a.vocab, SKIP).index(loader(chunks[:1]))                   # warm-up
        for k_ in spent:
            spent[k_] = 0.0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        index_d = bm25.Bm25Indexer(None, dev, a.vocab, SKIP).index(loader(chunks))
        torch.cuda.synchronize()
        t_index = time.perf_counter() - t0
        t0 = time.perf_counter()
        ret = bm25.Bm25Retrieval({"out_dir": "unused"}, a.vocab, dev, index_d=index_d)
        torch.cuda.synchronize()
        t_open = time.perf_counter() - t0
    finally:
        bm25.token_counts, bm25.sparse_csr_build, bm25.bm25_weights = real
    out = {"passages": a.passages, "token_budget": a.token_budget, "postings": int(ret.hip_index.vals.numel()), "index_seconds": round(t_index, 3),
           "passages_per_second": round(a.passages / t_index, 1), "ms_inside": {k_: round(v, 2) for k_, v in spent.items()},
           "share_of_index_time": {k_: round(spent[k_] * 1e-3 / t_index, 4) for k_ in ("sr_token_counts", "sr_sparse_csr_build")},
           "open_seconds": round(t_open, 3), "note": "the rest of the index time is the loader: collating padded batches on the host and copying them"}
    ret.hip_index.close()
    return out


def search_leg(a, weighted, dev):
    from scaling_retriever_amd.scoring import SparseIndexHIP, token_counts
    indptr, doc_ids, w, N = weighted
    idx = SparseIndexHIP(indptr, doc_ids, w, N, device=dev)
    ids, _ = token_rows(a.nq, 8, a.vocab, dev, 11)
    g = torch.Generator(device=dev).manual_seed(12)
    real = torch.randint(6, 9, (a.nq,), device=dev, generator=g)
    mask = (torch.arange(8, device=dev)[None, :] >= (8 - real)[:, None]).to(torch.int64)
    q = token_counts(ids, mask, SKIP, a.vocab)[:3]
    before = idx.cert_stats()
    ms = alternating({"search": lambda: idx.search(*q, a.k)}, a.reps)["search"]              # one warm-up round, then the median of --reps
    after = idx.cert_stats()
    queries, redone = after["queries"] - before["queries"], after["redone_exact"] - before["redone_exact"]
    out = {"n_docs": N, "postings": int(w.numel()), "nq": a.nq, "k": a.k, "query_terms_mean": round(q[1].numel() / a.nq, 2), "search": summary(ms),
           "queries_per_second": round(a.nq / (statistics.median(ms) * 1e-3), 1), "certified_scorer_present": after["present"] == 1,
           "certified_queries": queries, "handed_back_to_exact": redone, "handed_back_share": round(redone / queries, 4) if queries else None,
           "batches_without_memory": after["batches_without_memory"] - before["batches_without_memory"]}
    idx.close()
    return out


def parent_leg(a, N, dev):
    from scaling_retriever_amd import _lib
    from scaling_retriever_amd.scoring import SparseIndexHIP
    parent = ctypes.CDLL(os.path.abspath(a.parent_lib))
    for name, (res, args) in _lib.SIGNATURES.items():              # the parent lacks the entries this change adds
        fn = getattr(parent, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    arrays = build_index(a.vocab, N, 128, dev, 3)[:3]

    def parent_index():
        keep, _lib._lib = _lib._lib, parent
        try:
            return SparseIndexHIP(*arrays, N, device=dev)
        finally:
            _lib._lib = keep
    idx = {"this": SparseIndexHIP(*arrays, N, device=dev), "parent": parent_index(), "parent_again": parent_index()}
    q = build_queries(a.vocab, a.nq, 32, dev, 4)
    got = {name: ix.search(*q, a.k) for name, ix in idx.items()}
    assert same_bytes(got["this"], got["parent"]), "sr_sparse_search: this build and the parent's differ"
    ms = alternating({name: (lambda ix=ix: ix.search(*q, a.k)) for name, ix in idx.items()}, a.parent_reps)
    t = {name: summary(v) for name, v in ms.items()}
    p = t["parent"]["median_ms"]
    spread = abs(t["parent_again"]["median_ms"] - p)
    out = {"shape": {"n_docs": N, "L0_d": 128, "L0_q": 32, "nq": a.nq, "k": a.k}, "outputs_equal_bytes": True, **t,
           "this_over_parent": round(t["this"]["median_ms"] / p, 4), "parent_again_over_parent": round(t["parent_again"]["median_ms"] / p, 4),
           "parent_spread_ms": round(spread, 3),
           "within_parent_spread_plus_one_percent": bool(t["this"]["median_ms"] <= max(p, t["parent_again"]["median_ms"]) + spread + 0.01 * p)}
    for ix in idx.values():
        ix.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the 8 841 823 documents (weights, search, parent)")
    ap.add_argument("--n-docs", type=int, default=8_841_823)
    ap.add_argument("--vocab", type=int, default=128256)
    ap.add_argument("--l0-d", type=int, default=50, help="distinct tokens per passage of the weights / search index")
    ap.add_argument("--shapes", type=str, default=SHAPES, help="B:L of the token-count legs, comma separated")
    ap.add_argument("--sweep-rows", type=int, default=16384)
    ap.add_argument("--passages", type=int, default=1_048_576)
    ap.add_argument("--token-budget", type=int, default=262144)
    ap.add_argument("--nq", type=int, default=6980)
    ap.add_argument("--k", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parent-reps", type=int, default=7)
    ap.add_argument("--legs", type=str, default=None, help="counts,weights,pipeline,search,parent (search needs weights)")
    ap.add_argument("--parent-lib", type=str, default=None, help="the parent commit's libsr_hip.so: enables the `parent` leg")
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "bm25.json"))
    a = ap.parse_args()
    legs = a.legs.split(",") if a.legs else ["counts", "weights", "pipeline", "search"] + (["parent"] if a.parent_lib else [])
    if "parent" in legs and not a.parent_lib:
        ap.error("the parent leg needs --parent-lib")
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    N = max(8 * (a.k + 1024), int(a.n_docs * a.scale))
    t0 = time.time()
    res = {"what": "BM25 on the device: sr_token_counts, sr_bm25_weights, Bm25Indexer, search of the weighted index (tools/bench_bm25.py)",
           "device": torch.cuda.get_device_name(0), "n_gpus": 1, "data": "synthetic: log-uniform (Zipf) token ids over the vocabulary; the Zipf index of tools/synth.py",
           "timing": f"HIP events around each call; variants alternate inside a round; median of {a.reps} rounds after 1 warm-up round",
           "hbm_GBps_reference": HBM_GBPS}
    if "counts" in legs:
        res["token_counts"] = counts_leg(a, dev)
    weighted = None
    if "weights" in legs:
        res["bm25_weights"], weighted = weights_leg(a, N, dev)
    if "search" in legs and weighted is not None:
        res["search"] = search_leg(a, weighted, dev)
        print("[search]", json.dumps(res["search"]), file=sys.stderr, flush=True)
    del weighted
    torch.cuda.empty_cache()
    if "pipeline" in legs:
        res["pipeline"] = pipeline_leg(a, dev)
        print("[pipeline]", json.dumps(res["pipeline"]), file=sys.stderr, flush=True)
    if "parent" in legs:
        res["sparse_search_against_parent"] = parent_leg(a, N, dev)
        print("[parent]", json.dumps(res["sparse_search_against_parent"]), file=sys.stderr, flush=True)
    every = res.get("token_counts", {}).get("shapes", []) + res.get("bm25_weights", [])
    res["outputs_equal_bytes"] = all(leg["outputs_equal_bytes"] for leg in every)
    res["shapes_that_lose_to_the_composition"] = [{k_: leg[k_] for k_ in ("B", "L", "postings") if k_ in leg} for leg in every
                                                  if not leg["kernel_not_slower_beyond_the_spread"]]
    res["seconds"] = round(time.time() - t0, 1)
    text = json.dumps(res, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
