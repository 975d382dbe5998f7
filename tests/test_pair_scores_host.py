"""Host side of pair scoring (no GPU): candidate lists of a run.json / jsonl file -> (qids, cand_indptr, positions), the
driver's argument validation, the fused score and the ranking - against numpy on hand-made examples."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from scaling_retriever_amd.rerank import (InverseIdMap, candidates_from_jsonl, candidates_from_run, fused_scores, rank_candidates, ranked_run, read_candidates)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_run_and_jsonl_become_csr_over_index_positions(tmp_path):
    inv = InverseIdMap(["d7", "d3", 11, "d9"])                   # position -> id, ids compared as str (run.json keys are strings)
    run = {"q2": {"d9": 1.0, "d7": 0.5}, "q1": {"11": 2.0}}
    qids, lists = candidates_from_run(run)
    indptr, pos = inv.positions(lists)
    assert qids == ["q2", "q1"] and indptr.tolist() == [0, 2, 3] and pos.tolist() == [3, 0, 2]
    lines = ['{"qid": "b", "docids": ["d3", "d3", "d7"]}', '{"qid": "a", "docids": []}', "", '{"qid": "b", "docids": [11]}',
             '{"qid": 5, "docids": ["d9"]}']
    qids, lists = candidates_from_jsonl(lines)
    indptr, pos = inv.positions(lists)
    assert qids == ["b", "a", "5"]                               # order of first appearance
    assert indptr.tolist() == [0, 4, 4, 5] and pos.tolist() == [1, 1, 0, 2, 3]      # duplicates kept, the empty list kept
    assert indptr.dtype == np.int64 and pos.dtype == np.int64
    with pytest.raises(KeyError, match="d404"):
        inv.positions([["d7"], ["d3", "d404"]])
    inv2 = InverseIdMap({4: "x", 0: "y"})                        # doc_ids.pkl: position -> id, documents without a posting absent
    assert inv2.positions([["y", "x"]])[1].tolist() == [0, 4] and inv2.get("nope") == -1
    (tmp_path / "run.json").write_text(json.dumps(run))
    (tmp_path / "c.jsonl").write_text("\n".join(lines))
    assert read_candidates(run_path=str(tmp_path / "run.json")) == candidates_from_run(run)
    assert read_candidates(jsonl_path=str(tmp_path / "c.jsonl")) == candidates_from_jsonl(lines)
    for kw in ({}, {"run_path": "a", "jsonl_path": "b"}):
        with pytest.raises(ValueError):
            read_candidates(**kw)


def test_eval_rerank_argument_validation(capsys):
    sys.path.insert(0, ROOT)
    import eval_rerank
    base = ["--rerank_type", "dense_encoder", "--model_name_or_path", "m", "--query_path", "q.tsv", "--output_dir", "o", "--index_dir", "i"]
    a = eval_rerank.parse_args(base + ["--run_path", "r.json"])
    assert a.run_path == "r.json" and a.jsonl_path is None and a.dense_index_dir == "i" and a.weights == (1.0, 1.0)
    a = eval_rerank.parse_args(base + ["--jsonl_path", "c.jsonl", "--weights", "0.25,2"])
    assert a.weights == (0.25, 2.0)
    for bad in (base + ["--run_path", "r.json", "--jsonl_path", "c.jsonl"], base,            # both / neither (eval_reranker.py:81)
                base[:-2] + ["--run_path", "r.json"],                                        # no index
                ["--rerank_type", "cross_encoder"] + base[2:] + ["--run_path", "r.json"],
                base + ["--run_path", "r.json", "--weights", "1"]):
        with pytest.raises(SystemExit):
            eval_rerank.parse_args(bad)
    capsys.readouterr()
    with pytest.raises(SystemExit):
        eval_rerank.parse_args(["--help"])
    assert "reranking is out of scope" in " ".join(capsys.readouterr().out.split())      # doc-sharded reranking: said in --help


def test_fused_score_and_ranking_against_numpy():
    rng = np.random.default_rng(0)
    dense = rng.standard_normal(40).astype(np.float32) * 37
    sparse = (rng.uniform(0, 30, 40)).astype(np.float32)
    for w in ((1.0, 1.0), (0.3, 1.7), (0.1, 0.0)):
        want = (np.float32(w[0]) * dense).astype(np.float32) + (np.float32(w[1]) * sparse).astype(np.float32)
        got = fused_scores(torch.from_numpy(dense), torch.from_numpy(sparse), w).numpy()
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.astype(np.float32).view(np.uint32))
        wide = np.float64(np.float32(w[0])) * dense + np.float64(np.float32(w[1])) * sparse       # not the definition: one rounding
        assert w == (1.0, 1.0) or w[1] == 0.0 or not np.array_equal(wide.astype(np.float32), want)
    # ranking: (score desc, position asc) inside each ragged row, then the cut
    scores = torch.tensor([1.0, 3.0, 3.0, 2.0,   5.0,   0.5, 0.5, 0.5], dtype=torch.float32)
    tie = torch.tensor([9, 8, 2, 4,   1,   7, 3, 5])
    indptr = torch.tensor([0, 4, 4, 5, 8])
    order, counts = rank_candidates(scores, tie, indptr)
    assert order.tolist() == [2, 1, 3, 0, 4, 6, 7, 5] and counts.tolist() == [4, 0, 1, 3]
    order, counts = rank_candidates(scores, tie, indptr, topk=2)
    assert order.tolist() == [2, 1, 4, 6, 7] and counts.tolist() == [2, 0, 1, 2]
    s, t, ip = scores.numpy(), tie.numpy(), indptr.numpy()
    for q in range(4):
        o = np.lexsort((t[ip[q]:ip[q + 1]], -s[ip[q]:ip[q + 1]].astype(np.float64))) + ip[q]
        assert order[sum(counts.tolist()[:q]):sum(counts.tolist()[:q + 1])].tolist() == o[:2].tolist()
    docs = [f"d{i}" for i in range(10)]
    res = ranked_run(["a", "b", "c", "d"], scores, tie, tie, indptr, docs)
    assert res == {"a": {"d2": 3.0, "d8": 3.0, "d4": 2.0, "d9": 1.0}, "c": {"d1": 5.0}, "d": {"d3": 0.5, "d5": 0.5, "d7": 0.5}}
    assert list(res["a"]) == ["d2", "d8", "d4", "d9"] and "b" not in res
    # a list that names a document twice (both entries carry the same score): one key in the run
    rep = ranked_run(["a"], torch.tensor([2.0, 7.0, 2.0, 7.0]), torch.tensor([4, 1, 4, 1]), torch.tensor([4, 1, 4, 1]), torch.tensor([0, 4]), docs)
    assert rep.counts.tolist() == [2] and rep.positions.tolist() == [[1, 4]] and rep == {"a": {"d1": 7.0, "d4": 2.0}}
