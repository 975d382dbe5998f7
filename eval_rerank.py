#!/usr/bin/env python3
"""Rerank driver on MI355X: scores the (query, document) pairs of a run with the vectors the indexes already hold.

Stands in for the reference's eval_reranker.py (--rerank_type dense_encoder | splade | hybrid_retriever; input a run.json or
`{"qid": ..., "docids": [...]}` lines, :91-105; output a run.json), which encodes both sides of every pair again
(rerank_forward, scaling_retriever/modeling/llm_encoder.py:593-615).  Here each distinct query is encoded once and the documents
come from the dense shard files / the inverted index written by eval_dense.py / eval_sparse.py / HybridIndexer:

  python eval_rerank.py --rerank_type dense_encoder --model_name_or_path <lora dir> --query_path <tsv> --run_path <run.json> \
         --index_dir <doc_embed_dir with plan.json> --output_dir <dir>
  python eval_rerank.py --rerank_type splade --model_name_or_path <lora dir> --query_path <tsv> --jsonl_path <jsonl> \
         --index_dir <inverted index dir> --output_dir <dir>
  python eval_rerank.py --rerank_type hybrid --model_name_or_path <dir> --query_path <tsv> --run_path <run.json> \
         --sparse_index_dir <dir> --dense_index_dir <dir> --output_dir <dir> --weights 1.0,1.0

Single process: the candidates' documents must all be in the indexes this process loads (doc-sharded reranking is not built).
A document id the index does not hold is an error (KeyError naming it), as is a qid without a query text; in hybrid mode a document
of the dense index that has no posting scores 0.0 on the sparse head.
"""
import argparse
import os

import numpy as np
import torch
from torch.utils.data import DataLoader, Subset

RERANK_TYPES = ("dense_encoder", "splade", "hybrid")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Score the candidates of a run from the resident indexes (single process; doc-sharded "
                                             "reranking is out of scope).")
    ap.add_argument("--rerank_type", type=str, required=True, choices=RERANK_TYPES)
    for name in ["model_name_or_path", "query_path", "run_path", "jsonl_path", "index_dir", "dense_index_dir", "sparse_index_dir",
                 "output_dir", "access_token"]:
        ap.add_argument("--" + name, type=str, default=None)
    ap.add_argument("--weights", type=str, default="1.0,1.0", help="hybrid: w_dense,w_sparse of fused = f32(w_d * dense) + f32(w_s * sparse)")
    ap.add_argument("--eval_batch_size", type=int, default=128)
    ap.add_argument("--query_max_length", type=int, default=64)
    ap.add_argument("--local_rank", type=int, default=0)
    args = ap.parse_args(argv)
    if (args.run_path is None) == (args.jsonl_path is None):                  # eval_reranker.py:81
        ap.error("give exactly one of --run_path and --jsonl_path")
    for name in ("model_name_or_path", "query_path", "output_dir"):
        if getattr(args, name) is None:
            ap.error(f"--{name} is required")
    try:
        args.weights = tuple(float(x) for x in args.weights.split(","))
        assert len(args.weights) == 2
    except (ValueError, AssertionError):
        ap.error("--weights takes two numbers: w_dense,w_sparse")
    args.dense_index_dir = args.dense_index_dir or args.index_dir
    args.sparse_index_dir = args.sparse_index_dir or args.index_dir
    need = {"dense_encoder": ["dense_index_dir"], "splade": ["sparse_index_dir"], "hybrid": ["dense_index_dir", "sparse_index_dir"]}
    for name in need[args.rerank_type]:
        if getattr(args, name) is None:
            ap.error(f"--rerank_type {args.rerank_type} needs --index_dir or --{name}")
    return args


def _query_loader(args, qids, collator):
    """The run's queries, each once, in the run's order."""
    from scaling_retriever_amd.dataset.dataset import MSMARCOQueryDataset
    queries = MSMARCOQueryDataset(args.query_path)
    row = {str(queries[i][0]): i for i in range(len(queries))}
    missing = [q for q in qids if q not in row]
    if missing:
        raise KeyError(f"query id {missing[0]!r} of the run is not in {args.query_path}")
    return DataLoader(Subset(queries, [row[q] for q in qids]), batch_size=args.eval_batch_size, shuffle=False, num_workers=0,
                      collate_fn=collator)


def _dense_index(dense_index_dir, hidden_size):
    from scaling_retriever_amd.indexer import DenseFlatIndexer
    from scaling_retriever_amd.utils.utils import obtain_doc_vec_dir_files
    index = DenseFlatIndexer()
    index.init_index(hidden_size)
    for vec_file, id_file in zip(*obtain_doc_vec_dir_files(dense_index_dir)):
        index.index_data(np.load(vec_file, mmap_mode="r"), np.load(id_file).tolist())
    return index


def rerank(args):
    from eval_dense import generate_query_vecs
    from scaling_retriever_amd.dataset.data_collator import LlamaDenseCollectionCollator, LlamaSparseCollectionCollator
    from scaling_retriever_amd.modeling.llm_encoder import retriever_class
    from scaling_retriever_amd.rerank import read_candidates
    qids, lists = read_candidates(args.run_path, args.jsonl_path)
    torch.cuda.set_device(args.local_rank)
    device = torch.device("cuda", args.local_rank)
    os.makedirs(args.output_dir, exist_ok=True)
    # queries are tokenised and encoded as the matching retrieval task does it, so that a pair's score is that task's score
    if args.rerank_type == "dense_encoder":
        from eval_dense import _tokenizer
        tokenizer = _tokenizer(args.model_name_or_path, args.access_token)
    else:
        from eval_sparse import _tokenizer
        tokenizer = _tokenizer(args.model_name_or_path)
        if args.rerank_type == "hybrid":
            tokenizer.padding_side = "left"      # the dense head pools the LAST tokens (eval_dense.py:185,206); the max-pool head does not care
    head = {"dense_encoder": "dense", "splade": "sparse", "hybrid": "hybrid"}[args.rerank_type]
    model = retriever_class(args.model_name_or_path, head).load_from_lora(args.model_name_or_path, access_token=args.access_token)
    model.to(device)
    model.eval()
    if args.rerank_type == "dense_encoder":
        loader = _query_loader(args, qids, LlamaDenseCollectionCollator(tokenizer=tokenizer, max_length=args.query_max_length))
        q_reps, got = generate_query_vecs(model, loader, device)           # the retrieval task's regime (eval_dense.py:94-106)
        assert [str(x) for x in got] == qids
        res = _dense_index(args.dense_index_dir, model.hidden_size).score_candidates(q_reps, lists, qids)
    else:
        from scaling_retriever_amd.indexer import HybridRetriever, SparseRetrieval
        loader = _query_loader(args, qids, LlamaSparseCollectionCollator(tokenizer=tokenizer, max_length=args.query_max_length))
        if args.rerank_type == "splade":
            retriever = SparseRetrieval(config={"index_dir": args.sparse_index_dir, "out_dir": args.output_dir}, model=model,
                                        dim_voc=model.vocab_size, device=args.local_rank)
            sparse_q, got = retriever._generate_query_vecs(loader)
            res = retriever.score_candidates(sparse_q, qids, lists)
        else:
            retriever = HybridRetriever(model, args.sparse_index_dir, args.dense_index_dir, args.output_dir, dim_voc=model.vocab_size,
                                        device=args.local_rank)
            sparse_q, dense_q, got = retriever._generate_query_vecs(loader)
            res = retriever.score_candidates(sparse_q, qids, lists, dense_query_vecs=dense_q, weights=args.weights)
        assert [str(x) for x in got] == qids
    res.dump(os.path.join(args.output_dir, "run.json"))
    return res


def main(argv=None):
    return rerank(parse_args(argv))


if __name__ == "__main__":
    main()
