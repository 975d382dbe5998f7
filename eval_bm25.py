#!/usr/bin/env python3
"""BM25 driver on MI355X: a lexical index and search from the tokenizer's ids, no model (scaling_retriever_amd/bm25.py).
Tasks, paths and artefacts as eval_sparse.py, whose dataset, tokenizer and perf helpers it uses:

  python eval_bm25.py --task_name indexing  --tokenizer_path <dir> --corpus_path <tsv> --index_dir <dir>/bm25_index
  python eval_bm25.py --task_name retrieval --tokenizer_path <dir> --query_path <tsv> --index_dir <dir>/bm25_index \
                      --out_dir <dir>/bm25 --top_k 1000 [--bm25_k1 0.9 --bm25_b 0.4] [--prf_depth 10]
  python eval_fuse.py --run_paths <dir>/bm25/run.json,<dir>/dense/run.json ...          (the hybrid with the dense head)

The index stores term frequencies: --bm25_k1 / --bm25_b / --bm25_lucene of the retrieval task re-weight it when it is opened (default:
what the indexing task recorded), so a parameter sweep needs no re-indexing."""
import argparse
import ast
import os

import torch
from torch.utils.data import DataLoader

import eval_sparse


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    for name in ["tokenizer_path", "corpus_path", "index_dir", "out_dir", "query_path", "eval_qrel_path", "eval_metric", "beir_dataset",
                 "beir_dataset_dir"]:
        ap.add_argument("--" + name, type=str, default=None)
    ap.add_argument("--task_name", type=str, default="", choices=["indexing", "retrieval"])
    ap.add_argument("--data_source", type=str, default=None)
    ap.add_argument("--is_beir", action="store_true")
    ap.add_argument("--eval_batch_size", type=int, default=128)
    ap.add_argument("--doc_max_length", type=int, default=192)
    ap.add_argument("--query_max_length", type=int, default=64)
    ap.add_argument("--top_k", type=int, default=100)
    ap.add_argument("--local_rank", type=int, default=0)
    ap.add_argument("--token_budget", type=int, default=16384,
                    help="indexing task: real tokens per batch (length-bucketed, multi-worker tokenisation); 0 = fixed batches of "
                         "--eval_batch_size rows")
    ap.add_argument("--tokenize_workers", type=int, default=4)
    ap.add_argument("--dim_voc", type=int, default=0, help="size of the term space (0: the tokenizer's vocabulary, added tokens included)")
    ap.add_argument("--bm25_k1", type=float, default=None, help="term-frequency saturation (indexing: recorded, default 0.9; retrieval: "
                                                                 "default what the index records)")
    ap.add_argument("--bm25_b", type=float, default=None, help="length normalisation in [0, 1] (default 0.4, as --bm25_k1)")
    ap.add_argument("--bm25_lucene", action="store_true", help="Lucene's rank-equivalent form: the factor k1 + 1 is left out of the scores")
    ap.add_argument("--bm25_binary_queries", action="store_true", help="retrieval task: a repeated query token counts once")
    ap.add_argument("--allowed_ids_file", type=str, default=None,
                    help="retrieval task: rank only the documents whose ids this file lists, one id per line (any order, repeats allowed)")
    ap.add_argument("--collapse_file", type=str, default=None,
                    help="retrieval task: a TSV of passage_id<TAB>group_id - rank the top_k best GROUPS, each scored by its best passage")
    ap.add_argument("--collapse_hits", type=int, default=0, help="with --collapse_file: also the up to M best passages inside every group")
    ap.add_argument("--prf_depth", type=int, default=0,
                    help="retrieval task: also a second round with Rocchio feedback from the M best documents, to prf/run.json (0: off)")
    ap.add_argument("--prf_alpha", type=float, default=1.0)
    ap.add_argument("--prf_beta", type=float, default=0.75)
    ap.add_argument("--prf_gamma", type=float, default=0.0)
    ap.add_argument("--prf_neg_depth", type=int, default=0)
    ap.add_argument("--prf_max_terms", type=int, default=128)
    ap.add_argument("--device_eval", action="store_true",
                    help="with --eval_qrel_path: the retrieval task writes a perf.json beside run.json (and prf/run.json) from the result arrays")
    args = ap.parse_args(argv)
    if not args.tokenizer_path:
        ap.error("--tokenizer_path is required (the terms are the tokenizer's ids)")
    for name in ("bm25_k1", "bm25_b"):
        v = getattr(args, name)
        if v is not None and (v < 0 or (name == "bm25_b" and v > 1)):
            ap.error("--bm25_k1 must be >= 0 and --bm25_b in [0, 1]")
    if not args.prf_depth and (args.prf_neg_depth or args.prf_gamma):
        ap.error("--prf_neg_depth / --prf_gamma need --prf_depth (they shape the feedback of the second round)")
    if args.prf_depth:
        if args.collapse_file:
            ap.error("--prf_depth cannot be combined with --collapse_file (feedback rebuilds passage queries, a collapsed run ranks groups)")
        if not 1 <= args.prf_depth <= 64 or not 0 <= args.prf_neg_depth <= 64:
            ap.error(f"--prf_depth must be in [1, 64] and --prf_neg_depth in [0, 64], got {args.prf_depth} and {args.prf_neg_depth}")
        if min(args.prf_alpha, args.prf_beta, args.prf_gamma) < 0 or args.prf_max_terms < 0:
            ap.error("--prf_alpha, --prf_beta, --prf_gamma and --prf_max_terms must be >= 0")
    if args.collapse_hits and not args.collapse_file:
        ap.error("--collapse_hits needs --collapse_file (hits are the passages inside the groups of a collapsed search)")
    if not 0 <= args.collapse_hits <= 64:
        ap.error(f"--collapse_hits must be in [0, 64], got {args.collapse_hits}")
    if args.eval_metric:
        args.eval_metric = ast.literal_eval(args.eval_metric)
    return args


def term_space(tokenizer, args):
    """(dim_voc, skip_ids): the size of the term space and the special ids that are no terms (BOS, EOS, pad)."""
    dim_voc = args.dim_voc or max(int(getattr(tokenizer, "vocab_size", 0) or 0), len(tokenizer) if hasattr(tokenizer, "__len__") else 0)
    skip = {getattr(tokenizer, name, None) for name in ("bos_token_id", "eos_token_id", "pad_token_id")}
    return dim_voc, sorted(int(x) for x in skip if x is not None)


def bm25_index(args):
    from scaling_retriever_amd.bm25 import Bm25Indexer
    from scaling_retriever_amd.dataset.data_collator import LlamaSparseCollectionCollator
    tokenizer = eval_sparse._tokenizer(args.tokenizer_path)
    collection = eval_sparse._collection_dataset(args)
    dim_voc, skip_ids = term_space(tokenizer, args)
    if args.token_budget > 0:
        from scaling_retriever_amd.dataset.pipeline import TokenBudgetCollectionLoader
        loader = TokenBudgetCollectionLoader(collection, tokenizer, max_length=args.doc_max_length, max_tokens=args.token_budget, max_seqs=1024,
                                             num_workers=args.tokenize_workers)
    else:
        loader = DataLoader(collection, batch_size=args.eval_batch_size, shuffle=False, num_workers=0,
                            collate_fn=LlamaSparseCollectionCollator(tokenizer=tokenizer, max_length=args.doc_max_length))
    index_dir = args.index_dir[:-1] if args.index_dir.endswith("/") else args.index_dir
    indexer = Bm25Indexer(index_dir, device=args.local_rank, dim_voc=dim_voc, skip_ids=skip_ids, k1=0.9 if args.bm25_k1 is None else args.bm25_k1,
                          b=0.4 if args.bm25_b is None else args.bm25_b, lucene=args.bm25_lucene)
    indexer.index(loader)
    return indexer


def bm25_retrieval(args):
    from scaling_retriever_amd.bm25 import Bm25Retrieval
    from scaling_retriever_amd.dataset.data_collator import LlamaSparseCollectionCollator
    tokenizer = eval_sparse._tokenizer(args.tokenizer_path)
    queries = eval_sparse._query_dataset(args)
    dim_voc, skip_ids = term_space(tokenizer, args)
    os.makedirs(args.out_dir, exist_ok=True)
    q_loader = DataLoader(queries, batch_size=args.eval_batch_size, shuffle=False, num_workers=0,
                          collate_fn=LlamaSparseCollectionCollator(tokenizer=tokenizer, max_length=args.query_max_length))
    retriever = Bm25Retrieval({"index_dir": args.index_dir, "out_dir": args.out_dir}, dim_voc=dim_voc, device=args.local_rank, skip_ids=skip_ids,
                              k1=args.bm25_k1, b=args.bm25_b, lucene=True if args.bm25_lucene else None,
                              query_tf=not args.bm25_binary_queries, compute_stats=True)
    allowed_ids = None
    if args.allowed_ids_file:
        from scaling_retriever_amd.scoring import read_allowed_ids_file
        allowed_ids = read_allowed_ids_file(args.allowed_ids_file)
    collapse = None
    if args.collapse_file:
        from scaling_retriever_amd.collapse import read_collapse_file
        group_of = read_collapse_file(args.collapse_file)
        collapse = lambda d: group_of[str(d)]      # noqa: E731  (collection ids may be ints, the file's are text)
    res = retriever.retrieve(q_loader, topk=args.top_k, threshold=0.0, allowed_ids=allowed_ids, collapse=collapse, hits=args.collapse_hits or None)
    perf = eval_sparse.device_perf_writer(args)
    perf("", res)
    if args.prf_depth:
        perf("prf", retriever.retrieve_prf(q_loader, topk=args.top_k, threshold=0.0, n_pos=args.prf_depth, n_neg=args.prf_neg_depth,
                                           alpha=args.prf_alpha, beta=args.prf_beta, gamma=args.prf_gamma, max_terms=args.prf_max_terms,
                                           fb_depth=args.prf_depth + args.prf_neg_depth, allowed_ids=allowed_ids))
    return res


def main(argv=None):
    args = parse_args(argv)
    torch.cuda.set_device(args.local_rank)
    if args.task_name == "indexing":
        bm25_index(args)
    elif args.task_name == "retrieval":
        return bm25_retrieval(args)
    else:
        raise NotImplementedError(args.task_name)


if __name__ == "__main__":
    main()
