#!/usr/bin/env python3
"""Sparse eval driver on MI355X: same tasks, flags and artefacts as /root/reference/eval_sparse.py
(SparseArguments :34-72; tasks indexing :75-106, retrieval :109-151, evaluate_msmarco), running the
HIP LlamaBiSparse encoder and the HIP inverted-index scorer.

  torchrun --nproc_per_node=2 eval_sparse.py --task_name indexing --model_name_or_path <lora dir> \
           --corpus_path <tsv> --index_dir <dir>/index --eval_batch_size 64 --doc_max_length 192
  python   -m scaling_retriever_amd.utils.inverted_index --model_name_or_path <base dir> --index_dir <dir>   (merge)
  python   eval_sparse.py --task_name retrieval --model_name_or_path <lora dir> --query_path <tsv> \
           --index_dir <dir>/index --out_dir <dir> --top_k 1000
"""
import argparse
import ast
import json
import os

import torch
import torch.distributed as dist
from torch.utils.data import DataLoader
from torch.utils.data.distributed import DistributedSampler

CORPUS_DATASOURCE = {"./data/msmarco-full/full_collection/raw.tsv": "msmarco"}


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    for name in ["model_name_or_path", "corpus_path", "index_dir", "out_dir", "query_path", "eval_run_path",
                 "eval_qrel_path", "eval_metric", "beir_dataset", "beir_dataset_dir", "access_token"]:
        ap.add_argument("--" + name, type=str, default=None)
    ap.add_argument("--task_name", type=str, default="")
    ap.add_argument("--data_source", type=str, default=None)
    ap.add_argument("--is_beir", action="store_true")
    ap.add_argument("--eval_batch_size", type=int, default=128)   # SparseArguments.eval_batch_size (eval_sparse.py:50)
    ap.add_argument("--doc_max_length", type=int, default=192)
    ap.add_argument("--query_max_length", type=int, default=64)
    ap.add_argument("--top_k", type=int, default=100)             # SparseArguments.top_k (eval_sparse.py:56); scripts pass 1000
    ap.add_argument("--local_rank", type=int, default=-1)
    ap.add_argument("--world_size", type=int, default=1)
    ap.add_argument("--token_budget", type=int, default=16384,
                    help="real tokens per encode batch of the indexing task (length-bucketed, multi-worker tokenisation); "
                         "0 = the reference's loader (eval_sparse.py:94-97)")
    ap.add_argument("--tokenize_workers", type=int, default=4)
    # term budgets (no counterpart in the reference's SparseArguments): keep only the largest terms of a row, 0 = all of them
    ap.add_argument("--allowed_ids_file", type=str, default=None,
                    help="retrieval task: rank only the documents whose ids this file lists, one id per line (any order, repeats allowed)")
    ap.add_argument("--collapse_file", type=str, default=None,
                    help="retrieval task: a TSV of passage_id<TAB>group_id - rank the top_k best GROUPS, each scored by its best passage "
                         "(MaxP); run.json is then keyed by group id")
    ap.add_argument("--collapse_hits", type=int, default=0,
                    help="with --collapse_file: also the up to M best passages inside every returned group, written as a passage-level run "
                         "to hits/run.json (0: off; at most 64)")
    ap.add_argument("--doc_max_terms", type=int, default=0, help="indexing task: terms indexed per document (index size)")
    ap.add_argument("--query_max_terms", type=int, default=0, help="retrieval task: terms searched per query (latency)")
    ap.add_argument("--prf_depth", type=int, default=0,
                    help="retrieval task: also a second round with pseudo-relevance feedback (Rocchio) - every query rebuilt from its M best "
                         "documents and searched again - written to prf/run.json beside the untouched run.json (0: off; at most 64)")
    ap.add_argument("--prf_alpha", type=float, default=1.0, help="with --prf_depth: weight of the original query")
    ap.add_argument("--prf_beta", type=float, default=0.75, help="with --prf_depth: weight of the mean of the M feedback documents")
    ap.add_argument("--prf_gamma", type=float, default=0.0, help="with --prf_neg_depth: weight of the mean of the negative documents")
    ap.add_argument("--prf_neg_depth", type=int, default=0,
                    help="with --prf_depth: the G documents ranked behind the M feedback documents are the negative set (0: none; at most 64)")
    ap.add_argument("--prf_max_terms", type=int, default=128, help="with --prf_depth: terms kept per rebuilt query (0: all)")
    ap.add_argument("--mmr_lambda", type=float, default=None,
                    help="retrieval task: also a diversified run - exact greedy MMR with this lambda in [0, 1] over the top "
                         "--mmr_fetch_k of every query, top_k picks - written to mmr/run.json beside the untouched run.json")
    ap.add_argument("--mmr_fetch_k", type=int, default=0,
                    help="with --mmr_lambda: candidates per query, top_k <= mmr_fetch_k <= the library's sr_mmr_max_candidates()")
    ap.add_argument("--mmr_sim", type=str, default="cosine", choices=["ip", "cosine"],
                    help="with --mmr_lambda: the document-document similarity, the inner product of two documents' term rows or their cosine")
    ap.add_argument("--device_eval", action="store_true",
                    help="evaluate on the device (scaling_retriever_amd/evaluation.py): the evaluate_msmarco / evaluate_beir tasks write the "
                         "same perf.json from arrays; the retrieval task with --eval_qrel_path writes a perf.json beside run.json (and "
                         "beside prf/run.json and mmr/run.json) from the result arrays")
    args = ap.parse_args(argv)
    if args.mmr_fetch_k and args.mmr_lambda is None:
        ap.error("--mmr_fetch_k needs --mmr_lambda (it is the candidate depth of the MMR selection)")
    if args.mmr_lambda is not None:
        if args.collapse_file:
            ap.error("--mmr_lambda cannot be combined with --collapse_file (MMR diversifies passages, a collapsed run ranks groups)")
        if args.prf_depth:
            ap.error("--mmr_lambda cannot be combined with --prf_depth (run the two second rounds one after the other)")
        if not 0.0 <= args.mmr_lambda <= 1.0:
            ap.error(f"--mmr_lambda must be in [0, 1], got {args.mmr_lambda}")
        if args.mmr_fetch_k < args.top_k:
            ap.error(f"--mmr_lambda needs --mmr_fetch_k >= top_k = {args.top_k}, got {args.mmr_fetch_k}")
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


def ddp_setup(args):
    if "LOCAL_RANK" in os.environ and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        args.local_rank = int(os.environ["LOCAL_RANK"])
        if os.environ.get("SR_SHARE_GPU") == "1":
            # dry run of the multi-rank path on a ONE-GPU box (tests): every rank on cuda:0, gloo instead of RCCL, which refuses
            # two ranks on one device; real runs leave it unset
            args.local_rank = 0
            torch.cuda.set_device(0)
            dist.init_process_group(backend="gloo")
        else:
            torch.cuda.set_device(args.local_rank)
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", args.local_rank))
        args.world_size = dist.get_world_size()
    else:
        args.local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(args.local_rank)
        args.world_size = 1


def _tokenizer(path):
    from transformers import AutoTokenizer
    tok = AutoTokenizer.from_pretrained(path)
    if tok.pad_token is None:
        tok.pad_token = tok.eos_token
    return tok     # eval_sparse.py never sets padding_side: the max-pool head does not depend on it


def _query_dataset(args):
    from scaling_retriever_amd.dataset.dataset import BeirDataset, MSMARCOQueryDataset
    if args.is_beir and args.beir_dataset is not None:             # eval_sparse.py:116-121
        from scaling_retriever_amd.utils.beir import load_beir
        _, queries, _ = load_beir(args.beir_dataset_dir, args.beir_dataset, split="test")
        return BeirDataset(queries, information_type="query")
    return MSMARCOQueryDataset(args.query_path)


def _collection_dataset(args):
    from scaling_retriever_amd.dataset.dataset import BeirDataset, CollectionDataset
    if args.is_beir and args.beir_dataset is not None:             # eval_sparse.py:80-85
        from scaling_retriever_amd.utils.beir import load_beir
        corpus, _, _ = load_beir(args.beir_dataset_dir, args.beir_dataset, split="test")
        return BeirDataset(corpus, information_type="document")
    source = args.data_source or CORPUS_DATASOURCE.get(args.corpus_path, "msmarco")
    return CollectionDataset(corpus_path=args.corpus_path, data_source=source)


def sparse_index(args):
    from scaling_retriever_amd.dataset.data_collator import LlamaSparseCollectionCollator
    from scaling_retriever_amd.indexer import SparseIndexer
    from scaling_retriever_amd.modeling.llm_encoder import retriever_class
    tokenizer = _tokenizer(args.model_name_or_path)
    collection = _collection_dataset(args)
    model = retriever_class(args.model_name_or_path, "sparse").load_from_lora(args.model_name_or_path)
    if args.token_budget > 0:
        from scaling_retriever_amd.dataset.pipeline import TokenBudgetCollectionLoader
        loader = TokenBudgetCollectionLoader(collection, tokenizer, max_length=args.doc_max_length, max_tokens=args.token_budget,
                                             max_seqs=256, num_workers=args.tokenize_workers,
                                             rank=dist.get_rank() if args.world_size > 1 else 0, world_size=args.world_size)
    else:
        sampler = DistributedSampler(collection, shuffle=False) if args.world_size > 1 else None
        loader = DataLoader(collection, batch_size=args.eval_batch_size, shuffle=False, num_workers=2, sampler=sampler,
                            collate_fn=LlamaSparseCollectionCollator(tokenizer=tokenizer, max_length=args.doc_max_length))
    index_dir = args.index_dir[:-1] if args.index_dir.endswith("/") else args.index_dir
    if args.world_size > 1:
        index_dir = f"{index_dir}_{dist.get_rank()}"               # eval_sparse.py:98-100
    indexer = SparseIndexer(model, index_dir=index_dir, compute_stats=True, dim_voc=model.vocab_size, device=args.local_rank,
                            doc_max_terms=args.doc_max_terms)
    indexer.index(loader)
    if args.world_size > 1:
        dist.barrier()


def sparse_retrieval(args):
    if args.allowed_ids_file and args.world_size > 1:           # before the model and the index shards are loaded
        raise NotImplementedError("--allowed_ids_file is not supported by the doc-sharded retrieval (world_size > 1): "
                                  "run the retrieval task on one process")
    if args.collapse_file and args.world_size > 1:
        raise NotImplementedError("--collapse_file is not supported by the doc-sharded retrieval (world_size > 1): "
                                  "run the retrieval task on one process")
    if args.prf_depth and args.world_size > 1:
        raise NotImplementedError("--prf_depth is not supported by the doc-sharded retrieval (world_size > 1): "
                                  "run the retrieval task on one process")
    if args.mmr_lambda is not None and args.world_size > 1:
        raise NotImplementedError("--mmr_lambda is not supported by the doc-sharded retrieval (world_size > 1): "
                                  "run the retrieval task on one process")
    from scaling_retriever_amd.dataset.data_collator import LlamaSparseCollectionCollator
    from scaling_retriever_amd.indexer import SparseRetrieval
    from scaling_retriever_amd.modeling.llm_encoder import retriever_class
    tokenizer = _tokenizer(args.model_name_or_path)
    queries = _query_dataset(args)
    model = retriever_class(args.model_name_or_path, "sparse").load_from_lora(args.model_name_or_path)
    collate = LlamaSparseCollectionCollator(tokenizer=tokenizer, max_length=args.query_max_length)
    os.makedirs(args.out_dir, exist_ok=True)
    config = {"index_dir": args.index_dir, "out_dir": args.out_dir}
    allowed_ids = None
    if args.allowed_ids_file:
        from scaling_retriever_amd.scoring import read_allowed_ids_file
        allowed_ids = read_allowed_ids_file(args.allowed_ids_file)
    if args.world_size > 1:
        # The reference asserts world_size == 1 here (eval_sparse.py:114) and needs merge_indexes first.  Doc-sharded: each rank
        # scores the index_dir_{rank} it built, encodes its block of the queries, ONE gather of per-shard top-k.
        from torch.utils.data import Subset
        from scaling_retriever_amd.distributed import query_slice
        from scaling_retriever_amd.indexer import ShardedSparseRetrieval
        lo, hi = query_slice(len(queries), dist.get_rank(), args.world_size)
        q_loader = DataLoader(Subset(queries, range(lo, hi)), batch_size=args.eval_batch_size, shuffle=False, num_workers=0,
                              collate_fn=collate)
        retriever = ShardedSparseRetrieval(config=config, model=model, compute_stats=True, dim_voc=model.vocab_size,
                                           device=args.local_rank, query_max_terms=args.query_max_terms)
        res = retriever.retrieve(q_loader, topk=args.top_k, threshold=0.0, allowed_ids=allowed_ids)      # NotImplementedError with a list
        dist.barrier()
        return res
    q_loader = DataLoader(queries, batch_size=args.eval_batch_size, shuffle=False, num_workers=0, collate_fn=collate)
    retriever = SparseRetrieval(config=config, model=model, compute_stats=True, dim_voc=model.vocab_size, device=args.local_rank,
                                query_max_terms=args.query_max_terms)
    collapse = None
    if args.collapse_file:
        from scaling_retriever_amd.collapse import read_collapse_file
        group_of = read_collapse_file(args.collapse_file)
        collapse = lambda d: group_of[str(d)]      # noqa: E731  (collection ids may be ints, the file's are text)
    res = retriever.retrieve(q_loader, topk=args.top_k, threshold=0.0, allowed_ids=allowed_ids, collapse=collapse,
                             hits=args.collapse_hits or None)
    perf = device_perf_writer(args)
    perf("", res)
    if args.prf_depth:
        # the second round, to prf/run.json: the queries are encoded again (retrieve keeps none of them)
        perf("prf", retriever.retrieve_prf(q_loader, topk=args.top_k, threshold=0.0, n_pos=args.prf_depth, n_neg=args.prf_neg_depth,
                                           alpha=args.prf_alpha, beta=args.prf_beta, gamma=args.prf_gamma, max_terms=args.prf_max_terms,
                                           fb_depth=args.prf_depth + args.prf_neg_depth, allowed_ids=allowed_ids))
    if args.mmr_lambda is not None:
        # the diversified run, to mmr/run.json: the queries are encoded again (retrieve keeps none of them)
        perf("mmr", retriever.retrieve_mmr(q_loader, topk=args.top_k, fetch_k=args.mmr_fetch_k, lam=args.mmr_lambda, sim=args.mmr_sim,
                                           threshold=0.0, allowed_ids=allowed_ids))
    return res


def device_perf_writer(args):
    """--device_eval with --eval_qrel_path: a function that writes {out_dir}/{sub}/perf.json from a RunResult's arrays (the judgements
    become arrays once, over the first run's document table); without them, or for a result that is no plain run, it does nothing."""
    if not (args.device_eval and args.eval_qrel_path):
        return lambda *a: None
    from scaling_retriever_amd import evaluation
    from scaling_retriever_amd.utils.run_file import RunResult
    state = {}

    def write(sub, res):
        if not isinstance(res, RunResult):
            return
        if "qrels" not in state or state["qrels"].docs is not res.docs:
            with open(args.eval_qrel_path) as f:
                state["qrels"] = evaluation.Qrels(json.load(f), res.docs)
        evaluation.write_run_perf(os.path.join(args.out_dir, sub, "perf.json"), args.eval_metric, state["qrels"], res)
    return write


def evaluate_msmarco(args):
    if args.device_eval:
        from scaling_retriever_amd.evaluation import device_eval_msmarco
        return device_eval_msmarco(args)
    from scaling_retriever_amd.utils.metrics import load_and_evaluate
    res = {metric: load_and_evaluate(args.eval_qrel_path, args.eval_run_path, metric) for metric in args.eval_metric}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "perf.json"), "w") as fout:
        json.dump(res, fout, indent=4)
    return res


def main(argv=None):
    args = parse_args(argv)
    if args.task_name not in ["evaluate_msmarco", "evaluate_beir"]:
        with open(os.path.join(args.model_name_or_path, "config.json")) as f:
            model_type = json.load(f).get("model_type", "llama")
        assert model_type in ("llama", "qwen2"), model_type        # the HIP path implements the Llama and Qwen2 families
        ddp_setup(args)
    if args.task_name == "indexing":
        sparse_index(args)
    elif args.task_name == "retrieval":
        sparse_retrieval(args)
    elif args.task_name == "evaluate_msmarco":
        evaluate_msmarco(args)
    elif args.task_name == "evaluate_beir":                        # eval_sparse.py:188-193
        from scaling_retriever_amd.utils.beir import load_beir
        from scaling_retriever_amd.utils.metrics import evaluate_beir
        _, _, qrels = load_beir(args.beir_dataset_dir, args.beir_dataset, split="test")
        if args.device_eval:
            from scaling_retriever_amd.evaluation import device_eval_beir
            return device_eval_beir(args, qrels)
        return evaluate_beir(args, qrels)
    else:
        raise NotImplementedError(args.task_name)
    if dist.is_available() and dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
