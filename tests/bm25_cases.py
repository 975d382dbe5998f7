"""Models and the error bound of the BM25 tests (tests/test_bm25_host.py, test_token_counts_gpu.py, test_bm25_weights_gpu.py,
test_bm25_search_gpu.py).  Nothing here imports scaling_retriever_amd.bm25: the host formulas are restated.

Three independent statements of the same thing:
  model_token_counts   sr_token_counts in numpy: per row np.unique over the counted slots.
  model_bm25_weights   sr_bm25_weights in numpy: np.float32 values, one rounded operation per line (with model_scalars / model_idf, the
                       host side one operation per line as well).
  textbook_scores      float64 BM25 over token lists with dicts - the formula as the papers print it, sharing no code with the models.

The bound: relative error of the fp32 weight against the real-number formula
----------------------------------------------------------------------------
Real numbers (k1 >= 0, 0 <= b <= 1, integers 1 <= tf, dl <= 2^24, N >= df >= 0, avgdl > 0):
    W* = idf* . tf (k1 + 1) / D*,   D* = tf + K*,   K* = a* + s* dl,   a* = k1 (1 - b),   s* = k1 b / avgdl,   idf* = log1p(x).
u = 2^-24 is the unit roundoff of fp32, every d_i below has |d_i| <= u, second-order terms are collected at the end.
  scalars   k1f = k1 (1 + d1), bf = b (1 + d2)                                               2 roundings (the casts)
  numer     f32(k1f + 1) = (k1 + 1 + k1 d1)(1 + d3): relative error <= u k1 / (k1 + 1) + u <= 2 u      (Lucene form: exactly 1)
  a         f32(1 - bf) = (1 - b - b d2)(1 + d4) = 1 - b + e with |e| <= b u + (1 - b) u = u - an ABSOLUTE error: the relative one is
            unbounded as b -> 1.  a = k1f . (1 - b + e) . (1 + d5), so |a - a*| <= 2 u a* + k1 u.
  s         f32(k1f . bf) carries d1, d2, d6; f32(avgdl) d7 (avgdl itself is a float64 quotient of integers: 2^-53, ignored against u);
            the division d8: |s - s*| <= 5 u s*.
  K         dl is exact in fp32 (<= 2^24).  f32(s . dl): one more rounding, |sl - s* dl| <= 6 u s* dl.  K = f32(a + sl):
            |K - K*| <= 2 u a* + k1 u + 6 u s* dl + u K* <= 7 u K* + k1 u.
  D         tf is exact.  D = f32(tf + K): |D - D*| <= 7 u K* + k1 u + u D*.  With K* < D* and D* >= tf >= 1:
            relative error of D <= (8 + k1) u.
  numerator f32(tf . numer): 2 u from numer, one rounding: <= 3 u.
  quotient  f32(numerator / D), correctly rounded: <= 3 u + (8 + k1) u + u = (12 + k1) u.
  idf       log1p in float64 (error ~2^-52, ignored against u), one rounding to fp32: u.
  product   f32(idf . quotient): one rounding.  Total: (12 + k1) u + u + u = (14 + k1) u.
Second-order terms: at most 16 factors (1 + d), their cross terms are below 16^2 u^2 / 2 < 2^-17 (14 + k1) u; the bound carries the factor
(1 + 2^-16), which also covers the float64 steps.  rel_bound(0.9) = 14.9 u; the largest error a CPU trial of 2 M random postings showed
was 3.9 u (N = 200 000, lengths 1 - 512, k1 = 0.9, b = 0.4): the bound is about four times what random inputs reach, as worst-case
bounds of a dozen roundings are.
"""
import math
from collections import Counter

import numpy as np

U = 2.0 ** -24


def rel_bound(k1):
    """The derived bound on |w_fp32 - W*| / W* (module docstring)."""
    return (14.0 + float(k1)) * U * (1.0 + 2.0 ** -16)


# ------------------------------------------------------------------------------------------------------------------ token counts
def counted_slots(ids, mask, skip_ids):
    ids = np.asarray(ids, np.int64)
    counted = np.ones(ids.shape, bool) if mask is None else np.asarray(mask) != 0
    for s in skip_ids:
        counted &= ids != s
    return counted


def model_token_counts(ids, mask=None, skip_ids=(), n_terms=None):
    """(row_ptr int64 [B + 1], cols int32, vals fp32, lengths int32 [B]) of sr_token_counts; a counted id outside [0, n_terms) raises
    ValueError with the smallest (row, position)."""
    ids = np.asarray(ids, np.int64)
    B = ids.shape[0]
    counted = counted_slots(ids, mask, skip_ids)
    bad = counted & ((ids < 0) | (ids >= n_terms))
    if bad.any():
        r, p = np.argwhere(bad)[0]
        raise ValueError(f"row {r}, position {p}, id {ids[r, p]}")
    row_ptr, cols, vals = [0], [], []
    for b in range(B):
        u, c = np.unique(ids[b][counted[b]], return_counts=True)
        cols.append(u.astype(np.int32))
        vals.append(c.astype(np.float32))
        row_ptr.append(row_ptr[-1] + len(u))
    cat = lambda xs, dt: np.concatenate(xs).astype(dt) if xs else np.zeros(0, dt)      # noqa: E731
    return np.asarray(row_ptr, np.int64), cat(cols, np.int32), cat(vals, np.float32), counted.sum(1).astype(np.int32)


# ----------------------------------------------------------------------------------------------------------------------- weights
def model_scalars(k1, b, avgdl, lucene=False):
    f = np.float32
    k1f = f(k1)
    bf = f(b)
    one_plus = f(k1f + f(1))
    numer = f(1) if lucene else one_plus
    one_minus_b = f(f(1) - bf)
    a = f(k1f * one_minus_b)
    if avgdl == 0:
        return numer, a, f(0)
    k1b = f(k1f * bf)
    s = f(k1b / f(avgdl))
    return numer, a, s


def model_idf(df, n_docs):
    df = np.asarray(df, np.float64)
    return np.log1p((np.float64(n_docs) - df + 0.5) / (df + 0.5)).astype(np.float32)


def model_bm25_weights(indptr, doc_ids, tf, doc_len, idf, numer, a, s):
    f = np.float32
    indptr = np.asarray(indptr, np.int64)
    term = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    tf = np.asarray(tf, f)
    dl = np.asarray(doc_len)[np.asarray(doc_ids, np.int64)].astype(f)
    sl = (f(s) * dl).astype(f)
    K = (f(a) + sl).astype(f)
    num = (tf * f(numer)).astype(f)
    den = (tf + K).astype(f)
    q = (num / den).astype(f)
    return (np.asarray(idf, f)[term] * q).astype(f)


def real_weights(indptr, doc_ids, tf, doc_len, n_docs, k1, b, avgdl, lucene=False):
    """The real-number formula in float64, from (k1, b, avgdl) themselves - not from rounded scalars."""
    indptr = np.asarray(indptr, np.int64)
    df = np.diff(indptr).astype(np.float64)
    idf = np.log1p((n_docs - df + 0.5) / (df + 0.5))
    term = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    tf = np.asarray(tf, np.float64)
    dl = np.asarray(doc_len, np.float64)[np.asarray(doc_ids, np.int64)]
    K = k1 * (1.0 - b) + (k1 * b / avgdl if avgdl else 0.0) * dl
    return idf[term] * tf * (1.0 if lucene else k1 + 1.0) / (tf + K)


def random_postings(rng, n_terms, n_docs, nnz, max_len=512, max_tf=None):
    """A random term-major CSR with document lengths: (indptr, doc_ids, tf, doc_len); doc ids ascending inside a term where they fit."""
    doc_len = rng.integers(1, max_len + 1, n_docs).astype(np.int32)
    term = np.sort(rng.integers(0, n_terms, nnz))
    indptr = np.concatenate([[0], np.cumsum(np.bincount(term, minlength=n_terms))]).astype(np.int64)
    doc_ids = rng.integers(0, n_docs, nnz).astype(np.int32)
    tf = rng.integers(1, (max_tf or max_len) + 1, nnz).astype(np.float32)
    return indptr, doc_ids, tf, doc_len


# ---------------------------------------------------------------------------------------------------------------------- textbook
def textbook_scores(docs, query, k1, b, lucene=False, query_tf=True):
    """{doc position: float64 BM25 score} of one query (a token list) over docs (token lists): the sum over the query's distinct terms of
    qtf . idf(t) . tf (k1 + 1) / (tf + k1 (1 - b + b |d| / avgdl)); documents that share no term are absent."""
    n = len(docs)
    avgdl = sum(len(d) for d in docs) / n if n else 0.0
    df = Counter()
    for d in docs:
        df.update(set(d))
    out = {}
    for t, qtf in sorted(Counter(query).items()):
        if t not in df:
            continue
        idf = math.log1p((n - df[t] + 0.5) / (df[t] + 0.5))
        for pos, d in enumerate(docs):
            tf = d.count(t)
            if tf:
                norm = k1 * (1.0 - b + (b * len(d) / avgdl if avgdl else 0.0))
                out[pos] = out.get(pos, 0.0) + (qtf if query_tf else 1) * idf * tf * (1.0 if lucene else k1 + 1.0) / (tf + norm)
    return out


# ------------------------------------------------------------------------------------------------------------------ test corpus
WORDS = [f"w{i}" for i in range(400)]


def word_corpus(n_docs, seed, min_words=3, max_words=40, zipf=1.3):
    """[(doc id, text)] of Zipf-distributed words: frequent words in most documents, rare ones in few."""
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, len(WORDS) + 1) ** zipf
    p /= p.sum()
    out = []
    for i in range(n_docs):
        n = int(rng.integers(min_words, max_words + 1))
        out.append((f"d{i}", " ".join(WORDS[j] for j in rng.choice(len(WORDS), n, p=p))))
    return out


def word_queries(n, seed, min_words=2, max_words=5):
    rng = np.random.default_rng(seed)
    return [(f"q{i}", " ".join(WORDS[j] for j in rng.integers(0, 120, int(rng.integers(min_words, max_words + 1))))) for i in range(n)]


def token_lists(pairs, tokenizer, max_length, skip_ids):
    """The counted tokens of every text, as the collator + sr_token_counts see them."""
    return [[t for t in tokenizer._encode(text, max_length, True) if t not in skip_ids] for _, text in pairs]


DOC_MAX_LENGTH, QUERY_MAX_LENGTH = 96, 16
EMPTY_DOC = 17


def search_case(n_docs=300, n_queries=24, seed=7):
    """([(doc id, text)], [(query id, text)]) of the search tests: documents of 10 - 80 words (document
    EMPTY_DOC has none), queries of 4 - 7."""
    docs = word_corpus(n_docs, seed=seed, min_words=10, max_words=80)
    docs[EMPTY_DOC] = (docs[EMPTY_DOC][0], "")             # no counted token: no posting, no doc_ids entry, but one of the N documents
    return docs, word_queries(n_queries, seed=seed + 1, min_words=4, max_words=7)


def near_tie_census(score_dicts, k, bound_of):
    """(adjacent pairs, pairs closer than the bound) over the float64 top-(k + 1) of every query: score_dicts = [{doc: score}], bound_of(q)
    = the relative bound of query q's scores."""
    pairs = close = 0
    for q, sc in enumerate(score_dicts):
        top = sorted(sc.values(), reverse=True)[:k + 1]
        for x, y in zip(top[:-1], top[1:]):
            pairs += 1
            close += (x - y) <= bound_of(q) * x
    return pairs, close
