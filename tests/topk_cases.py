"""The top-k protocol of csrc/topk.hip / csrc/topk_large.hip as a plain numpy model, and the case list that sr_topk_replay runs.

The model is written from the contract (csrc/common.h at TopkWS / topk_compact2, the header of csrc/topk.hip), not from the kernels:

  per query a running set of (score, id) entries, a threshold tau (-inf at first) and a second threshold tau2;
  per step the survivors are the step's entries with id >= 0 and, with `filter`, score >= tau; nc of them, nr held, n = nr + nc;
    nc == 0                                              nothing happens
    n <= k  or  (nr >= k and n <= clamp(select_over, k, 2k))   the survivors are appended; n == k sets tau to the smallest kept score
    otherwise                                            exactly the k best of the union are kept, tau = the score of the k-th best
  at the end the k best of the set, best first, padded with (pad_score, -1).

"Best" is score descending as FLOAT VALUES (so -0.0 and +0.0 tie), then id ascending: np.lexsort((id, -score as float64)).  The key
bit trick of the kernels is not used anywhere here.  Ids are unique within a query, so a set of entries is kept as arrays sorted by id.

The one implementation constant the model knows is the size of the in-register select (256 x 28 keys; 256 x 20 for k2 > 0 with
2k + 1024 <= 5120; k > 4096 runs the global-memory path).  It only names the path a (step, query) takes - the coverage the host test
asserts, and the steps at which tau2 MUST be refreshed - never an expected value.
"""
import numpy as np

MAX_TOPK = 4096
FLT_MAX = float(np.finfo(np.float32).max)
SUB_MIN = float(np.float32(1e-45))                      # smallest positive subnormal
NINF = float("-inf")

APPEND_LABELS = ("idle", "append<k", "append=k", "append>=k")
SELECT_LABELS = tuple(f"select {nr} {how}" for nr in ("nr=0", "nr<k", "nr>=k") for how in ("regs", "mem", "large"))
ALL_LABELS = APPEND_LABELS + SELECT_LABELS


def reg_limit(k, k2):
    """Largest union the select of this (k, k2) holds in registers; None on the global-memory path."""
    if k > MAX_TOPK:
        return None
    return 256 * 20 if (k2 > 0 and 2 * k + 1024 <= 5120) else 256 * 28


def best_first(scores, ids, by_bits=False):
    """Permutation that puts the entries best first.  by_bits: the (wrong) order of the raw key bits, -0.0 below +0.0 - a mutation."""
    if by_bits:
        u = scores.astype(np.float32).view(np.uint32).astype(np.int64)
        o = np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)
        return np.lexsort((ids, -o))
    return np.lexsort((ids, -scores.astype(np.float64)))


# ------------------------------------------------------------------------------------------------------------------ streams ---
def _scores(kind, n, rng, c):
    f32 = np.float32
    if kind == "random":
        return rng.standard_normal(n).astype(f32)
    if kind == "abs":                                   # non-negative, as the sparse scorer's
        return np.abs(rng.standard_normal(n)).astype(f32)
    if kind == "asc":                                   # every entry survives
        return np.sort(rng.standard_normal(n).astype(f32))
    if kind == "asc_abs":
        return np.sort(np.abs(rng.standard_normal(n)).astype(f32))
    if kind == "desc":                                  # nothing survives once k are held
        return np.sort(rng.standard_normal(n).astype(f32))[::-1].copy()
    if kind in ("plateau", "zeros"):                    # `above` better entries, `plateau` equal ones, the rest worse; shuffled
        a, p = c["above"], c["plateau"]
        s = np.empty(n, f32)
        s[:a] = 1.0 + np.abs(rng.standard_normal(a))
        if kind == "plateau":
            s[a:a + p] = 0.5
        else:                                           # zeros of both signs: equal as floats, different as bits
            s[a:a + p] = np.where(rng.integers(0, 2, p) == 1, f32(-0.0), f32(0.0))
        s[a + p:] = -1.0 - np.abs(rng.standard_normal(n - a - p))
        return s[rng.permutation(n)]
    if kind == "ulp":                                   # neighbours in the last mantissa bits, many exact ties
        return (np.float32(1.0).view(np.int32) + rng.integers(0, 48, n).astype(np.int32)).view(f32)
    if kind == "values":
        special = np.array([np.inf, -np.inf, FLT_MAX, -FLT_MAX, SUB_MIN, -SUB_MIN, 0.0, -0.0, c["pad_score"], 1.0, -1.0], f32)
        s = (rng.standard_normal(n) * 1e-3).astype(f32)
        s[rng.choice(n, len(special), replace=False)] = special
        return s
    raise ValueError(kind)


def make_stream(c):
    """scores fp32 [nq, n], ids int64 [nq, n] of a case (deterministic in its seed)."""
    nq, steps = c["nq"], c["steps"]
    n = steps[-1]
    scores, ids = np.empty((nq, n), np.float32), np.empty((nq, n), np.int64)
    for q in range(nq):
        rng = np.random.default_rng([c["seed"], q])
        s = _scores(c["gen"], n, rng, c)
        i = rng.permutation(n).astype(np.int64)
        if c.get("big_ids"):                            # 0 and 1 are there already
            for small, big in ((n - 1, 2 ** 31), (n - 2, 2 ** 32 - 2), (n - 3, 2 ** 32 - 1)):
                i[i == small] = big
        if c.get("holes"):
            i[rng.random(n) < c["holes"]] = -1
        if c.get("valid_pattern"):                      # producer p of every step keeps its first pattern[p % len] entries
            pat, g = c["valid_pattern"], c["seg_group"]
            for a, b in zip(steps[:-1], steps[1:]):
                for p, lo in enumerate(range(a, b, g)):
                    i[lo + pat[p % len(pat)]:min(lo + g, b)] = -1
        row = c.get("rows", {}).get(q)
        if row == "empty":
            i[:] = -1
        elif row == "short":                            # fewer than k entries in all
            keep = rng.choice(n, max(1, c["k"] // 3), replace=False)
            m = np.ones(n, bool)
            m[keep] = False
            i[m] = -1
        elif row == "desc":
            s = np.sort(s)[::-1].copy()
        scores[q], ids[q] = s, i
    return scores, ids


# -------------------------------------------------------------------------------------------------------------------- model ---
def run_model(c, mutate=None):
    """The protocol on a case.  mutate: None, or one defect the cases must be able to see -
    'gt' (keep > T instead of >= T), 'skip_nk' (no threshold at n == k), 'bits' (order by the key bits)."""
    scores, ids = make_stream(c)
    nq, k, k2, steps = c["nq"], c["k"], c["k2"], c["steps"]
    S = len(steps) - 1
    over = min(max(c["select_over"], k), 2 * k)
    lim = reg_limit(k, k2)
    by_bits = mutate == "bits"
    r = dict(cand=np.zeros((S, nq), np.int32), run=np.zeros((S, nq), np.int32), tau=np.full((S, nq), NINF, np.float32),
             kth2=np.full((S, nq), np.nan, np.float32), n=np.zeros((S, nq), np.int64), label=[[None] * nq for _ in range(S)],
             run_set=[[None] * nq for _ in range(S)], brute=[[None] * nq for _ in range(S)],
             out_scores=np.full((nq, k), c["pad_score"], np.float32), out_ids=np.full((nq, k), -1, np.int64),
             out_counts=np.zeros(nq, np.int32), scores=scores, ids=ids)
    for q in range(nq):
        run_s, run_i = np.empty(0, np.float32), np.empty(0, np.int64)
        tau = np.float32(NINF)
        for st in range(S):
            s, i = scores[q, steps[st]:steps[st + 1]], ids[q, steps[st]:steps[st + 1]]
            m = i >= 0
            if c["filter"]:
                m &= s >= tau
            nc, nr = int(m.sum()), len(run_i)
            n = nr + nc
            if nc == 0:
                label = "idle"
            else:
                u_s, u_i = np.concatenate([run_s, s[m]]), np.concatenate([run_i, i[m]])
                o = best_first(u_s, u_i, by_bits)
                if n <= k or (nr >= k and n <= over):
                    run_s, run_i = u_s, u_i
                    if n == k and mutate != "skip_nk":
                        tau = u_s[o[k - 1]]
                    label = "append<k" if n < k else ("append=k" if n == k else "append>=k")
                else:
                    keep = o[:k - 1] if mutate == "gt" else o[:k]
                    run_s, run_i = u_s[keep], u_i[keep]
                    tau = u_s[o[k - 1]]
                    if k2 > 0:
                        r["kth2"][st, q] = u_s[o[k2 - 1]]
                    how = "large" if lim is None else ("regs" if n <= lim else "mem")
                    label = f"select {'nr=0' if nr == 0 else ('nr<k' if nr < k else 'nr>=k')} {how}"
            by_id = np.argsort(run_i)
            run_s, run_i = run_s[by_id], run_i[by_id]
            r["cand"][st, q], r["run"][st, q], r["tau"][st, q], r["n"][st, q] = nc, len(run_i), tau, n
            r["label"][st][q] = label
            r["run_set"][st][q] = (run_i, run_s)
            seen_s, seen_i = scores[q, :steps[st + 1]], ids[q, :steps[st + 1]]
            v = seen_i >= 0
            b = best_first(seen_s[v], seen_i[v], by_bits)[:k]
            r["brute"][st][q] = (seen_i[v][b], seen_s[v][b])
        o = best_first(run_s, run_i, by_bits)[:k]
        r["out_scores"][q, :len(o)], r["out_ids"][q, :len(o)], r["out_counts"][q] = run_s[o], run_i[o], len(o)
    return r


_expected = {}


def expected(c):
    """The model's result of a case, computed once per process and never modified by its readers."""
    if c["name"] not in _expected:
        _expected[c["name"]] = run_model(c)
    return _expected[c["name"]]


# -------------------------------------------------------------------------------------------------------------------- cases ---
def offsets(lengths):
    return [0] + [int(x) for x in np.cumsum(lengths)]


def _case(name, k, lengths, gen="random", nq=5, k2=0, select_over=None, filter=1, seg_n=0, seg_group=1, tau2_init=NINF,
          pad_score=-FLT_MAX, **extra):
    c = dict(name=name, nq=nq, k=k, k2=k2, select_over=2 * k if select_over is None else select_over, filter=filter, seg_n=seg_n,
             seg_group=seg_group, tau2_init=tau2_init, pad_score=pad_score, steps=offsets(lengths), gen=gen)
    c.update(extra)
    return c


def _chunks(k, total):
    """k // 2 entries, then up to exactly k (n == k while tau is still -inf), then pieces of about 0.7 k until `total`."""
    first = max(1, k // 2)
    out = [first, k - first] if k > first else [first]
    piece = (7 * k) // 10 + 37
    while sum(out) < total:
        out.append(min(piece, total - sum(out)))
    return out


def _build():
    cases = []
    nqs = (1, 5, 9)

    def add(*a, **kw):
        kw.setdefault("nq", nqs[len(cases) % 3])
        kw["seed"] = 1000 + len(cases)
        cases.append(_case(*a, **kw))

    # k edges: LDS select and sort up to 4096 (the 64 KB sort), the global-memory path beyond
    for k in (1, 2, 255, 256, 257, 1000, 2048, 2049, 4095, 4096, 4097, 5000):
        add(f"k{k}_random", k, _chunks(k, min(3 * k + 700, 20000)))
    add("k70000_random", 70000, [50000, 50000, 60000], nq=1)      # two tiled merge stages in the final sort

    # union sizes at the in-register boundaries, each from an empty, a partly filled and a full running set.  Ascending scores: every
    # entry survives, so the step lengths are the counts; one random step follows the select
    def boundary(tag, k, k2, over, sizes):
        for n in sizes:
            for state, head in (("nr0", []), ("nrlt", [k // 3]), ("nrge", [k])):
                add(f"{tag}_n{n}_{state}", k, head + [n - sum(head), 500], gen="asc", k2=k2, select_over=over)
    boundary("r28", 3000, 0, 6000, (7167, 7168, 7169))
    boundary("r20", 2048, 1024, 4096, (5119, 5120, 5121))
    boundary("r28k2", 3072, 1536, 3072 + 1024, (7168, 7169))       # the dense filter's shape: k2 > 0 on the 28-key instance
    for state, head in (("nr0", [6000]), ("nrlt", [2000, 4000]), ("nrge", [4500, 5000])):
        add(f"large_{state}", 4500, head + [700], gen="asc")

    # select_over, and its clamp into [k, 2k] on both sides
    for over in (1500, 1501, 1500 + 1024, 3000, 100, 10 ** 6):
        add(f"over{over}", 1500, [700, 800] + [300] * 12, select_over=over, k2=750)

    # stream shapes, on the LDS path and on the global-memory path
    for tag, k, total in (("s", 300, 2400), ("l", 4500, 16000)):
        step = [k // 2, k - k // 2] + [(total - k) // 8] * 8
        add(f"{tag}_asc", k, step, gen="asc")
        add(f"{tag}_desc", k, step, gen="desc")
        add(f"{tag}_plateau_straddle", k, step, gen="plateau", above=k // 2, plateau=k)            # the id digits decide
        add(f"{tag}_plateau_exact", k, step, gen="plateau", above=k // 2, plateau=k - k // 2)      # the plateau ends at rank k
        add(f"{tag}_ulp", k, step, gen="ulp")
        add(f"{tag}_zeros", k, step, gen="zeros", above=k // 2, plateau=k)
        add(f"{tag}_mixed_rows", k, step, nq=5, rows={0: "empty", 1: "short", 3: "desc"}, holes=0.2)
        add(f"{tag}_plateau_nofilter", k, step, gen="plateau", above=k // 2, plateau=k, filter=0)
        add(f"{tag}_random_nofilter", k, step, filter=0, select_over=k + 1)
    add("l_plateau_exact_one_step", 4500, [9100], gen="plateau", above=2250, plateau=2250)        # the select ends with the score digits
    add("l_plateau_exact_full_set", 4500, [4500, 4600], gen="plateau", above=2250, plateau=2250)
    add("one_plateau_all_passes", 4500, [3000, 3000, 3000, 3000], gen="plateau", above=0, plateau=12000)

    # values
    for k in (4, 16, 60):
        add(f"values_k{k}", k, [16] * 4, gen="values", pad_score=-1.0, big_ids=True)
        add(f"values_k{k}_nofilter", k, [16] * 4, gen="values", pad_score=-1.0, big_ids=True, filter=0)
    add("zeros_small", 4, [3, 3, 6], gen="zeros", above=2, plateau=8)
    add("zeros_one_step", 40, [500], gen="zeros", above=20, plateau=300)
    add("big_ids_plateau", 5, [4, 4, 8], gen="plateau", above=0, plateau=16, big_ids=True)
    add("big_ids_keep_all_but_one", 15, [4, 4, 8], gen="plateau", above=0, plateau=16, big_ids=True)

    # segmented candidate slots (4 slots per segment)
    add("seg_g1", 50, [20] * 10, seg_n=8, seg_group=1)                                            # producers beyond seg_n
    add("seg_g8_counts", 100, [480] * 4, gen="asc", seg_n=48, seg_group=8, valid_pattern=[0, 1, 4, 5, 8, 3])   # 5 and 8 overflow
    add("seg_two_rounds", 1000, [600, 600, 600], gen="asc", seg_n=520, seg_group=1)               # 130 count words: a second gather round
    add("seg_two_rounds_g8", 1000, [2400] * 3, seg_n=288, seg_group=8, holes=0.6)
    add("seg_fills_head", 120, [100, 200, 150], gen="asc", seg_n=64, seg_group=1)                 # step 1: 64 + 136 = seg_off
    add("seg_random_k2", 256, [512] * 16, seg_n=64, seg_group=8, k2=128, select_over=256 + 64)
    add("seg_nofilter", 64, [96] * 6, seg_n=16, seg_group=8, filter=0, holes=0.3)
    add("seg_mixed_rows", 300, [400] * 6, nq=9, seg_n=40, seg_group=8, rows={2: "empty", 4: "short", 8: "desc"})

    # k2 / tau2: -inf as the dense filter starts it, 0 as the certified sparse scorer does (its scores are never negative; a
    # tau2_init above the scores is outside the caller's protocol: topk_compact2 assigns, it does not take a maximum)
    for k2 in (1, 256, 511):
        add(f"k2_{k2}_inf", 512, [200, 312] + [350] * 8, k2=k2, select_over=512 + 128)
        add(f"k2_{k2}_zero", 512, [200, 312] + [350] * 8, gen="abs", k2=k2, tau2_init=0.0, select_over=512)
    add("k2_mem_then_regs", 2048, [2048, 1500, 1600, 2000], gen="asc_abs", k2=1024, tau2_init=0.0, select_over=2048 + 1500)
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    return cases


CASES = _build()
BY_NAME = {c["name"]: c for c in CASES}
