"""CPU: the numpy model of the top-k protocol (tests/topk_cases.py) against brute force and the oracle, the paths its case list
reaches - asserted, so that an edit of the list cannot silently lose one - and three mutations of the model the cases must see."""
import numpy as np
import pytest

import topk_cases as TC
from oracle import scoring as SC


@pytest.mark.parametrize("c", TC.CASES, ids=lambda c: c["name"])
def test_model_against_brute_force_and_oracle(c):
    r = TC.expected(c)
    k = c["k"]
    for st in range(len(c["steps"]) - 1):
        for q in range(c["nq"]):
            b_ids, b_scores = r["brute"][st][q]
            run_ids, _ = r["run_set"][st][q]
            if c["filter"]:             # the kept set holds the brute-force top-k of everything seen so far
                assert np.isin(b_ids, run_ids).all(), (c["name"], st, q)
            if len(b_ids) == k:         # tau never lies above the true k-th best score
                assert r["tau"][st, q] <= b_scores[-1], (c["name"], st, q)
            else:
                assert r["tau"][st, q] == TC.NINF
            assert r["run"][st, q] == len(run_ids) == len(set(run_ids.tolist()))
    for q in range(c["nq"]):
        v = r["ids"][q] >= 0
        e_ids, e_scores = SC.select_topk(r["ids"][q][v], -r["scores"][q][v], k)
        cnt = len(e_ids)
        assert r["out_counts"][q] == cnt == min(k, int(v.sum()))
        assert np.array_equal(r["out_ids"][q, :cnt], e_ids) and np.array_equal(r["out_scores"][q, :cnt], e_scores)
        assert (r["out_ids"][q, cnt:] == -1).all() and (r["out_scores"][q, cnt:] == np.float32(c["pad_score"])).all()


def test_case_list_limits():
    """What the hook's contract and the suite's running time ask of every case."""
    for c in TC.CASES:
        assert c["nq"] in (1, 5, 9) and c["steps"][0] == 0 and all(a <= b for a, b in zip(c["steps"], c["steps"][1:])), c["name"]
        assert c["steps"][-1] <= 20000 or c["name"] == "k70000_random", c["name"]
        assert 0 <= c["k2"] < c["k"] and c["seg_n"] % 4 == 0 and (c["k"] <= TC.MAX_TOPK or (c["k2"] == 0 and c["seg_n"] == 0)), c["name"]
        scores, ids = TC.make_stream(c)
        assert not np.isnan(scores).any() and ids.max(initial=-1) < 2 ** 32
        for q in range(c["nq"]):
            v = ids[q][ids[q] >= 0]
            assert len(np.unique(v)) == len(v), c["name"]
        if c["tau2_init"] != TC.NINF:      # the sparse scorer's situation: tau2 starts at 0 under scores that are never negative
            assert c["tau2_init"] == 0.0 and (scores >= 0).all(), c["name"]


def test_case_list_reaches_every_path():
    """Coverage is a condition: every path label with every state of the running set, the named union sizes on both sides of both
    register limits, the second rank under a select from registers and from memory, and the shapes that only some cases have."""
    labels, sizes, k2_how, seg_counts = set(), set(), set(), set()
    final_cut_large = final_cut_lds = False
    gather_second_round = head_filled = short_query = empty_query = uneven_step = early_exit_shape = False
    for c in TC.CASES:
        r = TC.expected(c)
        S, lim = len(c["steps"]) - 1, TC.reg_limit(c["k"], c["k2"])
        for st in range(S):
            row = r["label"][st]
            labels.update(row)
            uneven_step |= "idle" in row and any(x != "idle" for x in row) and st > 0
            for q, lab in enumerate(row):
                if lab.startswith("select"):
                    state = lab.split()[1]
                    sizes.add((lim, c["k2"] > 0, int(r["n"][st, q]), state))
                    if c["k2"] > 0:
                        k2_how.add((lim, lab.split()[2]))
                    if lim is None:     # the union's k best end exactly where a plateau of equal scores ends
                        end = c["steps"][st + 1]
                        kth = r["brute"][st][q][1][-1]
                        seen = r["scores"][q, :end][r["ids"][q, :end] >= 0]       # filter = 1: the union's k best are the k best seen
                        early_exit_shape |= c["filter"] == 1 and (seen == kth).sum() > 1 and (seen >= kth).sum() == c["k"]
            if c["seg_n"]:
                a, b, g = c["steps"][st], c["steps"][st + 1], c["seg_group"]
                for q in range(c["nq"]):
                    tau = r["tau"][st - 1, q] if st else np.float32(TC.NINF)
                    ok = r["ids"][q, a:b] >= 0
                    if c["filter"]:
                        ok &= r["scores"][q, a:b] >= tau
                    per = np.add.reduceat(ok.astype(np.int64), np.arange(0, b - a, g))
                    seg_counts.update((int(x), bool(p < c["seg_n"])) for p, x in enumerate(per))
                    gather_second_round |= bool((per[256:c["seg_n"]] > 0).any())
                    head = int(per[c["seg_n"]:].sum() + per[:c["seg_n"]][per[:c["seg_n"]] > 4].sum())
                    longest = max(y - x for x, y in zip(c["steps"], c["steps"][1:]))
                    head_filled |= head > 0 and head < int(per.sum()) == longest
        for q in range(c["nq"]):
            final_cut_large |= c["k"] > TC.MAX_TOPK and r["run"][S - 1, q] > c["k"]
            final_cut_lds |= c["k"] <= TC.MAX_TOPK and r["run"][S - 1, q] > c["k"]
            short_query |= 0 < r["out_counts"][q] < c["k"]
            empty_query |= r["out_counts"][q] == 0
    assert labels == set(TC.ALL_LABELS), sorted(set(TC.ALL_LABELS) ^ labels)
    for state in ("nr=0", "nr<k", "nr>=k"):
        for n in (7167, 7168, 7169):
            assert (7168, False, n, state) in sizes, (n, state)
        for n in (5119, 5120, 5121):
            assert (5120, True, n, state) in sizes, (n, state)
        for n in (7168, 7169):
            assert (7168, True, n, state) in sizes, (n, state)
    assert k2_how >= {(5120, "regs"), (5120, "mem"), (7168, "regs"), (7168, "mem")}, k2_how
    assert final_cut_large and final_cut_lds and short_query and empty_query and uneven_step and early_exit_shape
    for cnt in (0, 1, 4, 5):
        assert (cnt, True) in seg_counts, cnt
    assert any(cnt > 0 and not inside for cnt, inside in seg_counts) and gather_second_round and head_filled
    ks = {c["k"] for c in TC.CASES}
    assert ks >= {1, 2, 255, 256, 257, 1000, 2048, 2049, 4095, 4096, 4097, 5000, 70000}
    by_k = {}
    for c in TC.CASES:
        by_k.setdefault(c["k"], set()).add(c["select_over"])
    assert any(o >= {k, k + 1, k + 1024, 2 * k} and min(o) < k and max(o) > 2 * k for k, o in by_k.items())
    assert {(c["seg_group"]) for c in TC.CASES if c["seg_n"]} >= {1, 8}
    assert {c["tau2_init"] for c in TC.CASES if c["k2"]} == {TC.NINF, 0.0}
    assert any({1, k // 2, k - 1} <= {c["k2"] for c in TC.CASES if c["k"] == k} for k in ks)
    assert any(c["filter"] == 0 and c["seg_n"] for c in TC.CASES) and any(c["filter"] == 0 and c["k"] > TC.MAX_TOPK for c in TC.CASES)


def _differs(a, b):
    return any(not np.array_equal(a[key], b[key]) for key in ("cand", "run", "tau", "out_scores", "out_ids", "out_counts"))


@pytest.mark.parametrize("mutation", ["gt", "skip_nk", "bits"])
def test_cases_see_a_mutated_model(mutation):
    """keep > T instead of >= T, no threshold at n == k, +-0 ordered by their bits: each changes what some case expects (the cheap
    cases are tried first, one is enough)."""
    seen = []
    for c in sorted(TC.CASES, key=lambda c: c["nq"] * c["steps"][-1]):
        if _differs(TC.expected(c), TC.run_model(c, mutation)):
            seen.append(c["name"])
            if len(seen) == 3:
                break
    assert seen, mutation
    if mutation == "bits":      # and what the final output holds differs, not only a trace
        c = TC.BY_NAME["zeros_small"]
        assert not np.array_equal(TC.expected(c)["out_ids"], TC.run_model(c, "bits")["out_ids"])
