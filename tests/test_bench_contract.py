"""CPU: the contract line bench.py prints as the LAST line of stdout is what the driver can parse - compact (the round-5 line had
grown to 23 KB and the driver's record came back unparsed), strict JSON (no NaN / Infinity tokens anywhere on it), with the metric
fields, `roofline` of the dominant kernel and `cpu_baseline`.  Checked twice: on the line `bench.contract_line` makes from a full
record (profiles/r05_bench_line.json is round 5's full record), and on the line committed for the current round
(profiles/r06_bench_line.json, `python bench.py` on one MI355X).  Guards the line's shape, not its numbers."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURRENT = os.path.join(ROOT, "profiles", "r06_bench_line.json")


def _reject_constant(name):
    raise ValueError(f"non-finite constant {name} on the contract line")


def check_contract_line(text):
    text = text.rstrip("\n")
    assert "\n" not in text                                     # ONE line
    assert len(text) < 8192, len(text)
    assert "Infinity" not in text and "NaN" not in text
    d = json.loads(text, parse_constant=_reject_constant)
    for key, typ in (("metric", str), ("value", float), ("unit", str), ("n_gpus", int), ("steps", int), ("warmup", int),
                     ("ms_per_step", float), ("higher_is_better", bool), ("scaling", str), ("dtype", str), ("data", str), ("config", dict)):
        assert isinstance(d[key], typ), key
    assert d["higher_is_better"] is True and d["vs_baseline"] is None and d["data"] == "synthetic"
    assert "workload" in d["config"] and "model" not in d["config"] and d["config"]["ranks"]["world_size"] == d["n_gpus"]
    assert abs(d["value"] - d["config"]["n_queries"] / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-3
    r = d["roofline"]
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s") and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert r["traffic"] is None or r["traffic"] > 0
    # the achieved figure is algorithmic work per launch over the measured launch duration
    assert abs(r["flop_per_launch"] / (r["avg_launch_ms"] * 1e-3) / 1e12 - r["achieved"]) / r["achieved"] < 1e-2
    if d["n_gpus"] == 1:
        c = d["cpu_baseline"]
        assert c["kind"] in ("port", "reference") and c["cores"] >= 1 and c["value"] > 0 and c["sample"] and c["unit"] == d["unit"]
        assert len(c["sample"]) <= 200
    assert "bit-identical" in d["parity"]
    return d


def test_contract_line_from_a_full_record_is_compact_and_strict():
    sys.path.insert(0, ROOT)
    argv, sys.argv = sys.argv, ["bench.py"]
    try:
        import bench
    finally:
        sys.argv = argv
    with open(os.path.join(ROOT, "profiles", "r05_bench_line.json")) as f:
        full = json.load(f)
    assert "Infinity" in json.dumps(full)                       # the record that broke the driver's parser in round 5
    full["breakdown"]["query_encode_ms"] = float("inf")         # and a non-finite number on top of it
    d = check_contract_line(bench.contract_line(full))
    assert d["breakdown"]["query_encode_ms"] is None
    assert d["sparse"]["qps"] == full["sparse"]["value"] and d["encode"]["frac"] == full["encode"]["roofline"]["frac"]
    assert d["sparse"]["sweep"]["cells"] == len(full["sparse"]["sparse_sweep"]["rows"])
    assert len(bench.contract_line(full)) < bench.CONTRACT_LINE_MAX <= 4096


@pytest.mark.skipif(not os.path.exists(CURRENT), reason="no bench line committed for this round yet")
def test_committed_bench_line_of_this_round():
    with open(CURRENT) as f:
        d = check_contract_line(f.read())
    assert d["n_gpus"] == 1
    for leg in ("breakdown", "exact_kernel", "drop_in", "encode", "sparse", "config5_8b", "small_batch"):
        assert d.get(leg), leg
    assert d["sparse"]["traffic"] is None or d["sparse"]["traffic"] > 0
    assert d["sparse"]["sweep"]["cells"] >= 12 and d["sparse"]["sweep"]["all_bit_exact"] is True
    assert d["encode"]["padded_128_passages_per_s"] > 0


def _import_bench():
    sys.path.insert(0, ROOT)
    argv, sys.argv = sys.argv, ["bench.py"]
    try:
        import bench
    finally:
        sys.argv = argv
    return bench


def test_plain_run_record_gives_a_strict_line_with_the_headline_fields():
    """A run without --full emits the record of the timed steps alone: the headline fields and `roofline`, every other leg null."""
    import argparse
    bench = _import_bench()
    with open(os.path.join(ROOT, "profiles", "r05_bench_line.json")) as f:
        full = json.load(f)
    args = argparse.Namespace(n_queries=6980, steps=3, warmup=1, topk=1000, n_docs=8_841_823, query_batch=6980, exact_kernel=False)
    ranks = {"world_size": 1, "backend": None, "shard_docs": [8_841_823], "queries_encoded_per_rank": [6980]}
    res = bench.record(args, dict(bench.LION_1B), 1, 1.5, ranks, roofline=full["roofline"])
    assert all(res[k] is None for k in bench.LEGS if k != "roofline")
    text = bench.contract_line(res)
    assert "\n" not in text and len(text) < bench.CONTRACT_LINE_MAX
    d = json.loads(text, parse_constant=_reject_constant)
    assert d["metric"] == full["metric"] and d["unit"] == "queries/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["steps"] == 3 and d["ms_per_step"] == 500.0 and abs(d["value"] - 6980 / 0.5) < 1e-6
    assert d["roofline"]["bound"] == "mfma" and d["cpu_baseline"] is None and d["sparse"] is None


def test_dump_outputs_writes_every_row_within_64_mb_and_samples_a_larger_output(tmp_path):
    import numpy as np
    import torch
    bench = _import_bench()
    g = torch.Generator().manual_seed(0)
    s = torch.randn((6980, 1000), generator=g)
    i = torch.randint(0, 8_841_823, (6980, 1000), generator=g)
    bench.dump_outputs(str(tmp_path / "a"), s, i, n_docs=8_841_823)
    files = {f: np.load(tmp_path / "a" / f) for f in ("scores.npy", "ids.npy", "query_rows.npy")}
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64_000_000
    assert files["scores.npy"].dtype == np.float32 and files["ids.npy"].dtype == np.float32 and files["query_rows.npy"].dtype == np.float64
    assert np.array_equal(files["scores.npy"], s.numpy()) and np.array_equal(files["ids.npy"].astype(np.int64), i.numpy())
    assert np.array_equal(files["query_rows.npy"], np.arange(6980))
    # ids beyond 2^24 need float64: the 6 980 rows no longer fit, a fixed sample of them is written, the same one every time
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), s, i + (1 << 24), n_docs=1 << 25)
    rows = np.load(tmp_path / "b" / "query_rows.npy").astype(np.int64)
    assert 0 < len(rows) < 6980 and np.all(np.diff(rows) > 0)
    assert sum(os.path.getsize(tmp_path / "b" / f) for f in files) <= 64_000_000
    ids = np.load(tmp_path / "b" / "ids.npy")
    assert ids.dtype == np.float64 and np.array_equal(ids.astype(np.int64), i.numpy()[rows] + (1 << 24))
    for f in files:
        assert np.array_equal(np.load(tmp_path / "b" / f), np.load(tmp_path / "c" / f))
