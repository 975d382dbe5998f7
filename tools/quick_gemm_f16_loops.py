#!/usr/bin/env python3
"""fp16-plane residual GEMM (EPI_RESID_F32_H through sr_gemm_f16_scaled) at the o_proj and down_proj shapes of a 1B layer, per plane
segment count (K' = 2 K, 3 K): the eight-wave against the four-wave 256 x 256 loop (SR_GEMM_BIG=8w | 4w), alternating, HIP events.
The gate-up GEMM's epilogue has no entry point of its own: its two loops are compared by the kernel rows of a profile
(rocprofv3 --kernel-trace --stats over tools/quick_query_encode.py with SR_GEMM_BIG=8w and =4w).
python tools/quick_gemm_f16_loops.py [tokens] [OUT.json]"""
import json
import os
import sys

os.environ["SR_DEV_SWITCHES"] = "1"   # the library reads its development switches only with this set
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from scaling_retriever_amd import _lib as L  # noqa: E402

lib = L.load()
M = int(sys.argv[1]) if len(sys.argv) > 1 else 60841


def run(N, K, loop, iters=10):
    g = torch.Generator(device="cuda").manual_seed(0)
    A = torch.randn((M, K), device="cuda", generator=g).half()
    W = (torch.randn((N, K), device="cuda", generator=g) * 0.02).half()
    a_s = torch.ones(M, device="cuda")
    w_s = torch.ones(N, device="cuda")
    C = torch.zeros((M, N), dtype=torch.float32, device="cuda")
    os.environ["SR_GEMM_BIG"] = loop

    def f():
        L.check(lib.sr_gemm_f16_scaled(A.data_ptr(), W.data_ptr(), M, N, K, a_s.data_ptr(), w_s.data_ptr(), C.data_ptr(), L.stream_ptr()))
    for _ in range(2):
        f()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


rows = []
for name, N, K in (("o_proj", 2048, 2048), ("down_proj", 2048, 8192)):
    for nseg in (2, 3):
        t = {"8w": [], "4w": []}
        for rnd in range(3):
            for loop in ("8w", "4w"):
                t[loop].append(round(run(N, nseg * K, loop), 4))
        row = {"gemm": name, "M": M, "N": N, "K": K, "segments": nseg, "ms_8w": t["8w"], "ms_4w": t["4w"],
               "four_over_eight": round(min(t["4w"]) / min(t["8w"]), 4)}
        rows.append(row)
        print(json.dumps(row), flush=True)
if len(sys.argv) > 2:
    with open(sys.argv[2], "w") as f:
        json.dump(rows, f, indent=1)
