"""Shared by tests/test_qwen2_cpu.py and tests/test_qwen2_gpu.py: the Qwen2 fixtures' weights and the oracle restatement of a
Qwen2 layer - oracle.llama_bi driven through a Hooks subclass whose `lin` adds the bias that belongs to the weight array it is
handed (a Qwen2 layer is a Llama layer whose q_proj / k_proj / v_proj carry a bias, added before the rotation)."""
import json
import os

import numpy as np

from golden_weights import make_weights
from oracle import llama_bi as LB

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("enc_qwen2_hd64", "enc_qwen2_hd128")


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def load_case(name):
    """(fixture, config dict, weights incl. biases)."""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    cfg = json.loads(str(z["config_json"]))
    w = make_weights(cfg, int(z["weight_seed"]))
    for k in z.files:
        if k.startswith("bias:"):
            w[k[5:]] = z[k]
    return z, cfg, w


def random_biases(cfg, seed, std=1.0):
    rng = np.random.default_rng(seed)
    nh, nkv = cfg["num_attention_heads"], cfg["num_key_value_heads"]
    hd = cfg.get("head_dim") or cfg["hidden_size"] // nh
    out = {}
    for i in range(cfg["num_hidden_layers"]):
        for nm, n in (("q", nh * hd), ("k", nkv * hd), ("v", nkv * hd)):
            out[f"model.layers.{i}.self_attn.{nm}_proj.bias"] = (rng.standard_normal(n, dtype=np.float32) * np.float32(std))
    return out


class BiasHooks(LB.Hooks):
    """Hooks whose nn.Linear adds `<name>.bias` when handed the array stored as `<name>.weight` (lookup by id()).
    fp32: every linear layer accumulates in float64 and rounds its result to fp32 once, so the restatement adds no GEMM rounding of
    its own to a comparison with an fp32 run (numpy's fp32 GEMM and the reference's sum the same 128-1 536 products in different
    orders; against the reference's goldens that alone was 4.0e-6 on a near-zero logit of enc_qwen2_hd64, 3.4e-6 with this).
    bf16: what autocast does - the bias cast to bf16, added to the fp32 accumulator, one rounding of the sum."""

    def __init__(self, weights, bf16=False):
        super().__init__(bf16=bf16)
        self.bias_of = {id(weights[k[:-4] + "weight"]): v for k, v in weights.items() if k.endswith(".bias")}
        self._keep = weights        # the ids stay valid as long as the arrays live

    def lin(self, x, w):
        b = self.bias_of.get(id(w))
        if self.bf16:
            if b is None:
                return super().lin(x, w)
            return LB.bf16_round(LB.bf16_round(x) @ LB.bf16_round(w).T + LB.bf16_round(b))
        y = np.asarray(x, np.float64) @ np.asarray(w, np.float64).T
        if b is not None:
            y += b.astype(np.float64)
        return y.astype(np.float32)
