"""CPU: the numpy model of what loading leaves on the device (tests/model_load_cases.py) holds its own properties, its checker sees
every defect a loader could have, and the loader's file routes (_read_checkpoint) return names, dtypes and values exactly."""
import json
import os
import re

import numpy as np
import pytest
import torch

import bf16_regime_cases as G
import fp32_plane_cases as P
import model_load_cases as M

F32 = np.float32


def _f16(words):
    return np.ascontiguousarray(words).view(np.float16)


@pytest.fixture(scope="module")
def model_bias():
    cfg = M.config(tied=False, bias=True)
    return cfg, M.tensors(cfg)


# ---------------------------------------------------------------------------------------------- the values
def test_value_sets_hold_the_edges():
    cfg = M.config(tied=False, bias=True)
    t, tb = M.tensors(cfg), M.tensors(cfg, bf16_only=True)
    assert [n for n, _ in M.tensor_shapes(cfg)] == list(t) == list(tb)
    r = M.SPECIAL_ROWS
    for name, shape in M.tensor_shapes(cfg):
        w, wb = t[name], tb[name]
        assert w.shape == shape and w.dtype == F32 and np.isfinite(w).all() and np.isfinite(wb).all()
        assert not (wb.view(np.uint32) & np.uint32(0xFFFF)).any(), name                 # bf16 numbers only
        if w.ndim == 1:
            u = w.view(np.uint32)
            assert (u == 0x80000000).any() and (u == 0).any() and ((u & 0x7F800000) == 0).sum() >= 8
            assert ((u & 0xFFFF) == 0x8000).sum() >= 4
            continue
        u = w[r["halfway"]].view(np.uint32)
        low, parity = u & 0xFFFF, (u >> 16) & 1
        for lw in (0x8000, 0x7FFF, 0x8001):
            for par in (0, 1):
                assert ((low == lw) & (parity == par)).sum() >= 8, (name, hex(lw), par)
        z = w[r["zeros_subnormals"]].view(np.uint32)
        assert (z == 0).any() and (z == 0x80000000).any() and (((z & 0x7F800000) == 0) & ((z & 0x7FFFFFFF) != 0)).sum() >= 7
        assert (np.abs(w[r["saturating"]]).view(np.uint32) >= 0x7F7F8000).sum() == 2
        assert not w[r["all_zero"]].any() and not wb[r["all_zero"]].any()
        for x in (w, wb):
            assert np.abs(x[r["pow2_max"]]).max() == 0.5
            below = np.abs(x[r["below_pow2_max"]]).max()
            assert 0.25 < below < 0.5
            assert P.row_scale_pow2(below) == 2 * P.row_scale_pow2(F32(0.5))           # the scale changes between the two rows
            row = np.abs(x[r["far_below_max"]]).astype(np.float64)
            assert 2.0 ** -32 < row[9] / row.max() < 2.0 ** -30
        assert np.nextafter(F32(0.5), F32(0)) == np.abs(w[r["below_pow2_max"]]).max()


# ---------------------------------------------------------------------------------------------- the restatement's own properties
@pytest.mark.parametrize("bf16_only", [False, True])
def test_model_planes_reproduce_the_values(bf16_only):
    cfg = M.config(tied=True, bias=True)
    t = M.tensors(cfg, bf16_only=bf16_only)
    d = M.dims(cfg)
    for planes in (2, 3, 16):
        ex = M.expected(cfg, t, planes, finalized=False)
        for i in range(d["layers"]):
            w = t[f"model.layers.{i}.mlp.down_proj.weight"].astype(np.float64)
            K = w.shape[1]
            pl = ex[(i, M.DOWN, M.K_PLANES)]
            ordinary = np.abs(w) < 3e38
            ordinary &= ordinary.all(axis=1, keepdims=True)                          # fp16 planes: a saturating value takes its row's scale
            if planes == 16:
                inv = ex[(i, M.DOWN, M.K_W_INV)].astype(np.float64)
                assert P.is_pow2(inv).all()
                assert pl.shape == (w.shape[0], 3 * K) and np.array_equal(pl[:, :K], pl[:, 2 * K:])
                with np.errstate(invalid="ignore", over="ignore"):
                    val = (_f16(pl[:, :K]).astype(np.float64) + _f16(pl[:, K:2 * K]).astype(np.float64)) * inv
                    floor = 2.0 ** -25 * inv                                            # (S) of fp32_plane_cases: max(2^-22 |w sc|, 2^-25) / sc
                    ok = np.abs(val - w) <= np.maximum(2.0 ** -22 * np.abs(w), floor)
                assert ok[ordinary].all()
                mx = np.abs(w).max(axis=1)
                live = (mx > 0) & (mx < 3e38)
                scaled = mx[live] / inv[live, 0]
                assert ((scaled >= 2.0 ** 14) & (scaled < 2.0 ** 15)).all()
                assert (inv[~live] == 1).all()
            else:
                order = M.SPLIT_ORDER[planes]
                assert pl.shape == (w.shape[0], len(order) * K)
                segs = [G.bf16_value(pl[:, s * K:(s + 1) * K]).astype(np.float64) for s in range(len(order))]
                for a in range(len(order)):
                    for b in range(a + 1, len(order)):
                        if order[a] == order[b]:
                            assert np.array_equal(segs[a], segs[b])
                first = {p: order.index(p) for p in set(order)}
                total = sum(segs[first[p]] for p in sorted(first))
                if planes == 3:                                                      # exact down to 2^-110 (common.h split_bf16x3)
                    big = np.abs(w) >= 2.0 ** -110
                    assert np.array_equal(total[big], w[big]) and (np.abs(total - w)[~big] <= 2.0 ** -134).all()
                else:
                    assert (np.abs(total - w) <= np.maximum(2.0 ** -16 * np.abs(w), 2.0 ** -134)).all()
            # the bf16 layout: the nearest bf16 number
            words = ex[(i, M.DOWN, M.K_BF16)]
            with np.errstate(invalid="ignore", over="ignore"):
                err = np.abs(G.bf16_value(words).astype(np.float64) - w)
            assert (err[ordinary] <= G.half_spacing(w)[ordinary]).all()


def test_no_bf16_number_has_a_low_fp16_plane():
    """Every finite bf16 magnitude below 2^15 (a row's scaled maximum lies under it), as the scaled value itself: g1 is zero.  So
    bf16-valued weights always re-pack to 2 segments, the element 2^-31 below a row's maximum included."""
    v = G.bf16_value(np.arange(0, 0x7F80, dtype=np.uint16))
    v = v[v < 2.0 ** 15]
    g0, g1 = P.split_f16x2(v)
    assert len(v) > 18000 and not (g1.view(np.uint16) & np.uint16(0x7FFF)).any()
    lost = g0.astype(np.float64) != v.astype(np.float64)
    assert lost.any() and (np.abs(g0.astype(np.float64) - v)[lost] <= 2.0 ** -25).all()      # below fp16's normal range g0 loses bits
    cfg = M.config(tied=False, bias=False)
    tb = M.tensors(cfg, bf16_only=True)
    assert M.expected_segments(cfg, tb, 16) == [2] * 9
    assert M.expected_segments(cfg, M.tensors(cfg), 16) == [3] * 9
    # one entry with more significand bits than g0 holds: its matrix alone keeps [g0 | g1 | g0]
    name = "model.layers.1.mlp.down_proj.weight"
    w = tb[name].copy()
    w[7, 100] *= F32(1 + 2.0 ** -20)
    want = [2] * 9
    want[4 * 1 + 3] = 3
    assert M.expected_segments(cfg, dict(tb, **{name: w}), 16) == want
    assert M.expected_segments(cfg, tb, 3) == [6] * 9 and M.expected_segments(cfg, tb, 2) == [3] * 9
    assert M.expected_segments(cfg, tb, 0) == [0] * 9


def test_row_maps_and_tied_head():
    cfg = M.config(tied=True, bias=False)
    t = M.tensors(cfg)
    d = M.dims(cfg)
    ex = M.expected(cfg, t, 0)
    rows = np.concatenate([M.gate_row(np.arange(d["I"])), M.up_row(np.arange(d["I"]))])
    assert np.array_equal(np.sort(rows), np.arange(2 * d["I"]))               # a permutation of the 2 I rows
    with np.errstate(over="ignore"):
        gu = G.bf16_bits(G.bf16_round(P.interleave_gate_up(t["model.layers.1.mlp.gate_proj.weight"], t["model.layers.1.mlp.up_proj.weight"])))
    assert np.array_equal(ex[(1, M.GATE_UP, M.K_BF16)], gu)
    qkv = ex[(0, M.QKV, M.K_BF16)]
    with np.errstate(over="ignore"):
        for name, base, n in (("q", 0, d["nq"]), ("k", d["nq"], d["nkv"]), ("v", d["nq"] + d["nkv"], d["nkv"])):
            assert np.array_equal(qkv[base:base + n], G.bf16_bits(G.bf16_round(t[f"model.layers.0.self_attn.{name}_proj.weight"])))
        assert np.array_equal(ex[(-1, M.LM_HEAD, M.K_BF16)], G.bf16_bits(G.bf16_round(t["model.embed_tokens.weight"])))
    assert np.array_equal(ex[(-1, M.EMBED, M.K_F32)].view(np.uint32), t["model.embed_tokens.weight"].view(np.uint32))
    assert "lm_head.weight" not in t


# ---------------------------------------------------------------------------------------------- the checker sees every defect
@pytest.mark.parametrize("planes", M.PLANE_MODES)
def test_checker_passes_the_model_itself(model_bias, planes):
    cfg, t = model_bias
    for fin in (False, True):
        a, b = M.expected(cfg, t, planes, fin), M.expected(cfg, t, planes, fin)
        assert M.mismatches(planes, a, b) == []
        n_matrix = 4 * 2 + 1
        assert len(a) == 2 + n_matrix * {0: 1, 2: 2, 3: 2, 16: 3}[planes] + 2 * 2 + 2 * 2
    missing = dict(a)
    del missing[(1, M.LN2, M.K_F32)]
    assert M.mismatches(planes, missing, a) == ["layer 1 ln2 f32"]


@pytest.mark.parametrize("defect", sorted(M.DEFECTS))
def test_checker_sees_each_defect(model_bias, defect):
    cfg, t = model_bias
    hit = {"truncation": ("bf16", "planes"),"gate_up_swapped": ("gate_up",), "qkv_bases_rolled": ("qkv",), "segments_permuted": ("planes",),
           "w_inv_off_by_2": ("w_inv",), "low_plane_dropped": ("planes",), "bias_rounding_missing": ("bias bf16_as_f32",)}[defect]
    for planes in M.PLANE_MODES:
        want = M.expected(cfg, t, planes, finalized=False)
        got = M.expected(cfg, t, planes, finalized=False, defect=defect)
        bad = M.mismatches(planes, got, want)
        if planes in M.DEFECTS[defect]:
            assert bad and all(any(h in line for h in hit) for line in bad), (defect, planes, bad)
            if defect in ("gate_up_swapped", "qkv_bases_rolled"):
                assert len(bad) == 2 * {0: 1, 2: 2, 3: 2, 16: 3}[planes]       # every form of that matrix, both layers
        else:
            assert bad == [], (defect, planes, bad)


def test_checker_sees_round_half_up_and_a_zero_sign_only_where_it_counts(model_bias):
    cfg, t = model_bias
    want = M.expected(cfg, t, 16, finalized=False)
    # round half up instead of ties to even: only the halfway values with an even word below them move
    name = "model.layers.0.self_attn.o_proj.weight"
    w = t[name]
    up = ((w.view(np.uint32) + np.uint32(0x8000)) >> np.uint32(16)).astype(np.uint16)
    got = dict(want)
    got[(0, M.O, M.K_BF16)] = up
    bad = M.mismatches(16, got, want)
    assert len(bad) == 1 and "layer 0 o bf16" in bad[0] and "row 1 " in bad[0]
    diff = up != want[(0, M.O, M.K_BF16)]
    ties = [M.SPECIAL_ROWS["halfway"], M.SPECIAL_ROWS["zeros_subnormals"]]      # the second: the tie between bf16's subnormals 0 and 1
    assert diff[ties[0]].sum() >= 8 and diff[ties[1]].sum() == 1 and diff.sum() == diff[ties].sum()
    # the sign of a zero fp16 plane element is free, the sign of a bf16 zero is not
    flip = lambda a: np.where((a & np.uint16(0x7FFF)) == 0, a ^ np.uint16(0x8000), a)
    got = dict(want)
    got[(0, M.O, M.K_PLANES)] = flip(want[(0, M.O, M.K_PLANES)])
    assert M.mismatches(16, got, want) == []
    got[(0, M.O, M.K_BF16)] = flip(want[(0, M.O, M.K_BF16)])
    assert len(M.mismatches(16, got, want)) == 1


# ---------------------------------------------------------------------------------------------- LoRA bound, RoPE restatement
def test_lora_bound_holds_for_an_fp32_chain_and_sees_a_dropped_term():
    for r, in_f, out_f, scale in ((1, 255, 3, 2.0), (8, 257, 300, -0.25), (64, 256, 3, 0.5)):
        W, A, B = M.lora_case(r, in_f, out_f, scale)
        truth, bound = M.lora_truth(W, A, B, scale), M.lora_bound(W, A, B, scale)
        assert np.abs(truth).max() < 2.0 ** -8 * np.abs(W).max()                   # W nearly cancels the update
        acc = np.zeros((out_f, in_f), F32)
        for k in range(r):
            acc = (acc + (B[:, k:k + 1] * A[k:k + 1, :]).astype(F32)).astype(F32)
        chain = (W + (F32(scale) * acc).astype(F32)).astype(F32)
        assert (np.abs(chain - truth) <= bound).all()
        if r > 1:
            short = (W + (F32(scale) * (acc - (B[:, -1:] * A[-1:, :]).astype(F32))).astype(F32)).astype(F32)
            assert (np.abs(short - truth) > bound).mean() > 0.9


def test_rope_restatement_equals_the_oracle_formula():
    """model_load_cases.rope_inv_freq (element by element, as rope_tables) and oracle.llama_bi.rope_inv_freq (vectorised) are the same
    formula: double arithmetic, one rounding."""
    from oracle import llama_bi as LB
    for name, s in M.ROPE_SETS.items():
        inv = M.rope_inv_freq(s["head_dim"], s["rope_theta"], s["rope_scaling"])
        cfg = dict(num_attention_heads=1, hidden_size=s["head_dim"], head_dim=s["head_dim"], rope_theta=s["rope_theta"],
                   rope_scaling=s["rope_scaling"])
        assert M.ulps_apart(inv, LB.rope_inv_freq(cfg)).max() <= 1, name
        cos, sin = M.rope_tables(inv, M.ROPE_POSITIONS)
        assert cos.shape == (len(M.ROPE_POSITIONS), s["head_dim"] // 2) and (cos[0] == 1).all() and (sin[0] == 0).all()
        assert np.allclose(cos.astype(np.float64) ** 2 + sin.astype(np.float64) ** 2, 1, atol=2.0 ** -22, rtol=0)


# ---------------------------------------------------------------------------------------------- the loader's file routes
def _state(cfg, dtype):
    tb = M.tensors(cfg, bf16_only=True)
    if dtype == torch.float16:                 # fp16 holds fewer exponents: keep what it represents exactly
        tb = {k: torch.from_numpy(v.copy()).to(torch.float16).float().numpy() for k, v in tb.items()}
    return {k: torch.from_numpy(v.copy()).to(dtype) for k, v in tb.items()}


def _assert_same(got, want):
    assert set(got) == set(want)
    for k, v in want.items():
        g = got[k]
        assert g.dtype == v.dtype and tuple(g.shape) == tuple(v.shape), k
        bits = torch.int16 if v.element_size() == 2 else torch.int32
        assert torch.equal(g.contiguous().view(bits), v.contiguous().view(bits)), k


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_read_checkpoint_single_safetensors(tmp_path, dtype):
    from safetensors.torch import save_file
    from scaling_retriever_amd.modeling.llm_encoder import _read_checkpoint
    sd = _state(M.config(tied=False, bias=True), dtype)
    save_file(sd, str(tmp_path / "model.safetensors"))
    _assert_same(_read_checkpoint(str(tmp_path)), sd)


def test_read_checkpoint_sharded_bin_bare_inv_freq_and_tied(tmp_path):
    from safetensors.torch import save_file
    from scaling_retriever_amd.modeling.llm_encoder import _read_checkpoint
    sd = _state(M.config(tied=False, bias=True), torch.bfloat16)
    # a sharded pair: layer 1 and the head in the second file; a stale single file beside the index must not be read
    d = tmp_path / "sharded"
    os.makedirs(d)
    second = {k: v for k, v in sd.items() if ".layers.1." in k or k.startswith("lm_head")}
    first = {k: v for k, v in sd.items() if k not in second}
    save_file(first, str(d / "model-00001-of-00002.safetensors"))
    save_file(second, str(d / "model-00002-of-00002.safetensors"))
    wm = {k: "model-00001-of-00002.safetensors" for k in first}
    wm.update({k: "model-00002-of-00002.safetensors" for k in second})
    json.dump({"metadata": {}, "weight_map": wm}, open(d / "model.safetensors.index.json", "w"))
    save_file({"model.norm.weight": torch.zeros(3)}, str(d / "model.safetensors"))
    _assert_same(_read_checkpoint(str(d)), sd)
    # pytorch_model.bin
    d = tmp_path / "bin"
    os.makedirs(d)
    torch.save(sd, str(d / "pytorch_model.bin"))
    _assert_same(_read_checkpoint(str(d)), sd)
    # bare names (a LlamaModel checkpoint): no `model.` prefix, no head
    d = tmp_path / "bare"
    os.makedirs(d)
    bare = {k[len("model."):]: v for k, v in sd.items() if k.startswith("model.")}
    save_file(bare, str(d / "model.safetensors"))
    _assert_same(_read_checkpoint(str(d)), {k: v for k, v in sd.items() if k.startswith("model.")})
    # an extra rotary_emb.inv_freq key comes back under its name (build_engine skips it)
    d = tmp_path / "inv_freq"
    os.makedirs(d)
    extra = dict(sd)
    extra["model.layers.0.self_attn.rotary_emb.inv_freq"] = torch.arange(32, dtype=torch.float32)
    save_file(extra, str(d / "model.safetensors"))
    _assert_same(_read_checkpoint(str(d)), extra)
    # a tied checkpoint has no lm_head.weight
    d = tmp_path / "tied"
    os.makedirs(d)
    tied = _state(M.config(tied=True, bias=False), torch.bfloat16)
    assert "lm_head.weight" not in tied
    save_file(tied, str(d / "model.safetensors"))
    _assert_same(_read_checkpoint(str(d)), tied)
    with pytest.raises(FileNotFoundError):
        _read_checkpoint(str(tmp_path))


def test_readout_constants_match_the_header():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sr_hip.h")).read()
    defined = {k: int(v) for k, v in re.findall(r"#define SR_READOUT_([A-Z0-9_]+) (\d+)", src)}
    buffers = dict(EMBED=M.EMBED, LM_HEAD=M.LM_HEAD, NORM=M.NORM, ROPE_COS=M.ROPE_COS, ROPE_SIN=M.ROPE_SIN, QKV=M.QKV, O=M.O,
                   GATE_UP=M.GATE_UP, DOWN=M.DOWN, LN1=M.LN1, LN2=M.LN2, BIAS=M.BIAS)
    kinds = dict(F32=M.K_F32, BF16=M.K_BF16, PLANES=M.K_PLANES, W_INV=M.K_W_INV, BF16_AS_F32=M.K_BF16_AS_F32)
    assert defined == {**buffers, **kinds}
