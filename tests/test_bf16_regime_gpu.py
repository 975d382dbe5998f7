"""GPU: what the bf16 regime (fp32_planes = 0: store_embs, corpus encode, both heads) launches besides the attention, kernel by kernel
and element by element against float64 with the derived bounds of tests/bf16_regime_cases.py (test_bf16_regime_host.py shows on the
CPU that ideally rounded arithmetic is inside every bound and that the defects these tests are there for are outside).  Test hooks:
sr_rmsnorm_bf16, sr_dense_head_pool, sr_sparse_finish, sr_encode_plan (include/sr_hip.h, "building blocks"); the GEMM needs none:
sr_gemm_bf16 (epilogues 0 - 4) and sr_gemm_qkv_rope_bias (fp32_out 0 / 1) reach every bf16-operand epilogue.  No element and no case
is exempt; every output buffer is pre-filled with NaN and carries guard rows behind it that must come back untouched.

RMSNorm (launch_rmsnorm, csrc/encoder_kernels.hip):

  kernel               H       reached by
  rmsnorm_kernel<0>    64 320  test_rmsnorm[64] [320]: H % 256 != 0, second pass re-reads the row
  rmsnorm_kernel<1>    256     test_rmsnorm[256]
  rmsnorm_kernel<2>    512     test_rmsnorm[512]
  rmsnorm_kernel<4>    1024    test_rmsnorm[1024]
  rmsnorm_kernel<8>    2048    test_rmsnorm[2048]
  rmsnorm_kernel<12>   3072    test_rmsnorm[3072]
  rmsnorm_kernel<16>   4096    test_rmsnorm[4096]
  each with T = 1 3 4 5 9 (a workgroup holds four rows) and the argument combinations of the encoder's call sites: gather + norm
  (first layer), delta + norm (layers), delta only (w == NULL: "residual add only"), norm alone (sparse head), norm to fp32
  (sr_model_last_hidden), + gather and delta together with both outputs.  Rows: mean(x^2) comparable with eps, all zero, delta
  cancelling x to a few ulps, token ids out of order.  The row left in x is compared bit for bit.

GEMM (launch_gemm_bf16, csrc/gemm_bf16.hip) - every epilogue x every route below; M = 1 17 33 65 200 300, N = 128 320 (ragged
against both tile widths; QKV at head_dim 128: 256 384), K = 192 256 320 768 (3 4 5 12 k-steps) + K = 2048 at M 65, N 128:

  tile configuration (launch_cfg)              switches                                 reached by
  64 x 16 / 32 / 64, one wave, 4 stages        default                                  M = 1 / 17 / 33, K >= 256 (QKV head_dim 128: 128 features
                                                                                        wide, 4 / 4 / 3 stages)
  128 x 64, 4 waves, 3 stages                  default = SR_GEMM_TILE=128               M = 65 200 300, K >= 256
  128 x 64, 4 waves, not pipelined             default = SR_GEMM_TILE=128               M = 65 200 300, K = 192
  128 x 128, 2 x 2 waves, pipelined            SR_GEMM_SKINNY=0 [+ SR_GEMM_TILE=128]    M = 1 17 33, K >= 256; the 44-row tail of split:256
  128 x 128, 2 x 2 waves, not pipelined        default                                  M = 1 17 33, K = 192
  128 x 128, 1 x 4 waves                       default = SR_GEMM_TILE=128               QKV at head_dim 128, whenever no single-wave tile takes it
  256 x 256 four-wave, staged epilogue         SR_GEMM_TILE=256 (SR_GEMM_BIG unset)     epilogues 0 1 2 4 and QKV bf16 with n_rope % 128 == 0,
                                                                                        K >= 256 (+ SR_GEMM_SKINNY=0 below 65 rows)
  256 x 256 eight-wave, pipelined              SR_GEMM_TILE=256 + SR_GEMM_BIG=8w;       every epilogue, K >= 256; the silent fall-back of QKV bf16
                                               SR_GEMM_TILE=256 alone                   with n_rope % 128 != 0, epilogue 3 and QKV fp32
  256 x 256 eight-wave, not pipelined          SR_GEMM_TILE=256                         K = 192
  256 x 256 head + 128 x 128 tail (rows_from)  SR_GEMM_TILE=split:256 [+ BIG=8w]        M = 300: positions, sequence ids, C rows of the tail
  token-tile-fastest order                     SR_GEMM_MFAST=1 [+ SR_GEMM_TILE=256]     once per epilogue: M 300, N 320 (QKV: its last variant), K 768
  plain (not per-XCD) tile order               SR_GEMM_XCD=0 [+ SR_GEMM_TILE=256]       the same case

  epilogue                      what the case brings
  0 store bf16                  the bf16 store's half-spacing term on its own
  1 residual fp32               C pre-filled, the product added exactly once
  2 SwiGLU bf16                 |g| up to 100 of both signs (__expf(-g) overflows, v_rcp_f32 flushes)
  3 per-sequence max            a sequence of 1 next to one of 200, borders inside tiles and wave slabs, -2 rows with the largest values, an
                                all-negative column, a sequence without a row
  4 store fp32                  the MFMA chain on its own
  5 / 6 QKV + bias + RoPE       bf16 / fp32 output; head_dim 64 / 128, with / without bias, shuffled positions, n_rope a multiple of 128
                                and not, v features behind the rotated ones

All routes of a case are bit-identical to the first.

Heads and plan: dense_head_stats_kernel + dense_head_pool_kernel at H = 64 320 2048, B = 1 3, sequences of 0 1 2 70 tokens, pool_start
at / inside / beyond the span and shifted (test_dense_head); sparse_finish_kernel at n = 1 255 257 1000 with and without the bf16
rounding (test_sparse_finish); plan_rows_kernel + plan_scan_kernel + plan_tokens_kernel at L = 1 63 64 65 130, B = 1 5 257, every
mask kind x mode x row_shift, bit for bit (test_plan).

SwiGLU fast path.  The derived term rel_s = ((2 |g| + 2) sg + 4) e of bf16_regime_cases.py (argument rounding, 1 ulp each for
v_exp_f32 and v_rcp_f32, one rounding each for the sum and the product, flush-to-zero floor 2^-119) HOLDS on MI355X and is asserted
as derived, nothing widened: test_epilogue[swiglu-*] inside the whole epilogue, test_swiglu_fast_path_term on the sub-expression
silu(g) alone (u = 1 and g exact, 256 gates over [-100, 100]), where the kernel reaches 0.995 of h + rel_s |s| - the bf16 store's
half spacing h is all that is visible; a silu off by 2^-10, the issue's example, is outside.

Measured on MI355X, worst error as a fraction of its bound (information, not asserted; the bf16 outputs sit at the half spacing of
(B), which correct rounding reaches, exactly as the ideal arithmetic of test_bf16_regime_host.py does):
  rmsnorm_kernel<0> 0.999 (H 64) 0.997 (H 320)   <1> 0.998   <2> 0.996   <4> 0.992   <8> 0.984   <12> 0.977   <16> 0.969
  GEMM epilogue 0 store bf16 0.988   1 residual 0.719   2 SwiGLU 0.970   3 per-sequence max 0.006   4 store fp32 0.011
                5 QKV bf16 0.999   6 QKV fp32 0.114          (every other route: the bits of the first)
  dense head 0.026 (H 64) 0.006 (H 320) 0.001 (H 2048)       plan: bit-exact, 360 calls
  sparse finish 0.999 (an element whose 1 + m rounds to 1: the e of the sum).  With logf the kernel was OUTSIDE: 1.13 of the bound at
  n = 257 (x = 371.879: hipcc's logf = v_log_f32 x ln 2 was 1.99 ulps off log x, the HIP math API documents 1); sparse_finish_kernel
  now takes the logarithm in double and rounds once.
This file: 59 tests, 4.3 s on one MI355X."""
import itertools

import numpy as np
import pytest
import torch

import bf16_regime_cases as C

pytestmark = [pytest.mark.gpu]

SWITCHES = ("SR_GEMM_TILE", "SR_GEMM_BIG", "SR_GEMM_SKINNY", "SR_GEMM_MFAST", "SR_GEMM_XCD")
BF16_NAN = 0x7fc0
GUARD_ROWS = 2


def _lib():
    from scaling_retriever_amd import _lib as L
    return L, L.load()


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _bf16_dev(values):
    """fp32 holding bf16 numbers -> device int16 words."""
    return _dev(C.bf16_bits(values).view(np.int16))


def _nan_bf16(rows, cols):
    return torch.full((rows, cols), BF16_NAN, dtype=torch.int16, device="cuda")


def _bf16_host(t):
    return t.cpu().numpy().view(np.uint16)


def _untouched_bf16(t, what):
    assert np.all(_bf16_host(t) == BF16_NAN), what + ": guard rows of a bf16 output were written"


def _untouched_f32(t, what, fill=None):
    a = t.cpu().numpy()
    assert np.all(np.isnan(a)) if fill is None else np.all(a == fill), what + ": guard rows of an fp32 output were written"


# ------------------------------------------------------------------------------------------ RMSNorm
def run_norm(c, combo):
    """sr_rmsnorm_bf16 on a case under an argument combination -> (x after the call, xn as fp32 values or None, xn_f32 or None)."""
    L, lib = _lib()
    k = C.NORM_COMBOS[combo]
    T, H = c["T"], c["H"]
    x0 = np.full((T + GUARD_ROWS, H), 7.0, np.float32)                   # a gather overwrites whatever x held
    if not k["gather"]:
        x0[:T] = c["x"]
    d_x = _dev(x0)
    d_e, d_t = (_dev(c["embed"]), _dev(c["tok"])) if k["gather"] else (None, None)
    d_d = _bf16_dev(c["delta"]) if k["delta"] else None
    d_w = _dev(c["w"]) if k["w"] else None
    xn = _nan_bf16(T + GUARD_ROWS, H)
    xf = torch.full((T + GUARD_ROWS, H), float("nan"), device="cuda")
    L.check(lib.sr_rmsnorm_bf16(d_x.data_ptr(), _ptr(d_e), _ptr(d_t), _ptr(d_d), _ptr(d_w), xn.data_ptr() if k["xn"] else None,
                                xf.data_ptr() if k["f32"] else None, c["eps"], T, H, L.stream_ptr()), "sr_rmsnorm_bf16")
    torch.cuda.synchronize()
    what = f"H {H} T {T} {combo}"
    assert np.all(d_x[T:].cpu().numpy() == 7.0), what + ": rows behind x were written"
    _untouched_bf16(xn[T if k["xn"] else 0:], what)
    _untouched_f32(xf[T if k["f32"] else 0:], what)
    return (d_x[:T].cpu().numpy(), C.bf16_value(_bf16_host(xn[:T])) if k["xn"] else None, xf[:T].cpu().numpy() if k["f32"] else None)


@pytest.mark.parametrize("H", C.NORM_H)
def test_rmsnorm(H):
    worst = 0.0
    for T, combo in itertools.product(C.NORM_T, C.NORM_COMBOS):
        c = C.norm_case(H, T)
        x_after, xn, xf = run_norm(c, combo)
        assert C.check_norm(c, combo, x_after, xn=xn, xn_f32=xf) == [], f"H {H} (rmsnorm_kernel<{C.NORM_NCH[H]}>) T {T} {combo}"
        worst = max(worst, C.norm_ratio(c, combo, xn=xn, xn_f32=xf))
    print(f"rmsnorm H {H}: worst error {worst:.3f} of the bound")


# ------------------------------------------------------------------------------------------ GEMM epilogues
def routes(c):
    """[(name, {switch: value})] for a case: see the table in the module docstring."""
    epi, M, steps = c["epi"], c["M"], c["K"] // 64
    big = [("", {}), ("+8w", {"SR_GEMM_BIG": "8w"})] if epi in C.STAGED_4W else [("", {})]
    tiles = [("tile128", {"SR_GEMM_TILE": "128"})] + [("tile256" + n, dict(e, SR_GEMM_TILE="256")) for n, e in big]
    out = [("default", {})]
    if M <= 64 and steps >= 4:            # the single-wave tiles take these rows first: switch them off to reach the others
        out += [("skinny0", {"SR_GEMM_SKINNY": "0"})] + [(n + ",skinny0", dict(e, SR_GEMM_SKINNY="0")) for n, e in tiles]
    else:
        out += tiles
    if M > 256:
        out += [("split256" + n, dict(e, SR_GEMM_TILE="split:256")) for n, e in big]
    if M == 300 and c["K"] == 768 and c["N"] in (320, 384):
        for n, e in [("mfast", {"SR_GEMM_MFAST": "1"}), ("xcd0", {"SR_GEMM_XCD": "0"})]:
            out += [(n, e), ("tile256," + n, dict(e, SR_GEMM_TILE="256"))]
    return out


def run_gemm(c, env, monkeypatch, dev):
    """The case under the given switches -> the output as fp32 values (bf16 outputs decoded).  dev: the case's device arrays, filled once."""
    L, lib = _lib()
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if not dev:
        dev.update(A=_bf16_dev(c["A"]), W=_bf16_dev(c["W"]))
        for k in ("pos", "cos", "sin", "bias", "seq_of"):
            dev[k] = _dev(c.get(k))
    epi, M, N, K = c["epi"], c["M"], c["N"], c["K"]
    rows, cols = C.out_shape(c)
    if epi in C.BF16_OUT:
        out = _nan_bf16(rows + GUARD_ROWS, cols)
    elif epi == C.EPI_SEGMAX:
        out = torch.zeros((rows + GUARD_ROWS, cols), device="cuda")
        out[rows:] = -1.0                          # an integer atomicMax of anything positive would replace it
    else:
        out = torch.full((rows + GUARD_ROWS, cols), float("nan"), device="cuda")
        if epi == C.EPI_RESID:
            out[:rows] = _dev(c["C0"])
    if epi in (C.EPI_QKV, C.EPI_QKV_F32):
        L.check(lib.sr_gemm_qkv_rope_bias(dev["A"].data_ptr(), dev["W"].data_ptr(), M, N, K, out.data_ptr(), dev["pos"].data_ptr(),
                                          dev["cos"].data_ptr(), dev["sin"].data_ptr(), c["n_rope"], c["hd"], _ptr(dev["bias"]),
                                          1 if epi == C.EPI_QKV_F32 else 0, L.stream_ptr()), "sr_gemm_qkv_rope_bias")
    else:
        L.check(lib.sr_gemm_bf16(dev["A"].data_ptr(), dev["W"].data_ptr(), M, N, K, epi, out.data_ptr(), _ptr(dev["seq_of"]), L.stream_ptr()),
                "sr_gemm_bf16")
    torch.cuda.synchronize()
    for k in env:
        monkeypatch.delenv(k, raising=False)
    what = f"epilogue {epi} M {M} N {N} K {K} {env}"
    if epi in C.BF16_OUT:
        _untouched_bf16(out[rows:], what)
        return C.bf16_value(_bf16_host(out[:rows]))
    _untouched_f32(out[rows:], what, fill=-1.0 if epi == C.EPI_SEGMAX else None)
    return out[:rows].cpu().numpy()


@pytest.mark.parametrize("M", C.GEMM_M)
@pytest.mark.parametrize("name", list(C.EPILOGUES))
def test_epilogue(name, M, monkeypatch):
    """Every case of the epilogue at this M: the default route element-wise against the bound, every other route bit-identical."""
    worst, n_routes = 0.0, 0
    for c in C.epilogue_cases(C.EPILOGUES[name], Ms=[M]):
        what = {k: c[k] for k in ("epi", "M", "N", "K", "hd", "n_rope") if k in c}
        what["bias"] = c.get("bias") is not None
        dev, first = {}, None
        for rname, env in routes(c):
            out = run_gemm(c, env, monkeypatch, dev)
            if first is None:
                first = out
                assert C.check_gemm(c, out) == [], (what, rname)
                worst = max(worst, C.worst_ratio(c, out))
            else:
                assert np.array_equal(out.view(np.uint32), first.view(np.uint32)), (what, f"route {rname} != default")
            n_routes += 1
    print(f"{name} M {M}: {n_routes} launches, worst error {worst:.3f} of the bound")


def test_swiglu_fast_path_term(monkeypatch):
    """The sub-expression silu(g) = g rcp(1 + __expf(-g)) on its own, through epilogue 2 with u = 1 exactly: gate rows g e_0 against
    activations e_0 (one nonzero product per chain, so t~ = g exactly and u = 1 exactly), output bf16(silu~(g)).  Asserted: (B) with
    dy = rel_s |s| + 2^-119, the derived term.  Reported: the worst error as a fraction of that bound.  The bf16 store hides the fast
    path's few e under its 2^-9: what this pins is that the fast path is not off by more than the derived term PLUS half a bf16
    spacing - 2^-10 off, the issue's example, is outside."""
    K, I = 192, 256
    g = C.bf16_round(np.concatenate([np.linspace(-100, 100, I - 6), [-88.5, -87.5, -87.0, 88.0, 0.0, -0.0]]).astype(np.float32))
    wg = np.zeros((I, K), np.float32); wg[:, 0] = g                        # noqa: E702
    wu = np.zeros((I, K), np.float32); wu[:, 0] = 1.0                      # noqa: E702
    A = np.zeros((17, K), np.float32); A[:, 0] = 1.0                       # noqa: E702
    c = dict(epi=C.EPI_SWIGLU, M=17, N=2 * I, K=K, A=A, W=C.P.interleave_gate_up(wg, wu))
    out = run_gemm(c, {}, monkeypatch, {})
    s = C.P._silu(g.astype(np.float64))
    with np.errstate(over="ignore"):
        rel = ((2 * np.abs(g) + 2) / (1 + np.exp(g.astype(np.float64))) + 4) * C.E
    bound = C.store_bound(s, rel * np.abs(s) + 2.0 ** -119)
    assert np.all(np.abs(out - s[None, :]) <= bound[None, :]), np.abs(out - s[None, :]).max(axis=0) / bound
    assert np.array_equal(out, np.repeat(out[:1], 17, axis=0))              # every row computes the same
    off = C.bf16_round((s * (1 + 2.0 ** -10)).astype(np.float32))           # the issue's example defect is outside on some element
    assert not np.all(np.abs(off - s) <= bound)
    print(f"silu fast path: worst error {C.ratio(out[0], s, bound):.3f} of (B) with the derived term")


# ------------------------------------------------------------------------------------------ dense head
@pytest.mark.parametrize("H", C.HEAD_H)
def test_dense_head(H):
    L, lib = _lib()
    worst = 0.0
    for layout in C.HEAD_LAYOUTS:
        c = C.head_case(H, layout)
        B, T = c["B"], c["T"]
        d_x = _dev(c["x"]) if T else torch.zeros((1, H), device="cuda")
        d_w, d_cu, d_ps = _dev(c["w"]), _dev(c["cu"]), _dev(c["pool_start"])
        d_pos = _dev(c["pos"]) if T else torch.zeros((1,), dtype=torch.int32, device="cuda")
        stats = torch.full((max(T, 1), 2), float("nan"), device="cuda")
        out = torch.full((B + GUARD_ROWS, H), float("nan"), device="cuda")
        L.check(lib.sr_dense_head_pool(d_x.data_ptr(), d_w.data_ptr(), d_cu.data_ptr(), d_pos.data_ptr(), d_ps.data_ptr(), c["eps"], B, T, H,
                                       stats.data_ptr(), out.data_ptr(), L.stream_ptr()), "sr_dense_head_pool")
        torch.cuda.synchronize()
        _untouched_f32(out[B:], f"H {H} {layout}")
        got = out[:B].cpu().numpy()
        assert C.check_head(c, got) == [], f"H {H} layout {layout}"
        ref, bound, _ = C.head_reference(c)
        worst = max(worst, C.ratio(got, ref, bound))
    print(f"dense head H {H}: worst error {worst:.3f} of the bound")


# ------------------------------------------------------------------------------------------ sparse finish
def test_sparse_finish():
    L, lib = _lib()
    worst = 0.0
    for n, rb in itertools.product(C.FINISH_N, (0, 1)):
        c = C.finish_case(n)
        buf = torch.full((n + 300,), float("nan"), device="cuda")
        buf[:n] = _dev(c["v"])
        L.check(lib.sr_sparse_finish(buf.data_ptr(), n, float(c["scale"]), rb, L.stream_ptr()), "sr_sparse_finish")
        torch.cuda.synchronize()
        _untouched_f32(buf[n:], f"n {n}")
        got = buf[:n].cpu().numpy()
        assert C.check_finish(c, rb, got) == [], f"n {n} round_bf16 {rb}"
        ref, bound, _ = C.finish_reference(c, rb)
        worst = max(worst, C.ratio(got, ref, bound))
    print(f"sparse finish: worst error {worst:.3f} of the bound")


# ------------------------------------------------------------------------------------------ plan
PLAN_FILL = -77


def run_plan(c, mode, capacity):
    """sr_encode_plan -> (status, {array name: numpy}, n_tokens); every array starts as PLAN_FILL (key_valid: 0xb3)."""
    import ctypes
    L, lib = _lib()
    B, cap = c["B"], capacity
    i32 = lambda n: torch.full((max(n, 1),), PLAN_FILL, dtype=torch.int32, device="cuda")      # noqa: E731
    a = dict(span_start=i32(B), span_len=i32(B), pool_start=i32(B), row_len=i32(B), cu=i32(B + 1), tok_id=i32(cap), pos=i32(cap),
             key_valid=torch.full((max(cap, 1),), 0xb3, dtype=torch.uint8, device="cuda"), seq_of=i32(cap))
    d_ids, d_mask, d_rs = _dev(c["ids"]), _dev(c["mask"]), _dev(c["row_shift"])
    n = ctypes.c_int64(-1)
    rc = lib.sr_encode_plan(d_ids.data_ptr(), d_mask.data_ptr(), B, c["L"], mode, c["vocab"], _ptr(d_rs), a["span_start"].data_ptr(),
                            a["span_len"].data_ptr(), a["pool_start"].data_ptr(), a["row_len"].data_ptr(), a["cu"].data_ptr(),
                            a["tok_id"].data_ptr(), a["pos"].data_ptr(), a["key_valid"].data_ptr(), a["seq_of"].data_ptr(), cap,
                            ctypes.byref(n), L.stream_ptr())
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in a.items()}, n.value


@pytest.mark.parametrize("B", C.PLAN_B)
def test_plan(B):
    L, lib = _lib()
    n_calls = 0
    for Lq, kind, shift, mode in itertools.product(C.PLAN_L, C.PLAN_KINDS, (False, True), (0, 1, 2)):
        c = C.plan_case(B, Lq, kind, shift)
        ref = C.plan_reference(c, mode)
        T = int(ref["cu"][-1])
        rc, got, n = run_plan(c, mode, T + 8)
        what = f"B {B} L {Lq} {kind} row_shift {shift} mode {mode}"
        assert rc == L.SR_OK, (what, lib.sr_last_error())
        assert n == T, what
        assert [m for k, want in ref.items() for m in C.check_bits(k, got[k][:len(want)], want)] == [], what
        for k in ("tok_id", "pos", "seq_of"):
            assert np.all(got[k][T:] == PLAN_FILL), what + f": {k} written behind the last token"
        assert np.all(got["key_valid"][T:] == 0xb3), what + ": key_valid written behind the last token"
        n_calls += 1
    print(f"plan B {B}: {n_calls} calls, bit-exact")


def test_plan_refuses_a_batch_that_does_not_fit():
    L, lib = _lib()
    c = C.plan_case(5, 65, "left", False)
    T = int(C.plan_reference(c, 0)["cu"][-1])
    rc, got, n = run_plan(c, 0, capacity=T - 1)
    assert rc == L.SR_ERR_INVALID and b"packs to" in lib.sr_last_error() and n == T
    assert np.all(got["tok_id"] == PLAN_FILL) and np.all(got["seq_of"] == PLAN_FILL)          # nothing written past what fits
    assert C.check_bits("cu", got["cu"], C.plan_reference(c, 0)["cu"]) == []
    rc, got, n = run_plan(c, 0, capacity=T)
    assert rc == L.SR_OK and C.check_plan(c, 0, got) == []
