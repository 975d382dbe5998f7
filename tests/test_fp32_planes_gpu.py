"""GPU: what the fp32 regime on fp16 planes (fp32_planes = 16) launches around the attention, kernel by kernel and element by
element against float64 with the derived bounds of tests/fp32_plane_cases.py (test_fp32_planes_host.py shows on the CPU that
ideally rounded arithmetic is inside every bound and that the defects these tests are there for are outside).  Test hooks:
sr_rows_split_f16, sr_gu_cmax_f16, sr_gemm_f16_planes (include/sr_hip.h, "building blocks").

Row split (launch_rows_split_f16, csrc/encoder_f16_planes.hip):

  kernel                          K            reached by
  rows_split_h_kernel             64 192 320   test_row_split[64 / 192 / 320]: K % 256 != 0, the maximum in the last K tail
  rows_split_h_reg_kernel<8>      2048         test_row_split[2048]
  rows_split_h_reg_kernel<16>     4096         test_row_split[4096]
  rows_split_h_reg_kernel<32>     8192         test_row_split[8192]
  gu_cmax_kernel                  -            test_gu_cmax_and_act_scale (both segment counts), test_loose_bound
  each with T = 1 3 4 5 9 (a block holds four rows), nseg 2 / 3, without norm (bit-exact), with norm, with the embedding gather
  (ids out of order, source row written back), with and without gu_cmax.

GEMM (launch_gemm_bf16, csrc/gemm_bf16.hip) - every epilogue x every route below; M = 1 17 33 65 200 300, N = 128 320 (ragged
against both tile widths; QKV at head_dim 128: 256 384), K' of 3 4 5 12 15 k-steps at 2 and 3 segments:

  tile configuration                          switches                                     M that reach it
  64 x 16 / 32 / 64, one wave, 4 stages       default                                      1 / 17 / 33 (<= 64 rows, >= 4 k-steps)
  128 x 64, 4 waves, 3 stages                 default (SR_GEMM_SKINNY=0 below 65 rows)      65 200 300 (>= 4 k-steps); 33 with SKINNY=0
  128 x 128, 4 waves                          SR_GEMM_TILE=128; default below 4 k-steps     every M at 3 k-steps; QKV head_dim 128 everywhere
  128 x 128 / 128 x 64 not pipelined          default, 3 k-steps                           every M
  256 x 256 eight-wave                        SR_GEMM_TILE=256 [+ SR_GEMM_BIG=8w]           every M (+ SR_GEMM_SKINNY=0 below 65 rows)
  256 x 256 eight-wave not pipelined          SR_GEMM_TILE=256, 3 k-steps                  every M
  256 x 256 four-wave, staged epilogue        SR_GEMM_TILE=256 + SR_GEMM_BIG=4w            residual, SwiGLU split (the staged ones);
                                              SR_GEMM_TILE=256 alone                       SwiGLU split at 2 segments (FOUR_WAVE_AT_2SEG)
  256 x 256 head + 128 x 64 tail (rows_from)  SR_GEMM_TILE=split:256 [+ BIG=8w / 4w]       300: per-row scales, positions, sequence ids

  epilogue                 what the case brings
  9  QKV + bias + RoPE     head_dim 64 / 128, with / without bias, shuffled positions, n_rope a multiple of 128 and not, v features
  10 residual              C pre-filled, the product added exactly once
  11 SwiGLU fp32           |g| up to 100 of both signs (expf(-g) overflows)
  12 per-sequence max      a sequence of 1 next to one of 200, borders inside tiles and wave slabs, -2 rows with the largest
                           values, an all-negative column, a sequence without a row
  13 SwiGLU split          out_nseg 2 / 3, out_scale from the CPU and from sr_rows_split_f16, no inf / NaN, third = second segment

All routes of a case are bit-identical; two segments with a zero low weight plane give the bits of three.

Loose bound (test_loose_bound): one gate/up pair 32 x / 1024 x the others.  Measured on MI355X, worst error relative to the row's
largest element over the rows with log2(B / r) > 15 / 25 (the GEMM's accumulation error is part of both routes):
  factor 32:    fused 2^-21.3   unfused 2^-21.8   derived floor 2^-39 B / r = 2^-22.5
  factor 1024:  fused 2^-12.6   unfused 2^-21.5   derived floor 2^-39 B / r = 2^-12.5
The fused split stays inside its DERIVED bound (which contains that floor) and the test asserts so; that the bound is useless for
such weights is what sr_model_finalize's per-layer fallback answers (tests/test_fp32_regime_gpu.py asserts the model-level claim)."""
import itertools

import numpy as np
import pytest
import torch

import fp32_plane_cases as C

pytestmark = [pytest.mark.gpu, pytest.mark.fp32_regime]

SWITCHES = ("SR_GEMM_TILE", "SR_GEMM_BIG", "SR_GEMM_SKINNY")


def _lib():
    from scaling_retriever_amd import _lib as L
    return L, L.load()


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _f16(t):
    """fp16 planes travel as raw 16-bit words."""
    return t.cpu().numpy().view(np.float16)


# ------------------------------------------------------------------------------------------ row split
def run_split(x, nseg, w=None, embed=None, tok=None, eps=1e-5, cmax=None):
    """sr_rows_split_f16 -> (planes fp16, a_inv, src after the call, act_sc, act_inv)."""
    L, lib = _lib()
    T, K = x.shape
    d_x, d_w, d_e, d_t = _dev(x), _dev(w), _dev(embed), _dev(tok)
    planes = torch.full((T, nseg * K), 0x7e00, dtype=torch.int16, device="cuda")          # fp16 NaN: every element must be written
    inv = torch.full((T,), float("nan"), device="cuda")
    sc, si = (torch.full((T,), float("nan"), device="cuda") for _ in range(2))
    d_c = None if cmax is None else torch.tensor([cmax], dtype=torch.float32, device="cuda")
    L.check(lib.sr_rows_split_f16(_ptr(d_x), _ptr(d_e), _ptr(d_t), _ptr(d_w), eps, T, K, nseg, planes.data_ptr(), inv.data_ptr(),
                                  _ptr(d_c), _ptr(sc) if d_c is not None else None, _ptr(si) if d_c is not None else None,
                                  L.stream_ptr()), "sr_rows_split_f16")
    torch.cuda.synchronize()
    return _f16(planes), inv.cpu().numpy(), d_x.cpu().numpy(), sc.cpu().numpy(), si.cpu().numpy()


@pytest.mark.parametrize("K", C.SPLIT_K)
def test_row_split(K):
    for T, nseg in itertools.product(C.SPLIT_T, (2, 3)):
        c = C.split_case(K, T)
        x, w, eps = c["x"], c["w"], c["eps"]
        what = f"K {K} T {T} nseg {nseg}"
        planes, inv, src, _, _ = run_split(x, nseg)
        assert C.check_split_exact(x, nseg, planes, inv) == [], what + " (no norm)"
        assert np.array_equal(src.view(np.uint32), x.view(np.uint32)), what + ": the source rows changed"
        planes, inv, src, _, _ = run_split(x, nseg, w=w, eps=eps)
        assert C.check_split_norm(x, w, eps, nseg, planes, inv) == [], what + " (norm)"
        assert np.array_equal(src.view(np.uint32), x.view(np.uint32)), what + ": the source rows changed"
        # the gather: rows come from the table in the order of the token ids and are written back over whatever src held
        junk = np.full_like(x, 7.0)
        g = c["embed"][c["tok"]]
        planes_g, inv_g, src, _, _ = run_split(junk, nseg, w=w, embed=c["embed"], tok=c["tok"], eps=eps)
        assert C.check_split_norm(g, w, eps, nseg, planes_g, inv_g) == [], what + " (gather + norm)"
        assert np.array_equal(src.view(np.uint32), g.view(np.uint32)), what + ": gathered rows not written back"
        # ... and gives the bits of the norm of those rows without the gather
        planes_d, inv_d, _, _, _ = run_split(g, nseg, w=w, eps=eps)
        assert np.array_equal(planes_g.view(np.uint16), planes_d.view(np.uint16)) and np.array_equal(inv_g, inv_d), what
        # with gu_cmax: the same planes, plus the row scale of the SwiGLU output
        cmax = np.float32(0.37)
        planes_c, inv_c, _, sc, si = run_split(x, nseg, w=w, eps=eps, cmax=cmax)
        assert np.array_equal(planes_c.view(np.uint16), planes.view(np.uint16)) and np.array_equal(inv_c, inv), what + " (gu_cmax)"
        assert C.check_act_scale(x, w, eps, cmax, sc, si) == [], what + " (act_sc)"


@pytest.mark.parametrize("nseg", [2, 3])
def test_gu_cmax_and_act_scale(nseg):
    """gu_cmax_kernel on plane segments: a bound (>= the true maximum) within (K + 5) e of 1.001 x it, with the largest pair first,
    last, and inside a 16-pair block of the interleaved matrix; K below and above one pass of a wave (64 lanes)."""
    L, lib = _lib()
    rng = np.random.default_rng(nseg)
    for I, K, top in [(48, 64, 0), (48, 192, 47), (512, 320, 300), (32, 2048, 17)]:
        wg = (rng.standard_normal((I, K)) * np.exp(rng.uniform(-1, 1, (I, 1)))).astype(np.float32)
        wu = (rng.standard_normal((I, K)) * np.exp(rng.uniform(-1, 1, (I, 1)))).astype(np.float32)
        wg[top] *= 1000.0                                        # beyond the e^4 the magnitudes span
        w = C.interleave_gate_up(wg, wu)
        if nseg == 2:
            w = C.fp16_valued(w)
        W, w_inv = C.weight_planes(w, nseg)
        d_W, d_i = _dev(W.view(np.int16)), _dev(w_inv)
        out = torch.full((1,), 123.0, device="cuda")              # the hook zeroes it first
        L.check(lib.sr_gu_cmax_f16(d_W.data_ptr(), d_i.data_ptr(), I, K, nseg, out.data_ptr(), L.stream_ptr()), "sr_gu_cmax_f16")
        torch.cuda.synchronize()
        _, p = C.cmax_reference(W, w_inv, nseg)
        assert p.argmax() == top
        assert C.check_cmax(out.cpu().numpy()[0], W, w_inv, nseg) == [], (I, K, nseg)


# ------------------------------------------------------------------------------------------ GEMM epilogues
def routes(c):
    """[(name, {switch: value})] for a case: see the table in the module docstring."""
    epi, M, steps = c["epi"], c["M"], c["K"] // 64
    big = [("", {}), ("+8w", {"SR_GEMM_BIG": "8w"})] + ([("+4w", {"SR_GEMM_BIG": "4w"})] if epi in C.STAGED_4W else [])
    out = [("default", {}), ("tile128", {"SR_GEMM_TILE": "128"})]
    out += [("tile256" + n, dict(e, SR_GEMM_TILE="256")) for n, e in big]
    if M <= 64 and steps >= 4:            # the single-wave tiles take these rows first: switch them off to reach the others
        out += [(n + ",skinny0", dict(e, SR_GEMM_SKINNY="0")) for n, e in out[1:]] + [("skinny0", {"SR_GEMM_SKINNY": "0"})]
    if M > 256:
        out += [("split256" + n, dict(e, SR_GEMM_TILE="split:256")) for n, e in big]
    return out


def run_gemm(c, env, monkeypatch, dev=None, out_scale=None):
    """sr_gemm_f16_planes on a case under the given switches -> the output as numpy (fp32, or fp16 planes for epilogue 13)."""
    L, lib = _lib()
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    d = dev if dev is not None else {}
    if not d:
        d.update(A=_dev(c["A"].view(np.int16)), W=_dev(c["W"].view(np.int16)), a=_dev(c["a_inv"]), w=_dev(c["w_inv"]))
        for k in ("pos", "cos", "sin", "bias", "seq_of", "out_scale"):
            d[k] = _dev(c.get(k))
    epi, M, N = c["epi"], c["M"], c["N"]
    if epi == C.EPI_RESID:
        out = _dev(c["C0"])
    elif epi == C.EPI_SEGMAX:
        out = torch.zeros((c["n_seq"], N), dtype=torch.float32, device="cuda")
    elif epi == C.EPI_SPLIT:
        out = torch.full((M, c["out_nseg"] * N // 2), 0x7e00, dtype=torch.int16, device="cuda")
    else:
        out = torch.full((M, N // 2 if epi == C.EPI_SWIGLU else N), float("nan"), device="cuda")
    osc = d["out_scale"] if out_scale is None else out_scale
    L.check(lib.sr_gemm_f16_planes(d["A"].data_ptr(), d["W"].data_ptr(), M, N, c["K"], epi, c["nseg"], d["a"].data_ptr(), d["w"].data_ptr(),
                                   out.data_ptr(), _ptr(d["pos"]), _ptr(d["cos"]), _ptr(d["sin"]), c.get("n_rope", 0), c.get("hd", 0),
                                   _ptr(d["bias"]), _ptr(d["seq_of"]), _ptr(osc), c.get("out_nseg", 0), L.stream_ptr()),
            "sr_gemm_f16_planes")
    torch.cuda.synchronize()
    for k in env:
        monkeypatch.delenv(k, raising=False)
    return _f16(out) if epi == C.EPI_SPLIT else out.cpu().numpy()


def _bits(a):
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


@pytest.mark.parametrize("M", C.GEMM_M)
@pytest.mark.parametrize("name", list(C.EPILOGUES))
def test_epilogue(name, M, monkeypatch):
    """Every case of the epilogue at this M: the default route element-wise against the bound, every other route bit-identical."""
    worst, n_routes = 0.0, 0
    for c in C.epilogue_cases(C.EPILOGUES[name], Ms=[M]):
        what = {k: c[k] for k in ("epi", "M", "N", "nseg", "K0", "hd", "n_rope", "out_nseg") if k in c}
        dev, first = {}, None
        for rname, env in routes(c):
            out = run_gemm(c, env, monkeypatch, dev)
            if first is None:
                first = out
                assert C.check_gemm(c, out) == [], (what, rname)
                worst = max(worst, C.worst_ratio(c, out))
            else:
                assert np.array_equal(_bits(out), _bits(first)), (what, f"route {rname} != default")
            n_routes += 1
    print(f"{name} M {M}: {n_routes} launches, worst error {worst:.3f} of the bound")


@pytest.mark.parametrize("name", list(C.EPILOGUES))
def test_two_segments_with_zero_low_plane_equal_three(name, monkeypatch):
    """Weights without a low plane: [w0 | w0] against [low | high] activations gives the bits of [w0 | 0 | w0] against
    [low | high | high] - the product sr_model_finalize's segment drop relies on."""
    epi = C.EPILOGUES[name]
    for M, N in [(33, 128), (300, 320)]:
        c2 = C.epilogue_cases(epi, Ms=[M])
        c2 = [c for c in c2 if c["nseg"] == 2 and c["K0"] == 128 and (epi == C.EPI_QKV or c["N"] == N)][0]
        K0 = c2["K0"]
        hi = c2["W"][:, :K0]
        c3 = dict(c2, nseg=3, K=3 * K0, W=np.concatenate([hi, np.zeros_like(hi), hi], axis=1),
                  A=np.concatenate([c2["A"], c2["A"][:, K0:]], axis=1))
        a, b = run_gemm(c2, {}, monkeypatch), run_gemm(c3, {}, monkeypatch)
        assert np.array_equal(_bits(a), _bits(b)), (name, M, N)
        assert C.check_gemm(c3, b) == []


def test_split_epilogue_with_the_scale_of_the_row_split_kernel(monkeypatch):
    """The two kernels tied together as the encoder ties them: norm + split with gu_cmax gives the planes, a_inv and act_sc, the
    SwiGLU-split GEMM consumes all three.  No inf / NaN, reconstruction within the bound (with the kernel's own act_sc, which
    test_row_split holds to its definition)."""
    L, lib = _lib()
    rng = np.random.default_rng(5)
    for T, K0, I, out_nseg, env in [(9, 192, 64, 3, {}), (300, 320, 160, 2, {"SR_GEMM_TILE": "split:256"}), (65, 2048, 64, 3, {})]:
        x = (rng.standard_normal((T, K0)) * np.exp(rng.uniform(-3, 3, (T, 1)))).astype(np.float32)
        wn = rng.uniform(0.5, 1.5, K0).astype(np.float32)
        wg = (rng.standard_normal((I, K0)) * np.exp(rng.uniform(-1, 1, (I, 1))) / np.sqrt(K0)).astype(np.float32)
        wu = (rng.standard_normal((I, K0)) * np.exp(rng.uniform(-1, 1, (I, 1))) / np.sqrt(K0)).astype(np.float32)
        W, w_inv = C.weight_planes(C.interleave_gate_up(wg, wu), 3)
        cm = torch.zeros((1,), device="cuda")
        d_W = _dev(W.view(np.int16))
        d_wi = _dev(w_inv)
        L.check(lib.sr_gu_cmax_f16(d_W.data_ptr(), d_wi.data_ptr(), I, K0, 3, cm.data_ptr(), L.stream_ptr()))
        torch.cuda.synchronize()
        cmax = cm.cpu().numpy()[0]
        planes, inv, _, sc, si = run_split(x, 3, w=wn, eps=1e-5, cmax=cmax)
        assert C.check_act_scale(x, wn, 1e-5, cmax, sc, si) == []
        c = dict(epi=C.EPI_SPLIT, M=T, N=2 * I, nseg=3, K0=K0, K=3 * K0, A=planes, a_inv=inv, W=W, w_inv=w_inv, out_scale=sc, out_nseg=out_nseg)
        out = run_gemm(c, env, monkeypatch)
        assert C.check_gemm(c, out) == [], (T, K0, I)


# ------------------------------------------------------------------------------------------ the loose bound
@pytest.mark.parametrize("factor", [32, 1024])
def test_loose_bound(factor, monkeypatch):
    """One gate/up pair `factor` times the others (K0 = 256, I = 512, T = 16).  The fused route scales a row by the bound B, the
    unfused one (fp32 SwiGLU epilogue + row split) by the row's real maximum r: the fused low plane's floor is 2^-39 B, i.e.
    2^-39 B / r of the row's largest element.  Reported: both routes' reconstruction errors relative to r over the loose rows,
    next to that floor.  Asserted: B / r as constructed, both routes inside their DERIVED bounds (the fused one's contains the
    floor - it is honest, not tight), and the unfused route at the 2^-22 class whatever B is."""
    L, lib = _lib()
    c = C.loose_case(factor)
    r = C.loose_reference(c)
    T, K0, I = c["T"], c["K0"], c["I"]
    l2 = np.log2(r["B"] / r["rmax"])
    loose = l2 > C.LOOSE_LOG2[factor]
    assert loose.sum() >= T // 4
    d_W, d_wi = _dev(c["W"].view(np.int16)), _dev(c["w_inv"])
    cm = torch.zeros((1,), device="cuda")
    L.check(lib.sr_gu_cmax_f16(d_W.data_ptr(), d_wi.data_ptr(), I, K0, 3, cm.data_ptr(), L.stream_ptr()))
    torch.cuda.synchronize()
    cmax = cm.cpu().numpy()[0]
    assert C.check_cmax(cmax, c["W"], c["w_inv"], 3) == []
    planes, inv, _, sc, si = run_split(c["x"], 3, w=c["wn"], eps=c["eps"], cmax=cmax)
    assert C.check_act_scale(c["x"], c["wn"], c["eps"], cmax, sc, si) == []
    base = dict(M=T, N=2 * I, nseg=3, K0=K0, K=3 * K0, A=planes, a_inv=inv, W=c["W"], w_inv=c["w_inv"])
    fused_c = dict(base, epi=C.EPI_SPLIT, out_scale=sc, out_nseg=3)
    fused = run_gemm(fused_c, {}, monkeypatch)
    assert C.check_gemm(fused_c, fused) == []
    unf_c = dict(base, epi=C.EPI_SWIGLU)
    act = run_gemm(unf_c, {}, monkeypatch)
    assert C.check_gemm(unf_c, act) == []
    u_planes, u_inv, _, _, _ = run_split(act, 3)
    assert C.check_split_exact(act, 3, u_planes, u_inv) == []
    # truth of THESE planes (the GEMM's operands are the kernel's own split of the normalised rows)
    Y, _ = C.gemm_reference(unf_c)
    rmax = np.abs(Y).max(axis=1)
    e_f = np.abs(C.decode(fused_c, fused) - Y).max(axis=1) / rmax
    e_u = np.abs(C.planes_value(u_planes, u_inv, 3) - Y).max(axis=1) / rmax
    floor = 2.0 ** -39 * r["B"] / r["rmax"]
    print(f"factor {factor}: rows with log2(B / r) > {C.LOOSE_LOG2[factor]}: {int(loose.sum())} of {T}; worst error relative to the row maximum: "
          f"fused 2^{np.log2(e_f[loose].max()):.1f}, unfused 2^{np.log2(e_u[loose].max()):.1f}, derived floor 2^-39 B / r = 2^{np.log2(floor[loose].max()):.1f}; "
          f"other rows: fused 2^{np.log2(e_f[~loose].max()):.1f}, unfused 2^{np.log2(e_u[~loose].max()):.1f}")
    # the unfused route does not know B: GEMM term + 2^-22 of the split, relative to the row maximum
    _, ey = C.gemm_reference(unf_c)
    assert np.all(e_u <= (ey.max(axis=1) + 2.0 ** -22 * (rmax + ey.max(axis=1))) / rmax + 2.0 ** -25 * u_inv / rmax)
