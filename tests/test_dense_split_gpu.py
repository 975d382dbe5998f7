"""GPU: the split-bf16 score modes of the dense search (SR_PRECISION_BF16X3 / _BF16X6), kernel by kernel and pair by pair against
float64 with the derived bounds of tests/dense_split_cases.py (test_dense_split_host.py shows on the CPU that ideally rounded
arithmetic is inside every bound, that the closed form of tier B is reached to within 4 %, and that the defects these tests are there
for are outside).  No pair, no query and no case is sampled or exempt.

  kernel                                   what                                                     reached by
  split_bf16_kernel (sr_split_bf16)        the planes bit for bit against the restatement: +-0,     test_split_kernel_bit_for_bit: n = 4, 1 032 (two
                                           fp32 and bf16 subnormals, ties and their nextafter       blocks), 2^20 + 1 028 (1 026 blocks); 3, 2 and 1
                                           neighbours, the top binade up to FLT_MAX (p0 saturates:  planes (p1 / p2 null as split_segment passes
                                           finite planes for finite values), every data kind        them), guard words behind every plane
  dense_split_kernel<false, false>         every (query, document) score: a search with k = N;      test_every_pair[H-N-nq-kind], both modes
                                           tau stays -inf: the counted survivor path

  H     N              nq        nkt x3 / x6   query tiles (qt, bq, bd)   what the shape is there for
  64    255 256 257    65        3 / 6         1, 1, 32                   odd nkt, a plane switch at EVERY k-step, the whole k-loop in the two-step
                                                                          tail (nkt - 2 = 1 steady k-step for x3); ragged / full / full + 1 doc tile
  192   513            129       9 / 18        1, 1, 32                   H / 64 odd; 3 doc tiles, the last with one row
  128   700            257 513   6 / 12        2, 2, 16 and 3, 1, 32      ragged query tile (1 query / 1 query in the last), ragged doc tile
  64    33 100         300       3 / 6         2, 2, 16                   130 doc tiles x 2 = 512 slots > 256 workgroups: `carried` tiles, set_tile under
                                                                          the k-loop, the last-tile tail, slots past the last doc tile skipped
  64    66 000         65        3 / 6         1, 1, 32                   258 doc tiles, the same with qt = 1
  1024  2 000          130       48 / 96       1, 1, 32                   long k-loop, stretches of 16 k-steps per plane
  data kinds: gauss on every shape; same_sign aligned wide tiny bf16_exact zeros on 64 / 257 / 65 and 128 / 700 / 257.
  + three segments of strided ids (id_base = j, id_stride = 3), one shorter than a tile; a segment added after set_precision; the same
    documents in 1 and in 3 contiguous segments cut at multiples of 256: equal bits (test_segments_*).

  small k (tau rises, per-lane segments of SR_SEG_P slots; N = 100 000, H = 64, nq 65 / 300, k 1 10 1000 4096; launches of 65 536 /
  32 768 rows, then doubled): every returned score within dA of T, every document NOT returned has T - dA <= the k-th returned
  score, rows descending with ties in ascending id, no id twice, the k-prefix of the k = 4096 result bit for bit (test_small_k).

  dev switches (SR_DEV_SWITCHES=1, read per call): SR_SPLIT_SEG=0 (atomic appends only), SR_SPLIT_XCD=0 (query tile fastest, no
  rounding of the slot count), SR_SPLIT_PERSIST=0 (one workgroup per slot: no carried tile) give the bits of the default on one case
  of each kind (test_dev_switches_give_the_same_bits).

Measured on one MI355X, largest |s~ - T| / dA per case over all its pairs (information: printed by the tests, asserted only to be <= 1,
which the derivation gives; dA counts K e for a sum whose roundings mostly cancel, so a sound kernel sits near 1 % of it, and the
defects these tests are there for - test_dense_split_host.py - sit at tens to hundreds of dA):
  case [H-N-nq-kind]            bf16x3  bf16x6
  [64-255-65-gauss]             0.0079  0.0036
  [64-256-65-gauss]             0.0064  0.0029
  [64-257-65-gauss]             0.0059  0.0028
  [192-513-129-gauss]           0.0029  0.0015
  [128-700-257-gauss]           0.0043  0.0022
  [128-700-513-gauss]           0.0051  0.0026
  [64-33100-300-gauss]          0.0105  0.0057
  [64-66000-65-gauss]           0.0105  0.0050
  [1024-2000-130-gauss]         0.0007  0.0004
  [64-257-65-same_sign]         0.0145  0.0087
  [64-257-65-aligned]           0.0073  0.0036
  [64-257-65-wide]              0.0200  0.0097
  [64-257-65-tiny]              0.0054  0.0019
  [64-257-65-bf16_exact]        0.0066  0.0033
  [64-257-65-zeros]             0.0055  0.0031
  [128-700-257-same_sign]       0.0114  0.0058
  [128-700-257-aligned]         0.0035  0.0017
  [128-700-257-wide]            0.0138  0.0073
  [128-700-257-tiny]            0.0027  0.0016
  [128-700-257-bf16_exact]      0.0036  0.0018
  [128-700-257-zeros]           0.0036  0.0022
  [3 strided segments]          0.0073  0.0037
  [1 segment of 1000]           0.0050  0.0023
  [small k, nq 65]              0.0095  0.0047
  [small k, nq 300]             0.0107  0.0063
Checked once against deliberately broken builds (not committed): two query planes of the bf16x6 pair list exchanged (pq[1] with
pq[2]) fails 23 of these tests; the last k-step of every plane pair reading the next pair's planes fails 27; `lr0 + r <= rows_valid` in
the ragged-tail tests fails 10 (every shape whose last doc tile holds one row, and test_small_k at 300 queries).  Exchanging pq[2] with
pq[3] fails none and must not: both products read document plane 1, so the exchange only reorders the list
(test_dense_split_host.py::test_reordering_two_pairs_is_not_a_defect).
This file: 32 tests, 4 s on one MI355X."""
import numpy as np
import pytest
import torch

import dense_split_cases as C

pytestmark = [pytest.mark.gpu]

NAN_WORD = 0x7FC0
GUARD = 64
OTHER_KINDS = ("same_sign", "aligned", "wide", "tiny", "bf16_exact", "zeros")
SHAPES = [(64, 255, 65), (64, 256, 65), (64, 257, 65), (192, 513, 129), (128, 700, 257), (128, 700, 513), (64, 33100, 300),
          (64, 66000, 65), (1024, 2000, 130)]
EVERY_PAIR = [(h, n, nq, "gauss") for h, n, nq in SHAPES] + [(h, n, nq, k) for h, n, nq in ((64, 257, 65), (128, 700, 257)) for k in OTHER_KINDS]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------ a. the plane split
@pytest.mark.parametrize("n", [4, 4 * 257 + 4, (1 << 20) + 1028])
def test_split_kernel_bit_for_bit(n):
    from scaling_retriever_amd import _lib as L
    lib = L.load()
    v = C.split_vector(n)
    want = [C.plane_words(p) for p in C.split_planes(v)]
    for w in want:                                            # the requirement: the planes of a finite value are finite
        assert ((w & 0x7F80) != 0x7F80).all()
    src = _dev(v)
    for n_planes in (3, 2, 1):
        out = [torch.full((n + GUARD,), NAN_WORD, dtype=torch.int16, device="cuda") for _ in range(n_planes)]
        ptr = [o.data_ptr() for o in out] + [None] * (3 - n_planes)
        L.check(lib.sr_split_bf16(src.data_ptr(), n, ptr[0], ptr[1], ptr[2], L.stream_ptr()), "sr_split_bf16")
        torch.cuda.synchronize()
        for p, o in enumerate(out):
            got = o.cpu().numpy().view(np.uint16)
            assert (got[n:] == NAN_WORD).all(), (n_planes, p)
            bad = C.G.check_bits(f"plane {p} of {n_planes}", got[:n], want[p])
            if bad:
                i = int(np.argmax(got[:n] != want[p]))
                bad.append(f"v = {v[i]!r} (0x{int(v[i:i + 1].view(np.uint32)[0]):08x}): got 0x{int(got[i]):04x}, want 0x{int(want[p][i]):04x}")
            assert bad == [], bad


# ------------------------------------------------------------------------------------------ b. every pair
class Problem:
    """Q, D of a case on the device with the restated planes, and per mode (T, dA) - computed once, never written to."""

    def __init__(self, kind, H, N, nq):
        self.kind, self.H, self.N, self.nq = kind, H, N, nq
        self.Qn, self.Dn = C.case(kind, H, N, nq)
        self.Q, self.D = _dev(self.Qn), _dev(self.Dn)
        self.qp = [_dev(p) for p in C.split_planes(self.Qn)]
        self.dp = [_dev(p) for p in C.split_planes(self.Dn)]
        self._a = {}

    def tier_a(self, mode):
        if mode not in self._a:
            self._a[mode] = C.tier_a(self.qp, self.dp, mode)
        return self._a[mode]

    def index(self, mode, segments=None, precision_first=False):
        """segments: [(first row, end row, id_base, id_stride)]; default: one segment, ids = rows."""
        from scaling_retriever_amd.scoring import DenseIndexHIP
        idx = DenseIndexHIP(self.H)
        if precision_first:
            idx.set_precision(mode)
        for r0, r1, base, stride in segments or [(0, self.N, 0, 1)]:
            idx.add_device_rows(self.D[r0:r1], id_base=base, id_stride=stride)
        if not precision_first:
            idx.set_precision(mode)
        return idx

    def doc_of_id(self, segments=None):
        ids = torch.cat([base + stride * torch.arange(r1 - r0, device="cuda") for r0, r1, base, stride in segments or [(0, self.N, 0, 1)]])
        look = torch.full((int(ids.max()) + 1,), -1, dtype=torch.int64, device="cuda")
        look[ids] = torch.arange(self.N, device="cuda")
        return look


def _check_order(s, ids):
    assert (s[:, :-1] >= s[:, 1:]).all(), "rows are not descending"
    tie = s[:, :-1] == s[:, 1:]
    assert (ids[:, :-1][tie] < ids[:, 1:][tie]).all(), "ties are not in ascending id"


def _check_every_pair(pb, mode, s, ids, look, label):
    """s, ids [nq, N] of a k = N search -> the scores by document [nq, N]; every assertion of (b)."""
    assert s.shape == (pb.nq, pb.N) and ids.shape == (pb.nq, pb.N)
    assert ids.min() >= 0 and ids.max() < look.numel()
    docs = look[ids]
    assert (docs.sort(dim=1).values == torch.arange(pb.N, device="cuda")[None, :]).all(), "a row is not a permutation of all ids"
    _check_order(s, ids)
    S = torch.empty_like(s).scatter_(1, docs, s)
    T, dA = pb.tier_a(mode)
    r = C.ratio(S, T, dA)
    print(f"dense_split {label} {mode}: largest |s~ - T| / dA = {r:.4f}")
    err = (S.double() - T).abs()
    assert (err <= dA).all(), f"tier A: {int((~(err <= dA)).sum())} of {err.numel()} pairs outside, worst {r:.4g} of dA"
    qd, aqd = C.exact_product(pb.Q, pb.D)
    bound = dA + C.CB[mode] * aqd + C.tier_b_floor(pb.Q, pb.D)
    errb = (S.double() - qd).abs()
    assert (errb <= bound).all(), f"tier B: {int((~(errb <= bound)).sum())} pairs outside, worst {C.ratio(S, qd, bound):.4g}"
    if pb.kind == "zeros":
        zp = _dev(C.zero_pairs(pb.Qn, pb.Dn))
        assert zp.sum() > pb.nq and not S.view(torch.int32)[zp].any(), "a zero row or a zero query does not give exactly +0"
    return S, r


@pytest.mark.parametrize("H,N,nq,kind", EVERY_PAIR)
def test_every_pair(H, N, nq, kind):
    pb = Problem(kind, H, N, nq)
    look = pb.doc_of_id()
    S = {}
    for mode in C.MODES:
        idx = pb.index(mode)
        s, ids = idx.search(pb.Q, N)
        S[mode], r = _check_every_pair(pb, mode, s, ids, look, f"[{H}-{N}-{nq}-{kind}]")
        assert r <= 1.0
        del idx
    if kind == "bf16_exact":                  # the lo planes are zero: both modes have the same T, the exact product
        T3, dA3 = pb.tier_a("bf16x3")
        T6, dA6 = pb.tier_a("bf16x6")
        assert ((T3 - T6).abs() <= 2.0 ** -40 * dA6).all()           # float64's own rounding
        assert ((S["bf16x3"].double() - S["bf16x6"].double()).abs() <= dA3 + dA6).all()


def test_segments_strided_ids_and_a_segment_added_after_the_switch():
    H, nq = 64, 65
    segs = [(0, 300, 0, 3), (300, 400, 1, 3), (400, 757, 2, 3)]             # the middle one shorter than a tile
    pb = Problem("gauss", H, 757, nq)
    look = pb.doc_of_id(segs)
    for mode in C.MODES:
        idx = pb.index(mode, segs)
        s, ids = idx.search(pb.Q, pb.N)
        _check_every_pair(pb, mode, s, ids, look, "[3 strided segments]")
        late = pb.index(mode, segs[:1], precision_first=True)               # the first segment is split when it is added, the others too
        for r0, r1, base, stride in segs[1:]:
            late.add_device_rows(pb.D[r0:r1], id_base=base, id_stride=stride)
        s2, ids2 = late.search(pb.Q, pb.N)
        assert torch.equal(s, s2) and torch.equal(ids, ids2)


def test_segments_cut_at_tile_boundaries_give_the_bits_of_one_segment():
    pb = Problem("gauss", 128, 1000, 129)
    look = pb.doc_of_id()
    for mode in C.MODES:
        s1, i1 = pb.index(mode).search(pb.Q, pb.N)
        _check_every_pair(pb, mode, s1, i1, look, "[1 segment of 1000]")
        s3, i3 = pb.index(mode, [(0, 256, 0, 1), (256, 768, 256, 1), (768, 1000, 768, 1)]).search(pb.Q, pb.N)
        assert torch.equal(s1, s3) and torch.equal(i1, i3)


# ------------------------------------------------------------------------------------------ c. small k
SMALL_K = (1, 10, 1000)
_small = {}


@pytest.fixture(scope="module", autouse=True)
def _release_shared_references():
    yield
    _small.clear()                            # the tests behind this file size themselves by the free HBM
    torch.cuda.empty_cache()


def _small_problem(nq):
    if nq not in _small:
        _small.clear()                        # one at a time: T and dA of 300 x 100 000 pairs are 240 MB each
        _small[nq] = Problem("gauss", 64, 100000, nq)
    return _small[nq]


def _check_small_k(pb, mode, s, ids, k):
    T, dA = pb.tier_a(mode)
    assert s.shape == (pb.nq, k) and ids.min() >= 0 and ids.max() < pb.N
    err = (s.double() - T.gather(1, ids)).abs()
    assert (err <= dA.gather(1, ids)).all(), f"(i) k = {k}: worst {float((err / dA.gather(1, ids)).max()):.4g} of dA"
    lo = (T - dA).scatter_(1, ids, float("-inf"))                 # (T - dA is a new tensor: the shared reference is not written to)
    assert (lo.max(dim=1).values <= s[:, -1].double()).all(), f"(ii) k = {k}: a document that must be in the list is not"
    if k > 1:
        _check_order(s, ids)                                        # (iii)
        srt = ids.sort(dim=1).values
        assert (srt[:, 1:] != srt[:, :-1]).all(), f"(iv) k = {k}: an id appears twice"
    return float((err / dA.gather(1, ids)).max())


@pytest.mark.parametrize("mode", C.MODES)
@pytest.mark.parametrize("nq", [65, 300])
def test_small_k(nq, mode):
    pb = _small_problem(nq)
    idx = pb.index(mode)
    s4, i4 = idx.search(pb.Q, 4096)
    worst = _check_small_k(pb, mode, s4, i4, 4096)
    for k in SMALL_K:
        s, ids = idx.search(pb.Q, k)
        worst = max(worst, _check_small_k(pb, mode, s, ids, k))
        assert torch.equal(s, s4[:, :k]) and torch.equal(ids, i4[:, :k]), f"k = {k} is not the prefix of k = 4096"
    print(f"dense_split [small k, nq {nq}] {mode}: largest |s~ - T| / dA = {worst:.4f}")


# ------------------------------------------------------------------------------------------ d. the other paths
@pytest.mark.parametrize("mode", C.MODES)
def test_dev_switches_give_the_same_bits(mode, monkeypatch):
    """The per-tile arithmetic does not depend on which workgroup runs a tile, in which order, or where a survivor is stored."""
    big = Problem("gauss", 64, 33100, 300)
    small = _small_problem(300)
    want_big = big.index(mode).search(big.Q, big.N)
    want_small = small.index(mode).search(small.Q, 10)
    monkeypatch.setenv("SR_DEV_SWITCHES", "1")
    for switch in ("SR_SPLIT_SEG", "SR_SPLIT_XCD", "SR_SPLIT_PERSIST"):
        with monkeypatch.context() as m:
            m.setenv(switch, "0")
            got_big = big.index(mode).search(big.Q, big.N)            # a fresh index: the switches are read per call
            got_small = small.index(mode).search(small.Q, 10)
        assert torch.equal(got_big[0], want_big[0]) and torch.equal(got_big[1], want_big[1]), switch
        assert torch.equal(got_small[0], want_small[0]) and torch.equal(got_small[1], want_small[1]), switch
