"""CPU-only pieces shared by test_attention_bf16_host.py and test_attention_bf16_gpu.py: the kernel rows of csrc/attention.hip,
seeded case builders, the float64 reference of the operation, and the element-wise error bound.

Operation (per sequence, per q head h with kv head h // (nh / nkv)), on the bf16 inputs widened exactly to float64:

    s_j = q . k_j / sqrt(hd)   (-inf for a masked key),   p = softmax(s),   o_d = sum_j p_j v_jd,   a row without a valid key = 0.

With rope tables the operation is the same on the rotated q / k (HF rotate_half: x1' = x1 c - x2 s, x2' = x2 c + x1 s with
x2 = x[d + hd/2]); the tables of the rope cases hold quarter turns only, so the rotation is exact in every number format and
whatever the compiler contracts, and the rotated q / k are bf16 numbers again.

Bound.  Derived, never fitted, never computed from what a kernel returns.  Let p_j be the float64 probabilities, o_d the
reference output, A_d = sum_j p_j |v_jd| (>= |o_d|), n the sequence length, e = 2^-24 the unit roundoff of fp32 and u the unit
roundoff of bf16 under round to nearest even.  bf16 keeps 8 significant bits (one implicit, seven stored), so a number in
[1, 2) lies within half a spacing of 2^-7 of its rounding: u = 2^-8.  (The issue that asked for this file wrote 2^-9 for u; with
that value float64 arithmetic that does nothing but the two bf16 roundings below reaches 1.69 x the bound - 1 + 2^-8 rounds to
1 or to 1 + 2^-7, each 2^-8 away - so the value of the number format is used; every other term is as the issue states it.)
What the kernels do:

 1. The score: an MFMA dot product of exact bf16 products accumulated in fp32, |error| <= hd e sum_i |q_i k_ji|, times
    fl(scale * log2 e) (the constant carries two roundings, the product one), minus the row maximum, then exp2 (argument and
    result).  In natural-log units the score of key j is wrong by at most
        d_j = hd e scale sum_i |q_i k_ji| + 4 e |s_j| = hd 2^-24 scale sum_i |q_i k_ji| + 2^-22 |s_j|,
    delta = max_j d_j over the valid keys of the row.  A weight exp(s_j - m) / l moves by a factor within exp(+-2 delta) (its own
    score and the normaliser's), |p~_j - p_j| <= 2 delta p_j to first order: the output moves by at most 2 delta A_d.
 2. The normaliser and the P V sum: n fp32 additions each, one division or multiplication by 1 / l, one exp2 result rounding per
    weight: at most (n + 8) e relative on every term, (n + 8) e A_d together.
 3. P is rounded to bf16 once, |P_j - p~_j| <= u p~_j: u A_d.  The small and rope kernels round the normalised weight; the long
    kernel rounds the unnormalised exp2(s_j - m_running) <= 1 and divides the sum by l afterwards - the rounding is relative, the
    later rescale and division are common factors, so the term is the same u A_d.
 4. The output x is rounded to bf16 once: u |x| <= u (|o_d| + u A_d + ...): u |o_d| and the second-order u^2 A_d.

    |out_d - o_d| <= u (A_d + |o_d|) + A_d (u^2 + 2 delta + (n + 8) 2^-24),   u = 2^-8

A fully masked sequence has bound 0: its rows are exactly +0.  test_attention_bf16_host.py shows that ideally rounded
arithmetic (float64 with exactly those two bf16 roundings, in both forms of term 3) is within the bound on every element of
every case here, and that each of a list of kernel defects leaves it.

Kernel rows (launch_hd of csrc/attention.hip; SR_ATTN_CKB is its development switch, read on every call):

  row            head dim  SR_ATTN_CKB  longest sequence of the batch   kernel
  small<64,2>    64        -            <= 64                           attention_small_kernel<64, 2>
  small<64,4>    64        -            65 - 128                        attention_small_kernel<64, 4>
  small<64,6>    64        -            129 - 192                       attention_small_kernel<64, 6>
  small<64,8>    64        -            193 - 256                       attention_small_kernel<64, 8>
  long<64,8>     64        -            > 256                           attention_long_kernel<64, 8>     (chunks of 256 keys)
  small<128,2>   128       -            <= 64                           attention_small_kernel<128, 2>
  long<128,2>    128       -            > 64                            attention_long_kernel<128, 2>    (chunks of 64 keys)
  long<128,3>    128       3            > 64                            attention_long_kernel<128, 3>    (chunks of 96 keys)
  small<128,4>   128       8            65 - 128                        attention_small_kernel<128, 4>
  small<128,6>   128       8            129 - 192                       attention_small_kernel<128, 6>
  small<128,8>   128       8            193 - 256                       attention_small_kernel<128, 8>
  long<128,8>    128       8            > 256                           attention_long_kernel<128, 8>    (chunks of 256 keys)
  rope<64>       64        -            any, rope tables passed         attention_kernel<64, true>       (chunks of 256 keys)
  rope<128>      128       -            any, rope tables passed         attention_kernel<128, true>

Case kinds (all seeded, all built on the CPU): `lengths`, `masks`, `large`, `known` - see case()."""
import functools
import math

import torch

U_BF16 = 2.0 ** -8        # unit roundoff of bf16, round to nearest even: half the spacing 2^-7 of [1, 2)
E_F32 = 2.0 ** -24
MASKED_V = 8.0
MAX_POS = 1024          # rows of the rope tables of the rope cases

GEOMETRIES = [(4, 1), (32, 8), (2, 2), (2, 1), (8, 1)]
KINDS = ["lengths", "masks", "large", "known"]


def _row(hd, ckb, rope, unit, lo, hi, n0, lengths):
    """unit: keys per pass of the kernel's key loop that a mask pattern calls a `chunk` (the 32-key block of the all-in-registers
    kernels, the LDS chunk of the others); lo / hi: the bracket of the batch's longest sequence; n0: the length the mask
    patterns are sized to; lengths: the `lengths` batch."""
    assert lengths[0] != max(lengths) and 0 in lengths[1:-1] and lo <= max(lengths) and (hi is None or max(lengths) <= hi)
    return dict(hd=hd, ckb=ckb, rope=rope, unit=unit, lo=lo, hi=hi, n0=n0, lengths=lengths)


_LE64 = [33, 1, 64, 0, 32, 2, 63, 31]
_LE128 = [97, 1, 128, 0, 64, 65, 96, 33, 127, 95, 32, 100]
_LE192 = [161, 129, 192, 0, 1, 160, 128, 191, 159, 65, 100]
_LE256 = [225, 193, 256, 0, 224, 255, 223, 100, 31]
_GT256 = [257, 5, 700, 0, 511, 512, 513, 100, 256]
ROWS = {
    "small<64,2>": _row(64, None, False, 32, 1, 64, 64, _LE64),
    "small<64,4>": _row(64, None, False, 32, 65, 128, 128, _LE128),
    "small<64,6>": _row(64, None, False, 32, 129, 192, 192, _LE192),
    "small<64,8>": _row(64, None, False, 32, 193, 256, 256, _LE256),
    "long<64,8>": _row(64, None, False, 256, 257, None, 300, _GT256),
    "small<128,2>": _row(128, None, False, 32, 1, 64, 64, _LE64),
    "long<128,2>": _row(128, None, False, 64, 65, None, 200, [65, 1, 513, 0, 64, 128, 129, 192, 257, 100, 193, 63]),
    "long<128,3>": _row(128, "3", False, 96, 65, None, 250, [97, 1, 289, 0, 96, 192, 288, 95, 193, 100, 65]),
    "small<128,4>": _row(128, "8", False, 32, 65, 128, 128, _LE128),
    "small<128,6>": _row(128, "8", False, 32, 129, 192, 192, _LE192),
    "small<128,8>": _row(128, "8", False, 32, 193, 256, 256, _LE256),
    "long<128,8>": _row(128, "8", False, 256, 257, None, 300, [257, 5, 513, 0, 512, 100, 256]),
    "rope<64>": _row(64, None, True, 256, 1, None, 300, [100, 1, 300, 0, 257, 33, 513, 31]),
    "rope<128>": _row(128, None, True, 256, 1, None, 300, [100, 1, 300, 0, 257, 33, 513, 31]),
}
assert len(ROWS) == 14


def sequences(lens):
    t0 = 0
    for n in lens:
        yield t0, n
        t0 += n


# ------------------------------------------------------------------------------------------------------ cases
def mask_patterns(row):
    """[(name, n, [masked ranges])] of the `masks` batch of a row.  The longest sequence lies in the row's bracket and is not the
    first; the empty sequence sits between two others."""
    r = ROWS[row]
    U, n0, hi = r["unit"], r["n0"], r["hi"]
    three = 2 * U + U // 2 + 3
    if hi is not None and three > hi:                 # no room for three units: the masked stretch straddles the one unit edge
        middle = (hi, [(U // 2, U + U // 2)])
    else:
        middle = (three, [(U, 2 * U)])
    cap = (lambda n: n) if hi is None else (lambda n: min(n, hi))
    pats = [
        ("one masked key", n0 - 1, [(n0 // 2 + 5, n0 // 2 + 6)]),
        ("masked keys on a 32-key block edge", n0, [(31, 33)]),
        ("masked prefix", n0 - 3, [(0, 40)]),
        ("empty sequence", 0, []),
        ("masked suffix across a block edge", n0, [(n0 - 40, n0)]),
        ("a whole chunk masked in the middle", middle[0], middle[1]),
        ("the first chunk masked, later ones valid", cap(U + U // 2 + 1), [(0, U)]),
        ("one valid key only", cap(U + 7), [(0, cap(U + 7) - 3), (cap(U + 7) - 2, cap(U + 7))]),
        ("every key masked", cap(U + 5), [(0, cap(U + 5))]),
    ]
    assert (n0 // 2 + 5) % 32 not in (0, 31) and pats[0][1] != max(p[1] for p in pats) and r["lo"] <= max(p[1] for p in pats)
    assert hi is None or max(p[1] for p in pats) <= hi
    return pats


def _quarter_turn_tables(g, hd):
    turn = torch.randint(0, 4, (MAX_POS, hd // 2), generator=g)
    return torch.tensor([1.0, 0.0, -1.0, 0.0])[turn].contiguous(), torch.tensor([0.0, 1.0, 0.0, -1.0])[turn].contiguous()


def rotate(x, pos, cos, sin, partner_next=False, inverse=False):
    """HF rotate_half of x [T, heads, hd] with the table rows pos [T]; exact for quarter-turn tables.  partner_next: the
    DEFECT of pairing d with d + 1 instead of d + hd/2."""
    hd = x.shape[-1]
    c, s = cos[pos.long()].to(x)[:, None, :], sin[pos.long()].to(x)[:, None, :]
    if inverse:
        s = -s
    x1 = x[..., :hd // 2]
    x2 = x[..., 1:hd // 2 + 1] if partner_next else x[..., hd // 2:]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)


@functools.lru_cache(maxsize=8)
def case(row, kind, nh, nkv):
    """The inputs of one (kernel row, case kind, head geometry), on the CPU:
    qkv bf16 [T, (nh + 2 nkv) hd] as the kernel gets it, lens, key_valid uint8 [T]; rope rows: pos int32 [T], cos / sin fp32
    [MAX_POS, hd/2]; `known`: target int64 [T, nh] = the key each (row, head) attends to.

    lengths  randn, every key valid, the row's `lengths` batch (every 32-key block edge and chunk edge of the bracket, an empty
             sequence between two others, the longest not first).
    masks    randn, one sequence per mask pattern (mask_patterns); masked keys carry v = 8.0 in every dim.
    large    the `lengths` batch with keys of norm sqrt(hd) and q row r of head h = c (k[t] + 0.99 k[u]) + noise, c sqrt(hd) =
             300: the scaled scores of keys t and u are ~300 and ~297, every other key far below; t and u walk through the
             sequence with r, so for most rows the dominant keys lie in a later chunk than the first.  Rounded to bf16.
    known    the `lengths` batch; k of (key j, kv head g) = a random sign vector, q of (row r, head h) = 16 x the sign vector of
             its key t(r, h) in its kv head; v of (key j, kv head g) = [j % 256, j // 256, g, 0 ... 1 at 3 + j % (hd - 3) ... 0]:
             every entry exact in bf16; the output row names the key and the kv head."""
    r = ROWS[row]
    hd, G = r["hd"], nh // nkv
    g = torch.Generator().manual_seed(100000 * list(ROWS).index(row) + 1000 * nh + 10 * nkv + KINDS.index(kind))
    if kind == "masks":
        pats = mask_patterns(row)
        lens = [n for _, n, _ in pats]
        key_valid = torch.ones(sum(lens), dtype=torch.uint8)
        for (t0, n), (_, _, masked) in zip(sequences(lens), pats):
            for a, b in masked:
                key_valid[t0 + a:t0 + b] = 0
    else:
        lens = list(r["lengths"])
        key_valid = torch.ones(sum(lens), dtype=torch.uint8)
    T = sum(lens)
    q = torch.randn((T, nh, hd), generator=g)
    k = torch.randn((T, nkv, hd), generator=g)
    v = torch.randn((T, nkv, hd), generator=g)
    extra = {}
    if kind == "masks":
        v[key_valid == 0] = MASKED_V
    if kind == "large":
        k = k / k.norm(dim=-1, keepdim=True) * math.sqrt(hd)
        c = 300.0 / math.sqrt(hd)
        for t0, n in sequences(lens):
            i = torch.arange(n)
            for h in range(nh):
                t, u = (7 * i + 3 * h + 3) % max(n, 1), (7 * i + 3 * h + 4) % max(n, 1)
                q[t0 + i, h] = c * (k[t0 + t, h // G] + 0.99 * k[t0 + u, h // G]) + 0.1 * q[t0 + i, h]
    if kind == "known":
        k = torch.where(torch.rand((T, nkv, hd), generator=g) < 0.5, -1.0, 1.0)
        v = torch.zeros((T, nkv, hd))
        target = torch.zeros((T, nh), dtype=torch.int64)
        for t0, n in sequences(lens):
            j = torch.arange(n)
            for gk in range(nkv):
                v[t0 + j, gk, 0] = (j % 256).float()
                v[t0 + j, gk, 1] = (j // 256).float()
                v[t0 + j, gk, 2] = float(gk)
                v[t0 + j, gk, 3 + j % (hd - 3)] = 1.0
            for h in range(nh):
                t = (5 * j + 3 * h + 1) % max(n, 1)
                target[t0 + j, h] = t
                q[t0 + j, h] = 16.0 * k[t0 + t, h // G]
        extra["target"] = target
    q, k, v = q.bfloat16().float(), k.bfloat16().float(), v.bfloat16().float()
    if r["rope"]:
        # q / k above are what the kernel must see AFTER its rotation: hand it their exact inverse rotation
        cos, sin = _quarter_turn_tables(g, hd)
        pos = torch.randint(0, MAX_POS, (T,), generator=g).int()        # not monotone, repeats allowed
        q, k = rotate(q, pos, cos, sin, inverse=True), rotate(k, pos, cos, sin, inverse=True)
        extra.update(pos=pos, cos=cos, sin=sin)
    qkv = torch.cat([q.reshape(T, -1), k.reshape(T, -1), v.reshape(T, -1)], dim=1).bfloat16().contiguous()
    return dict(row=row, kind=kind, nh=nh, nkv=nkv, hd=hd, qkv=qkv, lens=lens, key_valid=key_valid, **extra)


def fully_masked_rows(c):
    """bool [T]: rows of a sequence without a valid key."""
    out = torch.zeros(sum(c["lens"]), dtype=torch.bool)
    for t0, n in sequences(c["lens"]):
        if n and not bool(c["key_valid"][t0:t0 + n].any()):
            out[t0:t0 + n] = True
    return out


# ------------------------------------------------------------------------------------------------------ float64 arithmetic
def rne_bf16(x):
    """float64 -> the nearest bf16 number (8 significant bits, ties to even), as float64; one rounding, not two."""
    m, e = torch.frexp(x)
    return torch.ldexp(torch.round(m * 256.0), e - 8)


def _operands(c, device, rope_partner_next=False):
    """q [T, nh, hd], k, v [T, nkv, hd] float64 as the softmax sees them (rotated for a rope row); the last two cases are kept."""
    key = (c["row"], c["kind"], c["nh"], c["nkv"], str(device), rope_partner_next)
    if key not in _OPERANDS:
        if len(_OPERANDS) >= 2:
            _OPERANDS.pop(next(iter(_OPERANDS)))
        _OPERANDS[key] = _widen(c, device, rope_partner_next)
    return _OPERANDS[key]


_OPERANDS = {}


def _widen(c, device, rope_partner_next):
    T, nh, nkv, hd = sum(c["lens"]), c["nh"], c["nkv"], c["hd"]
    x = c["qkv"].to(device).double()
    q = x[:, :nh * hd].reshape(T, nh, hd)
    k = x[:, nh * hd:(nh + nkv) * hd].reshape(T, nkv, hd)
    v = x[:, (nh + nkv) * hd:].reshape(T, nkv, hd)
    if "pos" in c:
        pos, cos, sin = c["pos"].to(device), c["cos"].to(device), c["sin"].to(device)
        q, k = rotate(q, pos, cos, sin, rope_partner_next), rotate(k, pos, cos, sin, rope_partner_next)
    return q, k, v


HEAD_BLOCK = 8      # q heads per einsum: bounds the [heads, n, n] float64 temporaries


def _attend(q, k, v, valid, hd, forms=(None,), want_bound=False, exp2_of_ln=False):
    """One sequence, q / k / v [n, H, hd] float64 (k, v already expanded to the q heads), valid bool [n], at least one valid.
    Returns ([one output [n, H, hd] per entry of forms], bound or None).  form None: the float64 reference; 'normalised' /
    'unnormalised': the same with P rounded to bf16 in that form and the output rounded to bf16.  exp2_of_ln: the DEFECT of a
    missing log2 e."""
    n, H = q.shape[0], q.shape[1]
    outs, bound = [torch.empty_like(q) for _ in forms], (torch.empty_like(q) if want_bound else None)
    scale = 1.0 / math.sqrt(hd)
    for h0 in range(0, H, HEAD_BLOCK):
        hs = slice(h0, min(H, h0 + HEAD_BLOCK))
        sc = torch.einsum("qhd,khd->hqk", q[:, hs], k[:, hs]) / math.sqrt(hd)
        sc = sc.masked_fill(~valid[None, None, :], float("-inf"))
        if exp2_of_ln:
            sc = sc * math.log(2.0)
        e = torch.exp(sc - sc.max(dim=-1, keepdim=True).values)
        l = e.sum(dim=-1, keepdim=True)
        p = e / l
        for out, form in zip(outs, forms):
            if form == "unnormalised":
                out[:, hs] = rne_bf16(torch.einsum("hqk,khd->qhd", rne_bf16(e), v[:, hs]) / l[:, :, 0].transpose(0, 1)[:, :, None])
            elif form == "normalised":
                out[:, hs] = rne_bf16(torch.einsum("hqk,khd->qhd", rne_bf16(p), v[:, hs]))
            else:
                out[:, hs] = torch.einsum("hqk,khd->qhd", p, v[:, hs])
        if want_bound:
            o = outs[forms.index(None)][:, hs]
            d = hd * E_F32 * scale * torch.einsum("qhd,khd->hqk", q[:, hs].abs(), k[:, hs].abs()) + 4 * E_F32 * sc.abs()
            delta = d.masked_fill(~valid[None, None, :], 0.0).max(dim=-1).values.transpose(0, 1)[:, :, None]       # [n, h, 1]
            A = torch.einsum("hqk,khd->qhd", p, v[:, hs].abs())
            bound[:, hs] = U_BF16 * (A + o.abs()) + A * (U_BF16 ** 2 + 2 * delta + (n + 8) * E_F32)
    return outs, bound


DEFECTS = ["unmask_first", "unmask_edge", "unmask_last", "drop_last_key", "kv_head_off_by_one", "exp2_of_ln", "masked_row_is_mean_v",
           "swap_key_blocks", "rope_partner_next"]


def _unmask_index(valid, which):
    """Index of the masked key whose flag the defect ignores, or None when the sequence has no such key (or no valid key at all:
    that is the `masked_row_is_mean_v` defect's business)."""
    masked = (~valid).nonzero().flatten().tolist()
    if not masked or not bool(valid.any()):
        return None
    if which == "unmask_first":
        return masked[0]
    if which == "unmask_last":
        return masked[-1]
    edge = [j for j in masked if j % 32 in (0, 31)]
    return edge[0] if edge else None


def compute(c, device="cpu", form=None, defect=None, want_bound=False, only_t0=None, forms=None):
    """Yields (t0, n, out [n, nh hd], bound or None) float64 on the CPU per non-empty sequence: the float64 reference (form None) or
    ideally rounded arithmetic (form 'normalised' / 'unnormalised'), optionally with one of DEFECTS applied.  With a defect,
    only the sequences that contain its feature are yielded.  only_t0: just the sequence that starts at that token row.  forms: several forms from one
    pass over the scores; `out` is then a list, one output per form."""
    forms = (form,) if forms is None else tuple(forms)
    assert defect is None or defect in DEFECTS
    nh, nkv, hd = c["nh"], c["nkv"], c["hd"]
    G = nh // nkv
    q, k, v = _operands(c, device, rope_partner_next=(defect == "rope_partner_next"))
    kv_of = torch.arange(nh, device=device) // G
    if defect == "kv_head_off_by_one":
        assert nkv > 1
        kv_of = (kv_of + 1) % nkv
    key_valid = c["key_valid"].to(device).bool()
    for t0, n in sequences(c["lens"]):
        if n == 0 or (only_t0 is not None and t0 != only_t0):
            continue
        sl = slice(t0, t0 + n)
        valid = key_valid[sl].clone()
        kk, vv = k[sl][:, kv_of], v[sl][:, kv_of]
        if defect in ("unmask_first", "unmask_edge", "unmask_last"):
            j = _unmask_index(valid, defect)
            if j is None:
                continue
            valid[j] = True
        elif defect == "drop_last_key":
            if n < 2 or not bool(valid[n - 1]) or int(valid.sum()) < 2:
                continue
            valid[n - 1] = False
        elif defect == "swap_key_blocks":
            if n < 64:
                continue
            perm = torch.cat([torch.arange(32, 64), torch.arange(0, 32), torch.arange(64, n)]).to(device)
            vv = vv[perm]          # the weights of block 0 meet the values of block 1 and the other way round
        elif defect == "masked_row_is_mean_v" and bool(valid.any()):
            continue
        if not bool(valid.any()):
            o = vv.mean(dim=0, keepdim=True).expand(n, nh, hd) if defect == "masked_row_is_mean_v" else torch.zeros_like(q[sl])
            os_, b = [o if f is None else rne_bf16(o) for f in forms], (torch.zeros_like(q[sl]) if want_bound else None)
        else:
            os_, b = _attend(q[sl], kk, vv, valid, hd, forms, want_bound, exp2_of_ln=(defect == "exp2_of_ln"))
        os_ = [o.reshape(n, nh * hd).cpu() for o in os_]
        yield t0, n, (os_[0] if len(os_) == 1 else os_), (b.reshape(n, nh * hd).cpu() if want_bound else None)


def reference(c, device="cpu"):
    """(ref, bound): float64 [T, nh hd] on the CPU; rows of an empty or fully masked sequence: ref 0, bound 0."""
    T = sum(c["lens"])
    ref, bound = torch.zeros((T, c["nh"] * c["hd"]), dtype=torch.float64), torch.zeros((T, c["nh"] * c["hd"]), dtype=torch.float64)
    for t0, n, o, b in compute(c, device, want_bound=True):
        ref[t0:t0 + n], bound[t0:t0 + n] = o, b
    return ref, bound


def weight_of_the_other_keys(c, device="cpu"):
    """`known` cases: the largest float64 softmax weight, over every (row, head), of all keys but the heaviest one together."""
    nh, G, hd = c["nh"], c["nh"] // c["nkv"], c["hd"]
    q, k, _ = _operands(c, device)
    worst = 0.0
    for t0, n in sequences(c["lens"]):
        if n < 2:
            continue
        sc = torch.einsum("qhd,khd->hqk", q[t0:t0 + n], k[t0:t0 + n].repeat_interleave(G, dim=1)) / math.sqrt(hd)
        p = torch.softmax(sc, dim=-1)
        p.scatter_(-1, p.argmax(dim=-1, keepdim=True), 0.0)
        worst = max(worst, float(p.sum(dim=-1).max()))
    return worst


def sdpa_bf16_cpu(c):
    """The yardstick of the measured table: torch's scaled_dot_product_attention on the CPU on the bf16 tensors (rotated for a
    rope row) with a boolean key mask - the arithmetic of the reference's autocast pass.  float64 [T, nh hd]; rows of a
    fully masked sequence are NaN there and returned as NaN."""
    nh, hd, G = c["nh"], c["hd"], c["nh"] // c["nkv"]
    q, k, v = (x.bfloat16() for x in _operands(c, "cpu"))
    out = torch.full((sum(c["lens"]), nh, hd), float("nan"), dtype=torch.float64)
    for t0, n in sequences(c["lens"]):
        sl = slice(t0, t0 + n)
        if n == 0 or not bool(c["key_valid"][sl].any()):
            continue
        kk, vv = k[sl].repeat_interleave(G, dim=1), v[sl].repeat_interleave(G, dim=1)
        o = torch.nn.functional.scaled_dot_product_attention(q[sl].transpose(0, 1)[None], kk.transpose(0, 1)[None], vv.transpose(0, 1)[None],
                                                             attn_mask=c["key_valid"][sl].bool()[None, None, None, :])
        out[sl] = o[0].transpose(0, 1).double()
    return out.reshape(-1, nh * hd)


def worst_ratio(out, ref, bound):
    """Largest |out - ref| / bound over the elements with a positive bound (nan-free `out` expected there)."""
    keep = bound > 0
    return float(((out.double() - ref).abs()[keep] / bound[keep]).max()) if bool(keep.any()) else 0.0


if __name__ == "__main__":
    # the torch column of the measured table in test_attention_bf16_gpu.py (CPU only)
    for row_name in ROWS:
        for kind_name in ("lengths", "masks", "large"):
            worst = 0.0
            for geometry in GEOMETRIES:
                cs = case(row_name, kind_name, *geometry)
                rf, bd = reference(cs)
                y = sdpa_bf16_cpu(cs)
                ok = ~torch.isnan(y)
                worst = max(worst, float(((y - rf).abs()[ok & (bd > 0)] / bd[ok & (bd > 0)]).max()))
            print(f"{row_name:14s} {kind_name:8s} torch bf16 SDPA (CPU) max |err| / bound = {worst:.3f}", flush=True)
