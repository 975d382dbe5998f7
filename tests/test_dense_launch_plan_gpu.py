"""The launch plan of a dense search: how many kernel launches a search makes and how many row bytes they cover.

Results are exact whatever the chunking, so a scan driver that cuts the rows differently passes every result test and shows
only as a speed change.  The handle counts its launches (sr_dense_index_profile / _profile_read); here one search per case is
compared with a restatement of the schedule:

  streaming kernel (<= 64 queries): launches of step rows, step = 65 536 doubling up to cap = min(limit / (8 nq), 2^22) rounded
      down to 128 rows;
  tiled kernels and the 16-bit passes: step = max(ceil((k + 1024) / 256) * 256, 256 * ceil(256 / qtiles)) doubling up to
      chunk = 256 * unit * ceil(wgs / (unit * qtiles)), unit = 256 / gcd(256, qtiles), wgs = 2 048 (7 168 for the 16-bit
      passes), and at most limit / (8 nq) rounded down to 256 rows (at least 256);
  the doubling carries across segment boundaries; a launch never spans two segments.

The certified filter's pass runs with k' = max(3 k, k + 2 048) candidates per query and reports 4 bytes per row element.
"""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

WS_DEFAULT = 4 << 30
N = 200_000


def _stream_steps(nq, limit):
    cap = max(min(limit // (8 * nq), 1 << 22) // 128 * 128, 128)
    return min(65536, cap), cap


def _tiled_steps(nq, k, limit, wgs):
    tn = 256 if nq > 128 else 128 if nq > 64 else 64 if nq > 32 else 32
    qtiles = -(-nq // tn)
    unit = 256 // math.gcd(256, qtiles)
    chunk = 256 * unit * -(-wgs // (unit * qtiles))
    chunk = min(chunk, max(limit // (8 * nq) // 256 * 256, 256))
    step = max(-(-(k + 1024) // 256) * 256, 256 * -(-256 // qtiles))
    return min(step, chunk), chunk


def _launches(segments, step, cap):
    n = 0
    for rows in segments:
        r0 = 0
        while r0 < rows:
            r0 = min(r0 + step, rows)
            step = min(2 * step, cap)
            n += 1
    return n


@pytest.fixture(scope="module")
def rows():
    g = torch.Generator(device="cuda").manual_seed(7)
    return {H: torch.randn((N, H), generator=g, device="cuda", dtype=torch.float32) for H in (64, 128)}


def _profiled_search(idx, Q, k):
    from scaling_retriever_amd import _lib
    lib = _lib.load()
    _lib.check(lib.sr_dense_index_profile(idx._h, 1))
    idx.search(Q, k)
    torch.cuda.synchronize()
    _lib.check(lib.sr_dense_index_profile(idx._h, 0))
    n_l, ms, fl, by = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    _lib.check(lib.sr_dense_index_profile_read(idx._h, ctypes.byref(n_l), ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by)))
    return n_l.value, by.value


def _index(rows, H, segments, precision=None):
    from scaling_retriever_amd.scoring import DenseIndexHIP
    idx = DenseIndexHIP(H)
    if precision:
        idx.set_precision(precision)
    r0 = 0
    for n in segments:
        idx.add_device_rows(rows[H][r0:r0 + n])
        r0 += n
    return idx


def _queries(nq, H):
    g = torch.Generator(device="cuda").manual_seed(100 + nq)
    return torch.randn((nq, H), generator=g, device="cuda", dtype=torch.float32)


SEGS = [(N,), (150_000, 50_000)]


@pytest.mark.parametrize("segments", SEGS)
def test_streaming_launch_plan(rows, segments):
    nq, k, H = 16, 10, 64
    idx = _index(rows, H, segments)
    n_l, by = _profiled_search(idx, _queries(nq, H), k)
    want = _launches(segments, *_stream_steps(nq, WS_DEFAULT))
    print(f"streaming nq={nq} segments={segments}: n_launches={n_l} expected={want} d_bytes={by:.0f}")
    assert n_l == want
    assert by == N * H * 4


@pytest.mark.parametrize("segments", SEGS)
@pytest.mark.parametrize("nq", [70, 300])
def test_tiled_launch_plan(rows, nq, segments):
    k, H = 10, 64
    idx = _index(rows, H, segments)
    n_l, by = _profiled_search(idx, _queries(nq, H), k)
    want = _launches(segments, *_tiled_steps(nq, k, WS_DEFAULT, 2048))
    print(f"tiled nq={nq} segments={segments}: n_launches={n_l} expected={want} d_bytes={by:.0f}")
    assert n_l == want
    assert by == N * H * 4


def test_tiled_batch_invariant_launch_plan(rows):
    nq, k, H = 16, 10, 64
    idx = _index(rows, H, (N,))
    idx.set_batch_invariant(True)
    n_l, by = _profiled_search(idx, _queries(nq, H), k)
    want = _launches((N,), *_tiled_steps(nq, k, WS_DEFAULT, 2048))
    print(f"tiled batch-invariant nq={nq}: n_launches={n_l} expected={want} d_bytes={by:.0f}")
    assert n_l == want
    assert by == N * H * 4


def test_tiled_workspace_cap_launch_plan(rows):
    """1 MiB of workspace for 300 queries: 436 candidate slots per query, so the cap - one 256-row tile per launch - decides."""
    nq, k, H, n = 300, 10, 64, 5000
    idx = _index(rows, H, (n,))
    idx.set_workspace_limit(1 << 20)
    n_l, by = _profiled_search(idx, _queries(nq, H), k)
    step, chunk = _tiled_steps(nq, k, 1 << 20, 2048)
    assert (step, chunk) == (256, 256)
    want = _launches((n,), step, chunk)
    print(f"tiled capped nq={nq}: n_launches={n_l} expected={want} d_bytes={by:.0f}")
    assert n_l == want == 20
    assert by == n * H * 4


def test_filter_pass_launch_plan(rows):
    """n_launches counts the filter's pass and the launches of any exact re-do: with Gaussian rows no query is re-done, which is
    asserted, and the count is the pass alone."""
    nq, k, H = 200, 10, 128
    idx = _index(rows, H, (N,), "fp32_filtered")
    n_l, by = _profiled_search(idx, _queries(nq, H), k)
    kp = min(max(3 * k, k + 2048), 4096)
    want = _launches((N,), *_tiled_steps(nq, kp, WS_DEFAULT, 7168))
    print(f"filter pass nq={nq}: n_launches={n_l} expected={want} d_bytes={by:.0f} stats={idx.filter_query_stats()}")
    assert idx.filter_query_stats() == (nq, 0)
    assert n_l == want
    assert by == N * H * 4


def test_bf16x3_launch_plan(rows):
    nq, k, H = 200, 10, 64
    idx = _index(rows, H, (N,), "bf16x3")
    n_l, by = _profiled_search(idx, _queries(nq, H), k)
    want = _launches((N,), *_tiled_steps(nq, k, WS_DEFAULT, 7168))
    print(f"bf16x3 nq={nq}: n_launches={n_l} expected={want} d_bytes={by:.0f}")
    assert n_l == want
    assert by == N * H * 4
