"""sr_doc_mask_remap (scoring.doc_mask_remap): a bitmap carried over to another numbering, against three lines of numpy."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _reference(src_bits, map_, n_dst):
    ok = (map_ >= 0) & (map_ < len(src_bits))
    dst = np.zeros(n_dst, bool)
    dst[ok] = src_bits[map_[ok]]
    return dst


@pytest.mark.parametrize("n_src", [1, 45, 8200])
@pytest.mark.parametrize("n_dst", [0, 1, 31, 32, 33, 8193])
def test_remap_equals_numpy(n_dst, n_src):
    from scaling_retriever_amd.scoring import doc_mask_remap, pack_doc_mask
    rng = np.random.default_rng(100 * n_dst + n_src)
    src = rng.random(n_src) < 0.5
    words = pack_doc_mask(src).copy()
    if n_src % 32:
        words[-1] |= np.uint32((0xFFFFFFFF << (n_src % 32)) & 0xFFFFFFFF)      # bits at or beyond n_src_bits: never a source
    # entries: valid (with repeats of a source bit), -1, other negatives, n_src and beyond
    map_ = rng.integers(0, n_src, size=n_dst).astype(np.int64)
    kind = rng.integers(0, 6, size=n_dst)
    map_[kind == 0] = -1
    map_[kind == 1] = n_src + rng.integers(0, 100, size=int((kind == 1).sum()))
    map_[kind == 2] = int(np.nonzero(src)[0][0]) if src.any() else 0            # many entries name one source bit
    if n_dst > 2:
        map_[0], map_[1], map_[2] = -(1 << 40), n_src, (1 << 40)
    want = pack_doc_mask(_reference(src, map_, n_dst))
    for form in (words, torch.from_numpy(words.view(np.int32)).cuda()):
        got = doc_mask_remap(form, n_src, map_, n_dst)
        assert got.dtype == torch.int32 and got.numel() == (n_dst + 31) // 32
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want)
    with pytest.raises(ValueError):
        doc_mask_remap(words, n_src, map_[:-1] if n_dst else np.zeros(1, np.int64), n_dst)


def test_identity_and_permutation():
    from scaling_retriever_amd.scoring import doc_mask_remap, pack_doc_mask
    n = 8193
    rng = np.random.default_rng(9)
    src = rng.random(n) < 0.3
    words = pack_doc_mask(src)
    assert np.array_equal(doc_mask_remap(words, n, np.arange(n), n).cpu().numpy().view(np.uint32), words)
    perm = rng.permutation(n)
    assert np.array_equal(doc_mask_remap(words, n, perm, n).cpu().numpy().view(np.uint32), pack_doc_mask(src[perm]))
    with pytest.raises(ValueError, match="words"):
        doc_mask_remap(words[:-1], n, perm, n)
