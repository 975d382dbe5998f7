"""Document filters of the searches, in one place: allow-lists of positions (`subset=`), bitmaps over positions (`mask=`, one for all
queries; `masks=` + `query_group=`, one per group of queries), and the conversions between them (sr_doc_mask_from_list,
sr_doc_list_from_mask, sr_doc_mask_remap).  scoring.py re-exports the public names.

A bitmap argument is resolved in two steps, because the first must work without a device:

  mask_argument      host only: packed words (int32 / uint32) or bool flags, the dtype, the rank, at least one group (2-D), and - for packed
                     input alone - the word count against the number of bits the index expects (asked of the index only then)
  mask_on_device     (int32 words with a valid pointer, n_bits) on a device: packed words are moved as they are (a tensor already there is
                     not copied), flags are packed there and their own length is n_bits, which the library compares with the index

Order of checks of a filtered search, pinned by tests that run without a device and with queries=None:

  1. one filter only ("subset or mask, not both": one_filter)
  2. the filter's host step (mask_argument)
  3. the queries' dtype and shape
  4. query_group against the number of queries (query_group_argument)
  5. the queries' device
  6. only then anything that uploads, or asks the library for id_end (asked before only for packed input, in step 2)
"""
import ctypes
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib


# ------------------------------------------------------------------------------------------ C-ABI plumbing (shared with scoring.py)
def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _to_dev(x, dt, device):
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x))
    elif not torch.is_tensor(x):
        x = torch.as_tensor(x)
    return x.to(device=device, dtype=dt).contiguous()


def _valid(t):
    """t, or one zero of its type where t is empty: a valid pointer for the C ABI."""
    return t if t.numel() else torch.zeros(1, dtype=t.dtype, device=t.device)


def _call(device, name, *args, stream=True, lib=None):
    """One C-ABI call on `device` (the library allocates its workspace on the current device): entry `name` with `args`, then torch's
    current stream of that device where the entry takes one (stream=True: it is the last argument of every such entry); the status goes
    through _lib.check under the entry's name."""
    with torch.cuda.device(device):
        fn = getattr(_lib.load() if lib is None else lib, name)
        _lib.check(fn(*args, _lib.stream_ptr()) if stream else fn(*args), name)


def _cuda_device(t=None):
    """The device of a cuda tensor, else the current one."""
    return t.device if torch.is_tensor(t) and t.is_cuda else torch.device("cuda", torch.cuda.current_device())


# ------------------------------------------------------------------------------------------------------------------- allow-lists
def _subset(subset, device):
    """(int64 device tensor with a valid pointer, m) of an allow-list for the *_search_subset entry points; its order and content are
    checked by the kernels."""
    subset = _to_dev(subset, torch.int64, device)
    if subset.dim() != 1:
        raise ValueError(f"expected a 1-D subset, got {tuple(subset.shape)}")
    return _valid(subset), subset.numel()


def allowed_positions(allowed_ids, position_of, what="document id"):
    """External document ids (any order, duplicates allowed) -> sorted unique positions, np.int64: the allow-list the subset searches take.
    position_of maps an id to its position (a dict's .get, or any callable that returns None for an unknown id); an unknown id raises
    ValueError naming it."""
    out = set()
    for d in allowed_ids:
        p = position_of(d)
        if p is None:
            raise ValueError(f"allowed_ids: unknown {what} {d!r}")
        out.add(int(p))
    return np.fromiter(sorted(out), dtype=np.int64, count=len(out))


def allowed_positions_on(allowed_ids, inverse, device, skip_unknown=False):
    """allowed_positions through an inverse id map (rerank.InverseIdMap: str(id) -> position), as an int64 tensor on `device`.
    skip_unknown: an id the map does not hold is left out instead of raising."""
    position_of = lambda d: inverse.pos.get(str(d))      # noqa: E731
    if skip_unknown:
        allowed_ids = [d for d in allowed_ids if position_of(d) is not None]
    return torch.from_numpy(allowed_positions(allowed_ids, position_of)).to(device)


def read_allowed_ids_file(path):
    """One document id per line (surrounding white space and empty lines ignored) -> list of str, in file order."""
    with open(path) as f:
        return [line.strip() for line in f if line.strip()]


def one_filter(who, allowed_masks=None, query_group=None, **filters):
    """The argument rules of the filtered searches, checked before anything is uploaded: at most one of `filters` (the one-for-all-queries
    filters, by keyword: subset / mask, or allowed_ids / allowed_mask), not together with the per-group pair, whose two halves go together."""
    given = [name for name, value in filters.items() if value is not None]
    if len(given) > 1:
        raise ValueError(f"{who}: pass {' or '.join(filters)}, not both")
    if (allowed_masks is not None or query_group is not None) and given:
        raise ValueError(f"{who}: pass allowed_masks / query_group or one filter for all queries ({', '.join(filters)}), not both")
    if (allowed_masks is None) != (query_group is None):
        raise ValueError(f"{who}: allowed_masks and query_group go together (one bitmap per group, one group id per query)")


class Filter(NamedTuple):
    """A filter that is resolved and on the device: what the retrieval classes hand down, once per call."""
    kind: str                                   # "subset": positions int64; "mask": packed words; "groups": packed words [G, W] + group ids
    data: torch.Tensor
    groups: Optional[torch.Tensor] = None       # int64 [nq], kind "groups" only


# ----------------------------------------------------------------------------------------------------------------------- bitmaps
def pack_doc_mask(allowed):
    """A boolean array over document indices -> the bitmap the masked search takes: bit (i & 31) of word i >> 5 is allowed[i], the unused
    bits of the last word are 0 (include/sr_hip.h sr_dense_search_masked).  A numpy array is packed on the host and comes back as
    np.uint32 [ceil(n / 32)]; a torch tensor is packed on its own device and comes back as int32 words (torch has no arithmetic on
    uint32; the bits are the same)."""
    if torch.is_tensor(allowed):
        if allowed.dim() != 1:
            raise ValueError(f"expected a 1-D boolean mask, got {tuple(allowed.shape)}")
        n = allowed.numel()
        bits = torch.zeros(((n + 31) // 32) * 32, dtype=torch.int64, device=allowed.device)
        bits[:n] = allowed.to(torch.bool)
        weights = torch.ones(32, dtype=torch.int64, device=allowed.device) << torch.arange(32, dtype=torch.int64, device=allowed.device)
        return (bits.view(-1, 32) * weights).sum(dim=1).to(torch.int32)      # int64 -> int32 keeps the low 32 bits
    allowed = np.asarray(allowed)
    if allowed.ndim != 1:
        raise ValueError(f"expected a 1-D boolean mask, got {allowed.shape}")
    n_words = (allowed.size + 31) // 32
    raw = np.zeros(4 * n_words, dtype=np.uint8)
    packed = np.packbits(allowed.astype(bool), bitorder="little")         # bit i & 7 of byte i >> 3
    raw[:packed.size] = packed
    return raw.view("<u4").astype(np.uint32)                              # little-endian words: bit i & 31 of word i >> 5


def pack_doc_masks(flags, device=None):
    """A bool [G, n_bits] tensor or array -> the stacked bitmaps the grouped search takes (include/sr_hip.h sr_dense_search_grouped): int32
    [G, ceil(n_bits / 32)], row g = pack_doc_mask(flags[g]).  Packed on `device` (None: where a tensor lives; an array on the host), a
    few rows at a time, so the unpacked intermediate stays at 256 MB however many groups there are."""
    if not torch.is_tensor(flags):
        flags = torch.from_numpy(np.ascontiguousarray(np.asarray(flags), dtype=bool))
    if flags.dim() != 2:
        raise ValueError(f"expected a 2-D boolean [groups, n_bits] mask, got {tuple(flags.shape)}")
    if flags.dtype != torch.bool:
        raise ValueError(f"expected a boolean [groups, n_bits] mask, got {flags.dtype}")
    device = flags.device if device is None else torch.device(device)
    n_groups, n = flags.shape
    n_words = (n + 31) // 32
    out = torch.empty((n_groups, n_words), dtype=torch.int32, device=device)
    if n_words == 0:
        return out
    weights = torch.ones(32, dtype=torch.int64, device=device) << torch.arange(32, dtype=torch.int64, device=device)
    rows = max(1, (1 << 25) // (32 * n_words))
    for g0 in range(0, n_groups, rows):
        part = flags[g0:g0 + rows].to(device)
        bits = torch.zeros((part.shape[0], 32 * n_words), dtype=torch.int64, device=device)
        bits[:, :n] = part
        out[g0:g0 + rows] = (bits.view(part.shape[0], n_words, 32) * weights).sum(dim=2).to(torch.int32)   # keeps the low 32 bits
    return out


def _is_packed(mask):
    """Packed bitmap words: an np.uint32 / np.int32 array, or an int32 / uint32 tensor."""
    if isinstance(mask, np.ndarray):
        return mask.dtype in (np.uint32, np.int32)
    return mask.dtype in (torch.int32, getattr(torch, "uint32", torch.int32))


def _mask_words(words, device, ndim=1):
    """Packed bitmap words (np.uint32 / np.int32 array, or an int32 / uint32 tensor) -> a contiguous int32 tensor on the device."""
    if not _is_packed(words):
        raise ValueError(f"packed mask words must be uint32 or int32, got {words.dtype}")
    if isinstance(words, np.ndarray):
        words = torch.from_numpy(np.ascontiguousarray(words).view(np.int32))
    elif words.dtype != torch.int32:
        words = words.view(torch.int32)
    if words.dim() != ndim:
        raise ValueError(f"expected {ndim}-D mask words, got {tuple(words.shape)}")
    return words.to(device).contiguous()


def mask_argument(mask, n_bits_of, what, ndim=1):
    """The host step of a bitmap argument (`mask=`: ndim 1; `masks=`: ndim 2, [groups, ...]): (mask as tensor / array, n_bits), n_bits =
    None for bool flags.  n_bits_of() - asked only for packed input - is the number of bits the index expects (`what` names it in the
    message); the word count is verified against it."""
    if not torch.is_tensor(mask) and not isinstance(mask, np.ndarray):
        mask = np.asarray(mask)
    packed = _is_packed(mask)
    if not packed and mask.dtype not in (np.bool_, torch.bool):
        raise ValueError(("mask must be a bool tensor / array over the documents, or packed int32 / uint32 words (pack_doc_mask), got " if ndim == 1
                          else "masks must be a bool [groups, n_bits] tensor / array, or packed int32 / uint32 words [groups, words] "
                          "(pack_doc_masks), got ") + str(mask.dtype))
    if len(mask.shape) != ndim:
        raise ValueError(f"expected a 1-D mask, got {tuple(mask.shape)}" if ndim == 1 else f"expected 2-D masks [groups, ...], got {tuple(mask.shape)}")
    if ndim == 2 and mask.shape[0] < 1:
        raise ValueError("masks must hold at least one group")
    if not packed:
        return mask, None
    n_bits = int(n_bits_of())
    if mask.shape[-1] != (n_bits + 31) // 32:
        raise ValueError(f"a packed mask of this index holds {(n_bits + 31) // 32} words ({what} = {n_bits}), got {mask.shape[-1]}")
    return mask, n_bits


def mask_on_device(mask, n_bits, device):
    """The device step of what mask_argument returned: (int32 words on the device with a valid pointer, n_bits).  Flags (n_bits None) are
    packed on the device and their own length is n_bits (the library compares it with the index)."""
    ndim = len(mask.shape)
    if n_bits is not None:
        return _valid(_mask_words(mask, device, ndim)), n_bits
    if ndim == 2:
        return _valid(pack_doc_masks(mask, device)), int(mask.shape[1])
    return _valid(pack_doc_mask(_to_dev(mask, torch.bool, device))), int(mask.shape[0])


def query_group_argument(query_group, nq):
    """query_group as given -> an int array / tensor of nq entries, checked without a device (the library checks the range)."""
    if not torch.is_tensor(query_group) and not isinstance(query_group, np.ndarray):
        query_group = np.asarray(query_group)
    is_int = (not query_group.dtype.is_floating_point and not query_group.dtype.is_complex and query_group.dtype != torch.bool) \
        if torch.is_tensor(query_group) else query_group.dtype.kind in "iu"
    if not is_int:
        raise ValueError(f"query_group must hold integer group ids, got {query_group.dtype}")
    if len(query_group.shape) != 1 or query_group.shape[0] != nq:
        raise ValueError(f"query_group must hold one group id per query ({nq}), got {tuple(query_group.shape)}")
    return query_group


def group_ids_int32(query_group, device):
    """Group ids as the library takes them: int32 on the device."""
    # an id that does not fit int32 must not wrap into range: it is clamped to one the library rejects
    return _to_dev(query_group, torch.int64, device).clamp(-1, 2 ** 31 - 1).to(torch.int32)


def check_group_ids(who, groups, n_groups):
    """The library's range check of the group ids, for a driver that indexes by them itself: groups an int64 tensor [nq]."""
    bad = torch.nonzero((groups < 0) | (groups >= n_groups))
    if bad.numel():
        raise ValueError(f"{who}: query {int(bad[0])} is in group {int(groups[int(bad[0])])}, outside [0, {n_groups})")


def group_argument(masks, query_group, nq_of, n_bits_of, what):
    """The host step of a masks= / query_group= pair, in the order listed at the top: mask_argument (2-D), then nq_of() - the caller's
    check of its queries' dtype and shape, which returns their number - then query_group_argument."""
    masks = mask_argument(masks, n_bits_of, what, ndim=2)
    return masks, query_group_argument(query_group, nq_of())


def group_filter(argument, device):
    """The device step of what group_argument returned: ("_grouped", words int32 [G, W], G, n_bits, group ids int32 [nq]), tensors on the
    device with valid pointers."""
    masks, query_group = argument
    words, n_bits = mask_on_device(*masks, device)
    return "_grouped", words, int(masks[0].shape[0]), n_bits, _valid(group_ids_int32(query_group, device))


def range_filter_kwargs(filt, nq, n_bits, device):
    """A resolved Filter (None: none) -> the filter keywords of the index classes' range_search over nq queries: masks / query_group for
    groups, else mask - an allow-list becomes its bitmap over [0, n_bits) (doc_mask_from_list)."""
    if filt is not None and filt.kind == "groups":
        if filt.groups.numel() != nq:
            raise ValueError(f"range_search: query_group must hold one group id per query ({nq}), got {filt.groups.numel()}")
        return dict(masks=filt.data, query_group=filt.groups)
    if filt is not None and filt.kind == "subset":
        return dict(mask=doc_mask_from_list(filt.data, n_bits, device=device))
    return dict(mask=None if filt is None else filt.data)


class FilterKeywords:
    """The filter keywords of the retrieval classes (allowed_ids, allowed_mask, allowed_masks + query_group), resolved and uploaded once
    per call.  A class that mixes this in has inverse_id_map() and states _filter_space() -> (device, number of positions, what a position
    is called in a message): DenseFlatIndexer filters index positions, SparseRetrieval the document positions of the inverted index."""

    def allowed_subset(self, allowed_ids):
        """External ids (any order, duplicates allowed) -> the sorted unique positions as an int64 tensor on the index's device: the
        allow-list of the searches, uploaded once per call.  An unknown id: ValueError naming it."""
        return allowed_positions_on(allowed_ids, self.inverse_id_map(), self._filter_space()[0])

    def allowed_mask_words(self, allowed_mask):
        """A boolean array / tensor with one flag per position -> the packed bitmap on the index's device, uploaded and packed once per
        call (flags_to_words)."""
        device, n, what = self._filter_space()
        return flags_to_words(allowed_mask, n, what, device)

    def allowed_group_words(self, allowed_masks, query_group):
        """allowed_masks bool [G, positions] and query_group int [number of queries] (both or neither) -> (packed bitmaps int32 [G, W] on
        the index's device, group ids int64 on the device), packed once per call (flags_to_words)."""
        device, n, what = self._filter_space()
        words = flags_to_words(allowed_masks, (None, n), what, device)
        groups = query_group if isinstance(query_group, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(query_group))
        if groups.dim() != 1 or groups.dtype.is_floating_point or groups.dtype == torch.bool:
            raise ValueError(f"query_group must hold one integer group id per query, got {groups.dtype} {tuple(groups.shape)}")
        return words, groups.to(device=device, dtype=torch.int64)

    def _resolve(self, who, allowed_ids=None, allowed_mask=None, allowed_masks=None, query_group=None):
        """The filter keywords of a search -> a Filter on the index's device (None: no filter), resolved and uploaded once per call; the
        argument rules (one_filter) come before anything is uploaded."""
        one_filter(who, allowed_masks, query_group, allowed_ids=allowed_ids, allowed_mask=allowed_mask)
        if allowed_ids is not None:
            return Filter("subset", self.allowed_subset(allowed_ids))
        if allowed_mask is not None:
            return Filter("mask", self.allowed_mask_words(allowed_mask))
        if allowed_masks is not None:
            return Filter("groups", *self.allowed_group_words(allowed_masks, query_group))
        return None


def flags_to_words(flags, n, what, device):
    """Bool flags over positions, given by a caller of the retrieval classes -> the packed bitmap on `device`, uploaded and packed once:
    [n] flags (`allowed_mask`) -> int32 [W]; [G, n] flags with G >= 1 (`allowed_masks`) -> int32 [G, W].  `what` names a position in the
    message ("index position", "document position"); the rank is that of the expected shape `n` = n or (None, n)."""
    grouped = isinstance(n, tuple)
    n = n[1] if grouped else n
    flags = flags if torch.is_tensor(flags) else torch.from_numpy(np.ascontiguousarray(flags, dtype=bool))
    if grouped:
        if flags.dim() != 2 or flags.shape[0] < 1 or flags.shape[1] != n:
            raise ValueError(f"allowed_masks must hold one row of flags per group, one flag per {what} ({n}), got {tuple(flags.shape)}")
        return pack_doc_masks(flags.to(torch.bool), device)
    if flags.dim() != 1 or flags.numel() != n:
        raise ValueError(f"allowed_mask must hold one flag per {what} ({n}), got {tuple(flags.shape)}")
    return pack_doc_mask(flags.to(device=device, dtype=torch.bool))


def doc_mask_from_list(ids, n_bits, device=None):
    """Document indices (int64, any order, repeats allowed; tensor / array / list) -> the bitmap over [0, n_bits) as int32 words on the
    device (sr_doc_mask_from_list).  An entry outside [0, n_bits): ValueError."""
    _lib.require_gpu()
    device = _cuda_device() if device is None else torch.device(device)
    ids, m = _subset(ids, device)
    n_bits = int(n_bits)
    words = torch.empty((max(1, (n_bits + 31) // 32),), dtype=torch.int32, device=device)
    _call(device, "sr_doc_mask_from_list", _ptr(ids), m, _ptr(words), n_bits)
    return words[:(n_bits + 31) // 32]


def doc_list_from_mask(words, n_bits, capacity=None):
    """The set bits below n_bits of a packed bitmap (int32 / uint32 words, tensor or array) as an ascending int64 tensor on the device
    (sr_doc_list_from_mask).  capacity (None: room for every bit): at most that many entries are written; returns (list, count) with
    count = the number of set bits whatever the capacity."""
    _lib.require_gpu()
    words = _mask_words(words, _cuda_device(words))
    n_bits = int(n_bits)
    if words.numel() < (n_bits + 31) // 32:
        raise ValueError(f"{n_bits} bits need {(n_bits + 31) // 32} words, got {words.numel()}")
    cap = n_bits if capacity is None else int(capacity)
    out = torch.empty((max(1, cap),), dtype=torch.int64, device=words.device)
    count = torch.zeros(1, dtype=torch.int64, device=words.device)
    words = _valid(words)
    _call(words.device, "sr_doc_list_from_mask", _ptr(words), n_bits, _ptr(out), cap, _ptr(count))
    c = int(count.item())
    return out[:min(c, cap)], c


def doc_mask_remap(words, n_src_bits, map, n_dst_bits):
    """A bitmap carried over to another numbering (sr_doc_mask_remap): bit i of the result = bit map[i] of `words` (packed int32 / uint32
    words over n_src_bits bits) where 0 <= map[i] < n_src_bits, else 0; map int64 [n_dst_bits].  Returns int32 words
    [ceil(n_dst_bits / 32)] on the device."""
    _lib.require_gpu()
    device = _cuda_device(words)
    words = _mask_words(words, device)
    n_src_bits, n_dst_bits = int(n_src_bits), int(n_dst_bits)
    if words.numel() < (n_src_bits + 31) // 32:
        raise ValueError(f"{n_src_bits} bits need {(n_src_bits + 31) // 32} words, got {words.numel()}")
    map = _to_dev(map, torch.int64, device)
    if map.dim() != 1 or map.numel() != n_dst_bits:
        raise ValueError(f"expected a map of {n_dst_bits} entries, got {tuple(map.shape)}")
    out = torch.empty((max(1, (n_dst_bits + 31) // 32),), dtype=torch.int32, device=device)
    words, map = _valid(words), _valid(map)
    _call(device, "sr_doc_mask_remap", _ptr(words), n_src_bits, _ptr(map), n_dst_bits, _ptr(out))
    return out[:(n_dst_bits + 31) // 32]
