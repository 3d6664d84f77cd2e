"""The token movement of the expert-sharded forward (csrc/dga_rows.hip) kernel by kernel, at the sizes where its own machinery
starts: dga_route_slots with several workgroups reserving in the same buckets, dga_route_tokens with several groups per thread,
dga_copy_rows / dga_copy_rows2 with a row split over several workgroups and on each fall-back from 16-byte lanes to bytes.  All
checks are exact: integers against the contract (tests/route_cases.py, proved on the numpy model in tests/test_route_model.py),
bytes against torch indexing on the same device tensors.  Every destination lies inside a wider buffer of 0xA5 that is compared
whole, so a byte written outside the copied spans fails the case."""
import numpy as np
import pytest
import torch

import route_cases as R

pytestmark = pytest.mark.gpu
E_SHAPE, E_ALIGN, E_RANGE = -2, -4, -9        # include/dga_hip.h


# ---- dga_route_slots

def _route_through(dga):
    def route(keys, key_stride, key_off, rows, buckets, cap, counts, dest, overflow, key_div=1, key_sub=0, key_mul=1, zero_counts=True,
              tags=None, tag_stride=0, tag_off=0, inverse=None, inverse_base=0):
        dga.route_slots(keys, key_stride, rows, buckets, cap, counts, dest, overflow, key_div=key_div, key_sub=key_sub, key_mul=key_mul,
                        zero_counts=zero_counts, tags=tags, tag_stride_bytes=tag_stride, keys_byte_offset=key_off,
                        tags_byte_offset=tag_off, inverse=inverse, inverse_base=inverse_base)
        torch.cuda.synchronize()
    return route


@pytest.mark.parametrize("name", list(R.CASES))
def test_route_slots(dga, name):
    case = R.CASES[name]
    done = R.run_case(case, _route_through(dga), torch.device("cuda"), with_inverse=True)
    assert len(done) == len(case["calls"])
    if name == "hot-fits":
        assert done == [(0, 3 * R.ROWS_PER_BLOCK)]
    if name == "hot-cap5000":
        assert done == [(3 * R.ROWS_PER_BLOCK - 5000, 5000)]
    if name == "hot-cap0":
        assert done == [(3 * R.ROWS_PER_BLOCK, 0)]


def test_route_slots_refusals(dga):
    from deepgemm_ascend_amd import _lib
    L = _lib.lib()
    keys = torch.zeros(64, dtype=torch.int32, device="cuda")
    counts = torch.zeros(4100, dtype=torch.int32, device="cuda")
    dest = torch.full((16,), -5, dtype=torch.int64, device="cuda")
    overflow = torch.zeros(1, dtype=torch.int32, device="cuda")

    def call(key_ptr, key_stride, buckets=8, rows=16):
        return L.dga_route_slots(key_ptr, key_stride, rows, 1, 0, 1, buckets, 4, counts.data_ptr(), 1, dest.data_ptr(), None, 0,
                                 overflow.data_ptr(), None, 0, None)
    p = keys.data_ptr()
    assert call(p, 3) == E_SHAPE and call(p, 0) == E_SHAPE and call(p, -4) == E_SHAPE
    assert call(p, 6) == E_ALIGN and call(p + 2, 4) == E_ALIGN and call(p + 1, 8) == E_ALIGN
    assert call(p, 4, buckets=4097) == E_RANGE
    torch.cuda.synchronize()
    assert (dest == -5).all() and int(overflow[0]) == 0, "a refused call wrote its outputs"
    assert call(p, 4) == 0 and call(p + 4, 8, rows=8) == 0
    torch.cuda.synchronize()
    assert counts[:8].tolist() == [4, 0, 0, 0, 0, 0, 0, 0] and int(overflow[0]) == 12 + 4      # 16, then 8 rows of key 0 at cap 4


# ---- dga_route_tokens

def _check_route_tokens(dga, ids, G):
    counts, pos = dga.route_tokens(ids, G)
    torch.cuda.synchronize()
    ok = (ids >= 0) & (ids < G)
    assert torch.equal(counts, torch.bincount(ids[ok], minlength=G))
    assert (pos[~ok] == -1).all()
    valid = int(ok.sum())
    assert torch.equal(torch.sort(pos[ok]).values, torch.arange(valid, device="cuda"))      # a permutation of 0 .. valid - 1
    by_slot = torch.empty(valid, dtype=torch.int64, device="cuda")
    by_slot[pos[ok]] = ids[ok]
    assert (by_slot[1:] >= by_slot[:-1]).all()                                               # that sorts by expert


@pytest.mark.parametrize("G", [257, 1000, 4096])       # 2, 4 and 16 groups per thread of the prefix sum; trailing threads own none
def test_route_tokens_many_groups(dga, G):
    g = torch.Generator(device="cuda").manual_seed(G)
    _check_route_tokens(dga, torch.randint(0, G, (20000,), device="cuda", generator=g), G)


@pytest.mark.parametrize("G", [37, 1000])
def test_route_tokens_ids_out_of_range(dga, G):
    g = torch.Generator(device="cuda").manual_seed(G + 1)
    ids = torch.randint(0, G, (20000,), device="cuda", generator=g)
    u = torch.rand(20000, device="cuda", generator=g)
    below = torch.randint(-G, 0, (20000,), device="cuda", generator=g)
    above = torch.randint(G, 2 * G + 3, (20000,), device="cuda", generator=g)
    ids = torch.where(u < 0.05, below, torch.where(u < 0.10, above, ids))
    ids[17], ids[18], ids[19] = -(1 << 40), 1 << 40, G
    assert 0.05 < float(((ids < 0) | (ids >= G)).float().mean()) < 0.15
    _check_route_tokens(dga, ids, G)


def test_route_tokens_refuses_too_many_groups(dga):
    from deepgemm_ascend_amd import _lib
    ids = torch.zeros(8, dtype=torch.int64, device="cuda")
    counts = torch.full((4100,), -5, dtype=torch.int64, device="cuda")
    pos = torch.full((8,), -5, dtype=torch.int64, device="cuda")
    assert _lib.lib().dga_route_tokens(ids.data_ptr(), 8, 4097, counts.data_ptr(), pos.data_ptr(), None) == E_SHAPE
    torch.cuda.synchronize()
    assert (counts == -5).all() and (pos == -5).all()


# ---- dga_copy_rows / dga_copy_rows2

class _Rows:
    """`rows` rows at a byte stride with guard bytes before (at least a row, a multiple of 256 so that the stride alone decides the
    rows' alignment) and a guard row after: .view is the 2-D tensor a call gets, .whole the buffer that is compared."""

    def __init__(self, rows, stride, fill=None, seed=0):
        self.lead = lead = (stride + 255) // 256 * 256
        n = lead + (rows + 1) * stride
        if fill is None:
            g = torch.Generator(device="cuda").manual_seed(seed)
            self.whole = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)
        else:
            self.whole = torch.full((n,), fill, dtype=torch.uint8, device="cuda")
        self.view = self.whole[lead:lead + rows * stride].view(rows, stride)
        assert self.view.data_ptr() == self.whole.data_ptr() + lead and self.view.data_ptr() % 256 == 0

    def copy(self):
        c = _Rows.__new__(_Rows)
        c.whole, c.lead = self.whole.clone(), self.lead
        rows, stride = self.view.shape
        c.view = c.whole[c.lead:c.lead + rows * stride].view(rows, stride)
        return c

    def first_difference(self, want):
        bad = torch.nonzero(self.whole != want.whole).flatten()
        if bad.numel() == 0:
            return None
        at = int(bad[0]) - self.lead
        return f"{bad.numel()} bytes differ, the first in row {at // self.view.shape[1]} at byte {at % self.view.shape[1]} of it"


def _index(n, rows_in_tensor, seed, negatives):
    """n distinct rows of a tensor of rows_in_tensor rows, in a random order, with -1 at `negatives`."""
    ix = torch.from_numpy(np.random.default_rng(seed).permutation(rows_in_tensor)[:n].astype(np.int64))
    for i in negatives:
        if i < n:
            ix[i] = -1
    return ix.cuda()


def _expect(dst, src, dst_index, src_index, n, row_bytes, dst_off, src_off):
    """torch indexing on the copy `dst` (a _Rows): what the call must leave behind."""
    di = dst_index[:n] if dst_index is not None else torch.arange(n, device="cuda")
    si = src_index[:n] if src_index is not None else torch.arange(n, device="cuda")
    ok = (di >= 0) & (si >= 0)
    assert dst_off + row_bytes <= dst.view.shape[1] and src_off + row_bytes <= src.view.shape[1]
    assert int(di.max()) < dst.view.shape[0] and int(si.max()) < src.view.shape[0] and torch.unique(di[ok]).numel() == int(ok.sum())
    dst.view[di[ok], dst_off:dst_off + row_bytes] = src.view[si[ok], src_off:src_off + row_bytes]


def _run_copy_rows(dga, row_bytes, n, mode, dst_stride, src_stride, dst_off=0, src_off=0, extra_index=0, seed=0, off16=None):
    """One dga_copy_rows call: `mode` says which side is indexed; extra_index entries behind the first n (valid rows that no other
    entry names) must not be used.  off16: how many of the five things the 16-byte lanes need are no multiple of 16."""
    spare = 2                                      # rows of the indexed tensor that no index entry names
    dneg, sneg = ((1, 4), (2, 6)) if n > 4 else ((1,), ())
    dst_rows = n + extra_index + (spare if mode in ("scatter", "both") else 0)
    src_rows = n + extra_index + (spare if mode in ("gather", "both") else 0)
    dst, src = _Rows(dst_rows, dst_stride, fill=R.FILL), _Rows(src_rows, src_stride, seed=seed + 1)
    dst_index = _index(n + extra_index, dst_rows, seed + 2, dneg) if mode in ("scatter", "both") else None
    src_index = _index(n + extra_index, src_rows, seed + 3, sneg) if mode in ("gather", "both") else None
    if off16 is not None:                          # the case is about this path: 16-byte lanes need all five aligned
        five = (dst.view.data_ptr() + dst_off, src.view.data_ptr() + src_off, dst.view.stride(0), src.view.stride(0), row_bytes)
        assert sum(x % 16 != 0 for x in five) == off16, five
    want, src_before = dst.copy(), src.whole.clone()
    if n and row_bytes:
        _expect(want, src, dst_index, src_index, n, row_bytes, dst_off, src_off)
    dga.copy_rows(dst.view, src.view, dst_index, src_index, rows=n, row_bytes=row_bytes, dst_byte_offset=dst_off,
                  src_byte_offset=src_off)
    torch.cuda.synchronize()
    assert torch.equal(src.whole, src_before)
    if n and row_bytes:
        assert not torch.equal(want.whole, torch.full_like(want.whole, R.FILL)), "the case copies nothing"
    assert dst.first_difference(want) is None, dst.first_difference(want)


@pytest.mark.parametrize("mode", ["gather", "scatter"])
@pytest.mark.parametrize("row_bytes", [16384, 16400, 20480, 65536 + 16])     # 1 (four chunks per thread, exactly), 2, 2 and 5 parts
def test_copy_rows_long_rows_vector(dga, row_bytes, mode):
    _run_copy_rows(dga, row_bytes, 9, mode, row_bytes + 32, row_bytes + 48, seed=row_bytes, off16=0)


@pytest.mark.parametrize("mode", ["gather", "scatter"])
@pytest.mark.parametrize("row_bytes", [1025, 7411])                         # 2 and 8 parts of single bytes
def test_copy_rows_long_rows_scalar(dga, row_bytes, mode):
    _run_copy_rows(dga, row_bytes, 50, mode, row_bytes + 7, row_bytes + 16, seed=row_bytes)


@pytest.mark.parametrize("row_bytes,vec", [(64 * 1024 * 16 + 4096 + 16, True), (70001, False)])
def test_copy_rows_clamped_at_64_parts(dga, row_bytes, vec):
    """More than 64 x 1024 chunks (bytes) per row: 64 workgroups per row, a thread loops five times."""
    assert (row_bytes // (16 if vec else 1) + 1023) // 1024 > 64
    pad = 16 if vec else 3
    _run_copy_rows(dga, row_bytes, 3, "both", row_bytes + pad, row_bytes + 2 * pad, seed=5, off16=None if not vec else 0)


@pytest.mark.parametrize("what,kw", [
    ("nothing", dict(row_bytes=20480, dst_stride=20480 + 32, src_stride=20480 + 48, off16=0)),
    ("dst base", dict(row_bytes=20480, dst_stride=20480 + 32, src_stride=20480 + 48, dst_off=4, off16=1)),
    ("src base", dict(row_bytes=20480, dst_stride=20480 + 32, src_stride=20480 + 48, src_off=8, off16=1)),
    ("dst stride", dict(row_bytes=20480, dst_stride=20480 + 36, src_stride=20480 + 48, off16=1)),
    ("src stride", dict(row_bytes=20480, dst_stride=20480 + 32, src_stride=20480 + 40, off16=1)),
    ("row bytes", dict(row_bytes=20484, dst_stride=20480 + 32, src_stride=20480 + 48, off16=1)),
])
def test_copy_rows_one_misalignment(dga, what, kw):
    """Exactly one of the five things the 16-byte lanes need is off (by 4 or 8 bytes): the byte path, the same result."""
    _run_copy_rows(dga, n=7, mode="both", seed=11, **kw)


@pytest.mark.parametrize("mode", ["gather", "scatter", "both"])
def test_copy_rows_uses_the_first_rows_entries_only(dga, mode):
    _run_copy_rows(dga, 4096 + 16, 5, mode, 4096 + 32, 4096 + 64, extra_index=4, seed=13)


@pytest.mark.parametrize("row_bytes,n", [(0, 5), (20480, 0)])
def test_copy_rows_no_ops(dga, row_bytes, n):
    _run_copy_rows(dga, row_bytes, n, "both", 20480 + 32, 20480 + 48, extra_index=5 - n, seed=17)


def _run_copy_rows2(dga, bytes0, bytes1, n, mode, same_dst=False, seed=0, want_vec=None, negatives=True):
    """One dga_copy_rows2 call.  Streams 0 and 1 have their own tensors; same_dst packs both into the rows of one tensor (stream 1
    behind stream 0, as the dispatch packs scales behind the fp8 bytes)."""
    spare = 2
    dst_rows = n + (spare if mode in ("scatter", "both") else 0)
    src_rows = n + (spare if mode in ("gather", "both") else 0)
    al = 16 if (bytes0 | bytes1) % 16 == 0 else 1
    if same_dst:
        d0 = d1 = _Rows(dst_rows, bytes0 + bytes1 + 20 * al, fill=R.FILL)
        d1_off = bytes0
    else:
        d0, d1 = _Rows(dst_rows, bytes0 + 2 * al, fill=R.FILL), _Rows(dst_rows, bytes1 + 3 * al, fill=R.FILL)
        d1_off = al
    s0, s1 = _Rows(src_rows, bytes0 + 4 * al, seed=seed + 1), _Rows(src_rows, bytes1 + 5 * al, seed=seed + 2)
    s0_off, s1_off = al, 2 * al
    neg = (lambda *a: a) if negatives else (lambda *a: ())
    dst_index = _index(n, dst_rows, seed + 3, negatives=neg(1, 4)) if mode in ("scatter", "both") else None
    src_index = _index(n, src_rows, seed + 4, negatives=neg(2, 6)) if mode in ("gather", "both") else None
    if want_vec is not None:
        ptrs = (d0.view.data_ptr(), s0.view.data_ptr() + s0_off, d1.view.data_ptr() + d1_off, s1.view.data_ptr() + s1_off)
        strides = (d0.view.stride(0), s0.view.stride(0), d1.view.stride(0), s1.view.stride(0))
        assert all(x % 16 == 0 for x in ptrs + strides + (bytes0, bytes1)) == want_vec
    w0 = d0.copy()
    w1 = w0 if same_dst else d1.copy()
    _expect(w0, s0, dst_index, src_index, n, bytes0, 0, s0_off)
    _expect(w1, s1, dst_index, src_index, n, bytes1, d1_off, s1_off)
    s0_before, s1_before = s0.whole.clone(), s1.whole.clone()
    dga.copy_rows2(d0.view, s0.view, bytes0, d1.view, s1.view, bytes1, dst_index=dst_index, src_index=src_index, rows=n,
                   src0_off=s0_off, dst1_off=d1_off, src1_off=s1_off)
    torch.cuda.synchronize()
    assert torch.equal(s0.whole, s0_before) and torch.equal(s1.whole, s1_before)
    for name, got, want in (("stream 0", d0, w0), ("stream 1", d1, w1)):
        assert got.first_difference(want) is None, f"{name}: {got.first_difference(want)}"


@pytest.mark.parametrize("mode", ["gather", "scatter", "both"])
@pytest.mark.parametrize("bytes0,bytes1,vec", [
    (20480, 16, True),        # parts = 2 from stream 0; stream 1 is one chunk of part 0
    (16, 20480, True),        # the same, the long stream second
    (7168, 12, False),        # K = 7168 with the scale row of K = 384: the whole call on the byte path, 7 parts
    (12, 7168, False),
    (20480, 0, True),         # an empty second stream with valid pointers
    (0, 1025, False),
])
def test_copy_rows2_unequal_streams(dga, bytes0, bytes1, vec, mode):
    _run_copy_rows2(dga, bytes0, bytes1, 9, mode, seed=bytes0 + 3 * bytes1, want_vec=vec)


@pytest.mark.parametrize("bytes0,bytes1", [(7168, 224), (7168, 12), (16400, 16)])
def test_copy_rows2_packs_payload_rows(dga, bytes0, bytes1):
    """Both streams into one destination row, through a destination index with negative entries (the dispatch's pack)."""
    _run_copy_rows2(dga, bytes0, bytes1, 40, "scatter", same_dst=True, seed=bytes1)


def test_copy_rows2_without_negative_entries(dga):
    _run_copy_rows2(dga, 20480, 16, 9, "both", seed=3, want_vec=True, negatives=False)


def test_copy_rows2_no_ops(dga):
    dst, src = _Rows(5, 64, fill=R.FILL), _Rows(5, 64, seed=1)
    want = dst.copy()
    ix = torch.arange(5, device="cuda")
    dga.copy_rows2(dst.view, src.view, 0, dst.view, src.view, 0, dst_index=ix)
    dga.copy_rows2(dst.view, src.view, 32, dst.view, src.view, 16, dst_index=ix, rows=0, dst1_off=32)
    torch.cuda.synchronize()
    assert torch.equal(dst.whole, want.whole)
