"""CPU: indexer_topk is exported through every layer, the numpy reference of tests/indexer_topk_ref.py agrees with a literal loop on tiny
rows (all three range forms, negative and oversized bounds, relative, a table with bad entries), key orders the special values as stated, and
the C entry and the Python wrapper refuse what they must before any launch."""
import ctypes
import re

import numpy as np
import pytest
import torch

import indexer_topk_ref as R
from test_build import CSRC, ROOT

I32 = torch.int32


def test_the_entry_is_exported_through_every_layer(dga):
    from deepgemm_ascend_amd import _lib, api
    header = (ROOT / "include" / "dga_hip.h").read_text()
    makefile = (CSRC / "Makefile").read_text()
    shared = ctypes.CDLL(str(_lib.LIB_PATH))
    assert re.search(r"\bdga_indexer_topk\s*\(", header)
    assert hasattr(shared, "dga_indexer_topk") and "dga_indexer_topk" in _lib.SIGNATURES
    assert "indexer_topk" in dga.__all__ and callable(dga.indexer_topk)
    assert re.search(r"^SRCS = .*\bdga_indexer_topk\.hip\b", makefile, flags=re.M)
    assert "#define DGA_ABI_VERSION 7\n" in header
    assert re.search(r"#define DGA_INDEXER_TOPK_MAX_K %d\b" % api.INDEXER_TOPK_MAX_K, header) and api.INDEXER_TOPK_MAX_K == R.MAX_K == 2048
    assert re.search(r"#define DGA_INDEXER_TOPK_CANDIDATES %d\b" % api.INDEXER_TOPK_CANDIDATES, header)
    assert api.INDEXER_TOPK_CANDIDATES >= api.INDEXER_TOPK_MAX_K
    # one workgroup per row that waits for nobody: no atomics on global memory, no spinning
    text = (CSRC / "dga_indexer_topk.hip").read_text()
    code = "\n".join(line.split("//")[0] for line in text.splitlines())
    assert "while" not in code and "__threadfence" not in code and "atomicCAS" not in code
    assert all(re.match(r"atomicAdd\(&(hist\[|ncand)", a) for a in re.findall(r"atomic\w+\([^,]*", code))


def test_key_orders_the_special_values_as_stated():
    keys = R.key(R.SPECIALS)          # -NaN, -inf, -1, -0, +0, the least subnormal, 1, +inf, NaN
    assert keys[0] == keys[8] == 0xFFFFFFFF
    assert list(np.argsort(keys[1:8], kind="stable")) == list(range(7)) and len(set(keys[1:8].tolist())) == 7
    assert keys[3] == 0x7FFFFFFF and keys[4] == 0x80000000 and keys[1] == 0x007FFFFF and keys[7] == 0xFF800000
    assert (R.key(R.from_bits([0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF])) == 0xFFFFFFFF).all()      # any payload, either sign
    # as values the order is the usual one wherever that is defined
    x = np.random.default_rng(0).standard_normal(1000).astype(np.float32)
    assert np.array_equal(np.argsort(R.key(x), kind="stable"), np.argsort(x, kind="stable"))
    # the order is total: NaN above +inf, ties to the lower column
    row = R.from_bits([0x7F800000, 0x7FC00000, 0x3F800000, 0x3F800000, 0xFFC00000])[None]
    assert R.reference(row, 2).tolist() == [[1, 4]] and R.reference(row, 4).tolist() == [[0, 1, 2, 4]]
    assert R.reference(row, 3).tolist() == [[0, 1, 4]] and R.reference(row[:, 2:4], 1).tolist() == [[0]]


def _tiny(seed, m, n):
    rng = np.random.default_rng(seed)
    x = rng.integers(-3, 4, size=(m, n)).astype(np.float32)               # many ties
    x[rng.random((m, n)) < 0.15] = np.float32("nan")
    x[rng.random((m, n)) < 0.1] = -np.float32("inf")
    x[rng.random((m, n)) < 0.1] = np.float32(-0.0)
    return x


def test_the_reference_agrees_with_a_literal_loop():
    m, n = 8, 23
    x = _tiny(1, m, n)
    starts = np.array([0, -4, 3, 22, 9, 30, 5, 1], np.int32)
    ends = np.array([23, 10, 3, 23, 4, 40, 99, 2], np.int32)              # full, negative start, empty, one, reversed, beyond N, oversized, one
    lo, hi = R.ranges(m, n, starts, ends)
    assert lo.tolist() == [0, 0, 3, 22, 9, 23, 5, 1] and hi.tolist() == [23, 10, 3, 23, 4, 23, 23, 2]
    lens = np.array([-2, 1, 23, 50], np.int32)
    assert R.ranges(8, n, context_lens=lens, next_n=2)[1].tolist() == [0, 0, 0, 1, 22, 23, 22, 23]
    assert R.ranges(4, n, context_lens=lens)[1].tolist() == [0, 1, 23, 23]
    tables = np.array([[1, 2, 3], [4, -1, 0], [2, 6, 0x7FFFFFFF], [0, 5, 1]], np.int32)      # pages of 4 and 8: a negative entry, num_blocks, garbage
    forms = [dict(), dict(row_starts=starts, row_ends=ends), dict(row_starts=starts, row_ends=ends, relative=True),
             dict(context_lens=lens, next_n=2), dict(context_lens=lens, next_n=2, relative=True),
             dict(context_lens=lens, next_n=2, block_tables=tables, page_size=8, num_blocks=6),
             dict(context_lens=lens, next_n=2, block_tables=tables, page_size=4, num_blocks=6),
             dict(context_lens=np.array([5, 23, 0, 7, -1, 12, 23, 3], np.int32), next_n=1, block_tables=np.tile(tables, (2, 1)), page_size=8,
                  num_blocks=6)]
    for k in (1, 2, 5, 22, 23, 24, 40):
        for form in forms:
            got, want = R.reference(x, k, **form), R.literal_loop(x, k, **form)
            assert got.dtype == np.int32 and got.shape == (m, k) and np.array_equal(got, want), (k, sorted(form))
    # what the forms say, on one row read by eye: columns 2 .. 8 of [3, 1, nan, 1, -inf, 2, 2, -0, 0]
    row = np.array([[3, 1, np.nan, 1, -np.inf, 2, 2, -0.0, 0.0]], np.float32)
    ks, ke = np.array([2], np.int32), np.array([9], np.int32)
    assert R.reference(row, 3, ks, ke).tolist() == [[2, 5, 6]] and R.reference(row, 3, ks, ke, relative=True).tolist() == [[0, 3, 4]]
    assert R.reference(row, 5, ks, ke).tolist() == [[2, 3, 5, 6, 8]] and R.reference(row, 6, ks, ke).tolist() == [[2, 3, 5, 6, 7, 8]]
    assert R.reference(row, 9, ks, ke).tolist() == [[2, 3, 4, 5, 6, 7, 8, -1, -1]]          # -inf is a candidate; the tail is -1
    table = np.array([[7, 9, -1]], np.int32)
    got = R.reference(row, 4, context_lens=np.array([9], np.int32), block_tables=table, page_size=2, num_blocks=9)
    assert got.tolist() == [[14, -1, -1, -1]]                                # columns 0, 2, 5, 6: pages 0, 1 (entry 9 = num_blocks), 2 (-1), 3 (no entry)
    # a range no longer than k never looks at a value
    assert R.reference(np.full((1, 9), np.nan, np.float32), 9, ks, ke).tolist() == [[2, 3, 4, 5, 6, 7, 8, -1, -1]]


def test_the_case_builders_build_what_they_say():
    k = 64
    x = R.special_rows(2, k + 100, k, seed=0)
    keys = R.key(x)
    assert ((keys >= 0x80000000).sum(axis=1) == k).all() and (keys == 0x7FFFFFFF).sum() > 100 and (keys == 0x80000000).sum() > 60
    x = R.lowest_bit_rows(2, 300, k, seed=0)
    ordered = np.sort(R.key(x), axis=1)[:, ::-1]
    assert (ordered[:, k - 1] == 0xBF800001).all() and (ordered[:, k] == 0xBF800000).all()
    x = R.shared_digit_rows(1, 5000, seed=0)
    assert len(set((R.key(x) >> 21).ravel().tolist())) == 1 and len(set(R.key(x).ravel().tolist())) == 5000
    x = R.two_valued_rows(3, 500, k, seed=0)
    assert [(row == 2.5).sum() for row in x] == [k - 5, k - 6, k - 7]
    same = R.bits(R.equal_rows(8, 4))
    assert len({row.tobytes() for row in same}) == 8 and (same[:, :1] == same).all()


def test_the_c_entry_checks_its_arguments_before_any_launch(dga):
    from deepgemm_ascend_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_char * 128)()
    p = (ctypes.addressof(buf) + 15) & ~15
    OK, E_NULL, E_SHAPE, E_ALIGN, E_RANGE = 0, -1, -2, -4, -9

    def topk(m=4, n=100, stride=100, k=8, ks=None, ke=None, lens=None, next_n=1, relative=0, tables=None, max_blocks=0, page=64, nb=0,
             logits=p, out=p):
        return L.dga_indexer_topk(logits, m, n, stride, k, ks, ke, lens, next_n, relative, tables, max_blocks, page, nb, out, None)
    paged = dict(lens=p, tables=p, max_blocks=2, nb=5)
    for bad in (dict(m=-1), dict(n=0), dict(stride=99)):
        assert topk(**bad) == E_SHAPE, bad
    assert topk(m=0, logits=None, out=None) == OK and topk(m=0, k=0, logits=None, out=None) == OK
    for bad in (dict(logits=None), dict(out=None), dict(ks=p), dict(ke=p)):
        assert topk(**bad) == E_NULL, bad
    for bad in (dict(logits=p + 2), dict(out=p + 1), dict(ks=p + 2, ke=p), dict(ks=p, ke=p + 3), dict(lens=p + 2), dict(paged, tables=p + 2)):
        assert topk(**bad) == E_ALIGN, bad
    for bad in (dict(k=0), dict(k=2049), dict(k=-1), dict(n=0x7FFF0001, stride=0x7FFF0001), dict(m=1 << 31),
                dict(ks=p, ke=p, lens=p), dict(relative=1, **paged), dict(tables=p, max_blocks=2, nb=5),
                dict(lens=p, next_n=0), dict(lens=p, next_n=3), dict(m=1 << 30, stride=1 << 40),
                dict(paged, page=0), dict(paged, page=-64), dict(paged, max_blocks=0), dict(paged, nb=0),
                dict(paged, nb=1 << 25), dict(paged, page=1, nb=1 << 31), dict(paged, max_blocks=1 << 61)):
        assert topk(**bad) == E_RANGE, bad
    assert topk(m=3, lens=p, next_n=2) == E_SHAPE


def _logits(m=6, n=100):
    return torch.zeros((m, n))


def test_the_wrapper_refuses_before_any_launch(dga):
    def refused(word, logits=None, **kw):
        with pytest.raises(dga.DGAError, match=word):
            dga.indexer_topk(_logits() if logits is None else logits, **kw)
    z = lambda *shape: torch.zeros(shape, dtype=I32)                      # noqa: E731
    paged = dict(context_lens=z(3), next_n=2, block_tables=z(3, 2), num_blocks=5)
    # what is valid reaches the device guard (host tensors: "no CPU path")
    for kw in (dict(), dict(k=1), dict(k=2048), dict(row_starts=z(6), row_ends=z(6)), dict(row_starts=z(6), row_ends=z(6), relative=True),
               dict(context_lens=z(6)), dict(context_lens=z(3), next_n=2, relative=True), paged, dict(paged, page_size=1),
               dict(out=torch.zeros((6, 2048), dtype=I32)), dict(logits=torch.zeros((6, 130))[:, :100]), dict(logits=torch.zeros((0, 100))),
               dict(logits=torch.zeros((6, 1)))):
        refused("HIP device", **kw)
    refused("float32 \\[M, N\\]", logits=torch.zeros((6, 100), dtype=torch.float16))
    refused("float32 \\[M, N\\]", logits=torch.zeros(100))
    refused("float32 \\[M, N\\]", logits=torch.zeros((2, 3, 100)))
    refused("at least one column", logits=torch.zeros((6, 0)))
    refused("contiguous last dimension", logits=torch.zeros((6, 200))[:, ::2])
    refused("contiguous last dimension", logits=torch.zeros((100, 6)).t())
    refused("stride\\(0\\) >= N", logits=torch.zeros(100).expand(6, 100))
    for k in (0, 2049, -1, 8.0, None):
        refused("k must be an integer in \\[1, 2048\\]", k=k)
    refused("come together or not at all", row_starts=z(6))
    refused("come together or not at all", row_ends=z(6))
    refused("exclude each other", row_starts=z(6), row_ends=z(6), context_lens=z(6))
    refused("relative and block_tables exclude each other", relative=True, **paged)
    refused("block_tables needs context_lens", block_tables=z(6, 2), num_blocks=5)
    refused("row_starts must be contiguous int32 \\[6\\]", row_starts=z(5), row_ends=z(6))
    refused("row_starts must be contiguous int32 \\[6\\]", row_starts=torch.zeros(6, dtype=torch.int64), row_ends=z(6))
    refused("row_ends must be contiguous int32 \\[6\\]", row_starts=z(6), row_ends=z(12)[::2])
    refused("next_n must be 1 or 2", context_lens=z(2), next_n=3)
    refused("next_n must be 1 or 2", context_lens=z(6), next_n=0)
    refused("B next_n rows, got 5 with next_n = 2", logits=_logits(5), context_lens=z(2), next_n=2)
    refused("context_lens must be contiguous int32 \\[3\\]", context_lens=z(6), next_n=2)
    refused("context_lens must be contiguous int32 \\[6\\]", context_lens=torch.zeros(6, dtype=torch.int64))
    refused("max_blocks >= 1", **dict(paged, block_tables=z(3, 0)))
    refused("max_blocks >= 1", **dict(paged, block_tables=z(6)))
    refused("block_tables must be contiguous int32 \\[3, 2\\]", **dict(paged, block_tables=z(4, 2)))
    refused("block_tables must be contiguous int32 \\[3, 2\\]", **dict(paged, block_tables=torch.zeros((3, 2), dtype=torch.int64)))
    refused("page_size must be an integer >= 1", **dict(paged, page_size=0))
    refused("num_blocks is required", **dict(paged, num_blocks=None))
    refused("num_blocks is required", **dict(paged, num_blocks=0))
    refused("below 2\\^31, got 33554432 x 64", **dict(paged, num_blocks=1 << 25))
    refused("out must be contiguous int32 \\[6, 2048\\]", out=torch.zeros((6, 2047), dtype=I32))
    refused("out must be contiguous int32 \\[6, 7\\]", k=7, out=torch.zeros((6, 7), dtype=torch.int64))
    refused("out must be contiguous int32 \\[6, 7\\]", k=7, out=torch.zeros((6, 14), dtype=I32)[:, ::2])
