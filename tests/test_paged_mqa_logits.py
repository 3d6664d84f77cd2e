"""CPU: fp8_paged_mqa_logits and per_token_cast_to_fp8_paged are exported through every layer, the float64 reference of
tests/paged_mqa_logits_ref.py agrees with a literal loop (lengths below next_n, beyond N and negative, an out-of-range entry on a needed
page, garbage on unneeded ones), pack and gather invert each other, and the C entries and the Python wrappers refuse what they must before
any launch."""
import ctypes
import re

import numpy as np
import pytest
import torch

import mqa_logits_ref as M
import paged_mqa_logits_ref as R
from test_build import CSRC, ROOT


def test_the_entries_are_exported_through_every_layer(dga):
    from deepgemm_ascend_amd import _lib, api
    header = (ROOT / "include" / "dga_hip.h").read_text()
    makefile = (CSRC / "Makefile").read_text()
    shared = ctypes.CDLL(str(_lib.LIB_PATH))
    for entry, unit, name in (("dga_fp8_paged_mqa_logits", "dga_paged_mqa_logits.hip", "fp8_paged_mqa_logits"),
                              ("dga_cast_to_fp8_1x128_paged", "dga_cast_paged.hip", "per_token_cast_to_fp8_paged")):
        assert re.search(r"\b%s\s*\(" % entry, header), entry
        assert hasattr(shared, entry) and entry in _lib.SIGNATURES, entry
        assert name in dga.__all__ and callable(getattr(dga, name)), name
        assert re.search(r"^SRCS = .*\b%s\b" % re.escape(unit), makefile, flags=re.M), unit
    assert "#define DGA_ABI_VERSION 7\n" in header
    for name, value in (("BLOCK_KV", R.BLOCK_KV), ("BLOCK_BYTES", R.BLOCK_BYTES), ("CHUNK_N", api.PAGED_MQA_LOGITS_CHUNK_N)):
        assert re.search(r"#define DGA_PAGED_MQA_LOGITS_%s %d\b" % (name, value), header), name
    assert (api.PAGED_MQA_LOGITS_BLOCK_KV, api.PAGED_MQA_LOGITS_BLOCK_BYTES) == (R.BLOCK_KV, R.BLOCK_BYTES)
    assert api.PAGED_MQA_LOGITS_CHUNK_N % 256 == 0 and R.BLOCK_BYTES == R.BLOCK_KV * (R.D + 4)
    assert not hasattr(dga, "get_paged_mqa_logits_metadata")
    # the device text that fixes the bits is one header, included by both units and defined in neither
    for unit in ("dga_mqa_logits.hip", "dga_paged_mqa_logits.hip"):
        text = (CSRC / unit).read_text()
        assert '#include "dga_mqa_device.hpp"' in text and "mqa_cvt8(mqa_v2i" not in text and "__shfl_xor" not in text, unit


def _tiny(rng, b, nn, h, nb, max_blocks):
    q = rng.integers(0, 256, size=(b, nn, h, R.D)).astype(np.uint8)
    k = rng.integers(0, 256, size=(nb, R.BLOCK_KV, R.D)).astype(np.uint8)
    q[q & 0x7F == 0x7F] = 0x30                                           # (no NaN codes here)
    k[k & 0x7F == 0x7F] = 0x30
    kscale = rng.uniform(0.5, 2.0, size=(nb, R.BLOCK_KV)).astype(np.float32)
    weights = rng.normal(size=(b * nn, h)).astype(np.float32)
    return q, R.pack(k, kscale), weights


def test_the_reference_agrees_with_a_literal_loop():
    rng = np.random.default_rng(11)
    b, nn, h, nb, max_blocks, n = 6, 2, 2, 4, 2, 70
    q, buf, weights = _tiny(rng, b, nn, h, nb, max_blocks)
    #        ctx < next_n   ctx > N    negative     bad entry on a needed page   plain        64 max_blocks < ctx (n = 200 below)
    lens = np.array([1, n + 30, -4, 68, 66, 3], np.int32)
    tables = np.array([[2, -1], [0, 3], [-7, 0x7FFFFFFF], [1, nb], [3, 1], [0, -1]], np.int32)     # garbage where no page is needed
    want = R.literal_loop(q, buf, weights, lens, tables, n)
    got, mag = R.reference(q, buf, weights, lens, tables, n)
    hi = R.row_ends(lens, nn, n, max_blocks)
    assert list(hi) == [0, 1, n - 1, n, 0, 0, 67, 68, 65, 66, 2, 3]
    inside = np.arange(n)[None, :] < hi[:, None]
    inside[6:8, 64:] = False                                             # the page behind the out-of-range entry
    assert np.array_equal(np.isneginf(got), ~inside) and np.array_equal(np.isneginf(want), ~inside)
    assert np.isfinite(got[6:8, :64]).all() and inside.sum() == 1 + 2 * n - 1 + 128 + 131 + 5
    assert np.allclose(got[inside], want[inside], rtol=1e-13, atol=0)
    assert (np.abs(got[inside]) <= mag[inside] * (1 + 1e-12)).all() and (mag[~inside] == 0).all()
    # 64 max_blocks < N clamps the length
    wide_got, _ = R.reference(q, buf, weights, np.full(b, 1000, np.int32), np.tile(np.array([[1, 2]], np.int32), (b, 1)), 200)
    wide_want = R.literal_loop(q, buf, weights, np.full(b, 1000, np.int32), np.tile(np.array([[1, 2]], np.int32), (b, 1)), 200)
    assert list(R.row_ends(np.full(b, 1000), nn, 200, max_blocks)[:2]) == [127, 128]
    assert np.array_equal(np.isneginf(wide_got), np.isneginf(wide_want)) and np.isneginf(wide_got[:, 128:]).all()
    fin = ~np.isneginf(wide_got)
    assert np.allclose(wide_got[fin], wide_want[fin], rtol=1e-13, atol=0)
    # what a call writes
    w = R.written(lens, nn, n, max_blocks, clean=False)
    assert list(w.sum(axis=1)) == [64, 64, n, n, 0, 0, n, n, n, n, 64, 64] and R.written(lens, nn, n, max_blocks, clean=True).all()


def test_pack_followed_by_gather_is_the_identity():
    rng = np.random.default_rng(5)
    nb = 5
    k = rng.integers(0, 256, size=(nb, R.BLOCK_KV, R.D)).astype(np.uint8)
    kscale = rng.uniform(0.1, 3.0, size=(nb, R.BLOCK_KV)).astype(np.float32)
    for stride in (R.BLOCK_BYTES, R.BLOCK_BYTES + 64):
        buf = R.pack(k, kscale, stride)
        assert buf.shape == (nb, stride) and (buf[:, R.BLOCK_BYTES:] == R.PAD_BYTE).all()
        codes, scales = R.unpack(buf)
        assert np.array_equal(codes, k) and np.array_equal(scales.view(np.uint32), kscale.view(np.uint32))
        # key 3 of block 4 sits where the layout says: codes first, then scales
        assert np.array_equal(buf[4, 3 * R.D:4 * R.D], k[4, 3])
        assert np.array_equal(buf[4, 8192 + 12:8192 + 16], kscale[4, 3:4].view(np.uint8))
        table = np.array([3, 0, 4, 1], np.int32)
        kg, sg, ok = R.gather(buf, table, 3 * 64 + 7)
        assert ok.all() and np.array_equal(kg, np.concatenate([k[3], k[0], k[4], k[1, :7]]))
        assert np.array_equal(sg, np.concatenate([kscale[3], kscale[0], kscale[4], kscale[1, :7]]))
        _, _, ok = R.gather(buf, np.array([3, nb, -1, 1], np.int32), 4 * 64)
        assert ok[:64].all() and not ok[64:192].any() and ok[192:].all()
    tables, num_blocks = R.make_tables((0, 1, 64, 65, 513), 600, 10, seed=0, share=(3, 4))
    named = [tables[i, p] for i, c in enumerate((0, 1, 1, 2, 9)) for p in range(c)]
    assert tables[3, 0] == tables[4, 0] and len(set(named)) == len(named) - 1 and num_blocks == 15 and max(named) < num_blocks
    rest = [tables[i, p] for i, c in enumerate((0, 1, 1, 2, 9)) for p in range(c, 10)]
    assert set(rest) == set(R.UNUSED)


def test_the_exact_case_is_exactly_summable():
    q, buf, weights, lens, tables, want = R.exact_case(32, 2, (0, 1, 64, 65), 100, 2, share=(2, 3))
    fin = ~np.isneginf(want)
    assert fin.sum() == 0 + 0 + 0 + 1 + 63 + 64 + 64 + 65 and not np.isnan(want).any()
    assert np.array_equal(want[fin].astype(np.float32).astype(np.float64), want[fin]) and len(np.unique(want[fin])) > 50
    assert np.isin(q, M.HALVES).all() and np.isin(R.unpack(buf)[0], M.HALVES).all()


def test_the_c_entries_check_their_arguments_before_any_launch(dga):
    from deepgemm_ascend_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_char * 128)()
    p = (ctypes.addressof(buf) + 15) & ~15
    OK, E_NULL, E_SHAPE, E_DTYPE, E_ALIGN, E_RANGE = 0, -1, -2, -3, -4, -9
    assert (_lib.DT_FP32, _lib.DT_BF16, _lib.DT_FP16) and E_DTYPE == L.dga_cast_to_fp8_1x128_paged(p, 99, 1, p, 1, 8448, p, 0, None)

    def score(batch=2, nn=2, heads=64, dim=128, nb=4, stride=8448, max_blocks=3, n=100, clean=1, q=p, kv=p, weights=p, lens=p, tables=p, logits=p):
        return L.dga_fp8_paged_mqa_logits(q, kv, weights, lens, tables, batch, nn, heads, dim, nb, stride, max_blocks, n, clean, logits, None)
    for bad in (dict(batch=-1), dict(nn=0), dict(nn=3), dict(heads=48), dict(heads=16), dict(dim=64), dict(nb=0), dict(stride=8447),
                dict(stride=8432), dict(max_blocks=0), dict(n=0)):
        assert score(**bad) == E_SHAPE, bad
    assert score(batch=0, q=None, kv=None, logits=None) == OK
    for name in ("q", "kv", "weights", "lens", "tables", "logits"):
        assert score(**{name: None}) == E_NULL, name
    for bad in (dict(q=p + 4), dict(kv=p + 8), dict(weights=p + 8), dict(lens=p + 2), dict(tables=p + 1), dict(logits=p + 2), dict(stride=8456)):
        assert score(**bad) == E_ALIGN, bad
    assert score(n=0x7FFFFC01) == E_RANGE and score(nb=1 << 60) == E_RANGE and score(batch=1 << 40, n=1 << 20) == E_RANGE
    assert score(max_blocks=1 << 60) == E_RANGE and score(batch=1 << 33, n=1) == E_RANGE

    def write(tokens=4, dtype=_lib.DT_BF16, nb=4, stride=8448, flags=0, x=p, kv=p, slots=p):
        return L.dga_cast_to_fp8_1x128_paged(x, dtype, tokens, kv, nb, stride, slots, flags, None)
    assert write(flags=2) == E_RANGE
    assert write(tokens=-1) == E_SHAPE and write(nb=0) == E_SHAPE and write(stride=8440) == E_SHAPE
    assert write(tokens=0, x=None, kv=None, slots=None) == OK
    for name in ("x", "kv", "slots"):
        assert write(**{name: None}) == E_NULL, name
    assert write(dtype=77) == E_DTYPE
    assert write(x=p + 8) == E_ALIGN and write(kv=p + 8) == E_ALIGN and write(slots=p + 4) == E_ALIGN and write(stride=8456) == E_ALIGN
    assert write(nb=1 << 60) == E_RANGE and write(tokens=1 << 40) == E_RANGE


def _args(b=3, nn=2, h=64, d=128, nb=5, max_blocks=4):
    return [torch.zeros((b, nn, h, d), dtype=torch.uint8), torch.zeros((nb, 64, 1, 132), dtype=torch.uint8), torch.ones((b * nn, h)),
            torch.zeros(b, dtype=torch.int32), torch.zeros((b, max_blocks), dtype=torch.int32)]


def test_the_scoring_wrapper_refuses_before_any_launch(dga):
    def refused(args, word, **kw):
        kw.setdefault("max_model_len", 100)
        with pytest.raises(dga.DGAError, match=word):
            dga.fp8_paged_mqa_logits(*args, **kw)
    refused(_args(), "HIP device")                                       # CPU tensors
    refused(_args(), "HIP device", schedule_metadata=object())           # (accepted, never looked at)
    a = _args()
    a[0] = a[0][0]
    refused(a, "q must be \\[B, next_n, H, 128\\]")
    refused(_args(nn=3), "next_n 1 or 2, got 3")
    refused(_args(h=48), "32 or 64 heads, got 48")
    refused(_args(d=64), "head dimension 64")
    a = _args()
    a[0] = torch.zeros((3, 2, 128, 128), dtype=torch.uint8)[:, :, ::2]
    refused(a, "q must be contiguous")
    a = _args()
    a[0] = a[0].to(torch.float32)
    refused(a, "fp8 operand")
    for bad, word in ((torch.zeros((5, 64, 132), dtype=torch.uint8), "kv_cache must be \\[num_blocks, 64, 1, 132\\] or"),
                      (torch.zeros((5, 32, 1, 132), dtype=torch.uint8), "blocks of 64 keys, got 32"),
                      (torch.zeros((5, 64, 1, 131), dtype=torch.uint8), "1 x 131 bytes per key"),
                      (torch.zeros((5, 8447), dtype=torch.uint8), "got 8447 bytes per block"),
                      (torch.zeros((5, 64, 1, 132), dtype=torch.int8), "kv_cache must be uint8"),
                      (torch.zeros((0, 64, 1, 132), dtype=torch.uint8), "at least one block"),
                      (torch.zeros((5, 8448 + 8), dtype=torch.uint8)[:, :8448], "multiple of 16, got stride\\(0\\) = 8456"),
                      (torch.zeros(5 * 8448, dtype=torch.uint8).as_strided((5, 8448), (8432, 1)), "got stride\\(0\\) = 8432"),
                      (torch.zeros((5, 64, 1, 264), dtype=torch.uint8)[..., ::2], "contiguous inside a block"),
                      (torch.zeros((5, 2 * 8448), dtype=torch.uint8)[:, ::2], "contiguous inside a block")):
        a = _args()
        a[1] = bad
        refused(a, word)
    a = _args()
    a[2] = a[2].to(torch.float64)
    refused(a, "weights must be contiguous float32 \\[6, 64\\]")
    a = _args()
    a[2] = a[2][:5]
    refused(a, "weights must be contiguous float32 \\[6, 64\\]")
    a = _args()
    a[3] = a[3].to(torch.int64)
    refused(a, "context_lens must be contiguous int32 \\[3\\]")
    a = _args()
    a[3] = torch.zeros((3, 2), dtype=torch.int32)
    refused(a, "context_lens must be contiguous int32 \\[3\\]")
    a = _args()
    a[4] = a[4].to(torch.int64)
    refused(a, "block_tables must be contiguous int32 \\[3, 4\\]")
    a = _args()
    a[4] = a[4][:2]
    refused(a, "block_tables must be contiguous int32 \\[3, 4\\]")
    a = _args()
    a[4] = a[4][:, :0]
    refused(a, "max_blocks >= 1")
    refused(_args(), "max_model_len is required", max_model_len=None)
    refused(_args(), "max_model_len must be at least 1", max_model_len=0)
    refused(_args(), "out must be contiguous float32 \\[6, 100\\]", out=torch.zeros((6, 99)))
    refused(_args(), "out must be contiguous float32 \\[6, 100\\]", out=torch.zeros((6, 100), dtype=torch.float16))
    # upstream's positional order: schedule_metadata sixth, max_model_len seventh
    with pytest.raises(dga.DGAError, match="HIP device"):
        dga.fp8_paged_mqa_logits(*_args(), None, 100)
    with pytest.raises(dga.DGAError, match="max_model_len is required"):
        dga.fp8_paged_mqa_logits(*_args())


def test_the_writer_wrapper_refuses_before_any_launch(dga):
    def refused(word, x=None, kv=None, slots=None, **kw):
        x = torch.zeros((4, 128), dtype=torch.bfloat16) if x is None else x
        kv = torch.zeros((5, 64, 1, 132), dtype=torch.uint8) if kv is None else kv
        slots = torch.zeros(4, dtype=torch.int64) if slots is None else slots
        with pytest.raises(dga.DGAError, match=word):
            dga.per_token_cast_to_fp8_paged(x, kv, slots, **kw)
    refused("HIP device")
    refused("HIP device", use_ue8m0=True)
    refused("x must be a contiguous \\[T, 128\\]", x=torch.zeros((4, 256)))
    refused("x must be a contiguous \\[T, 128\\]", x=torch.zeros((4, 1, 128)))
    refused("x must be a contiguous \\[T, 128\\]", x=torch.zeros((4, 256))[:, ::2])
    refused("float32, bfloat16 or float16", x=torch.zeros((4, 128), dtype=torch.float64))
    refused("blocks of 64 keys, got 16", kv=torch.zeros((5, 16, 1, 132), dtype=torch.uint8))
    refused("got stride\\(0\\) = 8456", kv=torch.zeros((5, 8456), dtype=torch.uint8)[:, :8448])
    refused("slot_mapping must be contiguous int64 \\[4\\]", slots=torch.zeros(4, dtype=torch.int32))
    refused("slot_mapping must be contiguous int64 \\[4\\]", slots=torch.zeros(5, dtype=torch.int64))


@pytest.mark.parametrize("nn", (1, 2))
@pytest.mark.parametrize("mirrored", (False, True), ids=("codes_in_k", "codes_in_q"))
def test_the_all_codes_case_keeps_every_code_inside_the_row_ends(mirrored, nn):
    h = 32
    q, buf, weights, lens, tables, n, want = R.all_codes_case(h, nn, mirrored)
    fq, fk, fw, head = M.all_codes_operands(h, mirrored)
    b = q.shape[0]
    assert np.array_equal(q.reshape(b * nn, h, R.D), fq) and np.array_equal(weights, fw) and (lens == n).all() and n == fk.shape[0]
    # two tables, shared by the even and by the odd sequences, over disjoint blocks that hold the same keys; the rest holds NaN codes
    assert np.array_equal(tables[::2], np.tile(tables[0], (len(tables[::2]), 1))) and np.array_equal(tables[1::2], np.tile(tables[1], (b // 2, 1)))
    assert len(set(tables[0]) | set(tables[1])) == 2 * tables.shape[1] and tables.shape[1] == (n + 63) // 64
    for row in tables[:2]:
        kg, sg, ok = R.gather(buf, row, n)
        assert ok.all() and np.array_equal(kg, fk) and (sg == 1).all()
    codes, _ = R.unpack(buf)
    spare = np.setdiff1d(np.arange(buf.shape[0]), tables[:2].reshape(-1))
    assert len(spare) == 3 and (codes[spare] == M.NAN_CODE).all()
    # the prefill case's values on the columns below each row's end, -inf behind it
    flat = M.all_codes_case(h, mirrored)[6]
    inside = np.arange(n)[None, :] < R.row_ends(lens, nn, n, tables.shape[1])[:, None]
    assert inside.sum() == b * nn * n - b * (nn - 1) and np.array_equal(want[inside], flat[inside]) and np.isneginf(want[~inside]).all()
    assert np.array_equal(want[inside].astype(np.float32).astype(np.float64), want[inside])
    assert np.array_equal(np.unique(want[inside]), np.unique(np.abs(M.TABLE[M.FINITE])))
    # every code still meets a unit code inside a row's range
    t, col = np.nonzero(inside)
    seen = fq[t, head[t], col % R.D] if mirrored else fk[col, t % R.D]
    assert np.array_equal(np.unique(seen), M.FINITE)
    # a wrong conversion is rejected here as well
    fq, fk, fscale, fw, ks, ke, _ = M.all_codes_case(h, mirrored)
    for kind in ("subnormal", "sign"):                                  # one subnormal code flushed to zero; -0.5 read as +0.5
        wrong = np.where(inside, M.reference(fq, fk, fscale, fw, ks, ke, M.broken_table(kind))[0], -np.inf)
        assert 0 < (wrong != want).sum() < want.size // 50
        with pytest.raises(AssertionError):
            M.assert_same_values(wrong.astype(np.float32), want)
