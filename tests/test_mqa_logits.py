"""CPU: fp8_mqa_logits is exported through every layer, the float64 reference of tests/mqa_logits_ref.py agrees with a literal triple loop,
the exactly summable operands are what they claim to be, and the C entry and the Python wrapper refuse what they must before any launch."""
import ctypes
import re

import numpy as np
import pytest
import torch

import mqa_logits_ref as R
from test_build import CSRC, ROOT


def test_the_entry_is_exported_through_every_layer(dga):
    from deepgemm_ascend_amd import _lib, api
    header = (ROOT / "include" / "dga_hip.h").read_text()
    assert re.search(r"\bdga_fp8_mqa_logits\s*\(", header)
    assert hasattr(ctypes.CDLL(str(_lib.LIB_PATH)), "dga_fp8_mqa_logits") and "dga_fp8_mqa_logits" in _lib.SIGNATURES
    assert "fp8_mqa_logits" in dga.__all__ and callable(dga.fp8_mqa_logits)
    assert re.search(r"^SRCS = .*\bdga_mqa_logits\.hip\b", (CSRC / "Makefile").read_text(), flags=re.M)
    assert "#define DGA_ABI_VERSION 7\n" in header
    for name, value in (("HEAD_DIM", R.D), ("BLOCK_N", R.BN), ("BLOCK_M", R.BM)):
        assert "#define DGA_MQA_LOGITS_%s %d" % (name, value) in header, name
    assert (api.MQA_LOGITS_BLOCK_M, api.MQA_LOGITS_BLOCK_N, api.MQA_LOGITS_HEAD_DIM, api.MQA_LOGITS_HEADS) == (R.BM, R.BN, R.D, R.HEADS)


def test_the_reference_agrees_with_a_literal_triple_loop():
    rng = np.random.default_rng(3)
    m, h, n = 3, 4, 7
    q = rng.integers(0, 256, size=(m, h, R.D)).astype(np.uint8)
    k = rng.integers(0, 256, size=(n, R.D)).astype(np.uint8)
    q[q & 0x7F == 0x7F] = 0x30                                           # (no NaN codes here)
    k[k & 0x7F == 0x7F] = 0x30
    kscale = rng.uniform(0.5, 2.0, size=n).astype(np.float32)
    weights = rng.normal(size=(m, h)).astype(np.float32)
    ks, ke = np.array([0, 2, 5], np.int32), np.array([7, 6, 3], np.int32)
    want = R.triple_loop(q, k, kscale, weights, ks, ke)
    got, mag = R.reference(q, k, kscale, weights, ks, ke)
    inside = R.in_range(ks, ke, n)
    assert inside.sum() == 7 + 4 + 0 and np.array_equal(np.isneginf(got), ~inside) and np.array_equal(np.isneginf(want), ~inside)
    assert np.allclose(got[inside], want[inside], rtol=1e-13, atol=0)
    assert (np.abs(got[inside]) <= mag[inside] * (1 + 1e-12)).all()
    # out-of-bounds ranges are clamped, and a NaN code poisons its row / its column inside the ranges only
    q2, k2 = q.copy(), k.copy()
    q2[1, 2, 5], k2[4, 9] = R.NAN_CODE, 0xFF
    got2, _ = R.reference(q2, k2, kscale, weights, np.array([-3, 2, 5], np.int32), np.array([99, 6, 3], np.int32))
    assert np.isnan(got2[1, 2:6]).all() and np.isnan(got2[0, 4]) and np.isneginf(got2[1, :2]).all() and np.isneginf(got2[2]).all()
    assert np.array_equal(got2[0, [0, 1, 2, 3, 5, 6]], got[0, [0, 1, 2, 3, 5, 6]])


def test_the_exact_operands_are_exactly_summable():
    q, k, kscale, weights = R.exact_operands(5, 15, 64)
    assert set(np.unique(R.TABLE[R.HALVES])) == set(np.arange(-4, 5) / 2.0)
    assert np.isin(q, R.HALVES).all() and np.isin(k, R.HALVES).all() and len(np.unique(q)) == 9 and len(np.unique(k)) == 9
    assert (weights * 8 == np.round(weights * 8)).all() and weights.min() >= -4 and weights.max() < 4
    assert all(len(set(row)) == 64 for row in weights)
    mant, _ = np.frexp(kscale)
    assert (mant == 0.5).all() and len(np.unique(kscale)) > 3
    want, _ = R.reference(q, k, kscale, weights, *R.ranges("full", 5, 15))
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)      # the result is a float32 value
    assert R.bound(64) == 2.0 ** -22 + 67 * 2.0 ** -24
    for kind in R.RANGE_KINDS:
        ks, ke = R.ranges(kind, R.BM + 3, 2 * R.BN + 37)
        assert ks.dtype == np.int32 and ke.dtype == np.int32 and ks.shape == ke.shape == (R.BM + 3,)
    ks, ke = R.ranges("windows", R.BM + 3, 2 * R.BN + 37)
    assert ((ks % 4 != 0) & (ke % 4 != 0)).all() and (ke > ks).sum() > R.BM // 2
    ks, ke = R.ranges("empty", 9, 40)
    assert (ke <= ks).all()
    ks, ke = R.ranges("beyond", 9, 40)
    assert (ks < 0).all() and (ke > 40).all()


def test_the_c_entry_checks_its_arguments_before_any_launch(dga):
    from deepgemm_ascend_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_char * 128)()
    p = (ctypes.addressof(buf) + 15) & ~15
    OK, E_NULL, E_SHAPE, E_ALIGN, E_RANGE = 0, -1, -2, -4, -9

    def call(m=4, n=8, heads=64, dim=128, q=p, k=p, kscale=p, weights=p, ks=p, ke=p, logits=p):
        return L.dga_fp8_mqa_logits(q, k, kscale, weights, ks, ke, m, n, heads, dim, logits, None)
    assert call(m=-1) == E_SHAPE and call(n=0) == E_SHAPE and call(dim=64) == E_SHAPE and call(heads=48) == E_SHAPE
    assert call(heads=16) == E_SHAPE and call(heads=128) == E_SHAPE
    assert call(m=0, q=None, logits=None) == OK
    for name in ("q", "k", "kscale", "weights", "ks", "ke", "logits"):
        assert call(**{name: None}) == E_NULL, name
    assert call(q=p + 4) == E_ALIGN and call(k=p + 1) == E_ALIGN and call(weights=p + 8) == E_ALIGN and call(logits=p + 2) == E_ALIGN
    assert call(n=0x7FFFFF01) == E_RANGE and call(m=1 << 40, n=1 << 20) == E_RANGE


def _args(m=3, h=64, d=128, n=9):
    q = torch.zeros((m, h, d), dtype=torch.uint8)
    kv = (torch.zeros((n, d), dtype=torch.uint8), torch.ones(n))
    return [q, kv, torch.ones((m, h)), torch.zeros(m, dtype=torch.int32), torch.full((m,), n, dtype=torch.int32)]


def test_the_wrapper_refuses_before_any_launch(dga):
    def refused(args, word, **kw):
        with pytest.raises(dga.DGAError, match=word):
            dga.fp8_mqa_logits(*args, **kw)
    refused(_args(), "HIP device")                                       # CPU tensors
    refused(_args(d=64), "head dimension 64")
    refused(_args(h=48), "32 or 64 heads, got 48")
    a = _args()
    a[0] = torch.zeros((3, 128, 128), dtype=torch.uint8)[:, ::2]
    refused(a, "q must be contiguous")
    a = _args()
    a[0] = a[0].to(torch.float32)
    refused(a, "fp8 operand")
    a = _args()
    a[1] = (a[1][0], torch.ones(8))
    refused(a, "kscale must be contiguous float32 \\[9\\]")
    a = _args()
    a[1] = (a[1][0][:, :64], a[1][1])
    refused(a, "k must be")
    a = _args()
    a[2] = a[2].to(torch.float64)
    refused(a, "weights must be contiguous float32")
    a = _args()
    a[3] = a[3].to(torch.int64)
    refused(a, "cu_seq_len_k_start must be contiguous int32")
    a = _args()
    a[4] = a[4].to(torch.int64)
    refused(a, "cu_seq_len_k_end must be contiguous int32")
    a = _args()
    a[4] = a[4][:2]
    refused(a, "cu_seq_len_k_end must be contiguous int32 \\[3\\]")
    refused(_args(), "out must be contiguous float32 \\[3, 9\\]", out=torch.zeros((3, 8)))
    refused(_args(), "out must be contiguous float32 \\[3, 9\\]", out=torch.zeros((3, 9), dtype=torch.float16))
    a = _args()
    a[1] = a[1][0]
    refused(a, "kv must be")


@pytest.mark.parametrize("h", R.HEADS)
@pytest.mark.parametrize("mirrored", (False, True), ids=("codes_in_k", "codes_in_q"))
def test_the_all_codes_case_covers_every_code_exactly(mirrored, h):
    q, k, kscale, weights, ks, ke, want = R.all_codes_case(h, mirrored)
    m, n = (R.MIRROR_M, R.MIRROR_N) if mirrored else (R.CODES_M, R.CODES_N)
    assert q.shape == (m, h, R.D) and k.shape == (n, R.D) and (kscale == 1).all() and R.in_range(ks, ke, n).all()
    assert len(R.FINITE) == 254 and not np.isnan(R.TABLE[R.FINITE]).any() and np.isnan(R.TABLE[[0x7F, 0xFF]]).all()
    assert R.TABLE[R.ONE] == 1 and R.TABLE[R.MINUS_ONE] == -1
    assert not np.isin([0x7F, 0xFF], q).any() and not np.isin([0x7F, 0xFF], k).any()
    # more than one token run and key block, with ragged ends, in one of the two cases each
    assert (m > 4 * R.BM and m % R.BM and n == 2 * R.D) if mirrored else (n > R.BN and n % R.BN and m == 2 * R.D)
    # one weight a token, 1.0, and all 254 codes inside the ranges opposite the unit codes
    assert ((weights != 0).sum(axis=1) == 1).all() and weights.max() == 1 and len(np.unique(weights.argmax(axis=1))) == h
    seen = R.all_codes_seen(h, mirrored)
    assert np.array_equal(seen, R.FINITE) and np.isin(R.SUBNORMAL, seen).all() and 0x80 in seen and len(R.SUBNORMAL) == 14
    # the expected logits: float32 values, relu of +- the code's value, the 127 magnitudes and nothing else
    assert np.isfinite(want).all() and np.array_equal(want.astype(np.float32).astype(np.float64), want)
    magnitudes = np.unique(np.abs(R.TABLE[R.FINITE]))
    assert len(magnitudes) == 127 and magnitudes[1] == 2.0 ** -9 and magnitudes[-1] == 448 and np.array_equal(np.unique(want), magnitudes)
    t, col = np.arange(m)[:, None], np.arange(n)[None, :]
    head = weights.argmax(axis=1)
    if mirrored:
        value = np.where(col < R.D, 1, -1) * R.TABLE[q[np.arange(m), head]][:, np.arange(n) % R.D]
    else:
        value = np.where(t < R.D, 1, -1) * R.TABLE[k][:, np.arange(m) % R.D].T
    assert np.array_equal(want, np.maximum(value, 0))
    assert (value > 0).sum() > m * n // 3 and (value < 0).sum() > m * n // 3
    # any order of summation gives the same float32: every product but one a logit is a zero, or meets a zero weight
    mag = R.reference(q, k, kscale, weights, ks, ke)[1]
    assert np.array_equal(mag, np.abs(value))
    R.assert_same_values(want.astype(np.float32), want)
    R.assert_same_values(np.where(want == 0, -0.0, want).astype(np.float32), want)        # a zero of either sign is zero


@pytest.mark.parametrize("kind", ("subnormal", "sign"))
@pytest.mark.parametrize("mirrored", (False, True), ids=("codes_in_k", "codes_in_q"))
def test_the_value_check_rejects_a_wrong_conversion(mirrored, kind):
    """what a kernel that flushed one subnormal code to zero, or read -0.5 as +0.5, would return"""
    q, k, kscale, weights, ks, ke, want = R.all_codes_case(32, mirrored)
    table = R.broken_table(kind)
    assert (table != R.TABLE)[R.FINITE].sum() == 1
    wrong = R.reference(q, k, kscale, weights, ks, ke, table)[0]
    assert 0 < (wrong != want).sum() < want.size // 50
    with pytest.raises(AssertionError):
        R.assert_same_values(wrong.astype(np.float32), want)
    # on the nine codes of the other exact tests neither fault shows where the code does not occur
    eq, ek, escale, ew = R.exact_operands(5, 15, 32)
    if kind == "subnormal":
        r = R.ranges("full", 5, 15)
        assert np.array_equal(R.reference(eq, ek, escale, ew, *r, table)[0], R.reference(eq, ek, escale, ew, *r)[0])
    # and the checker's other refusals: a NaN, a -inf out of place, one float32 step
    for bad in (np.nan, -np.inf, np.nextafter(np.float32(want[3, 3]), np.float32(1e9))):
        got = want.astype(np.float32)
        got[3, 3] = bad
        with pytest.raises(AssertionError):
            R.assert_same_values(got, want)
