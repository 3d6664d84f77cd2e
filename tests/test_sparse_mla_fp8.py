"""CPU: the fp8 latent cache's reference (tests/sparse_mla_fp8_ref.py) against torch's float8_e4m3fn on every code, pack and unpack under
both cache shapes, the two entries declared, exported and in the ctypes table, the C entries' refusals (none of which launches) and every
refusal the wrappers make (there is no CPU path, so a call with nothing to refuse is refused for its device)."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import sparse_mla_fp8_ref as F
from sparse_mla_support import _aligned, _bad_caches, _cache, _refused

ROOT = Path(__file__).resolve().parent.parent
SCALES = (1.0, 0.3, 2.0 ** -140, 2.0 ** 120, 0.0, -1.5, np.inf, np.nan)   # ordinary, subnormal products, bf16 overflow, zero, negative, inf, NaN


def test_deq_agrees_with_torch_on_every_code_under_every_scale():
    # rows 0, 1: codes 0 .. 127 / 128 .. 255 under scales 0 .. 3; rows 2, 3: the same under scales 4 .. 7
    codes = np.stack([np.tile((np.arange(128) + 128 * half).astype(np.uint8), 4) for _ in range(2) for half in range(2)])
    scales = np.array([SCALES[:4], SCALES[:4], SCALES[4:], SCALES[4:]], np.float32)
    rope = np.arange(4 * 64, dtype=np.uint16).reshape(4, 64) * 251
    got = F.deq_bits(codes, scales, rope)
    assert got.shape == (4, 576) and np.array_equal(got[:, 512:], rope)
    tc = torch.from_numpy(codes).view(torch.float8_e4m3fn)
    want_t = (tc.float() * torch.from_numpy(scales).repeat_interleave(128, -1)).to(torch.bfloat16)
    want = want_t.view(torch.int16).numpy().view(np.uint16)
    nan = torch.isnan(want_t).numpy()
    assert np.array_equal(np.isnan(F.bits_to_f32(got[:, :512])), nan)
    assert np.array_equal(got[:, :512][~nan], want[~nan])
    # what the cases are there for: NaN codes, subnormal and overflowing products, signed zeros, inf and NaN scales
    val = F.bits_to_f32(got[:, :512])
    assert nan[0, 127] and nan[1, 127] and not nan[0, :127].any() and nan[3, 384:].all() and nan[2, 256 + 127]
    sub = val[0, 256:384]                                               # 2^-140 times the positive codes: every product a subnormal float32
    assert ((got[0, 256:383] & 0x7F80) == 0).all() and (sub[:127] >= 0).all()                                   # ... and a subnormal bf16 or zero:
    assert got[0, 256 + 126] == 4 and got[0, 256 + 120] == 2 and got[0, 256 + 8] == 0      # 3.5, 2 and 2^-13 units of 2^-133 (ties to even)
    assert np.isposinf(val[0, 384 + 126]) and np.isneginf(val[1, 384 + 126]) and np.isfinite(val[0, 384 + 64])      # 448 x 2^120 overflows bf16
    assert (got[2, 1:127] == 0).all() and (got[3, 1:127] == 0x8000).all()                                       # scale 0: zeros of the code's sign
    assert val[2, 128 + 126] == -672.0 and np.isposinf(val[2, 256 + 1]) and nan[2, 256] and nan[3, 256]              # inf x 0 is NaN
    # the table itself: torch's value of every code
    table = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float().numpy()
    assert np.array_equal(np.isnan(table), np.isnan(F.E4M3)) and np.array_equal(table[~np.isnan(table)], F.E4M3[~np.isnan(table)])
    assert np.array_equal(np.signbit(table)[~np.isnan(table)], np.signbit(F.E4M3)[~np.isnan(table)])           # (-0 among them)
    assert np.flatnonzero(np.isnan(F.E4M3)).tolist() == list(F.NAN_CODES)


def test_bf16_bits_rounds_to_nearest_even_and_keeps_subnormals():
    rng = np.random.default_rng(1)
    x = rng.standard_normal(4096).astype(np.float32) * np.float32(2.0) ** rng.integers(-149, 127, 4096).astype(np.float32)
    x[:6] = [np.float32(1 + 2.0 ** -8), np.float32(1 + 2.0 ** -7 + 2.0 ** -8), 2.0 ** -133, 2.0 ** -134, np.float32(3.4e38), -0.0]
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(F.bf16_bits(x), want)
    assert F.bf16_bits(x)[:6].tolist() == [0x3F80, 0x3F82, 0x0001, 0x0000, 0x7F80, 0x8000]


@pytest.mark.parametrize("page,pad", ((1, 0), (1, 48), (16, 16), (64, 0), (64, 304)))
def test_pack_then_unpack_is_the_identity(page, pad):
    rng = np.random.default_rng(page + pad)
    s = 3 * page + (page + 1) // 2                                      # a partly filled last block
    codes = rng.integers(0, 256, (s, 512)).astype(np.uint8)
    scales = rng.standard_normal((s, 4)).astype(np.float32)
    rope = rng.integers(0, 65536, (s, 64)).astype(np.uint16)
    stride = page * F.ROW + pad
    buf = F.pack(codes, scales, rope, page, stride, fill=0xEE)
    nb = -(-s // page)
    assert buf.shape == (nb, stride) and buf.dtype == np.uint8
    c2, s2, r2 = F.unpack(buf, page, s)
    assert np.array_equal(c2, codes) and np.array_equal(s2.view(np.uint32), scales.view(np.uint32)) and np.array_equal(r2, rope)
    # every byte that is no row's is the fill: the padding between blocks and the rows beyond S
    mask = F.row_bytes_mask(np.arange(s), nb, page, stride)
    assert mask.sum() == s * F.ROW and (buf[~mask] == 0xEE).all() and (~mask).sum() == nb * stride - s * F.ROW
    # a row where the layout says: row s - 1, byte by byte
    at = int(F.row_at(s - 1, page, stride))
    flat = buf.reshape(-1)
    assert at == (s - 1) // page * stride + (s - 1) % page * 656
    assert np.array_equal(flat[at:at + 512], codes[-1]) and np.array_equal(flat[at + 512:at + 528].view(np.float32).view(np.uint32), scales[-1].view(np.uint32))
    assert np.array_equal(flat[at + 528:at + 656].view(np.uint16), rope[-1])
    # the torch view the operators take
    t = torch.from_numpy(buf)
    view = t[:, :page * F.ROW].view(nb, page, 1, F.ROW) if page > 1 else t[:, :F.ROW]
    assert view.stride(0) == stride and view.stride(-1) == 1
    assert np.array_equal(view.reshape(-1, F.ROW)[:s, :512].numpy(), codes)


def test_the_writers_reference_touches_its_rows_only(oracle):
    rng = np.random.default_rng(5)
    page, stride, nb = 16, 16 * F.ROW + 32, 3
    buf = rng.integers(0, 256, (nb, stride)).astype(np.uint8)
    kv_c = rng.standard_normal((6, 512)).astype(np.float32)
    k_pe = rng.standard_normal((6, 64)).astype(np.float32)
    slots = np.array([47, -1, 0, nb * page, 17, -2 ** 63], np.int64)
    out = F.written(buf, kv_c, F.bf16_bits(k_pe), slots, page, oracle.quant_1x128)
    mask = F.row_bytes_mask([47, 0, 17], nb, page, stride)
    assert np.array_equal(out[~mask], buf[~mask]) and mask.sum() == 3 * F.ROW
    codes, scales, rope = F.unpack(out, page)
    wq, wsf = oracle.quant_1x128(kv_c[[0, 2, 4]])
    assert np.array_equal(codes[[47, 0, 17]], wq) and np.array_equal(scales[[47, 0, 17]].view(np.uint32), wsf.view(np.uint32))
    assert np.array_equal(rope[[47, 0, 17]], F.bf16_bits(k_pe[[0, 2, 4]]))
    # and the value of a written row is within the quantisation step of its input
    val = F.deq(codes[[47]], scales[[47]], rope[[47]])[0]
    assert np.abs(val[:512] - kv_c[0]).max() <= np.abs(kv_c[0]).max() / 448 * 32 and np.array_equal(F.bf16_bits(val[512:]), F.bf16_bits(k_pe[0]))


def test_symbols_are_declared_exported_and_in_the_table(dga):
    from deepgemm_ascend_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "dga_hip.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+dga_sparse_mla_fwd_fp8\s*\(", text) and re.search(r"\bint\s+dga_cast_mla_kv_to_fp8_paged\s*\(", text)
    assert re.search(r"#define\s+DGA_SPARSE_MLA_FP8_ROW_BYTES\s+656\b", text)
    so = ctypes.CDLL(str(_lib.LIB_PATH))
    assert hasattr(so, "dga_sparse_mla_fwd_fp8") and hasattr(so, "dga_cast_mla_kv_to_fp8_paged")
    restype, argtypes = _lib.SIGNATURES["dga_sparse_mla_fwd_fp8"]
    assert restype is ctypes.c_int and len(argtypes) == 16
    restype, argtypes = _lib.SIGNATURES["dga_cast_mla_kv_to_fp8_paged"]
    assert restype is ctypes.c_int and len(argtypes) == 13
    assert dga.SPARSE_MLA_FP8_ROW_BYTES == 656 == F.ROW and callable(dga.sparse_mla_fwd_fp8) and callable(dga.mla_kv_cast_to_fp8_paged)
    assert "sparse_mla_fwd_fp8" in dga.__all__ and "mla_kv_cast_to_fp8_paged" in dga.__all__
    assert _lib.lib().dga_abi_version() == 7                            # the change only adds


def test_attention_c_entry_checks_before_any_launch(dga):
    """the C entry's own refusals and M == 0, none of which touches a device"""
    from deepgemm_ascend_amd import _lib
    L = _lib.lib()
    buf, p = _aligned()

    def call(q=p, kv=p, idx=p, off=None, m=1, heads=16, nb=2, page=4, stride=4 * 656, topk=2, idx_stride=2, flags=0, out=p, lse=p):
        return L.dga_sparse_mla_fwd_fp8(q, kv, idx, off, m, heads, nb, page, stride, topk, idx_stride, 0.1, flags, out, lse, None)

    codes = {call(m=-1), call(heads=8), call(heads=144), call(heads=24), call(nb=0), call(page=0), call(topk=0), call(stride=4 * 656 - 16),
             call(stride=0), call(idx_stride=1), call(page=1 << 62)}
    assert len(codes) == 1 and 0 not in codes                                      # one status: the shape
    assert call(m=0) == 0 and call(m=0, q=None, out=None, kv=None) == 0
    assert call(q=None) == call(lse=None) == call(idx=None) == call(kv=None) != 0 and call(q=None) not in codes
    a = call(kv=p + 8)
    assert a != 0 and a == call(q=p + 2) == call(out=p + 4) == call(lse=p + 2) == call(off=p + 1) == call(stride=4 * 656 + 8) and a not in codes
    r = call(flags=2)
    assert r != 0 and r not in codes and r != a
    assert r == call(nb=1 << 29, page=4) == call(nb=1 << 31, page=1, stride=656) == call(nb=1 << 30, page=1, stride=1 << 34)
    # the same statuses as the bf16 entry's, refusal by refusal
    def bf16(q=p, kv=p, m=1, heads=16, s=4, flags=0):
        return L.dga_sparse_mla_fwd(q, kv, p, None, m, heads, s, 576, 2, 2, 0.1, flags, p, p, None)
    assert bf16(heads=8) in codes and bf16(q=None) == call(q=None) and bf16(kv=p + 8) == a and bf16(flags=2) == r == bf16(s=1 << 31)


def test_writer_c_entry_checks_before_any_launch(dga):
    from deepgemm_ascend_amd import _lib
    L = _lib.lib()
    buf, p = _aligned()

    def call(kv_c=p, ld_c=512, k_pe=p, ld_pe=64, dtype=_lib.DT_BF16, tokens=3, cache=p, nb=2, page=4, stride=4 * 656, slots=p, flags=0):
        return L.dga_cast_mla_kv_to_fp8_paged(kv_c, ld_c, k_pe, ld_pe, dtype, tokens, cache, nb, page, stride, slots, flags, None)

    codes = {call(tokens=-1), call(nb=0), call(page=0), call(stride=4 * 656 - 16), call(ld_c=504), call(ld_pe=56), call(page=1 << 62)}
    assert len(codes) == 1 and 0 not in codes
    assert call(tokens=0) == 0 and call(tokens=0, kv_c=None, k_pe=None, cache=None, slots=None) == 0
    n = call(kv_c=None)
    assert n != 0 and n == call(k_pe=None) == call(cache=None) == call(slots=None) and n not in codes
    d = call(dtype=99)
    assert d != 0 and d not in codes and d != n
    a = call(kv_c=p + 8)
    assert a != 0 and a == call(k_pe=p + 4) == call(cache=p + 8) == call(slots=p + 4) == call(stride=4 * 656 + 8) == call(ld_c=516) == call(ld_pe=68)
    assert a == call(dtype=_lib.DT_FP32, ld_c=514) and call(dtype=_lib.DT_FP32, ld_c=516, tokens=0) == 0 and a not in codes and a not in (n, d)
    r = call(flags=2)
    assert r != 0 and r not in codes and r not in (n, d, a)
    assert r == call(nb=1 << 29, page=4) == call(nb=1 << 30, page=1, stride=1 << 34) == call(ld_c=1 << 61) == call(ld_pe=1 << 61)
    assert r == call(tokens=1 << 40, ld_c=1 << 24)                      # tokens times the row pitch leaves int64


def _args(m=2, h=16, topk=4):
    return torch.zeros((m, h, 576), dtype=torch.bfloat16), _cache(), torch.zeros((m, topk), dtype=torch.int32)


def test_every_attention_refusal_comes_from_the_wrapper(dga):
    q, cache, idx = _args()
    bad = {
        "q dtype": lambda: dga.sparse_mla_fwd_fp8(q.float(), cache, idx, 0.1),
        "q rank": lambda: dga.sparse_mla_fwd_fp8(q[0], cache, idx, 0.1),
        "q d": lambda: dga.sparse_mla_fwd_fp8(torch.zeros((2, 16, 512), dtype=torch.bfloat16), cache, idx, 0.1),
        "q not contiguous": lambda: dga.sparse_mla_fwd_fp8(torch.zeros((2, 32, 576), dtype=torch.bfloat16)[:, ::2], cache, idx, 0.1),
        "Hq = 8": lambda: dga.sparse_mla_fwd_fp8(_args(h=8)[0], cache, idx, 0.1),
        "Hq = 24": lambda: dga.sparse_mla_fwd_fp8(_args(h=24)[0], cache, idx, 0.1),
        "Hq = 144": lambda: dga.sparse_mla_fwd_fp8(_args(h=144)[0], cache, idx, 0.1),
        "d_v": lambda: dga.sparse_mla_fwd_fp8(q, cache, idx, 0.1, 576),
        "a bf16 cache": lambda: dga.sparse_mla_fwd_fp8(q, torch.zeros((8, 576), dtype=torch.bfloat16), idx, 0.1),
        "indices dtype": lambda: dga.sparse_mla_fwd_fp8(q, cache, idx.long(), 0.1),
        "indices rank": lambda: dga.sparse_mla_fwd_fp8(q, cache, idx[0], 0.1),
        "indices rows": lambda: dga.sparse_mla_fwd_fp8(q, cache, idx[:1], 0.1),
        "indices empty": lambda: dga.sparse_mla_fwd_fp8(q, cache, idx[:, :0], 0.1),
        "indices last dimension strided": lambda: dga.sparse_mla_fwd_fp8(q, cache, torch.zeros((2, 8), dtype=torch.int32)[:, ::2], 0.1),
        "offsets dtype": lambda: dga.sparse_mla_fwd_fp8(q, cache, idx, 0.1, index_offsets=torch.zeros(2, dtype=torch.int64)),
        "offsets shape": lambda: dga.sparse_mla_fwd_fp8(q, cache, idx, 0.1, index_offsets=torch.zeros(3, dtype=torch.int32)),
        "out shape": lambda: dga.sparse_mla_fwd_fp8(q, cache, idx, 0.1, out=torch.zeros((2, 16, 576), dtype=torch.bfloat16)),
        "out dtype": lambda: dga.sparse_mla_fwd_fp8(q, cache, idx, 0.1, out=torch.zeros((2, 16, 512), dtype=torch.float32)),
        "lse shape": lambda: dga.sparse_mla_fwd_fp8(q, cache, idx, 0.1, lse=torch.zeros((2, 16, 1), dtype=torch.float32)),
        "lse dtype": lambda: dga.sparse_mla_fwd_fp8(q, cache, idx, 0.1, lse=torch.zeros((2, 16), dtype=torch.bfloat16)),
    }
    for what, c in _bad_caches().items():
        bad[what] = (lambda c: lambda: dga.sparse_mla_fwd_fp8(q, c, idx, 0.1))(c)
    flat = torch.zeros((12, 672), dtype=torch.uint8)[:, :656]
    _refused(dga, bad, (lambda: dga.sparse_mla_fwd_fp8(q, cache, idx, 0.1),
                        lambda: dga.sparse_mla_fwd_fp8(q, _cache(pad=48), idx.view(2, 1, 4), 0.1, 512, torch.zeros(2, dtype=torch.int32)),
                        lambda: dga.sparse_mla_fwd_fp8(q, flat, torch.zeros((2, 9), dtype=torch.int32)[:, :4], 0.1),
                        lambda: dga.sparse_mla_fwd_fp8(q, torch.zeros((1, 1, 1, 656), dtype=torch.uint8), idx, 0.1)))


def test_every_writer_refusal_comes_from_the_wrapper(dga):
    cache = _cache()
    kv_c, k_pe, slots = torch.zeros((5, 512), dtype=torch.bfloat16), torch.zeros((5, 64), dtype=torch.bfloat16), torch.zeros(5, dtype=torch.int64)
    both = torch.zeros((5, 576), dtype=torch.float32)
    bad = {
        "kv_c width": lambda: dga.mla_kv_cast_to_fp8_paged(torch.zeros((5, 576), dtype=torch.bfloat16), k_pe, cache, slots),
        "kv_c rank": lambda: dga.mla_kv_cast_to_fp8_paged(kv_c[0], k_pe, cache, slots),
        "k_pe width": lambda: dga.mla_kv_cast_to_fp8_paged(kv_c, torch.zeros((5, 128), dtype=torch.bfloat16), cache, slots),
        "k_pe rows": lambda: dga.mla_kv_cast_to_fp8_paged(kv_c, k_pe[:4], cache, slots),
        "kv_c dtype": lambda: dga.mla_kv_cast_to_fp8_paged(kv_c.double(), k_pe.double(), cache, slots),
        "mixed dtypes": lambda: dga.mla_kv_cast_to_fp8_paged(kv_c, k_pe.half(), cache, slots),
        "mixed dtypes, fp32": lambda: dga.mla_kv_cast_to_fp8_paged(kv_c.float(), k_pe, cache, slots),
        "kv_c last dimension strided": lambda: dga.mla_kv_cast_to_fp8_paged(torch.zeros((5, 1024), dtype=torch.bfloat16)[:, ::2], k_pe, cache, slots),
        "kv_c rows not a multiple of 16 bytes apart": lambda: dga.mla_kv_cast_to_fp8_paged(torch.zeros((5, 516), dtype=torch.bfloat16)[:, :512], k_pe, cache, slots),
        "k_pe misaligned": lambda: dga.mla_kv_cast_to_fp8_paged(kv_c, torch.zeros((5, 72), dtype=torch.bfloat16)[:, 4:68], cache, slots),
        "slot_mapping dtype": lambda: dga.mla_kv_cast_to_fp8_paged(kv_c, k_pe, cache, slots.int()),
        "slot_mapping shape": lambda: dga.mla_kv_cast_to_fp8_paged(kv_c, k_pe, cache, slots[:4]),
        "slot_mapping strided": lambda: dga.mla_kv_cast_to_fp8_paged(kv_c, k_pe, cache, torch.zeros(10, dtype=torch.int64)[::2]),
    }
    for what, c in _bad_caches().items():
        bad[what] = (lambda c: lambda: dga.mla_kv_cast_to_fp8_paged(kv_c, k_pe, c, slots))(c)
    _refused(dga, bad, (lambda: dga.mla_kv_cast_to_fp8_paged(kv_c, k_pe, cache, slots),
                        lambda: dga.mla_kv_cast_to_fp8_paged(both[:, :512], both[:, 512:], _cache(pad=16), slots, use_ue8m0=True),
                        lambda: dga.mla_kv_cast_to_fp8_paged(kv_c.half(), k_pe.half(), torch.zeros((12, 656), dtype=torch.uint8), slots)))
