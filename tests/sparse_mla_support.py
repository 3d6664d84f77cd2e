"""What more than one sparse MLA test module uses, in one copy: the operands and refusal loops of the CPU tests (host tensors only), and the
device helpers of the GPU tests -- outputs pre-filled with a NaN pattern, the check against tests/sparse_mla_ref.py, the fp8 cache's views
and dequantised rows.  Nothing here touches a device until a GPU test calls it."""
import ctypes

import numpy as np
import pytest
import torch

import sparse_mla_fp8_ref as F
import sparse_mla_ref as R

NAN_FILL = 0x7FC12345
NAN_FILL16 = 0x7FC5


# ---- CPU: the C entries' and the wrappers' refusals ---------------------------------------------------------------------------------

def _aligned():
    buf = ctypes.create_string_buffer(8192 + 64)
    return buf, (ctypes.addressof(buf) + 63) & ~63


def _refused(dga, bad, accepted):
    for what, call in bad.items():
        with pytest.raises(dga.DGAError) as e:
            call()
        assert "HIP device" not in str(e.value), what                  # refused for what it is, not for where it lives
    for call in accepted:                                               # nothing to refuse but the device
        with pytest.raises(dga.DGAError) as e:
            call()
        assert "HIP device" in str(e.value)


def _args(m=2, h=16, s=8, topk=4):
    q = torch.zeros((m, h, 576), dtype=torch.bfloat16)
    kv = torch.zeros((s, 576), dtype=torch.bfloat16)
    idx = torch.zeros((m, topk), dtype=torch.int32)
    return q, kv, idx


def _cache(nb=3, page=4, pad=0):
    return torch.zeros((nb, page * 656 + pad), dtype=torch.uint8)[:, :page * 656].view(nb, page, 1, 656)


def _bad_caches():
    """every way a cache is refused, by name"""
    return {
        "cache dtype": _cache().view(torch.int8),
        "cache rank": torch.zeros((3, 4, 656), dtype=torch.uint8),
        "cache row width": torch.zeros((3, 4, 1, 640), dtype=torch.uint8),
        "cache flat row width": torch.zeros((12, 576), dtype=torch.uint8),
        "cache third dimension": torch.zeros((3, 2, 2, 656), dtype=torch.uint8),
        "cache empty": _cache()[:0],
        "cache stride(1) != 656": torch.zeros((3, 4, 1, 672), dtype=torch.uint8)[..., :656],
        "cache stride(3) != 1": torch.zeros((3, 4, 1, 1312), dtype=torch.uint8)[..., ::2],
        "cache flat stride(1) != 1": torch.zeros((12, 1312), dtype=torch.uint8)[:, ::2],
        "cache block stride not a multiple of 16": _cache(pad=8),
        "cache flat stride not a multiple of 16": torch.zeros((12, 664), dtype=torch.uint8)[:, :656],
        "cache block stride too small": torch.zeros((3 * 4 * 656,), dtype=torch.uint8).as_strided((3, 4, 1, 656), (3 * 656 + 16, 656, 656, 1)),
        "cache flat stride too small": torch.zeros((12 * 656,), dtype=torch.uint8).as_strided((12, 656), (640, 1)),
        "cache misaligned": torch.zeros((3 * 4 * 656 + 8,), dtype=torch.uint8)[8:].view(3, 4, 1, 656),
        "cache of 2^31 rows": torch.empty((1 << 25, 64, 1, 656), dtype=torch.uint8, device="meta"),      # (no storage behind it)
        "cache flat of 2^31 rows": torch.empty((1 << 31, 656), dtype=torch.uint8, device="meta"),
    }


# ---- GPU: operands, pre-filled outputs, the check against the reference --------------------------------------------------------------

def _bf16(a):
    """the bf16 device tensor of float values that bf16 holds exactly (NaN allowed)"""
    a = np.asarray(a, dtype=np.float32)
    t = torch.from_numpy(a.copy()).to(torch.bfloat16)
    assert np.array_equal(t.float().numpy(), a, equal_nan=True)
    return t.cuda()


def _filled(m, h):
    out = torch.full((m, h, R.D_V), NAN_FILL16, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    lse = torch.full((m, h), NAN_FILL, dtype=torch.int32, device="cuda").view(torch.float32)
    return out, lse


def _check(got, ref, scale, topk, exact_rows=(), out_bound=True):
    """every element of out and lse against the reference: +0 and -inf for a token without a valid position, the bits of
    RNE_bf16(out) on the tokens of exact_rows, the derived bounds everywhere (out_bound=False: of lse alone -- the bound of out is
    relative to the weighted values and has no room for weights that underflow fp32, which the one-hot case is made of)"""
    out, bits, lse = got
    assert not np.isnan(out).any() and not np.isnan(lse).any()
    empty = ref["count"] == 0
    assert (bits[empty] == 0).all() and np.isneginf(lse[empty]).all()
    assert np.isfinite(lse[~empty]).all()
    for t in exact_rows:
        assert np.array_equal(bits[t], R.bf16_bits(ref["out"][t])), t
    err, bar = np.abs(out - ref["out"]), R.bound_out(ref, scale, topk)
    if not out_bound:
        err = np.zeros_like(err)
    assert (err <= bar).all(), (int((err > bar).sum()), np.argwhere(err > bar)[:4])
    lerr, lbar = np.abs(lse[~empty].astype(np.float64) - ref["lse"][~empty]), R.bound_lse(ref, scale, topk)[~empty]
    assert (lerr <= lbar).all(), (float((lerr / lbar).max()), np.argwhere(lerr > lbar)[:4])
    both = float((err[~empty] / np.maximum(bar[~empty], 1e-300)).max()) if (~empty).any() else 0.0
    return both, float((lerr / lbar).max()) if (~empty).any() else 0.0


# ---- GPU: the paged fp8 latent cache -------------------------------------------------------------------------------------------------

def _view(t, page):
    """the operators' view of a uint8 [num_blocks, block_stride] buffer: [num_blocks, page, 1, 656], or flat [S, 656] for page 1"""
    nb = t.shape[0]
    return t[:, :F.ROW] if page == 1 else t[:, :page * F.ROW].view(nb, page, 1, F.ROW)


def _bf16_from_bits(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(torch.bfloat16).cuda()


def _deq_tensor(buf, page):
    """bf16 [S, 576] on the device: the values the rows of a host buffer stand for"""
    return _bf16_from_bits(F.deq_bits(*F.unpack(buf, page)))


def _nan16(b):
    return (b & 0x7FFF) > 0x7F80


def _nan32(b):
    return (b & 0x7FFFFFFF) > 0x7F800000


def _written_by_the_writer(dga, kv, page, pad, fill=0):
    """the host copy of a cache of ceil(S / page) blocks, `pad` bytes between blocks, whose rows 0 .. S - 1 the new writer wrote from the
    bf16 rows kv [S, 576]"""
    s = kv.shape[0]
    nb, stride = F.geometry(s, page, page * F.ROW + pad)
    t = torch.full((nb, stride), fill, dtype=torch.uint8, device="cuda")
    both = _bf16(kv)
    dga.mla_kv_cast_to_fp8_paged(both[:, :F.LATENT], both[:, F.LATENT:], _view(t, page), torch.arange(s, dtype=torch.int64, device="cuda"), sync=True)
    return t.cpu().numpy()
