"""CPU: mla_bwd_dense's entries declared, exported and in the ctypes table, the wrapper's refusals before a launch, the workspace size, the
operands its GPU tests run on (test_indexer_kl_dense.dense_case with what a backward is given: out and lse of the float64 forward
reference rounded to bf16 / fp32, d_out seeded normal bf16) and the room sparse_mla_bwd_ref's bounds leave on them.
The bounds are the sparse backward's, unchanged: the per-tile arithmetic is its phases A, B and C; dq sums over at most N + 32 positions
(an unaligned range of n keys meets at most ceil(n / 32) + 1 tiles); dkv's sum -- a chunk's blocks on the matrix pipe, then the chunks
and the prior -- is one fixed order of the 2 Hq n terms that bound_dkv allows in any order, a chunk without a term adding an exact 0
("Dense MLA attention, backward")."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import sparse_mla_bwd_ref as B
import sparse_mla_ref as R
from deepgemm_ascend_amd import _lib
from sparse_mla_support import _args, _refused
from test_indexer_kl_dense import KINDS, N, dense_case


@functools.lru_cache(maxsize=None)
def operands(h, kind):
    """((q, kv, ks, ke, out, lse, d_out), the ranges as [M, N] lists), read-only"""
    (q, kv, ks, ke, _), idx, fwd = dense_case(h, kind)
    d_out = torch.randn(fwd["out"].shape, generator=torch.Generator(device="cpu").manual_seed(7 + h)).to(torch.bfloat16).float().numpy()
    out = R.bf16_round(fwd["out"].astype(np.float32)).astype(np.float32)
    return R._frozen(q, kv, ks, ke, out, fwd["lse"].astype(np.float32), d_out), idx


@functools.lru_cache(maxsize=None)
def expected(h, kind, rounded=False):
    (q, kv, _, _, out, lse, d_out), idx = operands(h, kind)
    return B.reference(q, kv, out, d_out, idx, lse, R.SCALE4, rounded=rounded)


def test_the_entries_are_exported(dga):
    so = ctypes.CDLL(str(_lib.LIB_PATH))
    assert all(hasattr(so, n) and n in _lib.SIGNATURES for n in ("dga_mla_bwd_dense", "dga_mla_bwd_dense_workspace_bytes"))
    assert "mla_bwd_dense" in dga.__all__ and callable(dga.mla_bwd_dense)


def test_every_refusal_comes_from_the_wrapper(dga):
    q, kv, _ = _args()
    z = lambda shape, dtype=torch.bfloat16: torch.zeros(shape, dtype=dtype)
    f32, i32 = torch.float32, torch.int32
    good = dict(q=q, kv=kv, out=z((2, 16, 512)), d_out=z((2, 16, 512)), ks=z(2, i32), ke=z(2, i32), lse=z((2, 16), f32))
    call = lambda **kw: (lambda a: dga.mla_bwd_dense(*(a.pop(k) for k in ("q", "kv", "out", "d_out", "ks", "ke", "lse")), a.pop("sm_scale", 0.1), **a))({**good, **kw})
    odd = lambda n, dtype: torch.zeros(n + 1, dtype=dtype)[1:]                           # a base 2 or 4 bytes off 16
    bad = {
        "ks dtype": lambda: call(ks=z(2, torch.int64)), "ke rank": lambda: call(ke=z((1, 2), i32)), "ks length": lambda: call(ks=z(3, i32)),
        "Hq = 24": lambda: call(q=_args(h=24)[0]), "kv stride 580": lambda: call(kv=z((8, 580))[:, :576]), "sm_scale": lambda: call(sm_scale="1"),
        "d_v": lambda: call(d_v=576), "out dtype": lambda: call(out=z((2, 16, 512), f32)), "out strided": lambda: call(out=z((2, 16, 1024))[:, :, ::2]),
        "d_out shape": lambda: call(d_out=z((2, 8, 512))), "d_out misaligned": lambda: call(d_out=odd(2 * 16 * 512, torch.bfloat16).view(2, 16, 512)),
        "lse dtype": lambda: call(lse=z((2, 16))), "lse shape": lambda: call(lse=z((2, 16, 1), f32)), "dq shape": lambda: call(dq=z((2, 16, 512))),
        "dq misaligned": lambda: call(dq=odd(2 * 16 * 576, torch.bfloat16).view(2, 16, 576)), "dkv dtype": lambda: call(dkv=z((8, 576))),
        "dkv rows": lambda: call(dkv=z((7, 576), f32)), "dkv stride 578": lambda: call(dkv=z((8, 578), f32)[:, :576]),
        "dkv misaligned": lambda: call(dkv=odd(8 * 576, f32).view(8, 576)),
    }
    given = lambda: call(kv=z((8, 1, 584))[..., :576], dkv=z((8, 640), f32)[:, :576], dq=z((2, 16, 576)), _flags=1)
    _refused(dga, bad, (call, given))


def test_the_workspace_is_a_function_of_the_shape_and_splits_the_test_cases():
    ws = _lib.lib().dga_mla_bwd_dense_workspace_bytes
    assert ws(0, 16, N) == ws(5, 24, N) == ws(5, 144, N) == ws(5, 16, 0) == 0
    assert ws(5, 128, N) == ws(5, 128, N) and ws(4096, 128, 32768) == ws(4096, 128, 32768) > 0
    one_chunk = lambda m, h: -(-N // 32) * 32 * (576 * 4 + 4) + m * h * 4                # partials, named flags, delta
    assert ws(5, 128, N) > one_chunk(5, 128) and ws(5, 16, N) > one_chunk(5, 16) and ws(5, 16, N) <= ws(5, 128, N)


@pytest.mark.parametrize("kind", KINDS)
def test_the_bounds_leave_room_on_the_dense_lists(kind):
    """the reference with p, dS and dq rounded to bf16 as the kernels round them stays inside the bounds the GPU tests use"""
    h = 48
    ref, got = expected(h, kind), expected(h, kind, True)
    assert (np.abs(got["dq"] - ref["dq"]) <= B.bound_dq(ref, N + 32)).all() and (np.abs(got["dkv"] - ref["dkv"]) <= B.bound_dkv(ref, h)).all()
    assert ref["count"].any() and not ref["dq"][3].any() and np.abs(ref["dq"][0]).min() > 0
