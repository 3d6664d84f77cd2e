"""CPU: the dense cases indexer_kl_loss_dense's GPU tests run on (a token's range written out as an [M, N] list for the existing references),
the bound its computed lse is held to, the existing reference's room on those cases, and the wrapper's refusals before a launch."""
import functools

import numpy as np
import pytest
import torch

import indexer_kl_ref as K
import mqa_logits_ref as Q
import sparse_mla_ref as R
from sparse_mla_support import _args, _refused

M, N = R.M4, R.S4
KINDS = ("full", "shifted", "windows", "mixed")


def ranges(kind, empty=True):
    """mqa_logits_ref.ranges, or the shifted causal ke = N - M + m + 1; token 3 crossed (empty) unless told otherwise"""
    ks, ke = (np.zeros(M, np.int32), (N - M + 1 + np.arange(M)).astype(np.int32)) if kind == "shifted" else Q.ranges(kind, M, N)
    if empty:
        ks[3], ke[3] = 200, 150
    return ks, ke


def lists(ks, ke):
    """the [M, N] lists the references take: n where in range, -1 elsewhere"""
    return np.where(Q.in_range(ks, ke, N), np.arange(N, dtype=np.int32)[None, :], np.int32(-1)).astype(np.int32)


def bound_lse(fwd, scale):
    """the bar of the computed lse ("Indexer KL loss, dense" derives it): e_s, then in units of u 34 for a term's exponent and
    v_exp_f32, per tile the rescale (3 + log2 n), the tile's partial and eight additions a lane (1 + 8), a range of n keys meeting at
    most ceil(n / 32) + 1 tiles, 34 + 1 + 8 for the merge of a head's eight pairs, and sparse_mla_ref.bound_lse's 4 u (|lse| + ln n)"""
    n = np.maximum(fwd["count"], 2)[:, None].astype(np.float64)
    lse = np.where(np.isfinite(fwd["lse"]), fwd["lse"], 0.0)
    return R.e_s(scale, fwd["mag"]) + (77 + (np.ceil(n / R.TILE) + 1) * (12 + np.log2(n))) * R.U + 4 * R.U * (np.abs(lse) + np.log(n))


@functools.lru_cache(maxsize=None)
def dense_case(h, kind, scale=R.SCALE4, peaked=False):
    """sparse_mla_ref.random_case(h)'s q and kv under ranges of `kind`, logits normal (peaked: uniform over +-40, every range kept) and NaN
    outside the ranges: ((q, kv, ks, ke, logits), lists, the float64 forward reference)"""
    q, kv, _ = R.random_case(h)
    ks, ke = ranges(kind, empty=not peaked)
    rng = np.random.default_rng([h, len(kind)])
    logits = (rng.uniform(-40, 40, (M, N)) if peaked else 3 * rng.standard_normal((M, N))).astype(np.float32)
    logits[~Q.in_range(ks, ke, N)] = np.nan
    idx = lists(ks, ke)
    return R._frozen(q, kv, ks, ke, logits), idx, R.reference(q, kv, idx, scale)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("h", K.HEADS)
def test_the_bounds_leave_room_on_the_dense_lists(h, kind):
    (q, kv, _, _, logits), idx, fwd = dense_case(h, kind)
    ops = (q, kv, idx, fwd["lse"].astype(np.float32), R.SCALE4, logits)
    K.inside(K.kernel_order(*ops, grad_scale=K.GRAD_SCALE), K.reference(*ops, grad_scale=K.GRAD_SCALE))


def test_every_refusal_comes_from_the_wrapper(dga):
    q, kv, _ = _args()
    z = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype)
    good = dict(q=q, kv=kv, ks=z(2, torch.int32), ke=z(2, torch.int32), logits=z((2, 8)))
    call = lambda **kw: (lambda a: dga.indexer_kl_loss_dense(a.pop("q"), a.pop("kv"), a.pop("ks"), a.pop("ke"), a.pop("sm_scale", 0.1), a.pop("logits"), **a))({**good, **kw})
    bad = {
        "logits N != S": lambda: call(logits=z((2, 9))), "logits stride(0) < N": lambda: call(logits=z((8,)).expand(2, 8)), "ks dtype": lambda: call(ks=z(2, torch.int64)),
        "ke rows": lambda: call(ke=z(3, torch.int32)), "ks rank": lambda: call(ks=z((2, 1), torch.int32)), "lse shape": lambda: call(lse=z((2, 32))),
        "lse rank": lambda: call(lse=z((2, 16, 1))), "lse_out shape": lambda: call(lse_out=z((16, 2))), "lse and lse_out": lambda: call(lse=z((2, 16)), lse_out=z((2, 16))),
        "Hq = 24": lambda: call(q=_args(h=24)[0]), "kv stride 580": lambda: call(kv=torch.zeros((8, 580), dtype=torch.bfloat16)[:, :576]), "sm_scale": lambda: call(sm_scale="1"),
        "d_logits columns": lambda: call(d_logits=z((2, 4))), "d_logits strided": lambda: call(d_logits=z((2, 16))[:, ::2]), "target dtype": lambda: call(target=z((2, 8), torch.int32)),
        "loss shape": lambda: call(loss=z((2, 1))), "grad_scale": lambda: call(grad_scale=z(())),
    }
    wide = lambda: call(logits=z((2, 12))[:, 2:10], lse=z((2, 16)), d_logits=z((2, 11))[:, 1:9], target=z((2, 8)), loss=z((2,)), grad_scale=2)
    _refused(dga, bad, (call, wide, lambda: call(lse_out=z((2, 16)), want_target=True)))
