"""CPU: the float32 definitions of tests/indexer_prepare_ref.py inside their derived bounds against float64, the backward the transpose of the
forward's linear part, and every refusal of the three wrappers raised before the device guard."""
import re

import numpy as np
import pytest
import torch

import indexer_prepare_ref as P

EPS = 1e-6


@pytest.mark.parametrize("dtype,interleaved", [("fp32", False), ("bf16", True), ("fp16", False)])
def test_float32_definitions_stay_inside_their_bounds(dtype, interleaved):
    x = P.rows(300, dtype, scale=3.0) + P.to_dtype(np.linspace(-4, 4, 300)[:, None], dtype)      # (rows with a mean far from zero too)
    cs = P.table(300)
    r = P.rope32(x, cs, interleaved)
    assert np.abs(r - P.rope64(x, cs, interleaved)).max() <= 3 * P.U * np.abs(x).max() * 2
    err = np.abs(P.hadamard32(r) - P.hadamard64(r))
    bar = P.ROT_BAR * np.abs(r).astype(np.float64).sum(axis=1, keepdims=True) * float(P.C)
    print("rotation: worst error / bound", float((err / bar).max()))
    assert (err <= bar).all()
    mean, rstd = P.stats32(x, EPS)
    mu, _ = P.stats64(x, EPS)
    _, want = P.stats64(x, EPS, mean)
    print("mean, rstd: worst error / bound", float((np.abs(mean - mu) / (P.MEAN_BAR * np.abs(x).mean(axis=1))).max()),
          float((np.abs(rstd / want - 1) / P.RSTD_BAR).max()))
    assert (np.abs(mean - mu) <= P.MEAN_BAR * np.abs(x).mean(axis=1)).all() and (np.abs(rstd / want - 1) <= P.RSTD_BAR).all()
    gamma, beta = P.rows(1, dtype, 5)[0], P.rows(1, dtype, 6)[0]
    ln = torch.nn.functional.layer_norm(torch.from_numpy(x).double(), (P.D,), torch.from_numpy(gamma).double(), torch.from_numpy(beta).double(), EPS)
    assert np.abs(P.norm32(x, mean, rstd, gamma, beta) - ln.numpy()).max() <= 1e-4


@pytest.mark.parametrize("interleaved", [False, True])
def test_backward_is_the_transpose_of_the_forward_in_float64(interleaved):
    x, g, cs = P.rows(40, "fp32", 1), P.rows(40, "fp32", 2), P.table(40)
    lhs = (P.hadamard64(P.rope64(x, cs, interleaved)) * g).sum()
    rhs = (x * P.rope64(P.hadamard64(g), cs, interleaved, transposed=True)).sum()
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs)
    # ... and the float32 backward is that function: within the forward's bounds of it
    got, want = P.backward32(g, cs, interleaved), P.rope64(P.hadamard64(g), cs, interleaved, transposed=True)
    assert (np.abs(got - want) <= (P.ROT_BAR + 4 * P.U) * np.abs(g).sum(axis=1, keepdims=True) * float(P.C) * 2).all()


def _t(*shape, dtype=torch.bfloat16):
    return torch.zeros(shape, dtype=dtype)


Q, K, G, POS, CS = _t(4, 2, 128), _t(4, 128), _t(4, 2, 128, dtype=torch.float32), _t(4, dtype=torch.int32), _t(9, 64, dtype=torch.float32)
CACHE, SLOTS = _t(2, 8448, dtype=torch.uint8), _t(4, dtype=torch.int64)
REFUSALS = [
    ("q", (_t(4, 2, 128, dtype=torch.int32), POS, CS), {}, "q must be float32, bfloat16 or float16"),
    ("q", (_t(4, 2, 64), POS, CS), {}, "q must be [M, H, 128]"),
    ("q", (_t(4, 2, 136)[:, :, 8:], POS, CS), {}, "q must be contiguous [4, 2, 128]"),
    ("q", (_t(4 * 2 * 128 + 4)[4:].view(4, 2, 128), POS, CS), {}, "q must be 16-byte aligned"),
    ("q", (Q, POS.float(), CS), {}, "positions must be contiguous int32 or int64 [4]"),
    ("q", (Q, POS, _t(9, 32, dtype=torch.float32)), {}, "cos_sin must be [P, 64]: cos in columns 0 .. 31, sin in 32 .. 63"),
    ("q", (Q, POS, _t(9 * 64 + 1, dtype=torch.float32)[1:].view(9, 64)), {}, "cos_sin must be 16-byte aligned"),
    ("q", (Q, POS, CS), dict(weights=_t(4, 2, dtype=torch.float16)), "weights must be contiguous float32 or bfloat16 [4, 2]"),
    ("k", (_t(4, 2, 128), POS, CS), {}, "k must be [N, 128]"),
    ("k", (K, POS, CS), dict(norm_bias=_t(128)), "norm_bias needs norm_weight"),
    ("k", (K, POS, CS), dict(norm_weight=_t(128, dtype=torch.float16)), "norm_weight must be contiguous bfloat16 or float32 [128]"),
    ("k", (K, POS, CS), dict(kv_cache=CACHE), "kv_cache and slot_mapping go together"),
    ("k", (K, POS, CS), dict(contiguous=False), "one of contiguous and kv_cache must be asked for"),
    ("k", (K, POS, CS), dict(kv_cache=CACHE, slot_mapping=SLOTS.int()), "slot_mapping must be contiguous int64 [4]"),
    ("backward", (G.bfloat16(), POS, CS), {}, "grad must be float32"),
    ("backward", (_t(4, 130, dtype=torch.float32)[:, :128], POS, CS), {},
     "grad must have a contiguous last dimension and a stride(0) >= 128 that is a multiple of 4, got 130"),
    ("backward", (G, POS, CS), dict(row_div=_t(4, dtype=torch.float32)), "row_div must be contiguous float32 [4, 2]"),
    ("backward", (G, POS, CS), dict(d_weights=_t(4, 2, dtype=torch.float32)), "d_weights needs row_div"),
    ("backward", (G, POS, CS), dict(out_dtype=torch.float64), "out_dtype must be float32, bfloat16 or float16"),
    # ... and a call that passes every check gets as far as the device guard
    ("q", (Q, POS, CS), dict(weights=_t(4, 2)), "tensors must be on a HIP device (there is no CPU path)"),
    ("k", (K, POS, CS), dict(norm_weight=_t(128), norm_bias=_t(128), kv_cache=CACHE, slot_mapping=SLOTS), "tensors must be on a HIP device (there is no CPU path)"),
    ("backward", (G, POS, CS), dict(row_div=_t(4, 2, dtype=torch.float32), d_weights=_t(4, 2, dtype=torch.float32)),
     "tensors must be on a HIP device (there is no CPU path)"),
]


@pytest.mark.parametrize("op,args,kwargs,message", REFUSALS, ids=[f"{r[0]}-{i}" for i, r in enumerate(REFUSALS)])
def test_refusals_come_before_the_device_guard(dga, op, args, kwargs, message):
    with pytest.raises(dga.DGAError, match=re.escape(message)):
        getattr(dga, "indexer_prepare_" + op)(*args, **kwargs)
