"""CPU: tests/indexer_kl_ref.py against float64 autograd of the dense definition, its bounds against the kernel's own roundings, and every
refusal of indexer_kl_loss's wrapper before a launch."""
import numpy as np
import pytest
import torch

import indexer_kl_ref as K
import sparse_mla_ref as R
from sparse_mla_support import _args, _refused


def test_the_reference_is_autograd_of_the_dense_definition():
    """dense: softmax over all S rows, every row weighted by how often the list names it, -inf logits outside the list; lse in float64;
    offsets given; the derivative at a row is the sum of d_logits over the positions that name it"""
    q, kv, _ = R.random_case(16)
    off = -np.arange(1, 6, dtype=np.int32)
    idx = K.lists(33, seed=3, n=R.S4)
    idx = np.where(idx >= 0, idx - off[:, None], idx).astype(np.int32)
    rows, valid = R.rows_of(idx, R.S4, off)
    count = np.zeros((R.M4, R.S4))
    for t in range(R.M4):
        np.add.at(count[t], rows[t][valid[t]], 1)
    logits = np.where(count > 0, np.random.default_rng(0).standard_normal(count.shape), -np.inf)
    ref = K.reference(q, kv, idx, R.reference(q, kv, idx, R.SCALE4, off)["lse"], R.SCALE4, logits, off, grad_scale=K.GRAD_SCALE)
    keep = valid.any(1)
    c, named = torch.tensor(count[keep]), torch.tensor(count[keep] > 0)
    lt = torch.tensor(np.where(count > 0, logits, 0.0)[keep], requires_grad=True)
    mass = torch.softmax(R.SCALE4 * torch.einsum("thd,sd->ths", torch.tensor(q[keep], dtype=torch.float64), torch.tensor(kv, dtype=torch.float64))
                         + c.log()[:, None, :], dim=2).mean(1)
    a = torch.log_softmax(torch.where(named, lt + c.log(), torch.tensor(-np.inf, dtype=torch.float64)), dim=1) - c.log()
    loss = torch.where(named, mass * ((mass / c).log() - a), torch.tensor(0.0, dtype=torch.float64)).sum(1)
    (K.GRAD_SCALE * loss).sum().backward()
    dense = np.zeros(count.shape)
    for t in range(R.M4):
        np.add.at(dense[t], rows[t][valid[t]], ref["dl"][t, valid[t]])
    assert np.abs(ref["loss"][keep] - loss.detach().numpy()).max() <= 1e-12 * np.abs(ref["loss"]).max()
    assert np.abs(dense[keep] - lt.grad.numpy()).max() <= 1e-12 * np.abs(dense).max()
    assert (~keep).any() and not ref["loss"][~keep].any() and not ref["dl"][~valid].any() and count.max() > 1 and np.abs(ref["t"].sum(1)[keep] - 1).max() < 1e-12


@pytest.mark.parametrize("topk", K.TOPKS)
@pytest.mark.parametrize("h", K.HEADS)
def test_the_bounds_leave_room_for_the_kernels_roundings(h, topk):
    """the definition in float32 in the kernel's order of operations stays inside the bounds on the GPU bound test's inputs"""
    ops, ref = K.random_case(h, topk)
    K.inside(K.kernel_order(*ops, grad_scale=K.GRAD_SCALE), ref)


def test_every_refusal_comes_from_the_wrapper(dga):
    q, kv, idx = _args()
    z = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype)
    good = dict(lse=z((2, 16)), logits=z((2, 8)))
    call = lambda q=q, kv=kv, idx=idx, **kw: (lambda a: dga.indexer_kl_loss(q, kv, idx, a.pop("lse"), a.pop("sm_scale", 0.1), a.pop("logits"), **a))({**good, **kw})
    bad = {
        "q dtype": lambda: call(q=q.float()), "Hq = 24": lambda: call(q=_args(h=24)[0]), "kv stride 580": lambda: call(kv=torch.zeros((8, 580), dtype=torch.bfloat16)[:, :576]),
        "indices dtype": lambda: call(idx=idx.long()), "offsets dtype": lambda: call(index_offsets=z((2,))), "sm_scale": lambda: call(sm_scale="1"),
        "lse dtype": lambda: call(lse=z((2, 16), torch.bfloat16)), "lse shape": lambda: call(lse=z((2, 16, 1))), "lse strided": lambda: call(lse=z((2, 32))[:, ::2]),
        "logits dtype": lambda: call(logits=z((2, 8), torch.bfloat16)), "logits N != S": lambda: call(logits=z((2, 9))), "logits rank": lambda: call(logits=z((2, 1, 8))),
        "logits last dimension strided": lambda: call(logits=z((2, 16))[:, ::2]), "logits stride(0) < N": lambda: call(logits=z((8,)).expand(2, 8)),
        "loss dtype": lambda: call(loss=z((2,), torch.float64)), "loss shape": lambda: call(loss=z((2, 1))),
        "d_logits dtype": lambda: call(d_logits=z((2, 4), torch.bfloat16)), "d_logits shape": lambda: call(d_logits=z((2, 5))), "d_logits strided": lambda: call(d_logits=z((2, 8))[:, :4]),
        "target dtype": lambda: call(target=z((2, 4), torch.int32)), "target shape": lambda: call(target=z((4, 2))), "grad_scale": lambda: call(grad_scale=z(())),
    }
    wide = lambda: call(logits=z((2, 12))[:, 2:10], idx=torch.zeros((2, 9), dtype=torch.int32)[:, :4], index_offsets=torch.zeros(2, dtype=torch.int32),
                        loss=z((2,)), d_logits=z((2, 4)), target=z((2, 4)), grad_scale=2)
    _refused(dga, bad, (call, wide))
