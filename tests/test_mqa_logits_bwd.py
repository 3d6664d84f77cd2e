"""CPU: tests/mqa_logits_bwd_ref.py against float64 autograd and the design's own roundings; fp8_mqa_logits_bwd's refusals before the device guard."""
import numpy as np
import pytest
import torch

import mqa_logits_bwd_ref as B
import mqa_logits_ref as Q
import sparse_mla_ref as R
from sparse_mla_support import _refused


@pytest.mark.parametrize("h", Q.HEADS)
def test_reference_is_float64_autograd_of_the_dense_masked_definition(h):
    """every key weighted by the d_logits of the valid positions that name it; dk is the gradient at the dequantised key kscale k"""
    (q, k, ks, w, idx, dl), ref = B.random_case(h)
    rows, valid = R.rows_of(idx, B.N)
    dense = torch.zeros((B.M, B.N), dtype=torch.float64)
    for t in range(B.M):
        dense[t].index_add_(0, torch.from_numpy(rows[t][valid[t]]), torch.from_numpy(dl[t][valid[t]]).double())
    qt, kt, wt = (torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in (Q.TABLE[q], Q.TABLE[k] * ks[:, None].astype(np.float64), w))
    ((wt[:, :, None] * torch.relu(torch.einsum("mhd,nd->mhn", qt, kt))).sum(1) * dense).sum().backward()
    for got, want in ((ref["dq"], qt.grad), (ref["dk"], kt.grad), (ref["dw"], wt.grad)):
        assert np.abs(got - want.numpy()).max() <= 1e-12 * np.abs(want.numpy()).max() and np.abs(got).max() > 0


@pytest.mark.parametrize("h", Q.HEADS)
def test_the_bounds_leave_room_for_the_designs_roundings_and_few_triples_are_ambiguous(h):
    """Gk and Gq rounded to bf16 as the kernel rounds them stay inside the bounds on the GPU bound test's inputs, of which fewer than 1 in
    10^4 (m, h, j) are ambiguous (expected: about 10^-6)"""
    ops, ref = B.random_case(h)
    got = B.reference(*ops, rounded=True)
    assert (np.abs(got["dq"] - ref["dq"]) <= ref["err_dq"]).all() and (np.abs(got["dk"] - ref["dk"]) <= B.bound_dk(ref, h)).all()
    assert ref["ambiguous"] < 1e-4 * B.M * h * ops[4].shape[1] and ref["count"].max() > 1 and (ref["count"] == 0).any()


def test_every_refusal_comes_from_the_wrapper(dga):
    z = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype)
    odd = lambda n, dtype: torch.zeros(n + 1, dtype=dtype)[1:]                           # a base 1 or 4 bytes off 16
    good = dict(q=z((2, 32, 128), torch.uint8), k=z((8, 128), torch.uint8), kscale=z(8), weights=z((2, 32)), indices=z((2, 4), torch.int32), d_logits=z((2, 4)))
    call = lambda **kw: (lambda a: dga.fp8_mqa_logits_bwd(a.pop("q"), (a.pop("k"), a.pop("kscale")), a.pop("weights"), a.pop("indices"), a.pop("d_logits"), **a))({**good, **kw})
    bad = {
        "q dtype": lambda: call(q=z((2, 32, 128))), "48 heads": lambda: call(q=z((2, 48, 128), torch.uint8)), "k width": lambda: call(k=z((8, 64), torch.uint8)),
        "kscale rows": lambda: call(kscale=z(7)), "weights shape": lambda: call(weights=z((2, 64))), "q misaligned": lambda: call(q=odd(2 * 32 * 128, torch.uint8).view(2, 32, 128)),
        "indices dtype": lambda: call(indices=z((2, 4), torch.int64)), "indices rows": lambda: call(indices=z((3, 4), torch.int32)), "topk 0": lambda: call(indices=z((2, 0), torch.int32)),
        "indices strided": lambda: call(indices=z((2, 8), torch.int32)[:, ::2]), "d_logits dtype": lambda: call(d_logits=z((2, 4), torch.float64)),
        "d_logits topk": lambda: call(d_logits=z((2, 5))), "d_logits strided": lambda: call(d_logits=z((2, 8))[:, ::2]), "offsets dtype": lambda: call(index_offsets=z(2)),
        "dq dtype": lambda: call(dq=z((2, 32, 128), torch.bfloat16)), "dq shape": lambda: call(dq=z((2, 32, 64))), "dq misaligned": lambda: call(dq=odd(2 * 32 * 128, torch.float32).view(2, 32, 128)),
        "d_weights shape": lambda: call(d_weights=z((2, 64))), "dk dtype": lambda: call(dk=z((8, 128), torch.bfloat16)), "dk rows": lambda: call(dk=z((7, 128))),
        "dk last dimension strided": lambda: call(dk=z((8, 256))[:, ::2]), "dk stride 130": lambda: call(dk=z((8, 130))[:, :128]), "dk misaligned": lambda: call(dk=odd(8 * 128, torch.float32).view(8, 128)),
    }
    wide = dict(indices=z((2, 9), torch.int32)[:, :4], d_logits=z((2, 6))[:, :4], index_offsets=z(2, torch.int32), dk=z((8, 160))[:, :128], dq=z((2, 32, 128)), d_weights=z((2, 32)))
    _refused(dga, bad, (call, lambda: call(**wide)))
