"""CPU: mla_fwd_dense's entry declared, exported and in the ctypes table, and the wrapper's refusals before a launch.  (Its cases, reference
and bounds are test_indexer_kl_dense.dense_case, sparse_mla_ref.reference / bound_out and test_indexer_kl_dense.bound_lse: the kernel's lse
is an online maximum with one rescale a tile over at most ceil(n / 32) + 1 tiles and a merge of four lane groups, which bound_lse's
derivation covers term by term -- it allows eight pairs in the merge -- so no term is added here.)"""
import ctypes

import torch

from deepgemm_ascend_amd import _lib
from sparse_mla_support import _args, _refused


def test_the_entry_is_exported(dga):
    assert hasattr(ctypes.CDLL(str(_lib.LIB_PATH)), "dga_mla_fwd_dense") and "dga_mla_fwd_dense" in _lib.SIGNATURES
    assert "mla_fwd_dense" in dga.__all__ and callable(dga.mla_fwd_dense)


def test_every_refusal_comes_from_the_wrapper(dga):
    q, kv, _ = _args()
    z = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype)
    good = dict(q=q, kv=kv, ks=z(2, torch.int32), ke=z(2, torch.int32))
    call = lambda **kw: (lambda a: dga.mla_fwd_dense(a.pop("q"), a.pop("kv"), a.pop("ks"), a.pop("ke"), a.pop("sm_scale", 0.1), **a))({**good, **kw})
    bad = {
        "ks dtype": lambda: call(ks=z(2, torch.int64)), "ke dtype": lambda: call(ke=z(2)), "ks rank": lambda: call(ks=z((2, 1), torch.int32)),
        "ke rank": lambda: call(ke=z((1, 2), torch.int32)), "ks length": lambda: call(ks=z(3, torch.int32)), "ke length": lambda: call(ke=z(1, torch.int32)),
        "Hq = 24": lambda: call(q=_args(h=24)[0]), "kv stride 580": lambda: call(kv=torch.zeros((8, 580), dtype=torch.bfloat16)[:, :576]),
        "sm_scale": lambda: call(sm_scale="1"), "out shape": lambda: call(out=z((2, 16, 576), torch.bfloat16)), "out dtype": lambda: call(out=z((2, 16, 512))),
        "lse shape": lambda: call(lse=z((2, 32))), "lse dtype": lambda: call(lse=z((2, 16), torch.bfloat16)), "d_v": lambda: call(d_v=576),
    }
    given = lambda: call(kv=torch.zeros((8, 1, 584), dtype=torch.bfloat16)[..., :576], out=z((2, 16, 512), torch.bfloat16), lse=z((2, 16)), _flags=1)
    _refused(dga, bad, (call, given))
