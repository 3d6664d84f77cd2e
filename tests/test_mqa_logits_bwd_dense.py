"""CPU: fp8_mqa_logits_bwd_dense's refusals before the device guard, and the size of its scratch."""
import torch

from sparse_mla_support import _refused


def test_every_refusal_comes_from_the_wrapper(dga):
    z = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype)
    odd = lambda n, dtype: torch.zeros(n + 1, dtype=dtype)[1:]                           # a base 1 or 4 bytes off 16
    good = dict(q=z((2, 32, 128), torch.uint8), k=z((8, 128), torch.uint8), kscale=z(8), weights=z((2, 32)), d_logits=z((2, 8)), ks=z(2, torch.int32), ke=z(2, torch.int32))
    call = lambda **kw: (lambda a: dga.fp8_mqa_logits_bwd_dense(a.pop("q"), (a.pop("k"), a.pop("kscale")), a.pop("weights"), a.pop("d_logits"), a.pop("ks"), a.pop("ke"), **a))({**good, **kw})
    bad = {
        "q dtype": lambda: call(q=z((2, 32, 128))), "48 heads": lambda: call(q=z((2, 48, 128), torch.uint8)), "k width": lambda: call(k=z((8, 64), torch.uint8)),
        "kscale rows": lambda: call(kscale=z(7)), "weights shape": lambda: call(weights=z((2, 64))), "q misaligned": lambda: call(q=odd(2 * 32 * 128, torch.uint8).view(2, 32, 128)),
        "ks dtype": lambda: call(ks=z(2, torch.int64)), "ke rows": lambda: call(ke=z(3, torch.int32)), "d_logits dtype": lambda: call(d_logits=z((2, 8), torch.float64)),
        "d_logits columns": lambda: call(d_logits=z((2, 7))), "d_logits rows": lambda: call(d_logits=z((3, 8))), "d_logits strided": lambda: call(d_logits=z((2, 16))[:, ::2]),
        "dq dtype": lambda: call(dq=z((2, 32, 128), torch.bfloat16)), "dq shape": lambda: call(dq=z((2, 32, 64))), "dq misaligned": lambda: call(dq=odd(2 * 32 * 128, torch.float32).view(2, 32, 128)),
        "d_weights shape": lambda: call(d_weights=z((2, 64))), "dk dtype": lambda: call(dk=z((8, 128), torch.bfloat16)), "dk rows": lambda: call(dk=z((7, 128))),
        "dk last dimension strided": lambda: call(dk=z((8, 256))[:, ::2]), "dk stride 130": lambda: call(dk=z((8, 130))[:, :128]), "dk misaligned": lambda: call(dk=odd(8 * 128, torch.float32).view(8, 128)),
    }
    wide = dict(d_logits=z((2, 11))[:, 1:9], dk=z((8, 160))[:, :128], dq=z((2, 32, 128)), d_weights=z((2, 32)))
    _refused(dga, bad, (call, lambda: call(**wide)))


def test_scratch_is_a_function_of_the_shape_alone(dga):
    """splits x padded keys x (a row of fp32 partials + a flag): two runs of 64 tokens over five key tiles; one chunk once the key tiles
    alone fill the grid; nothing for an empty call"""
    ws = dga.lib().dga_fp8_mqa_logits_bwd_dense_workspace_bytes
    assert ws(70, 300) == 2 * 320 * 516 and ws(64, 300) == 320 * 516 and ws(4096, 8192) == 16 * 8192 * 516
    assert ws(4096, 64 * 4096) == 64 * 4096 * 516 and ws(0, 300) == 0
