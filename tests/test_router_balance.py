"""CPU: the references tests/balance_ref.py holds are checked against torch.autograd on float64, the C entries' argument checks return their
codes before any launch, the Python entries refuse what they must, and the new unit compiles for gfx950 without spills or scratch."""
import ctypes
import re
import subprocess

import numpy as np
import pytest
import torch

import balance_ref as B
import router_ref as R
from test_build import CSRC, _ship_flags


@pytest.mark.parametrize("normalize", (True, False), ids=("normalize", "plain"))
@pytest.mark.parametrize("func", R.FUNCS)
def test_references_against_autograd(func, normalize):
    seq_len, e, k, alpha = 7, 24, 5, 0.75
    t_n = B.SEGMENTS * seq_len
    g = torch.Generator().manual_seed(4)
    x = torch.randn(t_n, e, generator=g, dtype=torch.float64).requires_grad_()
    dloss = torch.randn(B.SEGMENTS, generator=g, dtype=torch.float64)
    ids = torch.randint(-1, e + 1, (t_n, k), generator=g)
    s = torch.softmax(x, dim=1) if func == "softmax" else torch.sigmoid(x)
    counts = torch.zeros(B.SEGMENTS, e, dtype=torch.float64)
    for t in range(t_n):
        for i in ids[t].tolist():
            if 0 <= i < e:
                counts[t // seq_len, i] += 1
    p = s / s.sum(dim=1, keepdim=True) if normalize else s
    psum = p.view(B.SEGMENTS, seq_len, e).sum(dim=1)
    loss = alpha * e / (k * seq_len * seq_len) * (counts * psum).sum(dim=1)
    (loss * dloss).sum().backward()

    rl, rc, rp = B.forward_ref(s.detach().numpy(), ids.numpy(), seq_len, alpha, normalize)
    assert np.array_equal(rc, counts.numpy().astype(np.int64)) and rc.sum() < t_n * k          # some ids were outside [0, e)
    assert np.allclose(rp, psum.detach().numpy(), rtol=1e-12) and np.allclose(rl, loss.detach().numpy(), rtol=1e-12)
    ref, m = B.backward_ref(dloss.numpy(), rc, s.detach().numpy(), k, func, seq_len, alpha, normalize)
    assert np.allclose(ref, x.grad.numpy(), rtol=1e-11, atol=1e-14)
    assert (m >= np.abs(ref) * (1 - 1e-12)).all() and (m[ref != 0] > 0).all()


def test_the_bias_reference_and_the_shared_cases():
    counts = np.array([[3, 0, 2, 1], [1, 2, 2, 1]], np.int32)                       # n = 4, 2, 4, 2; the mean is 3
    bias = np.array([0.5, -0.25, 0.0, 1.0], np.float32)
    assert B.bias_update_ref(bias, counts, 0.125).tolist() == [0.375, -0.125, -0.125, 1.125]
    counts[0] = [3, 1, 2, 0]                                                        # n = 4, 3, 4, 1: expert 1 exactly at the mean
    assert B.bias_update_ref(bias, counts, 0.125).tolist() == [0.375, -0.25, -0.125, 1.125]
    assert B.chunk_tokens(150) == 16 and B.chunk_tokens(8192) == 16 and B.chunk_tokens(32768) == 64 and B.chunk_tokens(8193) == 20
    for e, k in R.EK:
        scores, ids = B.synthetic_case(e, k, 50)
        assert (ids == -1).any() and (ids == e).any() and ((scores > 0) & (scores < 1)).all()
        assert B.counts_ref(ids, e, 50).sum() == ((ids >= 0) & (ids < e)).sum()
    assert B.psum_bar(37, 60) < B.loss_bar(37, 60) < B.backward_bar(60) < 2.0 ** -15


def test_entries_check_their_arguments_before_any_launch(dga):
    """No GPU is needed: every refusal, and the empty call, returns before the first launch."""
    from deepgemm_ascend_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)
    OK, E_NULL, E_SHAPE, E_DTYPE, E_RANGE = 0, -1, -2, -3, -9
    NORM = _lib.ROUTER_BALANCE_NORMALIZE
    BIG = 1 << 40

    def fwd(tokens=4, e=8, k=2, seq_len=2, flags=NORM, scores=p, ids=p, loss=p, counts=p, psum=p, ws=p, ws_bytes=BIG):
        return L.dga_router_balance_loss(scores, ids, tokens, e, k, seq_len, flags, 1.0, loss, counts, psum, ws, ws_bytes, None)

    for bad in (dict(tokens=-1), dict(e=-1), dict(k=0), dict(k=9), dict(seq_len=0), dict(seq_len=-2), dict(seq_len=3),
                dict(seq_len=3, scores=None, e=2000, k=100, flags=6), dict(tokens=0, seq_len=0)):                        # the shape goes first
        assert fwd(**bad) == E_SHAPE, bad
    assert fwd(tokens=0, scores=None, ids=None, loss=None, counts=None, psum=None, ws=None, ws_bytes=0, e=4096, k=100, flags=6) == OK
    for name in ("scores", "ids", "loss", "counts", "psum", "ws"):
        assert fwd(**{name: None}, e=2000, flags=6, ws_bytes=0) == E_NULL, name
    need = L.dga_router_balance_loss_workspace_bytes(4, 8, 2)
    assert need == 8 * 2 * 1 * 8
    for bad in (dict(e=1025), dict(e=128, k=65), dict(flags=2), dict(flags=NORM | 4), dict(ws_bytes=need - 1), dict(ws_bytes=0),
                dict(ws=p + 2), dict(tokens=1 << 32, seq_len=1, ws_bytes=1 << 62)):
        assert fwd(**bad) == E_RANGE, bad
    # the size query: 8 B chunks e, chunks of max(16, 4 ceil(tokens / 2048)) tokens; 0 for what the entry refuses
    wsb = L.dga_router_balance_loss_workspace_bytes
    assert wsb(150, 60, 50) == 8 * 3 * 4 * 60 and wsb(32768, 256, 32768) == 8 * 512 * 256 and wsb(32768, 256, 4096) == 8 * 8 * 64 * 256
    assert wsb(0, 8, 1) == 0 and wsb(4, 0, 2) == 0 and wsb(4, 8, 3) == 0 and wsb(4, 8, 0) == 0 and wsb(4, 1025, 2) == 0 and wsb(-4, 8, 2) == 0

    SOFTMAX, SIGMOID = _lib.ROUTER_SOFTMAX, _lib.ROUTER_SIGMOID

    def bwd(tokens=4, e=8, k=2, seq_len=2, func=SIGMOID, flags=0, dtype=_lib.DT_FP32, dloss=p, counts=p, scores=p, add_to=None, dlogits=p):
        return L.dga_router_balance_loss_backward(dloss, counts, scores, tokens, e, k, seq_len, func, flags, 1.0, add_to, dlogits, dtype, None)

    for bad in (dict(tokens=-1), dict(e=-1), dict(k=0), dict(k=9), dict(seq_len=0), dict(seq_len=3), dict(seq_len=3, dloss=None, dtype=99, e=2000, k=9)):
        assert bwd(**bad) == E_SHAPE, bad
    assert bwd(tokens=0, dloss=None, counts=None, scores=None, dlogits=None, dtype=99, e=4096, k=100, func=7) == OK
    for name in ("dloss", "counts", "scores", "dlogits"):
        assert bwd(**{name: None}, dtype=99, e=2000) == E_NULL, name
    assert bwd(dtype=99, e=2000) == E_DTYPE and bwd(dtype=_lib.DT_FP8_E4M3FN) == E_DTYPE
    for bad in (dict(e=1025), dict(e=128, k=65), dict(func=2), dict(func=-1), dict(flags=2), dict(tokens=4 * 0x7FFFFFFF + 2)):
        assert bwd(**bad) == E_RANGE, bad
    assert SOFTMAX == 0

    def upd(segments=2, e=8, bias=p, counts=p):
        return L.dga_router_bias_update(bias, counts, segments, e, 0.5, None)

    assert upd(segments=-1) == E_SHAPE and upd(e=-1, bias=None) == E_SHAPE
    assert upd(segments=0, bias=None, counts=None, e=4096) == OK and upd(e=0, bias=None, counts=None) == OK
    assert upd(bias=None, e=4096) == E_NULL and upd(counts=None, e=4096) == E_NULL
    assert upd(e=1025) == E_RANGE


def test_python_entries_refuse_what_the_c_entries_would(dga):
    s, ids = torch.zeros(6, 8), torch.zeros(6, 2, dtype=torch.int32)
    dloss, counts = torch.zeros(3), torch.zeros(3, 8, dtype=torch.int32)
    E = dga.DGAError
    for bad in (lambda: dga.router_balance_loss(s.double(), ids), lambda: dga.router_balance_loss(s, ids.long()),
                lambda: dga.router_balance_loss(s, ids[:4]), lambda: dga.router_balance_loss(s[:, :4], ids),          # not contiguous
                lambda: dga.router_balance_loss(s, ids, seq_len=4), lambda: dga.router_balance_loss(s, ids, seq_len=0),
                lambda: dga.router_balance_loss(s, ids, seq_len=2, out=(torch.zeros(3), torch.zeros(2, 8, dtype=torch.int32), torch.zeros(3, 8))),
                lambda: dga.router_balance_loss(s, ids, seq_len=2, out=(torch.zeros(3), torch.zeros(3, 8), torch.zeros(3, 8))),
                lambda: dga.router_balance_loss(s, ids, seq_len=2),                                                    # host tensors: no CPU path
                lambda: dga.router_balance_loss_backward(dloss, counts, s, 2, "tanh", seq_len=2),
                lambda: dga.router_balance_loss_backward(dloss.double(), counts, s, 2, "sigmoid", seq_len=2),
                lambda: dga.router_balance_loss_backward(dloss, counts.long(), s, 2, "sigmoid", seq_len=2),
                lambda: dga.router_balance_loss_backward(dloss, counts, s, 2, "sigmoid", seq_len=4),
                lambda: dga.router_balance_loss_backward(dloss[:2], counts, s, 2, "sigmoid", seq_len=2),
                lambda: dga.router_balance_loss_backward(dloss, counts, s, 2, "sigmoid", seq_len=2, add_to=torch.zeros(6, 8, dtype=torch.bfloat16)),
                lambda: dga.router_balance_loss_backward(dloss, counts, s, 2, "sigmoid", seq_len=2, out=torch.zeros(6, 8, dtype=torch.float64)),
                lambda: dga.router_balance_loss_backward(dloss, counts, s, 2, "sigmoid", seq_len=2),                   # host tensors
                lambda: dga.router_bias_update(torch.zeros(8, dtype=torch.float64), counts, 0.1),
                lambda: dga.router_bias_update(torch.zeros(7), counts, 0.1),
                lambda: dga.router_bias_update(torch.zeros(8), counts.float(), 0.1),
                lambda: dga.router_bias_update(torch.zeros(8), counts, 0.1)):                                          # host tensors
        with pytest.raises(E):
            bad()
    assert dga.router_balance_loss_workspace_bytes(150, 60, 50) == 8 * 3 * 4 * 60
    assert dga.router_balance_loss_workspace_bytes(4096, 256) == 8 * 256 * 256


def test_the_balance_unit_compiles_without_spills_or_scratch():
    """tests/test_build.py's method on csrc/dga_router_balance.hip with the flags the Makefile ships it with: 5 stage-one builds (one per
    lane width), stage two, 15 backward builds (3 output types x 5) and the bias update, none with a spilled register or a byte of
    scratch.  LDS is what the kernels declare: stage one's four waves meet in 4 x 64 V floats and as many integers, stage two keeps a
    float and an integer per thread and a float per wave, the bias update a 64-bit integer per thread; the backward uses none."""
    unit = "dga_router_balance.hip"
    flags = _ship_flags(unit)
    assert "--offload-arch=gfx950" in flags and "-O3" in flags
    cmd = ["/opt/rocm/bin/hipcc", *flags, "--cuda-device-only", "-S", "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage", str(CSRC / unit)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=str(CSRC))
    assert r.returncode == 0, r.stderr[-2000:]
    name, seen, lds = None, {}, {}
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"(VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]): (\d+)", line)
        if m:
            assert int(m.group(2)) == 0, f"{name}: {m.group(1)} = {m.group(2)}"
            seen[m.group(1)] = seen.get(m.group(1), 0) + 1
        m = re.search(r"LDS Size \[bytes/block\]: (\d+)", line)
        if m:
            lds[name] = int(m.group(1))
    assert len(seen) == 3 and all(n == 22 for n in seen.values()), seen
    want = {}
    for n in lds:
        v = re.search(r"balance_partial_kernelILi(\d+)E", n)
        want[n] = 2 * 4 * 64 * int(v.group(1)) * 4 if v else 1024 * 8 + 16 * 4 if "balance_finish_kernel" in n else 1024 * 8 if "bias_update_kernel" in n else 0
    assert lds == want and len(lds) == 22, (lds, want)
    assert sum("balance_partial_kernel" in n for n in lds) == 5 and sum("balance_backward_kernel" in n for n in lds) == 15
