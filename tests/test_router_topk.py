"""CPU: the references tests/router_ref.py holds are checked against independent ones -- the numpy selection against a brute-force sort, the
float64 backward against torch.autograd --, the C entries' argument checks return their codes before any launch, and the new unit compiles
for gfx950 without spills or scratch."""
import ctypes
import math
import re
import subprocess

import numpy as np
import pytest
import torch

import router_ref as R
from test_build import CSRC, _ship_flags

F32 = np.float32
NINF = float("-inf")


def _brute(row, k, bias, n_groups, topk_groups, renormalize, scale):
    """One row, element by element: python sorts on (-value, index), float32 scalars for the arithmetic."""
    e = len(row)
    sel = [F32(row[i]) + F32(bias[i]) if bias is not None else F32(row[i]) for i in range(e)]
    sel = [F32(NINF) if math.isnan(v) else v for v in sel]
    allowed = list(range(e))
    if n_groups > 1:
        gs = e // n_groups
        gv = []
        for g in range(n_groups):
            top = sorted((float(v) for v in sel[g * gs:(g + 1) * gs]), reverse=True)
            with np.errstate(invalid="ignore"):
                v = F32(top[0]) + F32(top[1])
            gv.append(NINF if math.isnan(v) else float(v))
        kept = sorted(range(n_groups), key=lambda g: (-gv[g], g))[:topk_groups]
        allowed = [i for i in range(e) if i // gs in kept]
    ids = sorted(allowed, key=lambda i: (-float(sel[i]), i))[:k]
    r = [F32(row[i]) for i in ids]
    if not renormalize:
        return ids, [v * F32(scale) for v in r]
    d = r[0]
    for v in r[1:]:
        d = F32(d + v)
    with np.errstate(invalid="ignore", divide="ignore"):
        return ids, [F32(F32(v / d) * F32(scale)) for v in r]


def _same(scores, k, bias=None, n_groups=1, topk_groups=1, renormalize=True, scale=1.0):
    ids, w = R.select_ref(scores, k, bias, n_groups, topk_groups, renormalize, scale)
    for t in range(scores.shape[0]):
        bi, bw = _brute(scores[t], k, bias, n_groups, topk_groups, renormalize, scale)
        assert ids[t].tolist() == bi, (t, ids[t], bi)
        assert np.array_equal(w[t].view(np.uint32), np.array(bw, F32).view(np.uint32), ), (t, w[t], bw)
        assert len(set(bi)) == k and all(0 <= i < scores.shape[1] for i in bi)


def test_selection_reference_on_hand_made_rows():
    nan, z, nz = float("nan"), 0.0, -0.0
    rows = np.array([[z, z, z, z, z, z, z, z],                      # all equal: 0 .. k-1
                     [nz, z, nz, z, 1.0, 1.0, nz, z],               # -0 ties +0, two equal maxima
                     [nan, 0.5, nan, 0.5, 0.25, nan, 0.25, 0.5],    # NaN counts as -inf, below every number
                     [NINF, NINF, NINF, NINF, NINF, NINF, NINF, NINF],
                     [nan, nan, nan, nan, nan, nan, nan, nan],
                     [0.125, 0.5, 0.5, 0.125, 0.75, 0.0, 0.75, 0.125]], F32)
    for k in (1, 3, 8):
        for renorm in (True, False):
            _same(rows, k, renormalize=renorm, scale=2.5)
    ids, _ = R.select_ref(rows, 3)
    assert ids[0].tolist() == [0, 1, 2] and ids[1].tolist() == [4, 5, 0] and ids[2].tolist() == [1, 3, 7] and ids[4].tolist() == [0, 1, 2]
    bias = np.array([0.0, -0.0, 0.25, 0.25, -1.0, 0.0, nan, 0.5], F32)
    for k in (2, 8):
        _same(rows, k, bias=bias)
    for n_groups, topk_groups, k in ((4, 2, 4), (4, 1, 2), (2, 1, 4), (2, 2, 8), (4, 3, 5)):
        _same(rows, k, bias=bias, n_groups=n_groups, topk_groups=topk_groups)
        _same(rows, k, n_groups=n_groups, topk_groups=topk_groups, renormalize=False)
    # groups: [z z | z z | ...] all equal -> the lower groups stay; the experts of the others never appear
    ids, _ = R.select_ref(rows[:1], 4, n_groups=4, topk_groups=2)
    assert ids[0].tolist() == [0, 1, 2, 3]
    ids, _ = R.select_ref(rows[5:], 2, n_groups=4, topk_groups=1)     # group values 0.625, 0.625, 0.75, 0.875 -> group 3
    assert ids[0].tolist() == [6, 7]


@pytest.mark.parametrize("e,k,n_groups,topk_groups", [(12, 5, 1, 1), (12, 12, 1, 1), (12, 4, 3, 2), (12, 4, 6, 2), (30, 7, 5, 3), (16, 8, 4, 2)])
def test_selection_reference_on_random_rows_full_of_ties(e, k, n_groups, topk_groups):
    rng = np.random.default_rng([e, k, n_groups])
    values = np.array([-0.0, 0.0, 0.25, 0.5, 0.5, 1.0, float("nan"), NINF], F32)
    scores = values[rng.integers(0, len(values), size=(40, e))]
    bias = np.array([0.0, 0.25, -0.25], F32)[rng.integers(0, 3, size=e)]
    _same(scores, k, None, n_groups, topk_groups)
    _same(scores, k, bias, n_groups, topk_groups, scale=2.5)
    _same(scores, k, bias, n_groups, topk_groups, renormalize=False)


@pytest.mark.parametrize("func", R.FUNCS)
@pytest.mark.parametrize("renormalize", (True, False))
def test_backward_reference_against_autograd(func, renormalize):
    t_n, e, k, scale = 9, 24, 5, 2.5
    g = torch.Generator().manual_seed(3)
    x = torch.randn(t_n, e, generator=g, dtype=torch.float64).requires_grad_()
    dw = torch.randn(t_n, k, generator=g, dtype=torch.float64)
    ids = torch.stack([torch.randperm(e, generator=g)[:k] for _ in range(t_n)])
    s = torch.softmax(x, dim=1) if func == "softmax" else torch.sigmoid(x)
    r = s.gather(1, ids)
    w = scale * r / r.sum(dim=1, keepdim=True) if renormalize else scale * r
    (w * dw).sum().backward()
    ref, m = R.backward_ref(dw.numpy(), s.detach().numpy(), ids.numpy(), func, renormalize, scale)
    assert np.allclose(ref, x.grad.numpy(), rtol=1e-11, atol=1e-14)
    assert (m >= np.abs(ref) * (1 - 1e-12)).all() and (m[ref != 0] > 0).all()
    if func == "sigmoid":
        off = np.ones((t_n, e), bool)
        off[np.arange(t_n)[:, None], ids.numpy()] = False
        assert not ref[off].any() and not m[off].any()


def test_the_score_references():
    x = R.tie_logits(60, 6, "bf16")
    p = R.scores64(x, "softmax")
    keep = np.ones(R.T, bool)
    keep[R.ROW_NAN] = False
    assert np.allclose(p[keep].sum(axis=1), 1.0) and (p[R.ROW_NEG_INF][np.isinf(x[R.ROW_NEG_INF])] == 0).all()
    assert np.allclose(p[R.ROW_ZEROS], 1 / 60) and np.isnan(p[R.ROW_NAN]).all()
    assert np.allclose(R.scores64(x, "sigmoid")[keep], torch.sigmoid(torch.from_numpy(x[keep]).double()).numpy())
    assert not R.score_checked(x, "softmax")[np.isinf(x)].any() and R.score_checked(x, "softmax")[R.ROW_ZEROS].all()
    for e, k in R.EK:                                  # the shared cases hold what they promise
        x = R.tie_logits(e, k, "fp16")
        for row in (R.ROW_NEG_INF, R.ROW_NEG_INF2):
            assert np.isfinite(x[row]).sum() >= min(k, e - 1) and (e < 60 or np.isinf(x[row]).any())
        assert (x[R.ROW_TWO_MAXIMA] == x[R.ROW_TWO_MAXIMA].max()).sum() == 2 and np.isnan(x[R.ROW_NAN]).sum() == 1
        assert np.array_equal(R.to_dtype(x, "fp16")[~np.isnan(x)], x[~np.isnan(x)])


def test_entries_check_their_arguments_before_any_launch(dga):
    """No GPU is needed: every refusal, and the empty call, returns before the first launch."""
    from deepgemm_ascend_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)
    OK, E_NULL, E_SHAPE, E_DTYPE, E_RANGE = 0, -1, -2, -3, -9
    SOFTMAX, SIGMOID, RENORM = _lib.ROUTER_SOFTMAX, _lib.ROUTER_SIGMOID, _lib.ROUTER_RENORMALIZE

    def fwd(tokens=4, e=8, k=2, dtype=_lib.DT_BF16, func=SOFTMAX, n_groups=1, topk_groups=1, flags=RENORM, logits=p, ids=p, weights=p, scores=p):
        return L.dga_router_topk(logits, dtype, tokens, e, k, func, None, n_groups, topk_groups, flags, 1.0, ids, weights, scores, None)

    for bad in (dict(tokens=-1), dict(e=-1), dict(k=0), dict(k=9), dict(e=0, k=0), dict(n_groups=0), dict(n_groups=3), dict(topk_groups=0),
                dict(n_groups=2, topk_groups=3), dict(n_groups=4, topk_groups=1, k=3), dict(n_groups=8, topk_groups=8, k=2),
                dict(k=0, logits=None), dict(k=0, dtype=99, e=2000)):                       # the shape goes first
        assert fwd(**bad) == E_SHAPE, bad
    assert fwd(tokens=0, logits=None, ids=None, weights=None, scores=None, dtype=99, e=4096, k=100, func=7) == OK    # nothing to do
    for name in ("logits", "ids", "weights", "scores"):
        assert fwd(**{name: None}, dtype=99, e=2000) == E_NULL, name
    assert fwd(dtype=99, e=2000) == E_DTYPE and fwd(dtype=_lib.DT_FP8_E4M3FN) == E_DTYPE
    for bad in (dict(e=1025), dict(e=2048, k=8, n_groups=8, topk_groups=4), dict(e=128, k=65), dict(func=2), dict(func=-1), dict(flags=2),
                dict(flags=RENORM | 4), dict(tokens=4 * 0x7FFFFFFF + 1)):
        assert fwd(**bad) == E_RANGE, bad

    def bwd(tokens=4, e=8, k=2, dtype=_lib.DT_FP32, func=SIGMOID, flags=0, dw=p, scores=p, ids=p, dlogits=p):
        return L.dga_router_topk_backward(dw, scores, ids, tokens, e, k, func, flags, 1.0, dlogits, dtype, None)

    for bad in (dict(tokens=-1), dict(e=-1), dict(k=0), dict(k=9), dict(k=9, dw=None, dtype=99)):
        assert bwd(**bad) == E_SHAPE, bad
    assert bwd(tokens=0, dw=None, scores=None, ids=None, dlogits=None, dtype=99, e=4096, k=100) == OK
    for name in ("dw", "scores", "ids", "dlogits"):
        assert bwd(**{name: None}, dtype=99, e=2000) == E_NULL, name
    assert bwd(dtype=99, e=2000) == E_DTYPE
    for bad in (dict(e=1025), dict(e=128, k=65), dict(func=2), dict(flags=2), dict(tokens=4 * 0x7FFFFFFF + 1)):
        assert bwd(**bad) == E_RANGE, bad


def test_python_entries_refuse_what_the_c_entries_would(dga):
    x = torch.zeros(4, 8)
    with pytest.raises(dga.DGAError):
        dga.router_topk(x, 2, score_func="tanh")
    with pytest.raises(dga.DGAError):
        dga.router_topk(x.double(), 2)
    with pytest.raises(dga.DGAError):
        dga.router_topk(x, 2, bias=torch.zeros(7))
    with pytest.raises(dga.DGAError):
        dga.router_topk(x, 2, out=(torch.zeros(4, 2, dtype=torch.int64), torch.zeros(4, 2), torch.zeros(4, 8)))
    with pytest.raises(dga.DGAError):                                      # host tensors: there is no CPU path
        dga.router_topk(x, 2)
    with pytest.raises(dga.DGAError):
        dga.router_topk_backward(torch.zeros(4, 2), torch.zeros(4, 8), torch.zeros(4, 2, dtype=torch.int32), "sigmoid")
    with pytest.raises(dga.DGAError):
        dga.router_topk_backward(torch.zeros(4, 3), torch.zeros(4, 8), torch.zeros(4, 2, dtype=torch.int32), "softmax")


def test_the_router_unit_compiles_without_spills_or_scratch():
    """tests/test_build.py's method on csrc/dga_router.hip with the flags the Makefile ships it with: 15 forward builds (3 input types x 5
    lane widths) and 15 backward builds (3 output types x 5), none with a spilled register, a byte of scratch or a byte of LDS (an array the
    compiler takes for indexed at run time would be moved there)."""
    unit = "dga_router.hip"
    flags = _ship_flags(unit)
    assert "--offload-arch=gfx950" in flags and "-O3" in flags
    cmd = ["/opt/rocm/bin/hipcc", *flags, "--cuda-device-only", "-S", "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage", str(CSRC / unit)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=str(CSRC))
    assert r.returncode == 0, r.stderr[-2000:]
    names, name, checked = [], None, {}
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            names.append(name)
        m = re.search(r"(VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m:
            assert int(m.group(2)) == 0, f"{name}: {m.group(1)} = {m.group(2)}"
            checked[m.group(1)] = checked.get(m.group(1), 0) + 1
    assert len(checked) == 4 and all(n == 30 for n in checked.values()), checked
    assert sum("router_topk_kernel" in n for n in names) == 15 and sum("router_topk_backward_kernel" in n for n in names) == 15, names
