"""CPU: the norm's entries are exported through every layer, the references tests/rms_norm_ref.py holds match torch.autograd on float64, the
C entries' argument checks return their codes before any launch, the Python entries refuse what they must, and the new unit compiles for
gfx950 without spills or scratch."""
import ctypes
import re
import subprocess

import numpy as np
import pytest
import torch

import rms_norm_ref as N
from test_build import CSRC, ROOT, _ship_flags

C_ENTRIES = ("dga_rms_norm_cast_to_fp8_1x128", "dga_rms_norm_backward", "dga_rms_norm_backward_workspace_bytes")
PY_ENTRIES = ("rms_norm_per_token_cast_to_fp8", "rms_norm_backward", "rms_norm_backward_workspace_bytes")


def test_the_entries_are_exported_through_every_layer(dga):
    from deepgemm_ascend_amd import _lib
    header = (ROOT / "include" / "dga_hip.h").read_text()
    L = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in C_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
    for name in PY_ENTRIES:
        assert name in dga.__all__ and callable(getattr(dga, name)), name
    assert "#define DGA_ABI_VERSION 7\n" in header and L.dga_abi_version() == 7
    assert "#define DGA_RMS_NORM_MAX_H %d\n" % N.MAX_H in header
    makefile = (CSRC / "Makefile").read_text()
    assert re.search(r"^SRCS = .*\bdga_rms_norm\.hip\b", makefile, flags=re.M)
    assert re.search(r"^\$\(OBJ\)/dga_cast\.o .*\$\(OBJ\)/dga_rms_norm\.o.*: dga_cast_device\.hpp$", makefile, flags=re.M)


def test_the_shared_cases_meet_every_value():
    assert 55 <= len(N.FORWARD_CASES) <= 65
    for column, values in enumerate((N.HS, N.TS, N.DTYPES, (False, True), (False, True), (False, True))):
        assert {c[column] for c in N.FORWARD_CASES} == set(values), column
    for table in (N.FORWARD_GEOMETRY, N.BACKWARD_GEOMETRY):                  # every geometry of both kernels is met by some case
        hs = N.HS if table is N.FORWARD_GEOMETRY else {h for _, h in N.BACKWARD_TH}
        assert {N.geometry(table, h) for h in hs} == {g for _, g in table}
    assert N.chunk_rows(300) == 8 and N.chunk_rows(8192) == 8 and N.chunk_rows(32768) == 32 and N.chunk_rows(8193) == 9
    assert {(t, h) for t in (1, 5, 300) for h in (7, 136, 2048, 7168)} <= set(N.BACKWARD_TH)


@pytest.mark.parametrize("with_residual", (False, True), ids=("plain", "residual"))
def test_references_against_autograd(with_residual):
    t_n, h, eps = 6, 37, 1e-3
    g = torch.Generator().manual_seed(5)
    x = torch.randn(t_n, h, generator=g, dtype=torch.float64).requires_grad_()
    res = torch.randn(t_n, h, generator=g, dtype=torch.float64).requires_grad_() if with_residual else None
    w = (1 + 0.3 * torch.randn(h, generator=g, dtype=torch.float64)).requires_grad_()
    gy = torch.randn(t_n, h, generator=g, dtype=torch.float64)
    z = x + res if with_residual else x
    y = torch.nn.functional.rms_norm(z, (h,), w, eps)
    (y * gy).sum().backward()

    xn, wn = x.detach().numpy(), w.detach().numpy()
    zn = z.detach().numpy()
    assert np.allclose(N.forward64(xn, res.detach().numpy() if with_residual else None, wn, eps), y.detach().numpy(), rtol=1e-13, atol=0)
    rstd = 1.0 / np.sqrt((zn * zn).mean(axis=1) + eps)
    assert np.allclose(N.rstd64(zn.astype(np.float32), eps), rstd, rtol=1e-6)           # (on the float32 z, with fl32(eps))
    dx, dw, m = N.backward64(gy.numpy(), zn, wn, rstd)
    assert np.allclose(dx, x.grad.numpy(), rtol=1e-11, atol=1e-14) and np.allclose(dw, w.grad.numpy(), rtol=1e-12, atol=1e-14)
    if with_residual:
        assert np.array_equal(res.grad.numpy(), x.grad.numpy())                         # the residual stream gets the same dx
    assert (N.dx_bar(m, h) > 0).all() and (N.dweight_bar(m, t_n) > 0).all()
    assert (m["dw_abs"] >= np.abs(dw)).all() and (m["a"] >= m["c"]).all()


def test_the_float32_references_follow_the_definition():
    x, res, w = N.forward_inputs(136, 3, "bf16", False)
    bits, z = N.residual_ref(x, res, "bf16")
    assert bits.dtype == np.uint16 and np.array_equal(N.to_dtype(x + res, "bf16"), z)
    rstd = N.rstd64(z, N.EPS).astype(np.float32)
    rstd[1] = np.nan
    y = N.y_ref(z, rstd, w)
    assert (y.view(np.uint32)[1] == N.CANONICAL_NAN).all() and np.isfinite(y[[0, 2]]).all()
    assert np.array_equal(y[0], (z[0] * rstd[0]).astype(np.float32) * w)
    assert (N.norm_bits(y, "bf16")[1] == 0x7FC0).all() and (N.norm_bits(y, "fp16")[1] == 0x7E00).all()
    assert N.rstd64(np.zeros((1, 8), np.float32), 1e-6)[0] == 1.0 / np.sqrt(np.float64(np.float32(1e-6)))


def test_entries_check_their_arguments_before_any_launch(dga):
    """No GPU is needed: every refusal, and the empty call, returns before the first launch."""
    from deepgemm_ascend_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_char * 128)()
    p = (ctypes.addressof(buf) + 15) & ~15                                                                              # 16-byte aligned
    OK, E_NULL, E_SHAPE, E_DTYPE, E_WORKSPACE, E_RANGE = 0, -1, -2, -3, -7, -9
    F32, BF16, F16, FP8 = _lib.DT_FP32, _lib.DT_BF16, _lib.DT_FP16, _lib.DT_FP8_E4M3FN

    def fwd(rows=4, h=8, eps=1e-6, flags=0, dt=BF16, wdt=BF16, x=p, res=None, w=p, q=p, sf=p, norm=None, res_out=None, rstd=p):
        return L.dga_rms_norm_cast_to_fp8_1x128(x, res, dt, w, wdt, rows, h, eps, q, sf, norm, res_out, rstd, flags, None)

    for bad in (dict(flags=2), dict(flags=-1), dict(flags=3, rows=-1, x=None)):                                        # the flags go first
        assert fwd(**bad) == E_RANGE, bad
    for bad in (dict(rows=-1), dict(h=-1), dict(h=N.MAX_H + 1), dict(h=1 << 40), dict(rows=-1, x=None, dt=99, eps=-1.0)):   # then the shape
        assert fwd(**bad) == E_SHAPE, bad
    assert fwd(rows=0, x=None, w=None, q=None, sf=None, rstd=None, dt=99, eps=-1.0) == OK
    assert fwd(h=0, x=None, w=None, q=None, sf=None, rstd=None, dt=99, eps=-1.0) == OK
    for bad in (dict(x=None), dict(w=None), dict(rstd=None), dict(sf=None), dict(q=None), dict(q=None, norm=p),          # q without sf, sf without q
                dict(q=None, sf=None), dict(res=p), dict(res_out=p), dict(q=None, sf=None, norm=p, res=p)):             # neither; residual and its output
        assert fwd(**bad, dt=99, eps=-1.0) == E_NULL, bad
    assert fwd(q=None, sf=None, norm=p, dt=99) == E_DTYPE                                                               # (norm_out alone is a valid set)
    for bad in (dict(dt=99), dict(dt=FP8), dict(dt=0), dict(wdt=F16), dict(dt=F32, wdt=BF16), dict(wdt=FP8), dict(dt=99, eps=-1.0)):
        assert fwd(**bad) == E_DTYPE, bad
    for bad in (dict(eps=-1e-6), dict(eps=float("inf")), dict(eps=float("nan")), dict(rows=1 << 40, h=N.MAX_H)):
        assert fwd(**bad) == E_RANGE, bad

    wsb = L.dga_rms_norm_backward_workspace_bytes
    assert wsb(300, 7168) == 4 * 38 * 7168 and wsb(1, 7) == 4 * 7 and wsb(32768, 2048) == 4 * 1024 * 2048 and wsb(8193, 8) == 4 * 911 * 8
    assert wsb(0, 8) == 0 and wsb(4, 0) == 0 and wsb(-4, 8) == 0 and wsb(4, -8) == 0 and wsb(4, N.MAX_H + 1) == 0
    BIG = 1 << 40

    def bwd(rows=4, h=8, dt=BF16, wdt=BF16, dxdt=BF16, gy=p, z=p, w=p, rstd=p, gr=None, dx=p, dweight=p, ws=p, ws_bytes=BIG):
        return L.dga_rms_norm_backward(gy, z, dt, w, wdt, rstd, gr, rows, h, dx, dxdt, dweight, ws, ws_bytes, None)

    for bad in (dict(rows=-1), dict(h=-1), dict(h=N.MAX_H + 1), dict(rows=-1, gy=None, dt=99)):
        assert bwd(**bad) == E_SHAPE, bad
    assert bwd(rows=0, gy=None, z=None, w=None, rstd=None, dx=None, dweight=None, ws=None, ws_bytes=0, dt=99) == OK
    assert bwd(h=0, gy=None, z=None, w=None, rstd=None, dx=None, dt=99) == OK
    for name in ("gy", "z", "w", "rstd", "dx", "ws"):
        assert bwd(**{name: None}, dt=99) == E_NULL, name
    assert bwd(dweight=None, ws=None, ws_bytes=0, dt=99) == E_DTYPE                                                     # (no dweight: no workspace)
    for bad in (dict(dt=99), dict(dt=FP8), dict(wdt=F16), dict(dxdt=F16), dict(dt=F32, dxdt=BF16), dict(dt=F32, wdt=F16, dxdt=F32)):
        assert bwd(**bad) == E_DTYPE, bad
    assert bwd(rows=1 << 40) == E_RANGE
    need = wsb(4, 8)
    assert need == 4 * 8
    for bad in (dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(ws_bytes=-1), dict(ws=p + 4)):                          # short, or not 16-byte aligned
        assert bwd(**bad) == E_WORKSPACE, bad


def test_python_entries_refuse_what_they_must(dga):
    x, w = torch.zeros(6, 16, dtype=torch.bfloat16), torch.ones(16, dtype=torch.bfloat16)
    rstd = torch.ones(6)
    E = dga.DGAError
    fwd, bwd = dga.rms_norm_per_token_cast_to_fp8, dga.rms_norm_backward
    for bad in (lambda: fwd(x.double(), w), lambda: fwd(x[:, :8], w[:8]), lambda: fwd(x[0], w), lambda: fwd(x.t().contiguous().t(), w),
                lambda: fwd(x, w.half()), lambda: fwd(x, w[:8]), lambda: fwd(x, torch.ones(32)[::2]), lambda: fwd(x.float(), w),
                lambda: fwd(torch.zeros(2, N.MAX_H + 8), torch.ones(N.MAX_H + 8)), lambda: fwd(torch.zeros(2, 0), torch.ones(0)),
                lambda: fwd(x, w, eps=-1e-6), lambda: fwd(x, w, eps=float("inf")), lambda: fwd(x, w, eps=float("nan")),
                lambda: fwd(x, w, residual=x.float()), lambda: fwd(x, w, residual=x[:4]),
                lambda: fwd(x, w, quantize=False), lambda: fwd(x, w, out=(x, x)), lambda: fwd(x, w, out={"y": x}),
                lambda: fwd(x, w, out={"norm": x}), lambda: fwd(x, w, out={"residual": x}),                                # given but not asked for
                lambda: fwd(x, w, out={"q": torch.zeros(6, 16)}), lambda: fwd(x, w, out={"sf": torch.zeros(6, 2)}),
                lambda: fwd(x, w, norm_out=True, out={"norm": x.float()}), lambda: fwd(x, w, out={"rstd": torch.zeros(5)}),
                lambda: fwd(x, w),                                                                                         # host tensors: no CPU path
                lambda: bwd(x, x.float(), w, rstd), lambda: bwd(x[:4], x, w, rstd), lambda: bwd(x, x, w.half(), rstd),
                lambda: bwd(x, x, w, rstd.double()), lambda: bwd(x, x, w, rstd[:5]), lambda: bwd(x, x[:, :8], w[:8], rstd),
                lambda: bwd(x, x, w, rstd, out_dtype=torch.float16), lambda: bwd(x, x, w, rstd, grad_residual=x.float()),
                lambda: bwd(x, x, w, rstd, grad_residual=x, out_dtype=torch.float32), lambda: bwd(x, x, w, rstd, out=(x,)),
                lambda: bwd(x, x, w, rstd, out=(x.float(), torch.zeros(16)), out_dtype=torch.bfloat16),
                lambda: bwd(x, x, w, rstd, out=(x.half(), torch.zeros(16))), lambda: bwd(x, x, w, rstd, out=(x, torch.zeros(8))),
                lambda: bwd(x, x, w, rstd, out=(x, torch.zeros(16)), need_dweight=False), lambda: bwd(x, x, w, rstd, out=(x, None)),
                lambda: bwd(x, x, w, rstd)):                                                                               # host tensors
        with pytest.raises(E):
            bad()
    assert dga.rms_norm_backward_workspace_bytes(300, 7168) == 4 * 38 * 7168


def test_the_norm_unit_compiles_without_spills_or_scratch():
    """tests/test_build.py's method on csrc/dga_rms_norm.hip with the flags the Makefile ships it with: 40 forward builds (8 geometries x the
    three types with the weight in x's type, and the two 16-bit ones with a float32 weight), 24 backward builds (3 types x 8 geometries)
    and stage two of dweight, none with a spilled register or a byte of scratch.  LDS is the cross-wave
    partials alone: a float per wave of the workgroup where a row spans more than one wave, 4 x 64 floats in stage two."""
    unit = "dga_rms_norm.hip"
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
    assert len(seen) == 3 and all(n == 65 for n in seen.values()), seen
    want = {}
    for n in lds:
        v = re.search(r"rms_norm_(cast|backward)_kernelI\w+?Li(\d+)ELi(\d+)EEE", n)
        if v:
            lanes = int(v.group(2))
            want[n] = 0 if lanes <= 64 else 4 * max(256, lanes) // 64
        else:
            assert "rms_norm_dweight_kernel" in n
            want[n] = 4 * 64 * 4
    assert lds == want and len(lds) == 65, (lds, want)
    assert sum("rms_norm_cast_kernel" in n for n in lds) == 40 and sum("rms_norm_backward_kernel" in n for n in lds) == 24
    for kind, table in (("cast", N.FORWARD_GEOMETRY), ("backward", N.BACKWARD_GEOMETRY)):
        built = {(int(v.group(1)), int(v.group(2))) for v in (re.search(r"rms_norm_%s_kernelI\w+?Li(\d+)ELi(\d+)EEE" % kind, n) for n in lds) if v}
        assert built == {g for _, g in table}, kind
