"""CPU: combine_tokens' and combine_tokens_weight_grad's exports, the C entries' refusals (nothing is launched), the Python argument checks,
the unit's compile-time guards (dga_combine.hip), and the numpy reference of tests/combine_ref.py held to float64."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import combine_ref as C
import deepgemm_ascend_amd as dga
from deepgemm_ascend_amd import _lib
from test_build import _ship_flags

OK, E_NULL, E_SHAPE, E_DTYPE, E_RANGE = 0, -1, -2, -3, -9   # include/dga_hip.h

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "deepgemm_ascend_amd", "csrc")
UNIT = "dga_combine.hip"


def test_the_symbols_are_exported():
    text = open(os.path.join(ROOT, "include", "dga_hip.h")).read()
    cpp = open(os.path.join(CSRC, "python_api_amd.cpp")).read()
    for py, c in (("combine_tokens", "dga_combine_rows"), ("combine_tokens_weight_grad", "dga_combine_rows_weight_grad")):
        assert py in dga.__all__
        assert c in _lib.SIGNATURES
        assert re.search(rf"\bint\s+{c}\s*\(", text)
        assert callable(getattr(_lib.lib(), c))                             # ... and the built library has it
        assert f'm.def("{py}"' in cpp
    assert "#define DGA_ABI_VERSION 7" in text                              # added symbols: the ABI version stays
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert UNIT in mk.split("SRCS =")[1].split("HDRS =")[0]
    dep = [l for l in mk.splitlines() if l.rstrip().endswith(": dga_cast_device.hpp")]
    assert len(dep) == 1 and "$(OBJ)/dga_combine.o" in dep[0].split()       # Elem / Store8 come from the shared device text


ptr = lambda v: None if v is None else ctypes.c_void_p(0x1000 * v)   # (never dereferenced: every case returns before a launch)


def _combine(src=1, dt=_lib.DT_BF16, s=8, h=128, dest=2, w=None, t=4, k=2, out=3, odt=None):
    return _lib.lib().dga_combine_rows(ptr(src), dt, s, h, ptr(dest), ptr(w), t, k, ptr(out), dt if odt is None else odt, None)


def _wgrad(src=1, grad=4, dt=_lib.DT_BF16, s=8, h=128, dest=2, t=4, k=2, dw=3):
    return _lib.lib().dga_combine_rows_weight_grad(ptr(src), ptr(grad), dt, s, h, ptr(dest), t, k, ptr(dw), None)


@pytest.mark.parametrize("call", [_combine, _wgrad], ids=["combine", "weight_grad"])
def test_c_abi_refuses_without_launching(call):
    # DGA_E_SHAPE: negative sizes, k < 1, tokens * k beyond int64 -- before nothing-to-do and the pointers
    assert call(s=-1) == E_SHAPE and call(h=-1) == E_SHAPE and call(t=-1) == E_SHAPE
    assert call(k=0) == E_SHAPE and call(k=-2) == E_SHAPE
    assert call(t=1 << 40, k=1 << 40) == E_SHAPE
    assert call(k=0, t=0) == E_SHAPE and call(k=0, src=None, dest=None) == E_SHAPE
    # DGA_OK: T == 0 or H == 0, whatever the pointers
    assert call(t=0) == OK and call(h=0) == OK
    assert call(t=0, src=None, dest=None) == OK and call(h=0, src=None, dest=None, dt=99) == OK
    # DGA_E_NULL: a required pointer, before the dtype
    assert call(src=None) == E_NULL and call(dest=None) == E_NULL
    assert call(src=None, dt=99) == E_NULL
    assert call(src=None, s=0, dt=99) == E_DTYPE                            # a source without rows needs no pointer
    # DGA_E_DTYPE
    assert call(dt=_lib.DT_FP8_E4M3FN) == E_DTYPE and call(dt=99) == E_DTYPE
    # DGA_E_RANGE: k beyond int32, element indices beyond int64, more workgroups than a grid holds
    assert call(t=2, k=1 << 31) == E_RANGE
    assert call(s=1 << 40, h=1 << 40) == E_RANGE and call(t=1 << 40, h=1 << 40) == E_RANGE
    assert call(t=1 << 31, h=8) == E_RANGE


def test_c_abi_refusals_of_each_entry_alone():
    assert _combine(out=None) == E_NULL and _combine(out=None, odt=99) == E_NULL
    assert _combine(odt=_lib.DT_FP16) == E_DTYPE and _combine(odt=99) == E_DTYPE                 # out: src's dtype or fp32
    assert _combine(dt=_lib.DT_FP32, odt=_lib.DT_BF16) == E_DTYPE
    assert _combine(dt=99, odt=_lib.DT_FP32) == E_DTYPE
    assert _combine(t=1 << 30, h=1 << 13) == E_RANGE                        # 2 parts a row: 2^31 workgroups
    assert _wgrad(grad=None) == E_NULL and _wgrad(dw=None) == E_NULL


def _z(*shape, dtype=torch.bfloat16):
    return torch.zeros(*shape, dtype=dtype)


COMBINE_ARGS = [
    ("src_rank", "src must be a contiguous"), ("src_strided", "src must be a contiguous"), ("src_dtype", "float32, bfloat16 or float16"),
    ("dest_dtype", r"dest must be a contiguous int64 \[T, k\]"), ("dest_rank", r"dest must be a contiguous int64 \[T, k\]"),
    ("dest_k0", "k >= 1"), ("w_dtype", r"weights must be contiguous float32 \[4, 2\]"), ("w_shape", r"weights must be contiguous float32 \[4, 2\]"),
    ("out_shape", r"out must be contiguous \[4, 200\]"), ("out_dtype", "out must have src's dtype or float32"),
]


@pytest.mark.parametrize("case,msg", COMBINE_ARGS, ids=[c[0] for c in COMBINE_ARGS])
def test_combine_argument_errors_raise(case, msg):
    src, dest, kw = _z(8, 200), torch.zeros(4, 2, dtype=torch.int64), {}
    if case == "src_rank":
        src = _z(2, 4, 200)
    elif case == "src_strided":
        src = _z(8, 400)[:, :200]
    elif case == "src_dtype":
        src = _z(8, 200, dtype=torch.float64)
    elif case == "dest_dtype":
        dest = dest.int()
    elif case == "dest_rank":
        dest = dest.view(-1)
    elif case == "dest_k0":
        dest = torch.zeros(4, 0, dtype=torch.int64)
    elif case == "w_dtype":
        kw["weights"] = torch.zeros(4, 2, dtype=torch.float64)
    elif case == "w_shape":
        kw["weights"] = torch.zeros(4, 3)
    elif case == "out_shape":
        kw["out"] = _z(4, 100)
    elif case == "out_dtype":
        kw["out"] = _z(4, 200, dtype=torch.float16)
    with pytest.raises(dga.DGAError, match=msg):
        dga.combine_tokens(src, dest, **kw)


WGRAD_ARGS = [
    ("src_dtype", "float32, bfloat16 or float16"), ("dest_dtype", r"dest must be a contiguous int64 \[T, k\]"),
    ("grad_shape", r"grad must be contiguous \[4, 200\]"), ("grad_dtype", "grad must have src's dtype"),
    ("out_dtype", r"out must be contiguous float32 \[4, 2\]"), ("out_shape", r"out must be contiguous float32 \[4, 2\]"),
]


@pytest.mark.parametrize("case,msg", WGRAD_ARGS, ids=[c[0] for c in WGRAD_ARGS])
def test_weight_grad_argument_errors_raise(case, msg):
    src, grad, dest, kw = _z(8, 200), _z(4, 200), torch.zeros(4, 2, dtype=torch.int64), {}
    if case == "src_dtype":
        src = _z(8, 200, dtype=torch.float64)
    elif case == "dest_dtype":
        dest = dest.int()
    elif case == "grad_shape":
        grad = _z(8, 200)
    elif case == "grad_dtype":
        grad = _z(4, 200, dtype=torch.float16)
    elif case == "out_dtype":
        kw["out"] = _z(4, 2)
    elif case == "out_shape":
        kw["out"] = torch.zeros(2, 4)
    with pytest.raises(dga.DGAError, match=msg):
        dga.combine_tokens_weight_grad(src, grad, dest, **kw)


@pytest.mark.parametrize("layout", ["plain", "weights", "out", "out_fp32", "weight_grad", "weight_grad_out"])
def test_a_valid_cpu_call_gets_past_every_argument_check(layout):
    """The same arguments without a fault reach the device guard (so each case above is refused by its own check): CPU tensors raise there."""
    src, dest = _z(8, 200), torch.zeros(4, 2, dtype=torch.int64)
    with pytest.raises(dga.DGAError, match="no CPU path"):
        if layout.startswith("weight_grad"):
            dga.combine_tokens_weight_grad(src, _z(4, 200), dest, **({"out": torch.zeros(4, 2)} if layout.endswith("out") else {}))
        else:
            kw = {"plain": {}, "weights": {"weights": torch.zeros(4, 2)}, "out": {"out": _z(4, 200)},
                  "out_fp32": {"out": torch.zeros(4, 200)}}[layout]
            dga.combine_tokens(src, dest, **kw)


def test_the_unit_compiles_without_spills_scratch_or_contraction(tmp_path):
    """tests/test_build.py's method on dga_combine.hip, with the Makefile's flags; and the combine kernels hold no fused multiply-add
    (the definition is two roundings), which the weight gradient's may."""
    flags = _ship_flags(UNIT)
    assert "--offload-arch=gfx950" in flags and "-O3" in flags
    asm = tmp_path / "dga_combine.s"
    cmd = ["/opt/rocm/bin/hipcc", *flags, "--cuda-device-only", "-S", "-o", str(asm), "-Rpass-analysis=kernel-resource-usage",
           os.path.join(CSRC, UNIT)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=CSRC)
    assert r.returncode == 0, r.stderr[-2000:]
    name, seen = None, set()
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            seen.add(name)
        m = re.search(r"(VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]): (\d+)", line)
        if m:
            assert int(m.group(2)) == 0, f"{name}: {m.group(1)} = {m.group(2)}"
    assert sum("combine_rows_kernel" in n for n in seen) == 10              # (bf16, fp16) x (out as src / fp32) x (weights or not), fp32 -> fp32 x 2
    assert sum("combine_rows_weight_grad_kernel" in n for n in seen) == 3
    kernel, fused = None, {}
    for line in asm.read_text().splitlines():
        m = re.match(r"(_ZN3dga\w+):", line)
        if m:
            kernel = m.group(1)
        elif kernel and re.match(r"\s+v_(pk_)?(fma|fmac|mad|mac)\w*_f32", line):
            fused[kernel] = fused.get(kernel, 0) + 1
    assert not [k for k in fused if "combine_rows_kernel" in k], fused
    assert all(fused.get(k, 0) > 0 for k in seen if "weight_grad" in k)      # (the search does find them where they are)


# ---- the numpy reference against float64

def _f64(a):
    return np.asarray(a, np.float64)


def test_the_reference_rounds_every_partial_sum_once_from_float64():
    """Case k = 8, H = 384, bf16, weighted.  A product of two float32 is exact in float64 and the float64 sum of two float32-sized terms
    rounds to float32 as the exact sum does (53 >= 2 * 24 + 2 bits), so every step of the definition can be checked against float64: the
    product is fl32 of the exact product, the partial sum fl32 of the exact sum of the previous partial sum and that product."""
    c = C.make_case(8, 384, "bf16")
    steps = C.combine_partial_sums(c["src"], c["dest"], c["w"])
    prev = np.zeros((C.T, 384), np.float32)
    for j, (ok, prod, acc) in enumerate(steps):
        rows = c["src"][np.where(ok, c["dest"][:, j], 0)][ok]
        exact = _f64(c["w"][ok, j])[:, None] * _f64(rows)
        assert np.array_equal(prod[ok].view(np.uint32), exact.astype(np.float32).view(np.uint32)), j
        want = (_f64(prev[ok]) + _f64(prod[ok])).astype(np.float32)
        assert np.array_equal(acc[ok].view(np.uint32), want.view(np.uint32)), j
        assert np.array_equal(acc[~ok].view(np.uint32), prev[~ok].view(np.uint32)), j          # a dropped choice changes nothing
        prev = acc
    assert np.isfinite(prev).all() and not prev[C.EMPTY_TOKEN].any() and not np.signbit(prev[C.EMPTY_TOKEN]).any()
    # the unweighted sum: the product is the value itself
    plain = C.combine_partial_sums(c["src"], c["dest"], None)
    assert all(np.array_equal(p[ok], c["src"][c["dest"][ok, j]]) for j, (ok, p, _) in enumerate(plain))


@pytest.mark.parametrize("dtype", C.DTYPES)
def test_a_fused_multiply_add_would_show_in_the_weighted_case(dtype):
    """The GPU test compares bits; that tells two roundings from one only if the case holds elements where they differ.  Emulated per step:
    fl32(acc + exact product) against fl32(acc + fl32(product)), both from the reference's own previous partial sum -- and the difference
    must survive to the bits of out, in the source type and in float32."""
    c = C.make_case(8, 384, dtype)
    prev = np.zeros((C.T, 384), np.float32)
    differ = 0
    for j, (ok, prod, acc) in enumerate(C.combine_partial_sums(c["src"], c["dest"], c["w"])):
        rows = c["src"][np.where(ok, c["dest"][:, j], 0)][ok]
        fused = (_f64(prev[ok]) + _f64(c["w"][ok, j])[:, None] * _f64(rows)).astype(np.float32)
        differ += int((fused.view(np.uint32) != acc[ok].view(np.uint32)).sum())
        prev = acc
    assert differ >= 100, differ
    # a kernel that fuses every step: its float32 output differs from the definition's (the 16-bit outputs round most of it away, which is
    # why the GPU test also takes out in float32)
    steps = C.combine_partial_sums(c["src"], c["dest"], c["w"])
    chain = np.zeros((C.T, 384), np.float32)
    for j, (ok, _, _) in enumerate(steps):
        chain[ok] = (_f64(chain[ok]) + _f64(c["w"][ok, j])[:, None] * _f64(c["src"][c["dest"][ok, j]])).astype(np.float32)
    assert (C.round_to(chain, "fp32") != C.round_to(steps[-1][2], "fp32")).sum() >= 100


def test_the_weight_gradient_bar_holds_for_a_float32_sum_in_another_order():
    """The bar is for any order: numpy's pairwise float32 sum of float32 products is one, a sequential one another."""
    c = C.make_case(8, 7176, "fp32")
    ref, bar = C.weight_grad_ref(c["src"], c["grad"], c["dest"])
    ok = C.valid(c["dest"], C.S)
    rows = c["src"][np.where(ok, c["dest"], 0)]
    with np.errstate(invalid="ignore"):
        prod = np.multiply(rows, c["grad"][:, None, :], dtype=np.float32)
    pairwise = np.where(ok, prod.sum(-1, dtype=np.float32), 0)
    seq = np.where(ok, np.cumsum(prod, axis=-1, dtype=np.float32)[..., -1], 0)
    for got in (pairwise, seq):
        assert (np.abs(_f64(got) - ref) <= bar).all()
    assert (bar[ok] > 0).all() and not bar[~ok].any() and not ref[~ok].any()
