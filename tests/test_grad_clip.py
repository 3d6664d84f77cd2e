"""CPU: grad_sumsq, grad_clip_scalars, clip_grad_norm_step_scalars and the optimizer's skip= are exported through every layer, the
reference tests/grad_clip_ref.py holds is torch.nn.utils.clip_grad_norm_ in float64, the C entries' argument checks return their codes
before any launch, the Python entries refuse what they must with whole-string messages, and the new unit compiles for gfx950 without
spills or scratch."""
import ctypes
import re
import subprocess

import numpy as np
import pytest
import torch

import grad_clip_ref as R
from test_build import CSRC, ROOT, _ship_flags

SYMBOLS = ("dga_grad_sumsq_workspace_bytes", "dga_grad_sumsq", "dga_grad_clip_scalars", "dga_adamw_cast_to_fp8_128x128_transposed_skip")
PY_ENTRIES = ("grad_sumsq", "grad_clip_scalars", "clip_grad_norm_step_scalars", "grad_sumsq_workspace_bytes")
OK, E_NULL, E_SHAPE, E_DTYPE, E_RANGE = 0, -1, -2, -3, -9


def test_the_entries_are_exported_through_every_layer(dga):
    from deepgemm_ascend_amd import _lib
    header = (ROOT / "include" / "dga_hip.h").read_text()
    L = ctypes.CDLL(str(_lib.LIB_PATH))
    for symbol in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % symbol, header), symbol
        assert hasattr(L, symbol) and symbol in _lib.SIGNATURES, symbol
    for name in PY_ENTRIES:
        assert name in dga.__all__ and callable(getattr(dga, name)), name
    assert "#define DGA_ABI_VERSION 7\n" in header and L.dga_abi_version() == 7
    assert "#define DGA_GRAD_SUMSQ_CHUNK %d\n" % R.CHUNK in header
    makefile = (CSRC / "Makefile").read_text()
    assert re.search(r"^SRCS = .*\bdga_grad_norm\.hip\b", makefile, flags=re.M)
    assert re.search(r"^\$\(OBJ\)/dga_cast\.o .*\$\(OBJ\)/dga_grad_norm\.o.*: dga_cast_device\.hpp$", makefile, flags=re.M)
    import inspect
    assert inspect.signature(dga.adamw_per_block_cast_to_fp8_transposed).parameters["skip"].default is None


def test_workspace_bytes(dga):
    C = R.CHUNK
    assert dga.grad_sumsq_workspace_bytes([]) == 0 and dga.grad_sumsq_workspace_bytes([0, 0]) == 0
    assert dga.grad_sumsq_workspace_bytes([1]) == 8 and dga.grad_sumsq_workspace_bytes([C, C + 1, 0, 3 * C + 5]) == 8 * (1 + 2 + 4)
    assert dga.grad_sumsq_workspace_bytes(R.SIZES) == 8 * sum(-(-n // C) for n in R.SIZES)
    assert dga.grad_sumsq_workspace_bytes([-1]) == 0 and dga.grad_sumsq_workspace_bytes([C << 31]) == 0      # what the entry refuses


@pytest.mark.parametrize("clipping", (True, False), ids=("clipping", "not_clipping"))
def test_the_reference_is_torch_clip_grad_norm(clipping):
    """clip_grad_norm_ on float64 CPU tensors: the total norm it returns and the factor it multiplied the gradients by, to 1e-15."""
    rng = np.random.default_rng(5)
    arrays = [rng.standard_normal(s) for s in ((33, 7), (129,), (4, 5, 6))]
    params = [torch.nn.Parameter(torch.zeros(a.shape, dtype=torch.float64)) for a in arrays]
    for p, a in zip(params, arrays):
        p.grad = torch.from_numpy(a.copy())
    exact = R.sumsq(arrays)
    max_norm = (0.5 if clipping else 2.0) * np.sqrt(exact)
    total = torch.nn.utils.clip_grad_norm_(params, max_norm)                  # eps = 1e-6 inside
    with np.errstate(all="ignore"):
        normd = np.sqrt(np.float64(exact))
        coefd = min(1.0, max_norm / (normd + 1e-6))
    assert abs(total.item() - normd) <= 1e-15 * normd
    factor = (params[0].grad.numpy() / arrays[0]).ravel()
    assert np.abs(factor - coefd).max() <= 1e-15 * coefd and (coefd < 1.0) == clipping
    norm, coef, scale, skip = R.clip_scalars(exact, max_norm)
    assert norm == np.float32(normd) and coef == np.float32(coefd) and scale == coef and skip == 0


def test_the_reference_follows_the_definition():
    f = np.float32
    assert R.sumsq([f([3, 4]), f([]), f([12])]) == 169.0 and R.count([f([3, 4]), f([]), f([12])]) == 3
    assert R.sumsq([f([1, np.inf])]) == np.inf and np.isnan(R.sumsq([f([1, -np.inf]), f([np.nan])])) and R.sumsq([f([-np.inf])]) == np.inf
    assert R.clip_scalars(64.0, 2.0, 1.0, 0.0) == (f(8), f(0.25), f(0.25), 0)
    assert R.clip_scalars(1024.0, 64.0, 0.5, 0.0) == (f(16), f(1), f(0.5), 0)
    assert R.clip_scalars(0.0, 1.0, 1.0, 0.0)[1:] == (f(1), f(1), 0) and R.clip_scalars(0.0, 0.0, 1.0, 0.0)[1:] == (f(1), f(1), 0)
    for bad in (np.inf, np.nan):
        norm, coef, scale, skip = R.clip_scalars(bad, 1.0)
        assert not np.isfinite(norm) and (coef, scale, skip) == (f(0), f(0), 1)
    assert np.array_equal(R.bf16(f([1.0, 1.00390625, 1.01171875])).view(np.uint32) >> 16, [0x3F80, 0x3F80, 0x3F82])     # ties to even


def _aligned(nbytes=256):
    buf = (ctypes.c_char * (nbytes + 16))()
    return buf, (ctypes.addressof(buf) + 15) & ~15


def test_grad_sumsq_checks_its_arguments_before_any_launch(dga):
    """No GPU is needed: every refusal returns before the first launch."""
    from deepgemm_ascend_amd import _lib
    L = _lib.lib()
    keep, p = _aligned()
    F32, BF16, F16 = _lib.DT_FP32, _lib.DT_BF16, _lib.DT_FP16

    def call(numel=(8, 0, 3), dts=(F32, BF16, F32), ptrs=None, count=None, tensors=True, sizes=True, types=True, sumsq=p, ws=p, ws_bytes=64):
        n = len(numel)
        ptrs = [p] * n if ptrs is None else ptrs
        a_p = (ctypes.c_void_p * max(n, 1))(*ptrs) if tensors else None
        a_n = (ctypes.c_int64 * max(n, 1))(*numel) if sizes else None
        a_d = (ctypes.c_int * max(n, 1))(*dts) if types else None
        return L.dga_grad_sumsq(a_p, a_n, a_d, n if count is None else count, sumsq, 0, ws, ws_bytes, None)

    for bad in (dict(count=-1), dict(numel=(8, -1, 3)), dict(count=-1, sumsq=None), dict(numel=(-1, 0, 0), sumsq=None, dts=(99, 99, 99))):
        assert call(**bad) == E_SHAPE, bad
    for bad in (dict(sizes=False), dict(sumsq=None), dict(tensors=False), dict(types=False), dict(ptrs=[p, None, None]), dict(ws=None),
                dict(sumsq=None, dts=(F16, F32, F32)), dict(ws=None, ws_bytes=0, dts=(99, F32, F32))):
        assert call(**bad) == E_NULL, bad
    for bad in (dict(dts=(F16, F32, F32)), dict(dts=(F32, F16, F32)), dict(dts=(F32, F32, 99)), dict(dts=(F32, F32, _lib.DT_FP8_E4M3FN)),
                dict(dts=(F16, F32, F32), ws_bytes=0)):
        assert call(**bad) == E_DTYPE, bad
    C = R.CHUNK
    for bad in (dict(ws_bytes=8), dict(ws_bytes=0), dict(numel=(C + 1, 0, 1), ws_bytes=16), dict(ws=p + 4), dict(numel=(C << 31, 0, 0)),
                dict(numel=(C << 30, C << 30, 1), ws_bytes=1 << 40), dict(numel=(1 << 62, 1 << 62, 1 << 62))):
        assert call(**bad) == E_RANGE, bad
    assert L.dga_grad_sumsq_workspace_bytes(-1, None) == 0 and L.dga_grad_sumsq_workspace_bytes(2, None) == 0
    assert L.dga_grad_sumsq_workspace_bytes(0, None) == 0


def test_grad_clip_scalars_checks_its_arguments_before_any_launch(dga):
    from deepgemm_ascend_amd import _lib
    L = _lib.lib()
    keep, p = _aligned()
    inf, nan = float("inf"), float("nan")

    def call(sumsq=p, mx=1.0, ps=1.0, eps=1e-6, sc=p, norm=p, coef=p, skip=p):
        return L.dga_grad_clip_scalars(sumsq, mx, ps, eps, sc, norm, coef, skip, None)

    for name in ("sumsq", "sc", "norm", "coef", "skip"):
        assert call(**{name: None}) == E_NULL, name
        assert call(**{name: None}, mx=-1.0) == E_NULL, name
    for bad in (dict(mx=-1.0), dict(mx=-1e-300), dict(mx=nan), dict(mx=-inf), dict(ps=0.0), dict(ps=-1.0), dict(ps=inf), dict(ps=nan),
                dict(eps=-1e-9), dict(eps=inf), dict(eps=nan)):
        assert call(**bad) == E_RANGE, bad


def test_the_skip_entry_checks_its_arguments_as_the_plain_one(dga):
    """The flag is one more pointer: NULL is valid, and every refusal of the existing entry comes back with or without it."""
    from deepgemm_ascend_amd import _lib
    L = _lib.lib()
    keep, p = _aligned()
    F32, F16 = _lib.DT_FP32, _lib.DT_FP16

    def call(groups=2, n=8, k=8, mdt=F32, gdt=F32, w=p, sc=p, b1=0.9, flags=0, q=None, skip=p):
        return L.dga_adamw_cast_to_fp8_128x128_transposed_skip(w, p, p, mdt, p, gdt, sc, b1, 0.95, 1e-8, 0.0, groups, n, k, p, p, q, None, flags,
                                                               skip, None)

    for skip in (p, None):
        assert call(flags=2, skip=skip) == E_RANGE and call(n=-1, skip=skip) == E_SHAPE and call(q=p, skip=skip) == E_SHAPE
        assert call(groups=0, w=None, skip=skip) == OK and call(w=None, skip=skip) == E_NULL and call(sc=None, skip=skip) == E_NULL
        assert call(mdt=F16, skip=skip) == E_DTYPE and call(gdt=F16, skip=skip) == E_DTYPE
        assert call(b1=1.0, skip=skip) == E_RANGE and call(groups=1 << 40, skip=skip) == E_RANGE


def _whole(msg):
    from deepgemm_ascend_amd import _lib
    return "^" + re.escape(f"host assert: status -2 ({_lib.status_string(-2)}) {msg}") + "$"


GUARD_MSG = "tensors must be on a HIP device (there is no CPU path)"
LIST_MSG = "tensors must be a tensor or a non-empty list or tuple of tensors"
ITEM_MSG = "tensors[%d] must be a contiguous float32 or bfloat16 tensor"
SUMSQ_MSG = "sumsq must be contiguous float64 [1]"
SCALARS_MSG = "step_scalars must be contiguous float32 [4]"
MAX_MSG = "max_norm must be >= 0 (it may be inf)"
PRE_MSG = "pre_scale must be finite and > 0"
EPS_MSG = "eps must be finite and >= 0"
SKIP_MSG = "skip must be contiguous int32 [1]"
_Z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype)
_F64, _I32 = torch.float64, torch.int32

SUMSQ_FAULTS = [
    (dict(tensors=[]), LIST_MSG), (dict(tensors=()), LIST_MSG), (dict(tensors=None), LIST_MSG), (dict(tensors=3.0), LIST_MSG),
    (dict(tensors=[_Z(4, dtype=torch.float16)]), ITEM_MSG % 0), (dict(tensors=[_Z(4), _Z(4, dtype=torch.float16)]), ITEM_MSG % 1),
    (dict(tensors=[_Z(4), _Z(4, 6)[:, ::2]]), ITEM_MSG % 1), (dict(tensors=_Z(6, 4).t()), ITEM_MSG % 0),
    (dict(tensors=[_Z(4, dtype=_F64)]), ITEM_MSG % 0), (dict(tensors=[_Z(4), [1.0]]), ITEM_MSG % 1),
    (dict(out=[0.0]), "out must be a tensor"), (dict(out=_Z(1)), "out " + SUMSQ_MSG), (dict(out=_Z(2, dtype=_F64)), "out " + SUMSQ_MSG),
    (dict(out=_Z((), dtype=_F64)), "out " + SUMSQ_MSG), (dict(accumulate=True), "accumulate=True needs out="),
    (dict(tensors=[], out=_Z(1)), LIST_MSG),
]


@pytest.mark.parametrize("fault,msg", SUMSQ_FAULTS, ids=[f"{i}-{'+'.join(f)}" for i, (f, _) in enumerate(SUMSQ_FAULTS)])
def test_grad_sumsq_gives_one_fault_its_own_message(dga, fault, msg):
    with pytest.raises(dga.DGAError, match=_whole(msg)):
        dga.grad_sumsq(**{**dict(tensors=[_Z(3, 5), _Z(0), _Z(7, dtype=torch.bfloat16)]), **fault})


def _clip_valid():
    return dict(sumsq=_Z(1, dtype=_F64), step_scalars=torch.ones(4), max_norm=1.0)


CLIP_FAULTS = [
    (dict(sumsq=_Z(1)), SUMSQ_MSG), (dict(sumsq=_Z(2, dtype=_F64)), SUMSQ_MSG), (dict(sumsq=_Z((), dtype=_F64)), SUMSQ_MSG),
    (dict(sumsq=1.0), "sumsq must be a tensor"),
    (dict(step_scalars=torch.ones(5)), SCALARS_MSG), (dict(step_scalars=torch.ones(4, dtype=_F64)), SCALARS_MSG),
    (dict(step_scalars=torch.ones(8)[::2]), SCALARS_MSG), (dict(step_scalars=[1.0] * 4), "step_scalars must be a tensor"),
    (dict(max_norm=-1.0), MAX_MSG), (dict(max_norm=float("nan")), MAX_MSG),
    (dict(pre_scale=0.0), PRE_MSG), (dict(pre_scale=-2.0), PRE_MSG), (dict(pre_scale=float("inf")), PRE_MSG), (dict(pre_scale=float("nan")), PRE_MSG),
    (dict(eps=-1e-6), EPS_MSG), (dict(eps=float("nan")), EPS_MSG), (dict(eps=float("inf")), EPS_MSG),
    (dict(out=(_Z(1), _Z(1))), "out must be (norm, coef, skip)"), (dict(out=_Z(1)), "out must be (norm, coef, skip)"),
    (dict(out=(_Z(1), _Z(2), _Z(1, dtype=_I32))), "out coef must be contiguous float32 [1]"),
    (dict(out=(_Z(1), _Z(1), _Z(1))), "out skip must be contiguous int32 [1]"),
    (dict(out=(_Z(1, dtype=_F64), _Z(1), _Z(1, dtype=_I32))), "out norm must be contiguous float32 [1]"),
    (dict(sumsq=_Z(1), max_norm=-1.0), SUMSQ_MSG), (dict(max_norm=-1.0, eps=-1.0), MAX_MSG),
]


@pytest.mark.parametrize("fault,msg", CLIP_FAULTS, ids=[f"{i}-{'+'.join(f)}" for i, (f, _) in enumerate(CLIP_FAULTS)])
def test_grad_clip_scalars_gives_one_fault_its_own_message(dga, fault, msg):
    with pytest.raises(dga.DGAError, match=_whole(msg)):
        dga.grad_clip_scalars(**{**_clip_valid(), **fault})


WRAPPER_FAULTS = [
    (dict(tensors=[]), LIST_MSG), (dict(tensors=[_Z(4, dtype=torch.float16)]), ITEM_MSG % 0), (dict(step_scalars=torch.ones(3)), SCALARS_MSG),
    (dict(max_norm=-0.5), MAX_MSG), (dict(pre_scale=0.0), PRE_MSG), (dict(eps=float("nan")), EPS_MSG),
    (dict(out=(_Z(1), _Z(1), _Z(1, dtype=_I32))), "out must be (norm, coef, skip, sumsq)"),
    (dict(out=(_Z(1), _Z(1), _Z(1, dtype=_I32), _Z(1))), "out " + SUMSQ_MSG),
    (dict(out=(_Z(1), _Z(1), _Z(1), _Z(1, dtype=_F64))), "out skip must be contiguous int32 [1]"),
]


@pytest.mark.parametrize("fault,msg", WRAPPER_FAULTS, ids=[f"{i}-{'+'.join(f)}" for i, (f, _) in enumerate(WRAPPER_FAULTS)])
def test_clip_grad_norm_step_scalars_gives_one_fault_its_own_message(dga, fault, msg):
    with pytest.raises(dga.DGAError, match=_whole(msg)):
        dga.clip_grad_norm_step_scalars(**{**dict(tensors=[_Z(3, 5)], step_scalars=torch.ones(4), max_norm=1.0), **fault})


def _adamw_valid():
    w = lambda: torch.zeros(2, 8, 16)
    return dict(w=w(), m=w(), v=w(), grad=w(), step_scalars=torch.ones(4))


@pytest.mark.parametrize("skip,msg", [(_Z(1), SKIP_MSG), (_Z(2, dtype=_I32), SKIP_MSG), (_Z((), dtype=_I32), SKIP_MSG),
                                      (_Z(1, dtype=torch.int64), SKIP_MSG), (_Z(1, 1, dtype=_I32), SKIP_MSG), (1, "skip must be a tensor")],
                         ids=("float32", "two", "0-d", "int64", "2-d", "int"))
def test_the_optimizer_refuses_a_skip_that_is_not_int32_1(dga, skip, msg):
    with pytest.raises(dga.DGAError, match=_whole(msg)):
        dga.adamw_per_block_cast_to_fp8_transposed(**_adamw_valid(), skip=skip)


def test_the_valid_arguments_reach_the_device_guard(dga):
    """... so that every case above is refused by its own check, which runs before the guard."""
    bf = torch.bfloat16
    for tensors in (_Z(3, 5), [_Z(3, 5)], (_Z(0), _Z(7, dtype=bf)), [_Z(2, 3, 4, dtype=bf), _Z(()), _Z(5)]):
        for extra in (dict(), dict(out=_Z(1, dtype=_F64)), dict(out=_Z(1, dtype=_F64), accumulate=True)):
            with pytest.raises(dga.DGAError, match=_whole(GUARD_MSG)):
                dga.grad_sumsq(tensors, **extra)
    for extra in (dict(), dict(max_norm=float("inf")), dict(max_norm=0, eps=0.0, pre_scale=1.0 / 65536),
                  dict(out=(_Z(1), _Z(1), _Z(1, dtype=_I32)))):
        with pytest.raises(dga.DGAError, match=_whole(GUARD_MSG)):
            dga.grad_clip_scalars(**{**_clip_valid(), **extra})
    for extra in (dict(), dict(pre_scale=0.5, eps=0.0), dict(out=(_Z(1), _Z(1), _Z(1, dtype=_I32), _Z(1, dtype=_F64)))):
        with pytest.raises(dga.DGAError, match=_whole(GUARD_MSG)):
            dga.clip_grad_norm_step_scalars([_Z(3, 5), _Z(4, dtype=bf)], torch.ones(4), 1.0, **extra)
    with pytest.raises(dga.DGAError, match=_whole(GUARD_MSG)):
        dga.adamw_per_block_cast_to_fp8_transposed(**_adamw_valid(), skip=_Z(1, dtype=_I32))
    with pytest.raises(dga.DGAError, match=_whole(GUARD_MSG)):
        dga.adamw_per_block_cast_to_fp8_transposed(**_adamw_valid(), skip=None, rowwise=True)


def test_the_unit_compiles_without_spills_or_scratch():
    """tests/test_build.py's method on csrc/dga_grad_norm.hip with the flags the Makefile ships it with: the two stages and the scalars'
    kernel, none with a spilled register or a byte of scratch; LDS is the four (sixteen) float64 of the waves' sums."""
    unit = "dga_grad_norm.hip"
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
    assert len(seen) == 3 and all(n == 3 for n in seen.values()), seen
    sizes = {re.search(r"(grad_\w+?_kernel)", n).group(1): size for n, size in lds.items()}
    assert sizes == {"grad_sumsq_chunks_kernel": 32, "grad_sumsq_final_kernel": 128, "grad_clip_scalars_kernel": 0}, lds
