"""CPU: adamw_per_block_cast_to_fp8_transposed is exported through every layer, the definition tests/adamw_ref.py holds is torch's AdamW in
float64 and, in float32, lies inside its derived bounds of the float64 one, the C entry's argument checks return their codes before any
launch, the Python entries refuse what they must, and the new unit compiles for gfx950 without spills or scratch."""
import ctypes
import re
import subprocess

import numpy as np
import pytest
import torch

import adamw_ref as A
from test_build import CSRC, ROOT, _ship_flags

SYMBOL = "dga_adamw_cast_to_fp8_128x128_transposed"
PY_ENTRIES = ("adamw_per_block_cast_to_fp8_transposed", "adamw_step_scalars")


def test_the_entry_is_exported_through_every_layer(dga):
    from deepgemm_ascend_amd import _lib
    header = (ROOT / "include" / "dga_hip.h").read_text()
    L = ctypes.CDLL(str(_lib.LIB_PATH))
    assert re.search(r"\b%s\s*\(" % SYMBOL, header)
    assert hasattr(L, SYMBOL) and SYMBOL in _lib.SIGNATURES
    for name in PY_ENTRIES:
        assert name in dga.__all__ and callable(getattr(dga, name)), name
    assert "#define DGA_ABI_VERSION 7\n" in header and L.dga_abi_version() == 7
    makefile = (CSRC / "Makefile").read_text()
    assert re.search(r"^SRCS = .*\bdga_adamw_cast\.hip\b", makefile, flags=re.M)
    assert re.search(r"^\$\(OBJ\)/dga_cast\.o .*\$\(OBJ\)/dga_adamw_cast\.o.*: dga_cast_device\.hpp$", makefile, flags=re.M)
    assert "#pragma clang fp contract(off)" in (CSRC / "dga_adamw_cast.hip").read_text()


def test_step_scalars(dga):
    s = dga.adamw_step_scalars(7, A.LR, A.BETA1, A.BETA2, 0.5, device="cpu")
    assert s.dtype == torch.float32 and tuple(s.shape) == (4,)
    assert np.array_equal(s.numpy().view(np.uint32), A.scalars(7, A.LR, A.BETA1, A.BETA2, 0.5).view(np.uint32))
    want = np.array([A.LR, 1 - A.BETA1 ** 7, (1 - A.BETA2 ** 7) ** 0.5, 0.5], np.float64).astype(np.float32)        # float64, rounded once
    assert np.array_equal(s.numpy(), want)
    out = torch.zeros(4)
    assert dga.adamw_step_scalars(1000, 1e-3, 0.9, 0.999, out=out) is out
    assert np.array_equal(out.numpy().view(np.uint32), A.scalars(1000, 1e-3, 0.9, 0.999).view(np.uint32))
    for bad in (lambda: dga.adamw_step_scalars(0, 1e-3, 0.9, 0.95), lambda: dga.adamw_step_scalars(1, 1e-3, 1.0, 0.95),
                lambda: dga.adamw_step_scalars(1, 1e-3, 0.9, -0.1), lambda: dga.adamw_step_scalars(1, 1e-3, 0.9, 0.95, out=torch.zeros(5)),
                lambda: dga.adamw_step_scalars(1, 1e-3, 0.9, 0.95, out=torch.zeros(4, dtype=torch.float64))):
        with pytest.raises(dga.DGAError):
            bad()


def test_the_float64_definition_is_torch_adamw():
    """Five steps of torch.optim.AdamW in float64 against the reference in float64 with float64 scalars: the formulas differ by
    rearrangement only (torch forms m' as m + (g - m)(1 - beta1)), held to 2^-40 max|w|."""
    rng = np.random.default_rng(11)
    shape = (3, 17, 23)
    w0 = rng.standard_normal(shape) * 0.05
    p = torch.nn.Parameter(torch.from_numpy(w0.copy()))
    opt = torch.optim.AdamW([p], lr=A.LR, betas=(A.BETA1, A.BETA2), eps=A.EPS, weight_decay=A.WD)
    w, m, v = w0.copy(), np.zeros(shape), np.zeros(shape)
    worst = 0.0
    for t in range(1, 6):
        g = rng.standard_normal(shape) * 1e-3 * 10.0 ** rng.uniform(-2, 1, shape)
        p.grad = torch.from_numpy(g.copy())
        opt.step()
        w, m, v = A.step(w, m, v, g, A.scalars(t, A.LR, A.BETA1, A.BETA2, dtype=np.float64), A.BETA1, A.BETA2, A.EPS, A.WD, dtype=np.float64)
        worst = max(worst, np.abs(w - p.detach().numpy()).max() / np.abs(w).max())
    print("float64 reference against torch.optim.AdamW, 5 steps: %.3g of max|w|" % worst)
    assert worst <= 2.0 ** -40
    st = opt.state[p]
    assert np.abs(m - st["exp_avg"].numpy()).max() <= 2.0 ** -40 * np.abs(m).max()
    assert np.abs(v - st["exp_avg_sq"].numpy()).max() <= 2.0 ** -40 * np.abs(v).max()


@pytest.mark.parametrize("step,wd,zero", ((1, 0.0, True), (3, A.WD, False), (1000, A.WD, False)), ids=("step1", "step3", "step1000"))
def test_float32_lies_inside_its_bounds_of_float64(step, wd, zero):
    """One step on the same float32 inputs and float32 scalars in float32 and in float64: the bounds of adamw_ref.bars (derived in DESIGN.md,
    "Optimizer").  The worst fraction of each bound is printed; DESIGN.md records it."""
    w, m, v, g = A.inputs((4, 96, 160), seed=step, zero_moments=zero)
    sc = A.scalars(step, A.LR, A.BETA1, A.BETA2, 0.5)
    b1, b2, eps, wd = A.f32(A.BETA1), A.f32(A.BETA2), A.f32(A.EPS), A.f32(wd)
    got = A.step(w, m, v, g, sc, b1, b2, eps, wd)
    exact, bar = A.bars(w, m, v, g, sc, b1, b2, eps, wd)
    for name, a, e, b in zip("wmv", got, exact, bar):
        assert a.dtype == np.float32
        frac = (np.abs(a.astype(np.float64) - e) / b).max()
        print("step %d: worst |%s' - exact| / bound = %.3f" % (step, name, frac))
        assert frac <= 1.0, name


def test_the_reference_follows_the_definition():
    """Hand-computed elements: a step from zero moments, a NaN and an infinite gradient, eps = 0 with a zero gradient, and the bfloat16
    store (round to nearest even, ties included, a NaN kept)."""
    f = np.float32
    sc = A.scalars(1, 0.25, 0.5, 0.75)
    assert np.array_equal(sc, np.array([0.25, 0.5, 0.5, 1.0], f))
    w, m, v = A.step(f([1.0, 1.0, 1.0, 1.0]), f([0, 0, 0, 0]), f([0, 0, 0, 0]), f([2.0, np.nan, np.inf, 0.0]), sc, 0.5, 0.75, 0.0, 0.5)
    # g = 2: m' = 1, v' = 1, den = sqrt(1) / 0.5 = 2, w1 = 1 - 0.125 = 0.875, w' = 0.875 - 0.5 * 0.5 = 0.625
    assert (w[0], m[0], v[0]) == (0.625, 1.0, 1.0)
    assert np.isnan(w[1]) and np.isnan(m[1]) and np.isnan(v[1])
    assert np.isnan(w[2]) and m[2] == np.inf and v[2] == np.inf
    assert np.isnan(w[3]) and m[3] == 0 and v[3] == 0                                          # eps = 0, v' = 0: 0 / 0
    w, m, v = A.step(f([1.0]), f([0]), f([0]), f([0.0]), sc, 0.5, 0.75, 1e-8, 0.5)
    assert w[0] == 0.875
    bits = A.moment_bits(np.array([0x3F808000, 0x3F818000, 0x3F808001, 0x7F7FFFFF, 0x7F800001, 0xFF800000], np.uint32).view(f), "bf16")
    assert [int(b) for b in bits[:4]] == [0x3F80, 0x3F82, 0x3F81, 0x7F80] and bits[4] & 0x7FFF > 0x7F80 and bits[5] == 0xFF80
    assert np.array_equal(A.stored(f([1.0, -2.5]), "bf16"), f([1.0, -2.5]))


def test_the_entry_checks_its_arguments_before_any_launch(dga):
    """No GPU is needed: every refusal, and the empty call, returns before the first launch."""
    from deepgemm_ascend_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_char * 128)()
    p = (ctypes.addressof(buf) + 15) & ~15
    OK, E_NULL, E_SHAPE, E_DTYPE, E_RANGE = 0, -1, -2, -3, -9
    F32, BF16, F16, FP8 = _lib.DT_FP32, _lib.DT_BF16, _lib.DT_FP16, _lib.DT_FP8_E4M3FN
    inf, nan = float("inf"), float("nan")

    def call(groups=2, n=8, k=8, mdt=F32, gdt=F32, w=p, m=p, v=p, grad=p, sc=p, b1=0.9, b2=0.95, eps=1e-8, wd=0.0, qt=p, sft=p, q=None,
             sf=None, flags=0):
        return getattr(L, SYMBOL)(w, m, v, mdt, grad, gdt, sc, b1, b2, eps, wd, groups, n, k, qt, sft, q, sf, flags, None)

    for bad in (dict(flags=2), dict(flags=-1), dict(flags=3, n=-1, w=None)):                                            # the flags go first
        assert call(**bad) == E_RANGE, bad
    for bad in (dict(groups=-1), dict(n=-1), dict(k=-1), dict(q=p), dict(sf=p), dict(n=-1, w=None, mdt=99, b1=2.0)):     # then the shape
        assert call(**bad) == E_SHAPE, bad
    nothing = dict(w=None, m=None, v=None, grad=None, sc=None, qt=None, sft=None, mdt=99, b1=2.0)
    for empty in (dict(groups=0), dict(n=0), dict(k=0)):
        assert call(**empty, **nothing) == OK, empty
    for name in ("w", "m", "v", "grad", "sc", "qt", "sft"):
        assert call(**{name: None}, mdt=99, b1=2.0) == E_NULL, name
    for bad in (dict(mdt=F16), dict(gdt=F16), dict(mdt=FP8), dict(gdt=99), dict(mdt=0), dict(mdt=F16, b1=2.0), dict(gdt=F16, eps=-1.0)):
        assert call(**bad) == E_DTYPE, bad
    for bad in (dict(b1=1.0), dict(b1=-0.1), dict(b1=nan), dict(b2=1.0), dict(b2=1.5), dict(b2=nan), dict(eps=-1e-9), dict(eps=inf),
                dict(eps=nan), dict(wd=-0.1), dict(wd=inf), dict(wd=nan), dict(groups=1 << 40), dict(n=1 << 40, k=1 << 40),
                dict(groups=1 << 20, n=1 << 20, k=1 << 20, mdt=BF16, gdt=BF16)):
        assert call(**bad) == E_RANGE, bad


def _whole(msg):
    from deepgemm_ascend_amd import _lib
    return "^" + re.escape(f"host assert: status -2 ({_lib.status_string(-2)}) {msg}") + "$"


def _valid():
    """Valid arguments on the host (distinct tensors): alone they reach the device guard, so each fault below is refused by its own check."""
    w = lambda: torch.zeros(2, 8, 16)
    return dict(w=w(), m=w(), v=w(), grad=w(), step_scalars=torch.ones(4))


GUARD_MSG = "tensors must be on a HIP device (there is no CPU path)"
W_MSG = "w must be a contiguous float32 [N, K] or [G, N, K] tensor"
MOMENT_MSG = "%s must be contiguous float32 or bfloat16 [2, 8, 16]"
SCALARS_MSG = "step_scalars must be contiguous float32 [4]"
BETA_MSG = "beta1 and beta2 must be in [0, 1) as float32"
EPS_MSG = "eps and weight_decay must be finite and >= 0"
_Z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype)
_U8 = torch.uint8
# (the arguments that replace valid ones, the whole message)
PY_FAULTS = [
    (dict(w=_Z(2, 8, 16, dtype=torch.bfloat16)), W_MSG), (dict(w=_Z(2, 8, 16, dtype=torch.float64)), W_MSG), (dict(w=_Z(16)), W_MSG),
    (dict(w=_Z(2, 16, 8).transpose(1, 2)), W_MSG), (dict(w=_Z(2, 2, 8, 16)), W_MSG), (dict(w=[1.0]), W_MSG),
    (dict(w=_Z(2, 8, 8)), "m must be contiguous float32 or bfloat16 [2, 8, 8]"),                  # w of another shape: m no longer fits
    (dict(m=_Z(2, 8, 8)), MOMENT_MSG % "m"), (dict(v=_Z(1, 8, 16)), MOMENT_MSG % "v"), (dict(grad=_Z(2, 16, 8)), MOMENT_MSG % "grad"),
    (dict(m=_Z(2, 8, 32)[:, :, ::2]), MOMENT_MSG % "m"),
    (dict(m=_Z(2, 8, 16, dtype=torch.float16), v=_Z(2, 8, 16, dtype=torch.float16)), MOMENT_MSG % "m"),          # fp16 moments
    (dict(v=_Z(2, 8, 16, dtype=torch.float16)), MOMENT_MSG % "v"), (dict(m=_Z(2, 8, 16, dtype=torch.float64)), MOMENT_MSG % "m"),
    (dict(grad=_Z(2, 8, 16, dtype=torch.float16)), MOMENT_MSG % "grad"),
    (dict(m=_Z(2, 8, 16, dtype=torch.bfloat16)), "m and v must be of one dtype"), (dict(v=_Z(2, 8, 16, dtype=torch.bfloat16)), "m and v must be of one dtype"),
    (dict(m=None), "m must be a tensor"), (dict(v=3.0), "v must be a tensor"), (dict(grad=[0.0]), "grad must be a tensor"),
    (dict(step_scalars=[1e-3, 0.1, 0.2, 1.0]), "step_scalars must be a tensor"),
    (dict(step_scalars=torch.ones(5)), SCALARS_MSG), (dict(step_scalars=torch.ones(4, 1)), SCALARS_MSG),
    (dict(step_scalars=torch.ones(4, dtype=torch.float64)), SCALARS_MSG), (dict(step_scalars=torch.ones(8)[::2]), SCALARS_MSG),
    (dict(beta1=1.0), BETA_MSG), (dict(beta2=-0.5), BETA_MSG), (dict(beta1=1.0 - 1e-12), BETA_MSG), (dict(beta2=float("nan")), BETA_MSG),
    (dict(eps=-1.0), EPS_MSG), (dict(eps=float("nan")), EPS_MSG), (dict(eps=float("inf")), EPS_MSG), (dict(weight_decay=float("inf")), EPS_MSG),
    (dict(weight_decay=-0.1), EPS_MSG),
    (dict(out=(_Z(2, 16, 8, dtype=_U8),)), "out must be (qt, sft)"), (dict(out=_Z(2, 16, 8, dtype=_U8)), "out must be (qt, sft)"),
    (dict(rowwise=True, out=(_Z(2, 16, 8, dtype=_U8),)), "out must be ((qt, sft), (q, sf))"),
    (dict(out=((_Z(2, 16, 8, dtype=_U8), _Z(2, 1, 1)), (_Z(2, 8, 16, dtype=_U8), _Z(2, 1, 1)))), "out must hold (qt, sft)"),   # nested without rowwise
    (dict(rowwise=True, out=(_Z(2, 16, 8, dtype=_U8), _Z(2, 1, 1))), "out must hold (qt, sft)"),                                # flat with it
    (dict(rowwise=True, out=((_Z(2, 16, 8, dtype=_U8), _Z(2, 1, 1)), (_Z(2, 8, 16, dtype=_U8),))), "out must hold (q, sf)"),
    (dict(out=(_Z(2, 8, 16, dtype=_U8), _Z(2, 1, 1))), "out qt must be contiguous [2, 16, 8]"),                                 # qt is [G, K, N]
    (dict(out=(_Z(2, 16, 8), _Z(2, 1, 1))), "fp8 operand must be float8_e4m3fn or uint8 bytes, got torch.float32"),
    (dict(out=(_Z(2, 16, 8, dtype=_U8), _Z(2, 1, 2))), "out sft must be contiguous float32 [2, 1, 1]"),
    (dict(rowwise=True, out=((_Z(2, 16, 8, dtype=_U8), _Z(2, 1, 1)), (_Z(2, 16, 8, dtype=_U8), _Z(2, 1, 1)))), "out q must be contiguous [2, 8, 16]"),
    (dict(rowwise=True, out=((_Z(2, 16, 8, dtype=_U8), _Z(2, 1, 1)), (_Z(2, 8, 16, dtype=_U8), _Z(2, 1, 1, dtype=torch.float64)))),
     "out sf must be contiguous float32 [2, 1, 1]"),
    # two faults at once: the checks run in the order of the arguments
    (dict(w=_Z(16), m=None), W_MSG), (dict(m=_Z(2, 8, 8), beta1=2.0), MOMENT_MSG % "m"), (dict(beta1=2.0, out=()), BETA_MSG),
]


@pytest.mark.parametrize("fault,msg", PY_FAULTS, ids=[f"{i}-{'+'.join(f)}" for i, (f, _) in enumerate(PY_FAULTS)])
def test_one_fault_gets_its_own_message(dga, fault, msg):
    with pytest.raises(dga.DGAError, match=_whole(msg)):
        dga.adamw_per_block_cast_to_fp8_transposed(**{**_valid(), **fault})


def test_tensors_that_share_memory_are_refused(dga):
    """w, m and v are updated in place: no two of w, m, v and grad may overlap, wholly or in part."""
    for a, b in (("w", "m"), ("w", "v"), ("w", "grad"), ("m", "v"), ("m", "grad"), ("v", "grad")):
        kw = _valid()
        kw[b] = kw[a]
        with pytest.raises(dga.DGAError, match=_whole(f"{a} and {b} must not share memory")):
            dga.adamw_per_block_cast_to_fp8_transposed(**kw)
    kw, both = _valid(), torch.zeros(2 * 256 + 8)
    kw["m"], kw["v"] = both[:256].view(2, 8, 16), both[8:264].view(2, 8, 16)            # v starts inside m
    with pytest.raises(dga.DGAError, match=_whole("m and v must not share memory")):
        dga.adamw_per_block_cast_to_fp8_transposed(**kw)
    kw["v"] = both[256:512].view(2, 8, 16)                                                # neighbours in one buffer are fine
    with pytest.raises(dga.DGAError, match=_whole(GUARD_MSG)):
        dga.adamw_per_block_cast_to_fp8_transposed(**kw)


def test_the_valid_arguments_reach_the_device_guard(dga):
    """... so that every case above is refused by its own check, which runs before the guard: host tensors, every valid combination of
    types, with and without rowwise and out=."""
    bf = lambda t: t.bfloat16()
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    for extra in (dict(), dict(rowwise=True), dict(use_ue8m0=True, weight_decay=0.1, eps=0.0, beta1=0.0, beta2=0.0),
                  dict(out=(u8(2, 16, 8), torch.zeros(2, 1, 1))),
                  dict(rowwise=True, out=((u8(2, 16, 8).view(torch.float8_e4m3fn), torch.zeros(2, 1, 1)), (u8(2, 8, 16), torch.zeros(2, 1, 1))))):
        for moments16 in (False, True):
            for grad16 in (False, True):
                kw = {**_valid(), **extra}
                if moments16:
                    kw["m"], kw["v"] = bf(kw["m"]), bf(kw["v"])
                if grad16:
                    kw["grad"] = bf(kw["grad"])
                with pytest.raises(dga.DGAError, match=_whole(GUARD_MSG)):
                    dga.adamw_per_block_cast_to_fp8_transposed(**kw)
    kw = {k: t[0] if isinstance(t, torch.Tensor) and t.dim() == 3 else t for k, t in _valid().items()}     # the 2-D form
    with pytest.raises(dga.DGAError, match=_whole(GUARD_MSG)):
        dga.adamw_per_block_cast_to_fp8_transposed(**kw)


def test_the_unit_compiles_without_spills_or_scratch():
    """tests/test_build.py's method on csrc/dga_adamw_cast.hip with the flags the Makefile ships it with: 2 gradient types x 2 moment types
    x rowwise = 8 builds, none with a spilled register or a byte of scratch; LDS is the existing tail's 4 floats and 16 KB tile."""
    unit = "dga_adamw_cast.hip"
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
    assert len(seen) == 3 and all(n == 8 for n in seen.values()), seen
    assert len(lds) == 8 and all("adamw_cast_128x128_transposed_kernel" in n and size == 16 + 128 * 16 * 8 for n, size in lds.items()), lds
    kinds = {re.search(r"kernelI(f|NS_7Bf16TagE)(f|NS_7Bf16TagE|S\d_)Lb([01])E", n).groups() for n in lds}
    assert len(kinds) == 8, sorted(lds)
