"""The argument checks of the `deep_gemm_cpp` bindings (csrc/python_api_amd.cpp), message by message, in the manner of
test_api_refusals.py: a table of (binding, valid arguments with one fault, the whole first line of the RuntimeError) -- torch appends a
C++ stack after it.  Two faults at once show which check runs first.  The GEMM bindings check shapes and dtypes before the device, so host
tensors are enough for them; the quantiser and combine bindings check the device first, so their rows need a GPU, and there one valid
call per binding is compared with the api.py wrapper of the same name, bit for bit.  Nothing is launched in a refused row."""
import pytest
import torch

I32, I64, F32, F64, BF16, F16, U8 = torch.int32, torch.int64, torch.float32, torch.float64, torch.bfloat16, torch.float16, torch.uint8


@pytest.fixture(scope="module")
def ext(dga):
    from deepgemm_ascend_amd import build_ext
    build_ext.build()
    from deepgemm_ascend_amd import deep_gemm_cpp
    return deep_gemm_cpp


def z(*shape, dtype=F32, device="cpu"):
    return torch.zeros(*shape, dtype=dtype, device=device)


def first_line(ext, name, valid, fault):
    """Calls the binding with the valid arguments (positional, in their order) overlaid with the fault; a fault that is no argument of
    the valid call (strict, policy, an optional tensor) goes by keyword."""
    kw = {**valid, **fault}
    args = [kw.pop(k) for k in valid]
    with pytest.raises(RuntimeError) as e:
        getattr(ext, name)(*args, **kw)
    return str(e.value).split("\n")[0]


# ---- the module surface: every exported name in its order of registration, with pybind's rendered signature ----------------------------
T, OPT, PAIR = "torch.Tensor", "torch.Tensor | None = None", "tuple[torch.Tensor, torch.Tensor]"
FP8_ARGS = f"a: {T}, sfa: {T}, b: {T}, sfb: {T}, out: {T}"
SIGNATURES = [
    ("run_mmad_custom", f"(arg0: {T}, arg1: {T}, arg2: {T}) -> None"),
    ("run_mmad_rtc", f"(arg0: {T}, arg1: {T}, arg2: {T}) -> None"),
    ("run_mmad_bench", f"(arg0: {T}, arg1: {T}, arg2: {T}, arg3: {T}) -> None"),
    ("gemm_fp8_fp8_bf16_nt", f"({FP8_ARGS}, strict: bool = False, policy: str = '') -> None"),
    ("gemm_fp8_fp8_fp32_nt", f"({FP8_ARGS}, c: {OPT}) -> None"),
    ("wgrad_gemm_fp8_fp8_fp32_nt", f"({FP8_ARGS}, c: {OPT}) -> None"),
    ("k_grouped_wgrad_gemm_fp8_fp8_fp32_nt", f"({FP8_ARGS}, ks: {T}, c: {OPT}) -> None"),
    ("m_grouped_gemm_fp8_fp8_bf16_nt_masked",
     f"({FP8_ARGS}, masked_m: {T}, expected_m: typing.SupportsInt, strict: bool = False, policy: str = '') -> None"),
    ("m_grouped_gemm_fp8_fp8_bf16_nt_contiguous", f"({FP8_ARGS}, m_indices: {T}, strict: bool = False, policy: str = '') -> None"),
    ("get_m_alignment_for_contiguous_layout", "() -> int"),
    ("per_token_cast_to_fp8", f"(arg0: {T}) -> {PAIR}"),
    ("per_block_cast_to_fp8", f"(arg0: {T}) -> {PAIR}"),
    ("silu_and_mul_per_token_cast_to_fp8", f"(x: {T}, masked_m: {OPT}) -> {PAIR}"),
    ("silu_and_mul_backward_per_token_cast_to_fp8", f"(x: {T}, grad_h: {T}, masked_m: {OPT}, grad_x_out: {OPT}) -> {PAIR}"),
    ("per_token_cast_to_fp8_transposed", f"(x: {T}, m_indices: {OPT}) -> {PAIR}"),
    ("silu_and_mul_per_token_cast_to_fp8_transposed", f"(x: {T}, m_indices: {OPT}) -> {PAIR}"),
    ("per_block_cast_to_fp8_transposed", f"(w: {T}) -> {PAIR}"),
    ("gather_per_token_cast_to_fp8_transposed", f"(src: {T}, index: {T}, index_div: typing.SupportsInt = 1, row_scale: {OPT}) -> {PAIR}"),
    ("combine_tokens", f"(src: {T}, dest: {T}, weights: {OPT}) -> {T}"),
    ("combine_tokens_weight_grad", f"(src: {T}, grad: {T}, dest: {T}) -> {T}"),
    ("abi_version", "() -> int"),
]


def test_module_surface(ext):
    assert [n for n in vars(ext) if not n.startswith("__")] == [n for n, _ in SIGNATURES]
    for name, sig in SIGNATURES:
        assert getattr(ext, name).__doc__.split("\n")[0] == name + sig
    assert ext.__doc__ == "MI355X drop-in for deep_gemm_ascend's deep_gemm_cpp (C ABI: include/dga_hip.h)"
    assert ext.abi_version() == 7


# ---- CPU: the six GEMM bindings and the policy names ----------------------------------------------------------------------------------
DEVICE = "operand must live on a HIP device (there is no CPU path)"
POLICY = "policy must be one of 'fast', 'bf16_exact', 'strict', 'fast_ue8m0', 'bf16_exact_ue8m0'"


def fp8_msg(name):
    return f"{name} must be float8_e4m3fn or uint8 bytes, got Float"


# binding -> its valid arguments on the host, the smallest shapes the checks tell apart (test_api_refusals.py): G = 2, M = 4, N = 8, K = 256
GEMM_VALID = {
    "gemm_fp8_fp8_bf16_nt": lambda: dict(a=z(4, 256, dtype=U8), sfa=z(4, 2), b=z(8, 256, dtype=U8), sfb=z(1, 2), out=z(4, 8, dtype=BF16)),
    "gemm_fp8_fp8_fp32_nt": lambda: dict(a=z(4, 256, dtype=U8), sfa=z(4, 2), b=z(8, 256, dtype=U8), sfb=z(1, 2), out=z(4, 8)),
    "wgrad_gemm_fp8_fp8_fp32_nt": lambda: dict(a=z(4, 256, dtype=U8), sfa=z(4, 2), b=z(8, 256, dtype=U8), sfb=z(8, 2), out=z(4, 8)),
    "k_grouped_wgrad_gemm_fp8_fp8_fp32_nt": lambda: dict(a=z(4, 256, dtype=U8), sfa=z(4, 2), b=z(8, 256, dtype=U8), sfb=z(8, 2), out=z(2, 4, 8),
                                                         ks=z(2, dtype=I32)),
    "m_grouped_gemm_fp8_fp8_bf16_nt_masked": lambda: dict(a=z(2, 4, 256, dtype=U8), sfa=z(2, 4, 2), b=z(2, 8, 256, dtype=U8), sfb=z(2, 1, 2),
                                                          out=z(2, 4, 8, dtype=BF16), masked_m=z(2, dtype=I32), expected_m=4),
    "m_grouped_gemm_fp8_fp8_bf16_nt_contiguous": lambda: dict(a=z(8, 256, dtype=U8), sfa=z(8, 2), b=z(2, 8, 256, dtype=U8), sfb=z(2, 1, 2),
                                                              out=z(8, 8, dtype=BF16), m_indices=z(8, dtype=I32)),
}
POLICY_ROWS = [   # policy_tag, before anything else of the three bindings that take a policy; {rank}: the binding's rank message
    (dict(policy="exact"), POLICY), (dict(policy="auto"), POLICY), (dict(strict=True, policy="exact"), POLICY),
    (dict(strict=True, policy="fast"), "strict=True contradicts policy='fast'"),
    (dict(strict=True, policy="bf16_exact_ue8m0"), "strict=True contradicts policy='bf16_exact_ue8m0'"),
    (dict(policy="exact", a=z(256, dtype=U8)), POLICY), (dict(strict=True, policy="fast", b=z(8, 256)), "strict=True contradicts policy='fast'"),
    (dict(strict=True, policy="strict", a=z(256, dtype=U8)), "{rank}"), (dict(policy="fast_ue8m0", out=z(3)), "out must have rank {r}, got 1"),
]
DENSE_ROWS = [    # the operand sequence of the three dense bindings; {dt} / {other}: the output's dtype and one that it is not, {sfb}: its shape
    (dict(a=z(256, dtype=U8)), "a [M,K], b [N,K]"), (dict(b=z(1, 8, 256, dtype=U8)), "a [M,K], b [N,K]"),
    (dict(a=z(4, 256)), fp8_msg("a")), (dict(b=z(8, 256)), fp8_msg("b")), (dict(b=z(8, 128, dtype=U8)), "b must be [8, 256], got [8, 128]"),
    (dict(out="flat"), "out must have rank 2, got 1"), (dict(out="wide"), "out must be [4, 8], got [4, 9]"),
    (dict(out="other"), "out must be {dt}, got {other}"),
    (dict(sfa=z(8)), "sfa must have rank 2, got 1"), (dict(sfa=z(4, 3)), "sfa must be [4, 2], got [4, 3]"),
    (dict(sfa=z(4, 2, dtype=F64)), "sfa must be Float, got Double"),
    (dict(sfb=z(2)), "sfb must have rank 2, got 1"), (dict(sfb=z(2, 2)), "sfb must be {sfb}, got [2, 2]"),
    (dict(sfb="f64"), "sfb must be Float, got Double"),
    # two faults: the earlier check reports
    (dict(a=z(4, 256), b=z(1, 8, 256, dtype=U8)), "a [M,K], b [N,K]"), (dict(a=z(4, 256), b=z(8, 256)), fp8_msg("a")),
    (dict(b=z(8, 128), out="wide"), fp8_msg("b")), (dict(b=z(8, 128, dtype=U8), out="wide"), "b must be [8, 256], got [8, 128]"),
    (dict(out="wide+other"), "out must be [4, 8], got [4, 9]"), (dict(out="other", sfa=z(4, 3)), "out must be {dt}, got {other}"),
    (dict(sfa=z(4, 3, dtype=F64), sfb=z(2, 2)), "sfa must be [4, 2], got [4, 3]"), (dict(sfa=z(4, 2, dtype=F64), sfb=z(2, 2)), "sfa must be Float, got Double"),
]
C_ROWS = [        # the accumuland of the two dense fp32-output bindings, after the operands
    (dict(c=z(32)), "c must have rank 2, got 1"), (dict(c=z(4, 9)), "c must be [4, 8], got [4, 9]"), (dict(c=z(4, 8, dtype=BF16)), "c must be Float, got BFloat16"),
    (dict(c=z(4, 9, dtype=BF16)), "c must be [4, 8], got [4, 9]"), (dict(sfb="f64", c=z(4, 9)), "sfb must be Float, got Double"),
    (dict(c=z(4, 8)), DEVICE),
]


def _dense(name, dt, other, sfb, more=()):
    rows, valid = [], GEMM_VALID[name]()
    for fault, msg in DENSE_ROWS + list(more):
        fault = dict(fault)
        if isinstance(fault.get("out"), str):
            fault["out"] = {"flat": z(32, dtype=valid["out"].dtype), "wide": z(4, 9, dtype=valid["out"].dtype), "other": z(4, 8, dtype=F16),
                            "wide+other": z(4, 9, dtype=F16)}[fault["out"]]
        if isinstance(fault.get("sfb"), str):
            fault["sfb"] = valid["sfb"].to(F64)
        rows.append((name, fault, msg.format(dt=dt, other=other, sfb=sfb, rank="a [M,K], b [N,K]", r=2)))
    return rows


KG, MASKED, CONTIG = "k_grouped_wgrad_gemm_fp8_fp8_fp32_nt", "m_grouped_gemm_fp8_fp8_bf16_nt_masked", "m_grouped_gemm_fp8_fp8_bf16_nt_contiguous"
KG_RANK, MASKED_RANK, CONTIG_RANK = "a [M,K_total], b [N,K_total], out [G,M,N]", "a [G,Mmax,K], b [G,N,K]", "a [Msum,K], b [G,N,K]"
GEMM_CASES = _dense("gemm_fp8_fp8_bf16_nt", "BFloat16", "Half", "[1, 2]", POLICY_ROWS) + \
    _dense("gemm_fp8_fp8_fp32_nt", "Float", "Half", "[1, 2]", C_ROWS) + _dense("wgrad_gemm_fp8_fp8_fp32_nt", "Float", "Half", "[8, 2]", C_ROWS) + [
    (KG, dict(a=z(256, dtype=U8)), KG_RANK), (KG, dict(b=z(1, 8, 256, dtype=U8)), KG_RANK), (KG, dict(out=z(4, 8)), KG_RANK),
    (KG, dict(a=z(4, 200, dtype=U8)), "K_total must be a multiple of 128"),
    (KG, dict(a=z(4, 256)), fp8_msg("a")), (KG, dict(b=z(8, 256)), fp8_msg("b")), (KG, dict(b=z(8, 128, dtype=U8)), "b must be [8, 256], got [8, 128]"),
    (KG, dict(out=z(2, 4, 9)), "out must be [2, 4, 8], got [2, 4, 9]"), (KG, dict(out=z(2, 4, 8, dtype=BF16)), "out must be Float, got BFloat16"),
    (KG, dict(sfa=z(8)), "sfa must have rank 2, got 1"), (KG, dict(sfa=z(4, 3)), "sfa must be [4, 2], got [4, 3]"),
    (KG, dict(sfa=z(4, 2, dtype=F64)), "sfa must be Float, got Double"),
    (KG, dict(sfb=z(1, 2)), "sfb must be [8, 2], got [1, 2]"), (KG, dict(sfb=z(8, 2, dtype=F64)), "sfb must be Float, got Double"),
    (KG, dict(ks=z(2, 1, dtype=I32)), "ks must have rank 1, got 2"), (KG, dict(ks=z(3, dtype=I32)), "ks must be [2], got [3]"),
    (KG, dict(ks=z(2, dtype=I64)), "ks must be Int, got Long"),
    (KG, dict(c=z(4, 8)), "c must have rank 3, got 2"), (KG, dict(c=z(2, 4, 9)), "c must be [2, 4, 8], got [2, 4, 9]"),
    (KG, dict(c=z(2, 4, 8, dtype=BF16)), "c must be Float, got BFloat16"), (KG, dict(c=z(2, 4, 8)), DEVICE),
    (KG, dict(a=z(4, 200), out=z(4, 8)), KG_RANK), (KG, dict(a=z(4, 200), b=z(8, 200)), "K_total must be a multiple of 128"),
    (KG, dict(a=z(4, 256), out=z(2, 4, 9)), fp8_msg("a")), (KG, dict(out=z(2, 4, 9, dtype=BF16), sfa=z(4, 3)), "out must be [2, 4, 8], got [2, 4, 9]"),
    (KG, dict(sfb=z(8, 2, dtype=F64), ks=z(3, dtype=I32)), "sfb must be Float, got Double"), (KG, dict(ks=z(3, dtype=I64), c=z(4, 8)), "ks must be [2], got [3]"),
    (KG, dict(ks=z(2, dtype=I64), c=z(4, 8)), "ks must be Int, got Long"),

    (MASKED, dict(a=z(8, 256, dtype=U8)), MASKED_RANK), (MASKED, dict(b=z(16, 256, dtype=U8)), MASKED_RANK),
    (MASKED, dict(a=z(2, 4, 256)), fp8_msg("a")), (MASKED, dict(b=z(2, 8, 256)), fp8_msg("b")),
    (MASKED, dict(b=z(3, 8, 256, dtype=U8)), "b must be [2, 8, 256], got [3, 8, 256]"),
    (MASKED, dict(b=z(2, 8, 128, dtype=U8)), "b must be [2, 8, 256], got [2, 8, 128]"),
    (MASKED, dict(out=z(8, 8, dtype=BF16)), "out must have rank 3, got 2"), (MASKED, dict(out=z(2, 4, 9, dtype=BF16)), "out must be [2, 4, 8], got [2, 4, 9]"),
    (MASKED, dict(out=z(2, 4, 8)), "out must be BFloat16, got Float"),
    (MASKED, dict(sfa=z(8, 2)), "sfa must have rank 3, got 2"), (MASKED, dict(sfa=z(2, 4, 3)), "sfa must be [2, 4, 2], got [2, 4, 3]"),
    (MASKED, dict(sfa=z(2, 4, 2, dtype=F64)), "sfa must be Float, got Double"),
    (MASKED, dict(sfb=z(2, 8, 2)), "sfb must be [2, 1, 2], got [2, 8, 2]"), (MASKED, dict(sfb=z(2, 1, 2, dtype=F64)), "sfb must be Float, got Double"),
    (MASKED, dict(masked_m=z(2, 1, dtype=I32)), "masked_m must have rank 1, got 2"), (MASKED, dict(masked_m=z(3, dtype=I32)), "masked_m must be [2], got [3]"),
    (MASKED, dict(masked_m=z(2, dtype=I64)), "masked_m must be Int, got Long"),
    (MASKED, dict(a=z(8, 256), out=z(2, 4, 8)), MASKED_RANK), (MASKED, dict(a=z(2, 4, 256), b=z(3, 8, 256, dtype=U8)), fp8_msg("a")),
    (MASKED, dict(out=z(2, 4, 8), sfa=z(2, 4, 3)), "out must be BFloat16, got Float"),
    (MASKED, dict(sfb=z(2, 2, 2), masked_m=z(2, dtype=I64)), "sfb must be [2, 1, 2], got [2, 2, 2]"),
    (MASKED, dict(masked_m=z(3, dtype=I64)), "masked_m must be [2], got [3]"),

    (CONTIG, dict(a=z(2, 4, 256, dtype=U8)), CONTIG_RANK), (CONTIG, dict(b=z(16, 256, dtype=U8)), CONTIG_RANK),
    (CONTIG, dict(a=z(8, 256)), fp8_msg("a")), (CONTIG, dict(b=z(2, 8, 256)), fp8_msg("b")),
    (CONTIG, dict(b=z(2, 8, 128, dtype=U8)), "b must be [2, 8, 256], got [2, 8, 128]"),
    (CONTIG, dict(out=z(64, dtype=BF16)), "out must have rank 2, got 1"), (CONTIG, dict(out=z(8, 9, dtype=BF16)), "out must be [8, 8], got [8, 9]"),
    (CONTIG, dict(out=z(8, 8)), "out must be BFloat16, got Float"),
    (CONTIG, dict(sfa=z(16)), "sfa must have rank 2, got 1"), (CONTIG, dict(sfa=z(8, 3)), "sfa must be [8, 2], got [8, 3]"),
    (CONTIG, dict(sfa=z(8, 2, dtype=F64)), "sfa must be Float, got Double"),
    (CONTIG, dict(sfb=z(1, 2)), "sfb must have rank 3, got 2"), (CONTIG, dict(sfb=z(2, 1, 3)), "sfb must be [2, 1, 2], got [2, 1, 3]"),
    (CONTIG, dict(sfb=z(2, 1, 2, dtype=F64)), "sfb must be Float, got Double"),
    (CONTIG, dict(m_indices=z(8, 1, dtype=I32)), "m_indices must have rank 1, got 2"), (CONTIG, dict(m_indices=z(7, dtype=I32)), "m_indices must be [8], got [7]"),
    (CONTIG, dict(m_indices=z(8, dtype=I64)), "m_indices must be Int, got Long"),
    (CONTIG, dict(b=z(8, 256), out=z(8, 8)), CONTIG_RANK), (CONTIG, dict(b=z(2, 8, 256), out=z(8, 8)), fp8_msg("b")),
    (CONTIG, dict(out=z(8, 9), sfa=z(8, 3)), "out must be [8, 8], got [8, 9]"), (CONTIG, dict(sfa=z(8, 3), m_indices=z(8, dtype=I64)), "sfa must be [8, 2], got [8, 3]"),
    (CONTIG, dict(sfb=z(2, 1, 2, dtype=F64), m_indices=z(7, dtype=I32)), "sfb must be Float, got Double"),
] + [(name, fault, msg.format(rank=rank, r=r)) for name, rank, r in ((MASKED, MASKED_RANK, 3), (CONTIG, CONTIG_RANK, 2))
     for fault, msg in POLICY_ROWS]


def ids(cases):
    return [f"{i}-{c[0]}-{'+'.join(c[1])}" for i, c in enumerate(cases)]


@pytest.mark.parametrize("name,fault,msg", GEMM_CASES, ids=ids(GEMM_CASES))
def test_one_fault_gets_its_own_message(ext, name, fault, msg):
    assert first_line(ext, name, GEMM_VALID[name](), fault) == msg


@pytest.mark.parametrize("name", sorted(GEMM_VALID))
def test_the_valid_arguments_reach_the_device_check(ext, name):
    """... so that every case above is refused by its own check: with everything right, the device is what is left.  Every policy name
    passes, and c may be out itself."""
    valid = GEMM_VALID[name]()
    faults = [{}]
    if "bf16" in name:
        faults += [dict(policy=p) for p in ("fast", "bf16_exact", "strict", "fast_ue8m0", "bf16_exact_ue8m0")] + [dict(strict=True), dict(strict=True, policy="strict")]
    else:
        faults += [dict(c=valid["out"])]
    for fault in faults:
        assert first_line(ext, name, valid, fault) == DEVICE


# ---- GPU: the quantiser, fused-quantiser, transposed, gather and combine bindings, whose checks sit behind the device check --------------
def g(*shape, dtype=BF16):
    return z(*shape, dtype=dtype, device="cuda")


def no_device(name):
    return f"{name} must live on a HIP device (there is no CPU path)"


def dtypes(name):
    return f"{name} must be float32 / bfloat16 / float16"


EVEN = "the last dimension of x must be even (gate and up halves)"
ONE_DEVICE = "all tensors must live on one device"
SILU, SILU_BWD = "silu_and_mul_per_token_cast_to_fp8", "silu_and_mul_backward_per_token_cast_to_fp8"
CAST_T, SILU_T, BLOCK_T = "per_token_cast_to_fp8_transposed", "silu_and_mul_per_token_cast_to_fp8_transposed", "per_block_cast_to_fp8_transposed"
GATHER, COMBINE, COMBINE_WG = "gather_per_token_cast_to_fp8_transposed", "combine_tokens", "combine_tokens_weight_grad"
MASKED_M, M_INDICES = "masked_m must be int32 [G]", "m_indices must be a contiguous int32 [T]"
GRAD_H, GRAD_X = "grad_h must be [..., H] of x's dtype", "grad_x_out must be contiguous, of x's shape and dtype"
INDEX, ROW_SCALE = "index must be a contiguous int64 [T] tensor", "row_scale must be contiguous float32 with S * index_div elements"
DEST, WEIGHTS, GRAD = "dest must be a contiguous int64 [T, k] tensor with k >= 1", "weights must be contiguous float32 [T, k]", "grad must be contiguous [T, H] of src's dtype"

# binding -> its valid arguments on the device: a few hundred elements each
GPU_VALID = {
    "per_token_cast_to_fp8": lambda: dict(x=g(3, 130)),
    "per_block_cast_to_fp8": lambda: dict(x=g(3, 130)),
    SILU: lambda: dict(x=g(3, 256)),
    SILU_BWD: lambda: dict(x=g(3, 256), grad_h=g(3, 128)),
    CAST_T: lambda: dict(x=g(3, 130)),
    SILU_T: lambda: dict(x=g(3, 256)),
    BLOCK_T: lambda: dict(w=g(3, 130)),
    GATHER: lambda: dict(src=g(4, 130), index=g(5, dtype=I64)),
    COMBINE: lambda: dict(src=g(10, 130), dest=g(5, 2, dtype=I64)),
    COMBINE_WG: lambda: dict(src=g(10, 130), grad=g(5, 130), dest=g(5, 2, dtype=I64)),
}
GPU_CASES = [row for name in ("per_token_cast_to_fp8", "per_block_cast_to_fp8") for row in [
    (name, lambda: dict(x=z(3, 130)), no_device("x")), (name, lambda: dict(x=g(3, 260)[:, :130]), "x must be contiguous"),
    (name, lambda: dict(x=g(1, 3, 130)), "x must be [rows, k]"), (name, lambda: dict(x=g(3, 130, dtype=F64)), dtypes("x")),
    (name, lambda: dict(x=z(1, 3, 130, dtype=F64)), no_device("x")), (name, lambda: dict(x=g(1, 3, 260, dtype=F64)[:, :, :130]), "x must be contiguous"),
    (name, lambda: dict(x=g(1, 3, 130, dtype=F64)), "x must be [rows, k]"),
]] + [
    (SILU, lambda: dict(x=z(3, 256)), no_device("x")), (SILU, lambda: dict(x=g(3, 512)[:, :256]), "x must be contiguous"),
    (SILU, lambda: dict(x=g(1, 3, 256)), "x must be [rows, 2H]"), (SILU, lambda: dict(masked_m=g(3, dtype=I32)), "x must be [G, Mmax, 2H] with masked_m"),
    (SILU, lambda: dict(x=g(3, 256, dtype=F64)), dtypes("x")), (SILU, lambda: dict(x=g(3, 255)), EVEN),
    (SILU, lambda: dict(x=g(2, 3, 256), masked_m=z(2, dtype=I32)), no_device("masked_m")),
    (SILU, lambda: dict(x=g(2, 3, 256), masked_m=g(4, dtype=I32)[::2]), "masked_m must be contiguous"),
    (SILU, lambda: dict(x=g(2, 3, 256), masked_m=g(2, dtype=I64)), MASKED_M), (SILU, lambda: dict(x=g(2, 3, 256), masked_m=g(3, dtype=I32)), MASKED_M),
    (SILU, lambda: dict(x=g(2, 3, 256), masked_m=g(2, 1, dtype=I32)), MASKED_M),
    (SILU, lambda: dict(x=g(1, 3, 255, dtype=F64)), "x must be [rows, 2H]"), (SILU, lambda: dict(x=g(3, 255, dtype=F64)), dtypes("x")),
    (SILU, lambda: dict(x=g(2, 3, 255), masked_m=g(2, dtype=I64)), EVEN), (SILU, lambda: dict(x=z(2, 3, 256), masked_m=z(2, dtype=I32)), no_device("x")),

    (SILU_BWD, lambda: dict(x=z(3, 256)), no_device("x")), (SILU_BWD, lambda: dict(x=g(1, 3, 256)), "x must be [rows, 2H]"),
    (SILU_BWD, lambda: dict(x=g(3, 256, dtype=F64), grad_h=g(3, 128, dtype=F64)), dtypes("x")),
    (SILU_BWD, lambda: dict(x=g(3, 128), grad_h=g(3, 64)), "the last dimension of x must be 2H with H a multiple of 128"),
    (SILU_BWD, lambda: dict(x=g(2, 3, 256), grad_h=g(2, 3, 128), masked_m=g(2, dtype=I64)), MASKED_M),
    (SILU_BWD, lambda: dict(grad_h=z(3, 128, dtype=BF16)), no_device("grad_h")), (SILU_BWD, lambda: dict(grad_h=g(3, 256)[:, :128]), "grad_h must be contiguous"),
    (SILU_BWD, lambda: dict(grad_h=g(3, 256)), GRAD_H), (SILU_BWD, lambda: dict(grad_h=g(3, 128, dtype=F16)), GRAD_H),
    (SILU_BWD, lambda: dict(grad_x_out=z(3, 256, dtype=BF16)), no_device("grad_x_out")),
    (SILU_BWD, lambda: dict(grad_x_out=g(3, 512)[:, :256]), "grad_x_out must be contiguous"),
    (SILU_BWD, lambda: dict(grad_x_out=g(3, 128)), GRAD_X), (SILU_BWD, lambda: dict(grad_x_out=g(3, 256, dtype=F32)), GRAD_X),
    (SILU_BWD, lambda: dict(x=g(2, 3, 256), masked_m=g(2, dtype=I64), grad_h=z(3, 128)), MASKED_M),
    (SILU_BWD, lambda: dict(grad_h=g(3, 256), grad_x_out=g(3, 128)), GRAD_H), (SILU_BWD, lambda: dict(grad_h=z(3, 256), grad_x_out=z(3, 128)), no_device("grad_h")),
] + [row for name, layout in ((CAST_T, "x must be a contiguous [T, H] tensor"), (SILU_T, "x must be a contiguous [T, 2H] tensor")) for row in [
    (name, lambda: dict(x=z(3, 256)), no_device("x")), (name, lambda: dict(x=g(3, 512)[:, :256]), "x must be contiguous"),
    (name, lambda: dict(x=g(1, 3, 256)), layout), (name, lambda: dict(x=g(3, 256, dtype=F64)), dtypes("x")),
    (name, lambda: dict(m_indices=z(3, dtype=I32)), no_device("m_indices")), (name, lambda: dict(m_indices=g(6, dtype=I32)[::2]), "m_indices must be contiguous"),
    (name, lambda: dict(m_indices=g(3, dtype=I64)), M_INDICES), (name, lambda: dict(m_indices=g(4, dtype=I32)), M_INDICES),
    (name, lambda: dict(m_indices=g(3, 1, dtype=I32)), M_INDICES),
    (name, lambda: dict(x=g(1, 3, 256, dtype=F64)), layout), (name, lambda: dict(x=g(3, 256, dtype=F64), m_indices=g(4, dtype=I32)), dtypes("x")),
]] + [
    (SILU_T, lambda: dict(x=g(3, 255)), EVEN), (SILU_T, lambda: dict(x=g(3, 255, dtype=F64)), dtypes("x")),
    (SILU_T, lambda: dict(x=g(3, 255), m_indices=g(4, dtype=I32)), EVEN),

    (BLOCK_T, lambda: dict(w=z(3, 130)), no_device("w")), (BLOCK_T, lambda: dict(w=g(3, 260)[:, :130]), "w must be contiguous"),
    (BLOCK_T, lambda: dict(w=g(130)), "w must be a contiguous [N, K] or [G, N, K] tensor"),
    (BLOCK_T, lambda: dict(w=g(1, 1, 3, 130)), "w must be a contiguous [N, K] or [G, N, K] tensor"), (BLOCK_T, lambda: dict(w=g(3, 130, dtype=F64)), dtypes("w")),
    (BLOCK_T, lambda: dict(w=g(130, dtype=F64)), "w must be a contiguous [N, K] or [G, N, K] tensor"),

    (GATHER, lambda: dict(src=z(4, 130)), no_device("src")), (GATHER, lambda: dict(index=z(5, dtype=I64)), no_device("index")),
    (GATHER, lambda: dict(index=g(10, dtype=I64)[::2]), "index must be contiguous"),
    (GATHER, lambda: dict(src=g(1, 4, 130)), "src must be a contiguous [S, H] tensor"), (GATHER, lambda: dict(src=g(4, 130, dtype=F64)), dtypes("src")),
    (GATHER, lambda: dict(index=g(5, dtype=I32)), INDEX), (GATHER, lambda: dict(index=g(5, 1, dtype=I64)), INDEX), (GATHER, lambda: dict(index_div=0), "index_div must be >= 1"),
    (GATHER, lambda: dict(index_div=2, row_scale=z(8)), no_device("row_scale")), (GATHER, lambda: dict(row_scale=g(8, dtype=F32)[::2]), "row_scale must be contiguous"),
    (GATHER, lambda: dict(index_div=2, row_scale=g(4, dtype=F32)), ROW_SCALE), (GATHER, lambda: dict(row_scale=g(4)), ROW_SCALE),
    (GATHER, lambda: dict(src=z(4, 130), index=z(5, dtype=I32)), no_device("src")), (GATHER, lambda: dict(src=g(4, 130, dtype=F64), index=g(5, dtype=I32)), dtypes("src")),
    (GATHER, lambda: dict(index=g(5, dtype=I32), index_div=0), INDEX), (GATHER, lambda: dict(index_div=0, row_scale=g(3, dtype=F32)), "index_div must be >= 1"),

    (COMBINE, lambda: dict(src=z(10, 130)), no_device("src")), (COMBINE, lambda: dict(dest=z(5, 2, dtype=I64)), no_device("dest")),
    (COMBINE, lambda: dict(src=g(10, 260)[:, :130]), "src must be contiguous"), (COMBINE, lambda: dict(src=g(1, 10, 130)), "src must be a contiguous [S, H] tensor"),
    (COMBINE, lambda: dict(dest=g(5, 2, dtype=I32)), DEST), (COMBINE, lambda: dict(dest=g(10, dtype=I64)), DEST), (COMBINE, lambda: dict(dest=g(5, 0, dtype=I64)), DEST),
    (COMBINE, lambda: dict(src=g(10, 130, dtype=F64)), dtypes("src")),
    (COMBINE, lambda: dict(weights=z(5, 2)), no_device("weights")), (COMBINE, lambda: dict(weights=g(5, 4, dtype=F32)[:, ::2]), "weights must be contiguous"),
    (COMBINE, lambda: dict(weights=g(5, 2)), WEIGHTS), (COMBINE, lambda: dict(weights=g(5, 3, dtype=F32)), WEIGHTS),
    (COMBINE, lambda: dict(src=g(10, 130, dtype=F64), dest=g(5, 2, dtype=I32)), DEST), (COMBINE, lambda: dict(src=g(10, 130, dtype=F64), weights=g(5, 3, dtype=F32)), dtypes("src")),
    (COMBINE, lambda: dict(dest=z(5, 2, dtype=I32), weights=z(5, 3)), no_device("dest")),

    (COMBINE_WG, lambda: dict(src=z(10, 130)), no_device("src")), (COMBINE_WG, lambda: dict(src=g(1, 10, 130)), "src must be a contiguous [S, H] tensor"),
    (COMBINE_WG, lambda: dict(dest=g(5, 2, dtype=I32)), DEST), (COMBINE_WG, lambda: dict(src=g(10, 130, dtype=F64), grad=g(5, 130, dtype=F64)), dtypes("src")),
    (COMBINE_WG, lambda: dict(grad=z(5, 130)), no_device("grad")), (COMBINE_WG, lambda: dict(grad=g(5, 260)[:, :130]), "grad must be contiguous"),
    (COMBINE_WG, lambda: dict(grad=g(4, 130)), GRAD), (COMBINE_WG, lambda: dict(grad=g(5, 131)), GRAD), (COMBINE_WG, lambda: dict(grad=g(5, 130, dtype=F16)), GRAD),
    (COMBINE_WG, lambda: dict(src=g(10, 130, dtype=F64), grad=g(4, 130)), dtypes("src")), (COMBINE_WG, lambda: dict(dest=g(5, 2, dtype=I32), grad=z(5, 130)), DEST),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,fault,msg", GPU_CASES, ids=[f"{i}-{c[0]}" for i, c in enumerate(GPU_CASES)])
def test_one_fault_behind_the_device_check_gets_its_own_message(ext, name, fault, msg):
    assert first_line(ext, name, GPU_VALID[name](), fault()) == msg


def _bits(t):
    """A tensor's bit pattern: fp8 codes as uint8, 16- and 32-bit floats as integers of their width."""
    return t.view({1: U8, 2: torch.int16, 4: I32}[t.element_size()])


def _same(got, want):
    got, want = (got, want) if isinstance(got, tuple) else ((got,), (want,))
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a.shape == b.shape and a.element_size() == b.element_size() and torch.equal(_bits(a), _bits(b))


@pytest.mark.gpu
def test_valid_calls_give_the_api_wrappers_bits(ext, dga):
    """One valid call per binding (two where an optional tensor changes the C call) against the api.py wrapper of the same name on the
    same input: the right C entry is called with the right arguments in the right order."""
    gen = torch.Generator(device="cuda").manual_seed(5)
    rnd = lambda *shape, dtype=BF16: (torch.randn(*shape, device="cuda", generator=gen) * 3).to(dtype)
    x, x3, gh, gh3, w = rnd(5, 256), rnd(2, 3, 256, dtype=F16), rnd(5, 128), rnd(2, 3, 128, dtype=F16), rnd(2, 5, 130, dtype=F32)
    masked_m = torch.tensor([2, 3], dtype=I32, device="cuda")
    m_indices = torch.tensor([0, -1, 1, 1, -1], dtype=I32, device="cuda")
    src, grad = rnd(10, 130), rnd(5, 130)
    dest = torch.tensor([[0, 9], [3, -1], [10, 4], [7, 7], [-1, -1]], dtype=I64, device="cuda")
    weights = rnd(5, 2, dtype=F32)
    index = torch.tensor([3, 19, -1, 20, 0], dtype=I64, device="cuda")     # of 10 rows * index_div 2: 20 and -1 are out of range
    row_scale = rnd(20, dtype=F32)

    u = rnd(5, 130)
    for name in ("per_token_cast_to_fp8", "per_block_cast_to_fp8"):
        _same(getattr(ext, name)(u), getattr(dga, name)(u))
    _same(ext.silu_and_mul_per_token_cast_to_fp8(x), dga.silu_and_mul_per_token_cast_to_fp8(x))
    q, sf = ext.silu_and_mul_per_token_cast_to_fp8(x3, masked_m)
    wq, wsf = dga.silu_and_mul_per_token_cast_to_fp8(x3, masked_m=masked_m)
    for i, rows in enumerate(masked_m.tolist()):                                        # the rows a mask excludes hold no value
        _same((q[i, :rows], sf[i, :rows]), (wq[i, :rows], wsf[i, :rows]))
    gx, wgx = torch.empty_like(x), torch.empty_like(x)
    _same(ext.silu_and_mul_backward_per_token_cast_to_fp8(x, gh, grad_x_out=gx), dga.silu_and_mul_backward_per_token_cast_to_fp8(x, gh, grad_x_out=wgx))
    _same(gx, wgx)
    q, sf = ext.silu_and_mul_backward_per_token_cast_to_fp8(x3, gh3, masked_m)
    wq, wsf = dga.silu_and_mul_backward_per_token_cast_to_fp8(x3, gh3, masked_m=masked_m)
    for i, rows in enumerate(masked_m.tolist()):
        _same((q[i, :rows], sf[i, :rows]), (wq[i, :rows], wsf[i, :rows]))
    for name in (CAST_T, SILU_T):
        _same(getattr(ext, name)(x), getattr(dga, name)(x))
        _same(getattr(ext, name)(x, m_indices), getattr(dga, name)(x, m_indices=m_indices))
    _same(ext.per_block_cast_to_fp8_transposed(w), dga.per_block_cast_to_fp8_transposed(w))
    _same(ext.per_block_cast_to_fp8_transposed(w[0]), dga.per_block_cast_to_fp8_transposed(w[0]))
    _same(ext.gather_per_token_cast_to_fp8_transposed(src, index.clamp(max=9)), dga.gather_per_token_cast_to_fp8_transposed(src, index.clamp(max=9)))
    _same(ext.gather_per_token_cast_to_fp8_transposed(src, index, 2, row_scale), dga.gather_per_token_cast_to_fp8_transposed(src, index, 2, row_scale))
    _same(ext.combine_tokens(src, dest), dga.combine_tokens(src, dest))
    _same(ext.combine_tokens(src, dest, weights), dga.combine_tokens(src, dest, weights))
    _same(ext.combine_tokens_weight_grad(src, grad, dest), dga.combine_tokens_weight_grad(src, grad, dest))
