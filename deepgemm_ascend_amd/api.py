"""Host-side mirror of the reference's operator API, over the C ABI (no torch types cross it).

Reference surface being mirrored (paths relative to /root/reference):
  * ``deep_gemm_ascend.run_mmad_rtc(x, y, z)`` / ``run_mmad_bench(x, y, z, params)``
    (deep_gemm_ascend/framework/deep_gemm_ascend/__init__.py:1-4,
    framework/csrc/python_api.cpp:18-35): void return, output written in place into the
    caller-allocated ``z``, current device stream.
  * the aclnn operator ``CatlassDynamicMatmul(self, mat2) -> out`` hooks
    (aclnn_catlass_dynamic_matmul/op_host/catlass_dynamic_matmul.cpp:16-80): infer_shape,
    infer_dtype, tiling.
  * new for the fp8 hot path (names from upstream DeepGEMM):
    ``gemm_fp8_fp8_bf16_nt((a, sfa), (b, sfb), out)`` and
    ``m_grouped_gemm_fp8_fp8_bf16_nt_masked((a, sfa), (b, sfb), out, masked_m, expected_m)``.

PyTorch is used only for device memory and the current stream.
"""
from __future__ import annotations

import collections
import ctypes
import os
from typing import Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import DGAError, Platform, Problem, Tiling

_FP8 = getattr(torch, "float8_e4m3fn", None)


# Host time per call matters for the short shapes of the reference's sweep list (a 64 x 32768 x 512 GEMM is 6 us of device
# time): the helpers below keep a call at a handful of Python-level operations -- no tensor views, no stream / device objects,
# no message formatting unless a check fails (12.5 -> 5 us per call, profiles/r03_host_overhead.txt; scripts/api_host_time.py times the
# wrappers of today, profiles/api_host_time.txt).
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream_of(index: int) -> int:
    """The current HIP stream of device `index` as the raw handle the C ABI takes."""
    if _raw_stream is not None:
        return _raw_stream(index)
    return torch.cuda.current_stream(index).cuda_stream


def _stream_ptr(t: torch.Tensor) -> int:
    if t.is_cuda:
        return _stream_of(t.device.index)
    return 0


def _fail(msg: str):
    # DGA_HOST_ASSERT analogue (csrc/utils/exception.hpp:26-33)
    raise DGAError(-2, "host assert", msg)


def _require(cond: bool, msg: str, *args):
    """A check with a wording of its own: `msg % args` is formed when it fails, never before."""
    if not cond:
        _fail(msg % args if args else str(msg))


def _fp8_bytes(t: torch.Tensor) -> torch.Tensor:
    """Checks that `t` holds e4m3fn bytes; the tensor itself is returned (its data pointer is what the C ABI takes)."""
    if t.dtype != _FP8 and t.dtype != torch.uint8:
        _fail(f"fp8 operand must be float8_e4m3fn or uint8 bytes, got {t.dtype}")
    return t


# What the operator wrappers share ("Adding an operator's Python wrapper"): every argument check before the device guard, every
# message built only when its check fails, outputs from torch.empty.

def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _want(t: torch.Tensor, what, dtype, shape: tuple, prefix: str = "") -> None:
    """One tensor argument: of `dtype` (one dtype, a collection of them, None = not checked), exactly `shape`, contiguous -- or
    "<prefix><what> must be contiguous <dtype> <shape>"."""
    if t.shape != shape or not t.is_contiguous() or not (
            dtype is None or t.dtype == dtype or (not isinstance(dtype, torch.dtype) and t.dtype in dtype)):
        names = "" if dtype is None else " or ".join(str(d)[6:] for d in ([dtype] if isinstance(dtype, torch.dtype) else dtype)) + " "
        _fail("%s%s must be contiguous %s%s" % (prefix, what, names, list(shape)))


def _outputs(out, specs, device, label):
    """The outputs of a wrapper, specs = ((name, dtype, shape), ...): torch.empty, or the caller's out= -- `label` is the message for a tuple
    of another length or a member that is no tensor -- with every member through _want as "out <name>".  dtype uint8 means fp8 codes: bytes
    when allocated (_as_fp8 re-tags them on the way out), uint8 or float8_e4m3fn when they are the caller's."""
    if out is None:
        return [torch.empty(shape, dtype=dtype, device=device) for _, dtype, shape in specs]
    if not isinstance(out, (tuple, list)) or len(out) != len(specs):
        _fail(str(label))
    for t in out:
        if not isinstance(t, torch.Tensor):
            _fail(str(label))
    for t, (name, dtype, shape) in zip(out, specs):
        if dtype == torch.uint8:
            _fp8_bytes(t)
            dtype = None
        _want(t, name, dtype, shape, "out ")
    return out


def _nested_out(out, rowwise: bool):
    """out= of a transposing quantiser split into (out of the transposed pair, out of the row-wise pair): (qt, sft) or, with rowwise,
    ((qt, sft), (q, sf))."""
    if out is None:
        return None, None
    _require(isinstance(out, (tuple, list)) and len(out) == 2, "out must be ((qt, sft), (q, sf))" if rowwise else "out must be (qt, sft)")
    return out if rowwise else (out, None)


def _as_fp8(q: torch.Tensor) -> torch.Tensor:
    """Code bytes as float8_e4m3fn (a view: the caller's own tensor when it already is)."""
    return q.view(_FP8) if q.dtype == torch.uint8 else q


def _row_masks(masked_m: Optional[torch.Tensor], m_indices: Optional[torch.Tensor], groups: int, rows: int) -> None:
    """The row masks of the quantisers: masked_m int32 [groups], m_indices int32 [rows]."""
    if masked_m is not None:
        _require(masked_m.dtype == torch.int32 and tuple(masked_m.shape) == (groups,) and masked_m.is_contiguous(),
                 "masked_m must be a contiguous int32 [%d]", groups)
    if m_indices is not None:
        _require(m_indices.dtype == torch.int32 and tuple(m_indices.shape) == (rows,) and m_indices.is_contiguous(),
                 "m_indices must be a contiguous int32 [%d]", rows)


_WORKSPACES = {}   # (kind, device index, stream handle) -> uint8 tensor
_RETIRED = []      # outgrown buffers: a HIP graph captured earlier may still hold their address, so they stay alive


def _scratch(kind: str, device, need: int, stream: Optional[int] = None) -> Tuple[Optional[int], int]:
    """Device scratch, one grow-only buffer per (kind, device, stream): two GEMMs issued on different streams never
    share split-K slabs or padded operand copies, and the capture stream of a HIP graph has a buffer of its own.  A
    buffer that has to grow is replaced, not freed (a captured graph may replay into the old one); growth is geometric
    so that few are ever retired.  The callee never allocates (the op runtime hands the workspace in)."""
    if need == 0:
        return None, 0
    dev = device if isinstance(device, torch.device) else torch.device(device)
    index = dev.index if dev.index is not None else torch.cuda.current_device()
    key = (kind, index, _stream_of(index) if stream is None else stream)
    buf = _WORKSPACES.get(key)
    if buf is None or buf.numel() < need:
        if buf is not None:
            _RETIRED.append(buf)
            need = max(need, buf.numel() * 3 // 2)
        buf = torch.empty((need,), dtype=torch.uint8, device=dev)
        _WORKSPACES[key] = buf
    return buf.data_ptr(), buf.numel()


def release_scratch(retired_only: bool = True) -> int:
    """Frees the outgrown scratch buffers (`retired_only`) or every scratch buffer of the process; returns the bytes released.
    Worst case held per (device, stream): the selector bounds split-K slabs to 256 MiB (dga_tiling.cpp kMaxSlabBytes) and the
    odd-K padding copies to the operands' size, and growth is geometric, so at most ~1.5x the largest workspace ever asked for
    on that stream -- plus the retired ones until this is called.  Only call it when no captured HIP graph that ran a GEMM
    through this module will be replayed again (a graph holds the address of the buffer it was captured with)."""
    n = sum(b.numel() for b in _RETIRED)
    _RETIRED.clear()
    if not retired_only:
        n += sum(b.numel() for b in _WORKSPACES.values())
        _WORKSPACES.clear()
    return int(n)


_WS_BYTES = {}     # bytes of a Tiling -> dga_workspace_bytes of it (pure function of the struct)


def _workspace(t: Tiling, device, stream: Optional[int] = None) -> Tuple[Optional[int], int]:
    """Split-K slabs / odd-K padding of the fp8 kernels, sized by dga_workspace_bytes."""
    key = bytes(t)
    need = _WS_BYTES.get(key)
    if need is None:
        if len(_WS_BYTES) > 4096:
            _WS_BYTES.clear()
        need = _WS_BYTES[key] = workspace_bytes(t)
    return _scratch("fp8", device, need, stream)


def _mmad_workspace(batch, m, n, k, x) -> Tuple[Optional[int], int]:
    return _scratch("mmad", x.device, int(_lib.lib().dga_mmad_workspace_bytes(batch, m, n, k, x.data_ptr())))


POLICY_PLAIN, POLICY_PINGPONG, POLICY_CONTINUOUS, POLICY_STRICT, POLICY_LOADER_WAVES, POLICY_PERSISTENT = 0, 1, 2, 3, 4, 5
POLICY_CONTINUOUS_PERSISTENT = 6
POLICY_BF16_EXACT = 7

# The three arithmetic policies of the fp8 GEMMs (README.md "Numerics"; include/dga_hip.h, dispatchPolicyTag):
#   "fast"        the fp8 matrix instruction (whatever schedule the tiling names) -- the throughput form
#   "bf16_exact"  e4m3 -> bf16 in registers (exact), bf16 matrix instruction: exact products, fp32-class block sums
#   "strict"      fp32-input matrix instruction in the oracle's own order: bit-identical to the reference CPU path
#   "auto"        "bf16_exact" where it is nearly free -- the decode rows the one-launch workgroup split-K takes (the weights are
#                 streamed, the exact arithmetic rides along: +2..+15 %) -- and "fast" everywhere else; dense calls without an
#                 explicit tiling only.
# A call that names neither a policy nor a tiling runs $DGA_DEFAULT_POLICY, default "bf16_exact": the fastest policy whose outputs
# stay inside the operator's contract (within 2 bf16 ULP of the fp32-accumulate CPU path; <= 1e-5 of the outputs of a 4096^3
# problem differ by more, each a sum that cancels to the level of the fp32 reference's own rounding).  "fast" is an opt-in: the
# fp8 matrix instruction drops product bits ~13 below each octet's largest (6.7e-4 of the same outputs beyond 2 ULP).  An explicit
# tiling_ keeps the arithmetic its dispatchPolicyTag names.
#   "fast_ue8m0"  "fast" for scale tensors whose values are exact powers of two (UE8M0 scales: per_token_cast_to_fp8(...,
#                 use_ue8m0=True), upstream DeepGEMM's convention for hardware-scaled MFMAs): the scales ride in the matrix
#                 instruction's E8M0 operands and the MFMA accumulates in place -- no promotion on the vector pipe.  Same outputs
#                 as "fast" up to fp32 rounding order; a scale that is not a power of two is read as its exponent alone.
#   "bf16_exact_ue8m0"  "bf16_exact" for power-of-two scales: the scales are folded into the exact e4m3 -> bf16 conversions and the
#                 bf16 matrix instruction accumulates in place -- the in-contract arithmetic without its promotion.
ARITHMETIC_POLICIES = {"fast": None, "bf16_exact": POLICY_BF16_EXACT, "strict": POLICY_STRICT, "auto": None, "fast_ue8m0": None,
                       "bf16_exact_ue8m0": POLICY_BF16_EXACT | 16}
POLICY_UE8M0_SCALES = 16      # DGA_POLICY_UE8M0_SCALES: a flag beside the fast-path schedules


def default_policy() -> str:
    """$DGA_DEFAULT_POLICY as the C library parsed and validated it (dga_default_policy: once per process, the same answer for every
    front end); a value that names no policy raises instead of silently changing the arithmetic."""
    buf = ctypes.create_string_buffer(32)
    rc = _lib.lib().dga_default_policy(buf, 32)
    if rc:
        _fail(f"$DGA_DEFAULT_POLICY={os.environ.get('DGA_DEFAULT_POLICY')!r} names no arithmetic policy (one of {sorted(ARITHMETIC_POLICIES)})")
    return buf.value.decode()


class _DefaultPolicy:
    """Lazy `_DEFAULT_POLICY` (the library need not be loaded at import time): str(...) / == compare against the parsed name."""
    def __str__(self):
        return default_policy()

    def __eq__(self, other):
        return default_policy() == other

    def __hash__(self):
        return hash(default_policy())


_DEFAULT_POLICY = _DefaultPolicy()


def _with_policy(t: Tiling, strict: bool, policy: Optional[str] = None) -> Tiling:
    """A copy of the tiling with the arithmetic policy's dispatchPolicyTag (strict=True is policy="strict")."""
    if policy is not None and policy not in ARITHMETIC_POLICIES:
        _fail(f"policy must be one of {sorted(ARITHMETIC_POLICIES)}")
    _require(not (strict and policy not in (None, "strict")), "strict=True contradicts policy=%r", policy)
    tag = POLICY_STRICT if strict else ARITHMETIC_POLICIES.get(policy)
    if policy == "fast_ue8m0" and not strict:
        _require((t.dispatchPolicyTag & 15) not in (POLICY_STRICT, POLICY_BF16_EXACT), "policy='fast_ue8m0' needs a fast-path tiling")
        tag = (t.dispatchPolicyTag & 15) | POLICY_UE8M0_SCALES
    if tag is None or t.dispatchPolicyTag == tag:
        return t
    c = Tiling()
    ctypes.memmove(ctypes.byref(c), ctypes.byref(t), ctypes.sizeof(Tiling))
    c.dispatchPolicyTag = tag
    return c


class _NoGuard:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NO_GUARD = _NoGuard()


def _device_guard(*ts: torch.Tensor):
    """All tensors on one HIP device; that device current for the call (nothing to do when it already is)."""
    dev = ts[0].device
    for t in ts:
        if t.device != dev:
            _fail("all tensors must live on one device")
    if dev.type != "cuda":
        _fail("tensors must be on a HIP device (there is no CPU path)")
    return _NO_GUARD if torch.cuda.current_device() == dev.index else torch.cuda.device(dev)


def _launch(name: str, tensors, call, sync: bool = False) -> None:
    """The tail of a wrapper whose checks have passed: the device guard over `tensors` (None for an absent optional one), rc = call(library,
    stream) on the current stream of the first tensor's device -- scratch is allocated in there, behind the guard --, the status check, and
    the synchronise sync=True asks for.  (The dense and grouped GEMM entries keep this inline: a closure per call is host time there.)"""
    first = tensors[0]
    with _device_guard(*[t for t in tensors if t is not None]):
        rc = call(_lib.lib(), _stream_ptr(first))
        if rc:
            _lib.check(rc, name)
        if sync:
            torch.cuda.current_stream(first.device).synchronize()


_PLANS = {}        # what a GEMM call without an explicit tiling resolves to: key -> Tiling (with the policy's tag)


def _plans_clear():
    _PLANS.clear()


def _planned(index: int, m: int, n: int, k: int, groups: int, expected_m: int, contiguous: bool, strict: bool,
             policy: Optional[str]) -> Tiling:
    """tiling(...) + the arithmetic policy's tag, remembered per problem: the C side's (m,n,k) cache answers the same question, but
    through two ctypes calls and a struct copy per GEMM.  Dropped whenever the cache file, the cache or the predictor changes."""
    if policy is None and not strict:
        policy = default_policy()
    key = (index, m, n, k, groups, expected_m, contiguous, strict, policy)
    t = _PLANS.get(key)
    if t is None:
        if policy is not None and policy not in ARITHMETIC_POLICIES:
            _fail(f"policy (or $DGA_DEFAULT_POLICY) must be one of {sorted(ARITHMETIC_POLICIES)}")
        if policy == "auto":   # the exact arithmetic where the decode kernel carries it, the fast path elsewhere
            _require(not strict, "strict=True contradicts policy='auto'")
            t = tiling(m, n, k, policy="bf16_exact") if groups == 1 and not contiguous else None
            if t is None or t.kernelSerial != 6:   # DGA_KERNEL_SPLITK_WORKGROUP
                t = tiling(m, n, k, groups=groups, expected_m=expected_m, contiguous=contiguous)
        else:
            t = tiling(m, n, k, groups=groups, expected_m=expected_m, contiguous=contiguous,
                       policy="bf16_exact" if policy in ("bf16_exact", "bf16_exact_ue8m0") else None)
            t = _with_policy(t, strict, policy)
        _remember(key, t)
    return t


def _remember(key, t: Tiling) -> Tiling:
    """A plan into _PLANS, on a miss (the hit is the caller's own _PLANS.get: a call that finds its plan pays nothing for this).  The dict
    is emptied rather than grown past 4096 plans."""
    if len(_PLANS) > 4096:
        _PLANS.clear()
    _PLANS[key] = t
    return t


# ----------------------------------------------------------------------------- operator hooks

def infer_shape(self_shape: Sequence[int], mat2_shape: Sequence[int]) -> Tuple[int, int]:
    """InferShape hook (catlass_dynamic_matmul.cpp:16-35)."""
    a = (ctypes.c_int64 * len(self_shape))(*self_shape)
    b = (ctypes.c_int64 * len(mat2_shape))(*mat2_shape)
    out = (ctypes.c_int64 * 2)()
    _lib.check(_lib.lib().dga_infer_shape(a, len(self_shape), b, len(mat2_shape), out), "infer_shape")
    return int(out[0]), int(out[1])


def infer_dtype(self_dtype: int, mat2_dtype: int) -> int:
    """InferDataType hook (catlass_dynamic_matmul.cpp:37-46)."""
    out = ctypes.c_int(0)
    _lib.check(_lib.lib().dga_infer_dtype(self_dtype, mat2_dtype, ctypes.byref(out)), "infer_dtype")
    return out.value


def _problem(m, n, k, groups=1, expected_m=0, dtype=_lib.DT_FP8_E4M3FN, contiguous=False) -> Problem:
    return Problem(m, n, k, groups, expected_m, _lib.LAYOUT_ROW_MAJOR, _lib.LAYOUT_COLUMN_MAJOR,
                   _lib.LAYOUT_ROW_MAJOR, dtype, _lib.PROBLEM_CONTIGUOUS_M if contiguous else 0)


def tiling(m: int, n: int, k: int, groups: int = 1, expected_m: int = 0, contiguous: bool = False,
           policy: Optional[str] = None) -> Tiling:
    """TilingFunc hook with the (m,n,k) cache (catlass_dynamic_matmul_tiling.cpp:77-122).
    contiguous=True: the contiguous-grouped layout (m = total rows, groups = number of B matrices).
    policy="bf16_exact": that policy's own tile / split-K pick (dga_tiling_bf16_exact); "strict": the tag alone."""
    t = Tiling()
    p = _problem(m, n, k, groups, expected_m, contiguous=contiguous)
    if policy == "bf16_exact":
        _lib.check(_lib.lib().dga_tiling_bf16_exact(ctypes.byref(p), ctypes.byref(t)), "tiling_bf16_exact")
        return t
    _lib.check(_lib.lib().dga_tiling(ctypes.byref(p), ctypes.byref(t)), "tiling")
    return _with_policy(t, False, policy) if policy else t


def _default_tiling(entry: str, p: Problem) -> Tiling:
    """The C entry dga_<entry>(problem, tiling) behind tiling_fp32_out, tiling_wgrad and tiling_k_grouped_wgrad (tiling() itself runs on
    every call of the contiguous grouped GEMM and stays inline)."""
    t = Tiling()
    _lib.check(getattr(_lib.lib(), "dga_" + entry)(ctypes.byref(p), ctypes.byref(t)), entry)
    return t


def tiling_check(t: Tiling) -> int:
    """dga_tiling_check: 0 if the compiled menu holds this tiling, else the (negative) status every fp8 GEMM entry returns for
    it before any launch (the TilingFunc's GRAPH_FAILED, catlass_dynamic_matmul_tiling.cpp:86-100)."""
    return int(_lib.lib().dga_tiling_check(ctypes.byref(t)))


def select_kernel(m: int, n: int, k: int, platform: Optional[Platform] = None, groups: int = 1,
                  expected_m: int = 0) -> Tiling:
    """SelectKernel without the cache (select_kernel.cpp:333-369); platform None = MI355X."""
    t = Tiling()
    p = _problem(m, n, k, groups, expected_m)
    pp = ctypes.byref(platform) if platform is not None else None
    _lib.check(_lib.lib().dga_select_kernel(ctypes.byref(p), pp, ctypes.byref(t)), "select_kernel")
    return t


def predictor_load(path: Optional[str] = None) -> None:
    """Load a predictor weights file (None = tuned/predictor_mi355x.txt next to the library)."""
    _plans_clear()
    _lib.check(_lib.lib().dga_predictor_load(path.encode() if path else None), "predictor_load")


def predictor_unload() -> None:
    _plans_clear()
    _lib.lib().dga_predictor_unload()


def predictor_loaded() -> bool:
    return bool(_lib.lib().dga_predictor_loaded())


def predict_time_us(m: int, n: int, k: int, t: Tiling) -> float:
    """The model's time for running (m,n,k) with tiling t (TilingPredictor.predict_batch for one row)."""
    us = ctypes.c_float(0)
    p = _problem(m, n, k)
    _lib.check(_lib.lib().dga_predict_time_us(ctypes.byref(p), ctypes.byref(t), ctypes.byref(us)), "predict_time_us")
    return us.value


SELECTION_METHODS = {"greedy": 0, "topk_median": 1, "topk_dbscan": 2}   # get_best_config.py:431-525


def select_kernel_with_predictor(m: int, n: int, k: int, method: str = "greedy", topk: int = 10):
    """SelectKernelWithPredictor: (tiling, predicted_us, native_us); falls back to the heuristic tiling when the model
    is absent, the candidate list is short or the promised gain is below the threshold (get_best_config.py:587-621).  `method` /
    `topk`: the reference predictor's selection strategy (select_tiling_strategy, get_best_config.py:431-525)."""
    _require(method in SELECTION_METHODS, "method: one of %s", sorted(SELECTION_METHODS))
    t = Tiling()
    p = _problem(m, n, k)
    a, b = ctypes.c_float(0), ctypes.c_float(0)
    _lib.check(_lib.lib().dga_select_kernel_with_predictor_ex(ctypes.byref(p), ctypes.byref(t), ctypes.byref(a), ctypes.byref(b),
                                                              SELECTION_METHODS[method], int(topk)), "select_kernel_with_predictor")
    return t, a.value, b.value


def select_tiling_strategy(preds, tiles, method: str = "greedy", topk: int = 10, dbscan_eps: float = 0.8, dbscan_min_samples: int = 2,
                           random_state: int = 0):
    """select_tiling_strategy (get_best_config.py:431-525) on predicted times `preds` [count] and tile triples `tiles` [count][3]
    (mTile, nTile, kTile): returns (picked index, members of the winning cluster -- topk_dbscan only, else []).  The reference draws a
    random member of that cluster; this library takes its fastest (random_state = 0) or member random_state % size."""
    import numpy as np
    _require(method in SELECTION_METHODS, "method: one of %s", sorted(SELECTION_METHODS))
    pr = np.ascontiguousarray(preds, dtype=np.float32)
    tl = np.ascontiguousarray(tiles, dtype=np.int32).reshape(-1, 3) if tiles is not None else np.zeros((pr.size, 3), np.int32)
    _require(tl.shape[0] == pr.size, "one tile triple per prediction")
    picked, cnt = ctypes.c_int(-1), ctypes.c_int(0)
    members = (ctypes.c_int * max(1, pr.size))()
    _lib.check(_lib.lib().dga_select_tiling_strategy(pr.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                                     tl.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), int(pr.size),
                                                     SELECTION_METHODS[method], int(topk), float(dbscan_eps), int(dbscan_min_samples),
                                                     int(random_state), ctypes.byref(picked), members, ctypes.byref(cnt)),
               "select_tiling_strategy")
    return picked.value, [members[i] for i in range(cnt.value)]


def platform_mi355x() -> Platform:
    p = Platform()
    _lib.lib().dga_platform_mi355x(ctypes.byref(p))
    return p


def platform_ascend910b(core_num: int = 24) -> Platform:
    p = Platform()
    _lib.lib().dga_platform_ascend910b(ctypes.byref(p), core_num)
    return p


def workspace_bytes(t: Tiling) -> int:
    return int(_lib.lib().dga_workspace_bytes(ctypes.byref(t)))


def tiling_cache_open(path: Optional[str]):
    _plans_clear()
    _lib.check(_lib.lib().dga_tiling_cache_open(path.encode() if path else None), "tiling_cache_open")


def tiling_cache_clear():
    _plans_clear()
    _lib.lib().dga_tiling_cache_clear()


def tiling_cache_size() -> int:
    return int(_lib.lib().dga_tiling_cache_size())


# ----------------------------------------------------------------------------- 28-int Config

def get_best_config(batch: int, m: int, n: int, k: int) -> list:
    out = (ctypes.c_uint32 * 28)()
    _lib.check(_lib.lib().dga_get_best_config(batch, m, n, k, out), "get_best_config")
    return list(out)


def get_bench_config(m, n, k, m_sections, n_sections, m_sec_o_blocks, n_sec_o_blocks, k_o_iter_blocks,
                     db_o_blocks) -> list:
    out = (ctypes.c_uint32 * 28)()
    _lib.check(_lib.lib().dga_get_bench_config(m, n, k, m_sections, n_sections, m_sec_o_blocks, n_sec_o_blocks,
                                               k_o_iter_blocks, db_o_blocks, out), "get_bench_config")
    return list(out)


CONFIG_FIELDS = ("k_iters batch m n k m_sections n_sections m_blocks n_blocks k_blocks m_sc_blocks n_sc_blocks "
                 "m_sec_o_blocks n_sec_o_blocks k_o_iter_blocks db_o_blocks m_o_fix n_o_fix k_o_fix db_o_num "
                 "m_parts n_parts r_m_parts r_n_parts r_m_blocks r_n_blocks r_k_blocks r_db_num").split()


def bbit_params(m, n, k, m_sections, n_sections, m_sec_o_blocks, n_sec_o_blocks, k_o_iter_blocks, db_o_blocks):
    out = (ctypes.c_uint32 * 28)()
    _lib.check(_lib.lib().dga_bbit_params(m, n, k, m_sections, n_sections, m_sec_o_blocks, n_sec_o_blocks,
                                          k_o_iter_blocks, db_o_blocks, out), "bbit_params")
    return list(out)


def bench_params_fill(m: int, n: int, k: int, params6: Sequence[int]) -> list:
    arr = (ctypes.c_int32 * 28)(*list(params6)[:6], *([0] * 22))
    _lib.check(_lib.lib().dga_bench_params_fill(m, n, k, arr), "bench_params_fill")
    return list(arr)


# ----------------------------------------------------------------------------- the hot path

def _dense_fp8_operands(a, sfa, b, sfb, out, out_dtype, out_name: str, sfb_rows: bool = False):
    """The dense fp8 GEMM's argument checks (shapes, dtypes, strides); (m, n, k, lda, ldb).  sfb_rows: sfb is [N, KB] (one scale per
    row of B), not [ceil(N/128), KB]."""
    _fp8_bytes(a); _fp8_bytes(b)
    if a.dim() != 2 or b.dim() != 2 or out.dim() != 2:
        _fail("rank must be 2")
    m, k = a.shape
    n, k2 = b.shape
    if k != k2:
        _fail("self dimk is not equal with mat2 dimk")
    if out.shape[0] != m or out.shape[1] != n:
        _fail(f"out must be [{m},{n}]")
    if out.dtype != out_dtype:
        _fail(f"out must be {out_name}")
    kb, nb = (k + 127) // 128, (n if sfb_rows else (n + 127) // 128)
    if sfa.dtype != torch.float32 or sfb.dtype != torch.float32:
        _fail("scales must be float32")
    if sfa.dim() != 2 or sfa.shape[0] != m or sfa.shape[1] != kb:
        _fail(f"sfa must be [{m},{kb}]")
    if sfb.dim() != 2 or sfb.shape[0] != nb or sfb.shape[1] != kb:
        _fail(f"sfb must be [{nb},{kb}]")
    if not (sfa.is_contiguous() and sfb.is_contiguous() and out.is_contiguous()):
        _fail("scales and out must be contiguous")
    if (k > 1 and (a.stride(1) != 1 or b.stride(1) != 1)) or (m > 1 and a.stride(0) < k) or (n > 1 and b.stride(0) < k):
        _fail("operands must be row-major with unit inner stride (row-strided views are accepted)")
    lda = a.stride(0) if m > 1 else k
    ldb = b.stride(0) if n > 1 else k
    return m, n, k, lda, ldb


def _zero_padded_flags(a: torch.Tensor, b: torch.Tensor, zero_padded: Optional[Tuple[bool, bool]]) -> int:
    """The ROWS_*_ZERO_PADDED flags of a call on row-strided operands: the caller's promise, else the mark the aligned_rows quantisers leave."""
    if zero_padded is None:
        zero_padded = (getattr(a, "_dga_zero_padded", False), getattr(b, "_dga_zero_padded", False))
    return (_lib.ROWS_A_ZERO_PADDED if zero_padded[0] else 0) | (_lib.ROWS_B_ZERO_PADDED if zero_padded[1] else 0)


def _accumuland(c: torch.Tensor, shape: tuple, out: torch.Tensor) -> None:
    """The c of the fp32-output GEMMs: contiguous float32 of out's `shape`, and out itself or clear of it."""
    if c.dtype != torch.float32 or tuple(c.shape) != shape or not c.is_contiguous():
        if len(shape) == 3:    # (the k-grouped entry words it in one message, the dense entries fault by fault)
            _fail("c must be a contiguous float32 %s" % list(shape))
        _fail("c must be float32" if c.dtype != torch.float32 else "c must be contiguous" if tuple(c.shape) == shape else "c must be [%d,%d]" % shape)
    lo, hi, nbytes = c.data_ptr(), out.data_ptr(), 4 * out.numel()
    if lo != hi and c.device == out.device and lo < hi + nbytes and hi < lo + nbytes:
        _fail("c must be out itself or not overlap it")


def gemm_fp8_fp8_bf16_nt(lhs: Tuple[torch.Tensor, torch.Tensor], rhs: Tuple[torch.Tensor, torch.Tensor],
                         out: torch.Tensor, tiling_: Optional[Tiling] = None, sync: bool = False,
                         strict: bool = False, policy: Optional[str] = None,
                         zero_padded: Optional[Tuple[bool, bool]] = None) -> None:
    """out[M,N] (bf16, written in place) = (A[M,K] fp8, sfa[M,ceil(K/128)]) x (B[N,K] fp8, sfb[ceil(N/128),ceil(K/128)])^T.

    A and B may be row-strided views (unit inner stride; a row stride that is K or a multiple of 16 bytes): rows that start on
    16-byte boundaries are read where they lie.  For K % 16 != 0 that also needs zeros from byte K to the next 16-byte boundary
    of each row -- true of what per_token_cast_to_fp8 / per_block_cast_to_fp8(..., aligned_rows=True) return (they mark their
    results), or promised by the caller with zero_padded=(a_is, b_is); an operand without the promise is re-laid out by the
    padding pass, alone (dga_gemm_fp8_fp8_bf16_nt_strided).

    strict=True (= policy="strict") runs the exact-arithmetic kernel (dispatchPolicyTag 3): fp32 products and sums in the
    reference CPU path's own order, bit-identical to the oracle, at the fp32 matrix rate.  policy="bf16_exact"
    (dispatchPolicyTag 7) up-converts the bytes to bf16 in registers and sums on the bf16 matrix instruction: exact products,
    fp32-class sums, about half the fast path's rate.  The default fp8-MFMA path ("fast") differs from both on
    cancellation-dominated outputs (README.md, "Numerics").

    Asynchronous on the current stream (the reference syncs on every call, gemm.hpp:110;
    pass sync=True for that behaviour)."""
    a, sfa = lhs
    b, sfb = rhs
    m, n, k, lda, ldb = _dense_fp8_operands(a, sfa, b, sfb, out, torch.bfloat16, "bfloat16")
    strided = lda != k or ldb != k
    with _device_guard(a, b, sfa, sfb, out):
        index = out.device.index
        if tiling_ is None:
            tiling_ = _planned(index, m, n, k, 1, 0, False, strict, policy)
        else:
            tiling_ = _with_policy(tiling_, strict, policy)
        stream = _stream_of(index)
        ws_ptr, ws_bytes = _workspace(tiling_, out.device, stream)
        if strided:
            flags = _zero_padded_flags(a, b, zero_padded)
            rc = _lib.lib().dga_gemm_fp8_fp8_bf16_nt_strided(a.data_ptr(), lda, sfa.data_ptr(), b.data_ptr(), ldb, sfb.data_ptr(),
                                                             out.data_ptr(), m, n, k, flags, ctypes.byref(tiling_), ws_ptr,
                                                             ws_bytes, stream)
        else:
            rc = _lib.lib().dga_gemm_fp8_fp8_bf16_nt(a.data_ptr(), sfa.data_ptr(), b.data_ptr(), sfb.data_ptr(),
                                                     out.data_ptr(), m, n, k, ctypes.byref(tiling_), ws_ptr, ws_bytes, stream)
        if rc:
            _lib.check(rc, "gemm_fp8_fp8_bf16_nt")
        if sync:
            torch.cuda.current_stream(out.device).synchronize()


def tiling_fp32_out(m: int, n: int, k: int) -> Tiling:
    """dga_tiling_fp32_out: the default tiling of gemm_fp8_fp8_fp32_nt -- the bf16-exact pick, with names of builds that have no fp32
    epilogue mapped onto the in-register build of the same tile; the strict tag under $DGA_DEFAULT_POLICY=strict."""
    return _default_tiling("tiling_fp32_out", _problem(m, n, k, 1, 0))


def tiling_check_fp32_out(t: Tiling) -> int:
    """dga_tiling_check_fp32_out: 0 if gemm_fp8_fp8_fp32_nt takes this tiling, else the status it returns before any launch."""
    return int(_lib.lib().dga_tiling_check_fp32_out(ctypes.byref(t)))


_FP32_OUT_POLICIES = ("bf16_exact", "strict")   # the arithmetic policies with an fp32 epilogue


def gemm_fp8_fp8_fp32_nt(lhs: Tuple[torch.Tensor, torch.Tensor], rhs: Tuple[torch.Tensor, torch.Tensor], out: torch.Tensor,
                         c: Optional[torch.Tensor] = None, tiling_: Optional[Tiling] = None, sync: bool = False,
                         strict: bool = False, policy: Optional[str] = None,
                         zero_padded: Optional[Tuple[bool, bool]] = None) -> None:
    """out[M,N] (fp32, written in place) = c[M,N] (fp32, optional) + (A[M,K] fp8, sfa) x (B[N,K] fp8, sfb)^T -- the fp32 result the
    reference's run_mmad_rtc writes (python_api.cpp:18), with upstream DeepGEMM's fp32-output accumulation.

    Operands, scales, row-strided views and zero_padded exactly as in gemm_fp8_fp8_bf16_nt.  out and c: contiguous [M,N] float32 on
    the operands' device; c may be out itself (in-place accumulation), a c that partially overlaps out is refused.  c is added once
    to the finished product, out = fl(acc + c); c=None writes every element of out without reading it.

    Arithmetic: "bf16_exact" (the default: the accumulator gemm_fp8_fp8_bf16_nt rounds, bit for bit) or "strict" (strict=True: the
    oracle's fp32 result, bit for bit).  "fast", "auto" and the _ue8m0 policies have no fp32 epilogue and raise; a process default
    ($DGA_DEFAULT_POLICY) of "strict" gives strict, any other gives bf16_exact."""
    _fp32_out_call("gemm_fp8_fp8_fp32_nt", lhs, rhs, out, c, tiling_, sync, strict, policy, zero_padded, sfb_rows=False)


def tiling_wgrad(m: int, n: int, k: int) -> Tiling:
    """dga_tiling_wgrad: the default tiling of wgrad_gemm_fp8_fp8_fp32_nt -- tiling_fp32_out's pick, with the builds that have no
    per-row-sfb form (workgroup split-K and its decode / register builds, one-launch Stream-K) mapped onto the same tile's two-launch
    split-K or plain raster; the strict tag under $DGA_DEFAULT_POLICY=strict."""
    return _default_tiling("tiling_wgrad", _problem(m, n, k, 1, 0))


def tiling_check_wgrad(t: Tiling) -> int:
    """dga_tiling_check_wgrad: 0 if wgrad_gemm_fp8_fp8_fp32_nt takes this tiling, else the status it returns before any launch."""
    return int(_lib.lib().dga_tiling_check_wgrad(ctypes.byref(t)))


def wgrad_gemm_fp8_fp8_fp32_nt(lhs: Tuple[torch.Tensor, torch.Tensor], rhs: Tuple[torch.Tensor, torch.Tensor], out: torch.Tensor,
                               c: Optional[torch.Tensor] = None, tiling_: Optional[Tiling] = None, sync: bool = False,
                               strict: bool = False, policy: Optional[str] = None,
                               zero_padded: Optional[Tuple[bool, bool]] = None) -> None:
    """Upstream DeepGEMM's weight-gradient GEMM: out[M,N] (fp32, written in place) = c[M,N] (fp32, optional) + (A[M,K] fp8,
    sfa[M,ceil(K/128)]) x (B[N,K] fp8, sfb[N,ceil(K/128)])^T, with per-1x128 scales on BOTH operands -- one sfb per row of B per
    128-wide k block, what per_token_cast_to_fp8 returns for an activation.  For dW = dY^T . X: lhs = per_token_cast_to_fp8(dY^T),
    rhs = per_token_cast_to_fp8(X^T), K = tokens, c=out to accumulate micro-batches.

    Everything else -- row-strided views, zero_padded, c, in-place use, policies ("bf16_exact" default, "strict") -- is
    gemm_fp8_fp8_fp32_nt's; "fast", "auto" and the _ue8m0 policies raise.  The promotion scale of an output is fl(sfa[m] * sfb[n]):
    with every row of a 128-row block of B on one scale the result is gemm_fp8_fp8_fp32_nt's on the same tiling, bit for bit."""
    _fp32_out_call("wgrad_gemm_fp8_fp8_fp32_nt", lhs, rhs, out, c, tiling_, sync, strict, policy, zero_padded, sfb_rows=True)


def _planned_fp32_out(index: int, m: int, n: int, k: int, strict: bool, policy: Optional[str], sfb_rows: bool) -> Tiling:
    """What gemm_fp8_fp8_fp32_nt (sfb_rows=False) or wgrad_gemm_fp8_fp8_fp32_nt (True) runs without an explicit tiling, remembered
    per problem as _planned does."""
    # (the output kind and the scale layout are part of the key: never a bf16 call's plan, nor the other fp32 entry's)
    key = ("wgrad" if sfb_rows else "fp32_out", index, m, n, k, strict, policy)
    t = _PLANS.get(key)
    if t is None:
        t = _remember(key, _with_policy((tiling_wgrad if sfb_rows else tiling_fp32_out)(m, n, k), strict, policy))
    return t


def _fp32_out_call(name: str, lhs, rhs, out, c, tiling_, sync, strict, policy, zero_padded, sfb_rows: bool) -> None:
    """gemm_fp8_fp8_fp32_nt (sfb_rows=False) and wgrad_gemm_fp8_fp8_fp32_nt (sfb_rows=True): checks, plan, launch."""
    a, sfa = lhs
    b, sfb = rhs
    _require(policy is None or policy in _FP32_OUT_POLICIES, "%s: policy must be one of %s", name, list(_FP32_OUT_POLICIES))
    _require(not (strict and policy not in (None, "strict")), "strict=True contradicts policy=%r", policy)
    m, n, k, lda, ldb = _dense_fp8_operands(a, sfa, b, sfb, out, torch.float32, "float32", sfb_rows)
    if k == 0:
        lda = ldb = 0   # (a zero-width view has no meaningful row stride: nothing is read, out = c)
    if c is not None:
        _accumuland(c, (m, n), out)
    flags = _zero_padded_flags(a, b, zero_padded) if lda != k or ldb != k else 0
    with _device_guard(a, b, sfa, sfb, out, *(() if c is None else (c,))):
        index = out.device.index
        if tiling_ is None:
            tiling_ = _planned_fp32_out(index, m, n, k, strict, policy, sfb_rows)
        else:
            tiling_ = _with_policy(tiling_, strict, policy)
        stream = _stream_of(index)
        ws_ptr, ws_bytes = _workspace(tiling_, out.device, stream)
        entry = _lib.lib().dga_wgrad_gemm_fp8_fp8_fp32_nt if sfb_rows else _lib.lib().dga_gemm_fp8_fp8_fp32_nt
        rc = entry(a.data_ptr(), lda, sfa.data_ptr(), b.data_ptr(), ldb, sfb.data_ptr(), None if c is None else c.data_ptr(),
                   out.data_ptr(), m, n, k, flags, ctypes.byref(tiling_), ws_ptr, ws_bytes, stream)
        if rc:
            _lib.check(rc, name)
        if sync:
            torch.cuda.current_stream(out.device).synchronize()


def tiling_k_grouped_wgrad(m: int, n: int, k_total: int, groups: int) -> Tiling:
    """dga_tiling_k_grouped_wgrad: the default tiling of k_grouped_wgrad_gemm_fp8_fp8_fp32_nt -- a rule on the G x tiles(M, N) raster
    (the persistent 128 x 256 build where it fills the CUs, else a one-tile build whose raster does), no split-K, no workspace, no
    tiling-cache lookup; the strict tag under $DGA_DEFAULT_POLICY=strict."""
    return _default_tiling("tiling_k_grouped_wgrad", _problem(m, n, k_total, groups, 0))


def tiling_check_k_grouped_wgrad(t: Tiling) -> int:
    """dga_tiling_check_k_grouped_wgrad: 0 if k_grouped_wgrad_gemm_fp8_fp8_fp32_nt takes this tiling, else the status it returns
    before any launch."""
    return int(_lib.lib().dga_tiling_check_k_grouped_wgrad(ctypes.byref(t)))


def k_grouped_wgrad_gemm_fp8_fp8_fp32_nt(lhs: Tuple[torch.Tensor, torch.Tensor], rhs: Tuple[torch.Tensor, torch.Tensor],
                                         out: torch.Tensor, ks: Sequence[int], ks_tensor: Optional[torch.Tensor] = None,
                                         c: Optional[torch.Tensor] = None, tiling_: Optional[Tiling] = None, sync: bool = False,
                                         strict: bool = False, policy: Optional[str] = None) -> None:
    """Upstream DeepGEMM's MoE weight-gradient GEMM, the groups along K (the tokens): for every expert g,
    out[g] (fp32 [M,N], written in place) = c[g] (optional) + A[:, k0_g : k0_g + ks[g]] . B[:, k0_g : k0_g + ks[g]]^T, dequantised,
    with k0_g = sum(ks[:g]).  lhs = (A [M, K_total] fp8, sfa [M, K_total/128]) = per_token_cast_to_fp8(dY^T), rhs = (B [N, K_total]
    fp8, sfb [N, K_total/128]) = per_token_cast_to_fp8(X^T) of the token buffer in the contiguous forward layout; out and c are
    [G, M, N] float32, contiguous (c may be out itself: accumulate).  A and B may be row-strided views (row stride >= K_total, a
    multiple of 16 bytes).

    ks: the tokens per expert, G host ints -- each a multiple of 128 (get_m_alignment_for_contiguous_layout()), 0 allowed, sum <=
    K_total -- used to check the call only.  The kernel reads ks_tensor (device int32 [G], the same counts) while it executes, so a
    captured graph replays with whatever ks_tensor holds then.  ks_tensor=None builds it from ks: a host-to-device copy, not
    capture-safe.  An empty expert gets c[g] exactly, or zeros.

    Arithmetic: "bf16_exact" (default) -- every group is wgrad_gemm_fp8_fp8_fp32_nt on contiguous copies of its slices with the
    same tile and no split-K, bit for bit, then + c[g]; "strict" (strict=True) -- the oracle's fp32 result, bit for bit.  "fast",
    "auto" and the _ue8m0 policies raise."""
    name = "k_grouped_wgrad_gemm_fp8_fp8_fp32_nt"
    a, sfa = lhs
    b, sfb = rhs
    _require(policy is None or policy in _FP32_OUT_POLICIES, "%s: policy must be one of %s", name, list(_FP32_OUT_POLICIES))
    _require(not (strict and policy not in (None, "strict")), "strict=True contradicts policy=%r", policy)
    _fp8_bytes(a); _fp8_bytes(b)
    if a.dim() != 2 or b.dim() != 2:
        _fail("A and B must be rank 2")
    if out.dim() != 3 or out.dtype != torch.float32 or not out.is_contiguous():
        _fail("out must be a contiguous float32 [G, M, N]")
    g, m, n = out.shape
    k_total = a.shape[1]
    if a.shape[0] != m or b.shape[0] != n or b.shape[1] != k_total:
        _fail(f"A must be [{m}, K_total] and B [{n}, K_total] with out [{g}, {m}, {n}]")
    if k_total % 128:
        _fail("K_total must be a multiple of 128")
    kb = k_total // 128
    if sfa.dtype != torch.float32 or sfb.dtype != torch.float32:
        _fail("scales must be float32")
    if sfa.dim() != 2 or sfa.shape[0] != m or sfa.shape[1] != kb:
        _fail(f"sfa must be [{m},{kb}]")
    if sfb.dim() != 2 or sfb.shape[0] != n or sfb.shape[1] != kb:
        _fail(f"sfb must be [{n},{kb}] (one scale per row of B: per_token_cast_to_fp8)")
    if not (sfa.is_contiguous() and sfb.is_contiguous()):
        _fail("scales must be contiguous")
    if (k_total > 1 and (a.stride(1) != 1 or b.stride(1) != 1)) or (m > 1 and a.stride(0) < k_total) or (n > 1 and b.stride(0) < k_total):
        _fail("operands must be row-major with unit inner stride (row-strided views are accepted)")
    lda = a.stride(0) if m > 1 else k_total
    ldb = b.stride(0) if n > 1 else k_total
    if k_total == 0:
        lda = ldb = 0
    elif lda % 16 or ldb % 16:
        _fail("row strides of A and B must be multiples of 16 bytes")
    ks = [int(v) for v in ks]
    if len(ks) != g:
        _fail(f"ks must hold {g} counts, one per group")
    if any(v < 0 or v % 128 for v in ks):
        _fail("every ks[g] must be >= 0 and a multiple of 128")
    if sum(ks) > k_total:
        _fail(f"sum(ks) = {sum(ks)} exceeds K_total = {k_total}")
    if ks_tensor is not None:
        if ks_tensor.dtype != torch.int32 or ks_tensor.dim() != 1 or ks_tensor.shape[0] != g or not ks_tensor.is_contiguous():
            _fail(f"ks_tensor must be a contiguous int32 [{g}]")
        if ks_tensor.device != out.device:
            _fail("ks_tensor must live on the operands' device")
    if c is not None:
        _accumuland(c, (g, m, n), out)
    with _device_guard(a, b, sfa, sfb, out, *(() if c is None else (c,)), *(() if ks_tensor is None else (ks_tensor,))):
        index = out.device.index
        if tiling_ is None:
            # (the entry is part of the key: never a plan of the dense fp32 or wgrad entries)
            key = ("k_grouped_wgrad", index, m, n, k_total, g, strict, policy)
            tiling_ = _PLANS.get(key)
            if tiling_ is None:
                tiling_ = _remember(key, _with_policy(tiling_k_grouped_wgrad(m, n, k_total, g), strict, policy))
        else:
            tiling_ = _with_policy(tiling_, strict, policy)
        if ks_tensor is None:
            ks_tensor = torch.tensor(ks, dtype=torch.int32, device=out.device)
        rc = _lib.lib().dga_k_grouped_wgrad_gemm_fp8_fp8_fp32_nt(
            a.data_ptr(), lda, sfa.data_ptr(), b.data_ptr(), ldb, sfb.data_ptr(), _ptr(c),
            out.data_ptr(), ks_tensor.data_ptr(), g, m, n, k_total, 0, ctypes.byref(tiling_), None, 0, _stream_of(index))
        if rc:
            _lib.check(rc, name)
        if sync:
            torch.cuda.current_stream(out.device).synchronize()


def gemm_fp8_loop_clock(lhs, rhs, out: torch.Tensor, tiling_: Optional[Tiling] = None, launches: int = 50):
    """(clock_mhz, loop_us): the shader clock the chip holds inside the main loop of the dense kernel `tiling_` selects,
    and that loop's duration, from the loop-clock build (dga_gemm_fp8_loop_clock; a diagnostic: it synchronises)."""
    a, sfa = lhs
    b, sfb = rhs
    _fp8_bytes(a); _fp8_bytes(b)
    m, k = a.shape
    n = b.shape[0]
    with _device_guard(a, b, sfa, sfb, out):
        if tiling_ is None:
            tiling_ = tiling(m, n, k)
        tiles = -(-m // max(1, tiling_.m1)) * -(-n // max(1, tiling_.n1))
        ws_ptr, ws_bytes = _scratch("clock", out.device, tiles * 128)
        mhz, us = ctypes.c_float(0), ctypes.c_float(0)
        rc = _lib.lib().dga_gemm_fp8_loop_clock(a.data_ptr(), sfa.data_ptr(), b.data_ptr(), sfb.data_ptr(), out.data_ptr(),
                                                m, n, k, ctypes.byref(tiling_), ws_ptr, ws_bytes, int(launches),
                                                _stream_ptr(out), ctypes.byref(mhz), ctypes.byref(us))
        _lib.check(rc, "gemm_fp8_loop_clock")
    return mhz.value, us.value


def mfma_ceiling(policy: str = "fast", launches: int = 300, device=None) -> float:
    """TFLOP/s the matrix pipe of this device sustains on the policy's inner step with the operands already in registers
    (dga_mfma_ceiling: matrix instruction + fp32 promotion [+ in-register conversions], two waves per SIMD on every CU,
    random e4m3 bytes, the last of `launches` back-to-back launches).  A diagnostic: it synchronises."""
    _require(policy in ("fast", "bf16_exact"), "mfma_ceiling: policy must be 'fast' or 'bf16_exact'")
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    with torch.cuda.device(dev):
        cus = torch.cuda.get_device_properties(dev).multi_processor_count
        ws_ptr, ws_bytes = _scratch("ceiling", dev, 16384 + 2048 * cus)
        tf = ctypes.c_float(0)
        rc = _lib.lib().dga_mfma_ceiling(0 if policy == "fast" else 1, int(launches), ws_ptr, ws_bytes,
                                         torch.cuda.current_stream(dev).cuda_stream, ctypes.byref(tf))
        _lib.check(rc, "mfma_ceiling")
    return tf.value


def m_grouped_gemm_fp8_fp8_bf16_nt_masked(lhs, rhs, out: torch.Tensor, masked_m: torch.Tensor, expected_m: int,
                                          tiling_: Optional[Tiling] = None, sync: bool = False,
                                          strict: bool = False, policy: Optional[str] = None) -> None:
    """Grouped masked-M GEMM: a [G,Mmax,K], sfa [G,Mmax,KB], b [G,N,K], sfb [G,NB,KB], out [G,Mmax,N] bf16;
    only rows < masked_m[g] of out[g] are written (upstream DeepGEMM's convention)."""
    a, sfa = lhs
    b, sfb = rhs
    _fp8_bytes(a); _fp8_bytes(b)
    if a.dim() != 3 or b.dim() != 3 or out.dim() != 3:
        _fail("rank must be 3")
    g, mmax, k = a.shape
    g2, n, k2 = b.shape
    if g != g2 or k != k2:
        _fail("group / k mismatch")
    if tuple(out.shape) != (g, mmax, n) or out.dtype != torch.bfloat16:
        _fail("out must be [G,Mmax,N] bfloat16")
    kb, nb = (k + 127) // 128, (n + 127) // 128
    if tuple(sfa.shape) != (g, mmax, kb) or sfa.dtype != torch.float32:
        _fail(f"sfa must be [{g},{mmax},{kb}] f32")
    if tuple(sfb.shape) != (g, nb, kb) or sfb.dtype != torch.float32:
        _fail(f"sfb must be [{g},{nb},{kb}] f32")
    if masked_m.dtype != torch.int32 or masked_m.dim() != 1 or masked_m.shape[0] != g:
        _fail("masked_m must be int32 [G]")
    if not (a.is_contiguous() and b.is_contiguous() and sfa.is_contiguous() and sfb.is_contiguous() and out.is_contiguous() and
            masked_m.is_contiguous()):
        _fail("operands must be contiguous")
    expected_m = int(expected_m)
    with _device_guard(a, b, sfa, sfb, out, masked_m):
        index = out.device.index
        if tiling_ is None:
            tiling_ = _planned(index, mmax, n, k, g, expected_m, False, strict, policy)
        else:
            tiling_ = _with_policy(tiling_, strict, policy)
        stream = _stream_of(index)
        ws_ptr, ws_bytes = _workspace(tiling_, out.device, stream)
        rc = _lib.lib().dga_m_grouped_gemm_fp8_fp8_bf16_nt_masked(
            a.data_ptr(), sfa.data_ptr(), b.data_ptr(), sfb.data_ptr(), out.data_ptr(), masked_m.data_ptr(),
            g, mmax, n, k, expected_m, ctypes.byref(tiling_), ws_ptr, ws_bytes, stream)
        if rc:
            _lib.check(rc, "m_grouped_gemm_fp8_fp8_bf16_nt_masked")
        if sync:
            torch.cuda.current_stream(out.device).synchronize()


def m_grouped_gemm_fp8_fp8_bf16_nt_masked_indexed(a_rows: torch.Tensor, sfa_src: torch.Tensor, sfa_byte_offset: int,
                                                  sfa_ld: int, rhs, out_rows: torch.Tensor, row_index: torch.Tensor,
                                                  masked_m: torch.Tensor, m_max: int, expected_m: int = 0,
                                                  tiling_: Optional[Tiling] = None, sync: bool = False,
                                                  strict: bool = False, policy: Optional[str] = None) -> None:
    """Masked grouped GEMM on rows that stay where they are (dga_m_grouped_gemm_fp8_fp8_bf16_nt_masked_indexed):
    row r of group g is row row_index[g * m_max + r] of the flat byte rows `a_rows` [rows, lda] (first K bytes = fp8),
    its 1x128 scales start at byte sfa_byte_offset of row row_index[...] of `sfa_src` viewed with sfa_ld floats per row
    (the same payload rows, or a separate [rows, KB] float tensor with offset 0), and its result is written to that row
    of `out_rows` [rows, ldc] bf16.  b [G,N,K], sfb [G,NB,KB]; only r < masked_m[g] is read or written."""
    b, sfb = rhs
    _fp8_bytes(b); _fp8_bytes(a_rows)
    _require(a_rows.dim() == 2 and a_rows.stride(1) == 1 and out_rows.dim() == 2 and out_rows.stride(1) == 1, "2-D row tensors")
    g, n, k = b.shape
    rows, lda = a_rows.shape[0], a_rows.stride(0)
    kb, nb = (k + 127) // 128, (n + 127) // 128
    _require(a_rows.shape[1] >= k and out_rows.shape[1] >= n and out_rows.dtype == torch.bfloat16, "row widths")
    _require(out_rows.shape[0] >= rows, "out_rows must have a row for every source row")
    _require(tuple(sfb.shape) == (g, nb, kb) and sfb.dtype == torch.float32, "sfb must be [%d,%d,%d] f32", g, nb, kb)
    _require(row_index.dtype == torch.int64 and row_index.numel() >= g * m_max and row_index.is_contiguous(), "row_index int64[G*m_max]")
    _require(masked_m.dtype == torch.int32 and tuple(masked_m.shape) == (g,), "masked_m must be int32 [G]")
    _require(sfa_byte_offset % 4 == 0 and sfa_ld >= kb, "scale rows must be float-aligned")
    # the kernel reads row r's scales at sfa_src + offset + r * sfa_ld floats: the tensor has to be what that arithmetic assumes
    _require(sfa_src.dim() == 2 and sfa_src.stride(1) == 1 and sfa_src.dtype in (torch.float32, torch.uint8),
             "sfa_src must be a 2-D float32 (or uint8 payload) row tensor with unit inner stride")
    _require(sfa_src.stride(0) * sfa_src.element_size() == 4 * sfa_ld, "sfa_ld must be sfa_src's row stride in floats")
    _require(sfa_src.data_ptr() % 4 == 0 and sfa_src.shape[0] >= rows and
             sfa_byte_offset + 4 * kb <= sfa_src.shape[1] * sfa_src.element_size(),
             "sfa_src must hold ceil(K/128) floats at sfa_byte_offset of each of the source's rows")
    with _device_guard(a_rows, b, sfb, out_rows, row_index, masked_m, sfa_src):
        if tiling_ is None:
            tiling_ = _planned(out_rows.device.index, m_max, n, k, g, int(expected_m), False, strict, policy)
        else:
            tiling_ = _with_policy(tiling_, strict, policy)
        rc = _lib.lib().dga_m_grouped_gemm_fp8_fp8_bf16_nt_masked_indexed(
            a_rows.data_ptr(), lda, sfa_src.data_ptr() + sfa_byte_offset, sfa_ld, b.data_ptr(), sfb.data_ptr(),
            out_rows.data_ptr(), out_rows.stride(0), row_index.data_ptr(), rows, masked_m.data_ptr(), g, m_max, n, k,
            int(expected_m), ctypes.byref(tiling_), None, 0, _stream_ptr(out_rows))
        _lib.check(rc, "m_grouped_gemm_fp8_fp8_bf16_nt_masked_indexed")
        if sync:
            torch.cuda.current_stream(out_rows.device).synchronize()


def catlass_dynamic_matmul(self_: torch.Tensor, mat2: torch.Tensor, out: torch.Tensor, sync: bool = False) -> None:
    """The aclnn operator CatlassDynamicMatmul in its own dtypes: out[M,N] = self[M,K] @ mat2[K,N], all fp16 or all bf16.
    mat2 is the logical [K,N] matrix in column-major storage, i.e. the transposed view of a contiguous [N,K] tensor
    (`b.t()`), the operator's only layout (catlass_dynamic_matmul_tiling.cpp:83-84)."""
    _require(self_.dim() == 2 and mat2.dim() == 2 and out.dim() == 2, "rank must be 2")
    m, k = self_.shape
    k2, n = mat2.shape
    _require(k == k2, "self dimk is not equal with mat2 dimk")
    _require(self_.dtype in (torch.float16, torch.bfloat16) and mat2.dtype == self_.dtype and out.dtype == self_.dtype,
             "self, mat2 and out must share one 16-bit dtype")
    _require(tuple(out.shape) == (m, n) and out.is_contiguous() and self_.is_contiguous(), "self / out must be contiguous")
    _require(n == 0 or k == 0 or (mat2.stride(0) == 1 and mat2.stride(1) == k) or (k == 1 and mat2.stride(1) == 1) or
             (n == 1 and mat2.stride(0) == 1), "mat2 must be the transposed view of a contiguous [N,K] tensor (NT)")
    dt = _lib.DT_BF16 if self_.dtype == torch.bfloat16 else _lib.DT_FP16
    with _device_guard(self_, mat2, out):
        need = int(_lib.lib().dga_catlass_dynamic_matmul_workspace_bytes(m, n, k, self_.data_ptr(), mat2.data_ptr()))
        ws_ptr, ws_bytes = _scratch("op16", out.device, need)
        rc = _lib.lib().dga_catlass_dynamic_matmul(self_.data_ptr(), mat2.data_ptr(), out.data_ptr(), m, n, k, dt,
                                                   ws_ptr, ws_bytes, _stream_ptr(out))
        _lib.check(rc, "catlass_dynamic_matmul")
        if sync:
            torch.cuda.current_stream(out.device).synchronize()


def get_m_alignment_for_contiguous_layout() -> int:
    """Row alignment of the group segments in the contiguous-grouped layout (upstream DeepGEMM's name)."""
    return _lib.CONTIGUOUS_M_ALIGNMENT


def m_grouped_gemm_fp8_fp8_bf16_nt_contiguous(lhs, rhs, out: torch.Tensor, m_indices: torch.Tensor,
                                              tiling_: Optional[Tiling] = None, sync: bool = False,
                                              strict: bool = False, policy: Optional[str] = None) -> None:
    """Contiguous-grouped GEMM (the prefill-side MoE layout): a [Msum,K], sfa [Msum,KB], b [G,N,K], sfb [G,NB,KB],
    out [Msum,N] bf16, m_indices int32 [Msum].  Row r is multiplied with b[m_indices[r]]; rows with a negative index
    are padding and stay untouched.  Group segments start at multiples of get_m_alignment_for_contiguous_layout()
    rows, padding rows follow a segment's valid rows."""
    a, sfa = lhs
    b, sfb = rhs
    _fp8_bytes(a); _fp8_bytes(b)
    _require(a.dim() == 2 and b.dim() == 3 and out.dim() == 2, "a/out rank 2, b rank 3")
    msum, k = a.shape
    g, n, k2 = b.shape
    _require(k == k2, "k mismatch")
    _require(tuple(out.shape) == (msum, n) and out.dtype == torch.bfloat16, "out must be [Msum,N] bfloat16")
    kb, nb = (k + 127) // 128, (n + 127) // 128
    _require(tuple(sfa.shape) == (msum, kb) and sfa.dtype == torch.float32, "sfa must be [%d,%d] f32", msum, kb)
    _require(tuple(sfb.shape) == (g, nb, kb) and sfb.dtype == torch.float32, "sfb must be [%d,%d,%d] f32", g, nb, kb)
    _require(m_indices.dtype == torch.int32 and tuple(m_indices.shape) == (msum,), "m_indices must be int32 [Msum]")
    for t in (a, b, sfa, sfb, out, m_indices):
        _require(t.is_contiguous(), "operands must be contiguous")
    with _device_guard(a, b, sfa, sfb, out, m_indices):
        if tiling_ is None:   # (the C side buckets Msum in its cache key and re-derives the workgroup count per call: not memoised here)
            if policy is None and not strict:
                policy = default_policy()      # no tiling, no policy: the operator's default arithmetic, as in the other entries
            _require(policy != "auto" or not strict, "strict=True contradicts policy='auto'")
            policy = "fast" if policy == "auto" else policy
            tiling_ = tiling(msum, n, k, groups=g, contiguous=True, policy="bf16_exact" if policy in ("bf16_exact", "bf16_exact_ue8m0") else None)
        tiling_ = _with_policy(tiling_, strict, policy)
        ws_ptr, ws_bytes = _workspace(tiling_, out.device)
        rc = _lib.lib().dga_m_grouped_gemm_fp8_fp8_bf16_nt_contiguous(
            a.data_ptr(), sfa.data_ptr(), b.data_ptr(), sfb.data_ptr(), out.data_ptr(), m_indices.data_ptr(),
            msum, g, n, k, ctypes.byref(tiling_), ws_ptr, ws_bytes, _stream_ptr(out))
        _lib.check(rc, "m_grouped_gemm_fp8_fp8_bf16_nt_contiguous")
        if sync:
            torch.cuda.current_stream(out.device).synchronize()


_CAST_DT = {torch.float32: _lib.DT_FP32, torch.bfloat16: _lib.DT_BF16, torch.float16: _lib.DT_FP16}


def _cast(fn_name: str, x: torch.Tensor, block_rows: int, aligned_rows: bool = False, use_ue8m0: bool = False):
    _require(x.dim() == 2 and x.is_contiguous(), "x must be a contiguous [rows, k] tensor")
    _require(x.dtype in _CAST_DT, "x must be float32, bfloat16 or float16")
    rows, k = x.shape
    ldq = (k + 127) // 128 * 128 if aligned_rows else k   # whole 128-byte lines: a row's k blocks never straddle two
    q = torch.empty((rows, ldq), dtype=torch.uint8, device=x.device)
    sf = torch.empty(((rows + block_rows - 1) // block_rows, (k + 127) // 128), dtype=torch.float32, device=x.device)
    # (the _ex entry alone: the C entries without ldq or flags are the same call with k and 0.  DGA_CAST_UE8M0: scales rounded up to 2^n)
    _launch(fn_name, (x,), lambda L, stream: getattr(L, fn_name + "_ex")(
        x.data_ptr(), _CAST_DT[x.dtype], rows, k, q.data_ptr(), ldq, sf.data_ptr(), _lib.CAST_UE8M0 if use_ue8m0 else 0, stream))
    q = q.view(torch.float8_e4m3fn)
    if ldq != k:
        q = q[:, :k]
        q._dga_zero_padded = True   # (a Python attribute: views and copies made from it do not carry the promise)
    return q, sf


def per_token_cast_to_fp8(x: torch.Tensor, aligned_rows: bool = False, use_ue8m0: bool = False):
    """Activation quantiser: x [rows,k] -> (e4m3fn [rows,k], fp32 scales [rows, ceil(k/128)]), one scale per 1x128
    block: scale = amax/448, q = RNE-satfinite(x/scale) (the A-operand format of gemm_fp8_fp8_bf16_nt).
    aligned_rows=True: the result is a [rows, k] view of rows round_up(k, 128) bytes apart with zero tails, which
    gemm_fp8_fp8_bf16_nt reads in place whatever k is (no padding pass for k % 16 != 0; 1279 x 5003 x 7681: 80.6 -> 65.8 us.
    Rows only 16-byte aligned are read in place too but gain nothing: a 128-byte row piece that straddles two cache lines
    costs two requests on every re-read, profiles/r04_odd_k_rows.txt).
    use_ue8m0=True (upstream DeepGEMM's keyword): scale = 2^ceil(log2(amax / 448)), a power of two -- operands quantised this way
    on BOTH sides may be multiplied under policy="fast_ue8m0" (the scales ride in the matrix instruction's E8M0 operands)."""
    return _cast("dga_cast_to_fp8_1x128", x, 1, aligned_rows, use_ue8m0)


def per_block_cast_to_fp8(x: torch.Tensor, aligned_rows: bool = False, use_ue8m0: bool = False):
    """Weight quantiser: x [rows,k] -> (e4m3fn [rows,k], fp32 scales [ceil(rows/128), ceil(k/128)]), one scale per
    128x128 block (the B-operand format).  aligned_rows, use_ue8m0: as per_token_cast_to_fp8."""
    return _cast("dga_cast_to_fp8_128x128", x, 128, aligned_rows, use_ue8m0)


_FUSED_LAST_DIM = {2: "the last dimension of x must be even (gate and up halves)",
                   256: "the last dimension of x must be 2H with H a multiple of 128 (gate and up halves of whole 1x128 blocks)"}


def _fused_layout(x: torch.Tensor, masked_m: Optional[torch.Tensor], m_indices: Optional[torch.Tensor], multiple: int, last: str = "2H"):
    """The row layouts of the fused quantisers, checked: x [rows, 2H], or [G, Mmax, 2H] with masked_m int32 [G], or [rows, 2H] with m_indices
    int32 [rows]; the last dimension a multiple of `multiple` (`last`: its name in the messages -- per_token_cast_to_fp8_transposed has no
    halves).  Returns (H, the leading dimensions, groups, rows per group)."""
    _require(masked_m is None or m_indices is None, "masked_m and m_indices exclude each other")
    if masked_m is not None:
        _require(x.dim() == 3 and x.is_contiguous(), "x must be a contiguous [G, Mmax, %s] tensor with masked_m", last)
    else:
        _require(x.dim() == 2 and x.is_contiguous(), "x must be a contiguous [rows, %s] tensor", last)
    _require(x.dtype in _CAST_DT, "x must be float32, bfloat16 or float16")
    if multiple != 1:    # (1: per_token_cast_to_fp8_transposed, any width)
        _require(x.shape[-1] % multiple == 0, _FUSED_LAST_DIM[multiple])
    lead = tuple(x.shape[:-1])
    groups, rows = (lead if masked_m is not None else (1, lead[0]))
    _row_masks(masked_m, m_indices, groups, rows)
    return x.shape[-1] // 2, lead, groups, rows


def _row_pair(lead: tuple, width: int, q_name: str = "q", sf_name: str = "sf"):
    """_outputs' specs of per-token codes [lead, width] and their 1x128 scales."""
    return (q_name, torch.uint8, lead + (width,)), (sf_name, torch.float32, lead + ((width + 127) // 128,))


def silu_and_mul_per_token_cast_to_fp8(x: torch.Tensor, masked_m: Optional[torch.Tensor] = None,
                                       m_indices: Optional[torch.Tensor] = None,
                                       out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, use_ue8m0: bool = False,
                                       sync: bool = False):
    """The activation of an expert MLP fused into the quantiser of its second GEMM (dga_silu_mul_cast_to_fp8_1x128):
    (q, sf) = per_token_cast_to_fp8(silu(x[..., :H]) * x[..., H:]) with the product kept in fp32, x [..., 2H] float32 / bfloat16 /
    float16 (gate first, up second: the silu_and_mul convention) -> q [..., H] float8_e4m3fn, sf [..., ceil(H/128)] float32.
      x [rows, 2H]                                   every row
      x [G, Mmax, 2H], masked_m int32 [G]            rows r >= masked_m[g] are neither read nor written (the masked grouped GEMM's layout)
      x [rows, 2H],    m_indices int32 [rows]        rows with a negative index are neither read nor written (the contiguous one's)
    The masks are read on the device: a captured graph follows the routing.  out=(q, sf) writes into the caller's tensors (q uint8
    or float8_e4m3fn); without it both are torch.empty, so the rows a mask excludes are UNINITIALISED -- pass out to give them
    a value.  For gate >= 20 the result is the quantiser's on fl32(gate * up) bit for bit, for |gate| <= 16 the fp32 product is
    within relative 2^-18 of the real-number value; use_ue8m0 as in per_token_cast_to_fp8."""
    h, lead, groups, rows = _fused_layout(x, masked_m, m_indices, 2)
    q, sf = _outputs(out, _row_pair(lead, h), x.device, "out must be (q, sf)")
    _launch("silu_and_mul_per_token_cast_to_fp8", (x, q, sf, masked_m, m_indices), lambda L, stream: L.dga_silu_mul_cast_to_fp8_1x128(
        x.data_ptr(), _CAST_DT[x.dtype], groups, rows, h, _ptr(masked_m), _ptr(m_indices), q.data_ptr(), sf.data_ptr(),
        _lib.CAST_UE8M0 if use_ue8m0 else 0, stream), sync)
    return _as_fp8(q), sf


def silu_and_mul_backward_per_token_cast_to_fp8(x: torch.Tensor, grad_h: torch.Tensor, masked_m: Optional[torch.Tensor] = None,
                                                m_indices: Optional[torch.Tensor] = None,
                                                out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                                                grad_x_out: Optional[torch.Tensor] = None, use_ue8m0: bool = False,
                                                sync: bool = False):
    """The backward of silu_and_mul_per_token_cast_to_fp8's activation fused into the quantiser of the dgrad of the first GEMM
    (dga_silu_mul_bwd_cast_to_fp8_1x128): with gate = x[..., :H], up = x[..., H:] and s = sigmoid(gate),
      dgate = grad_h * up * (s + gate s (1 - s)),   dup = grad_h * gate s,   (dq, dsf) = per_token_cast_to_fp8([dgate | dup])
    with both gradients kept in fp32.  x [..., 2H] (the tensor the forward read) and grad_h [..., H] share dtype (float32 / bfloat16 /
    float16) and leading dimensions, both contiguous -> dq [..., 2H] float8_e4m3fn, dsf [..., 2H/128] float32: the lhs of
    gemm_fp8_fp8_bf16_nt and the grouped entries with K = 2H.  H % 128 == 0 is required (no 1x128 block straddles the two halves).
    Row layouts, masks (read on the device), out=(dq, dsf), use_ue8m0 and sync: as silu_and_mul_per_token_cast_to_fp8; a row a mask
    excludes is neither read nor written, in any output.  grad_x_out: a contiguous [..., 2H] tensor of x's dtype that receives the
    unquantised gradient in the same pass (fp32 rounded to nearest even for the 16-bit types) on the valid rows -- what
    per_token_cast_to_fp8_transposed (same mask) turns into the operand of k_grouped_wgrad_gemm_fp8_fp8_fp32_nt.  For gate >= 20 the result is the quantiser's
    on [fl32(grad_h * up) | fl32(grad_h * gate)] bit for bit; for |gate| <= 16 dup is within relative 2^-18 and dgate within
    2^-17 |grad_h up| (s + |gate| s (1 - s)) of the real-number value.
    silu_and_mul_backward_per_token_cast_to_fp8_transposed(rowwise=True) returns this (dq, dsf) and the dW1 operand from one read, without grad_x_out."""
    h, lead, groups, rows = _fused_layout(x, masked_m, m_indices, 256)
    _want(grad_h, "grad_h", None, lead + (h,))
    _require(grad_h.dtype == x.dtype, "grad_h must have x's dtype")
    q, sf = _outputs(out, _row_pair(lead, 2 * h, "dq", "dsf"), x.device, "out must be (dq, dsf)")
    if grad_x_out is not None:
        _want(grad_x_out, "grad_x_out", None, tuple(x.shape))
        _require(grad_x_out.dtype == x.dtype, "grad_x_out must have x's dtype")
    _launch("silu_and_mul_backward_per_token_cast_to_fp8", (x, grad_h, q, sf, masked_m, m_indices, grad_x_out),
            lambda L, stream: L.dga_silu_mul_bwd_cast_to_fp8_1x128(
                x.data_ptr(), grad_h.data_ptr(), _CAST_DT[x.dtype], groups, rows, h, _ptr(masked_m), _ptr(m_indices), q.data_ptr(),
                sf.data_ptr(), _ptr(grad_x_out), _lib.CAST_UE8M0 if use_ue8m0 else 0, stream), sync)
    return _as_fp8(q), sf


def _cast_transposed(c_name: str, name: str, x, h: int, lead: tuple, groups: int, rows: int, masked_m, m_indices, rowwise: bool,
                     aligned_rows: bool, use_ue8m0: bool, out, sync: bool, call=None, also=()):
    """What the transposing quantisers share once the layout of x is known (h: the channels of the result): the outputs -- torch.empty, or
    the caller's out= checked --, the call of the C entry `c_name`, and the nesting of the result.  call: an entry with other inputs than
    (x, masked_m, m_indices) -- call(fn, qt, ldqt, sft, q, sf, flags, stream) -> rc, q and sf pointers or None; also: its further tensors."""
    t_n = groups * rows
    ldqt = (t_n + 127) // 128 * 128 if aligned_rows else t_n
    out_t, out_r = _nested_out(out, rowwise)
    sft_shape = (h, (t_n + 127) // 128)
    if out_t is None:
        qt = torch.empty((h, ldqt), dtype=torch.uint8, device=x.device)[:, :t_n]
        sft = torch.empty(sft_shape, dtype=torch.float32, device=x.device)
    else:    # (qt is the one output that need not be contiguous: its rows are ldqt bytes apart)
        _require(isinstance(out_t, (tuple, list)) and len(out_t) == 2, "out must hold (qt, sft)")
        qt, sft = out_t
        _fp8_bytes(qt)
        _require(tuple(qt.shape) == (h, t_n) and (t_n <= 1 or qt.stride(1) == 1) and (h <= 1 or qt.stride(0) == ldqt),
                 "out qt must be [%d, %d] with rows %d bytes apart", h, t_n, ldqt)
        _want(sft, "sft", torch.float32, sft_shape, "out ")
    q, sf = _outputs(out_r, _row_pair(lead, h), x.device, "out must be (q, sf)") if rowwise else (None, None)
    flags = _lib.CAST_UE8M0 if use_ue8m0 else 0
    if call is None:
        call = lambda fn, *outputs: fn(x.data_ptr(), _CAST_DT[x.dtype], groups, rows, h, _ptr(masked_m), _ptr(m_indices), *outputs)
    _launch(name, (x, qt, sft, *also, masked_m, m_indices, q, sf), lambda L, stream: call(
        getattr(L, c_name), qt.data_ptr(), ldqt, sft.data_ptr(), _ptr(q), _ptr(sf), flags, stream), sync)
    qt = qt.view(torch.float8_e4m3fn)   # (always a new tensor object: the promise below is never left on a tensor of the caller's)
    if ldqt != t_n:
        qt._dga_zero_padded = True      # (as _cast: the tails are zero, and views made from qt do not carry the promise)
    return ((qt, sft), (_as_fp8(q), sf)) if rowwise else (qt, sft)


def per_token_cast_to_fp8_transposed(x: torch.Tensor, masked_m: Optional[torch.Tensor] = None, m_indices: Optional[torch.Tensor] = None,
                                     rowwise: bool = False, aligned_rows: bool = False, use_ue8m0: bool = False, out=None,
                                     sync: bool = False):
    """per_token_cast_to_fp8 of the transpose of token-major activations in one pass (dga_cast_to_fp8_1x128_transposed): the operands
    of wgrad_gemm_fp8_fp8_fp32_nt / k_grouped_wgrad_gemm_fp8_fp8_fp32_nt, which run K along the tokens, without x.t().contiguous().
      (qt, sft) = per_token_cast_to_fp8(x0.t().contiguous(), aligned_rows, use_ue8m0),  x0 = x with the rows a mask excludes set to zero,
    byte for byte and bit for bit: qt [H, T] float8_e4m3fn, sft [H, ceil(T/128)] float32, T the number of rows of x over all groups.
      x [T, H]                                     every row
      x [G, Mmax, H], masked_m int32 [G]           rows r >= masked_m[g] are not read and count as zeros (T = G * Mmax)
      x [T, H],       m_indices int32 [T]          rows with a negative index are not read and count as zeros
    The masks are read on the device: a captured graph follows the routing.  Unlike in the fused quantisers EVERY element of qt and sft
    is written: an excluded token has code 0, a 128-token block without a valid token has scale 1 (NaN or garbage in the padding rows
    of a contiguous-layout buffer changes nothing: no masked_fill before the call).  aligned_rows=True: qt is a [H, T] view of rows
    round_up(T, 128) bytes apart with zero tails, as in per_token_cast_to_fp8.
    rowwise=True also returns (q, sf) = per_token_cast_to_fp8(x) from the same read of x -- the form fprop and dgrad take -- on the valid
    rows (q [..., H], sf [..., ceil(H/128)]; the rows a mask excludes are not written), and the result is ((qt, sft), (q, sf)).
    out= takes the caller's tensors in the same nesting, (qt, sft) or ((qt, sft), (q, sf)); qt with the row stride aligned_rows asks for."""
    _, lead, groups, rows = _fused_layout(x, masked_m, m_indices, 1, "H")
    return _cast_transposed("dga_cast_to_fp8_1x128_transposed", "per_token_cast_to_fp8_transposed", x, x.shape[-1], lead, groups, rows,
                            masked_m, m_indices, rowwise, aligned_rows, use_ue8m0, out, sync)


def silu_and_mul_per_token_cast_to_fp8_transposed(x: torch.Tensor, masked_m: Optional[torch.Tensor] = None,
                                                  m_indices: Optional[torch.Tensor] = None, rowwise: bool = False,
                                                  aligned_rows: bool = False, use_ue8m0: bool = False, out=None, sync: bool = False):
    """The operand of the weight gradient of an expert MLP's second GEMM, dW2[g] = dout_g^T . h_g with h = silu(x[..., :H]) * x[..., H:],
    from gate_up in one pass (dga_silu_mul_cast_to_fp8_1x128_transposed): per_token_cast_to_fp8_transposed of h, with h kept in fp32
    registers and never written.
      (qt, sft) = per_token_cast_to_fp8(h0.t().contiguous(), aligned_rows, use_ue8m0),  h0 = h with the rows a mask excludes set to +0:
    qt [H, T] float8_e4m3fn, sft [H, ceil(T/128)] float32, T the number of rows of x over all groups.  x [T, 2H], or [G, Mmax, 2H] with
    masked_m int32 [G], or [T, 2H] with m_indices int32 [T] (float32 / bfloat16 / float16, gate first): silu_and_mul_per_token_cast_to_fp8's
    layouts, with per_token_cast_to_fp8_transposed's meaning for the output -- a row a mask excludes is not read and counts as zeros (code
    0, a 128-token block without a valid token has scale 1), and EVERY element of qt and sft is written.  The product is the forward
    quantiser's: for gate >= 20 the result is per_token_cast_to_fp8_transposed's on fl32(gate * up) byte for byte, for |gate| <= 16 the
    fp32 product is within relative 2^-18 of the real-number value and every block amax is rounded from an fp64 value.
    rowwise=True also returns (q, sf) = silu_and_mul_per_token_cast_to_fp8(x, same mask, use_ue8m0), bit for bit, from the same read of x
    on the valid rows (the rows a mask excludes are not written), and the result is ((qt, sft), (q, sf)): a training forward gets the
    operand of its second GEMM and that of dW2 in one pass.  aligned_rows, out=, use_ue8m0, sync: as per_token_cast_to_fp8_transposed."""
    h, lead, groups, rows = _fused_layout(x, masked_m, m_indices, 2)
    return _cast_transposed("dga_silu_mul_cast_to_fp8_1x128_transposed", "silu_and_mul_per_token_cast_to_fp8_transposed", x, h, lead,
                            groups, rows, masked_m, m_indices, rowwise, aligned_rows, use_ue8m0, out, sync)


def silu_and_mul_backward_per_token_cast_to_fp8_transposed(x: torch.Tensor, grad_h: torch.Tensor, masked_m: Optional[torch.Tensor] = None,
                                                           m_indices: Optional[torch.Tensor] = None, rowwise: bool = False,
                                                           aligned_rows: bool = False, use_ue8m0: bool = False, out=None,
                                                           sync: bool = False):
    """The operand of the weight gradient of an expert MLP's first GEMM, dW1[g] = dY1_g^T . x_g with dY1 = [dgate | dup] the backward of
    silu(x[..., :H]) * x[..., H:], from (x, grad_h) in one pass (dga_silu_mul_bwd_cast_to_fp8_1x128_transposed):
    per_token_cast_to_fp8_transposed of dY1, with dY1 kept in fp32 registers and never written.  x [..., 2H] and grad_h [..., H] are
    silu_and_mul_backward_per_token_cast_to_fp8's inputs (one dtype of float32 / bfloat16 / float16, H % 128 == 0, its three row
    layouts) -> qt [2H, T] float8_e4m3fn, sft [2H, ceil(T/128)] float32, T the number of rows over all groups: channels 0 .. H-1 are
    dgate^T, H .. 2H-1 dup^T, the operand k_grouped_wgrad_gemm_fp8_fp8_fp32_nt and wgrad_gemm_fp8_fp8_fp32_nt take as it is.
    The contract is by composition: with G the float32 grad_x_out that silu_and_mul_backward_per_token_cast_to_fp8 writes for
    (x.float(), grad_h.float()) under the same mask,
      (qt, sft) = per_token_cast_to_fp8_transposed(G, same mask, aligned_rows, use_ue8m0)
    byte for byte and bit for bit, for every dtype and every input (NaN, infinities, gate <= -88.8): the gradient that is quantised was
    never rounded to 16 bits, and its accuracy is that entry's.  The output has per_token_cast_to_fp8_transposed's meaning: a row a mask
    excludes is not read and counts as zeros (code 0, a 128-token block without a valid token has scale 1), and EVERY element of qt and
    sft is written.  rowwise=True also returns (dq, dsf) = silu_and_mul_backward_per_token_cast_to_fp8(x, grad_h, same mask, use_ue8m0),
    bit for bit, from the same read on the valid rows (the rows a mask excludes are not written), and the result is
    ((qt, sft), (dq, dsf)): the backward gets the lhs of its dgrad and the operand of dW1 in one pass.  There is no grad_x_out: a caller
    who wants the 16-bit gradient uses silu_and_mul_backward_per_token_cast_to_fp8.  aligned_rows, out=, use_ue8m0, sync: as
    per_token_cast_to_fp8_transposed."""
    h, lead, groups, rows = _fused_layout(x, masked_m, m_indices, 256)
    _want(grad_h, "grad_h", None, lead + (h,))
    _require(grad_h.dtype == x.dtype, "grad_h must have x's dtype")
    call = lambda fn, *outputs: fn(x.data_ptr(), grad_h.data_ptr(), _CAST_DT[x.dtype], groups, rows, h, _ptr(masked_m), _ptr(m_indices),
                                   *outputs)
    return _cast_transposed("dga_silu_mul_bwd_cast_to_fp8_1x128_transposed", "silu_and_mul_backward_per_token_cast_to_fp8_transposed", x,
                            2 * h, lead, groups, rows, masked_m, m_indices, rowwise, aligned_rows, use_ue8m0, out, sync, call=call,
                            also=(grad_h,))


def gather_per_token_cast_to_fp8_transposed(src: torch.Tensor, index: torch.Tensor, index_div: int = 1,
                                            row_scale: Optional[torch.Tensor] = None, masked_m: Optional[torch.Tensor] = None,
                                            rowwise: bool = False, aligned_rows: bool = False, use_ue8m0: bool = False, out=None,
                                            sync: bool = False):
    """The dispatch of an MoE layer fused into per_token_cast_to_fp8_transposed (dga_gather_cast_to_fp8_1x128_transposed): the rows are read
    through a table, and the gathered tensor is never written.  src [S, H] contiguous float32 / bfloat16 / float16, any H >= 1; index int64
    [T], or [G, Mmax] with masked_m int32 [G]; P = S * index_div pairs.  Row r is valid iff masked_m does not exclude it and
    0 <= index[r] < P; an index entry that masked_m excludes is not read (route_slots leaves stale values there), a value outside [0, P)
    excludes the row and dereferences nothing.  A valid row is
      xg[r] = src[index[r] // index_div]                                  (src's dtype)
      xg[r] = row_scale[index[r]] * src[index[r] // index_div].float()    (row_scale: float32, P elements; xg is float32)
    and the result is per_token_cast_to_fp8_transposed(xg, m_indices=where(valid, 0, -1), rowwise, aligned_rows, use_ue8m0), byte for byte
    and bit for bit, with that entry's contract: excluded rows count as zeros and are never read, every element of qt [H, T] and
    sft [H, ceil(T/128)] is written (T = index.numel()), a 128-token block without a valid token has scale 1; rowwise=True also returns
    (q, sf) with index's leading dimensions, written on the valid rows only, and the result is ((qt, sft), (q, sf)); out= takes the same
    nesting; aligned_rows keeps its row stride.  On route_slots(keys = the top-k ids flattened, cap = Mmax): index = inverse.view(G, Mmax),
    index_div = k, masked_m = counts is the lhs of the step's first GEMM (with rowwise) and the operand of dW1; the same call on dY with
    row_scale = w.view(-1) is dOut = w * dY[token], never written; a 1-D index with -1 on the padding rows is the contiguous layout.
    The table is read on the device: a captured graph follows the routing."""
    _require(src.dim() == 2 and src.is_contiguous(), "src must be a contiguous [S, H] tensor")
    _require(src.dtype in _CAST_DT, "src must be float32, bfloat16 or float16")
    _require(isinstance(index_div, int) and index_div >= 1, "index_div must be an integer >= 1")
    want_dim = 2 if masked_m is not None else 1
    _require(index.dtype == torch.int64 and index.dim() == want_dim and index.is_contiguous(),
             "index must be a contiguous int64 [G, Mmax] tensor with masked_m" if masked_m is not None else "index must be a contiguous int64 [T] tensor")
    lead = tuple(index.shape)
    groups, rows = (lead if masked_m is not None else (1, lead[0]))
    _row_masks(masked_m, None, groups, rows)
    s_n, h = src.shape
    if row_scale is not None:
        _require(row_scale.dtype == torch.float32 and row_scale.numel() == s_n * index_div and row_scale.is_contiguous(),
                 "row_scale must be contiguous float32 with %d elements", s_n * index_div)
    call = lambda fn, *outputs: fn(src.data_ptr(), _CAST_DT[src.dtype], s_n, h, index.data_ptr(), index_div, _ptr(row_scale), groups, rows,
                                   _ptr(masked_m), *outputs)
    return _cast_transposed("dga_gather_cast_to_fp8_1x128_transposed", "gather_per_token_cast_to_fp8_transposed", src, h, lead, groups, rows,
                            masked_m, None, rowwise, aligned_rows, use_ue8m0, out, sync, call=call, also=(index, row_scale))


def _combine_layout(src: torch.Tensor, dest: torch.Tensor):
    """The checks combine_tokens and combine_tokens_weight_grad share: src [S, H], dest int64 [T, k] with k >= 1.  Returns (S, H, T, k)."""
    _require(src.dim() == 2 and src.is_contiguous(), "src must be a contiguous [S, H] tensor")
    _require(src.dtype in _CAST_DT, "src must be float32, bfloat16 or float16")
    _require(dest.dtype == torch.int64 and dest.dim() == 2 and dest.is_contiguous() and dest.shape[1] >= 1,
             "dest must be a contiguous int64 [T, k] tensor with k >= 1")
    return src.shape[0], src.shape[1], dest.shape[0], dest.shape[1]


def combine_tokens(src: torch.Tensor, dest: torch.Tensor, weights: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                   sync: bool = False) -> torch.Tensor:
    """The combine of an MoE layer on route_slots' pair -> slot table (dga_combine_rows): y[t] = sum_j weights[t, j] * src[dest[t, j]].
    src [S, H] contiguous float32 / bfloat16 / float16, dest int64 [T, k], weights float32 [T, k] or None, out [T, H] of src's dtype
    (the default) or float32.  Per element, in float32: acc = +0; for j = 0 .. k-1 in that order, where 0 <= dest[t, j] < S,
    acc = fl32(acc + fl32(weights[t, j] * src[dest[t, j], c])) -- two roundings, never a fused multiply-add; without weights the product is
    the value itself -- and out[t, c] = acc rounded to nearest even.  A choice whose dest is outside [0, S) is skipped whatever its weight
    (route_slots marks dropped rows with -1), a token without a valid choice gets a row of +0, and every element of out is written.  The
    definition is numpy float32 arithmetic, so a host reference matches bit for bit.  weights=None is the backward of the dispatch,
    dX[t] = sum_j dX_slots[dest[t, j]]."""
    s_n, h, t_n, k = _combine_layout(src, dest)
    if weights is not None:
        _want(weights, "weights", torch.float32, (t_n, k))
    if out is None:
        out = torch.empty((t_n, h), dtype=src.dtype, device=src.device)
    else:
        _want(out, "out", None, (t_n, h))
        _require(out.dtype in (src.dtype, torch.float32), "out must have src's dtype or float32")
    _launch("combine_tokens", (src, dest, out, weights), lambda L, stream: L.dga_combine_rows(
        src.data_ptr(), _CAST_DT[src.dtype], s_n, h, dest.data_ptr(), _ptr(weights), t_n, k, out.data_ptr(), _CAST_DT[out.dtype], stream), sync)
    return out


def combine_tokens_weight_grad(src: torch.Tensor, grad: torch.Tensor, dest: torch.Tensor, out: Optional[torch.Tensor] = None,
                               sync: bool = False) -> torch.Tensor:
    """The gradient of combine_tokens with respect to its weights (dga_combine_rows_weight_grad): dw[t, j] = <src[dest[t, j]], grad[t]>,
    float32 [T, k].  src [S, H] and grad [T, H] contiguous, of one dtype (float32 / bfloat16 / float16), dest int64 [T, k].  Products and
    sums are float32 in a fixed order -- no floating-point atomics, two runs give the same bits --, |dw - exact| <= (H + 2) 2^-24 sum_c
    |src grad|.  A choice whose dest is outside [0, S) gets +0; every element of dw is written; grad[t] is read once per 8 choices."""
    s_n, h, t_n, k = _combine_layout(src, dest)
    _want(grad, "grad", None, (t_n, h))
    _require(grad.dtype == src.dtype, "grad must have src's dtype")
    if out is None:
        out = torch.empty((t_n, k), dtype=torch.float32, device=src.device)
    else:
        _want(out, "out", torch.float32, (t_n, k))

    def call(L, stream):
        if h == 0:
            out.zero_()   # (the C entry touches nothing for an empty row)
        return L.dga_combine_rows_weight_grad(src.data_ptr(), grad.data_ptr(), _CAST_DT[src.dtype], s_n, h, dest.data_ptr(), t_n, k,
                                              out.data_ptr(), stream)
    _launch("combine_tokens_weight_grad", (src, grad, dest, out), call, sync)
    return out


_SCORE_FUNCS = {"softmax": _lib.ROUTER_SOFTMAX, "sigmoid": _lib.ROUTER_SIGMOID}


def _router_func(score_func) -> int:
    _require(score_func in _SCORE_FUNCS, 'score_func must be "softmax" or "sigmoid"')
    return _SCORE_FUNCS[score_func]


def _dlogits_out(out: Optional[torch.Tensor], t_n: int, e: int, device) -> torch.Tensor:
    """dlogits [T, E] of the two backward entries: float32 from torch.empty, or the caller's out in any of the three float types."""
    if out is None:
        return torch.empty((t_n, e), dtype=torch.float32, device=device)
    _require(out.dtype in _CAST_DT and tuple(out.shape) == (t_n, e) and out.is_contiguous(),
             "out must be contiguous [%d, %d], float32, bfloat16 or float16", t_n, e)
    return out


def router_topk(logits: torch.Tensor, k: int, score_func: str = "softmax", bias: Optional[torch.Tensor] = None, n_groups: int = 1,
                topk_groups: int = 1, renormalize: bool = True, scale: float = 1.0, out=None, sync: bool = False):
    """The gate of an MoE layer in one launch (dga_router_topk): logits [T, E] contiguous float32 / bfloat16 / float16 ->
    (ids int32 [T, k], weights float32 [T, k], scores float32 [T, E]).  1 <= k <= E <= 1024, k <= 64, E % n_groups == 0,
    1 <= topk_groups <= n_groups, topk_groups * (E / n_groups) >= k, groups of at least two experts when n_groups > 1.
    scores = softmax(logits) or sigmoid(logits) row by row, in float32 against float64: |p - p64| <= (E + 128) 2^-24 p64 where
    |x_i - max x| <= 16 (softmax), |s - s64| <= 2^-18 s64 where |x| <= 16 (sigmoid).  ids and weights are exact float32 functions of the
    scores returned, so a numpy float32 reference on those scores matches bit for bit: sel = fl32(scores + bias) (bias float32 [E],
    DeepSeek-V3's correction bias: selection only; a NaN sel counts as -inf); comparisons are IEEE >, equal values tie and the lower index
    wins; with n_groups > 1 a group's value is fl32(largest sel + second largest sel) of its experts, the topk_groups largest groups stay
    (ties: the lower group) and no expert of another group is chosen; ids[t] = the k largest sel of what may be chosen, in descending
    order -- always k distinct values in [0, E), whatever the logits hold; r_j = scores[t, ids[t, j]]; renormalize:
    D = ((r_0 + r_1) + ...) + r_{k-1}, w_j = fl32(fl32(r_j / D) * scale), else w_j = fl32(r_j * scale).  A row with a NaN or +inf, or
    of nothing but -inf, may give NaN scores and weights.  out=(ids, weights, scores) takes the caller's tensors; every element of all three
    is written.  ids.view(-1) is route_slots' keys (key_stride_bytes=4), weights feeds combine_tokens and row_scale=weights.view(-1) as it
    is, scores is what router_topk_backward (and a balance loss) reads.  Nothing depends on the host: a captured graph follows the logits."""
    _require(logits.dim() == 2 and logits.is_contiguous(), "logits must be a contiguous [T, E] tensor")
    _require(logits.dtype in _CAST_DT, "logits must be float32, bfloat16 or float16")
    func = _router_func(score_func)
    _require(all(isinstance(v, int) for v in (k, n_groups, topk_groups)), "k, n_groups and topk_groups must be integers")
    t_n, e = logits.shape
    if bias is not None:
        _want(bias, "bias", torch.float32, (e,))
    if out is None:
        _require(k >= 1, "k must be >= 1")
    ids, weights, scores = _outputs(out, (("ids", torch.int32, (t_n, k)), ("weights", torch.float32, (t_n, k)), ("scores", torch.float32, (t_n, e))),
                                    logits.device, "out must hold (ids, weights, scores)")
    _launch("router_topk", (logits, ids, weights, scores, bias), lambda L, stream: L.dga_router_topk(
        logits.data_ptr(), _CAST_DT[logits.dtype], t_n, e, k, func, _ptr(bias), n_groups, topk_groups, _lib.ROUTER_RENORMALIZE if renormalize else 0,
        float(scale), ids.data_ptr(), weights.data_ptr(), scores.data_ptr(), stream), sync)
    return ids, weights, scores


def router_topk_backward(dw: torch.Tensor, scores: torch.Tensor, ids: torch.Tensor, score_func: str, renormalize: bool = True,
                         scale: float = 1.0, out: Optional[torch.Tensor] = None, sync: bool = False) -> torch.Tensor:
    """The backward of router_topk (dga_router_topk_backward): dw float32 [T, k] (combine_tokens_weight_grad's output), scores float32
    [T, E] and ids int32 [T, k] as the forward wrote them -> dlogits [T, E], float32 by default or bfloat16 / float16 through out (rounded
    to nearest even); every element is written.  bias and the choice of groups get no gradient.  With r_j = scores[t, ids[t, j]] and D, w
    as in the forward: g_j = (scale dw_j - sum_l dw_l w_l) / D with renormalize, else scale dw_j; ds_i = g_j at i = ids[t, j], else 0;
    sigmoid: dlogits_i = ds_i s_i (1 - s_i), +0 off the selection; softmax: dlogits_i = s_i (ds_i - sum_l ds_l s_l).  float32 in a fixed
    order without atomics -- two runs give the same bits --, |dlogits - ref64| <= (E + k + 8) 2^-24 M against float64 on the same scores,
    M the same expression with every term replaced by its absolute value and (1 - s_i) by 1."""
    func = _router_func(score_func)
    _require(scores.dtype == torch.float32 and scores.dim() == 2 and scores.is_contiguous(), "scores must be a contiguous float32 [T, E] tensor")
    t_n, e = scores.shape
    _require(ids.dtype == torch.int32 and ids.dim() == 2 and ids.shape[0] == t_n and ids.is_contiguous(),
             "ids must be a contiguous int32 [%d, k] tensor", t_n)
    k = ids.shape[1]
    _want(dw, "dw", torch.float32, (t_n, k))
    out = _dlogits_out(out, t_n, e, scores.device)
    _launch("router_topk_backward", (scores, dw, ids, out), lambda L, stream: L.dga_router_topk_backward(
        dw.data_ptr(), scores.data_ptr(), ids.data_ptr(), t_n, e, k, func, _lib.ROUTER_RENORMALIZE if renormalize else 0, float(scale),
        out.data_ptr(), _CAST_DT[out.dtype], stream), sync)
    return out


def _balance_shape(scores: torch.Tensor, k, seq_len, alpha) -> Tuple[int, int, int, int, float]:
    """The checks the balance entries share -> (T, E, L, B, coef); coef = alpha E / (k L^2), formed in double."""
    _require(scores.dtype == torch.float32 and scores.dim() == 2 and scores.is_contiguous(), "scores must be a contiguous float32 [T, E] tensor")
    t_n, e = scores.shape
    seq = (t_n if t_n else 1) if seq_len is None else seq_len
    _require(isinstance(k, int) and isinstance(seq, int) and k >= 1 and seq >= 1, "k and seq_len must be integers >= 1")
    _require(t_n % seq == 0, "seq_len must divide the %d tokens", t_n)
    return t_n, e, seq, t_n // seq, float(alpha) * e / (float(k) * seq * seq)


def router_balance_loss_workspace_bytes(tokens: int, experts: int, seq_len: Optional[int] = None) -> int:
    """Bytes of scratch router_balance_loss takes for this shape (dga_router_balance_loss_workspace_bytes): 8 B chunks E, one float32 and
    one int32 partial [E] for each chunk of max(16, 4 ceil(T / 2048)) consecutive tokens of each of the B = T / seq_len segments."""
    return int(_lib.lib().dga_router_balance_loss_workspace_bytes(tokens, experts, tokens if seq_len is None else seq_len))


def router_balance_loss(scores: torch.Tensor, ids: torch.Tensor, seq_len: Optional[int] = None, alpha: float = 1.0, normalize: bool = False,
                        out=None, sync: bool = False):
    """The load-balancing loss of a router on router_topk's outputs (dga_router_balance_loss): scores float32 [T, E], ids int32 [T, k] ->
    (loss float32 [B], counts int32 [B, E], psum float32 [B, E]) over B = T / seq_len segments of seq_len consecutive tokens (the default,
    seq_len = T, is Switch / GShard's global loss; seq_len = a sequence's length is DeepSeek-V3's sequence-wise loss).  For segment b:
    counts[b, e] = the pairs (t, j) of the segment with ids[t, j] == e, exact (an id outside [0, E) counts nowhere); p[t, e] =
    scores[t, e] / sum_e scores[t, e] with normalize, else scores[t, e]; psum[b, e] = sum_t p[t, e]; loss[b] = coef sum_e counts psum
    with coef = alpha E / (k seq_len^2) -- alpha sum_e f_e P_e, f_e = E / (k L) counts, P_e = psum / L.  In float32 against float64 on
    the same scores, u = 2^-24, gamma(n) = n u / (1 - n u): |psum - P64| <= gamma(L + E + 1) P64, |loss - loss64| <= gamma(L + 2 E + 4)
    loss64.  A NaN score makes its own segment's loss NaN and touches no other.  Fixed-order sums, no floating-point atomics: two runs give
    the same bits.  out=(loss, counts, psum) takes the caller's tensors; every element of all three is written.  Nothing depends on the
    host: the entry can be captured.  1 <= k <= E <= 1024, k <= 64."""
    _require(ids.dtype == torch.int32 and ids.dim() == 2 and ids.is_contiguous(), "ids must be a contiguous int32 [T, k] tensor")
    t_n, e, seq, b_n, coef = _balance_shape(scores, ids.shape[1], seq_len, alpha)
    _require(ids.shape[0] == t_n, "ids must hold %d rows", t_n)
    loss, counts, psum = _outputs(out, (("loss", torch.float32, (b_n,)), ("counts", torch.int32, (b_n, e)), ("psum", torch.float32, (b_n, e))),
                                  scores.device, "out must hold (loss, counts, psum)")

    def call(L, stream):
        ws_ptr, ws_bytes = _scratch("balance", scores.device, int(L.dga_router_balance_loss_workspace_bytes(t_n, e, seq)))
        return L.dga_router_balance_loss(scores.data_ptr(), ids.data_ptr(), t_n, e, ids.shape[1], seq, _lib.ROUTER_BALANCE_NORMALIZE if normalize else 0,
                                         coef, loss.data_ptr(), counts.data_ptr(), psum.data_ptr(), ws_ptr, ws_bytes, stream)
    _launch("router_balance_loss", (scores, ids, loss, counts, psum), call, sync)
    return loss, counts, psum


def router_balance_loss_backward(dloss: torch.Tensor, counts: torch.Tensor, scores: torch.Tensor, k: int, score_func: str,
                                 seq_len: Optional[int] = None, alpha: float = 1.0, normalize: bool = False,
                                 add_to: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, sync: bool = False) -> torch.Tensor:
    """The backward of router_balance_loss into the logits (dga_router_balance_loss_backward): dloss float32 [B], counts int32 [B, E] and
    scores float32 [T, E] as the forward took and wrote them (the counts carry no gradient), k, seq_len, alpha and normalize as in the
    forward -> dlogits [T, E], float32 by default or bfloat16 / float16 through out (rounded to nearest even); every element is written.
    q[b, e] = dloss[b] coef counts[b, e]; ds[t, i] = (q_i - sum_e q_e p_e) / S_t with normalize, else q_i; sigmoid: aux_i = ds_i s_i
    (1 - s_i); softmax: aux_i = s_i (ds_i - sum_e ds_e s_e).  |aux - ref64| <= gamma(4 E + 8) M against float64 on the same inputs, M the
    same expression with every term replaced by its absolute value and (1 - s_i) by 1.  add_to (float32 [T, E], what router_topk_backward
    wrote; it may be out itself): the result is fl32(add_to + aux), bit for bit the sum of add_to and the entry's own float32 result
    without it, so the step's dlogits is complete after this call.  One wave per token, fixed order, no atomics."""
    func = _router_func(score_func)
    t_n, e, seq, b_n, coef = _balance_shape(scores, k, seq_len, alpha)
    _want(dloss, "dloss", torch.float32, (b_n,))
    _want(counts, "counts", torch.int32, (b_n, e))
    if add_to is not None:
        _want(add_to, "add_to", torch.float32, (t_n, e))
    out = _dlogits_out(out, t_n, e, scores.device)
    _launch("router_balance_loss_backward", (scores, dloss, counts, out, add_to), lambda L, stream: L.dga_router_balance_loss_backward(
        dloss.data_ptr(), counts.data_ptr(), scores.data_ptr(), t_n, e, k, seq, func, _lib.ROUTER_BALANCE_NORMALIZE if normalize else 0, coef,
        _ptr(add_to), out.data_ptr(), _CAST_DT[out.dtype], stream), sync)
    return out


def router_bias_update(bias: torch.Tensor, counts: torch.Tensor, rate: float, sync: bool = False) -> torch.Tensor:
    """DeepSeek-V3's auxiliary-loss-free balancing step, in place on router_topk's bias float32 [E] (dga_router_bias_update), from
    router_balance_loss's counts int32 [B, E]: n_e = sum_b counts[b, e]; sgn_e = sign(sum_e' n_e' - E n_e), compared as integers (+1 below
    the mean load, -1 above, 0 exactly at it); bias[e] = fl32(bias[e] + fl32(rate sgn_e)), which numpy float32 reproduces bit for bit.
    One small launch, capturable: the next router_topk reads the new bias.  Returns bias."""
    _require(bias.dtype == torch.float32 and bias.dim() == 1 and bias.is_contiguous(), "bias must be a contiguous float32 [E] tensor")
    e = bias.shape[0]
    _require(counts.dtype == torch.int32 and counts.dim() == 2 and counts.shape[1] == e and counts.is_contiguous(),
             "counts must be a contiguous int32 [B, %d] tensor", e)
    _launch("router_bias_update", (bias, counts), lambda L, stream: L.dga_router_bias_update(
        bias.data_ptr(), counts.data_ptr(), counts.shape[0], e, float(rate), stream), sync)
    return bias


RmsNormCast = collections.namedtuple("RmsNormCast", ("q", "sf", "norm", "residual", "rstd"))
RMS_NORM_MAX_H = 16384


def _norm_operands(x: torch.Tensor, weight: torch.Tensor, what: str) -> Tuple[int, int]:
    """The row tensor and the weight the two norm entries share, checked -> (T, H)."""
    _require(x.dim() == 2 and x.is_contiguous(), "%s must be a contiguous [T, H] tensor", what)
    _require(x.dtype in _CAST_DT, "%s must be float32, bfloat16 or float16", what)
    t_n, h = x.shape
    _require(1 <= h <= RMS_NORM_MAX_H, "H must be in [1, %d]", RMS_NORM_MAX_H)
    _want(weight, "weight", (x.dtype, torch.float32), (h,))
    return t_n, h


def rms_norm_per_token_cast_to_fp8(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-6, residual: Optional[torch.Tensor] = None,
                                   quantize: bool = True, norm_out: bool = False, out=None, use_ue8m0: bool = False,
                                   sync: bool = False) -> RmsNormCast:
    """The norm in front of an MoE block fused into the quantiser of what reads it (dga_rms_norm_cast_to_fp8_1x128): x [T, H] contiguous
    float32 / bfloat16 / float16, weight [H] of x's dtype or float32, residual None or like x, 1 <= H <= 16384, eps >= 0 finite -> the named
    tuple (q, sf, norm, residual, rstd), None for what was not asked.  Per row, in float32, every operation rounded on its own:
      z = x, or with residual the STORED residual out = RNE(fl(x + residual)) -- what rms_norm_backward reads;
      rstd ~ (mean(z^2) + eps)^(-1/2), float32 [T], always returned: |rstd - exact| <= (H / 2 + 6) 2^-24 exact against float64 on z, its sum
      in an order (H, dtype) alone fixes -- a row's result does not depend on T or on where the row sits, and two runs give the same bits;
      y = fl(fl(z rstd) weight), a NaN replaced by the one NaN 0x7FC00000;  norm = RNE(y) in x's dtype (norm_out=True);
      (q, sf) = per_token_cast_to_fp8(y, use_ue8m0=...) on the float32 y, byte for byte (quantize=True): y never passes through 16 bits.
    Everything below rstd is an exact float32 function of the rstd returned.  Nothing is rescaled: squares that overflow give rstd = 0 and
    y = +-0; a NaN makes its own row's rstd NaN and its codes 0x7F and touches no other row.  One of quantize and norm_out must be set
    (norm_out alone is a fused add + RMSNorm).  out: a mapping or an RmsNormCast with the caller's tensors under the same names (q uint8
    or float8_e4m3fn; residual may be the input residual or x: in place); what it leaves out is allocated.  One launch, capturable."""
    t_n, h = _norm_operands(x, weight, "x")
    if residual is not None:
        _want(residual, "residual", x.dtype, (t_n, h))
    eps = float(eps)
    _require(eps >= 0.0 and eps != float("inf"), "eps must be finite and >= 0")
    _require(quantize or norm_out, "one of quantize and norm_out must be set")
    given = {} if out is None else out._asdict() if isinstance(out, RmsNormCast) else out
    _require(isinstance(given, dict) and all(k in RmsNormCast._fields and (v is None or isinstance(v, torch.Tensor)) for k, v in given.items()),
             "out must map q, sf, norm, residual, rstd to tensors")
    asked = {"q": quantize, "sf": quantize, "norm": norm_out, "residual": residual is not None, "rstd": True}
    specs = {"q": (torch.uint8, (t_n, h)), "sf": (torch.float32, (t_n, (h + 127) // 128)), "norm": (x.dtype, (t_n, h)),
             "residual": (x.dtype, (t_n, h)), "rstd": (torch.float32, (t_n,))}
    o = {}
    for name, (dtype, shape) in specs.items():
        t = given.get(name)
        if not asked[name]:
            _require(t is None, "out %s is given but not asked for", name)
            o[name] = None
        elif t is None:
            o[name] = torch.empty(shape, dtype=dtype, device=x.device)
        else:
            if name == "q":
                _fp8_bytes(t)
            _want(t, name, None if name == "q" else dtype, shape, "out ")
            o[name] = t
    _launch("rms_norm_per_token_cast_to_fp8", (x, weight, residual) + tuple(o.values()), lambda L, stream: L.dga_rms_norm_cast_to_fp8_1x128(
        x.data_ptr(), _ptr(residual), _CAST_DT[x.dtype], weight.data_ptr(), _CAST_DT[weight.dtype], t_n, h, eps, _ptr(o["q"]), _ptr(o["sf"]),
        _ptr(o["norm"]), _ptr(o["residual"]), o["rstd"].data_ptr(), _lib.CAST_UE8M0 if use_ue8m0 else 0, stream), sync)
    if o["q"] is not None:
        o["q"] = _as_fp8(o["q"])
    return RmsNormCast(**o)


def rms_norm_backward_workspace_bytes(rows: int, h: int) -> int:
    """Bytes of scratch rms_norm_backward takes for dweight (dga_rms_norm_backward_workspace_bytes): 4 chunks H, one float32 partial [H] for
    each chunk of max(8, ceil(T / 1024)) consecutive rows."""
    return int(_lib.lib().dga_rms_norm_backward_workspace_bytes(rows, h))


def rms_norm_backward(grad_y: torch.Tensor, z: torch.Tensor, weight: torch.Tensor, rstd: torch.Tensor,
                      grad_residual: Optional[torch.Tensor] = None, out=None, out_dtype: Optional[torch.dtype] = None,
                      need_dweight: bool = True, sync: bool = False):
    """The backward of rms_norm_per_token_cast_to_fp8's norm (dga_rms_norm_backward): grad_y and z [T, H] of one dtype, z what the forward
    normalised (x, or its residual output), weight as in the forward, rstd float32 [T] the forward's own -> (dx, dweight).  With
    x^ = z rstd, g = grad_y weight, c = sum_i g_i x^_i / H:  dx = rstd (g - x^ c), in z's dtype or float32 (out_dtype, or out's);
    dweight[j] = sum_t grad_y[t, j] x^[t, j], float32 [H], overwritten (None with need_dweight=False).  All in float32; against float64 on the
    same inputs, u = 2^-24, A = sum_i |g_i x^_i| / H:  |dx - exact| <= u rstd (4 |g| + |x^| (6 |c| + (H + 8) A)) for the float32 dx, of
    which the 16-bit dx is the RNE;  |dweight - exact| <= (T + 4) u sum_t |grad_y x^|.  grad_residual (dx's dtype and shape, the gradient
    arriving on the residual stream; it may be out's dx itself): dx = RNE(fl(dx + grad_residual)), bit for bit the separate sum.  Every sum
    runs in an order (T, H, dtype) alone fixes, without floating-point atomics: two runs give the same bits, and a row's dx does not depend
    on where the row sits.  out=(dx, dweight) takes the caller's tensors (dweight None with need_dweight=False).  Capturable."""
    t_n, h = _norm_operands(z, weight, "z")
    _want(grad_y, "grad_y", z.dtype, (t_n, h))
    _want(rstd, "rstd", torch.float32, (t_n,))
    dx = dweight = None
    if out is not None:
        _require(isinstance(out, (tuple, list)) and len(out) == 2 and isinstance(out[0], torch.Tensor)
                 and (isinstance(out[1], torch.Tensor) if need_dweight else out[1] is None), "out must be (dx, dweight)")
        dx, dweight = out
        _require(out_dtype is None or out_dtype == dx.dtype, "out_dtype contradicts out")
    dx_dtype = dx.dtype if dx is not None else z.dtype if out_dtype is None else out_dtype
    _require(dx_dtype in (z.dtype, torch.float32), "dx must be of z's dtype or float32")
    if dx is None:
        dx = torch.empty((t_n, h), dtype=dx_dtype, device=z.device)
    else:
        _want(dx, "dx", dx_dtype, (t_n, h), "out ")
    if need_dweight and dweight is None:
        dweight = torch.empty((h,), dtype=torch.float32, device=z.device)
    elif need_dweight:
        _want(dweight, "dweight", torch.float32, (h,), "out ")
    if grad_residual is not None:
        _want(grad_residual, "grad_residual", dx_dtype, (t_n, h))

    def call(L, stream):
        ws_ptr, ws_bytes = _scratch("rms_norm", z.device, int(L.dga_rms_norm_backward_workspace_bytes(t_n, h)) if need_dweight else 0)
        return L.dga_rms_norm_backward(grad_y.data_ptr(), z.data_ptr(), _CAST_DT[z.dtype], weight.data_ptr(), _CAST_DT[weight.dtype],
                                       rstd.data_ptr(), _ptr(grad_residual), t_n, h, dx.data_ptr(), _CAST_DT[dx_dtype], _ptr(dweight), ws_ptr,
                                       ws_bytes, stream)
    _launch("rms_norm_backward", (z, grad_y, weight, rstd, grad_residual, dx, dweight), call, sync)
    return dx, dweight


def per_block_cast_to_fp8_transposed(w: torch.Tensor, rowwise: bool = False, use_ue8m0: bool = False, out=None, sync: bool = False):
    """per_block_cast_to_fp8 of the transposes of grouped expert weights in one pass (dga_cast_to_fp8_128x128_transposed): the rhs of dgrad,
    and with rowwise=True the rhs of fprop too, from the master weights -- no loop over the experts, no w[g].t().contiguous(), no stack.
      (qt[g], sft[g]) = per_block_cast_to_fp8(w[g].t().contiguous(), use_ue8m0=use_ue8m0)   for every g, byte for byte and bit for bit,
    w [G, N, K] contiguous, float32 / bfloat16 / float16 -> qt [G, K, N] float8_e4m3fn, sft [G, ceil(K/128), ceil(N/128)] float32.  A 2-D
    w [N, K] gives 2-D results.  (A 128x128 block's amax does not change under transposition: these are per_block_cast_to_fp8(w[g])'s codes
    and scales transposed, and no scale block mixes two experts, whatever N is.)
    rowwise=True also returns (q[g], sf[g]) = per_block_cast_to_fp8(w[g], use_ue8m0=use_ue8m0) from the same read of w, q [G, N, K],
    sf [G, ceil(N/128), ceil(K/128)], and the result is ((qt, sft), (q, sf)).  out= takes the caller's tensors in the same nesting,
    (qt, sft) or ((qt, sft), (q, sf)), codes uint8 or float8_e4m3fn, all contiguous and of exactly these shapes; every element of every
    output is written.  The results are what the grouped GEMM entries (and, 2-D, gemm_fp8_fp8_bf16_nt) take as rhs as they are."""
    _require(w.dim() in (2, 3) and w.is_contiguous(), "w must be a contiguous [N, K] or [G, N, K] tensor")
    _require(w.dtype in _CAST_DT, "w must be float32, bfloat16 or float16")
    lead = tuple(w.shape[:-2])
    groups = lead[0] if lead else 1
    n, k = w.shape[-2:]
    nb, kb = (n + 127) // 128, (k + 127) // 128
    out_t, out_r = _nested_out(out, rowwise)
    qt, sft = _outputs(out_t, (("qt", torch.uint8, lead + (k, n)), ("sft", torch.float32, lead + (kb, nb))), w.device, "out must hold (qt, sft)")
    q, sf = _outputs(out_r, (("q", torch.uint8, lead + (n, k)), ("sf", torch.float32, lead + (nb, kb))), w.device,
                     "out must hold (q, sf)") if rowwise else (None, None)
    _launch("per_block_cast_to_fp8_transposed", (w, qt, sft, q, sf), lambda L, stream: L.dga_cast_to_fp8_128x128_transposed(
        w.data_ptr(), _CAST_DT[w.dtype], groups, n, k, qt.data_ptr(), sft.data_ptr(), _ptr(q), _ptr(sf), _lib.CAST_UE8M0 if use_ue8m0 else 0,
        stream), sync)
    return ((_as_fp8(qt), sft), (_as_fp8(q), sf)) if rowwise else (_as_fp8(qt), sft)


def adamw_step_scalars(step: int, lr: float, beta1: float, beta2: float, grad_scale: float = 1.0, out: Optional[torch.Tensor] = None,
                       device=None) -> torch.Tensor:
    """What adamw_per_block_cast_to_fp8_transposed reads of a step: float32 [4] = {lr, bc1, bc2s, grad_scale} with bc1 = 1 - beta1^step and
    bc2s = sqrt(1 - beta2^step), formed on the host in float64 and rounded once to float32.  step >= 1.  grad_scale is where a caller puts
    1 / loss_scale or a clip coefficient.  Without out= a new tensor on `device` (default: the current HIP device, the host without one); with
    out= (contiguous float32 [4], any device) the values are copied into it on the current stream, which is how a captured graph is given
    its next step."""
    step = int(step)
    _require(step >= 1, "step must be >= 1")
    b1, b2 = float(beta1), float(beta2)
    _require(0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0, "beta1 and beta2 must be in [0, 1)")
    host = torch.tensor([float(lr), 1.0 - b1 ** step, (1.0 - b2 ** step) ** 0.5, float(grad_scale)], dtype=torch.float64).to(torch.float32)
    if out is None:
        return host.to(device if device is not None else "cuda" if torch.cuda.is_available() else "cpu")
    _require(isinstance(out, torch.Tensor), "out must be a tensor")
    _want(out, "step_scalars", torch.float32, (4,), "out ")
    out.copy_(host)
    return out


def adamw_per_block_cast_to_fp8_transposed(w: torch.Tensor, m: torch.Tensor, v: torch.Tensor, grad: torch.Tensor, step_scalars: torch.Tensor,
                                           beta1: float = 0.9, beta2: float = 0.95, eps: float = 1e-8, weight_decay: float = 0.0,
                                           rowwise: bool = False, use_ue8m0: bool = False, out=None, sync: bool = False,
                                           skip: Optional[torch.Tensor] = None):
    """The optimizer step of grouped expert weights and per_block_cast_to_fp8_transposed of the result in one pass
    (dga_adamw_cast_to_fp8_128x128_transposed): w [G, N, K] or [N, K] contiguous float32 master weights, m and v like w and both float32 or
    both bfloat16, grad like w in float32 or bfloat16 (read only), step_scalars a contiguous float32 [4] DEVICE tensor {lr, bc1, bc2s,
    grad_scale} (adamw_step_scalars) that the kernel reads -- nothing of a step's changing state is a launch argument, so one captured graph
    runs weight gradient -> optimizer -> the next forward at every step.  w, m and v are updated in place; no two of w, m, v and grad may
    share memory.  Per element in float32, every
    operation rounded on its own, beta1, beta2, eps and weight_decay rounded to float32 first:
      g   = fl(grad grad_scale)
      m'  = fl(fl(beta1 m) + fl(fl(1 - beta1) g))
      v'  = fl(fl(beta2 v) + fl(fl(fl(1 - beta2) g) g))
      den = fl(fl(sqrt(v') / bc2s) + eps)
      w'  = fl(fl(w fl(1 - fl(lr weight_decay))) - fl(fl(lr / bc1) fl(m' / den)))
    with IEEE square root and division and subnormals kept: numpy in float32 reproduces w', m' and v' bit for bit.  m' and v' are stored
    round-to-nearest-even in their dtype, the update uses the unrounded ones.  Returns (qt, sft), or with rowwise ((qt, sft), (q, sf)):
    exactly per_block_cast_to_fp8_transposed(w, rowwise=..., use_ue8m0=...) on the w the call leaves behind, byte for byte; out= as there.
    A NaN or infinite gradient poisons its own element of w, m and v only; eps = 0 with v' = 0 gives NaN, as torch does.
    skip (a contiguous int32 [1] device tensor, typically grad_clip_scalars', read by the kernel): where skip[0] != 0 nothing is stored to w,
    m and v -- their bits stay, whatever grad holds -- and the codes are per_block_cast_to_fp8_transposed of the unchanged w, every element
    of every output written; where it is 0, and without skip, every bit of every result is the same as ever.  The step number stays the
    caller's: it reads skip back when convenient and does not advance step after a skipped one."""
    _require(isinstance(w, torch.Tensor) and w.dim() in (2, 3) and w.is_contiguous() and w.dtype == torch.float32,
             "w must be a contiguous float32 [N, K] or [G, N, K] tensor")
    shape = tuple(w.shape)
    moments = (torch.float32, torch.bfloat16)
    for t, what in ((m, "m"), (v, "v"), (grad, "grad"), (step_scalars, "step_scalars")):
        _require(isinstance(t, torch.Tensor), "%s must be a tensor", what)
    _want(m, "m", moments, shape)
    _want(v, "v", moments, shape)
    _require(m.dtype == v.dtype, "m and v must be of one dtype")
    _want(grad, "grad", moments, shape)
    _want(step_scalars, "step_scalars", torch.float32, (4,))
    # (updated in place, a lane's elements read before they are written: two of them on the same memory would make the result depend on
    # the order of the workgroups)
    spans = [(what, t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) for t, what in ((w, "w"), (m, "m"), (v, "v"), (grad, "grad"))]
    for i, (a, a0, a1) in enumerate(spans):
        for b, b0, b1 in spans[i + 1:]:
            _require(a0 >= b1 or b0 >= a1, "%s and %s must not share memory", a, b)
    b1, b2, e, wd = (ctypes.c_float(float(x)).value for x in (beta1, beta2, eps, weight_decay))
    _require(0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0, "beta1 and beta2 must be in [0, 1) as float32")
    _require(0.0 <= e < float("inf") and 0.0 <= wd < float("inf"), "eps and weight_decay must be finite and >= 0")
    if skip is not None:
        _require(isinstance(skip, torch.Tensor), "skip must be a tensor")
        _want(skip, "skip", torch.int32, (1,))
    lead = shape[:-2]
    groups = lead[0] if lead else 1
    n, k = shape[-2:]
    nb, kb = (n + 127) // 128, (k + 127) // 128
    out_t, out_r = _nested_out(out, rowwise)
    qt, sft = _outputs(out_t, (("qt", torch.uint8, lead + (k, n)), ("sft", torch.float32, lead + (kb, nb))), w.device, "out must hold (qt, sft)")
    q, sf = _outputs(out_r, (("q", torch.uint8, lead + (n, k)), ("sf", torch.float32, lead + (nb, kb))), w.device,
                     "out must hold (q, sf)") if rowwise else (None, None)
    _launch("adamw_per_block_cast_to_fp8_transposed", (w, m, v, grad, step_scalars, qt, sft, q, sf, skip),
            lambda L, stream: L.dga_adamw_cast_to_fp8_128x128_transposed_skip(
                w.data_ptr(), m.data_ptr(), v.data_ptr(), _CAST_DT[m.dtype], grad.data_ptr(), _CAST_DT[grad.dtype], step_scalars.data_ptr(),
                b1, b2, e, wd, groups, n, k, qt.data_ptr(), sft.data_ptr(), _ptr(q), _ptr(sf), _lib.CAST_UE8M0 if use_ue8m0 else 0,
                _ptr(skip), stream), sync)
    return ((_as_fp8(qt), sft), (_as_fp8(q), sf)) if rowwise else (_as_fp8(qt), sft)


GradClip = collections.namedtuple("GradClip", ("norm", "coef", "skip"))
GradClipNorm = collections.namedtuple("GradClipNorm", ("norm", "coef", "skip", "sumsq"))
_GRAD_DT = {torch.float32: _lib.DT_FP32, torch.bfloat16: _lib.DT_BF16}


def grad_sumsq_workspace_bytes(numels: Sequence[int]) -> int:
    """Bytes of device scratch grad_sumsq needs for tensors of these element counts (dga_grad_sumsq_workspace_bytes): one float64 partial
    per chunk of 16384 consecutive elements of one tensor; 0 for a list the entry refuses."""
    numels = [int(x) for x in numels]
    return int(_lib.lib().dga_grad_sumsq_workspace_bytes(len(numels), (ctypes.c_int64 * max(len(numels), 1))(*numels)))


def _sumsq_args(tensors, out, accumulate: bool):
    """grad_sumsq's checks -> (the list, out or None)."""
    if isinstance(tensors, torch.Tensor):
        tensors = (tensors,)
    _require(isinstance(tensors, (list, tuple)) and len(tensors) > 0, "tensors must be a tensor or a non-empty list or tuple of tensors")
    for i, t in enumerate(tensors):
        _require(isinstance(t, torch.Tensor) and t.dtype in _GRAD_DT and t.is_contiguous(),
                 "tensors[%d] must be a contiguous float32 or bfloat16 tensor", i)
    if out is not None:
        _require(isinstance(out, torch.Tensor), "out must be a tensor")
        _want(out, "sumsq", torch.float64, (1,), "out ")
    _require(out is not None or not accumulate, "accumulate=True needs out=")
    return tensors, out


def _sumsq_run(tensors, out, accumulate: bool, sync: bool) -> torch.Tensor:
    count = len(tensors)
    if out is None:
        out = torch.empty((1,), dtype=torch.float64, device=tensors[0].device)
    ptrs = (ctypes.c_void_p * count)(*[t.data_ptr() for t in tensors])
    numel = (ctypes.c_int64 * count)(*[t.numel() for t in tensors])
    dts = (ctypes.c_int * count)(*[_GRAD_DT[t.dtype] for t in tensors])

    def call(L, stream):
        ws_ptr, ws_bytes = _scratch("grad_sumsq", out.device, int(L.dga_grad_sumsq_workspace_bytes(count, numel)))
        return L.dga_grad_sumsq(ptrs, numel, dts, count, out.data_ptr(), 1 if accumulate else 0, ws_ptr, ws_bytes, stream)
    _launch("grad_sumsq", (out,) + tuple(tensors), call, sync)
    return out


def grad_sumsq(tensors, out: Optional[torch.Tensor] = None, accumulate: bool = False, sync: bool = False) -> torch.Tensor:
    """The sum of squares of a list of gradient tensors as a float64 [1] device tensor (dga_grad_sumsq): tensors is a tensor or a non-empty
    list or tuple of contiguous float32 or bfloat16 device tensors of any shape (numel == 0 included; the dtypes may be mixed; float16 is
    refused, as by the optimizer), all on one device.  sumsq[0] = sum_i sum_e x_i[e]^2 with every product and every sum in float64: the
    squares are exact and can neither overflow nor underflow, subnormals are kept, and  |sumsq - exact| <= (n + 1) 2^-53 exact  for n
    elements.  A NaN or an infinity anywhere makes sumsq non-finite and nothing else can, so isfinite(sumsq) is the overflow check of a
    loss-scaled step.  The order of the additions is fixed by the list of (numel, dtype) alone, without floating-point atomics: two runs
    give the same bits, wherever the tensors lie.  out= takes the caller's float64 [1]; accumulate=True (with out=) adds out[0] last,
    fl64(out[0] + sum), so that several calls build one sum.  Nothing is read back, the scratch is the module's: capturable."""
    tensors, out = _sumsq_args(tensors, out, accumulate)
    return _sumsq_run(tensors, out, accumulate, sync)


def _clip_args(step_scalars, max_norm, pre_scale, eps):
    """grad_clip_scalars' checks behind sumsq's -> max_norm, pre_scale and eps as floats."""
    _require(isinstance(step_scalars, torch.Tensor), "step_scalars must be a tensor")
    _want(step_scalars, "step_scalars", torch.float32, (4,))
    mx, ps, e = float(max_norm), float(pre_scale), float(eps)
    _require(mx >= 0.0, "max_norm must be >= 0 (it may be inf)")
    _require(0.0 < ps < float("inf"), "pre_scale must be finite and > 0")
    _require(0.0 <= e < float("inf"), "eps must be finite and >= 0")
    return mx, ps, e


_CLIP_SPECS = (("norm", torch.float32, (1,)), ("coef", torch.float32, (1,)), ("skip", torch.int32, (1,)))


def _clip_run(sumsq, step_scalars, mx, ps, e, outs, sync):
    norm, coef, skip = outs
    _launch("grad_clip_scalars", (sumsq, step_scalars, norm, coef, skip), lambda L, stream: L.dga_grad_clip_scalars(
        sumsq.data_ptr(), mx, ps, e, step_scalars.data_ptr(), norm.data_ptr(), coef.data_ptr(), skip.data_ptr(), stream), sync)
    return norm, coef, skip


def grad_clip_scalars(sumsq: torch.Tensor, step_scalars: torch.Tensor, max_norm: float, pre_scale: float = 1.0, eps: float = 1e-6, out=None,
                      sync: bool = False):
    """From the sum of squares to what the optimizer reads (dga_grad_clip_scalars): sumsq a float64 [1] device tensor (grad_sumsq's, possibly
    all-reduced across ranks in between), step_scalars the optimizer's float32 [4], of which only element 3 is written -> the named tuple
    (norm, coef, skip).  One lane on the device, float64, rounded once to float32 on store:
      finite = isfinite(sumsq[0])
      normd  = pre_scale sqrt(sumsq[0])                      the norm of the unscaled gradients; pre_scale = 1 / loss_scale
      coefd  = min(1, max_norm / (normd + eps))              torch.nn.utils.clip_grad_norm_'s; max_norm = inf never clips; 0 / 0 gives 1
      norm[0] = f32(normd), non-finite as it comes;  coef[0] = finite ? f32(coefd) : 0;  step_scalars[3] = finite ? f32(pre_scale coefd) : 0
      skip[0] = finite ? 0 : 1                               int32, overwritten at every call
    norm and coef are float32 [1] device tensors (parameters that stay with torch's optimizer multiply their gradients by coef), skip is
    the int32 [1] that adamw_per_block_cast_to_fp8_transposed(..., skip=) reads.  max_norm >= 0 (it may be inf), pre_scale finite and > 0,
    eps finite and >= 0: launch arguments, C doubles.  out=(norm, coef, skip) takes the caller's tensors.  Nothing is read back: capturable."""
    _require(isinstance(sumsq, torch.Tensor), "sumsq must be a tensor")
    _want(sumsq, "sumsq", torch.float64, (1,))
    mx, ps, e = _clip_args(step_scalars, max_norm, pre_scale, eps)
    outs = _outputs(out, _CLIP_SPECS, sumsq.device, "out must be (norm, coef, skip)")
    return GradClip(*_clip_run(sumsq, step_scalars, mx, ps, e, outs, sync))


def clip_grad_norm_step_scalars(tensors, step_scalars: torch.Tensor, max_norm: float, pre_scale: float = 1.0, eps: float = 1e-6, out=None):
    """grad_sumsq(tensors) then grad_clip_scalars(sumsq, step_scalars, max_norm, pre_scale, eps): the global gradient norm, the clip
    coefficient into step_scalars[3] and the skip flag, with nothing decided on the host -> the named tuple (norm, coef, skip, sumsq).
    out=(norm, coef, skip, sumsq) takes the caller's tensors.  Every argument is checked before the first launch.  Capturable: a captured
    graph runs weight gradient -> this -> adamw_per_block_cast_to_fp8_transposed(..., skip=skip) -> the next GEMMs."""
    _require(out is None or (isinstance(out, (tuple, list)) and len(out) == 4), "out must be (norm, coef, skip, sumsq)")
    tensors, sumsq = _sumsq_args(tensors, None if out is None else out[3], False)
    mx, ps, e = _clip_args(step_scalars, max_norm, pre_scale, eps)
    outs = _outputs(None if out is None else tuple(out[:3]), _CLIP_SPECS, tensors[0].device, "out must be (norm, coef, skip, sumsq)")
    sumsq = _sumsq_run(tensors, sumsq, False, False)
    return GradClipNorm(*_clip_run(sumsq, step_scalars, mx, ps, e, outs, False), sumsq)


MQA_LOGITS_HEAD_DIM, MQA_LOGITS_HEADS = 128, (32, 64)
MQA_LOGITS_BLOCK_M, MQA_LOGITS_BLOCK_N = 64, 256   # the kernel's token run and key block (DGA_MQA_LOGITS_BLOCK_*)


def fp8_mqa_logits(q: torch.Tensor, kv: Tuple[torch.Tensor, torch.Tensor], weights: torch.Tensor, cu_seq_len_k_start: torch.Tensor,
                   cu_seq_len_k_end: torch.Tensor, out: Optional[torch.Tensor] = None, sync: bool = False) -> torch.Tensor:
    """The scoring kernel of the lightning indexer of DeepSeek sparse attention, upstream DeepGEMM's fp8_mqa_logits (dga_fp8_mqa_logits):
    logits[m, n] = kscale[n] * sum_h weights[m, h] * relu(sum_d q[m, h, d] k[n, d]) for clamp(ks[m]) <= n < clamp(ke[m]), -inf elsewhere.
    q [M, H, 128] float8_e4m3fn (or uint8 bytes) without a scale -- the caller folds it into weights, as upstream --, kv = (k [N, 128] fp8,
    kscale float32 [N]), weights float32 [M, H], cu_seq_len_k_start / cu_seq_len_k_end int32 [M] device tensors, all contiguous;
    H 32 or 64, any M >= 0, any N >= 1.  Returns float32 [M, N] (out= takes the caller's; it needs no pre-fill: every element is written,
    in-range values and -inf).  The ranges are read and clamped to [0, N] on the device, so a captured graph follows new ones; ke <= ks is a
    row of -inf.  The dot products are four chained bf16 matrix instructions on exactly converted codes with fp32 accumulation, the ReLU
    keeps a NaN, the head sum has one order that H fixes and kscale multiplies once after it: two runs give the same bits, and
    |logits - exact| <= (2^-22 + (H + 3) 2^-24) kscale[n] sum_h |weights| sum_d |q k| on every in-range element.  A NaN code in q poisons
    its row, one in k its column, inside the ranges only.  A token whose range misses a block of 256 keys costs that block nothing but the
    -inf stores, so a causal prefill costs about half the dense work.  M == 0 returns without a launch."""
    _require(isinstance(kv, (tuple, list)) and len(kv) == 2, "kv must be (k, kscale)")
    k, kscale = kv
    _require(q.dim() == 3, "q must be [M, H, %d]", MQA_LOGITS_HEAD_DIM)
    m, h, d = q.shape
    _require(d == MQA_LOGITS_HEAD_DIM, "q must be [M, H, %d]: head dimension %d is not supported", MQA_LOGITS_HEAD_DIM, d)
    _require(h in MQA_LOGITS_HEADS, "q must have 32 or 64 heads, got %d", h)
    _want(_fp8_bytes(q), "q", None, (m, h, d))
    _require(k.dim() == 2 and k.shape[0] >= 1, "k must be [N, %d] with N >= 1", d)
    n = k.shape[0]
    _want(_fp8_bytes(k), "k", None, (n, d))
    _want(kscale, "kscale", torch.float32, (n,))
    _want(weights, "weights", torch.float32, (m, h))
    _want(cu_seq_len_k_start, "cu_seq_len_k_start", torch.int32, (m,))
    _want(cu_seq_len_k_end, "cu_seq_len_k_end", torch.int32, (m,))
    if out is None:
        out = torch.empty((m, n), dtype=torch.float32, device=q.device)
    else:
        _want(out, "out", torch.float32, (m, n))
    # (M == 0: the C entry returns before any launch)
    _launch("fp8_mqa_logits", (q, k, kscale, weights, cu_seq_len_k_start, cu_seq_len_k_end, out), lambda L, stream: L.dga_fp8_mqa_logits(
        q.data_ptr(), k.data_ptr(), kscale.data_ptr(), weights.data_ptr(), cu_seq_len_k_start.data_ptr(), cu_seq_len_k_end.data_ptr(),
        m, n, h, d, out.data_ptr(), stream), sync)
    return out


PAGED_MQA_LOGITS_BLOCK_KV, PAGED_MQA_LOGITS_BLOCK_BYTES = 64, 8448   # keys of a cache block; its bytes: 64 * 128 codes + 64 fp32 scales
PAGED_MQA_LOGITS_CHUNK_N = 512                                       # columns of one workgroup (DGA_PAGED_MQA_LOGITS_CHUNK_N)


def _paged_cache(kv_cache: torch.Tensor):
    """The indexer's paged key cache, checked: uint8 [num_blocks, 64, 1, 132] or [num_blocks, 8448], the bytes of a block contiguous,
    blocks stride(0) >= 8448 bytes apart, a multiple of 16.  Returns (num_blocks, block stride)."""
    _require(kv_cache.dtype == torch.uint8, "kv_cache must be uint8, got %s", kv_cache.dtype)
    _require(kv_cache.dim() in (2, 4), "kv_cache must be [num_blocks, 64, 1, 132] or [num_blocks, %d]", PAGED_MQA_LOGITS_BLOCK_BYTES)
    if kv_cache.dim() == 4:
        nb, bs, one, row = kv_cache.shape
        _require(bs == PAGED_MQA_LOGITS_BLOCK_KV, "kv_cache must have blocks of 64 keys, got %d", bs)
        _require(one == 1 and row == MQA_LOGITS_HEAD_DIM + 4, "kv_cache must be [num_blocks, 64, 1, 132]: %d x %d bytes per key", one, row)
        inner = kv_cache.stride(1) == row and kv_cache.stride(3) == 1
    else:
        nb, row = kv_cache.shape
        _require(row == PAGED_MQA_LOGITS_BLOCK_BYTES, "kv_cache must be [num_blocks, %d], got %d bytes per block", PAGED_MQA_LOGITS_BLOCK_BYTES, row)
        inner = kv_cache.stride(1) == 1
    _require(nb >= 1, "kv_cache must have at least one block")
    _require(inner, "kv_cache must be contiguous inside a block")
    stride = kv_cache.stride(0) if nb > 1 else PAGED_MQA_LOGITS_BLOCK_BYTES
    _require(stride >= PAGED_MQA_LOGITS_BLOCK_BYTES and stride % 16 == 0,
             "kv_cache blocks must be at least %d bytes apart and a multiple of 16, got stride(0) = %d", PAGED_MQA_LOGITS_BLOCK_BYTES, stride)
    return nb, stride


def fp8_paged_mqa_logits(q: torch.Tensor, kv_cache: torch.Tensor, weights: torch.Tensor, context_lens: torch.Tensor,
                         block_tables: torch.Tensor, schedule_metadata=None, max_model_len: Optional[int] = None,
                         clean_logits: bool = True, out: Optional[torch.Tensor] = None, sync: bool = False) -> torch.Tensor:
    """The decode half of the lightning indexer's scoring, upstream DeepGEMM's fp8_paged_mqa_logits in its positional order
    (dga_fp8_paged_mqa_logits): each of B sequences scores its next_n newest tokens against its whole context in a paged key cache.
    q [B, next_n, H, 128] float8_e4m3fn (or uint8 bytes) without a scale, next_n 1 or 2, H 32 or 64; kv_cache uint8
    [num_blocks, 64, 1, 132] or [num_blocks, 8448]: block b holds the codes of its 64 keys, key-major, in bytes 0 .. 8191 and their 64
    float32 scales in bytes 8192 .. 8447 (upstream's fused layout; per_token_cast_to_fp8_paged writes it), stride(0) >= 8448 and a multiple
    of 16; weights float32 [B next_n, H]; context_lens int32 [B] and block_tables int32 [B, max_blocks], device tensors read on the device;
    max_model_len = N, the width of the result, is required.  With ctx_i = min(max(context_lens[i], 0), N, 64 max_blocks) and row
    r = i next_n + j: logits[r, n] = kscale sum_h weights[r, h] relu(sum_d q[i, j, h, d] k[d]) for n < max(ctx_i - next_n + j + 1, 0), k the
    key n % 64 of block block_tables[i, n // 64], and -inf from there to N.  Returns float32 [B next_n, N] (out= takes the caller's).
    A table entry is read only for pages below ceil(ctx_i / 64); one of those outside [0, num_blocks) dereferences nothing and gives -inf
    on its page's columns.  clean_logits=True writes every element; clean_logits=False writes the rows of sequence i only in columns
    below 64 ceil(ctx_i / 64) and touches nothing from there on (what serving engines use: the -inf fill can cost as much as the scoring).
    The arithmetic is fp8_mqa_logits': on the keys and scales gathered through a sequence's table the in-range elements are that
    function's bit for bit, with its bound; no atomics, two runs give the same bits.
    schedule_metadata is accepted for upstream call sites and never read: upstream's value is a per-SM work split for a persistent
    scheduler, while this kernel's grid, B x ceil(N / 512), is fixed by the shapes and no workgroup assumes residency -- there is no such
    table, and no get_paged_mqa_logits_metadata.  B == 0 returns without a launch."""
    _require(q.dim() == 4, "q must be [B, next_n, H, %d]", MQA_LOGITS_HEAD_DIM)
    b, nn, h, d = q.shape
    _require(d == MQA_LOGITS_HEAD_DIM, "q must be [B, next_n, H, %d]: head dimension %d is not supported", MQA_LOGITS_HEAD_DIM, d)
    _require(nn in (1, 2), "q must have next_n 1 or 2, got %d", nn)
    _require(h in MQA_LOGITS_HEADS, "q must have 32 or 64 heads, got %d", h)
    _want(_fp8_bytes(q), "q", None, (b, nn, h, d))
    nb, stride = _paged_cache(kv_cache)
    _want(weights, "weights", torch.float32, (b * nn, h))
    _want(context_lens, "context_lens", torch.int32, (b,))
    _require(block_tables.dim() == 2 and block_tables.shape[1] >= 1, "block_tables must be [B, max_blocks] with max_blocks >= 1")
    max_blocks = block_tables.shape[1]
    _want(block_tables, "block_tables", torch.int32, (b, max_blocks))
    _require(max_model_len is not None, "max_model_len is required: it is the width of the result")
    n = int(max_model_len)
    _require(n >= 1, "max_model_len must be at least 1, got %d", n)
    if out is None:
        out = torch.empty((b * nn, n), dtype=torch.float32, device=q.device)
    else:
        _want(out, "out", torch.float32, (b * nn, n))
    # (B == 0: the C entry returns before any launch)
    _launch("fp8_paged_mqa_logits", (q, kv_cache, weights, context_lens, block_tables, out), lambda L, stream: L.dga_fp8_paged_mqa_logits(
        q.data_ptr(), kv_cache.data_ptr(), weights.data_ptr(), context_lens.data_ptr(), block_tables.data_ptr(), b, nn, h, d, nb, stride,
        max_blocks, n, 1 if clean_logits else 0, out.data_ptr(), stream), sync)
    return out


def per_token_cast_to_fp8_paged(x: torch.Tensor, kv_cache: torch.Tensor, slot_mapping: torch.Tensor, use_ue8m0: bool = False,
                                sync: bool = False) -> torch.Tensor:
    """The writer of fp8_paged_mqa_logits' key cache (dga_cast_to_fp8_1x128_paged): x [T, 128] float32 / bfloat16 / float16, kv_cache as
    there, slot_mapping int64 [T] on the device.  For every t with 0 <= slot_mapping[t] < 64 num_blocks the 128 codes of
    per_token_cast_to_fp8(x, use_ue8m0=...)[0][t] go to bytes 128 (slot % 64) .. of block slot // 64 and the scale [1][t, 0] to bytes
    8192 + 4 (slot % 64) .. of that block, byte for byte.  Any other slot value (engines pad with -1) skips the token and dereferences
    nothing; no other byte of the cache is touched.  Duplicate valid slots in one call are the caller's error.  Returns kv_cache."""
    _require(x.dim() == 2 and x.shape[1] == MQA_LOGITS_HEAD_DIM and x.is_contiguous(), "x must be a contiguous [T, %d] tensor", MQA_LOGITS_HEAD_DIM)
    _require(x.dtype in _CAST_DT, "x must be float32, bfloat16 or float16")
    t = x.shape[0]
    nb, stride = _paged_cache(kv_cache)
    _want(slot_mapping, "slot_mapping", torch.int64, (t,))
    # (T == 0: the C entry returns before any launch)
    _launch("per_token_cast_to_fp8_paged", (x, kv_cache, slot_mapping), lambda L, stream: L.dga_cast_to_fp8_1x128_paged(
        x.data_ptr(), _CAST_DT[x.dtype], t, kv_cache.data_ptr(), nb, stride, slot_mapping.data_ptr(),
        _lib.CAST_UE8M0 if use_ue8m0 else 0, stream), sync)
    return kv_cache


INDEXER_TOPK_MAX_K = 2048            # DGA_INDEXER_TOPK_MAX_K
INDEXER_TOPK_CANDIDATES = 8192       # keys of the kernel's LDS candidate buffer (DGA_INDEXER_TOPK_CANDIDATES)


def indexer_topk(logits: torch.Tensor, k: int = 2048, row_starts: Optional[torch.Tensor] = None, row_ends: Optional[torch.Tensor] = None,
                 context_lens: Optional[torch.Tensor] = None, next_n: int = 1, relative: bool = False,
                 block_tables: Optional[torch.Tensor] = None, page_size: int = 64, num_blocks: Optional[int] = None,
                 out: Optional[torch.Tensor] = None, sync: bool = False) -> torch.Tensor:
    """The selecting half of the lightning indexer (dga_indexer_topk): per row of fp8_mqa_logits' / fp8_paged_mqa_logits' output, the
    indices of the k highest-scoring keys inside the row's range, ascending, as int32 [M, k].  logits float32 [M, N] with a contiguous
    last dimension and any stride(0) >= N (a column slice logits[:, :64 max_blocks] of a wider buffer is accepted); 1 <= k <= 2048.
    The range [lo, hi) of row m is formed on the device from exactly one of: row_starts, row_ends int32 [M] (both or neither; the tensors
    given to fp8_mqa_logits): lo = min(max(ks, 0), N), hi = min(max(ke, 0), N);  context_lens int32 [B] with next_n 1 or 2 and
    M = B next_n: ctx = min(max(context_lens[m // next_n], 0), N), lo = 0, hi = max(ctx - next_n + m % next_n + 1, 0)
    (fp8_paged_mqa_logits' rule);  neither: lo = 0, hi = N.
    The order is total and defined on the bits: key(x) = bits(x) ^ (0xFFFFFFFF if bits(x) >> 31 else 0x80000000), every NaN 0xFFFFFFFF
    (above +inf, as torch.topk ranks it; -0 below +0); column a precedes b iff its key is greater, or equal and a < b.  With
    c = min(hi - lo, k), out[m, :c] is the first c columns of [lo, hi) in that order, sorted ascending by column, and out[m, c:] is -1;
    every element of out is written.  Membership is by column, never by value (an in-range -inf is a candidate); no byte of logits outside
    [lo, hi) is read, so a buffer fp8_paged_mqa_logits(clean_logits=False) left unwritten beyond a sequence's last page is valid
    input; a row with hi - lo <= k reads no logits.  What is written for a selected column n: n;  relative=True: n - lo (what a prefill
    caller hands to sparse attention);  block_tables int32 [B, max_blocks] with page_size >= 1 and num_blocks (lengths form only):
    block_tables[m // next_n, n // page_size] page_size + n % page_size, and -1 where n // page_size >= max_blocks or the entry lies
    outside [0, num_blocks); entries of unselected columns are not read.  The result is a pure function of the in-range bits: two
    runs give the same bytes, and a stable numpy argsort reproduces them.  One launch, capturable; M == 0 returns without one."""
    _require(logits.dim() == 2 and logits.dtype == torch.float32, "logits must be a float32 [M, N] tensor")
    m, n = logits.shape
    _require(n >= 1, "logits must have at least one column")
    _require((n == 1 or logits.stride(1) == 1) and (m <= 1 or logits.stride(0) >= n),
             "logits must have a contiguous last dimension and stride(0) >= N")
    _require(isinstance(k, int) and 1 <= k <= INDEXER_TOPK_MAX_K, "k must be an integer in [1, %d]", INDEXER_TOPK_MAX_K)
    _require((row_starts is None) == (row_ends is None), "row_starts and row_ends come together or not at all")
    _require(row_starts is None or context_lens is None, "row_starts / row_ends and context_lens exclude each other")
    _require(not (relative and block_tables is not None), "relative and block_tables exclude each other")
    _require(block_tables is None or context_lens is not None, "block_tables needs context_lens")
    if row_starts is not None:
        _want(row_starts, "row_starts", torch.int32, (m,))
        _want(row_ends, "row_ends", torch.int32, (m,))
    b, max_blocks, blocks = 0, 0, 0
    if context_lens is not None:
        _require(next_n in (1, 2), "next_n must be 1 or 2")
        _require(m % next_n == 0, "logits must have B next_n rows, got %d with next_n = %d", m, next_n)
        b = m // next_n
        _want(context_lens, "context_lens", torch.int32, (b,))
    if block_tables is not None:
        _require(block_tables.dim() == 2 and block_tables.shape[1] >= 1, "block_tables must be [B, max_blocks] with max_blocks >= 1")
        max_blocks = block_tables.shape[1]
        _want(block_tables, "block_tables", torch.int32, (b, max_blocks))
        _require(isinstance(page_size, int) and page_size >= 1, "page_size must be an integer >= 1")
        _require(isinstance(num_blocks, int) and num_blocks >= 1, "num_blocks is required with block_tables: an integer >= 1")
        _require(num_blocks * page_size < 1 << 31, "num_blocks page_size must be below 2^31, got %d x %d", num_blocks, page_size)
        blocks = num_blocks
    if out is None:
        out = torch.empty((m, k), dtype=torch.int32, device=logits.device)
    else:
        _want(out, "out", torch.int32, (m, k))
    stride = logits.stride(0) if m > 1 else n
    # (M == 0: the C entry returns before any launch)
    _launch("indexer_topk", (logits, row_starts, row_ends, context_lens, block_tables, out), lambda L, stream: L.dga_indexer_topk(
        logits.data_ptr(), m, n, stride, k, _ptr(row_starts), _ptr(row_ends), _ptr(context_lens), next_n if context_lens is not None else 1,
        1 if relative else 0, _ptr(block_tables), max_blocks, page_size if block_tables is not None else 1, blocks, out.data_ptr(), stream),
        sync)
    return out


SPARSE_MLA_D_QK = 576                # DGA_SPARSE_MLA_D_QK: 512 latent + 64 rope dimensions
SPARSE_MLA_D_V = 512                 # DGA_SPARSE_MLA_D_V
SPARSE_MLA_MAX_HEADS = 128           # DGA_SPARSE_MLA_MAX_HEADS


def _smla_bf16_rows(q: torch.Tensor, kv: torch.Tensor) -> Tuple[int, int]:
    """kv of sparse_mla_fwd and its split forms, checked (and q's alignment with it): (S, kv_stride)"""
    _require(kv.dtype == torch.bfloat16 and (kv.dim() == 2 or (kv.dim() == 3 and kv.shape[1] == 1)) and kv.shape[-1] == SPARSE_MLA_D_QK,
             "kv must be a bfloat16 [S, %d] or [S, 1, %d] tensor", SPARSE_MLA_D_QK, SPARSE_MLA_D_QK)
    s = kv.shape[0]
    _require(1 <= s < 1 << 31, "kv must have between 1 and 2^31 - 1 rows, got %d", s)
    kv_stride = kv.stride(0) if s > 1 else SPARSE_MLA_D_QK
    _require(kv.stride(-1) == 1 and kv_stride >= SPARSE_MLA_D_QK and kv_stride % 8 == 0,
             "kv must have a contiguous last dimension and a stride(0) >= %d that is a multiple of 8, got %d", SPARSE_MLA_D_QK, kv_stride)
    _require(kv.data_ptr() % 16 == 0 and q.data_ptr() % 16 == 0, "q and kv must be 16-byte aligned")
    return s, kv_stride


def _smla_outputs(out: Optional[torch.Tensor], lse: Optional[torch.Tensor], m: int, heads: int, device):
    """out bfloat16 [M, Hq, 512] and lse float32 [M, Hq]: torch.empty, or the caller's, checked"""
    if out is None:
        out = torch.empty((m, heads, SPARSE_MLA_D_V), dtype=torch.bfloat16, device=device)
    else:
        _want(out, "out", torch.bfloat16, (m, heads, SPARSE_MLA_D_V))
    if lse is None:
        lse = torch.empty((m, heads), dtype=torch.float32, device=device)
    else:
        _want(lse, "lse", torch.float32, (m, heads))
    return out, lse


# The six attention forms are one problem -- q, a row source, indices -- run by three bodies: one pass, partials, partials and merge.  The
# row source is bf16 rows (fp8=False: _smla_bf16_rows) or the paged fp8 latent cache (fp8=True: _mla_fp8_cache, below); the C entries of
# the two differ by "_fp8" in the name and by the source's geometry among the arguments.
_SMLA_ENTRY = {False: "sparse_mla_fwd", True: "sparse_mla_fwd_fp8"}


def _smla_problem(fp8: bool, q: torch.Tensor, rows: torch.Tensor, indices: torch.Tensor, sm_scale, d_v: int,
                  index_offsets: Optional[torch.Tensor]):
    """What every attention form checks, in the order every form reports: q, the rows, indices.  Returns (M, Hq, topk, args): what the
    bodies size their outputs by, and the arguments that follow the four pointers in every C entry of the family -- M, Hq, the source's
    geometry, topk, idx_stride, sm_scale.  (The pointers are taken at the launch, behind the guard: a refused call pays for its checks.)"""
    _require(q.dim() == 3 and q.dtype == torch.bfloat16 and q.shape[2] == SPARSE_MLA_D_QK and q.is_contiguous(),
             "q must be a contiguous bfloat16 [M, Hq, %d] tensor", SPARSE_MLA_D_QK)
    m, heads = q.shape[0], q.shape[1]
    _require(heads % 16 == 0 and 16 <= heads <= SPARSE_MLA_MAX_HEADS, "Hq must be a multiple of 16 in [16, %d], got %d",
             SPARSE_MLA_MAX_HEADS, heads)
    _require(d_v == SPARSE_MLA_D_V, "d_v must be %d", SPARSE_MLA_D_V)
    _require(isinstance(sm_scale, (int, float)), "sm_scale must be a number")
    if fp8:
        geometry = _mla_fp8_cache(rows)
        _require(q.data_ptr() % 16 == 0, "q must be 16-byte aligned")
    else:
        geometry = _smla_bf16_rows(q, rows)
    _require(indices.dtype == torch.int32 and (indices.dim() == 2 or (indices.dim() == 3 and indices.shape[1] == 1))
             and indices.shape[0] == m and indices.shape[-1] >= 1, "indices must be an int32 [M, topk] or [M, 1, topk] tensor with topk >= 1")
    topk = indices.shape[-1]
    idx_stride = indices.stride(0) if m > 1 else topk
    _require((topk == 1 or indices.stride(-1) == 1) and idx_stride >= topk, "indices must have a contiguous last dimension and stride(0) >= topk")
    if index_offsets is not None:
        _want(index_offsets, "index_offsets", torch.int32, (m,))
    return m, heads, topk, (m, heads, *geometry, topk, idx_stride, float(sm_scale))


def _smla_one_pass(fp8: bool, q, rows, indices, sm_scale, d_v, index_offsets, out, lse, sync: bool, flags: int, checked=None):
    """The body of sparse_mla_fwd / sparse_mla_fwd_fp8: the checks (or `checked`, what _smla_problem returned to the split body), the
    outputs, one launch"""
    m, heads, _, args = checked or _smla_problem(fp8, q, rows, indices, sm_scale, d_v, index_offsets)
    name = _SMLA_ENTRY[fp8]
    out, lse = _smla_outputs(out, lse, m, heads, q.device)
    # (M == 0: the C entry returns before any launch)
    _launch(name, (q, rows, indices, index_offsets, out, lse), lambda L, stream: getattr(L, "dga_" + name)(
        q.data_ptr(), rows.data_ptr(), indices.data_ptr(), _ptr(index_offsets), *args, flags, out.data_ptr(), lse.data_ptr(), stream), sync)
    return out, lse


def sparse_mla_fwd(q: torch.Tensor, kv: torch.Tensor, indices: torch.Tensor, sm_scale: float, d_v: int = 512,
                   index_offsets: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, lse: Optional[torch.Tensor] = None,
                   sync: bool = False, _flags: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """What the indexer selects for (dga_sparse_mla_fwd): sparse MLA attention, forward, over indexer_topk's indices, in MLA's absorbed
    (MQA) form; the positional order is FlashMLA's flash_mla_sparse_fwd.  q bfloat16 [M, Hq, 576] contiguous, Hq a multiple of 16 in
    [16, 128];  kv bfloat16 [S, 576] or [S, 1, 576] with a contiguous last dimension, stride(0) >= 576 and a multiple of 8, a 16-byte
    aligned base and 1 <= S < 2^31 -- every row is key (all 576 columns) and value (its first 512); a flat view of a paged bf16 latent
    cache is valid input and indexer_topk(block_tables=...)'s physical slots index it directly;  indices int32 [M, topk] or [M, 1, topk]
    with a contiguous last dimension and stride(0) >= topk >= 1 (a slice idx[:, :k'] is accepted);  index_offsets int32 [M] or None: the
    kv row of position j is indices[m, j] + index_offsets[m] (fp8_mqa_logits' row_starts beside indexer_topk(relative=True));
    d_v must be 512.
    Everything is read on the device.  A position is valid iff indices[m, j] >= 0 and its row lies in [0, S); an invalid one
    (indexer_topk's -1 padding, any other negative, anything >= S) dereferences nothing and contributes nothing; duplicates count once
    per position; no other kv row and no column >= 576 of any row is read.  Over the valid positions, with r_j the row:
    s_j = sm_scale sum_d q[m, h, d] kv[r_j, d];  lse[m, h] = ln sum_j exp(s_j) (float32 [M, Hq], natural log: what a merge over chunks of
    topk or over ranks needs);  out[m, h, :] = sum_j exp(s_j - lse) kv[r_j, :512] (bfloat16 [M, Hq, 512]).  A token with no valid
    position gets out = +0 and lse = -inf.  Every element of both outputs is written.
    Arithmetic: exact bf16 products summed in fp32 on the matrix pipe over d ascending; an online softmax over tiles of 32 positions in
    list order; the weights rounded to bf16 (RNE) for the second product while their sum l stays unrounded fp32; one multiplication by
    1 / l at the end.  One writer per element, no atomics: two runs give the same bytes.  Returns (out, lse), the caller's out= / lse=
    when given.  One launch, capturable -- a replayed graph follows new indices, offsets, kv and q; M == 0 returns without one."""
    return _smla_one_pass(False, q, kv, indices, sm_scale, d_v, index_offsets, out, lse, sync, _flags)


SPARSE_MLA_FP8_ROW_BYTES = 656       # DGA_SPARSE_MLA_FP8_ROW_BYTES: 512 e4m3fn codes, 4 float32 scales, 64 bfloat16 rope values


def _mla_fp8_cache(kv_cache: torch.Tensor):
    """Sparse MLA's paged fp8 latent cache, checked: uint8 [num_blocks, page_size, 1, 656] (stride(3) == 1, stride(1) == 656, blocks
    stride(0) >= 656 page_size bytes apart) or [S, 656] (stride(1) == 1, rows stride(0) >= 656 apart: page_size 1), the stride a multiple
    of 16, the base 16-byte aligned, 1 <= S < 2^31.  Returns (num_blocks, page_size, block stride)."""
    row = SPARSE_MLA_FP8_ROW_BYTES
    _require(kv_cache.dtype == torch.uint8, "kv_cache must be uint8, got %s", kv_cache.dtype)
    _require(kv_cache.dim() in (2, 4) and kv_cache.shape[-1] == row and (kv_cache.dim() == 2 or kv_cache.shape[2] == 1),
             "kv_cache must be [num_blocks, page_size, 1, %d] or [S, %d], got %s", row, row, list(kv_cache.shape))
    nb, page = kv_cache.shape[0], (kv_cache.shape[1] if kv_cache.dim() == 4 else 1)
    _require(nb >= 1 and page >= 1, "kv_cache must have at least one row")
    _require(kv_cache.stride(-1) == 1 and (kv_cache.dim() == 2 or page == 1 or kv_cache.stride(1) == row),
             "kv_cache must have contiguous rows, %d bytes apart inside a block (stride(1) == %d)", row, row)
    stride = kv_cache.stride(0) if nb > 1 else page * row
    _require(stride >= page * row and stride % 16 == 0,
             "kv_cache blocks must be at least %d bytes apart and a multiple of 16, got stride(0) = %d", page * row, stride)
    _require(nb * page < 1 << 31, "kv_cache must have fewer than 2^31 rows, got %d x %d", nb, page)
    _require(kv_cache.data_ptr() % 16 == 0, "kv_cache must be 16-byte aligned")
    return nb, page, stride


def sparse_mla_fwd_fp8(q: torch.Tensor, kv_cache: torch.Tensor, indices: torch.Tensor, sm_scale: float, d_v: int = 512,
                       index_offsets: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, lse: Optional[torch.Tensor] = None,
                       sync: bool = False, _flags: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """sparse_mla_fwd over a paged fp8 latent cache, read in place (dga_sparse_mla_fwd_fp8).  kv_cache uint8
    [num_blocks, page_size, 1, 656] (stride(3) == 1, stride(1) == 656, stride(0) >= 656 page_size and a multiple of 16, any page_size >= 1)
    or [S, 656] (stride(1) == 1, stride(0) >= 656 and a multiple of 16), the base 16-byte aligned, 1 <= S = num_blocks page_size < 2^31.
    Row r lives at (r // page_size) stride(0) + (r % page_size) 656 and holds, in FlashMLA's layout of this model's cache: bytes 0 .. 511
    the 512 e4m3fn codes of the latent part, bytes 512 .. 527 four float32 scales (one per 128 codes), bytes 528 .. 655 the 64 rope values
    in bfloat16 (mla_kv_cast_to_fp8_paged writes it).  With page_size 64 and a block table, indexer_topk(block_tables=..., page_size=64)
    emits exactly these row numbers.  The value of a row is defined on the bits:
    deq[r, d] = RNE_bf16(fl32(e4m3(code[r, d]) scale[r, d // 128])) for d < 512 -- in torch
    (codes.view(torch.float8_e4m3fn).float() * scales.repeat_interleave(128, -1)).to(torch.bfloat16) -- and the rope values as stored.
    The result is sparse_mla_fwd(q, deq, ...)'s: out and lse byte for byte wherever that is not NaN, NaN in exactly the same elements;
    q, indices, index_offsets, out, lse, the validity rule, the arithmetic and its bounds are that function's.  No byte of an unselected
    row and no byte between a block's last row and the next block is read.  One launch, capturable; M == 0 returns without one."""
    return _smla_one_pass(True, q, kv_cache, indices, sm_scale, d_v, index_offsets, out, lse, sync, _flags)


SPARSE_MLA_MAX_SPLITS = 64           # DGA_SPARSE_MLA_MAX_SPLITS


def _smla_splits(num_splits, topk: int) -> int:
    """num_splits of the split forms, checked: the effective P = min(num_splits, ceil(topk / 32))"""
    _require(isinstance(num_splits, int) and not isinstance(num_splits, bool) and 1 <= num_splits <= SPARSE_MLA_MAX_SPLITS,
             "num_splits must be an int in [1, %d], got %r", SPARSE_MLA_MAX_SPLITS, num_splits)
    return min(num_splits, (topk + 31) // 32)


def _smla_partials(partial_out, partial_lse, p: int, m: int, heads: int, device):
    """partial_out float32 [P, M, Hq, 512] and partial_lse float32 [P, M, Hq]: torch.empty, or the first P splits of the caller's
    contiguous [>= P, ...] buffers (what lies beyond them is not touched)"""
    made = []
    for t, what, shape in ((partial_out, "partial_out", (m, heads, SPARSE_MLA_D_V)), (partial_lse, "partial_lse", (m, heads))):
        if t is None:
            t = torch.empty((p,) + shape, dtype=torch.float32, device=device)
        else:
            _require(t.dtype == torch.float32 and t.dim() == len(shape) + 1 and tuple(t.shape[1:]) == shape and t.shape[0] >= p
                     and t.is_contiguous(), "%s must be contiguous float32 [>= %d, %s]", what, p, ", ".join(map(str, shape)))
            t = t[:p]
        made.append(t)
    return made


def _smla_partial(fp8: bool, q, rows, indices, sm_scale, num_splits, d_v, index_offsets, partial_out, partial_lse, sync: bool, flags: int):
    """The body of sparse_mla_fwd_partial / sparse_mla_fwd_fp8_partial: the checks, num_splits, the partials, one launch"""
    m, heads, topk, args = _smla_problem(fp8, q, rows, indices, sm_scale, d_v, index_offsets)
    name = _SMLA_ENTRY[fp8] + "_partial"
    p = _smla_splits(num_splits, topk)
    po, pl = _smla_partials(partial_out, partial_lse, p, m, heads, q.device)
    # (M == 0: the C entry returns before any launch)
    _launch(name, (q, rows, indices, index_offsets, po, pl), lambda L, stream: getattr(L, "dga_" + name)(
        q.data_ptr(), rows.data_ptr(), indices.data_ptr(), _ptr(index_offsets), *args, flags, p, None, po.data_ptr(), pl.data_ptr(), stream), sync)
    return po, pl


def sparse_mla_fwd_partial(q: torch.Tensor, kv: torch.Tensor, indices: torch.Tensor, sm_scale: float, num_splits: int, d_v: int = 512,
                           index_offsets: Optional[torch.Tensor] = None, partial_out: Optional[torch.Tensor] = None,
                           partial_lse: Optional[torch.Tensor] = None, sync: bool = False, _flags: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """The first half of split-topk sparse MLA decode (dga_sparse_mla_fwd_partial): sparse_mla_fwd with P workgroups a token and head block
    in place of one, for the small M at which one workgroup a token leaves the device idle.  q, kv, indices, sm_scale, d_v and
    index_offsets are sparse_mla_fwd's; num_splits an int in [1, 64].  With tiles = ceil(topk / 32) and P = min(num_splits, tiles), split p
    owns the contiguous tiles [p tiles // P, (p + 1) tiles // P) of every token's list and writes its own attention result in float32, not
    rounded to bfloat16: partial_out[p, m, h, :] = sum_j exp(s_j - partial_lse[p, m, h]) kv[r_j, :512] and
    partial_lse[p, m, h] = ln sum_j exp(s_j) over the split's valid positions, +0 and -inf where it has none.  Per tile the arithmetic is
    sparse_mla_fwd's.  Returns (partial_out float32 [P, M, Hq, 512], partial_lse float32 [P, M, Hq]) with the effective P as their first
    dimension: fresh tensors, or the first P splits of the caller's contiguous float32 [>= P, M, Hq, 512] and [>= P, M, Hq] buffers, of which
    every element is written and nothing beyond them is.  sparse_mla_merge turns them into (out, lse); with P = 1 the two calls give
    sparse_mla_fwd's bytes.  One launch, capturable; two runs give the same bytes; M == 0 returns without a launch."""
    return _smla_partial(False, q, kv, indices, sm_scale, num_splits, d_v, index_offsets, partial_out, partial_lse, sync, _flags)


def sparse_mla_fwd_fp8_partial(q: torch.Tensor, kv_cache: torch.Tensor, indices: torch.Tensor, sm_scale: float, num_splits: int, d_v: int = 512,
                               index_offsets: Optional[torch.Tensor] = None, partial_out: Optional[torch.Tensor] = None,
                               partial_lse: Optional[torch.Tensor] = None, sync: bool = False,
                               _flags: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """sparse_mla_fwd_partial over sparse_mla_fwd_fp8's paged fp8 latent cache, read in place (dga_sparse_mla_fwd_fp8_partial).  kv_cache is
    that function's, everything else sparse_mla_fwd_partial's.  Both partials are sparse_mla_fwd_partial(q, deq, ...)'s byte for byte
    wherever those are not NaN, NaN in exactly the same elements.  One launch, capturable; M == 0 returns without one."""
    return _smla_partial(True, q, kv_cache, indices, sm_scale, num_splits, d_v, index_offsets, partial_out, partial_lse, sync, _flags)


def sparse_mla_merge(partial_out: torch.Tensor, partial_lse: torch.Tensor, out: Optional[torch.Tensor] = None,
                     lse: Optional[torch.Tensor] = None, sync: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """The merge of attention partials (dga_sparse_mla_merge): partial_out float32 [P, M, Hq, 512] and partial_lse float32 [P, M, Hq]
    (natural log), both contiguous, 1 <= P <= 64 -- sparse_mla_fwd_partial's, or the (out, lse) of context-parallel ranks or of chunks of a
    longer list in float32 -- into out bfloat16 [M, Hq, 512] and lse float32 [M, Hq]:
    lse = ln sum_p exp(partial_lse[p]);  out = sum_p exp(partial_lse[p] - lse) partial_out[p];  every partial_lse -inf: +0 and -inf.
    Arithmetic, float32, nothing contracted, p ascending: M = max_p partial_lse[p] (a NaN passed over), mu = M or 0 when M = -inf;
    w_p = exp2((partial_lse[p] - mu) log2 e);  L = ((w_0 + w_1) + w_2) + ...;  N = ((w_0 po_0 + w_1 po_1) + w_2 po_2) + ...;
    out = RNE_bf16(N (1 / L)), lse = mu + ln 2 log2 L.  A split of lse -inf weighs 0 (its partial_out must be finite: the partial kernels
    write +0); a NaN partial_lse makes the head NaN.  With P = 1: out = RNE_bf16(partial_out[0]) and lse = partial_lse[0], bit for bit.
    One writer per element, no atomics; nothing of a split beyond P is read.  Returns (out, lse), the caller's when given.  One launch,
    capturable; M == 0 returns without one."""
    _require(partial_out.dim() == 4 and partial_out.dtype == torch.float32 and partial_out.shape[3] == SPARSE_MLA_D_V
             and partial_out.is_contiguous(), "partial_out must be a contiguous float32 [P, M, Hq, %d] tensor", SPARSE_MLA_D_V)
    p, m, heads = partial_out.shape[0], partial_out.shape[1], partial_out.shape[2]
    _require(1 <= p <= SPARSE_MLA_MAX_SPLITS, "partial_out must hold between 1 and %d splits, got %d", SPARSE_MLA_MAX_SPLITS, p)
    _require(heads % 16 == 0 and 16 <= heads <= SPARSE_MLA_MAX_HEADS, "Hq must be a multiple of 16 in [16, %d], got %d",
             SPARSE_MLA_MAX_HEADS, heads)
    _want(partial_lse, "partial_lse", torch.float32, (p, m, heads))
    _require(partial_out.data_ptr() % 16 == 0, "partial_out must be 16-byte aligned")
    out, lse = _smla_outputs(out, lse, m, heads, partial_out.device)
    # (M == 0: the C entry returns before any launch)
    _launch("sparse_mla_merge", (partial_out, partial_lse, out, lse), lambda L, stream: L.dga_sparse_mla_merge(
        partial_out.data_ptr(), partial_lse.data_ptr(), p, m, heads, out.data_ptr(), lse.data_ptr(), stream), sync)
    return out, lse


def sparse_mla_num_splits(m: int, heads: int, topk: int, device=None) -> int:
    """The number of splits sparse_mla_fwd_split(num_splits=None) runs M tokens of Hq = heads heads and topk positions with
    (dga_sparse_mla_splits): max(1, min(CUs // (M head_blocks), tiles // 4, 64)), head_blocks = ceil(Hq / 64), tiles = ceil(topk / 32) -- as
    many splits as the device has idle compute units for, none shorter than four tiles (DGA_SPARSE_MLA_MIN_TILES: DESIGN.md has the sweep
    behind it), 1 once M head_blocks workgroups fill the device.  The CU count is the library's, of `device` or of the current device."""
    _require(all(isinstance(x, int) and x >= 1 for x in (m, heads, topk)), "m, heads and topk must be ints >= 1")
    with _NO_GUARD if device is None else torch.cuda.device(device):
        return int(_lib.lib().dga_sparse_mla_splits(m, heads, topk, 0))


def _smla_split(fp8: bool, q, rows, indices, sm_scale, d_v, index_offsets, num_splits, out, lse, sync: bool):
    """The body of sparse_mla_fwd_split / sparse_mla_fwd_fp8_split: the checks, once.  num_splits=None: the rule, on q's device; a rule of 1
    is the one-pass body on what has been checked.  Otherwise the partial entry and the merge, two launches on one stream, the partials in
    scratch of that device and stream."""
    checked = m, heads, topk, args = _smla_problem(fp8, q, rows, indices, sm_scale, d_v, index_offsets)
    if num_splits is None:
        if q.is_cuda and m:
            with _device_guard(q):
                num_splits = int(_lib.lib().dga_sparse_mla_splits(m, heads, topk, 0))
        if num_splits is None or num_splits == 1:
            return _smla_one_pass(fp8, q, rows, indices, sm_scale, d_v, index_offsets, out, lse, sync, 0, checked)
    name = _SMLA_ENTRY[fp8]
    p = _smla_splits(num_splits, topk)
    out, lse = _smla_outputs(out, lse, m, heads, q.device)

    def call(L, stream):
        n = p * m * heads
        ws, _ = _scratch("sparse_mla_split", out.device, n * (SPARSE_MLA_D_V + 1) * 4, stream)
        pl = None if ws is None else ws + n * SPARSE_MLA_D_V * 4
        return getattr(L, "dga_" + name + "_partial")(
            q.data_ptr(), rows.data_ptr(), indices.data_ptr(), _ptr(index_offsets), *args, 0, p, None, ws, pl, stream) or L.dga_sparse_mla_merge(
            ws, pl, p, m, heads, out.data_ptr(), lse.data_ptr(), stream)
    _launch(name + "_split", (q, rows, indices, index_offsets, out, lse), call, sync)
    return out, lse


def sparse_mla_fwd_split(q: torch.Tensor, kv: torch.Tensor, indices: torch.Tensor, sm_scale: float, d_v: int = 512,
                         index_offsets: Optional[torch.Tensor] = None, num_splits: Optional[int] = None, out: Optional[torch.Tensor] = None,
                         lse: Optional[torch.Tensor] = None, sync: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """sparse_mla_fwd for low-batch decode: the list split over num_splits workgroups a token and head block, and merged.  Arguments and
    result are sparse_mla_fwd's.  num_splits=None applies sparse_mla_num_splits(M, Hq, topk) on q's device; when that is 1 -- M head_blocks
    workgroups fill the device, or the list is short -- the call is sparse_mla_fwd itself, one launch.  An explicit num_splits in [1, 64], 1
    included, always runs sparse_mla_fwd_partial and sparse_mla_merge: two launches on one stream, no memset, no flags, no atomics,
    capturable -- a replayed graph follows new q, kv, indices and offsets -- with the partials in library scratch of that device and
    stream.  The result is sparse_mla_merge(*sparse_mla_fwd_partial(..., num_splits)) byte for byte; with num_splits=1 sparse_mla_fwd's
    bytes; otherwise within the bound of DESIGN.md, "Split-topk sparse MLA decode", of the exact result; NaN where sparse_mla_fwd has it."""
    return _smla_split(False, q, kv, indices, sm_scale, d_v, index_offsets, num_splits, out, lse, sync)


def sparse_mla_fwd_fp8_split(q: torch.Tensor, kv_cache: torch.Tensor, indices: torch.Tensor, sm_scale: float, d_v: int = 512,
                             index_offsets: Optional[torch.Tensor] = None, num_splits: Optional[int] = None,
                             out: Optional[torch.Tensor] = None, lse: Optional[torch.Tensor] = None,
                             sync: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """sparse_mla_fwd_split over sparse_mla_fwd_fp8's paged fp8 latent cache: num_splits=None and a rule of 1 is sparse_mla_fwd_fp8 itself, an
    explicit num_splits runs sparse_mla_fwd_fp8_partial and sparse_mla_merge.  The result is sparse_mla_fwd_split(q, deq, ...)'s."""
    return _smla_split(True, q, kv_cache, indices, sm_scale, d_v, index_offsets, num_splits, out, lse, sync)


def mla_kv_cast_to_fp8_paged(kv_c: torch.Tensor, k_pe: torch.Tensor, kv_cache: torch.Tensor, slot_mapping: torch.Tensor,
                             use_ue8m0: bool = False, sync: bool = False) -> torch.Tensor:
    """The writer of sparse_mla_fwd_fp8's cache (dga_cast_mla_kv_to_fp8_paged).  kv_c [T, 512] and k_pe [T, 64], float32 / bfloat16 /
    float16 and both of one dtype, each with a contiguous last dimension and a row stride of its own, 16-byte aligned with rows a multiple
    of 16 bytes apart (x[:, :512] and x[:, 512:] of one [T, 576] tensor are valid); kv_cache as there; slot_mapping int64 [T] on the device.
    For every t with 0 <= slot_mapping[t] < S, row slot receives the 512 codes and 4 scales of per_token_cast_to_fp8(kv_c,
    use_ue8m0=...) row t, byte for byte, and the rope part RNE_bf16(k_pe[t]) (bfloat16 input: its bits).  Any other slot value (engines pad
    with -1) skips the token, whose inputs are not read; no other byte of the cache is touched.  Duplicate valid slots in one call are the
    caller's error.  T == 0 returns without a launch.  Returns kv_cache."""
    _require(kv_c.dim() == 2 and kv_c.shape[1] == SPARSE_MLA_D_V, "kv_c must be a [T, %d] tensor", SPARSE_MLA_D_V)
    t = kv_c.shape[0]
    _require(k_pe.dim() == 2 and k_pe.shape == (t, SPARSE_MLA_D_QK - SPARSE_MLA_D_V), "k_pe must be a [T, %d] tensor with kv_c's T",
             SPARSE_MLA_D_QK - SPARSE_MLA_D_V)
    _require(kv_c.dtype in _CAST_DT, "kv_c must be float32, bfloat16 or float16")
    _require(k_pe.dtype == kv_c.dtype, "kv_c and k_pe must have one dtype, got %s and %s", kv_c.dtype, k_pe.dtype)
    size = kv_c.element_size()
    strides = []
    for x, what in ((kv_c, "kv_c"), (k_pe, "k_pe")):
        ld = x.stride(0) if t > 1 else x.shape[1]
        _require(x.stride(1) == 1 and ld >= x.shape[1] and ld * size % 16 == 0 and x.data_ptr() % 16 == 0,
                 "%s must have a contiguous last dimension, a 16-byte aligned base and rows a multiple of 16 bytes apart", what)
        strides.append(ld)
    nb, page, stride = _mla_fp8_cache(kv_cache)
    _want(slot_mapping, "slot_mapping", torch.int64, (t,))
    # (T == 0: the C entry returns before any launch)
    _launch("mla_kv_cast_to_fp8_paged", (kv_c, k_pe, kv_cache, slot_mapping), lambda L, stream: L.dga_cast_mla_kv_to_fp8_paged(
        kv_c.data_ptr(), strides[0], k_pe.data_ptr(), strides[1], _CAST_DT[kv_c.dtype], t, kv_cache.data_ptr(), nb, page, stride,
        slot_mapping.data_ptr(), _lib.CAST_UE8M0 if use_ue8m0 else 0, stream), sync)
    return kv_cache


def route_tokens(expert_ids: torch.Tensor, groups: int):
    """(counts int64 [groups], pos int64 [T]): pos[t] = slot of token t in the expert-sorted order (dga_route_tokens)."""
    _require(expert_ids.dtype == torch.int64 and expert_ids.dim() == 1 and expert_ids.is_contiguous(), "expert_ids int64 [T]")
    counts = torch.empty((groups,), dtype=torch.int64, device=expert_ids.device)
    pos = torch.empty((expert_ids.numel(),), dtype=torch.int64, device=expert_ids.device)
    _launch("route_tokens", (expert_ids,), lambda L, stream: L.dga_route_tokens(
        expert_ids.data_ptr(), expert_ids.numel(), groups, counts.data_ptr(), pos.data_ptr(), stream))
    return counts, pos


def route_slots(keys: torch.Tensor, key_stride_bytes: int, rows: int, buckets: int, cap: int, counts: torch.Tensor,
                dest: torch.Tensor, overflow: torch.Tensor, key_div: int = 1, key_sub: int = 0, key_mul: int = 1,
                zero_counts: bool = True, tags: Optional[torch.Tensor] = None, tag_stride_bytes: int = 0,
                keys_byte_offset: int = 0, tags_byte_offset: int = 0, inverse: Optional[torch.Tensor] = None,
                inverse_base: int = 0) -> None:
    """Capacity-bounded slot assignment on the device (dga_route_slots): dest[r] = bucket(key_r) * cap + next free slot,
    -1 for unused rows and for rows of a full bucket (which also raises the sticky device flag `overflow`);
    inverse[dest[r]] = r + inverse_base (the slot -> row table of the indexed grouped GEMM)."""
    if inverse is not None:
        _require(inverse.dtype == torch.int64 and inverse.numel() >= buckets * cap and inverse.is_contiguous(),
                 "inverse int64[buckets * cap]")
    _require(counts.dtype == torch.int32 and counts.numel() >= buckets and counts.is_contiguous(), "counts int32[buckets]")
    _require(dest.dtype == torch.int64 and dest.numel() >= rows and dest.is_contiguous(), "dest int64[rows]")
    _require(overflow.dtype == torch.int32 and overflow.numel() >= 1, "overflow int32[1]")
    _launch("route_slots", (dest, keys, counts, overflow), lambda L, stream: L.dga_route_slots(
        keys.data_ptr() + keys_byte_offset, key_stride_bytes, rows, key_div, key_sub, key_mul, buckets, cap, counts.data_ptr(),
        1 if zero_counts else 0, dest.data_ptr(), (tags.data_ptr() + tags_byte_offset) if tags is not None else None, tag_stride_bytes,
        overflow.data_ptr(), _ptr(inverse), inverse_base, stream))


def copy_rows(dst: torch.Tensor, src: torch.Tensor, dst_index: Optional[torch.Tensor] = None,
              src_index: Optional[torch.Tensor] = None, rows: Optional[int] = None, row_bytes: Optional[int] = None,
              dst_byte_offset: int = 0, src_byte_offset: int = 0) -> None:
    """Indexed row copy between 2-D (row-strided) device tensors viewed as bytes (dga_copy_rows)."""
    _require(dst.dim() == 2 and src.dim() == 2 and dst.stride(1) == 1 and src.stride(1) == 1, "2-D row tensors")
    n = rows if rows is not None else (dst_index.numel() if dst_index is not None else
                                       src_index.numel() if src_index is not None else src.shape[0])
    rb = row_bytes if row_bytes is not None else min(dst.shape[1] * dst.element_size(), src.shape[1] * src.element_size())
    for ix in (dst_index, src_index):
        if ix is not None:
            _require(ix.dtype == torch.int64 and ix.is_contiguous() and ix.numel() >= n, "index must be int64[rows]")
    _launch("copy_rows", (dst, src), lambda L, stream: L.dga_copy_rows(
        dst.data_ptr() + dst_byte_offset, dst.stride(0) * dst.element_size(), _ptr(dst_index),
        src.data_ptr() + src_byte_offset, src.stride(0) * src.element_size(), _ptr(src_index), rb, n, stream))


def copy_rows2(dst0, src0, bytes0, dst1, src1, bytes1, dst_index=None, src_index=None, rows=None,
               dst0_off=0, src0_off=0, dst1_off=0, src1_off=0) -> None:
    """Two indexed row copies with shared indices in one launch (dga_copy_rows2); tensors are 2-D row tensors viewed as
    bytes, *_off are byte offsets inside a row."""
    for t in (dst0, src0, dst1, src1):
        _require(t.dim() == 2 and t.stride(1) == 1, "2-D row tensors")
    n = rows if rows is not None else (dst_index.numel() if dst_index is not None else
                                       src_index.numel() if src_index is not None else src0.shape[0])
    rs = lambda t: t.stride(0) * t.element_size()
    _launch("copy_rows2", (dst0, src0, dst1, src1), lambda L, stream: L.dga_copy_rows2(
        dst0.data_ptr() + dst0_off, rs(dst0), src0.data_ptr() + src0_off, rs(src0), bytes0,
        dst1.data_ptr() + dst1_off, rs(dst1), src1.data_ptr() + src1_off, rs(src1), bytes1, _ptr(dst_index), _ptr(src_index), n, stream))


# ----------------------------------------------------------------------------- the framework's 16-bit entry points

def _dt16(t: torch.Tensor) -> int:
    if t.dtype == torch.bfloat16:
        return _lib.DT_BF16
    if t.dtype == torch.float16:
        return _lib.DT_FP16
    raise DGAError(-3, "dtype", f"expected bfloat16/float16, got {t.dtype}")


def run_mmad_rtc(x: torch.Tensor, y: torch.Tensor, z: torch.Tensor) -> None:
    """z[B,M,N] (f32, in place) = x[B,M,K] @ y[B,K,N]  (python_api.cpp:18, gemm.hpp:68-111). Synchronous, as the reference."""
    _require(x.dim() == 3 and y.dim() == 3 and z.dim() == 3, "rank must be 3")
    batch, m, k = x.shape
    _, k2, n = y.shape
    _require(k == k2 and y.shape[0] == batch and tuple(z.shape) == (batch, m, n), "shape mismatch")
    _require(z.dtype == torch.float32 and x.dtype == y.dtype, "dtype mismatch")
    for t in (x, y, z):
        _require(t.is_contiguous(), "operands must be contiguous")
    with _device_guard(x, y, z):
        ws_ptr, ws_bytes = _mmad_workspace(batch, m, n, k, x)
        rc = _lib.lib().dga_run_mmad_rtc_ws(x.data_ptr(), y.data_ptr(), z.data_ptr(), batch, m, n, k, _dt16(x),
                                            ws_ptr, ws_bytes, _stream_ptr(z))
        _lib.check(rc, "run_mmad_rtc")
        torch.cuda.current_stream(z.device).synchronize()  # gemm.hpp:110


def run_mmad_bench(x: torch.Tensor, y: torch.Tensor, z: torch.Tensor, params: torch.Tensor) -> None:
    """z[M,N] (f32) = x[M,K] @ y[K,N]; params int32[28]: slots 0..5 knobs in, 6..27 written back
    (python_api.cpp:23, gemm_bench.hpp:49-113)."""
    _require(x.dim() == 2 and y.dim() == 2 and z.dim() == 2, "rank must be 2")
    m, k = x.shape
    k2, n = y.shape
    _require(k == k2 and tuple(z.shape) == (m, n), "shape mismatch")
    _require(params.dtype == torch.int32 and params.numel() == 28, "params must be int32[28]")
    host = params.detach().cpu().tolist()          # the reference does 6 .item() syncs (gemm_bench.hpp:52-57)
    filled = bench_params_fill(m, n, k, host[:6])
    params.copy_(torch.tensor(filled, dtype=torch.int32))  # gemm_bench.hpp:79-81
    with _device_guard(x, y, z):
        arr = (ctypes.c_int32 * 28)(*filled)
        ws_ptr, ws_bytes = _mmad_workspace(1, m, n, k, x)
        rc = _lib.lib().dga_run_mmad_bench_ws(x.data_ptr(), y.data_ptr(), z.data_ptr(), m, n, k, _dt16(x), arr,
                                              ws_ptr, ws_bytes, _stream_ptr(z))
        _lib.check(rc, "run_mmad_bench")
        torch.cuda.current_stream(z.device).synchronize()


def run_mmad_custom(x: torch.Tensor, y: torch.Tensor, z: torch.Tensor) -> None:
    """The reference's static kernel returns immediately (include/impls/mmad.cpp:79): a no-op, kept for API parity."""
    return None
