"""The 16-bit GEMM family (csrc/dga_b16.hip, gemm_b16_kernel.hpp, gemm_b16_wsk_kernel.hpp, gemm_b16_w4_kernel.hpp, dga_b16_w4.hip)
BIT FOR BIT against a float64 matmul on exactly summable operands (tests/b16_cases.py): small integer-valued inputs make every
partial sum an integer below 2^24, so the fp32 result is the exact sum in any order and the 16-bit result its round-to-nearest-even
-- no tolerance, for every plan, split-K slicing, tile, wave grid and route.  Then the edges nothing else feeds these kernels:
rounding at the fp16 overflow boundary and at hand-placed bf16 ties, NaN / Inf / -0 / subnormal inputs, K = 0, operands at unaligned
addresses and with poisoned memory around them.  The entry points are the ones shared with the reference: the operator
(/root/reference/aclnn_catlass_dynamic_matmul/op_kernel/catlass_dynamic_matmul.cpp:16-45) and run_mmad_rtc / run_mmad_bench
(/root/reference/deep_gemm_ascend/framework/csrc/jit_kernels/impls/gemm.hpp:68-111, gemm_bench.hpp:49-113)."""
import functools
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import b16_cases as C

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
DTYPES = [torch.bfloat16, torch.float16]
BIG = 1 << 28      # m n k from which the float64 reference is computed on the device (exact there too: integers below 2^53)


def _nt_make(dtype, m, n, k, seed=0):
    x, w = C.operands(dtype, m, n, k, seed)
    xd, wd = x.cuda(), w.cuda()
    s = C.exact(xd, wd) if m * n * k >= BIG else C.exact(x, w)
    return xd, wd, s


def _nn_make(dtype, batch, m, n, k, seed=0):
    x, y = C.operands(dtype, m, n, k, seed, "nn", batch=batch)
    xd, yd = x.cuda(), y.cuda()
    s = C.exact(xd, yd, "nn") if batch * m * n * k >= BIG else C.exact(x, y, "nn")
    return xd, yd, s


_small_nt, _large_nt = functools.lru_cache(maxsize=32)(_nt_make), functools.lru_cache(maxsize=2)(_nt_make)
_small_nn, _large_nn = functools.lru_cache(maxsize=32)(_nn_make), functools.lru_cache(maxsize=2)(_nn_make)


def _nt_case(dtype, m, n, k, seed=0):
    """x [M,K], w [N,K] on the device and the exact sums (numpy float64); computed once, shared, never written."""
    return (_large_nt if m * n > (1 << 21) else _small_nt)(dtype, m, n, k, seed)


def _nn_case(dtype, batch, m, n, k, seed=0):
    return (_large_nn if batch * m * n > (1 << 21) else _small_nn)(dtype, batch, m, n, k, seed)


def _op(dga, x, w, fill=float("nan")):
    out = torch.full((x.shape[0], w.shape[0]), fill, dtype=x.dtype, device="cuda")
    dga.catlass_dynamic_matmul(x, w.t(), out, sync=True)
    return out


def _rtc(dga, x, y):
    z = torch.full((x.shape[0], x.shape[1], y.shape[2]), float("nan"), dtype=torch.float32, device="cuda")
    dga.run_mmad_rtc(x, y, z)
    return z


def _lib():
    from deepgemm_ascend_amd import _lib as L
    return L


def _dt(dtype):
    return _lib().DT_BF16 if dtype == torch.bfloat16 else _lib().DT_FP16


def _op_c(x, w, out):
    """The operator's C entry with a NULL workspace."""
    m, k = x.shape
    rc = _lib().lib().dga_catlass_dynamic_matmul(x.data_ptr() or None, w.data_ptr() or None, out.data_ptr(), m, w.shape[0], k,
                                                 _dt(out.dtype), None, 0, None)
    torch.cuda.synchronize()
    assert rc == 0, rc
    return out


def _rtc_c(x, y, z):
    """run_mmad_rtc's C entry without a workspace."""
    b, m, k = x.shape
    rc = _lib().lib().dga_run_mmad_rtc(x.data_ptr(), y.data_ptr(), z.data_ptr(), b, m, y.shape[2], k, _dt(x.dtype), None)
    torch.cuda.synchronize()
    assert rc == 0, rc
    return z


# ---------------------------------------------------------------------------------------------------- every plan, forced

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tile", C.TILES)
@pytest.mark.parametrize("split", C.SPLITS)
@pytest.mark.parametrize("deep", ["0", "1"])
def test_operator_every_plan(dga, dtype, tile, split, deep):
    """Split 1: the tile epilogue's conversion (gemm_b16_kernel.hpp OUT16); split > 1: splitk_reduce_16_kernel."""
    m, n, k = C.MAIN
    x, w, s = _nt_case(dtype, m, n, k)
    with C.switches(plan=C.plan_of(tile, split), deep=deep):
        got = _op(dga, x, w)
    C.assert_exact(got, s, f"plan {tile} split {split} deep {deep}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tile", C.TILES)
@pytest.mark.parametrize("split", [1, 3])
@pytest.mark.parametrize("deep", ["0", "1"])
def test_operator_every_tile_on_padded_k(dga, dtype, tile, split, deep):
    """K % 64 != 0: both operands go through pad_rows into the workspace first."""
    m, n, _ = C.MAIN
    x, w, s = _nt_case(dtype, m, n, C.PAD_K)
    with C.switches(plan=C.plan_of(tile, split), deep=deep):
        got = _op(dga, x, w)
    C.assert_exact(got, s, f"plan {tile} split {split} deep {deep}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tile", C.TILES)
@pytest.mark.parametrize("split", C.SPLITS)
@pytest.mark.parametrize("n", [520, 523])
@pytest.mark.parametrize("k", [C.MAIN[2], C.PAD_K])
@pytest.mark.parametrize("deep", ["0", "1"])
def test_run_mmad_rtc_every_plan(dga, dtype, tile, split, n, k, deep):
    """fp32 out = the exact sums.  n = 520, K = 1344: y read in place (NN, ds_read_b64_tr_b16); n = 523: transpose_b16_kernel without
    vector loads and the scalar fp32 stores; K = 1000: the transposition with vector loads (n = 520) and pad_rows on x."""
    x, y, s = _nn_case(dtype, 2, C.MAIN[0], n, k)
    with C.switches(plan=C.plan_of(tile, split), deep=deep):
        got = _rtc(dga, x, y)
    C.assert_exact(got, s, f"plan {tile} split {split} deep {deep}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_run_mmad_bench_and_its_parameter_write_back(dga, dtype):
    m, n, k = C.MAIN
    x, y, s = _nn_case(dtype, 2, m, n, k)
    z = torch.full((m, n), float("nan"), dtype=torch.float32, device="cuda")
    knobs = [1, 1, 3, 8, 20, 10]
    params = torch.tensor(knobs + [0] * 22, dtype=torch.int32, device="cuda")
    with C.switches(plan="128,256,2"):
        dga.run_mmad_bench(x[1], y[1], z, params)
    C.assert_exact(z, s[1], "run_mmad_bench")
    p = params.cpu().tolist()
    assert p[:6] == knobs and p[6:10] == [m, n, k, 1] and p == dga.bench_params_fill(m, n, k, knobs)


# ---------------------------------------------------------------------------------------------------- the shipped rules

def _split_of(need, other, m, n):
    """The split-K factor a workspace-bytes answer holds: need = other + round256(s * m * n * 4) + 256."""
    slab = need - other - 256
    for s_ in range(2, 17):
        if slab == (s_ * m * n * 4 + 255) // 256 * 256:
            return s_
    return 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("route", ["wsk_rule_decode", "wsk_rule_two_row_tiles", "swept_wsk", "swept_tile", "cost_model"])
def test_operator_auto_planned_routes(dga, dtype, route):
    """No switch set: what runs is what ships (csrc/dga_b16.hip).
    wsk_rule_decode (8, 512, 2048): launch_b16_nt `wsk_rule`, m <= 16 arm (kp >= 1024, N K <= 32 M) -> launch_b16_wsk.
    wsk_rule_two_row_tiles (24, 1024, 2048): `wsk_rule`, 17..32-row arm (kp <= 4096, N K <= 16 M) -> launch_b16_wsk, TM = 2.
    swept_wsk (8, 4096, 14336): the one row of b16_plans_mi355x.inc with bm == 0 (`swept->bm == 0` in launch_b16_nt).
    swept_tile (20, 576, 7168): the row {32, 576, 7168, 16, 128, 8}, smallest N K of the table (b16_plan: `r && r->bm`); the
        workspace answer must hold the eight slabs of that row.
    cost_model (1000, 4100, 4096): b16_plan's `if (m > 64)` candidates loop (the shape the fuzz once found).
    The workspace answer of swept_tile is held to its split-K; run_mmad_rtc's is in the test below, the NULL-workspace one in
    test_operator_without_workspace."""
    m, n, k = C.AUTO_SHAPES[route]
    x, w, s = _nt_case(dtype, m, n, k)
    for name in ("DGA_B16_PLAN", "DGA_B16_DEEP", "DGA_B16_WSK", "DGA_B16_NO_TABLE", "DGA_B16_WSK_ODD"):
        assert name not in os.environ
    need = int(_lib().lib().dga_catlass_dynamic_matmul_workspace_bytes(m, n, k, x.data_ptr(), w.data_ptr()))
    if route == "swept_tile":
        assert _split_of(need, 0, m, n) == 8, need
    C.assert_exact(_op(dga, x, w), s, route)


@pytest.mark.parametrize("dtype", DTYPES)
def test_run_mmad_rtc_auto_planned_split_k(dga, dtype):
    """(1, 8, 2048, 4096), no switch: b16_plan falls through to its last rule (`tiles * 4 <= cus * 3 && ks_n >= 16`): 16-row tiles,
    split-K; dga_mmad_workspace_bytes = yT + slabs + 256 must say so (b16_workspace_bytes: x is read in place)."""
    b, m, n, k = 1, 8, 2048, 4096
    x, y, s = _nn_case(dtype, b, m, n, k)
    need = int(_lib().lib().dga_mmad_workspace_bytes(b, m, n, k, x.data_ptr()))
    assert _split_of(need, (b * n * k * 2 + 255) // 256 * 256, m, n) >= 2, need
    C.assert_exact(_rtc(dga, x, y), s, "run_mmad_rtc auto split-K")


# ---------------------------------------------------------------------------------------------------- workgroup split-K

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n,k", C.WSK_SHAPES)
def test_workgroup_split_k_every_instantiation(dga, dtype, m, n, k):
    """gemm_b16_wsk_kernel <1,4>, <2,3>, <3,2>, <1,3,2>, <2,2,2> (launch_b16_wsk's selection by `per` and `m > 16`; see
    b16_cases.WSK_SHAPES), $DGA_B16_WSK=1."""
    x, w, s = _nt_case(dtype, m, n, k, seed=m + n + k)
    with C.switches(wsk="1"):
        got = _op(dga, x, w)
    C.assert_exact(got, s, f"wsk {m} x {n} x {k}")


# ---------------------------------------------------------------------------------------------------- sub-tile tail

def _tail_shape(bm):
    """The smallest raster of bm x 256 tiles, 17 tile columns, with more tiles than CUs and a partial last round; ragged edges."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tn = 17
    tm = cus // tn + 1
    while (tm * tn) % cus == 0:
        tm += 1
    m = tm * bm - bm // 5
    assert (m + bm - 1) // bm * tn > cus and ((m + bm - 1) // bm * tn) % cus != 0
    return m, cus


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tile,sub", [("256,256", 128), ("256,256", 64), ("256,256", 32), ("128,256", 64), ("128,256", 32)])
@pytest.mark.parametrize("k", C.TAIL_KS)
@pytest.mark.parametrize("entry", ["operator", "run_mmad_rtc"])
def test_sub_tile_tail(dga, dtype, tile, sub, k, entry):
    """The last partial round of a 256 x 256 / 128 x 256 raster in sub-tiles (dga_b16.hip `go_tail`): a second launch whose tiles are
    addressed through tail_begin / tail_sub.  The operator at N = 4100 (ragged, scalar 16-bit stores at the edge), run_mmad_rtc at
    N = 4104 (y read in place, ragged)."""
    bm = int(tile.split(",")[0])
    m, cus = _tail_shape(bm)
    n = 4100 if entry == "operator" else 4104
    tiles = (m + bm - 1) // bm * ((n + 255) // 256)
    assert tiles > cus and tiles % cus != 0, (tiles, cus)
    with C.switches(plan=C.plan_of(tile, 1, sub)):
        if entry == "operator":
            x, w, s = _nt_case(dtype, m, n, k)
            got = _op(dga, x, w)
        else:
            x, y, s = _nn_case(dtype, 1, m, n, k)
            got = _rtc(dga, x, y)
    C.assert_exact(got, s, f"{entry} {m} x {n} x {k} plan {tile} tail {sub}")


# ---------------------------------------------------------------------------------------------------- process-wide switches

CHILD = r'''
import os, sys
sys.path[:0] = [%r, %r]
import numpy as np, torch
import deepgemm_ascend_amd as dga
import b16_cases as C
import test_b16_exact_gpu as T

def count(got, s):
    msg = C.mismatch(C.bits_of(got), C.want_bits(s, got.dtype), C.KIND[got.dtype])
    return 0 if msg is None else int(msg.split()[0])

for plan in (None, "256,256,1"):
    with C.switches(plan=plan):
        for dt in (torch.bfloat16, torch.float16):
            for (m, n, k) in C.CHILD_SHAPES:
                x, w = C.operands(dt, m, n, k, m + n + k)
                s = C.exact(x, w)
                out = torch.full((m, n), float("nan"), dtype=dt, device="cuda")
                dga.catlass_dynamic_matmul(x.cuda(), w.cuda().t(), out, sync=True)
                z = torch.full((1, m, n), float("nan"), dtype=torch.float32, device="cuda")
                dga.run_mmad_rtc(x.cuda()[None], w.t().contiguous().cuda()[None], z)
                print("CASE", plan, C.KIND[dt], m, n, k, "operator/run_mmad_rtc COUNTS", count(out, s), count(z[0], s))
        for dt in (torch.bfloat16, torch.float16):      # N = 523: run_mmad_rtc through the transposition whatever the switch
            m, n, k = C.CHILD_NN_ODD
            x, y = C.operands(dt, m, n, k, 5, "nn", batch=1)
            z = torch.full((1, m, n), float("nan"), dtype=torch.float32, device="cuda")
            dga.run_mmad_rtc(x.cuda(), y.cuda(), z)
            print("CASE", plan, C.KIND[dt], m, n, k, "run_mmad_rtc COUNTS", 0, count(z, C.exact(x, y, "nn")))
with C.switches(plan="256,256,1"):
    for dt in (torch.bfloat16, torch.float16):
        x, w, s, cols, bits = T._edge_case(dt, 300, 264, 320)
        out = torch.full((300, 264), float("nan"), dtype=dt, device="cuda")
        dga.catlass_dynamic_matmul(x.cuda(), w.cuda().t(), out, sync=True)
        print("CASE edges", C.KIND[dt], "all/planted COUNTS", count(out, s), int((C.bits_of(out)[T.EDGE_ROW, cols] != np.array(bits, np.uint16)).sum()))
'''


@pytest.mark.parametrize("env", [{"DGA_B16_W4": "1"}, {"DGA_B16_TRANSPOSE": "1"}, {"DGA_B16_PLAIN": "1"}, {"DGA_B16_RASTER": "1"},
                                 {"DGA_B16_RASTER": "3"}], ids=lambda e: "-".join(f"{k[8:]}{v}" for k, v in e.items()))
def test_process_wide_switches_in_a_child_process(env):
    """Switches the library reads once per process, each in a fresh child: $DGA_B16_W4=1 (the four-wave 32x32x16 build of the
    operator's unsplit 256 x 256 plan, gemm_b16_w4_kernel.hpp), $DGA_B16_TRANSPOSE=1 (run_mmad_rtc never reads y in place),
    $DGA_B16_PLAIN=1 (run_mmad_rtc's 256 x 256 tile without the continuous pipeline), $DGA_B16_RASTER (the raster group).  The child
    runs the operator and run_mmad_rtc, auto-planned and on the 256 x 256 tile (and run_mmad_rtc at N % 8 != 0: the transposed-y
    builds, with $DGA_B16_PLAIN the plain 256 x 256 one), computes the exact sums itself and prints the count of differing outputs
    per case; with the 256 x 256 plan also the rounding edges (fp16 overflow boundary, bf16 ties)."""
    e = dict(os.environ)
    for name in ("DGA_B16_W4", "DGA_B16_TRANSPOSE", "DGA_B16_PLAIN", "DGA_B16_RASTER", "DGA_B16_PLAN", "DGA_B16_DEEP", "DGA_B16_WSK"):
        e.pop(name, None)
    e.update(env)
    e["DGA_B16_DEV"] = "1"
    r = subprocess.run([sys.executable, "-c", CHILD % (str(ROOT), str(ROOT / "tests"))], env=e, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    cases = [l.split() for l in r.stdout.splitlines() if l.startswith("CASE")]
    assert len(cases) == 2 * 2 * (len(C.CHILD_SHAPES) + 1) + 2, r.stdout
    for c in cases:
        assert c[-3] == "COUNTS" and c[-2:] == ["0", "0"], r.stdout


# ---------------------------------------------------------------------------------------------------- no-workspace C entries

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("batch,m,n,k,odd", [(3, 150, 264, 100, True), (1, 130, 131, 96, False)])
def test_run_mmad_rtc_without_workspace_direct_kernel(dga, dtype, batch, m, n, k, odd):
    """dga_run_mmad_rtc -> mmad_nn_f32_kernel (no LDS, fragments gathered from global memory): an x at an address % 16 == 2 with
    K % 8 != 0 and batch 3 (element loads), and an aligned x with K % 8 == 0 (16-byte loads; N % 8 != 0 keeps the tile kernel out)."""
    x, y, s = _nn_case(dtype, batch, m, n, k)
    if odd:
        buf = torch.zeros(x.numel() + 1, dtype=dtype, device="cuda")
        buf[1:].copy_(x.reshape(-1))
        x = buf[1:].view(batch, m, k)
        assert x.data_ptr() % 16 == 2
    z = torch.full((batch, m, n), float("nan"), dtype=torch.float32, device="cuda")
    C.assert_exact(_rtc_c(x, y, z), s, "mmad_nn_f32_kernel")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m,n,k,route", [(150, 264, 72, "generic"), (150, 264, 192, "in_place"), (64, 4096, 1024, "unsplit")])
def test_operator_without_workspace(dga, dtype, m, n, k, route):
    """dga_catlass_dynamic_matmul with a NULL workspace: K % 64 != 0 -> gemm_b16_nt_generic_kernel (nothing to pad into); whole k
    steps -> the tile kernel on the operands where they lie; a plan that would split K (the workspace answer says so) runs unsplit
    (launch_b16_nt `if (!workspace) pl.splitk = 1`)."""
    x, w, s = _nt_case(dtype, m, n, k)
    if route == "unsplit":
        assert _split_of(int(_lib().lib().dga_catlass_dynamic_matmul_workspace_bytes(m, n, k, x.data_ptr(), w.data_ptr())), 0, m, n) >= 2
    out = torch.full((m, n), float("nan"), dtype=dtype, device="cuda")
    C.assert_exact(_op_c(x, w, out), s, route)


# ---------------------------------------------------------------------------------------------------- rounding at the edges

EDGE_ROW = 3
EDGE = {   # the sums planted at row EDGE_ROW, columns 1, 17, 33, ... and the bits they must round to
    torch.float16: ([65504, 65519, 65520, 65536, -65520], [0x7BFF, 0x7BFF, 0x7C00, 0x7C00, 0xFC00]),
    torch.bfloat16: ([257, 259, -257, 65536 + 256], [0x4380, 0x4382, 0xC380, 0x4780]),
}


def _edge_case(dtype, m, n, k):
    """Integer operands with row EDGE_ROW of x all ones and chosen rows of w summing to the values of EDGE[dtype]: fp16 thirty-two
    2047s (= 65504) plus a small remainder; bf16 256s and a remainder.  The large entries are spread over the whole of K, so that
    every split-K slice holds some.  Returns x, w (CPU), the exact sums, the planted columns and their bits."""
    x = C.int_operands(dtype, (m, k), 11)
    w = C.int_operands(dtype, (n, k), 12)
    x[EDGE_ROW] = 1.0
    sums, bits = EDGE[dtype]
    big = 2047 if dtype == torch.float16 else 256
    cols = [1 + 16 * i for i in range(len(sums))]
    for c, v in zip(cols, sums):
        cnt, rem = abs(v) // big, abs(v) % big
        assert cnt + 3 <= k and cnt * big + rem == abs(v)
        row = np.zeros(k)
        row[np.linspace(0, k - 4, cnt).astype(int)] = big
        assert (row != 0).sum() == cnt
        free = np.flatnonzero(row == 0)
        for j, piece in enumerate((rem // 2, rem - rem // 2)):       # the remainder in two pieces, both exactly representable
            row[free[-1 - j]] = piece
        w[c] = torch.from_numpy(np.sign(v) * row).to(dtype)
    s = C.exact(x, w)
    assert [int(v) for v in s[EDGE_ROW, cols]] == sums and np.abs(s).max() < 2 ** 24
    assert C.round16_bits(s, dtype)[EDGE_ROW, cols].tolist() == bits
    return x, w, s, cols, bits


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("route", ["tile", "splitk_reduce", "wsk", "generic"])
def test_rounding_at_the_edges(dga, dtype, route):
    """fp16: sums of exactly 65504, 65519, 65520, 65536 and -65520 -> 0x7BFF 0x7BFF 0x7C00 0x7C00 0xFC00 (the largest finite value,
    just below the midpoint to Inf, the midpoint -- ties to even: Inf --, beyond it, and its negative); bf16: the ties 257, 259, -257
    and 2^16 + 256 -> 256, 260, -256, 2^16.  Through every 16-bit output route: the tile epilogue, splitk_reduce_16_kernel, the
    workgroup split-K's combine, the element-wise kernel (the four-wave build: in the child process above)."""
    m, n, k = {"tile": (40, 264, 320), "splitk_reduce": (40, 264, 320), "wsk": (8, 264, 320), "generic": (40, 264, 328)}[route]
    x, w, s, cols, bits = _edge_case(dtype, m, n, k)
    xd, wd = x.cuda(), w.cuda()
    if route == "generic":
        got = _op_c(xd, wd, torch.full((m, n), float("nan"), dtype=dtype, device="cuda"))
    else:
        with C.switches(**{"tile": dict(plan="128,128,1", wsk="0"), "splitk_reduce": dict(plan="64,128,3", wsk="0"), "wsk": dict(wsk="1")}[route]):
            got = _op(dga, xd, wd)
    assert C.bits_of(got)[EDGE_ROW, cols].tolist() == bits, [hex(v) for v in C.bits_of(got)[EDGE_ROW, cols]]
    C.assert_exact(got, s, route)


# ---------------------------------------------------------------------------------------------------- special values

def _special_case(dtype, m, n, k):
    """One NaN in x; +Inf and -Inf in different rows of w; an exact 0 of x meeting the +Inf (-> NaN); a row of x all -0 (+0 against
    the finite rows of w -- the accumulators start at +0 --, NaN against the two infinite ones)."""
    x = C.int_operands(dtype, (m, k), 21)
    w = C.int_operands(dtype, (n, k), 22)
    kn, kp, km = (5 * k) // 9, k // 13, (7 * k) // 10       # the NaN lies in the middle slab of a three-way split
    x[7, kn] = float("nan")
    w[5, kp] = float("inf")
    w[n - 9, km] = float("-inf")
    x[2, kp] = 0.0
    x[4, kp] = 3.0
    x[m - 1] = -0.0
    s = C.exact_special(x, w)
    assert np.isnan(s[7]).all() and np.isnan(s[2, 5]) and s[4, 5] == np.inf and np.isnan(s[m - 1, 5]) and np.isnan(s[m - 1, n - 9])
    assert (s[m - 1, :5] == 0).all() and not np.signbit(s[m - 1, :5]).any()
    assert np.isinf(s[:, n - 9]).sum() > m // 2 and (s[:, n - 9] == np.inf).any() and (s[:, n - 9] == -np.inf).any()
    return x, w, s


SPECIAL_ROUTES = {   # entry, (m, n, k), switches
    "tile_unsplit": ("op", C.MAIN, dict(plan="128,128,1")),
    "tile_continuous": ("op", C.MAIN, dict(plan="256,256,1")),
    "split_k": ("op", C.MAIN, dict(plan="64,128,3", deep="0")),
    "wsk": ("op", (12, 520, 1344), dict(wsk="1")),
    "padded_k": ("op", (300, 520, 1000), dict(plan="128,256,1")),
    "generic": ("op_c", (150, 264, 1000), {}),
    "nn_in_place": ("rtc", C.MAIN, dict(plan="128,128,2")),
    "nn_transposed": ("rtc", (300, 523, 1344), dict(plan="128,128,1")),
    "direct": ("rtc_c", (150, 131, 100), {}),
}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("route", list(SPECIAL_ROUTES))
def test_special_values(dga, dtype, route):
    """NaN / +-Inf / -0 in integer operands against the float64 result: NaN positions must coincide (no sign or payload check),
    +-Inf must match with its sign, everything else bit for bit (b16_cases.mismatch)."""
    entry, (m, n, k), sw = SPECIAL_ROUTES[route]
    x, w, s = _special_case(dtype, m, n, k)
    xd, wd = x.cuda(), w.cuda()
    with C.switches(**sw):
        if entry == "op":
            got = _op(dga, xd, wd, fill=1.0)
        elif entry == "op_c":
            got = _op_c(xd, wd, torch.full((m, n), 1.0, dtype=dtype, device="cuda"))
        elif entry == "rtc":
            got = _rtc(dga, xd[None], wd.t().contiguous()[None])[0]
        else:
            got = _rtc_c(xd[None], wd.t().contiguous()[None], torch.full((1, m, n), 1.0, dtype=torch.float32, device="cuda"))[0]
    C.assert_exact(got, s, route)


# ---------------------------------------------------------------------------------------------------- subnormal inputs

def _subnormal_case(dtype, m=40, n=136, k=64):
    """fp16: x = j 2^-24 (|j| <= 1023, subnormal) against integers up to 128 with four +-1024 per row: every product and partial sum
    is a multiple of 2^-24 below 2^24 of them -- exactly held in fp32 in any order.  bf16: x = j 2^-133 (|j| <= 127, subnormal)
    against +-2^100 .. 2^102: multiples of 2^-33 below 2^24 of them.  The expectation is the IEEE value."""
    rng = np.random.default_rng(31)
    if dtype == torch.float16:
        x = rng.integers(-1023, 1024, size=(m, k)) * 2.0 ** -24
        w = rng.integers(-128, 129, size=(n, k)).astype(np.float64)
        for r in range(n):
            w[r, rng.choice(k, 4, replace=False)] = rng.choice([-1024.0, 1024.0], 4)
    else:
        x = rng.integers(-127, 128, size=(m, k)) * 2.0 ** -133
        w = rng.choice([-1.0, 1.0], size=(n, k)) * 2.0 ** rng.integers(100, 103, size=(n, k))
    xt, wt = torch.from_numpy(x).to(dtype), torch.from_numpy(w).to(dtype)
    assert np.array_equal(xt.double().numpy(), x) and np.array_equal(wt.double().numpy(), w)      # exactly representable
    tiny = 2.0 ** -14 if dtype == torch.float16 else 2.0 ** -126
    assert (np.abs(x) < tiny).all() and (x != 0).mean() > 0.9
    s = x @ w.T + 0.0
    unit = 2.0 ** -24 if dtype == torch.float16 else 2.0 ** -33
    assert (np.abs(x) @ np.abs(w).T / unit < 2 ** 24).all() and np.array_equal(s.astype(np.float32).astype(np.float64), s)
    return xt, wt, s


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("route", ["generic", "tile", "wsk", "run_mmad_rtc", "direct"])
def test_subnormal_inputs(dga, dtype, route):
    """Subnormal 16-bit inputs are numbers: the matrix instructions (v_mfma_f32_16x16x32_f16 / _bf16) must not flush them, as the
    element-wise kernel (software conversion + fma) does not."""
    x, w, s = _subnormal_case(dtype)
    m, n = s.shape
    xd, wd = x.cuda(), w.cuda()
    if route == "generic":      # K = 64 would take the tile kernel: drop to K = 63 for the element-wise one
        s = x[:, :63].double().numpy() @ w[:, :63].double().numpy().T + 0.0
        got = _op_c(xd[:, :63].contiguous(), wd[:, :63].contiguous(), torch.full((m, n), float("nan"), dtype=dtype, device="cuda"))
    elif route == "tile":
        with C.switches(plan="64,128,1", wsk="0"):
            got = _op(dga, xd, wd)
    elif route == "wsk":
        with C.switches(wsk="1"):
            got = _op(dga, xd[:16].contiguous(), wd)
        s = s[:16]
    elif route == "run_mmad_rtc":
        got = _rtc(dga, xd[None], wd.t().contiguous()[None])[0]
    else:
        got = _rtc_c(xd[None], wd[:-1].t().contiguous()[None], torch.full((1, m, n - 1), float("nan"), dtype=torch.float32, device="cuda"))[0]
        s = s[:, :-1]
    C.assert_exact(got, s, route)


# ---------------------------------------------------------------------------------------------------- K = 0

@pytest.mark.parametrize("dtype", DTYPES)
def test_k_zero_writes_plus_zero(dga, dtype):
    """An empty sum is +0: the operator through the wrapper and through the C entry (NULL operands allowed), run_mmad_rtc with k = 0,
    each over an `out` full of NaN."""
    m, n = 37, 150
    x, w = torch.empty((m, 0), dtype=dtype, device="cuda"), torch.empty((n, 0), dtype=dtype, device="cuda")
    zero = np.zeros((m, n))
    C.assert_exact(_op(dga, x, w), zero, "operator, wrapper")
    C.assert_exact(_op_c(x, w, torch.full((m, n), float("nan"), dtype=dtype, device="cuda")), zero, "operator, C entry")
    z = torch.full((2, m, n), float("nan"), dtype=torch.float32, device="cuda")
    dga.run_mmad_rtc(torch.empty((2, m, 0), dtype=dtype, device="cuda"), torch.empty((2, 0, n), dtype=dtype, device="cuda"), z)
    C.assert_exact(z, np.zeros((2, m, n)), "run_mmad_rtc")


# ---------------------------------------------------------------------------------------------------- guard bands, alignment

GUARD = 4096      # elements of poison / sentinel on either side


def _embedded(t, odd, poison=0xFFFF):
    """A copy of the 16-bit tensor `t` inside a larger buffer of NaN (0xFFFF) at an address % 16 == 0, or == 2 (`odd`)."""
    buf = torch.full((t.numel() + 2 * GUARD + 8,), poison - 0x10000, dtype=torch.int16, device="cuda")
    at = GUARD + (1 if odd else 0)
    v = buf[at:at + t.numel()].view(t.dtype).view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == (2 if odd else 0) and v.is_contiguous()
    return buf, v


def _out16(shape, dtype, odd):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD + 8,), 0x7FC1, dtype=torch.int16, device="cuda")
    at = GUARD + (1 if odd else 0)
    return buf, buf[at:at + n].view(dtype).view(shape), at


def _out32(shape, odd):
    """fp32 out at an address % 16 == 0, or == 4 (`odd`: the least offset a float array can lie at -- the scalar-store branch)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD + 8,), 0x7FC0A5A5, dtype=torch.int32, device="cuda")
    at = GUARD + (1 if odd else 0)
    v = buf[at:at + n].view(torch.float32).view(shape)
    assert v.data_ptr() % 16 == (4 if odd else 0)
    return buf, v, at


def _guards_untouched(buf, at, n, sentinel):
    b = buf.cpu().numpy()
    assert (b[:at] == sentinel).all() and (b[at + n:] == sentinel).all(), "the output's guard band was written"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("odd", [False, True], ids=["aligned", "odd"])
@pytest.mark.parametrize("sw", [{}, dict(plan="256,256,1"), dict(plan="128,256,1"), dict(plan="16,128,2", deep="1"), dict(wsk="1")],
                         ids=["auto", "256x256", "128x256", "16x128s2deep", "wsk"])
def test_operator_between_guard_bands(dga, dtype, odd, sw):
    """x, w and out inside larger buffers: NaN (0xFFFF) around the inputs, the sentinel 0x7FC1 around the output.  Aligned: the tile
    kernels and the workgroup split-K read the operands where they lie, ragged in M and N, so whatever the tile loop reads past
    the operands' ends ("the tile's following bytes, unused") is NaN -- and must reach no output.  Odd (each address % 16 == 2):
    the padded copies and the scalar 16-bit stores."""
    m, n, k = (12, 264, 192) if "wsk" in sw else C.SMALL
    x, w, s = _nt_case(dtype, m, n, k)
    (_, xe), (_, we) = _embedded(x, odd), _embedded(w, odd)
    buf, out, at = _out16((m, n), dtype, odd)
    with C.switches(**sw):
        dga.catlass_dynamic_matmul(xe, we.t(), out, sync=True)
    C.assert_exact(out, s, "in range")
    _guards_untouched(buf, at, m * n, 0x7FC1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("odd", [False, True], ids=["aligned", "odd"])
@pytest.mark.parametrize("sw", [{}, dict(plan="256,256,1"), dict(plan="128,256,1"), dict(plan="16,128,2", deep="1")],
                         ids=["auto", "256x256", "128x256", "16x128s2deep"])
def test_run_mmad_rtc_between_guard_bands(dga, dtype, odd, sw):
    """As above for run_mmad_rtc, batch 2.  Aligned: y [K,N] read in place through the transposing LDS reads.  Odd: x through
    pad_rows, y through transpose_b16_kernel's element loads, z (address % 16 == 4) through the scalar fp32 stores."""
    m, n, k = C.SMALL
    x, y, s = _nn_case(dtype, 2, m, n, k)
    (_, xe), (_, ye) = _embedded(x, odd), _embedded(y, odd)
    buf, z, at = _out32((2, m, n), odd)
    with C.switches(**sw):
        dga.run_mmad_rtc(xe, ye, z)
    C.assert_exact(z, s, "in range")
    _guards_untouched(buf, at, 2 * m * n, 0x7FC0A5A5)


@pytest.mark.parametrize("dtype", DTYPES)
def test_no_workspace_entries_between_guard_bands(dga, dtype):
    """The direct kernel (mmad_nn_f32_kernel) and the element-wise kernel on operands at odd addresses between NaN."""
    m, n, k = 150, 131, 100
    x, y, s = _nn_case(dtype, 1, m, n, k)
    (_, xe), (_, ye) = _embedded(x, True), _embedded(y, True)
    buf, z, at = _out32((1, m, n), True)
    C.assert_exact(_rtc_c(xe, ye, z), s, "direct")
    _guards_untouched(buf, at, m * n, 0x7FC0A5A5)
    (_, we) = _embedded(y[0].t().contiguous(), True)
    buf, out, at = _out16((m, n), dtype, True)
    C.assert_exact(_op_c(xe[0], we, out), s[0], "generic")
    _guards_untouched(buf, at, m * n, 0x7FC1)
