"""GPU: the three fp8 quantisers (per_token_cast_to_fp8, per_block_cast_to_fp8, silu_and_mul_per_token_cast_to_fp8) where a wrong
kernel would pass tests on random data: quotients on the rounding ties of e4m3fn, every 16-bit input pattern, the block maximum in
every lane and element, the two- and four-block kernels, and a misaligned input.  Inputs: tests/cast_cases.py (their properties are
checked on the CPU in tests/test_cast_cases.py).  The reference is the oracle's quantiser; scales are compared as bits and codes as
bytes: there is no tolerance anywhere."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import cast_cases as C

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent

_T16 = {"bf16": torch.bfloat16, "fp16": torch.float16}
_REF = {}


def _ref(key, make):
    """A reference computed once and shared by the cases that need it (never written to)."""
    if key not in _REF:
        _REF[key] = make()
        for a in _REF[key]:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return _REF[key]


def _dev16(kind, bits):
    return torch.from_numpy(np.array(bits, np.uint16).view(np.int16)).cuda().view(_T16[kind])


def _u8(t):
    return t.view(torch.uint8).cpu().numpy()


def _same(gq, gsf, wq, wsf, x):
    """As test_cast_gpu._check: scales as uint32, codes as bytes, the first mismatch with its input."""
    gsf, wsf = np.ascontiguousarray(gsf, np.float32), np.ascontiguousarray(wsf, np.float32)
    assert gsf.shape == wsf.shape and gq.shape == wq.shape, (gsf.shape, wsf.shape, gq.shape, wq.shape)
    sbad = np.nonzero(gsf.view(np.uint32) != wsf.view(np.uint32))
    assert sbad[0].size == 0, f"{sbad[0].size} scales differ, first at {[int(i[0]) for i in sbad]}: " \
                              f"{gsf[sbad][0]!r} ({gsf.view(np.uint32)[sbad][0]:#x}) vs {wsf[sbad][0]!r} ({wsf.view(np.uint32)[sbad][0]:#x})"
    bad = np.nonzero(gq != wq)
    assert bad[0].size == 0, f"{bad[0].size} of {gq.size} codes differ, first at {[int(i[0]) for i in bad]}: " \
                             f"{gq[bad][0]:#x} vs {wq[bad][0]:#x} for x={x[bad][0]!r} ({np.float32(x[bad][0]).view(np.uint32):#x})"


def _run(fn, x_t, want, x_np, ue8m0):
    q, sf = fn(x_t, use_ue8m0=ue8m0)
    torch.cuda.synchronize()
    _same(_u8(q), sf.cpu().numpy(), want[0].reshape(q.shape), want[1].reshape(sf.shape), x_np.reshape(q.shape))


UE = pytest.mark.parametrize("ue8m0", [False, True], ids=["f32scale", "ue8m0"])


# ---- ties: x / s within two fp32 ULP of a midpoint between two e4m3fn values, scales inside, at both ends of and beyond the fast path

N_TIE = 4096


def _tie_ref(oracle, ue8m0):
    def make():
        x = C.tie_blocks(N_TIE, C.TIE_EXPS, 11)
        return (x,) + oracle.quant_1x128(x, ue8m0=ue8m0)
    return _ref(("ties", ue8m0), make)


@UE
@pytest.mark.parametrize("k", [128, 1024])
def test_ties_per_token(dga, oracle, k, ue8m0):
    x, wq, wsf = _tie_ref(oracle, ue8m0)            # a row of k is k / 128 of the blocks side by side: the same bytes in another shape
    _run(dga.per_token_cast_to_fp8, torch.tensor(x.reshape(-1, k)).cuda(), (wq, wsf), x, ue8m0)


@UE
def test_ties_per_block(dga, oracle, ue8m0):
    """32 tiles of 128 x 128 (as many elements as the 4096 blocks above), one maximum per tile, as a [512, 1024] matrix."""
    def make():
        x = C.tiles_to_matrix(C.tie_tiles(32, C.TIE_EXPS, 12), 8)
        return (x,) + oracle.quant_128x128(x, ue8m0=ue8m0)
    x, wq, wsf = _ref(("tie tiles", ue8m0), make)
    _run(dga.per_block_cast_to_fp8, torch.tensor(x).cuda(), (wq, wsf), x, ue8m0)


@UE
@pytest.mark.parametrize("h", [128, 512])
def test_ties_fused(dga, oracle, h, ue8m0):
    """gate = 32 everywhere, up = ties / 32 (normal: cast_cases.TIE_EXPS_FUSED): for gate >= 20 the kernel's contract is the quantiser
    on fl32(gate * up) byte for byte, and that product is the tie input exactly.  Every row, then the masked layout."""
    def make():
        x = C.tie_blocks(N_TIE, C.TIE_EXPS_FUSED, 13)
        return (x,) + oracle.quant_1x128(x, ue8m0=ue8m0)
    x, wq, wsf = _ref(("fused ties", ue8m0), make)
    rows = N_TIE * 128 // h
    xin = np.concatenate([np.full((rows, h), 32.0, np.float32), (x.reshape(rows, h) * np.float32(2.0 ** -5)).astype(np.float32)], axis=1)
    xt = torch.from_numpy(xin).cuda()
    q, sf = dga.silu_and_mul_per_token_cast_to_fp8(xt, use_ue8m0=ue8m0, sync=True)
    _same(_u8(q), sf.cpu().numpy(), wq.reshape(rows, h), wsf.reshape(rows, h // 128), x.reshape(rows, h))
    groups, mmax = 4, rows // 4
    counts = [mmax, 0, 5, mmax - 3]
    masked = torch.tensor(counts, dtype=torch.int32, device="cuda")
    q = torch.full((groups, mmax, h), 0xA5, dtype=torch.uint8, device="cuda")
    sf = torch.full((groups, mmax, h // 128), 0x7FC0A5A5, dtype=torch.int32, device="cuda").view(torch.float32)
    dga.silu_and_mul_per_token_cast_to_fp8(xt.view(groups, mmax, 2 * h), masked_m=masked, out=(q, sf), use_ue8m0=ue8m0, sync=True)
    gq, gsf = q.cpu().numpy().reshape(rows, h), sf.cpu().numpy().reshape(rows, h // 128)
    valid = np.concatenate([np.arange(counts[g]) + g * mmax for g in range(groups)]).astype(np.int64)
    rest = np.setdiff1d(np.arange(rows), valid)
    _same(gq[valid], gsf[valid], wq.reshape(rows, h)[valid], wsf.reshape(rows, h // 128)[valid], x.reshape(rows, h)[valid])
    assert (gq[rest] == 0xA5).all() and (gsf[rest].view(np.uint32) == 0x7FC0A5A5).all(), "a masked row was written"


# ---- every 16-bit input

def _all16_ref(oracle, kind, ue8m0):
    def make():
        bits = C.all_16bit_blocks(kind)
        x = C.bits16_to_f32(kind, bits)
        return (bits, x) + oracle.quant_1x128(x, ue8m0=ue8m0)
    return _ref(("all16", kind, ue8m0), make)


@UE
@pytest.mark.parametrize("kind", ["bf16", "fp16"])
def test_all_16bit_per_token(dga, oracle, kind, ue8m0):
    """All 65 536 patterns (NaN payloads of both signs, +-Inf, subnormals), each under several block maxima and under an infinite one."""
    bits, x, wq, wsf = _all16_ref(oracle, kind, ue8m0)
    _run(dga.per_token_cast_to_fp8, _dev16(kind, bits.reshape(-1, 1024)), (wq, wsf), x, ue8m0)


@UE
@pytest.mark.parametrize("kind", ["bf16", "fp16"])
def test_all_16bit_per_block(dga, oracle, kind, ue8m0):
    """The same blocks, each as a tile of its own: the block repeated down the tile, over the first 16 of its rows only (the matrix
    has 16 rows: the full 128 would be eight times the data for the same quotients) and rolled by 8 columns per row, so that every
    pattern passes through each of the 16 eight-element groups of a row.  The tile's maximum is the block's."""
    def make():
        bits = C.all_16bit_blocks(kind)
        m = np.stack([np.roll(bits, 8 * r, axis=1) for r in range(16)]).reshape(16, -1)
        x = C.bits16_to_f32(kind, m)
        return (m, x) + oracle.quant_128x128(x, ue8m0=ue8m0)
    bits, x, wq, wsf = _ref(("all16 tiles", kind, ue8m0), make)
    _run(dga.per_block_cast_to_fp8, _dev16(kind, bits), (wq, wsf), x, ue8m0)


# ---- the block maximum in every position of the reductions

def _to(x, dtype):
    t = torch.from_numpy(x).cuda().to(dtype)
    assert torch.equal(t.float().cpu(), torch.from_numpy(x)), "the case is not exact in this type"
    return t


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_amax_position_per_token(dga, oracle, dtype):
    x = C.one_hot_blocks("1x128")
    want = _ref("one hot 1x128", lambda: oracle.quant_1x128(x))
    _run(dga.per_token_cast_to_fp8, _to(x, dtype), want, x, False)
    _run(dga.per_token_cast_to_fp8, _to(np.ascontiguousarray(x.reshape(16, 1024)), dtype), want, x, False)
    # the fused kernel tracks the lane's maximum and its inputs by comparison: gate = 32, up = x / 32 (exact in both types)
    xin = np.concatenate([np.full_like(x, 32.0), x / np.float32(32.0)], axis=1)
    q, sf = dga.silu_and_mul_per_token_cast_to_fp8(_to(xin, dtype), sync=True)
    _same(_u8(q), sf.cpu().numpy(), want[0], want[1], x)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_amax_position_per_block(dga, oracle, dtype):
    x = C.one_hot_blocks("128x128").reshape(-1, 128)
    want = _ref("one hot 128x128", lambda: oracle.quant_128x128(x))
    assert (want[1].view(np.uint32) == (np.float32(100.0) / np.float32(448.0)).view(np.uint32)).all()
    _run(dga.per_block_cast_to_fp8, _to(x, dtype), want, x, False)


# ---- the two-block kernel that 16-bit inputs of 131 072 blocks and more run

@pytest.mark.parametrize("kind,rows,k,ue8m0", [("bf16", 3973, 4224, False), ("fp16", 4096, 4096, True)],
                         ids=["bf16-131109-blocks", "fp16-131072-blocks-ue8m0"])
def test_two_block_kernel(dga, oracle, kind, rows, k, ue8m0):
    """131 109 blocks: odd, the last group's second block is dead; 131 072: the threshold itself.  randn * 3 with tie rows (rounded
    to the type), a NaN and an all-zero block at the first block, at both sides of the seam between the kernel's two passes and at
    the last block."""
    kb = k // 128
    blocks = rows * kb
    assert blocks >= 131072 and k % 128 == 0
    g = torch.Generator(device="cuda").manual_seed(rows + k)
    x = (torch.randn((rows, k), device="cuda", generator=g) * 3.0).to(_T16[kind])
    flat = x.view(blocks, 128)
    half = (blocks + 1) // 2
    ties = torch.from_numpy(C.tie_blocks(8, range(-6, 7), 14)).cuda().to(_T16[kind])            # (inside fp16's range)
    for i, b in enumerate([0, half - 1, half, blocks - 1, 1, half - 2, half + 1, blocks - 2]):
        flat[b] = ties[i]
    flat[2, 77] = float("nan")
    flat[half + 2] = 0.0
    flat[blocks - 3, 5] = float("nan")
    flat[half - 3] = 0.0
    xn = x.float().cpu().numpy()
    want = oracle.quant_1x128(xn, ue8m0=ue8m0)
    _run(dga.per_token_cast_to_fp8, x, want, xn, ue8m0)


# ---- DGA_CAST_UNROLL = 2 and = 4: the switch is read once per process, so each value runs in one fresh child

CHILD = r'''
import sys
sys.path[:0] = [%r, %r]
import numpy as np
import torch
import deepgemm_ascend_amd as dga
from oracle import oracle as O
import cast_cases as C

bad = 0
for rows, k in [(1, 128), (5, 256), (5, 384), (7, 384)]:
    blocks = rows * k // 128
    ties = C.tie_blocks(blocks, C.TIE_EXPS, 15 + blocks).reshape(rows, k)
    g = torch.Generator(device="cuda").manual_seed(blocks)
    rnd = torch.randn((rows, k), device="cuda", generator=g) * 3.0
    for name, x in [("fp32 ties", torch.from_numpy(ties).cuda()), ("fp32", rnd), ("bf16", rnd.bfloat16()),
                    ("bf16 ties", torch.from_numpy(ties).cuda().bfloat16())]:
        for ue8m0 in (False, True):
            q, sf = dga.per_token_cast_to_fp8(x, use_ue8m0=ue8m0)
            torch.cuda.synchronize()
            xn = x.float().cpu().numpy()
            wq, wsf = O.quant_1x128(xn, ue8m0=ue8m0)
            gq, gsf = q.view(torch.uint8).cpu().numpy(), sf.cpu().numpy()
            ok = gq.shape == wq.shape and gsf.shape == wsf.shape and (gsf.view(np.uint32) == wsf.view(np.uint32)).all() and (gq == wq).all()
            print(rows, k, name, "ue8m0" if ue8m0 else "f32scale", "ok" if ok else
                  "MISMATCH: %%d scales, %%d codes" %% ((gsf.view(np.uint32) != wsf.view(np.uint32)).sum(), (gq != wq).sum()))
            bad += not ok
print("cases failed:", bad)
sys.exit(1 if bad else 0)
''' % (str(ROOT), str(ROOT / "tests"))


@pytest.mark.parametrize("unroll", [2, 4])
def test_unroll_switch(dga, unroll):
    """cast_1x128_unrolled_kernel<T, 2> and <T, 4> on 1, 10, 15 and 21 blocks (every remainder mod 4: dead blocks in the last
    groups), fp32 and bf16, against the oracle inside the child.  A child that fails is not run again."""
    env = dict(os.environ)
    env["DGA_CAST_UNROLL"] = str(unroll)
    r = subprocess.run([sys.executable, "-c", CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"exit status {r.returncode}\n{r.stdout[-4000:]}\n{r.stderr[-2000:]}"
    assert r.stdout.count(" ok") == 32 and "cases failed: 0" in r.stdout, r.stdout


# ---- an input that is contiguous but not 16-byte aligned: scalar loads on a k % 128 == 0 shape

@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_misaligned_input_pointer(dga, oracle, dtype):
    rows, k = 64, 512
    g = torch.Generator(device="cuda").manual_seed(21)
    buf = (torch.randn((rows * k + 8,), device="cuda", generator=g) * 3.0).to(dtype)
    x = buf[1:1 + rows * k].view(rows, k)
    assert x.is_contiguous() and x.data_ptr() % 16 == buf.element_size() and buf.data_ptr() % 16 == 0
    xn = x.float().cpu().numpy()
    for ue8m0 in (False, True):
        _run(dga.per_token_cast_to_fp8, x, oracle.quant_1x128(xn, ue8m0=ue8m0), xn, ue8m0)
        _run(dga.per_block_cast_to_fp8, x, oracle.quant_128x128(xn, ue8m0=ue8m0), xn, ue8m0)
