"""GPU: adamw_per_block_cast_to_fp8_transposed against its definition.  In every case w, m and v are compared bit for bit with the numpy
float32 reference (tests/adamw_ref.py; where the reference is a NaN the device's value must be a NaN) and every output with
per_block_cast_to_fp8_transposed on the w the call left behind, byte for byte and scale bit for scale bit: no tolerance anywhere.  Every
tensor the call writes lies in a buffer with canary values on both sides; the outputs go through out=, pre-filled with 0xA5 codes and
0x7FC0A5A5 scales, so an element the kernel leaves unwritten shows; grad is compared with what it held before."""
import numpy as np
import pytest
import torch

import adamw_ref as A

pytestmark = pytest.mark.gpu

SENTINEL_Q, SENTINEL_SF = 0xA5, 0x7FC0A5A5
CANARY = -12288.0                  # exact in bfloat16
PAD = 8                            # elements of canary on each side: 32 (16) bytes, so an aligned buffer gives a 16-byte aligned tensor
TORCH_DT = {"fp32": torch.float32, "bf16": torch.bfloat16}
HYPER = dict(beta1=A.BETA1, beta2=A.BETA2, eps=A.EPS, weight_decay=A.WD)


class Guarded:
    """A contiguous device tensor of `a`'s values `shift` elements past the canary in front of it."""
    def __init__(self, a, kind, shift=0):
        self.n, self.lo = a.size, PAD + shift
        self.buf = torch.full((a.size + 2 * PAD + shift,), CANARY, dtype=TORCH_DT[kind], device="cuda")
        self.t = self.buf[self.lo:self.lo + a.size].view(a.shape)
        self.t.copy_(torch.from_numpy(np.ascontiguousarray(a, np.float32)))
        assert self.t.is_contiguous() and bool(shift) == bool(self.t.data_ptr() % 16)

    def bits(self):
        view = torch.int32 if self.t.dtype == torch.float32 else torch.int16
        return self.t.view(view).cpu().numpy().view(np.uint32 if self.t.dtype == torch.float32 else np.uint16)

    def untouched_around(self):
        return bool((self.buf[:self.lo] == CANARY).all()) and bool((self.buf[self.lo + self.n:] == CANARY).all())


class Codes:
    """An output pair in sentinel-filled buffers: codes `shift` bytes into theirs, canaries behind both."""
    def __init__(self, shape_q, shape_sf, shift=0):
        nq, ns = int(np.prod(shape_q)), int(np.prod(shape_sf))
        self.nq, self.ns, self.lo = nq, ns, shift
        self.qbuf = torch.full((nq + 16 + shift,), SENTINEL_Q, dtype=torch.uint8, device="cuda")
        self.sbuf = torch.full((ns + 4,), SENTINEL_SF, dtype=torch.int32, device="cuda")
        self.q = self.qbuf[shift:shift + nq].view(shape_q)
        self.sf = self.sbuf[:ns].view(torch.float32).view(shape_sf)

    def pair(self):
        return (self.q, self.sf)

    def untouched_around(self):
        return bool((self.qbuf[:self.lo] == SENTINEL_Q).all()) and bool((self.qbuf[self.lo + self.nq:] == SENTINEL_Q).all()) \
            and bool((self.sbuf[self.ns:] == SENTINEL_SF).all())


def _out_shapes(shape):
    lead, (n, k) = tuple(shape[:-2]), shape[-2:]
    nb, kb = (n + 127) // 128, (k + 127) // 128
    return (lead + (k, n), lead + (kb, nb)), (lead + (n, k), lead + (nb, kb))


def _device_scalars(sc):
    return torch.from_numpy(np.ascontiguousarray(sc, np.float32)).cuda()


def _assert_same(name, got_bits, want_bits, want_values):
    bad = A.same_bits(got_bits, want_bits, want_values)
    assert bad[0].size == 0, f"{name}: {bad[0].size} of {got_bits.size} elements differ, first at {[int(i[0]) for i in bad]}: " \
                             f"{int(got_bits[bad][0]):#x} vs {int(want_bits[bad][0]):#x}"


def _run(dga, w, m, v, grad, sc, grad_dtype="fp32", moment="fp32", rowwise=False, ue8m0=False, shift=0, code_shift=0, hyper=HYPER):
    """One call on guarded copies of the float32 arrays (grad exact in grad_dtype, m and v in moment) with everything checked: -> the new
    (w, m, v) as float32 arrays of what the device holds, and the device outputs as the entry returned them."""
    W, M, V, Gr = Guarded(w, "fp32", shift), Guarded(m, moment, shift), Guarded(v, moment, shift), Guarded(grad, grad_dtype, shift)
    grad_before = Gr.bits().copy()
    ts, rs = _out_shapes(tuple(w.shape))
    T, R = Codes(*ts, shift=code_shift), Codes(*rs, shift=code_shift)
    out = (T.pair(), R.pair()) if rowwise else T.pair()
    scd = _device_scalars(sc)
    res = dga.adamw_per_block_cast_to_fp8_transposed(W.t, M.t, V.t, Gr.t, scd, rowwise=rowwise, use_ue8m0=ue8m0, out=out, sync=True, **hyper)
    h = {name: A.f32(x) for name, x in hyper.items()}
    w2, m2, v2 = A.step(w, m, v, grad, sc, h["beta1"], h["beta2"], h["eps"], h["weight_decay"])
    _assert_same("w", W.bits(), w2.view(np.uint32), w2)
    _assert_same("m", M.bits(), A.moment_bits(m2, moment), m2)
    _assert_same("v", V.bits(), A.moment_bits(v2, moment), v2)
    assert np.array_equal(Gr.bits(), grad_before), "grad was written"
    assert np.array_equal(scd.cpu().numpy().view(np.uint32), np.ascontiguousarray(sc, np.float32).view(np.uint32)), "step_scalars was written"
    for what, t in (("w", W), ("m", M), ("v", V), ("grad", Gr), ("qt / sft", T), ("q / sf", R)):
        assert t.untouched_around(), f"a canary beside {what} was overwritten"
    if not rowwise:
        assert bool((R.qbuf == SENTINEL_Q).all())
    # the codes: the stand-alone quantiser on the w the call left behind
    want = dga.per_block_cast_to_fp8_transposed(W.t, rowwise=rowwise, use_ue8m0=ue8m0, sync=True)
    rt, wt = (res[0], want[0]) if rowwise else (res, want)
    pairs = [("qt", rt[0], wt[0]), ("sft", rt[1], wt[1])] + ([("q", res[1][0], want[1][0]), ("sf", res[1][1], want[1][1])] if rowwise else [])
    assert rt[0].dtype == torch.float8_e4m3fn and rt[0].data_ptr() == T.q.data_ptr() and rt[1].data_ptr() == T.sf.data_ptr()
    for name, got, exp in pairs:
        assert got.shape == exp.shape, name
        if got.dtype == torch.float32:
            gb, eb = got.view(torch.int32), exp.view(torch.int32)
            assert not bool((gb == SENTINEL_SF).any()), f"{name}: a scale was not written"
        else:
            gb, eb = got.view(torch.uint8), exp.view(torch.uint8)
        nbad = int((gb != eb).sum())
        assert nbad == 0, f"{name}: {nbad} of {gb.numel()} differ from per_block_cast_to_fp8_transposed on the returned w"
    new = (W.t.cpu().numpy(), M.t.float().cpu().numpy(), V.t.float().cpu().numpy())
    return new, res


GRAD = pytest.mark.parametrize("grad_dtype", A.DTYPES, ids=["g32", "g16"])
MOMENT = pytest.mark.parametrize("moment", A.DTYPES, ids=["m32", "m16"])
ROWWISE = pytest.mark.parametrize("rowwise", [False, True], ids=["transposed", "rowwise"])
UE8M0 = pytest.mark.parametrize("ue8m0", [False, True], ids=["f32scale", "ue8m0"])
SC3 = A.scalars(3, A.LR, A.BETA1, A.BETA2)


@GRAD
@MOMENT
@ROWWISE
@UE8M0
@pytest.mark.parametrize("shape", A.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_shapes(dga, shape, ue8m0, rowwise, moment, grad_dtype):
    w, m, v, g = A.inputs(shape, grad_dtype, moment, seed=1)
    _, res = _run(dga, w, m, v, g, SC3, grad_dtype, moment, rowwise, ue8m0)
    if ue8m0:
        bits = (res[0] if rowwise else res)[1].view(torch.int32)
        assert bool(((bits & 0x007FFFFF) == 0).all()) and bool((bits > 0).all()), "a scale is not a power of two"


# ---- steps and scalars

SHAPE = (2, 136, 264)


@MOMENT
@pytest.mark.parametrize("case", ["step1", "step1000", "wd0", "lr0", "scale_half", "scale_zero"])
def test_steps_and_scalars(dga, case, moment):
    step, lr, gs, hyper = 3, A.LR, 1.0, dict(HYPER)
    zero = case == "step1"
    if case == "step1":
        step = 1
    elif case == "step1000":
        step = 1000
    elif case == "wd0":
        hyper["weight_decay"] = 0.0
    elif case == "lr0":
        lr = 0.0
    elif case == "scale_half":
        gs = 0.5
    elif case == "scale_zero":
        gs = 0.0
    w, m, v, g = A.inputs(SHAPE, "fp32", moment, seed=2, zero_moments=zero)
    (w2, m2, v2), _ = _run(dga, w, m, v, g, A.scalars(step, lr, A.BETA1, A.BETA2, gs), "fp32", moment, True, hyper=hyper)
    if case == "lr0":
        assert np.isfinite(w2).all() and np.array_equal(w2.view(np.uint32), w.view(np.uint32)), "lr = 0 changed the bits of w"
        assert not np.array_equal(m2, m)
    if case == "scale_zero":
        assert np.array_equal(m2, A.stored(np.float32(A.BETA1) * m, moment)) and not np.array_equal(w2, w)
    if case == "step1":
        assert (m2 != 0).any() and (v2 > 0).any()


@MOMENT
def test_three_consecutive_steps(dga, moment):
    """Each step is fed the state the device left: the moments as stored in their type."""
    w, m, v, _ = A.inputs(SHAPE, "fp32", moment, seed=3, zero_moments=True)
    for step in (1, 2, 3):
        g = A.inputs(SHAPE, "bf16", seed=10 + step)[3]
        (w, m, v), _ = _run(dga, w, m, v, g, A.scalars(step, A.LR, A.BETA1, A.BETA2), "bf16", moment, step == 2)
    assert np.isfinite(w).all() and (v > 0).any()


# ---- special values

@MOMENT
@ROWWISE
def test_nan_and_infinite_gradients_poison_their_own_elements(dga, moment, rowwise):
    """NaN, +Inf and -Inf gradients in an interior tile, an edge tile and the last element: w is NaN there and nowhere else, every other
    element and every scale is what the clean gradient gives (the poisoned elements are not their tiles' maxima: their w is 0), and the
    poisoned elements' codes are sign | 0x7F."""
    shape = (2, 136, 264)
    w, m, v, g = A.inputs(shape, "fp32", moment, seed=4)
    at = ((0, 3, 5), (0, 64, 127), (0, 127, 128), (1, 135, 263), (1, 130, 7), (0, 0, 256))
    for i in at:
        w[i] = 0.0
    (wc, mc, vc), clean = _run(dga, w, m, v, g, SC3, "fp32", moment, rowwise)
    gp = g.copy()
    for n, i in enumerate(at):
        gp[i] = (np.nan, np.inf, -np.inf)[n % 3]
    (wp, mp, vp), res = _run(dga, w, m, v, gp, SC3, "fp32", moment, rowwise)
    mask = np.zeros(shape, bool)
    for i in at:
        mask[i] = True
    assert np.isnan(wp[mask]).all() and not np.isnan(wp[~mask]).any()
    for a, b in ((wp, wc), (mp, mc), (vp, vc)):
        assert np.array_equal(a[~mask].view(np.uint32), b[~mask].view(np.uint32))
    for n, i in enumerate(at):
        if n % 3 == 0:
            assert np.isnan(mp[i]) and np.isnan(vp[i]), i
        else:
            assert mp[i] == (np.inf, -np.inf)[n % 3 - 1] and vp[i] == np.inf, i
    ct, pt = (clean[0], res[0]) if rowwise else (clean, res)
    assert torch.equal(ct[1].view(torch.int32), pt[1].view(torch.int32)), "a poisoned element changed a scale"
    qt_c, qt_p = ct[0].view(torch.uint8).cpu().numpy(), pt[0].view(torch.uint8).cpu().numpy()
    mask_t = np.swapaxes(mask, -1, -2)
    assert np.array_equal(qt_c[~mask_t], qt_p[~mask_t]) and ((qt_p[mask_t] & 0x7F) == 0x7F).all()
    if rowwise:
        q_c, q_p = clean[1][0].view(torch.uint8).cpu().numpy(), res[1][0].view(torch.uint8).cpu().numpy()
        assert np.array_equal(q_c[~mask], q_p[~mask]) and ((q_p[mask] & 0x7F) == 0x7F).all()


@MOMENT
@pytest.mark.parametrize("case", ["all_zero", "eps0", "tiny_grad", "zero_tile"])
def test_zeros_and_subnormals(dga, case, moment):
    shape = (2, 130, 136)
    w, m, v, g = A.inputs(shape, "fp32", moment, seed=5)
    hyper = dict(HYPER)
    if case == "all_zero":                      # zero gradient and state, eps > 0: w' = w1 exactly
        m[:], v[:], g[:] = 0, 0, 0
    elif case == "eps0":                        # eps = 0: 0 / 0 where v' = 0, ordinary elsewhere
        hyper["eps"] = 0.0
        m[0], v[0], g[0] = 0, 0, 0
    elif case == "tiny_grad":                   # v' = (0.05 g) g is subnormal or zero
        m[:], v[:] = 0, 0
        g[:] = np.where(g > 0, 1e-25, -1e-25).astype(np.float32)
        g[1, :, ::3] *= np.float32(1e4)
    else:                                       # a tile whose w' is all zero: scale 1, codes 0
        w[0, :128, :128], m[0, :128, :128], g[0, :128, :128] = 0, 0, 0
    (w2, m2, v2), res = _run(dga, w, m, v, g, SC3, "fp32", moment, True, hyper=hyper)
    (qt, sft), (q, sf) = res
    if case == "all_zero":
        assert np.array_equal(w2, w * (np.float32(1) - np.float32(SC3[0]) * np.float32(A.WD))) and not m2.any() and not v2.any()
    elif case == "eps0":
        assert np.isnan(w2[0]).all() and np.isfinite(w2[1]).all() and not m2[0].any()
        assert bool((sf[0] == 1.0).all()) and bool(((q[0].view(torch.uint8) & 0x7F) == 0x7F).all())
    elif case == "tiny_grad":
        tiny = np.float32(2.0 ** -126)
        assert (v2[0] < tiny).all() and (v2[0] == 0).any() and np.isfinite(w2).all()
        if moment == "fp32":
            assert ((v2 > 0) & (v2 < tiny)).any(), "no subnormal v' was kept"
    else:
        assert sf[0, 0, 0].item() == 1.0 and sft[0, 0, 0].item() == 1.0 and not bool(q[0, :128, :128].view(torch.uint8).any())
        assert not w2[0, :128, :128].any()


# ---- alignment, position, repeatability

@GRAD
@MOMENT
def test_unaligned_views(dga, grad_dtype, moment):
    """A shape that allows the 16- and 8-byte accesses on pointers that do not: w, m, v and grad one element into their storage, qt and q
    one byte into theirs.  The same bits as on aligned tensors, none outside."""
    w, m, v, g = A.inputs(SHAPE, grad_dtype, moment, seed=6)
    _, res = _run(dga, w, m, v, g, SC3, grad_dtype, moment, True, shift=1, code_shift=1)
    assert res[0][0].data_ptr() % 8 == 1 and res[1][0].data_ptr() % 8 == 1
    _, ref = _run(dga, w, m, v, g, SC3, grad_dtype, moment, True)
    for a, b in zip(res[0] + res[1], ref[0] + ref[1]):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_one_tensor_unaligned_at_a_time(dga):
    """The accesses are chosen per tensor: each of w, m, v, grad alone one element into its storage."""
    w, m, v, g = A.inputs((2, 136, 136), "bf16", "bf16", seed=7)
    want = A.step(w, m, v, g, SC3, *(A.f32(HYPER[n]) for n in ("beta1", "beta2", "eps", "weight_decay")))
    for odd in range(4):
        ts = [Guarded(a, kind, int(i == odd)) for i, (a, kind) in enumerate(((w, "fp32"), (m, "bf16"), (v, "bf16"), (g, "bf16")))]
        dga.adamw_per_block_cast_to_fp8_transposed(*(t.t for t in ts), _device_scalars(SC3), sync=True, **HYPER)
        _assert_same("w", ts[0].bits(), want[0].view(np.uint32), want[0])
        _assert_same("m", ts[1].bits(), A.moment_bits(want[1], "bf16"), want[1])
        _assert_same("v", ts[2].bits(), A.moment_bits(want[2], "bf16"), want[2])
        assert all(t.untouched_around() for t in ts)


def test_position_and_repeatability(dga):
    """A group's result is the same alone and as group 2 of 3, and two runs give the same bits."""
    w, m, v, g = A.inputs((3, 130, 200), "fp32", "bf16", seed=8)
    (w3, m3, v3), ((qt3, sft3), (q3, sf3)) = _run(dga, w, m, v, g, SC3, "fp32", "bf16", True)
    (w1, m1, v1), ((qt1, sft1), (q1, sf1)) = _run(dga, w[2:], m[2:], v[2:], g[2:], SC3, "fp32", "bf16", True)
    (wr, mr, vr), ((qtr, sftr), (qr, sfr)) = _run(dga, w, m, v, g, SC3, "fp32", "bf16", True)
    for a, b, c in ((w3, w1, wr), (m3, m1, mr), (v3, v1, vr)):
        assert np.array_equal(a[2:].view(np.uint32), b.view(np.uint32)) and np.array_equal(a.view(np.uint32), c.view(np.uint32))
    for a, b, c in ((qt3, qt1, qtr), (sft3, sft1, sftr), (q3, q1, qr), (sf3, sf1, sfr)):
        assert torch.equal(a[2:].view(torch.uint8), b.view(torch.uint8)) and torch.equal(a.view(torch.uint8), c.view(torch.uint8))


def test_without_out_and_the_2d_form(dga):
    """Without out= the results are new tensors; the 2-D form is the grouped form of one group."""
    w, m, v, g = A.inputs((1, 200, 136), "fp32", "fp32", seed=9)
    dev = lambda a: torch.from_numpy(a.copy()).cuda()
    sc = _device_scalars(SC3)
    t3 = [dev(a) for a in (w, m, v, g)]
    t2 = [dev(a[0]) for a in (w, m, v, g)]
    (qt3, sft3), (q3, sf3) = dga.adamw_per_block_cast_to_fp8_transposed(*t3, sc, rowwise=True, sync=True, **HYPER)
    (qt2, sft2), (q2, sf2) = dga.adamw_per_block_cast_to_fp8_transposed(*t2, sc, rowwise=True, sync=True, **HYPER)
    assert qt2.shape == (136, 200) and sft2.shape == (2, 2) and q2.shape == (200, 136) and qt3.dtype == torch.float8_e4m3fn
    for a, b in ((qt3[0], qt2), (sft3[0], sft2), (q3[0], q2), (sf3[0], sf2), (t3[0][0], t2[0]), (t3[1][0], t2[1]), (t3[2][0], t2[2])):
        assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ---- in the pipeline

@MOMENT
def test_captured_with_the_gemm_that_reads_it(dga, moment):
    """One captured graph of the operator (2-D [256, 384], rowwise) followed by gemm_fp8_fp8_bf16_nt of 128 rows of A on the (q, sf) it
    wrote; replayed after a new gradient and a new adamw_step_scalars(..., out=).  The replay equals the eager calls bit for bit."""
    n, k, rows = 256, 384, 128
    w, m, v, g1 = A.inputs((n, k), "bf16", moment, seed=20, zero_moments=True)
    g2 = A.inputs((n, k), "bf16", seed=21)[3]
    dt = TORCH_DT[moment]
    dev = lambda a, d=torch.float32: torch.from_numpy(a.copy()).to(d).cuda()
    gen = torch.Generator(device="cuda").manual_seed(3)
    aq, asf = dga.per_token_cast_to_fp8(torch.randn((rows, k), device="cuda", generator=gen).bfloat16())

    def state():
        ts, rs = _out_shapes((n, k))
        T, R = Codes(*ts), Codes(*rs)
        return {"w": dev(w), "m": dev(m, dt), "v": dev(v, dt), "g": dev(g1, torch.bfloat16), "sc": torch.zeros(4, device="cuda"),
                "out": (T.pair(), R.pair()), "y": torch.zeros((rows, n), dtype=torch.bfloat16, device="cuda")}

    def step(s):
        dga.adamw_per_block_cast_to_fp8_transposed(s["w"], s["m"], s["v"], s["g"], s["sc"], rowwise=True, out=s["out"], **HYPER)
        dga.gemm_fp8_fp8_bf16_nt((aq, asf), s["out"][1], s["y"])

    def give(s, number, grad):
        s["g"].copy_(dev(grad, torch.bfloat16))
        dga.adamw_step_scalars(number, A.LR, A.BETA1, A.BETA2, out=s["sc"])

    eager, graphed = state(), state()
    for number, grad in ((1, g1), (2, g2)):
        give(eager, number, grad)
        step(eager)
    torch.cuda.synchronize()

    give(graphed, 1, g1)
    saved = {name: graphed[name].clone() for name in ("w", "m", "v")}
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        step(graphed)                                     # the warm-up advances the state: it is put back below
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        step(graphed)
    torch.cuda.synchronize()
    for name, t in saved.items():
        graphed[name].copy_(t)
    torch.cuda.synchronize()
    graph.replay()                                        # step 1
    give(graphed, 2, g2)
    torch.cuda.synchronize()
    graph.replay()                                        # step 2
    torch.cuda.synchronize()
    b = lambda t: t.view(torch.uint8)
    for name in ("w", "m", "v", "y"):
        assert torch.equal(b(graphed[name]), b(eager[name])), name
    for got, want in zip(graphed["out"][0] + graphed["out"][1], eager["out"][0] + eager["out"][1]):
        assert torch.equal(b(got), b(want))
    # the eager chain itself: two steps of the reference, and a product that moved with the weights
    wr, mr, vr = w, m, v
    for number, grad in ((1, g1), (2, g2)):
        wr, mr, vr = A.step(wr, mr, vr, grad, A.scalars(number, A.LR, A.BETA1, A.BETA2), *(A.f32(HYPER[x]) for x in ("beta1", "beta2", "eps", "weight_decay")))
        mr, vr = A.stored(mr, moment), A.stored(vr, moment)
    assert np.array_equal(eager["w"].cpu().numpy().view(np.uint32), wr.view(np.uint32))
    assert eager["y"].float().abs().sum().item() > 0 and not np.array_equal(wr, w)
