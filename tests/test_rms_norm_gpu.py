"""GPU: rms_norm_per_token_cast_to_fp8 and rms_norm_backward against tests/rms_norm_ref.py.  Forward: the 65 cases of
rms_norm_ref.FORWARD_CASES (every H of every geometry and of the bounded path, T not a multiple of the rows of a workgroup, the three types,
the weight in x's type and in float32, with and without residual, both scale kinds), every output pre-filled with sentinels: rstd inside
its bound against float64 on the z the device normalised; residual_out, norm_out, q and sf equal to the float32 definition on the RETURNED
rstd bit for bit, q and sf also equal to per_token_cast_to_fp8 run on the float32 y on the device; quantize=False and norm_out=False leave
the other outputs as they were; residual_out in place.  Then row independence, and the special rows.  Backward: float32 dx and dweight
inside their bounds against float64 (rstd as given), the 16-bit dx the RNE of the float32 one, grad_residual the separate sum bit for bit
(aliased and not), the same bits twice, and need_dweight=False leaving dx as it was."""
import numpy as np
import pytest
import torch

import rms_norm_ref as N
import router_ref as R

pytestmark = pytest.mark.gpu

EPS = N.EPS
SENT16 = 0x7FC1


def _dev(a, dtype="fp32"):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(N.TORCH_DT[dtype]).cuda()      # (converted on the host: exact values)


def _sentinels(dtype, *shape):
    """A tensor of `dtype` ('fp32', 'bf16', 'fp16', 'u8') full of a value no result takes."""
    if dtype == "u8":
        return torch.full(shape, 0xA5, dtype=torch.uint8, device="cuda")
    if dtype == "fp32":
        return torch.full(shape, R.SENTINEL_F32, dtype=torch.int32, device="cuda").view(torch.float32)
    return torch.full(shape, SENT16, dtype=torch.int16, device="cuda").view(N.TORCH_DT[dtype])


def _forward(dga, x, w, dtype, w_f32, res=None, ue8m0=False, quantize=True, norm_out=True, eps=EPS):
    """One call on pre-filled outputs -> dict of the outputs' bits (numpy) by name."""
    t_n, h = x.shape
    out = {"rstd": _sentinels("fp32", t_n)}
    if quantize:
        out["q"], out["sf"] = _sentinels("u8", t_n, h), _sentinels("fp32", t_n, (h + 127) // 128)
    if norm_out:
        out["norm"] = _sentinels(dtype, t_n, h)
    if res is not None:
        out["residual"] = _sentinels(dtype, t_n, h)
    got = dga.rms_norm_per_token_cast_to_fp8(_dev(x, dtype), _dev(w, "fp32" if w_f32 else dtype), eps=eps,
                                             residual=None if res is None else _dev(res, dtype), quantize=quantize, norm_out=norm_out,
                                             out=out, use_ue8m0=ue8m0, sync=True)
    for name in N_FIELDS:
        t = getattr(got, name)
        assert (t is None) == (name not in out) and (t is None or t.data_ptr() == out[name].data_ptr()), name
    assert got.q is None or got.q.dtype == torch.float8_e4m3fn
    return {name: N.bits_of(t) for name, t in out.items()}


N_FIELDS = ("q", "sf", "norm", "residual", "rstd")


def _check_forward(dga, oracle, x, res, w, dtype, w_f32, ue8m0, where, eps=EPS, nan_rows=(), overflow_rows=()):
    """Every check of one forward case -> the outputs' bits.  nan_rows: rstd must be NaN there; overflow_rows: the squares overflow float32,
    rstd must be 0; the bound on rstd holds on all other rows."""
    t_n, h = x.shape
    got = _forward(dga, x, w, dtype, w_f32, res, ue8m0, eps=eps)
    if res is None:
        z = x
    else:
        want, z = N.residual_ref(x, res, dtype)
        assert np.array_equal(got["residual"], want), where
    rstd = got["rstd"].view(np.float32)
    exact = N.rstd64(z, eps)
    ok_rows = np.setdiff1d(np.arange(t_n), list(nan_rows) + list(overflow_rows))
    err = np.abs(rstd.astype(np.float64) - exact)[ok_rows]
    worst = float((err / (N.rstd_bar(h) * exact[ok_rows])).max()) if len(ok_rows) else 0.0
    print(f"{where} rstd: worst error = {worst:.3f} of the bound")
    assert (err <= N.rstd_bar(h) * exact[ok_rows]).all(), (where, worst)
    assert np.isnan(rstd[list(nan_rows)]).all() and (rstd[list(overflow_rows)] == 0).all()
    y = N.y_ref(z, rstd, w)
    assert np.array_equal(got["norm"], N.norm_bits(y, dtype)), where
    q, sf = oracle.quant_1x128(y, ue8m0)
    assert np.array_equal(got["q"], q) and np.array_equal(got["sf"], sf.view(np.uint32)), where
    dq, dsf = dga.per_token_cast_to_fp8(torch.from_numpy(y).cuda(), use_ue8m0=ue8m0)
    torch.cuda.synchronize()
    assert np.array_equal(got["q"], N.bits_of(dq)) and np.array_equal(got["sf"], N.bits_of(dsf)), where
    return got


@pytest.mark.parametrize("h,t_n,dtype,w_f32,with_res,ue8m0", N.FORWARD_CASES)
def test_forward_cases(dga, oracle, h, t_n, dtype, w_f32, with_res, ue8m0):
    where = f"[{t_n},{h},{dtype},w_f32={w_f32},res={with_res},ue8m0={ue8m0}]"
    x, res, w = N.forward_inputs(h, t_n, dtype, w_f32)
    res = res if with_res else None
    full = _check_forward(dga, oracle, x, res, w, dtype, w_f32, ue8m0, where)
    # the same bits twice; fewer outputs leave the others as they were
    for kwargs in (dict(), dict(quantize=False), dict(norm_out=False)):
        part = _forward(dga, x, w, dtype, w_f32, res, ue8m0, **kwargs)
        assert len(part) == len(full) - 2 * ("quantize" in kwargs) - ("norm_out" in kwargs)
        for name, bits in part.items():
            assert np.array_equal(bits, full[name]), (where, kwargs, name)
    if with_res:
        # in place: residual_out is the residual itself, then x itself
        for alias in ("residual", "x"):
            d_x, d_res = _dev(x, dtype), _dev(res, dtype)
            got = dga.rms_norm_per_token_cast_to_fp8(d_x, _dev(w, "fp32" if w_f32 else dtype), eps=EPS, residual=d_res, norm_out=True,
                                                     out={"residual": d_res if alias == "residual" else d_x}, use_ue8m0=ue8m0, sync=True)
            assert got.residual.data_ptr() == (d_res if alias == "residual" else d_x).data_ptr()
            for name in N_FIELDS:
                assert np.array_equal(N.bits_of(getattr(got, name)), full[name]), (where, alias, name)


@pytest.mark.parametrize("h,dtype", [(136, "bf16"), (2056, "fp16"), (7168, "bf16"), (520, "fp32")])
def test_a_row_gives_the_same_bits_wherever_it_sits(dga, h, dtype):
    x, res, w = N.forward_inputs(h, 257, dtype, False, seed=3)
    row_x, row_res = x[100].copy(), res[100].copy()
    x[0], res[0], x[256], res[256] = row_x, row_res, row_x, row_res
    big = _forward(dga, x, w, dtype, False, res)
    one = _forward(dga, row_x[None], w, dtype, False, row_res[None])
    again = _forward(dga, x, w, dtype, False, res)
    for name in N_FIELDS:
        assert np.array_equal(big[name], again[name]), name                     # two runs, the same bits
        for r in (0, 100, 256):
            assert np.array_equal(big[name][r], one[name][0]), (name, r)


@pytest.mark.parametrize("h,dtype", [(129, "fp32"), (520, "bf16"), (2056, "fp16"), (7168, "bf16")])
def test_a_nan_touches_only_its_own_row(dga, oracle, h, dtype):
    x, res, w = N.forward_inputs(h, 5, dtype, True, seed=4)
    clean = _forward(dga, x, w, dtype, True, None)
    x[2, h // 3] = np.nan
    got = _check_forward(dga, oracle, x, None, w, dtype, True, False, f"NaN [{h},{dtype}]", nan_rows=(2,))
    assert np.isnan(got["rstd"].view(np.float32)[2]) and ((got["q"][2] & 0x7F) == 0x7F).all() and (got["sf"].view(np.float32)[2] == 1.0).all()
    assert np.isnan(N.from_bits(got["norm"][2], dtype)).all()
    keep = [0, 1, 3, 4]
    for name in clean:
        assert np.array_equal(got[name][keep], clean[name][keep]), name


@pytest.mark.parametrize("dtype", N.DTYPES)
def test_special_rows(dga, oracle, dtype):
    h = 520
    x, _, w = N.forward_inputs(h, 5, dtype, False, seed=5)
    w = N.to_dtype(np.abs(w) + np.float32(0.5), dtype)                            # positive: a row of zeros gives +0
    x[1] = 0.0                                                                    # a row of zeros
    big = 3e38 if dtype != "fp16" else 65504.0
    x[3, ::7] = N.to_dtype(np.array([big], np.float32), dtype)[0]                 # squares that overflow (fp16: they do not, 65504^2 < 2^128)
    tiny = {"fp32": 1e-40, "bf16": 1e-40, "fp16": 6e-8}[dtype]                    # subnormal in x's type
    x[4] = N.to_dtype(np.full(h, tiny, np.float32), dtype) * np.where(np.arange(h) % 2, -1, 1).astype(np.float32)
    assert (x[4] != 0).all() and (np.abs(x[4]) < {"fp32": 2.0 ** -126, "bf16": 2.0 ** -126, "fp16": 2.0 ** -14}[dtype]).all()
    got = _check_forward(dga, oracle, x, None, w, dtype, False, False, f"specials [{dtype}]", eps=1.0,
                         overflow_rows=(3,) if dtype != "fp16" else ())
    rstd = got["rstd"].view(np.float32)
    assert (got["q"][1] == 0).all() and (got["sf"].view(np.float32)[1] == 1.0).all() and (got["norm"][1] == 0).all()   # +0 codes, scale 1
    if dtype != "fp16":
        assert rstd[3] == 0.0 and ((got["q"][3] & 0x7F) == 0).all()               # rstd = 0, y = +-0
    y4 = N.from_bits(got["norm"][4], dtype)
    if dtype == "fp32":
        assert (y4 != 0).all() and (np.abs(y4) < 2.0 ** -126).all()               # subnormal in, subnormal out: nothing was flushed
    # eps = 1e-6 on the row of zeros: rstd = fl32(eps)^(-1/2) inside the bound (checked in there), 1000 to a few units
    got = _check_forward(dga, oracle, x[:2], None, w, dtype, False, True, f"zeros [{dtype}]")
    assert abs(got["rstd"].view(np.float32)[1] - 1000.0) < 0.01 and (got["q"][1] == 0).all()


# ---------------------------------------------------------------------------------------------------------------- the backward

def _backward(dga, gy, z, w, rstd, dtype, w_f32, dx_dtype, gr=None, alias=False, need_dweight=True):
    """-> (dx bits, dweight bits or None) from pre-filled outputs; alias: dx is grad_residual's own tensor."""
    t_n, h = z.shape
    d_gr = None if gr is None else _dev(gr, dx_dtype)
    dx = d_gr if alias else _sentinels(dx_dtype, t_n, h)
    dw = _sentinels("fp32", h) if need_dweight else None
    got = dga.rms_norm_backward(_dev(gy, dtype), _dev(z, dtype), _dev(w, "fp32" if w_f32 else dtype), _dev(rstd), grad_residual=d_gr,
                                out=(dx, dw), need_dweight=need_dweight, sync=True)
    assert got[0] is dx and got[1] is dw
    return N.bits_of(dx), None if dw is None else N.bits_of(dw)


def test_the_longest_case_spans_three_chunks_with_a_ragged_last_one(dga):
    t_n = max(t for t, _ in N.BACKWARD_TH)
    for h in (7, 7168):
        chunks, rest = divmod(dga.rms_norm_backward_workspace_bytes(t_n, h), 4 * h)
        assert rest == 0 and chunks >= 3 and chunks == -(-t_n // N.chunk_rows(t_n)) and t_n % N.chunk_rows(t_n) != 0


@pytest.mark.parametrize("dtype", N.DTYPES)
@pytest.mark.parametrize("t_n,h", N.BACKWARD_TH)
def test_backward_cases(dga, t_n, h, dtype):
    w_f32 = (t_n + h) % 2 == 1
    where = f"[{t_n},{h},{dtype},w_f32={w_f32}]"
    gy, z, w, rstd = N.backward_inputs(t_n, h, dtype, w_f32)
    dx_bits, dw_bits = _backward(dga, gy, z, w, rstd, dtype, w_f32, "fp32")
    assert (dx_bits != R.SENTINEL_F32).all() and (dw_bits != R.SENTINEL_F32).all(), where
    dx, dw = dx_bits.view(np.float32), dw_bits.view(np.float32)
    ref_dx, ref_dw, m = N.backward64(gy, z, w, rstd)
    err, bar = np.abs(dx.astype(np.float64) - ref_dx), N.dx_bar(m, h)
    werr, wbar = np.abs(dw.astype(np.float64) - ref_dw), N.dweight_bar(m, t_n)
    worst = float((err[bar > 0] / bar[bar > 0]).max())
    worst_w = float((werr[wbar > 0] / wbar[wbar > 0]).max())
    print(f"{where} dx: worst error = {worst:.3f} of the bound; dweight: {worst_w:.3f} of the bound")
    assert (err <= bar).all() and (werr <= wbar).all(), (where, worst, worst_w)
    again = _backward(dga, gy, z, w, rstd, dtype, w_f32, "fp32")
    assert np.array_equal(again[0], dx_bits) and np.array_equal(again[1], dw_bits), where            # two runs, the same bits
    alone = _backward(dga, gy, z, w, rstd, dtype, w_f32, "fp32", need_dweight=False)
    assert alone[1] is None and np.array_equal(alone[0], dx_bits), where
    # the 16-bit dx is the RNE of the float32 one; dweight does not depend on dx's type
    if dtype != "fp32":
        d16, w16 = _backward(dga, gy, z, w, rstd, dtype, w_f32, dtype)
        assert np.array_equal(d16, R.round_to(dx, dtype)) and np.array_equal(w16, dw_bits), where
    # grad_residual: RNE(fl32(dx + grad_residual)) in dx's type, into another tensor and into grad_residual itself
    rng = np.random.default_rng([21, t_n, h])
    for dx_dtype in {"fp32", dtype}:
        gr = N.to_dtype(rng.standard_normal((t_n, h)) * (np.abs(dx).max() + 1e-3), dx_dtype)
        want = R.round_to(np.add(dx, gr, dtype=np.float32), dx_dtype)
        for alias in (False, True):
            summed, w_again = _backward(dga, gy, z, w, rstd, dtype, w_f32, dx_dtype, gr=gr, alias=alias)
            assert np.array_equal(summed, want) and np.array_equal(w_again, dw_bits), (where, dx_dtype, alias)


def test_a_rows_dx_does_not_depend_on_where_it_sits(dga):
    gy, z, w, rstd = N.backward_inputs(300, 2048, "bf16", False, seed=2)
    for r in (0, 299):
        gy[r], z[r], rstd[r] = gy[150], z[150], rstd[150]
    big, _ = _backward(dga, gy, z, w, rstd, "bf16", False, "fp32")
    one, _ = _backward(dga, gy[150:151], z[150:151], w, rstd[150:151], "bf16", False, "fp32")
    for r in (0, 150, 299):
        assert np.array_equal(big[r], one[0]), r
