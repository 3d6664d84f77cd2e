"""GPU: one whole training step of a MoE expert MLP through the public entries, every tensor handed from the entry that produces it to the
entry that consumes it, in the contiguous and in the masked layout, against the float64 reference of tests/moe_mlp_ref.py.

  F1  per_token_cast_to_fp8_transposed(X, mask, rowwise=True)                         (X^T q, sX^T), (Xq, sX)
  F2  grouped GEMM (Xq, sX) x W1q                                                      Y1 bf16 [.., 2H]
  F3  silu_and_mul_per_token_cast_to_fp8_transposed(Y1, mask, rowwise=True)            (h^T q, sh^T), (hq, sh)
  F4  grouped GEMM (hq, sh) x W2q                                                      Out bf16 [.., D]
  B1  per_token_cast_to_fp8_transposed(dOut, mask, rowwise=True)                       (dO^T q, ..), (dOq, ..)
  B2  grouped GEMM dOq x (W2^T)q                                                       grad_h bf16 [.., H]
  B3  silu_and_mul_backward_per_token_cast_to_fp8(Y1, grad_h, mask, grad_x_out=dY1)    (dq, dsf), dY1 bf16
  B4  grouped GEMM (dq, dsf) x (W1^T)q                                                 dX bf16 [.., D]
  B5  k_grouped_wgrad_gemm_fp8_fp8_fp32_nt(dO^T, h^T, ks)                              dW2 [G, D, H] fp32
  B6  per_token_cast_to_fp8_transposed(dY1, mask), k_grouped_wgrad(dY1^T, X^T, ks)     dW1 [G, 2H, D] fp32

D = 384, H = 256, G = 4 experts with [200, 0, 77, 1] tokens.  Contiguous: segments padded to 128 rows, ks = [256, 0, 128, 128], 128 trailing
padding rows, T = 640, m_indices -1 on padding.  Masked: Mmax = 256, masked_m = the tokens, ks = [256] * 4.  Every buffer a mask applies to
is made here and passed through out= / grad_x_out=: the excluded rows of X and dOut and of every bf16 buffer hold NaN (0x7FC1), those of the
quantised outputs 0xA5 bytes and 0x7FC0A5A5 scales.  Every bar is the one the entry's own test uses."""
import numpy as np
import pytest
import torch

import moe_mlp_ref as R
from fused_bounds import EPS, _reference

pytestmark = pytest.mark.gpu

SENTINEL_Q, SENTINEL_SF, NAN16 = 0xA5, 0x7FC0A5A5, 0x7FC1
D, H, G = R.D, R.H, R.G
BF16 = ("y1", "out", "grad_h", "dy1", "dx")
ROWWISE = (("x", D), ("h", H), ("do", D), ("d", 2 * H))                  # (q, sf) pairs with the width of q
TRANSPOSED = (("xt", D), ("ht", H), ("dot", D), ("dy1t", 2 * H))
WHOLE = {"dw1", "dw2"} | {n + s for n, _ in TRANSPOSED for s in ("_q", "_sf")}      # tensors without a token-row axis in front


class Layout:
    """Where the tokens of a case sit.  lead: the leading dimensions of every token buffer; rows[g]: the flat rows of expert g's tokens;
    k0[g], ks[g]: expert g's slice of the token axis of the transposed operands; mask(): the keyword the quantisers take."""

    def __init__(self, name, tokens):
        self.name, self.tokens = name, tuple(tokens)
        if name == "contiguous":
            self.ks = [(t + 127) // 128 * 128 for t in tokens]
            self.k0 = [int(v) for v in np.cumsum([0] + self.ks[:-1])]
            self.lead = (sum(self.ks) + 128,)
            self.counts = np.full(self.lead, -1, np.int32)                 # m_indices
            for g, t in enumerate(tokens):
                self.counts[self.k0[g]:self.k0[g] + t] = g
        else:
            self.ks = [R.MMAX] * len(tokens)
            self.k0 = [g * R.MMAX for g in range(len(tokens))]
            self.lead = (len(tokens), R.MMAX)
            self.counts = np.array(tokens, np.int32)                       # masked_m
        self.t_n = int(np.prod(self.lead))
        self.rows = [self.k0[g] + np.arange(t) for g, t in enumerate(tokens)]
        self.valid = np.zeros(self.t_n, bool)
        self.valid[np.concatenate(self.rows)] = True

    def mask(self, counts):
        return {"m_indices": counts} if self.name == "contiguous" else {"masked_m": counts}

    def scatter(self, per_expert, width):
        """bf16 [lead, width] on the host: the experts' rows where they belong, NaN (0x7FC1) everywhere else."""
        buf = torch.full((self.t_n, width), NAN16, dtype=torch.int16).view(torch.bfloat16)
        for rows, v in zip(self.rows, per_expert):
            buf[torch.from_numpy(rows)] = torch.from_numpy(v).to(torch.bfloat16)
        return buf.view(self.lead + (width,))


def _inputs(dga, lay, case, weights=None):
    """The device tensors of a case in a layout; the four quantised weights are made once per case (per_block_cast_to_fp8 per expert)."""
    inp = {"x": lay.scatter(case["X"], D).cuda(), "dout": lay.scatter(case["dOut"], D).cuda(), "counts": torch.from_numpy(lay.counts).cuda()}
    if weights is None:
        weights = {}
        for name, key, tr in (("w1", "W1", False), ("w2", "W2", False), ("w1t", "W1", True), ("w2t", "W2", True)):
            pairs = [dga.per_block_cast_to_fp8(torch.from_numpy(np.ascontiguousarray(w.T if tr else w, np.float32)).cuda()) for w in case[key]]
            weights[name] = (torch.stack([q.view(torch.uint8) for q, _ in pairs]), torch.stack([sf for _, sf in pairs]))
    inp.update(weights)
    return inp


def _buffers(lay):
    """Every output of the step, pre-filled: NaN in the bf16 and fp32 tensors, the two sentinels in codes and scales."""
    b = {}
    for name, width in zip(BF16, (2 * H, D, H, 2 * H, D)):
        b[name] = torch.full(lay.lead + (width,), NAN16, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    for name, width in ROWWISE:
        b[name + "_q"] = torch.full(lay.lead + (width,), SENTINEL_Q, dtype=torch.uint8, device="cuda")
        b[name + "_sf"] = torch.full(lay.lead + (width // 128,), SENTINEL_SF, dtype=torch.int32, device="cuda").view(torch.float32)
    for name, width in TRANSPOSED:
        b[name + "_q"] = torch.full((width, lay.t_n), SENTINEL_Q, dtype=torch.uint8, device="cuda")
        b[name + "_sf"] = torch.full((width, lay.t_n // 128), SENTINEL_SF, dtype=torch.int32, device="cuda").view(torch.float32)
    b["dw2"] = torch.full((G, D, H), float("nan"), dtype=torch.float32, device="cuda")
    b["dw1"] = torch.full((G, 2 * H, D), float("nan"), dtype=torch.float32, device="cuda")
    return b


def _step(dga, lay, inp, b, strict=False, c=None, ks_tensor=None):
    """F1 .. B6 on the current stream, public entries only.  c = (c1, c2): the addends of dW1 and dW2."""
    mask = lay.mask(inp["counts"])

    def gemm(lhs, rhs, out):
        if lay.name == "contiguous":
            dga.m_grouped_gemm_fp8_fp8_bf16_nt_contiguous(lhs, rhs, out, inp["counts"], strict=strict)
        else:
            dga.m_grouped_gemm_fp8_fp8_bf16_nt_masked(lhs, rhs, out, inp["counts"], R.MMAX, strict=strict)

    pair = lambda n: (b[n + "_q"], b[n + "_sf"])
    dga.per_token_cast_to_fp8_transposed(inp["x"], rowwise=True, out=(pair("xt"), pair("x")), **mask)                       # F1
    gemm(pair("x"), inp["w1"], b["y1"])                                                                                     # F2
    dga.silu_and_mul_per_token_cast_to_fp8_transposed(b["y1"], rowwise=True, out=(pair("ht"), pair("h")), **mask)           # F3
    gemm(pair("h"), inp["w2"], b["out"])                                                                                    # F4
    dga.per_token_cast_to_fp8_transposed(inp["dout"], rowwise=True, out=(pair("dot"), pair("do")), **mask)                  # B1
    gemm(pair("do"), inp["w2t"], b["grad_h"])                                                                               # B2
    dga.silu_and_mul_backward_per_token_cast_to_fp8(b["y1"], b["grad_h"], out=pair("d"), grad_x_out=b["dy1"], **mask)       # B3
    gemm(pair("d"), inp["w1t"], b["dx"])                                                                                    # B4
    c1, c2 = c if c is not None else (None, None)
    dga.k_grouped_wgrad_gemm_fp8_fp8_fp32_nt(pair("dot"), pair("ht"), b["dw2"], lay.ks, ks_tensor=ks_tensor, c=c2, strict=strict)    # B5
    dga.per_token_cast_to_fp8_transposed(b["dy1"], out=pair("dy1t"), **mask)                                                # B6
    dga.k_grouped_wgrad_gemm_fp8_fp8_fp32_nt(pair("dy1t"), pair("xt"), b["dw1"], lay.ks, ks_tensor=ks_tensor, c=c1, strict=strict)


def _host(tensors):
    """Device tensors -> numpy with the token dimensions flattened: bf16 as uint16 bits, codes as uint8, the rest as it is."""
    out = {}
    for k, t in tensors.items():
        if isinstance(t, tuple):
            out[k] = tuple(v.cpu().numpy() for v in t)
        elif t.dtype == torch.bfloat16:
            out[k] = t.view(torch.int16).cpu().numpy().view(np.uint16).reshape(-1, t.shape[-1])
        elif k in WHOLE or t.dim() == 1:
            out[k] = t.cpu().numpy()
        else:
            out[k] = t.cpu().numpy().reshape(-1, t.shape[-1])
    return out


_RUNS = {}


def _run(dga, name, strict):
    """The step on seed 0 in layout `name`, once per process: (layout, case, device inputs, device buffers, both on the host)."""
    if (name, strict) not in _RUNS:
        case = R.make_case(0)
        lay = Layout(name, case["tokens"])
        inp = _inputs(dga, lay, case)
        b = _buffers(lay)
        _step(dga, lay, inp, b, strict=strict)
        torch.cuda.synchronize()
        _RUNS[name, strict] = (lay, case, inp, b, _host(inp), _host(b))
    return _RUNS[name, strict]


LAYOUTS = pytest.mark.parametrize("name", ["contiguous", "masked"])


# ---- a. every link is right on what it was actually given

def _same(gq, gsf, wq, wsf, what):
    gsf, wsf = np.ascontiguousarray(gsf, np.float32), np.ascontiguousarray(wsf, np.float32)
    assert gsf.shape == wsf.shape and gq.shape == wq.shape, (what, gsf.shape, wsf.shape, gq.shape, wq.shape)
    sbad = np.nonzero(gsf.view(np.uint32) != wsf.view(np.uint32))
    assert sbad[0].size == 0, f"{what}: {sbad[0].size} scales differ, first at {[int(i[0]) for i in sbad]}: " \
                              f"{gsf.view(np.uint32)[sbad][0]:#x} vs {wsf.view(np.uint32)[sbad][0]:#x}"
    bad = np.nonzero(gq != wq)
    assert bad[0].size == 0, f"{what}: {bad[0].size} of {gq.size} codes differ, first at {[int(i[0]) for i in bad]}: " \
                             f"{gq[bad][0]:#x} vs {wq[bad][0]:#x}"


def _f32(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


def _check_fused(oracle, what, gq, gsf, ref, bound, cap, counted):
    """The tolerance family on real GEMM output.  gq, gsf: the device's codes and 1x128 scales; ref, bound: the float64 value and the entry's
    documented element bound.  Scale bits equal the oracle's on fl32(ref); every code decodes into [RNE((ref - bound) / s), RNE((ref + bound)
    / s)]; the share of the `counted` elements (bool, the valid tokens) whose code is not the oracle's on fl32(ref) -- excused because the
    value is within its bound of a rounding boundary -- is at most cap."""
    wq, wsf = oracle.quant_1x128(ref.astype(np.float32))
    sbad = int((gsf.view(np.uint32) != wsf.view(np.uint32)).sum())
    assert sbad == 0, f"{what}: {sbad} of {gsf.size} scales differ from the float64 reference's"
    scale = np.repeat(gsf.astype(np.float64), 128, axis=1)
    lo, hi = R.code_interval(oracle, ref, bound, scale)
    dec = oracle.e4m3fn_table()[gq].astype(np.float64)
    outside = (dec < lo) | (dec > hi) | np.isnan(dec)
    excused = (gq != wq) & ~outside & counted
    share = excused.sum() / max(1, int(counted.sum()))
    print(f"[{what}] {int(outside.sum())} of {dec.size} codes outside their interval; {int(excused.sum())} excused near a boundary: share "
          f"{share:.3e} (cap {cap:.3e}; {int(((lo != hi) & counted).sum())} elements have two admissible codes)")
    assert not outside.any(), f"{what}: {int(outside.sum())} codes outside the element bound"
    assert not (gq != wq)[~counted].any(), f"{what}: an excluded token's code is not 0"
    assert share <= cap, f"{what}: {share:.3e} of the codes excused, cap {cap:.3e}"


def _check_wgrad(oracle, what, lay, got, aq, asf, bq, bsf):
    """|d| <= 2^-22 S + 2^-24 |ref| per expert, against the float64 product of the dequantised slices (tests/test_k_grouped_wgrad_gpu.py)."""
    tab = oracle.e4m3fn_table()
    da, db = R.dequant_1x128(aq, asf, tab), R.dequant_1x128(bq, bsf, tab)
    for g in range(G):
        sl = slice(lay.k0[g], lay.k0[g] + lay.ks[g])
        ref, S = R.link_wgrad(da[:, sl], db[:, sl])
        excess = np.abs(got[g].astype(np.float64) - ref) - (2.0 ** -22 * S + 2.0 ** -24 * np.abs(ref))
        assert (excess <= 0).all(), f"{what} expert {g}: {int((excess > 0).sum())} outputs beyond the bar"


@LAYOUTS
def test_every_link_is_right_on_what_it_was_given(dga, oracle, name):
    """Default policy.  For each of F1 .. B6 the device bytes that went into the link, and the device output against the one-link float64
    reference on those bytes, under the bar of the entry's own test."""
    lay, case, inp, b, hin, hb = _run(dga, name, False)
    valid, mask = lay.valid, lay.mask(inp["counts"])
    lead2 = lambda t, w: t.reshape(lay.t_n, w)

    # the weights: per_block_cast_to_fp8 of W and of W^T is the oracle's 128x128 quantiser, per expert
    for wname, key, tr in (("w1", "W1", False), ("w2", "W2", False), ("w1t", "W1", True), ("w2t", "W2", True)):
        for g in range(G):
            wq, wsf = oracle.quant_128x128(np.ascontiguousarray(case[key][g].T if tr else case[key][g], np.float32))
            _same(hin[wname][0][g], hin[wname][1][g], wq, wsf, f"{wname}[{g}]")

    def plain_quantiser(link, src_bits, src_dev, pre, width):
        """F1 / B1 (/ B6 without the row-wise half): the definition's bytes and scale bits; row-wise also the stand-alone entry's."""
        x = _f32(src_bits)
        _same(hb[pre + "t_q"], hb[pre + "t_sf"], *R.link_quant_tokens(x, valid, oracle), f"{link} transposed")
        if pre + "_q" in hb:
            _same(hb[pre + "_q"][valid], hb[pre + "_sf"][valid], *R.link_quant_rows(x[valid], oracle), f"{link} row-wise")
            sq, ssf = dga.per_token_cast_to_fp8(lead2(src_dev, width))
            _same(hb[pre + "_q"][valid], hb[pre + "_sf"][valid], sq.view(torch.uint8).cpu().numpy()[valid], ssf.cpu().numpy()[valid],
                  f"{link} row-wise against per_token_cast_to_fp8")

    def gemm(link, lhs, rhs, out):
        """assert_parity against the oracle on the same bytes, per expert."""
        aq, asf, (wq, wsf), got = hb[lhs + "_q"], hb[lhs + "_sf"], hin[rhs], hb[out]
        for g, rows in enumerate(lay.rows):
            if rows.size:
                want = oracle.gemm_fp8_fp8_bf16_nt(aq[rows], asf[rows], wq[g], wsf[g], threads=4)
                oracle.assert_parity(got[rows], want, aq[rows], asf[rows], wq[g], wsf[g])
                assert not (got[rows] == NAN16).any(), f"{link}: a valid row of expert {g} was not written"

    plain_quantiser("F1", hin["x"], inp["x"], "x", D)
    gemm("F2", "x", "w1", "y1")

    # F3 on the bf16 that F2 wrote
    y1 = _f32(hb["y1"]).astype(np.float64)
    y1v = y1[valid]
    h_ref = R.act(y1v)
    _check_fused(oracle, "F3 row-wise", hb["h_q"][valid], hb["h_sf"][valid], h_ref, EPS * np.abs(h_ref), R.CAP_RELATIVE, np.ones(h_ref.shape, bool))
    h0 = np.zeros((lay.t_n, H)); h0[valid] = h_ref
    counted = np.broadcast_to(valid[None, :], (H, lay.t_n))
    _check_fused(oracle, "F3 transposed", hb["ht_q"], hb["ht_sf"], np.ascontiguousarray(h0.T), EPS * np.abs(h0.T), R.CAP_RELATIVE, counted)
    sq = torch.full_like(b["h_q"], SENTINEL_Q); ssf = torch.zeros_like(b["h_sf"])
    dga.silu_and_mul_per_token_cast_to_fp8(b["y1"], out=(sq, ssf), sync=True, **mask)
    _same(hb["h_q"][valid], hb["h_sf"][valid], lead2(sq, H).cpu().numpy()[valid], lead2(ssf, H // 128).cpu().numpy()[valid],
          "F3 row-wise against silu_and_mul_per_token_cast_to_fp8")
    gemm("F4", "h", "w2", "out")

    plain_quantiser("B1", hin["dout"], inp["dout"], "do", D)
    gemm("B2", "do", "w2t", "grad_h")

    # B3 on the bf16 that F2 and B2 wrote
    t64 = lambda v: torch.from_numpy(np.ascontiguousarray(v))
    grad_h = _f32(hb["grad_h"]).astype(np.float64)[valid]
    ref, bound = _reference(t64(y1v[:, :H]), t64(y1v[:, H:]), t64(grad_h))
    assert np.array_equal(ref, R.act_bwd(y1v, grad_h))
    gq, gsf = hb["d_q"][valid], hb["d_sf"][valid]
    nb = H // 128
    every = np.ones((ref.shape[0], H), bool)
    scale_gate = np.repeat(oracle.quant_1x128(ref[:, :H].astype(np.float32))[1].astype(np.float64), 128, axis=1)    # the reference's own
    cap_gate = R.dgate_cap(ref[:, :H], bound[:, :H], scale_gate)
    assert cap_gate <= 2.0 ** -6                       # (the derivation's estimate is 8 x about 2^-10; a cap far above that would bound nothing)
    _check_fused(oracle, "B3 dgate", gq[:, :H], gsf[:, :nb], ref[:, :H], bound[:, :H], cap_gate, every)
    _check_fused(oracle, "B3 dup", gq[:, H:], gsf[:, nb:], ref[:, H:], bound[:, H:], R.CAP_RELATIVE, every)
    # grad_x_out: the RNE of an fp32 value within the bound of the reference (RNE is monotone)
    dy1 = _f32(hb["dy1"]).astype(np.float64)[valid]
    r0, r1 = R.bf16_rne(ref - bound), R.bf16_rne(ref + bound)
    assert ((dy1 >= np.minimum(r0, r1)) & (dy1 <= np.maximum(r0, r1))).all(), "grad_x_out is not the RNE of a value within the element bound"
    print(f"[B3 grad_x_out] {(dy1 != R.bf16_rne(ref)).mean():.3e} of the elements differ from the RNE of the float64 reference")
    gemm("B4", "d", "w1t", "dx")

    _check_wgrad(oracle, "B5", lay, hb["dw2"], hb["dot_q"], hb["dot_sf"], hb["ht_q"], hb["ht_sf"])
    plain_quantiser("B6", hb["dy1"], b["dy1"], "dy1", 2 * H)
    _check_wgrad(oracle, "B6", lay, hb["dw1"], hb["dy1t_q"], hb["dy1t_sf"], hb["xt_q"], hb["xt_sf"])


# ---- b. nothing leaks and nothing is written that should not be

def _assert_sentinels(lay, hb, what):
    rest = ~lay.valid
    for k in BF16:
        assert (hb[k][rest] == NAN16).all(), f"{what}: an excluded row of {k} was written"
    for k, _ in ROWWISE:
        assert (hb[k + "_q"][rest] == SENTINEL_Q).all(), f"{what}: an excluded row of {k}_q was written"
        assert (hb[k + "_sf"][rest].view(np.uint32) == SENTINEL_SF).all(), f"{what}: an excluded row of {k}_sf was written"
    for k, _ in TRANSPOSED:
        assert (hb[k + "_sf"].view(np.uint32) != SENTINEL_SF).all(), f"{what}: a scale of {k}_sf was not written"
        assert not hb[k + "_q"][:, rest].any(), f"{what}: an excluded token of {k}_q is not code 0"


@LAYOUTS
def test_nothing_leaks_and_nothing_else_is_written(dga, oracle, name):
    lay, case, inp, b, hin, hb = _run(dga, name, False)
    assert np.isnan(_f32(hin["x"])[~lay.valid]).all() and np.isnan(_f32(hin["dout"])[~lay.valid]).all()      # the poison was there
    _assert_sentinels(lay, hb, name)
    empty, one = case["tokens"].index(0), case["tokens"].index(1)
    for k in ("dw1", "dw2"):
        assert np.isfinite(hb[k]).all(), f"{k} is not finite"
        assert not hb[k][empty].any(), f"the empty expert's {k} is not zero"
        assert hb[k][one].any(), f"the one-token expert's {k} is zero"
    # with c=: the empty expert's gradient is c[g] bit for bit, every other one fl32(plain + c[g]) (tests/test_k_grouped_wgrad_gpu.py)
    rng = np.random.default_rng(3)
    c_np = [rng.standard_normal(hb[k].shape).astype(np.float32) for k in ("dw1", "dw2")]
    if lay.ks[empty] == 0:
        c_np[0][empty, 0, :4] = -0.0     # (ks[g] = 0 copies c[g]; the masked layout adds its 256 zero tokens to it, and +0 + -0 is +0)
    c = tuple(torch.from_numpy(v).cuda() for v in c_np)
    b2 = _buffers(lay)
    _step(dga, lay, inp, b2, c=c)
    torch.cuda.synchronize()
    hb2 = _host(b2)
    _assert_sentinels(lay, hb2, name + " with c")
    for k, cc in zip(("dw1", "dw2"), c_np):
        for g in range(G):
            want = cc[g] if g == empty else (hb[k][g] + cc[g]).astype(np.float32)
            assert np.array_equal(hb2[k][g].view(np.uint32), want.view(np.uint32)), f"{k}[{g}] with c"


# ---- c. the two layouts are the same computation

def test_the_two_layouts_are_the_same_computation(dga, oracle):
    """strict=True on every GEMM: each is the oracle's fp32 chain in ascending k, and every quantiser works per row or per 128-token block
    of one expert, so the masked and the contiguous step on the same tokens agree bit for bit on every valid row of every token buffer
    (the row-wise codes and scales included) and on each expert's slice of the transposed operands; dW1 and dW2 agree numerically with
    equal NaN positions (an expert of at most 128 tokens has a trailing all-zero block in the masked layout only, which may turn -0
    into +0)."""
    lc, _, _, _, _, hc = _run(dga, "contiguous", True)
    lm, _, _, _, _, hm = _run(dga, "masked", True)
    for g in range(G):
        rc, rm = lc.rows[g], lm.rows[g]
        for k in BF16 + tuple(n + s for n, _ in ROWWISE for s in ("_q", "_sf")):
            a, bb = hc[k][rc], hm[k][rm]
            if a.dtype == np.float32:
                a, bb = a.view(np.uint32), bb.view(np.uint32)
            assert np.array_equal(a, bb), f"{k}: expert {g} differs between the layouts"
        for k, _ in TRANSPOSED:
            n = lc.ks[g]
            assert np.array_equal(hc[k + "_q"][:, lc.k0[g]:lc.k0[g] + n], hm[k + "_q"][:, lm.k0[g]:lm.k0[g] + n]), f"{k}_q expert {g}"
            assert not hm[k + "_q"][:, lm.k0[g] + n:lm.k0[g] + lm.ks[g]].any(), f"{k}_q expert {g}: the masked layout's empty blocks"
            sc, sm = hc[k + "_sf"][:, lc.k0[g] // 128:(lc.k0[g] + n) // 128], hm[k + "_sf"][:, lm.k0[g] // 128:(lm.k0[g] + n) // 128]
            assert np.array_equal(sc.view(np.uint32), sm.view(np.uint32)), f"{k}_sf expert {g}"
    for k in ("dw1", "dw2"):
        assert np.array_equal(np.isnan(hc[k]), np.isnan(hm[k])) and not np.isnan(hc[k]).any(), k
        assert np.array_equal(hc[k], hm[k]), f"{k} differs between the layouts"
        assert hc[k][0].any()


# ---- d. the step as a whole still trains

def test_the_step_as_a_whole_still_trains(dga, oracle):
    """Relative Frobenius error of Out, dX, dW1 and dW2 against step_exact, for the device step (default policy, contiguous layout, seed 0)
    and for step_emulated on seeds 0 .. 7.  The device differs from the emulation by accumulation order (<= 2^-22 S) and the 2^-18
    activation bound, both far below e4m3 quantisation noise, so its error may exceed the emulation's only by the emulation's own
    seed-to-seed spread: at most the largest of the eight (moe_mlp_ref.ERROR_SEEDS says why seed 0 must not be that largest one, and
    tests/test_moe_mlp_ref.py holds the recipe to it).  No number is written down here; the lines printed are what
    profiles/moe_mlp_step_error.txt holds."""
    lay, case, _, _, _, hb = _run(dga, "contiguous", False)
    dev = {k: [_f32(hb[n][rows]).astype(np.float64) for rows in lay.rows] for k, n in (("Out", "out"), ("dX", "dx"))}
    dev["dW1"], dev["dW2"] = hb["dw1"].astype(np.float64), hb["dw2"].astype(np.float64)
    exact = R.step_exact(case)
    got = [R.rel_error(dev[k], exact[k]) for k in R.ERROR_KEYS]
    emu = [R.emulated_errors(oracle, seed) for seed in R.ERROR_SEEDS]
    print("moe_mlp_step_error: relative Frobenius error against the float64 step" + " " * 11 + "".join(f"{k:>12}" for k in R.ERROR_KEYS))
    for seed, e in zip(R.ERROR_SEEDS, emu):
        print(f"moe_mlp_step_error: emulation seed {seed}" + " " * 43 + "".join(f"{v:12.7f}" for v in e))
    print("moe_mlp_step_error: device, seed 0 (default policy, contiguous layout)" + " " * 9 + "".join(f"{v:12.7f}" for v in got))
    for j, k in enumerate(R.ERROR_KEYS):
        worst = max(e[j] for e in emu)
        assert got[j] <= worst, f"{k}: device error {got[j]:.7f} above the largest emulated error {worst:.7f}"


# ---- e. one captured graph for the whole step

def test_one_captured_graph_for_the_whole_step_follows_masked_m(dga, oracle):
    """Masked layout, default policy.  Eager once, then F1 .. B6 captured on a side stream as one single-stream graph with ks_tensor on the
    device for both k-grouped calls.  masked_m is rewritten to [1, 256, 0, 130] (and X and dOut to tokens for those counts, NaN elsewhere)
    and the graph replayed: every output equals the eager step under the new counts bit for bit on the valid rows and in the transposed
    operands and weight gradients, and holds its sentinel everywhere else."""
    case = R.make_case(0)
    lay = Layout("masked", case["tokens"])
    inp = _inputs(dga, lay, case)
    weights = {k: inp[k] for k in ("w1", "w2", "w1t", "w2t")}
    ks_t = torch.tensor(lay.ks, dtype=torch.int32, device="cuda")
    static, fresh = _buffers(lay), _buffers(lay)
    _step(dga, lay, inp, static, ks_tensor=ks_t); torch.cuda.synchronize()       # eager once: the library is loaded and every workspace exists
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        _step(dga, lay, inp, static, ks_tensor=ks_t)                              # ... and the capture stream's own
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        _step(dga, lay, inp, static, ks_tensor=ks_t)
    torch.cuda.synchronize()

    counts = (1, 256, 0, 130)
    case2 = R.make_case(11, tokens=counts)
    case2["W1"], case2["W2"] = case["W1"], case["W2"]
    lay2 = Layout("masked", counts)
    inp2 = _inputs(dga, lay2, case2, weights)
    for k in ("x", "dout", "counts"):
        inp[k].copy_(inp2[k])
    for k in static:
        static[k].copy_(fresh[k])
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    got = _host(static)
    eager = _buffers(lay2)
    _step(dga, lay2, inp2, eager); torch.cuda.synchronize()
    want = _host(eager)
    _assert_sentinels(lay2, got, "replay")
    bits = lambda a: a.view(np.uint32) if a.dtype == np.float32 else a
    for k in got:
        if k in WHOLE:
            assert np.array_equal(bits(got[k]), bits(want[k])), f"replay: {k} differs from the eager step under the new counts"
        else:
            assert np.array_equal(bits(got[k][lay2.valid]), bits(want[k][lay2.valid])), f"replay: {k} differs on the valid rows"
    assert np.isfinite(got["dw1"]).all() and got["dw1"][0].any() and got["dw1"][1].any() and not got["dw1"][2].any() and got["dw2"][3].any()
