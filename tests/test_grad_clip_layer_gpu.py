"""GPU: the gradient norm, the clip coefficient and the skip decision between the weight gradient and the optimizer, with nothing decided
on the host.  The geometry of tests/test_adamw_cast_layer_gpu.py, G = 4 experts, W [G, N = 256, K = 384], 128 tokens per expert:
  k_grouped_wgrad_gemm_fp8_fp8_fp32_nt(dY^T, X^T, ks)                                        dW [G, N, K] fp32
  clip_grad_norm_step_scalars([dW, gamma_grad bf16 [384]], step_scalars, MAX_NORM, 1 / TOK)  sumsq, norm, coef, skip; step_scalars[3]
  adamw_per_block_cast_to_fp8_transposed(W, m, v, dW, step_scalars, rowwise=True, skip=skip) W, m, v in place; (qt, sft), (q, sf)
  m_grouped_gemm_fp8_fp8_bf16_nt_contiguous(X, (q, sf)), (dY', (qt, sft))                    the next forward and dgrad
eagerly once, then as one captured graph replayed four times after refilling inputs only: (a) a small dY, norm < MAX_NORM; (b) dY eight
times as large, norm > MAX_NORM; (c) one NaN in the dY the weight gradient reads: the step is skipped; (d) finite again.  dY' is the dY of
the step the two GEMMs belong to, the next one: it stays finite at (c), so what those GEMMs write shows whether the weights' codes are sound.

MAX_NORM: with the tokens of _tokens() the norms of the unscaled gradients, computed on the host in float64 from the bf16 tokens without
the fp8 quantisation (which moves a norm by a few per cent at most), are 55.2 .. 55.6 at scale 1 and 443.8 at scale 8.  150 lies a factor
2.7 above the first and 2.9 below the second."""
import numpy as np
import pytest
import torch

import adamw_ref as A
import grad_clip_ref as R

pytestmark = pytest.mark.gpu

G, N, K, TOK = 4, 256, 384, 128
T = G * TOK
PRE_SCALE = 1.0 / TOK
MAX_NORM, CLIP_EPS = 150.0, 1e-6
HYPER = dict(beta1=A.BETA1, beta2=A.BETA2, eps=A.EPS, weight_decay=A.WD)


def _bytes(t):
    return t.contiguous().view(torch.uint8).cpu().numpy()


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _tokens(number, scale):
    rng = np.random.default_rng([50, number])
    return R.bf16(rng.standard_normal((T, K))), R.bf16(rng.standard_normal((T, N)) * scale)


def _same(got, want):
    return bool(np.isnan(got)) if np.isnan(want) else int(_u32([got])[0]) == int(_u32([want])[0])


@pytest.mark.parametrize("moment", A.DTYPES, ids=["m32", "m16"])
def test_clip_and_skip_inside_one_captured_step(dga, oracle, moment):
    dt = {"fp32": torch.float32, "bf16": torch.bfloat16}[moment]
    rng = np.random.default_rng(7)
    w0 = (rng.standard_normal((G, N, K)) * (2.0 / np.sqrt(K))).astype(np.float32)
    gamma_grad = R.bf16(np.random.default_rng(51).standard_normal(384))
    host = {"w": w0, "m": np.zeros_like(w0), "v": np.zeros_like(w0)}
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8, device="cuda")
    f32 = lambda *s: torch.zeros(s, device="cuda")
    d = {"w": torch.from_numpy(w0.copy()).cuda(), "m": torch.zeros((G, N, K), dtype=dt, device="cuda"),
         "v": torch.zeros((G, N, K), dtype=dt, device="cuda"), "sc": f32(4), "dw": f32(G, N, K),
         "gamma": torch.from_numpy(gamma_grad).bfloat16().cuda(), "y": torch.zeros((T, N), dtype=torch.bfloat16, device="cuda"),
         "dx": torch.zeros((T, K), dtype=torch.bfloat16, device="cuda")}
    clip = (f32(1), f32(1), torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.float64, device="cuda"))
    out = ((u8(G, K, N), f32(G, K // 128, N // 128)), (u8(G, N, K), f32(G, N // 128, K // 128)))
    tok = {"xt": (u8(K, T), f32(K, T // 128)), "x": (u8(T, K), f32(T, K // 128)), "dyt": (u8(N, T), f32(N, T // 128)), "dy": (u8(T, N), f32(T, N // 128))}
    ks = [TOK] * G
    ks_t = torch.tensor(ks, dtype=torch.int32, device="cuda")
    m_idx = torch.arange(G, dtype=torch.int32, device="cuda").repeat_interleave(TOK).contiguous()

    def give(number, step_number, scale=1.0, poison=False):
        """The inputs of a replay: the tokens, quantised, and the step's {lr, bc1, bc2s} (element 3 is the device's to write)."""
        x, dy = _tokens(number, scale)
        tx, tdy = torch.from_numpy(x).bfloat16().cuda(), torch.from_numpy(dy).bfloat16().cuda()
        dga.per_token_cast_to_fp8_transposed(tx, rowwise=True, out=(tok["xt"], tok["x"]))
        dga.per_token_cast_to_fp8_transposed(tdy, rowwise=True, out=(tok["dyt"], tok["dy"]))
        if poison:                                            # the dY the weight gradient reads; the next dgrad's own dY stays as it is
            bad = tdy.clone()
            bad[TOK + 5, 77] = float("nan")
            dga.per_token_cast_to_fp8_transposed(bad, out=tok["dyt"])
        dga.adamw_step_scalars(step_number, A.LR, A.BETA1, A.BETA2, 123.0, out=d["sc"])
        torch.cuda.synchronize()

    def step():
        dga.k_grouped_wgrad_gemm_fp8_fp8_fp32_nt(tok["dyt"], tok["xt"], d["dw"], ks, ks_tensor=ks_t)
        dga.clip_grad_norm_step_scalars([d["dw"], d["gamma"]], d["sc"], MAX_NORM, pre_scale=PRE_SCALE, eps=CLIP_EPS, out=clip)
        dga.adamw_per_block_cast_to_fp8_transposed(d["w"], d["m"], d["v"], d["dw"], d["sc"], rowwise=True, out=out, skip=clip[2], **HYPER)
        dga.m_grouped_gemm_fp8_fp8_bf16_nt_contiguous(tok["x"], out[1], d["y"], m_idx)
        dga.m_grouped_gemm_fp8_fp8_bf16_nt_contiguous(tok["dy"], out[0], d["dx"], m_idx)

    def snapshot():
        return {name: _bytes(t) for name, t in (("w", d["w"]), ("m", d["m"]), ("v", d["v"]), ("qt", out[0][0]), ("sft", out[0][1]),
                                                ("q", out[1][0]), ("sf", out[1][1]))}

    def check(step_number, clipping, skipped=False):
        """Link by link on what the run wrote; advances the host's copy of the state unless the step was skipped."""
        dw = d["dw"].cpu().numpy()
        got_ss = float(clip[3].cpu().numpy()[0])
        sc = d["sc"].cpu().numpy()
        want_sc = A.scalars(step_number, A.LR, A.BETA1, A.BETA2, 123.0)
        assert np.array_equal(_u32(sc[:3]), _u32(want_sc[:3])), "step_scalars[0..2] were written"
        norm, coef, scale, skip = R.clip_scalars(got_ss, MAX_NORM, PRE_SCALE, CLIP_EPS)     # from the device's own sum, as the unit test does
        got = (clip[0].item(), clip[1].item(), float(sc[3]))
        print("step %d: sumsq %.17g norm %.9g coef %.9g grad_scale %.9g skip %d" % (step_number, got_ss, *got, clip[2].item()))
        assert clip[2].item() == skip == int(skipped)
        for name, g, w in zip(("norm", "coef", "grad_scale"), got, (norm, coef, scale)):
            assert _same(np.float32(g), w), (name, g, w)
        y, dx = d["y"].float().cpu().numpy(), d["dx"].float().cpu().numpy()
        assert np.isfinite(y).all() and np.isfinite(dx).all() and y.any() and dx.any()
        if skipped:
            assert not np.isfinite(dw).all() and not np.isfinite(got_ss) and got[1] == 0.0 and got[2] == 0.0
            return
        exact = R.sumsq([dw, gamma_grad])
        assert abs(got_ss - exact) <= R.bound(dw.size + gamma_grad.size, exact), (got_ss, exact)
        assert (got[1] < 1.0) == clipping and (got[0] > MAX_NORM) == clipping
        w2, m2, v2 = A.step(host["w"], host["m"], host["v"], dw, sc, *(A.f32(HYPER[x]) for x in ("beta1", "beta2", "eps", "weight_decay")))
        for name, want, kind in (("w", w2, "fp32"), ("m", m2, moment), ("v", v2, moment)):
            bits = d[name].view(torch.int32 if kind == "fp32" else torch.int16).cpu().numpy().view(np.uint32 if kind == "fp32" else np.uint16)
            bad = A.same_bits(bits, A.moment_bits(want, kind), want)
            assert bad[0].size == 0 and np.isfinite(want).all(), f"step {step_number}: {bad[0].size} elements of {name} differ from the reference"
        assert not np.array_equal(w2, host["w"])
        host.update(w=w2, m=A.stored(m2, moment), v=A.stored(v2, moment))
        (qt, sft), (q, sf) = ((_bytes(a), b.cpu().numpy()) for a, b in out)
        for g in range(G):
            for what, gq, gsf, src in (("q", q[g], sf[g], w2[g]), ("qt", qt[g], sft[g], w2[g].T)):
                wq, wsf = oracle.quant_128x128(np.ascontiguousarray(src, np.float32))
                assert np.array_equal(gq, wq) and np.array_equal(_u32(gsf), _u32(wsf)), f"step {step_number}: {what}[{g}] is not the oracle's"

    give(1, 1)
    step()
    torch.cuda.synchronize()
    check(1, clipping=False)

    saved = {name: d[name].clone() for name in ("w", "m", "v")}
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        step()                                            # the warm-up on the capture stream advances the state: it is put back below
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        step()
    torch.cuda.synchronize()
    for name, t in saved.items():
        d[name].copy_(t)

    def replay(number, step_number, **kw):
        give(number, step_number, **kw)
        for t in (d["dw"], d["y"], d["dx"]) + clip:
            t.zero_()
        clip[2].fill_(5)
        for q_, sf_ in out:
            q_.fill_(0xA5)
            sf_.view(torch.int32).fill_(0x7FC0A5A5)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()

    replay(2, 2)                                          # (a)
    check(2, clipping=False)
    replay(3, 3, scale=8.0)                               # (b)
    check(3, clipping=True)
    after_b = snapshot()
    replay(4, 4, poison=True)                             # (c): the caller does not advance the step number after it
    check(4, clipping=False, skipped=True)
    after_c = snapshot()
    for name in after_b:
        assert np.array_equal(after_b[name], after_c[name]), f"{name} differs after the skipped step"
    replay(5, 4)                                          # (d)
    check(4, clipping=False)
