"""GPU: the optimizer between the weight gradient of one step and the GEMMs of the next, G = 4 experts, W [G, N = 256, K = 384], 128 tokens
per expert in the contiguous layout:
  k_grouped_wgrad_gemm_fp8_fp8_fp32_nt(dY^T, X^T, ks)                                    dW [G, N, K] fp32
  adamw_per_block_cast_to_fp8_transposed(W, m, v, dW, step_scalars, rowwise=True)        W, m, v in place; (qt, sft), (q, sf)
  m_grouped_gemm_fp8_fp8_bf16_nt_contiguous(X, (q, sf))                                  the next forward, Y [T, N]
  m_grouped_gemm_fp8_fp8_bf16_nt_contiguous(dY, (qt, sft))                               the next dgrad, dX [T, K]
eagerly for step 1, then as one captured graph replayed for step 2 after new tokens and a new adamw_step_scalars(..., out=).  Every link
is checked on what the run itself produced, against the references of tests/test_moe_mlp_step_gpu.py: the weight gradient under its bar
against float64 on the dequantised operands, the optimizer bit for bit against tests/adamw_ref.py on the dW the GEMM wrote, the codes
against the oracle's 128x128 quantiser of the new W and of its transposes, and both GEMMs by assert_parity against the oracle."""
import numpy as np
import pytest
import torch

import adamw_ref as A
import moe_mlp_ref as R

pytestmark = pytest.mark.gpu

G, N, K, TOK = 4, 256, 384, 128
T = G * TOK
GRAD_SCALE = 1.0 / TOK
HYPER = dict(beta1=A.BETA1, beta2=A.BETA2, eps=A.EPS, weight_decay=A.WD)


def _bytes(t):
    return t.view(torch.uint8).cpu().numpy() if t.element_size() == 1 else t.view(torch.int32).cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("moment", A.DTYPES, ids=["m32", "m16"])
def test_the_optimizer_between_two_steps_eager_then_one_graph(dga, oracle, moment):
    dt = {"fp32": torch.float32, "bf16": torch.bfloat16}[moment]
    rng = np.random.default_rng(7)
    w0 = (rng.standard_normal((G, N, K)) * (2.0 / np.sqrt(K))).astype(np.float32)
    host = {"w": w0, "m": np.zeros_like(w0), "v": np.zeros_like(w0)}
    d = {"w": torch.from_numpy(w0.copy()).cuda(), "m": torch.zeros((G, N, K), dtype=dt, device="cuda"),
         "v": torch.zeros((G, N, K), dtype=dt, device="cuda"), "sc": torch.zeros(4, device="cuda"),
         "dw": torch.zeros((G, N, K), device="cuda"), "y": torch.zeros((T, N), dtype=torch.bfloat16, device="cuda"),
         "dx": torch.zeros((T, K), dtype=torch.bfloat16, device="cuda")}
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8, device="cuda")
    f32 = lambda *s: torch.zeros(s, device="cuda")
    out = ((u8(G, K, N), f32(G, K // 128, N // 128)), (u8(G, N, K), f32(G, N // 128, K // 128)))
    tok = {"xt": (u8(K, T), f32(K, T // 128)), "x": (u8(T, K), f32(T, K // 128)), "dyt": (u8(N, T), f32(N, T // 128)), "dy": (u8(T, N), f32(T, N // 128))}
    ks = [TOK] * G
    ks_t = torch.tensor(ks, dtype=torch.int32, device="cuda")
    m_idx = torch.arange(G, dtype=torch.int32, device="cuda").repeat_interleave(TOK).contiguous()
    rows = [np.arange(g * TOK, (g + 1) * TOK) for g in range(G)]

    def give(number):
        """The tokens of step `number`, quantised as the step test does, and its scalars."""
        gen = torch.Generator(device="cuda").manual_seed(40 + number)
        x = torch.randn((T, K), device="cuda", generator=gen).bfloat16()
        dy = torch.randn((T, N), device="cuda", generator=gen).bfloat16()
        dga.per_token_cast_to_fp8_transposed(x, rowwise=True, out=(tok["xt"], tok["x"]))
        dga.per_token_cast_to_fp8_transposed(dy, rowwise=True, out=(tok["dyt"], tok["dy"]))
        dga.adamw_step_scalars(number, A.LR, A.BETA1, A.BETA2, GRAD_SCALE, out=d["sc"])
        torch.cuda.synchronize()

    def step():
        dga.k_grouped_wgrad_gemm_fp8_fp8_fp32_nt(tok["dyt"], tok["xt"], d["dw"], ks, ks_tensor=ks_t)
        dga.adamw_per_block_cast_to_fp8_transposed(d["w"], d["m"], d["v"], d["dw"], d["sc"], rowwise=True, out=out, **HYPER)
        dga.m_grouped_gemm_fp8_fp8_bf16_nt_contiguous(tok["x"], out[1], d["y"], m_idx)
        dga.m_grouped_gemm_fp8_fp8_bf16_nt_contiguous(tok["dy"], out[0], d["dx"], m_idx)

    def check(number):
        """Link by link on what the run wrote; advances the host's copy of the state."""
        tab = oracle.e4m3fn_table()
        hb = {name: (_bytes(q), sf.cpu().numpy()) for name, (q, sf) in tok.items()}
        dw = d["dw"].cpu().numpy()
        da, db = R.dequant_1x128(*hb["dyt"], tab), R.dequant_1x128(*hb["xt"], tab)
        for g in range(G):
            ref, S = R.link_wgrad(da[:, rows[g]], db[:, rows[g]])
            excess = np.abs(dw[g].astype(np.float64) - ref) - (2.0 ** -22 * S + 2.0 ** -24 * np.abs(ref))
            assert (excess <= 0).all(), f"step {number}, dW of expert {g}: {int((excess > 0).sum())} outputs beyond the bar"
        sc = A.scalars(number, A.LR, A.BETA1, A.BETA2, GRAD_SCALE)
        assert np.array_equal(d["sc"].cpu().numpy().view(np.uint32), sc.view(np.uint32))
        w2, m2, v2 = A.step(host["w"], host["m"], host["v"], dw, sc, *(A.f32(HYPER[x]) for x in ("beta1", "beta2", "eps", "weight_decay")))
        for name, want, kind in (("w", w2, "fp32"), ("m", m2, moment), ("v", v2, moment)):
            got = d[name].view(torch.int32 if kind == "fp32" else torch.int16).cpu().numpy().view(np.uint32 if kind == "fp32" else np.uint16)
            bad = A.same_bits(got, A.moment_bits(want, kind), want)
            assert bad[0].size == 0 and np.isfinite(want).all(), f"step {number}: {bad[0].size} elements of {name} differ from the reference"
        host.update(w=w2, m=A.stored(m2, moment), v=A.stored(v2, moment))
        (qt, sft), (q, sf) = ((_bytes(a), b.cpu().numpy()) for a, b in out)
        for g in range(G):
            for what, gq, gsf, src in (("q", q[g], sf[g], w2[g]), ("qt", qt[g], sft[g], w2[g].T)):
                wq, wsf = oracle.quant_128x128(np.ascontiguousarray(src, np.float32))
                assert np.array_equal(gq, wq) and np.array_equal(gsf.view(np.uint32), np.ascontiguousarray(wsf, np.float32).view(np.uint32)), \
                    f"step {number}: {what}[{g}] is not the oracle's quantiser of the new weights"
        for link, lhs, (bq, bsf), res in (("fprop", "x", (q, sf), "y"), ("dgrad", "dy", (qt, sft), "dx")):
            aq, asf = hb[lhs]
            got = d[res].view(torch.int16).cpu().numpy().view(np.uint16)
            for g in range(G):
                want = oracle.gemm_fp8_fp8_bf16_nt(aq[rows[g]], asf[rows[g]], bq[g], bsf[g], threads=4)
                oracle.assert_parity(got[rows[g]], want, aq[rows[g]], asf[rows[g]], bq[g], bsf[g])
            assert got.any(), link
        return {name: _bytes(d[name]) if d[name].element_size() != 2 else d[name].view(torch.int16).cpu().numpy() for name in ("w", "dw", "y", "dx")}

    give(1)
    step()
    torch.cuda.synchronize()
    first = check(1)

    saved = {name: d[name].clone() for name in ("w", "m", "v")}
    give(2)
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
    for name in ("dw", "y", "dx"):
        d[name].zero_()
    for q_, sf_ in out:
        q_.fill_(0xA5)
        sf_.view(torch.int32).fill_(0x7FC0A5A5)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    second = check(2)
    for name in first:
        assert not np.array_equal(first[name], second[name]), name
