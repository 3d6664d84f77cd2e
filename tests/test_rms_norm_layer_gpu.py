"""GPU: the norm in front of an MoE block with everything that reads it, T = 130 tokens, H = 256, N = 128 output columns, E = 8 experts:
  rms_norm_per_token_cast_to_fp8(x, weight, residual=res, norm_out=True)          residual_out, rstd, norm, (q, sf)
  gemm_fp8_fp8_bf16_nt((q, sf), (Wq, sW))                                         a dense projection of all tokens, bf16 [T, N]
  router_topk(norm @ gate^T, k)                                                   the gate on the 16-bit norm
  rms_norm_backward(grad_y, residual_out, weight, rstd, grad_residual=...)        dx on the residual stream, dweight
eagerly, then as one captured single-stream graph that is replayed after the inputs are rewritten.  Every link is checked against the
references on what the replay itself produced; the GEMM link bit for bit against the same GEMM on per_token_cast_to_fp8 of the float32 y."""
import numpy as np
import pytest
import torch

import rms_norm_ref as N
import router_ref as R

pytestmark = pytest.mark.gpu

T, H, NOUT, E, K = 130, 256, 128, 8, 2
DTYPE, FUNC = "bf16", "softmax"


def _bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).cuda()


def _inputs(seed):
    x, res, w = N.forward_inputs(H, T, DTYPE, False, seed=seed)
    rng = np.random.default_rng([seed, 9])
    return x, res, w, N.to_dtype(rng.standard_normal((T, H)) * 0.5, DTYPE), N.to_dtype(rng.standard_normal((T, H)) * 0.25, DTYPE)


def test_the_layer_eager_then_one_graph(dga, oracle):
    x, res, w, gy, gr = _inputs(1)
    g = torch.Generator().manual_seed(3)
    wq, wsf = dga.per_block_cast_to_fp8((torch.randn(NOUT, H, generator=g) * 0.05).cuda())
    gate = (torch.randn(E, H, generator=g) * 0.2).to(torch.bfloat16).cuda()
    d = {"x": _bf16(x), "res": _bf16(res), "w": _bf16(w), "gy": _bf16(gy), "gr": _bf16(gr)}
    f32 = lambda *s: torch.full(s, R.SENTINEL_F32, dtype=torch.int32, device="cuda").view(torch.float32)
    b16 = lambda *s: torch.full(s, 0x7FC1, dtype=torch.int16, device="cuda").view(torch.bfloat16)

    def buffers():
        return {"q": torch.full((T, H), 0xA5, dtype=torch.uint8, device="cuda"), "sf": f32(T, H // 128), "norm": b16(T, H), "residual": b16(T, H),
                "rstd": f32(T), "proj": b16(T, NOUT), "logits": b16(T, E), "ids": torch.full((T, K), R.SENTINEL_ID, dtype=torch.int32, device="cuda"),
                "weights": f32(T, K), "scores": f32(T, E), "dx": b16(T, H), "dweight": f32(H)}
    b = buffers()

    def step():
        dga.rms_norm_per_token_cast_to_fp8(d["x"], d["w"], eps=N.EPS, residual=d["res"], norm_out=True,
                                           out={name: b[name] for name in ("q", "sf", "norm", "residual", "rstd")})
        dga.gemm_fp8_fp8_bf16_nt((b["q"], b["sf"]), (wq, wsf), b["proj"])
        torch.matmul(b["norm"], gate.t(), out=b["logits"])
        dga.router_topk(b["logits"], K, score_func=FUNC, out=(b["ids"], b["weights"], b["scores"]))
        dga.rms_norm_backward(d["gy"], b["residual"], d["w"], b["rstd"], grad_residual=d["gr"], out=(b["dx"], b["dweight"]))

    def check(x, res, w, gy, gr):
        n = {name: N.bits_of(t) for name, t in b.items()}
        want, z = N.residual_ref(x, res, DTYPE)
        assert np.array_equal(n["residual"], want)
        rstd = n["rstd"].view(np.float32)
        exact = N.rstd64(z, N.EPS)
        assert (np.abs(rstd - exact) <= N.rstd_bar(H) * exact).all()
        y = N.y_ref(z, rstd, w)
        assert np.array_equal(n["norm"], N.norm_bits(y, DTYPE))
        q, sf = oracle.quant_1x128(y)
        assert np.array_equal(n["q"], q) and np.array_equal(n["sf"], sf.view(np.uint32))
        # the projection: the same GEMM on the separate quantiser's output from the float32 y, bit for bit
        proj = torch.empty(T, NOUT, dtype=torch.bfloat16, device="cuda")
        dga.gemm_fp8_fp8_bf16_nt(dga.per_token_cast_to_fp8(torch.from_numpy(y).cuda()), (wq, wsf), proj, sync=True)
        assert np.array_equal(n["proj"], N.bits_of(proj)) and (n["proj"] != 0x7FC1).all()
        # the gate: a 16-bit matmul of the norm the run wrote, then the router on the logits the run wrote
        norm, gate32 = N.from_bits(n["norm"], DTYPE).astype(np.float64), gate.float().cpu().numpy().astype(np.float64)
        logits = N.from_bits(n["logits"], DTYPE)
        assert (np.abs(logits - norm @ gate32.T) <= 2.0 ** -7 * np.abs(norm @ gate32.T) + 2.0 ** -12 * (np.abs(norm) @ np.abs(gate32).T)).all()
        s = n["scores"].view(np.float32)
        p64 = R.scores64(logits, FUNC)
        assert (np.abs(s - p64) <= R.score_bar(E, FUNC) * p64).all()
        rid, rw = R.select_ref(s, K, None)
        assert np.array_equal(n["ids"].view(np.int32), rid) and np.array_equal(n["weights"], rw.view(np.uint32))
        # the backward, on the z and rstd the forward wrote: the float32 dx alone inside its bound, the step's dx the separate sum
        dx32, dw = dga.rms_norm_backward(d["gy"], b["residual"], d["w"], b["rstd"], out_dtype=torch.float32, sync=True)
        dx32, dw = dx32.cpu().numpy(), dw.cpu().numpy()
        ref_dx, ref_dw, m = N.backward64(gy, z, w, rstd)
        assert (np.abs(dx32 - ref_dx) <= N.dx_bar(m, H)).all() and (np.abs(dw - ref_dw) <= N.dweight_bar(m, T)).all()
        assert np.array_equal(n["dx"], R.round_to(np.add(dx32, gr, dtype=np.float32), DTYPE))
        assert np.array_equal(n["dweight"], dw.view(np.uint32))
        return n

    step(); torch.cuda.synchronize()
    first = check(x, res, w, gy, gr)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        step()
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        step()
    torch.cuda.synchronize()

    x, res, w, gy, gr = _inputs(2)
    for name, a in (("x", x), ("res", res), ("w", w), ("gy", gy), ("gr", gr)):
        d[name].copy_(_bf16(a))
    fresh = buffers()
    for name in b:
        b[name].copy_(fresh[name])
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    second = check(x, res, w, gy, gr)
    assert not np.array_equal(second["q"], first["q"]) and not np.array_equal(second["dx"], first["dx"])
