"""Times indexer_prepare_q / indexer_prepare_k / indexer_prepare_backward against what a user had before them, under the protocol of
scripts/indexer_kl_timing.py: old and new run alternately in one process on the same tensors, in windows of back-to-back calls between two
device events (each over 150 ms after a calibration, at least 3 calls), after a warm-up; mean and min..max over the windows.  Before any
time is reported the results are compared: the dequantised rows (codes x scale) to 2^-3 of their largest value -- the old path rounds to
bf16 after the norm, after the RoPE and inside the matmul, and a value that moves by 2^-9 can move its e4m3 code by one step, 2^-4 of the
row's largest value at the top binade -- and the backward's bf16 output to 2^-6 of its largest value.
  old   the torch path: layer_norm in float32 (k), RoPE in float32 on the first 64 dimensions and a cat, the rotation as a bf16 matmul
        against the 128 x 128 +-1 matrix times 128^-1/2 (what rotate_activation falls back to without fast_hadamard_transform),
        per_token_cast_to_fp8 or per_token_cast_to_fp8_paged, and weights * (H^-1/2 softmax_scale) * q_scale; the backward: the division by
        the scale, a float32 matmul, the transposed RoPE, a cat and the cast to bf16
  new   one launch each
Cases: q at M = 32768 and M = 128 tokens, H = 64, bf16; k (LayerNorm) at N = 32768 contiguous and N = 128 paged; the backward on the two
large shapes.  Beside each time: the bytes the call must move and the rate they amount to (the row-wise quantisers reach 4-5 TB/s on large
tensors).  The condition, set before the run: at every case the slowest new window is faster than the fastest old one.
Usage: python scripts/indexer_prepare_timing.py [--out profiles/indexer_prepare_timing.txt] [--windows N]"""
import argparse
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import deepgemm_ascend_amd as dga  # noqa: E402
from scripts.indexer_topk_timing import alternate  # noqa: E402

H, D, P, EPS = 64, 128, 65536, 1e-6
WS = H ** -0.5 * D ** -0.5


def hadamard(dtype):
    m = torch.ones((1, 1), device="cuda")
    for _ in range(7):
        m = torch.cat((torch.cat((m, m), 1), torch.cat((m, -m), 1)), 0)
    return (m * D ** -0.5).to(dtype)


def rope(x, cs, transposed=False):
    c, s = cs[..., :32], (-cs[..., 32:] if transposed else cs[..., 32:])
    a, b = x[..., :32].float(), x[..., 32:64].float()
    return torch.cat((a * c - b * s, a * s + b * c, x[..., 64:].float()), dim=-1)


def old_q(q, pos, table, w, hm):
    y = rope(q, table[pos][:, None, :]).to(torch.bfloat16) @ hm
    codes, sf = dga.per_token_cast_to_fp8(y.view(-1, D))
    return codes, sf.view(w.shape), w * WS * sf.view(w.shape)


def old_k(k, pos, table, gamma, beta, hm, cache, slots):
    z = torch.nn.functional.layer_norm(k.float(), (D,), gamma, beta, EPS)
    y = rope(z, table[pos]).to(torch.bfloat16) @ hm
    return dga.per_token_cast_to_fp8(y) if cache is None else dga.per_token_cast_to_fp8_paged(y, cache, slots)


def old_bwd(g, pos, table, div, hm32):
    y = (g if div is None else g / div[..., None]) @ hm32
    return rope(y, table[pos] if g.dim() == 2 else table[pos][:, None, :], transposed=True).to(torch.bfloat16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=3)
    args = ap.parse_args()
    lines, failed = [], []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    fmt = lambda v: f"{v.mean():9.1f} [{v.min():9.1f}..{v.max():9.1f}] us"
    say(f"# {torch.cuda.get_device_name(0)}; H = {H}, bf16 inputs; new = one launch, old = layer_norm / RoPE + cat / bf16 matmul against the "
        f"Hadamard matrix / per_token_cast_to_fp8(_paged) / weight fold in torch; device events around windows of back-to-back calls (>= 150 ms "
        f"each, at least 3 calls), {args.windows} windows per form, alternating; results compared first; mean [min..max] us per call")
    say("# bytes: what the new call must move; condition: max new < min old at every case")
    gen = torch.Generator(device="cuda").manual_seed(1)
    ang = torch.arange(P, device="cuda")[:, None] * 10000.0 ** (-torch.arange(32, device="cuda") / 32)[None, :]
    table = torch.cat((ang.cos(), ang.sin()), 1).contiguous()
    hm, hm32 = hadamard(torch.bfloat16), hadamard(torch.float32)
    gamma, beta = 1 + 0.1 * torch.randn(D, device="cuda", generator=gen), 0.1 * torch.randn(D, device="cuda", generator=gen)

    def report(name, new, old, nbytes, diff):
        tm = alternate([new, old], args.windows)
        us = tm[new].mean()
        say(f"{name:26s} | new {fmt(tm[new])} | old {fmt(tm[old])} | old / new {tm[old].mean() / us:6.2f} | {nbytes / 1e6:8.2f} MB, "
            f"{nbytes / (us * 1e-6) / 1e12:5.2f} TB/s | differs by {diff:.1e} of the largest value")
        if not tm[new].max() < tm[old].min():
            failed.append(name)

    def deq(codes, sf):
        return codes.float().view(-1, D) * sf.reshape(-1, 1)

    def rel(a, b):
        return float((a.float() - b.float()).abs().max()) / float(b.float().abs().max())

    for m in (32768, 128):
        q = torch.randn((m, H, D), device="cuda", generator=gen).to(torch.bfloat16)
        w = torch.randn((m, H), device="cuda", generator=gen)
        pos = torch.randint(0, P, (m,), device="cuda", generator=gen)
        out = dga.indexer_prepare_q(q, pos, table, weights=w, weight_scale=WS)
        new = lambda: dga.indexer_prepare_q(q, pos, table, weights=w, weight_scale=WS, out=out)
        old = lambda: old_q(q, pos, table, w, hm)
        ref = old()
        torch.cuda.synchronize()
        diff = rel(deq(out[0], out[1]), deq(ref[0], ref[1]))
        assert diff <= 2.0 ** -3, diff
        report(f"q        M = {m}", new, old, m * H * (2 * D + D + 4 + 8) + m * 8, diff)
        if m == 32768:
            g = torch.randn((m, H, D), device="cuda", generator=gen)
            gin = torch.empty((m, H, D), device="cuda", dtype=torch.bfloat16)
            new = lambda: dga.indexer_prepare_backward(g, pos, table, row_div=out[1], out=(gin,))
            old = lambda: old_bwd(g, pos, table, out[1], hm32)
            new()
            diff = rel(gin, old())
            assert diff <= 2.0 ** -6, diff
            report(f"backward [{m}, {H}, 128]", new, old, m * H * (4 * D + 2 * D + 4) + m * 8, diff)
            del g, gin
        del q, w, out, ref
        torch.cuda.empty_cache()
    for n, paged in ((32768, False), (128, True)):
        k = torch.randn((n, D), device="cuda", generator=gen).to(torch.bfloat16)
        pos = torch.randint(0, P, (n,), device="cuda", generator=gen)
        caches = [torch.zeros((4, 8448), dtype=torch.uint8, device="cuda") for _ in range(2)] if paged else [None, None]
        slots = torch.randperm(256, device="cuda", generator=gen)[:n] if paged else None
        kw = dict(norm_weight=gamma, norm_bias=beta, eps=EPS, kv_cache=caches[0], slot_mapping=slots, contiguous=not paged)
        out = dga.indexer_prepare_k(k, pos, table, **kw)
        new = lambda: dga.indexer_prepare_k(k, pos, table, out=out, **kw)
        old = lambda: old_k(k, pos, table, gamma, beta, hm, caches[1], slots)
        new(), old()
        torch.cuda.synchronize()
        if paged:
            pair = [(c[:, :8192].reshape(-1, D).view(torch.float8_e4m3fn), c[:, 8192:].contiguous().view(torch.float32)) for c in caches]
        else:
            pair = [(out.k_fp8, out.kscale), old()]
        diff = rel(deq(*pair[0]), deq(*pair[1]))
        assert diff <= 2.0 ** -3, diff
        report(f"k        N = {n}{' paged' if paged else ''}", new, old, n * (2 * D + D + 4 + 8 + 8 + (8 if paged else 0)), diff)
        if not paged:
            g = torch.randn((n, D), device="cuda", generator=gen)
            gin = torch.empty((n, D), device="cuda", dtype=torch.bfloat16)
            new = lambda: dga.indexer_prepare_backward(g, pos, table, out=(gin,))
            old = lambda: old_bwd(g, pos, table, None, hm32)
            new()
            diff = rel(gin, old())
            assert diff <= 2.0 ** -6, diff
            report(f"backward [{n}, 128]", new, old, n * (4 * D + 2 * D + 8), diff)
    say("# cases where new is not faster than old beyond the spread: " + ("; ".join(failed) if failed else "none"))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
