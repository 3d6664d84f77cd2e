"""Times rms_norm_per_token_cast_to_fp8 and rms_norm_backward against the torch expressions they replace, to
scripts/router_balance_timing.py's protocol: both forms run alternately in one process on the same tensors, in windows of back-to-back
calls between two device events (each window sized to well over 100 ms after a calibration), after a warm-up; mean and min..max over the
windows.  Before any time is reported the results are compared: rstd and the gradients to float32 rounding, the 16-bit outputs to a bf16
ULP, the dequantised codes to the fp8 step.
Cases (bf16, weight bf16): the forward at [32768, 7168], [32768, 2048] and [4096, 4096] with q only, q + norm_out, and q + norm_out +
residual; the backward at the first two shapes with and without grad_residual.
  new      rms_norm_per_token_cast_to_fp8(x, w, residual=..., norm_out=..., out=...);  rms_norm_backward(gy, z, w, rstd, grad_residual=..., out=...)
  torch    z = x + residual; n = torch.nn.functional.rms_norm(z, (H,), w, eps); per_token_cast_to_fp8(n);  autograd of that norm from
           a graph built once (torch.autograd.grad with retain_graph), plus the addition of grad_residual
TB/s: the bytes the fused kernel must move (forward 3, 5 and 9 per element: x in, codes out, norm out, residual in and out; backward 6 and
8: grad_y and z in, dx out, grad_residual in) over the new form's mean time.
The condition: the fused forward beats the pair at every case (new / torch < 1.0); no ratio is fixed in advance.
Usage: python scripts/rms_norm_cast_timing.py [--out profiles/rms_norm_cast_timing.txt] [--windows N]"""
import argparse
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import deepgemm_ascend_amd as dga  # noqa: E402
from scripts.cast_transposed_timing import alternate  # noqa: E402

FORWARD_SHAPES = ((32768, 7168), (32768, 2048), (4096, 4096))
BACKWARD_SHAPES = FORWARD_SHAPES[:2]
EPS = 1e-6


def dequantise(q, sf):
    t_n, h = q.shape
    return (q.float().view(t_n, h // 128, 128) * sf[:, :, None]).view(t_n, h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=4)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    fmt = lambda v: f"{v.mean():8.1f} [{v.min():8.1f}..{v.max():8.1f}] us"
    say(f"# {torch.cuda.get_device_name(0)}; bf16; new = the fused entry, torch = rms_norm (+ add) then per_token_cast_to_fp8, autograd for the "
        f"backward; device events around windows of back-to-back calls (>= 150 ms each), {args.windows} windows per form, alternating; "
        f"mean [min..max] us per call; TB/s of the bytes the fused kernel must move; condition: forward new / torch < 1.00")
    slower = []
    for t_n, h in FORWARD_SHAPES:
        g = torch.Generator(device="cuda").manual_seed(t_n + h)
        x = (torch.randn((t_n, h), device="cuda", generator=g) * 1.5).bfloat16()
        res = (torch.randn((t_n, h), device="cuda", generator=g) * 0.75).bfloat16()
        w = (1.0 + 0.25 * torch.randn((h,), device="cuda", generator=g)).bfloat16()
        for label, with_norm, with_res, bytes_per in (("q", False, False, 3), ("q + norm", True, False, 5), ("q + norm + residual", True, True, 9)):
            out = {"q": torch.empty((t_n, h), dtype=torch.uint8, device="cuda"), "sf": torch.empty((t_n, h // 128), device="cuda"),
                   "rstd": torch.empty((t_n,), device="cuda")}
            if with_norm:
                out["norm"] = torch.empty_like(x)
            if with_res:
                out["residual"] = torch.empty_like(x)
            new = lambda: dga.rms_norm_per_token_cast_to_fp8(x, w, eps=EPS, residual=res if with_res else None, norm_out=with_norm, out=out)

            def old():
                z = x + res if with_res else x
                n = torch.nn.functional.rms_norm(z, (h,), w, EPS)
                return (z, n) + tuple(dga.per_token_cast_to_fp8(n))

            name = f"forward  [{t_n}, {h}] {label:19s}"
            got = new()
            z, n, q, sf = old()
            torch.cuda.synchronize()
            rstd = torch.rsqrt(z.float().pow(2).mean(dim=-1) + EPS)
            assert torch.allclose(got.rstd, rstd, rtol=1e-5), f"{name}: rstd differs"
            assert not with_res or torch.equal(got.residual, z), f"{name}: the residual output differs"
            assert not with_norm or torch.allclose(got.norm.float(), n.float(), rtol=2.0 ** -7, atol=1e-30), f"{name}: the norm differs"
            deq = dequantise(got.q, got.sf)
            assert bool(((deq - n.float()).abs() <= 2.0 ** -3 * n.float().abs() + 2.0 ** -9 * dequantise(q, sf).abs().amax()).all()), f"{name}: the codes differ"
            del got, z, n, q, sf, rstd, deq
            t = alternate([new, old], args.windows)
            ratio = t[new].mean() / t[old].mean()
            tb = t_n * h * bytes_per / (t[new].mean() * 1e-6) / 1e12
            say(f"{name} | new {fmt(t[new])} | torch {fmt(t[old])} | new / torch {ratio:5.2f} | {tb:4.2f} TB/s")
            if ratio >= 1.0:
                slower.append(" ".join(name.split()))
            del out
            torch.cuda.empty_cache()
    for t_n, h in BACKWARD_SHAPES:
        g = torch.Generator(device="cuda").manual_seed(t_n + h + 1)
        z = (torch.randn((t_n, h), device="cuda", generator=g) * 1.5).bfloat16()
        gy = (torch.randn((t_n, h), device="cuda", generator=g) * 0.5).bfloat16()
        gr = (torch.randn((t_n, h), device="cuda", generator=g) * 0.25).bfloat16()
        w = (1.0 + 0.25 * torch.randn((h,), device="cuda", generator=g)).bfloat16()
        rstd = dga.rms_norm_per_token_cast_to_fp8(z, w, eps=EPS, quantize=False, norm_out=True).rstd
        zg, wg = z.detach().requires_grad_(), w.detach().requires_grad_()
        y = torch.nn.functional.rms_norm(zg, (h,), wg, EPS)
        for label, with_gr, bytes_per in (("", False, 6), ("+ grad_residual", True, 8)):
            out = (torch.empty_like(z), torch.empty((h,), device="cuda"))
            new = lambda: dga.rms_norm_backward(gy, z, w, rstd, grad_residual=gr if with_gr else None, out=out)

            def old():
                dz, dw = torch.autograd.grad(y, (zg, wg), gy, retain_graph=True)
                return (dz + gr if with_gr else dz), dw

            name = f"backward [{t_n}, {h}] {label:19s}"
            new()
            dz, dw = old()
            torch.cuda.synchronize()
            assert torch.allclose(out[0].float(), dz.float(), rtol=2.0 ** -6, atol=float(dz.float().abs().max()) * 2.0 ** -8), f"{name}: dx differs"
            assert torch.allclose(out[1], dw.float(), rtol=2e-2, atol=float(dw.float().abs().max()) * 1e-2), f"{name}: dweight differs"
            del dz, dw
            t = alternate([new, old], args.windows)
            ratio = t[new].mean() / t[old].mean()
            tb = t_n * h * bytes_per / (t[new].mean() * 1e-6) / 1e12
            say(f"{name} | new {fmt(t[new])} | torch {fmt(t[old])} | new / torch {ratio:5.2f} | {tb:4.2f} TB/s")
            del out
            torch.cuda.empty_cache()
        del y, zg, wg
    say("# forward cases not faster than the torch pair: " + ("; ".join(slower) if slower else "none"))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
