"""Times wgrad_gemm_fp8_fp8_fp32_nt (per-1x128 scales on both operands, "1D1D": sfb [N, KB]) against gemm_fp8_fp8_fp32_nt (per-128x128
sfb, "1D2D") on the SAME tiling -- the weight-gradient entry's default (dga_tiling_wgrad), bf16-exact arithmetic -- with and without
c is out, warm (one operand set, back to back, after a 400 ms pre-warm at sustained clocks) and cold (operand sets rotated past the
256 MB Infinity Cache).  Shapes: 4096^3, the weight-gradient shapes M x N x K = out_features x in_features x tokens, one odd K.
Prints one line per (shape, form); vs_1d2d is the 1D1D figure over the 1D2D one of the same c form.
Usage: python scripts/wgrad_timing.py [--out profiles/wgrad_timing.txt] [--shapes i,j]"""
import argparse
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import deepgemm_ascend_amd as dga  # noqa: E402

SHAPES = [(4096, 4096, 4096, "4096^3"), (7168, 2048, 4096, "wgrad"), (2048, 7168, 4096, "wgrad"), (7168, 2112, 8192, "wgrad"),
          (4096, 7168, 8192, "wgrad"), (1536, 7168, 4096, "wgrad"), (4096, 4096, 4100, "odd K (padding pass)")]


def time_us(fn, iters=100, prewarm_ms=400):
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < prewarm_ms:
        for _ in range(10):
            fn(0)
        torch.cuda.synchronize()
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(i)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def operands(m, n, k, sets):
    """(lhs, rhs 1D2D, rhs 1D1D) per set: the 1D1D sfb is the 1D2D one per row times a factor per row."""
    kb, nb = (k + 127) // 128, (n + 127) // 128
    out = []
    for s in range(sets):
        g = torch.Generator(device="cuda").manual_seed(s)
        a = torch.randint(0, 120, (m, k), dtype=torch.uint8, device="cuda", generator=g)
        b = torch.randint(0, 120, (n, k), dtype=torch.uint8, device="cuda", generator=g)
        sfa = torch.rand((m, kb), device="cuda", generator=g) + 0.5
        sfb = torch.rand((nb, kb), device="cuda", generator=g) + 0.5
        sfb1 = (sfb.repeat_interleave(128, dim=0)[:n] * (torch.rand((n, 1), device="cuda", generator=g) + 0.5)).contiguous()
        out.append(((a, sfa), (b, sfb), (b, sfb1)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default=None, help="indices into SHAPES (comma-separated)")
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"device {torch.cuda.get_device_name()}")
    say("shape             what                  form             warm_us  cold_us  vs_1d2d_warm  vs_1d2d_cold")
    pick = [int(i) for i in args.shapes.split(",")] if args.shapes else range(len(SHAPES))
    for m, n, k, what in (SHAPES[i] for i in pick):
        bytes_per_set = m * k + n * k
        sets = max(1, min(64, -(-512 * 2 ** 20 // bytes_per_set)))
        ops = operands(m, n, k, sets)
        o32 = torch.zeros((m, n), dtype=torch.float32, device="cuda")
        t = dga.tiling_wgrad(m, n, k)
        forms = {
            "1d2d": lambda i: dga.gemm_fp8_fp8_fp32_nt(ops[i % sets][0], ops[i % sets][1], o32, tiling_=t),
            "1d1d": lambda i: dga.wgrad_gemm_fp8_fp8_fp32_nt(ops[i % sets][0], ops[i % sets][2], o32, tiling_=t),
            "1d2d c=out": lambda i: dga.gemm_fp8_fp8_fp32_nt(ops[i % sets][0], ops[i % sets][1], o32, c=o32, tiling_=t),
            "1d1d c=out": lambda i: dga.wgrad_gemm_fp8_fp8_fp32_nt(ops[i % sets][0], ops[i % sets][2], o32, c=o32, tiling_=t),
        }
        got = {}
        for name, fn in forms.items():
            warm = time_us(lambda i: fn(0))
            cold = time_us(fn)
            got[name] = (warm, cold)
            ref = got[name.replace("1d1d", "1d2d")]
            say(f"{m}x{n}x{k:<6} {what:<21} {name:<12} {warm:8.1f} {cold:8.1f}  {warm / ref[0]:10.3f}  {cold / ref[1]:10.3f}"
                f"   (tiling kernelSerial {t.kernelSerial} build {t.build} {t.m1}x{t.n1} split {t.splitkFactor})")
        del ops
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
