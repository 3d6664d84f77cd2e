"""Times gemm_fp8_fp8_fp32_nt against gemm_fp8_fp8_bf16_nt on the default tiling (bf16-exact arithmetic): bf16 rows, fp32 rows, and fp32
rows with c is out (in-place accumulation), warm (one operand set, back to back, after a 400 ms pre-warm at sustained clocks) and cold
(operand sets rotated past the 256 MB Infinity Cache, as decode weights arrive).  Prints one line per (shape, form) and the shader
clock the dense kernel's main loop holds (gemm_fp8_loop_clock).  --flavours: the same forms on the two-round dense shapes under each
store flavour of the output rows ($DGA_OUT_NT = 0 plain, 1 nt, 2 sc0 sc1; the default picks 2 for rasters of at most two rounds), each
in a fresh child process (the variable is read once per process).
Usage: python scripts/fp32_out_timing.py [--out profiles/fp32_out_timing.txt] [--flavours] [--shapes i,j]"""
import argparse
import os
import subprocess
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import deepgemm_ascend_amd as dga  # noqa: E402

SHAPES = [(4096, 4096, 4096, "4096^3"), (4096, 2048, 7168, "configs[2]"), (128, 4096, 7168, "decode split-K"),
          (64, 4096, 7168, "decode split-K"), (8, 4096, 7168, "workgroup split-K"), (3511, 6151, 8191, "Stream-K")]


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
    kb, nb = (k + 127) // 128, (n + 127) // 128
    out = []
    for s in range(sets):
        g = torch.Generator(device="cuda").manual_seed(s)
        a = (torch.randint(0, 120, (m, k), dtype=torch.uint8, device="cuda", generator=g))
        b = (torch.randint(0, 120, (n, k), dtype=torch.uint8, device="cuda", generator=g))
        sfa = torch.rand((m, kb), device="cuda", generator=g) + 0.5
        sfb = torch.rand((nb, kb), device="cuda", generator=g) + 0.5
        out.append(((a, sfa), (b, sfb)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--flavours", action="store_true")
    ap.add_argument("--shapes", default=None, help="indices into SHAPES (comma-separated)")
    ap.add_argument("--no-clock", action="store_true")
    args = ap.parse_args()
    lines = []
    if args.flavours:
        for nt in ("0", "1", "2"):
            env = dict(os.environ, DGA_OUT_NT=nt)
            r = subprocess.run([sys.executable, __file__, "--shapes", "0,1", "--no-clock"], env=env, capture_output=True, text=True,
                               timeout=600)
            if r.returncode != 0:
                print(r.stdout + r.stderr, flush=True)
                sys.exit(r.returncode)
            lines += [f"DGA_OUT_NT={nt}: {l}" for l in r.stdout.splitlines() if "x" in l.split()[0]]
            print("\n".join(lines[-6:]), flush=True)
        if args.out:
            Path(args.out).write_text("\n".join(lines) + "\n")
        return

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if not args.no_clock:
        a, sfa, b, sfb = *operands(4096, 4096, 4096, 1)[0][0], *operands(4096, 4096, 4096, 1)[0][1]
        mhz, loop_us = dga.gemm_fp8_loop_clock((a, sfa), (b, sfb), torch.empty((4096, 4096), dtype=torch.bfloat16, device="cuda"))
        say(f"device {torch.cuda.get_device_name()}  main-loop shader clock {mhz:.0f} MHz (fast-path loop-clock build, 4096^3)")
    say("shape                  form          warm_us  cold_us  vs_bf16_warm  vs_bf16_cold")
    pick = [int(i) for i in args.shapes.split(",")] if args.shapes else range(len(SHAPES))
    for m, n, k, what in (SHAPES[i] for i in pick):
        bytes_per_set = m * k + n * k
        sets = max(1, min(64, -(-512 * 2 ** 20 // bytes_per_set)))
        ops = operands(m, n, k, sets)
        o16 = torch.empty((m, n), dtype=torch.bfloat16, device="cuda")
        o32 = torch.zeros((m, n), dtype=torch.float32, device="cuda")
        forms = {
            "bf16": lambda i: dga.gemm_fp8_fp8_bf16_nt(*ops[i % sets], o16),
            "fp32": lambda i: dga.gemm_fp8_fp8_fp32_nt(*ops[i % sets], o32),
            "fp32 c=out": lambda i: dga.gemm_fp8_fp8_fp32_nt(*ops[i % sets], o32, c=o32),
        }
        base = {}
        t = dga.tiling_fp32_out(m, n, k)
        for name, fn in forms.items():
            warm = time_us(lambda i: fn(0))
            cold = time_us(fn)
            base.setdefault("w", warm); base.setdefault("c", cold)
            say(f"{m}x{n}x{k:<6} {what:<17} {name:<12} {warm:8.1f} {cold:8.1f}  {warm / base['w']:10.3f}  {cold / base['c']:10.3f}"
                f"   (tiling kernelSerial {t.kernelSerial} build {t.build} {t.m1}x{t.n1} split {t.splitkFactor})")
        del ops
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
