"""Times k_grouped_wgrad_gemm_fp8_fp8_fp32_nt (one launch for every expert) against the loop it replaces: wgrad_gemm_fp8_fp8_fp32_nt once
per expert on contiguous copies of the expert's slices (made before timing).  Both run alternately in one process on the same operands,
device events, after a pre-warm; the outputs are checked to agree bit for bit (same tile, no split-K) before any time is reported.
Cases: (M, N) = (4096, 7168) and (7168, 2048), the gate/up and down projections of a 7168 / 2048 MoE, sum(ks) = 32768: G = 8 uniform,
G = 32 uniform, G = 32 Zipf-like with empty experts.  TFLOP/s = 2 M N sum(ks) / time, against the 2.5 PFLOP/s dense bf16 matrix peak.
Kernel time, per case: run each case alone under `rocprofv3 --kernel-trace --stats --output-format csv -d <dir>/<i> -o kgw -- python
scripts/k_grouped_wgrad_timing.py --only <i>` (i = 0..5), then `--kernel-stats <dir>` adds the kernel-time lines to --out: the k-grouped
kernel's average duration, the loop's kernel time per pass (its kernels' total over the passes, warm-up included -- the two forms run
alternately, so both ran as many passes), TFLOP/s of both from kernel time.
Usage: python scripts/k_grouped_wgrad_timing.py [--out profiles/k_grouped_wgrad_timing.txt] [--iters N] [--only i] [--kernel-stats dir]"""
import csv
import argparse
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import deepgemm_ascend_amd as dga  # noqa: E402

BF16_PEAK_TFLOPS = 2500.0


def zipf(g, total, empty):
    w = [1.0 / (i + 1) for i in range(g - empty)]
    ks = [int(total * x / sum(w)) // 128 * 128 for x in w]
    ks[0] += total - sum(ks)
    return ks + [0] * empty


CASES = [("G=8 uniform", [4096] * 8), ("G=32 uniform", [1024] * 32), ("G=32 zipf", zipf(32, 32768, 6))]
SHAPES = [(4096, 7168), (7168, 2048)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", type=int, default=None, help="run case i alone (shape i // 3, split i % 3)")
    ap.add_argument("--kernel-stats", default=None, help="directory of per-case rocprofv3 runs: report kernel time")
    args = ap.parse_args()
    if args.kernel_stats:
        return kernel_stats(args)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# {torch.cuda.get_device_name(0)}; bf16-exact, default tilings; loop = wgrad_gemm_fp8_fp8_fp32_nt per expert on contiguous copies")
    for si, (m, n) in enumerate(SHAPES):
        if args.only is not None and args.only // len(CASES) != si:
            continue
        k_total = 32768
        g = torch.Generator(device="cuda").manual_seed(m + n)
        a = torch.randint(0, 120, (m, k_total), dtype=torch.uint8, device="cuda", generator=g)
        b = torch.randint(0, 120, (n, k_total), dtype=torch.uint8, device="cuda", generator=g)
        sfa = torch.rand((m, k_total // 128), device="cuda", generator=g) + 0.5
        sfb = torch.rand((n, k_total // 128), device="cuda", generator=g) + 0.5
        for ci, (name, ks) in enumerate(CASES):
            if args.only is not None and args.only % len(CASES) != ci:
                continue
            gn = len(ks)
            t = dga.tiling_k_grouped_wgrad(m, n, k_total, gn)
            ks_t = torch.tensor(ks, dtype=torch.int32, device="cuda")
            out = torch.empty((gn, m, n), dtype=torch.float32, device="cuda")
            ref = torch.zeros((gn, m, n), dtype=torch.float32, device="cuda")
            parts, k0 = [], 0
            for i, kg in enumerate(ks):
                if kg:
                    sl = slice(k0, k0 + kg)
                    bl = slice(k0 // 128, (k0 + kg) // 128)
                    dt = dga.tiling_wgrad(m, n, kg)
                    dt.m1, dt.n1, dt.kernelSerial, dt.splitkFactor, dt.build = t.m1, t.n1, 0, 1, t.build
                    parts.append((i, (a[:, sl].contiguous(), sfa[:, bl].contiguous()), (b[:, sl].contiguous(), sfb[:, bl].contiguous()), dt))
                k0 += kg

            def grouped():
                dga.k_grouped_wgrad_gemm_fp8_fp8_fp32_nt((a, sfa), (b, sfb), out, ks, ks_tensor=ks_t, tiling_=t)

            def loop():
                for i, lhs, rhs, dt in parts:
                    dga.wgrad_gemm_fp8_fp8_fp32_nt(lhs, rhs, ref[i], tiling_=dt)

            grouped(); loop(); torch.cuda.synchronize()
            assert torch.equal(out.view(torch.int32), ref.view(torch.int32)), f"{m}x{n} {name}: outputs differ"
            t0 = time.perf_counter()
            while time.perf_counter() - t0 < 0.4:
                grouped(); loop()
            torch.cuda.synchronize()
            tg = tl = 0.0
            for _ in range(args.iters):
                for fn, acc in ((grouped, 0), (loop, 1)):
                    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
                    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
                    if acc == 0:
                        tg += e0.elapsed_time(e1)
                    else:
                        tl += e0.elapsed_time(e1)
            tg, tl = tg * 1e3 / args.iters, tl * 1e3 / args.iters
            fl = 2.0 * m * n * sum(ks) / 1e12
            build = {7: "persistent", 8: "one-tile"}.get(t.build, str(t.build))
            say(f"{m}x{n} {name:13s} tile {t.m1}x{t.n1} {build:10s} k_grouped {tg:9.1f} us {fl / tg * 1e6:7.1f} TFLOP/s "
                f"({fl / tg * 1e6 / BF16_PEAK_TFLOPS:5.1%} of bf16 peak) | loop {tl:9.1f} us {fl / tl * 1e6:7.1f} TFLOP/s | "
                f"loop / k_grouped {tl / tg:5.2f}")
            del parts
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(lines) + "\n")


def kernel_stats(args):
    lines = ["# kernel time (rocprofv3 --kernel-trace --stats, each case alone): k-grouped = its kernel's average, loop = the per-expert",
             "# kernels' total per pass"]
    for i in range(len(SHAPES) * len(CASES)):
        (m, n), (name, ks) = SHAPES[i // len(CASES)], CASES[i % len(CASES)]
        files = sorted(Path(args.kernel_stats, str(i)).rglob("*kernel_stats.csv"))
        if not files:
            lines.append(f"{m}x{n} {name:13s} (no trace)")
            continue
        kg_ns = kg_calls = loop_ns = 0.0
        for row in csv.DictReader(open(files[0])):
            if "dga::" not in row["Name"]:
                continue
            if "persistent_kernel<false, 1, 1, 1>" in row["Name"] or ", 1, 1, 1>(" in row["Name"]:
                kg_ns += float(row["TotalDurationNs"]); kg_calls += float(row["Calls"])
            else:
                loop_ns += float(row["TotalDurationNs"])
        tg, tl = kg_ns / kg_calls / 1e3, loop_ns / kg_calls / 1e3
        fl = 2.0 * m * n * sum(ks) / 1e12
        lines.append(f"{m}x{n} {name:13s} kernel: k_grouped {tg:9.1f} us {fl / tg * 1e6:7.1f} TFLOP/s ({fl / tg * 1e6 / BF16_PEAK_TFLOPS:5.1%} "
                     f"of bf16 peak) | loop {tl:9.1f} us {fl / tl * 1e6:7.1f} TFLOP/s | loop / k_grouped {tl / tg:5.2f}")
    print("\n".join(lines))
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
