"""Times per_token_cast_to_fp8 and per_block_cast_to_fp8 on [32768, 7168] (bf16, fp16, fp32): windows of back-to-back calls between two
device events (each sized to well over 100 ms after a calibration), after a warm-up; mean and min..max over the windows, and TB/s from
the bytes the call has to move (input + one byte per element + the scales).  Before any time is reported the first 64 rows are
compared with the oracle byte for byte.
A/B against another build of the library (the parent commit's, say): run once per build with --lib <path to its libdga_hip.so>, each in
a process of its own, and compare the lines.  $DGA_CAST_UNROLL (read once per process) selects the one-, two- or four-block kernel.
Usage: python scripts/cast_ab.py [--lib PATH] [--label TEXT] [--windows N] [--out profiles/cast_ab.txt]"""
import argparse
import os
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

ROWS, K = 32768, 7168


def window_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="another build of libdga_hip.so to load instead of the tree's")
    ap.add_argument("--label", default="tree")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import deepgemm_ascend_amd._lib as L
    if args.lib:
        L.LIB_PATH = Path(args.lib).resolve()
    import deepgemm_ascend_amd as dga
    from oracle import oracle
    oracle.build()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# {args.label}: {L.LIB_PATH.name if not args.lib else args.lib}; {torch.cuda.get_device_name(0)}; [{ROWS}, {K}]; "
        f"DGA_CAST_UNROLL={os.environ.get('DGA_CAST_UNROLL', '')!r}; {args.windows} windows >= 150 ms; mean [min..max] us per call")
    g = torch.Generator(device="cuda").manual_seed(1)
    x32 = torch.randn((ROWS, K), device="cuda", generator=g) * 3.0
    for dtype in (torch.bfloat16, torch.float16, torch.float32):
        x = x32.to(dtype)
        for name, fn, ofn, nscales in (("per_token", dga.per_token_cast_to_fp8, oracle.quant_1x128, ROWS * (K // 128)),
                                       ("per_block", dga.per_block_cast_to_fp8, oracle.quant_128x128, (ROWS // 128) * (K // 128))):
            q, sf = fn(x)
            torch.cuda.synchronize()
            head = 128 if name == "per_block" else 64
            wq, wsf = ofn(x[:head].float().cpu().numpy())
            assert (q[:head].view(torch.uint8).cpu().numpy() == wq).all() and (sf[:wsf.shape[0]].cpu().numpy() == wsf).all(), (name, dtype)
            window_ms(lambda: fn(x), 20)
            calls = max(50, int(150.0 / (window_ms(lambda: fn(x), 50) / 50)) + 1)
            t = np.array([window_ms(lambda: fn(x), calls) * 1e3 / calls for _ in range(args.windows)])
            nbytes = ROWS * K * (x.element_size() + 1) + 4 * nscales
            say(f"{args.label:8s} {name} {str(dtype)[6:]:8s} {t.mean():8.1f} [{t.min():8.1f}..{t.max():8.1f}] us  "
                f"{nbytes / (t.mean() * 1e-6) / 1e12:5.2f} TB/s")
        del x
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
