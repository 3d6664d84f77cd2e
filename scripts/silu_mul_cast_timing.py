"""Times silu_and_mul_per_token_cast_to_fp8 (one pass over the valid rows) against the pair it replaces: torch
F.silu(x[..., :H]) * x[..., H:] in bf16 followed by per_token_cast_to_fp8 on ALL rows.  Both run alternately in one process on the same
tensors, in windows of back-to-back calls between two device events (each window sized to well over 100 ms after a calibration), after
a warm-up; mean and min..max over the windows.  Before any time is reported the fused outputs pass the asserted criteria of the tolerance
family (tests/test_silu_mul_cast_gpu.py _check_tolerance: scales, codes, share of codes off the oracle's) on SAMPLE_ROWS valid rows spread
over the tensor, and the rows a mask excludes still hold their sentinels.
Cases (bf16, H = 2048): masked [256, 128, 4096] with full, random (randint(0, Mmax + 1), bench.py's grouped distribution) and 0..16-row
masks; flat 32768, 4096 and 64 rows.  TB/s = the bytes the valid rows need, (5 H + 4 ceil(H / 128)) per row, over the fused time.
Kernel time: run `rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o smc -- python scripts/silu_mul_cast_timing.py
--trace-pass` in a run of its own (every case: PASSES fused calls, then PASSES pairs; nothing else is launched in between), then
`--kernel-stats <dir>` appends the per-case kernel times to --out.
Usage: python scripts/silu_mul_cast_timing.py [--out profiles/silu_mul_cast_timing.txt] [--windows N] [--trace-pass] [--kernel-stats dir]"""
import argparse
import csv
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import deepgemm_ascend_amd as dga  # noqa: E402

H = 2048
G, MMAX = 256, 128
SAMPLE_ROWS = 192
PASSES = 20
CASES = ["masked full", "masked random", "masked 0..16", "flat 32768", "flat 4096", "flat 64"]


def row_bytes():
    return 5 * H + 4 * ((H + 127) // 128)


def masks():
    """The three masked_m of the masked cases (host tensors): every row, randint(0, MMAX + 1), randint(0, 17)."""
    cpu = torch.Generator().manual_seed(7)
    return (torch.full((G,), MMAX, dtype=torch.int32), torch.randint(0, MMAX + 1, (G,), generator=cpu, dtype=torch.int32),
            torch.randint(0, 17, (G,), generator=cpu, dtype=torch.int32))


FLAT_ROWS = (32768, 4096, 64)


def make_cases():
    """[(name, x, masked_m or None, valid row count)]: one [G, MMAX, 2H] tensor serves the masked cases and, flattened, the flat ones."""
    g = torch.Generator(device="cuda").manual_seed(2048)
    gate = (torch.randn((G, MMAX, H), device="cuda", generator=g) * 3.0).clamp(-16.0, 16.0).bfloat16()
    up = (torch.randn((G, MMAX, H), device="cuda", generator=g) * 3.0).bfloat16()
    x = torch.cat([gate, up], dim=-1).contiguous()
    del gate, up
    flat = x.view(G * MMAX, 2 * H)
    out = []
    for name, m in zip(CASES[:3], masks()):
        out.append((name, x, m.cuda(), int(m.sum())))
    for name, rows in zip(CASES[3:], FLAT_ROWS):
        out.append((name, flat[:rows], None, rows))
    return out


def forms(x, masked):
    lead = tuple(x.shape[:-1])
    q = torch.full(lead + (H,), 0xA5, dtype=torch.uint8, device="cuda")
    sf = torch.full(lead + (H // 128,), 0x7FC0A5A5, dtype=torch.int32, device="cuda").view(torch.float32)

    def fused():
        dga.silu_and_mul_per_token_cast_to_fp8(x, masked_m=masked, out=(q, sf))

    def pair():
        h = torch.nn.functional.silu(x[..., :H]) * x[..., H:]
        return dga.per_token_cast_to_fp8(h.view(-1, H))

    return fused, pair, q, sf


def check(name, x, masked, q, sf):
    """The tolerance family's criteria on SAMPLE_ROWS valid rows; the sentinels of the excluded rows."""
    from oracle import oracle
    from test_silu_mul_cast_gpu import _check_tolerance, _h_ref, _share_off_the_oracle
    oracle.build()
    rows_total = q.numel() // H
    if masked is not None:
        mm = masked.cpu().numpy()
        valid = np.concatenate([np.arange(mm[g]) + g * MMAX for g in range(G)]).astype(np.int64)
        rest = torch.from_numpy(np.setdiff1d(np.arange(rows_total), valid)).cuda()
        qr, sr = q.view(rows_total, H)[rest], sf.view(rows_total, -1)[rest].view(torch.int32)
        assert bool((qr == 0xA5).all()) and bool((sr == 0x7FC0A5A5).all()), f"{name}: an excluded row was written"
    else:
        valid = np.arange(rows_total)
    pick = torch.from_numpy(valid[np.linspace(0, valid.size - 1, min(SAMPLE_ROWS, valid.size)).astype(np.int64)]).cuda()
    xs = x.reshape(rows_total, 2 * H)[pick]
    gq = q.view(rows_total, H)[pick].cpu().numpy()
    gsf = sf.view(rows_total, -1)[pick].cpu().numpy()
    href = _h_ref(xs[:, :H], xs[:, H:])
    _check_tolerance(oracle, gq, gsf, href, False, np.arange(gq.shape[0]), name)      # scales, codes, share of codes off the oracle's
    _share_off_the_oracle(oracle, gq, gsf, href, False, name)                         # (printed: it counts the blocks whose scale is a ULP off)


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
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--trace-pass", action="store_true", help="PASSES fused calls then PASSES pairs per case, for a rocprofv3 run")
    ap.add_argument("--kernel-stats", default=None, help="directory of the rocprofv3 run of --trace-pass: report kernel time")
    args = ap.parse_args()
    if args.kernel_stats:
        return kernel_stats(args)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    cases = make_cases()
    if args.trace_pass:
        built = [forms(x, m) for _, x, m, _ in cases]
        torch.cuda.synchronize()
        for fused, pair, _, _ in built:
            for _ in range(PASSES):
                fused()
            for _ in range(PASSES):
                pair()
            torch.cuda.synchronize()
        return
    say(f"# {torch.cuda.get_device_name(0)}; bf16, H = {H}; fused = silu_and_mul_per_token_cast_to_fp8(out=...), pair = torch silu * up (bf16) "
        f"+ per_token_cast_to_fp8 on all rows")
    say(f"# device events around windows of back-to-back calls (>= 150 ms each), {args.windows} windows per form, alternating; "
        f"mean [min..max] us per call")
    for name, x, masked, valid in cases:
        fused, pair, q, sf = forms(x, masked)
        fused(); pair(); torch.cuda.synchronize()
        check(name, x, masked, q, sf)
        calls = {}
        for fn in (fused, pair):
            window_ms(fn, 20)                                       # warm-up, then a calibration window
            per_call = window_ms(fn, 50) / 50
            calls[fn] = max(50, int(150.0 / per_call) + 1)
        t = {fused: [], pair: []}
        for _ in range(args.windows):
            for fn in (fused, pair):
                t[fn].append(window_ms(fn, calls[fn]) * 1e3 / calls[fn])
        tf, tp = np.array(t[fused]), np.array(t[pair])
        tbs = valid * row_bytes() / (tf.mean() * 1e-6) / 1e12 if valid else 0.0
        say(f"{name:14s} valid rows {valid:6d} | fused {tf.mean():8.1f} [{tf.min():8.1f}..{tf.max():8.1f}] us {tbs:5.2f} TB/s | "
            f"pair {tp.mean():8.1f} [{tp.min():8.1f}..{tp.max():8.1f}] us | fused / pair {tf.mean() / tp.mean():5.2f}")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


def kernel_stats(args):
    """Per case from the dispatch order of the trace: the fused kernel's dispatches come PASSES at a time, and what runs between one
    case's and the next one's is that case's pairs."""
    files = sorted(Path(args.kernel_stats).rglob("*kernel_trace.csv"))
    assert files, f"no *kernel_trace.csv under {args.kernel_stats}"
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
    dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    is_fused = [("silu_mul_cast_1x128_kernel" in r["Kernel_Name"]) for r in rows]
    first = is_fused.index(True)
    rows, is_fused = rows[first:], is_fused[first:]                   # (input generation comes before the first fused call)
    lines = ["# kernel time (rocprofv3 --kernel-trace --stats, one run of --trace-pass): mean over the case's dispatches; pair = all of its "
             "kernels per pass"]
    fused_us, pair_us, case = [[] for _ in CASES], [[] for _ in CASES], -1
    seen = PASSES
    for r, f in zip(rows, is_fused):
        if f:
            if seen == PASSES:
                case, seen = case + 1, 0
            seen += 1
            fused_us[case].append(dur(r))
        else:
            pair_us[case].append(dur(r))
    rb = row_bytes()
    valid = [int(m.sum()) for m in masks()] + list(FLAT_ROWS)
    for i, name in enumerate(CASES):
        tf, tp = float(np.mean(fused_us[i])), float(np.sum(pair_us[i])) / PASSES
        tb = f"{valid[i] * rb / (tf * 1e-6) / 1e12:5.2f} TB/s" if valid[i] else ""
        lines.append(f"{name:14s} kernel: fused {tf:8.1f} us {tb} | pair {tp:8.1f} us ({len(pair_us[i]) // PASSES} kernels) | "
                     f"fused / pair {tf / tp:5.2f}")
    print("\n".join(lines))
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
