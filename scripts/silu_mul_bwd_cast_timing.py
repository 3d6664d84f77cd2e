"""Times silu_and_mul_backward_per_token_cast_to_fp8 (one pass over the valid rows), with and without grad_x_out, against the composition
it replaces: torch autograd of silu(gate) * up in bf16 (the backward alone: the forward graph is built once, outside the timed windows, and
kept), torch.cat of the two gradients, and per_token_cast_to_fp8 on ALL rows.  The forms run alternately in one process on the same tensors,
in windows of back-to-back calls between two device events (each window sized to well over 100 ms after a calibration), after a warm-up; mean
and min..max over the windows.  Before any time is reported the fused outputs pass the criteria of the tolerance family
(tests/test_silu_mul_bwd_cast_gpu.py _check_tolerance: element bounds, scales, codes) on SAMPLE_ROWS valid rows spread over the tensor -- the
fp32 gradient from an fp32 call on those rows, whose codes and scales must be the bf16 call's byte for byte --, grad_x_out is the RNE of that
fp32 gradient, and the rows a mask excludes still hold their sentinels in every output.
Cases (bf16, H = 2048): masked [256, 128, .] with full, random (randint(0, Mmax + 1)) and 0..16-row masks; flat 32768, 4096 and 64 rows.
TB/s = the bytes the valid rows need over the fused time: per row 6 H in (gate, up, grad) and 2 H + 4 (2 H / 128) out (codes, scales), and
4 H more with grad_x_out.
Kernel time: run `rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o smbc -- python scripts/silu_mul_bwd_cast_timing.py
--trace-pass` in a run of its own (every case: PASSES fused calls, PASSES with grad_x_out, then PASSES compositions; nothing else is
launched in between), then `--kernel-stats <dir>` appends the per-case kernel times to --out.
Usage: python scripts/silu_mul_bwd_cast_timing.py [--out profiles/silu_mul_bwd_cast_timing.txt] [--windows N] [--trace-pass]
[--kernel-stats dir]"""
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
FLAT_ROWS = (32768, 4096, 64)
KERNEL = "silu_mul_bwd_cast_1x128_kernel"


def row_bytes(with_gx):
    return 6 * H + 2 * H + 4 * (2 * H // 128) + (4 * H if with_gx else 0)


def masks():
    """The three masked_m of the masked cases (host tensors): every row, randint(0, MMAX + 1), randint(0, 17)."""
    cpu = torch.Generator().manual_seed(7)
    return (torch.full((G,), MMAX, dtype=torch.int32), torch.randint(0, MMAX + 1, (G,), generator=cpu, dtype=torch.int32),
            torch.randint(0, 17, (G,), generator=cpu, dtype=torch.int32))


def make_cases():
    """[(name, x, grad, masked_m or None, valid row count)]: one [G, MMAX, .] pair of tensors serves the masked cases and, flattened, the
    flat ones."""
    g = torch.Generator(device="cuda").manual_seed(2048)
    gate = (torch.randn((G, MMAX, H), device="cuda", generator=g) * 3.0).clamp(-16.0, 16.0).bfloat16()
    up = (torch.randn((G, MMAX, H), device="cuda", generator=g) * 3.0).bfloat16()
    grad = (torch.randn((G, MMAX, H), device="cuda", generator=g) * 0.5).bfloat16().contiguous()
    x = torch.cat([gate, up], dim=-1).contiguous()
    del gate, up
    fx, fg = x.view(G * MMAX, 2 * H), grad.view(G * MMAX, H)
    out = []
    for name, m in zip(CASES[:3], masks()):
        out.append((name, x, grad, m.cuda(), int(m.sum())))
    for name, rows in zip(CASES[3:], FLAT_ROWS):
        out.append((name, fx[:rows], fg[:rows], None, rows))
    return out


def forms(x, grad, masked):
    lead = tuple(x.shape[:-1])
    q = torch.full(lead + (2 * H,), 0xA5, dtype=torch.uint8, device="cuda")
    sf = torch.full(lead + (2 * H // 128,), 0x7FC0A5A5, dtype=torch.int32, device="cuda").view(torch.float32)
    gx = torch.full(lead + (2 * H,), 0xA5A5 - 0x10000, dtype=torch.int16, device="cuda").view(torch.bfloat16)
    # the composition's forward graph, built once: leaves that view x's two halves, as a training step holds them after its forward
    gate = x[..., :H].detach().requires_grad_(True)
    up = x[..., H:].detach().requires_grad_(True)
    hfwd = torch.nn.functional.silu(gate) * up

    def fused():
        dga.silu_and_mul_backward_per_token_cast_to_fp8(x, grad, masked_m=masked, out=(q, sf))

    def fused_gx():
        dga.silu_and_mul_backward_per_token_cast_to_fp8(x, grad, masked_m=masked, out=(q, sf), grad_x_out=gx)

    def composition():
        dgate, dup = torch.autograd.grad(hfwd, (gate, up), grad, retain_graph=True)
        return dga.per_token_cast_to_fp8(torch.cat([dgate, dup], dim=-1).view(-1, 2 * H))

    return fused, fused_gx, composition, q, sf, gx


def check(name, x, grad, masked, q, sf, gx):
    """The tolerance family's criteria on SAMPLE_ROWS valid rows; the sentinels of the excluded rows."""
    from oracle import oracle
    from test_silu_mul_bwd_cast_gpu import _check_tolerance, _reference
    oracle.build()
    rows_total = q.numel() // (2 * H)
    if masked is not None:
        mm = masked.cpu().numpy()
        valid = np.concatenate([np.arange(mm[g]) + g * MMAX for g in range(G)]).astype(np.int64)
        rest = torch.from_numpy(np.setdiff1d(np.arange(rows_total), valid)).cuda()
        qr, sr = q.view(rows_total, 2 * H)[rest], sf.view(rows_total, -1)[rest].view(torch.int32)
        gr = gx.view(rows_total, 2 * H)[rest].view(torch.int16)
        assert bool((qr == 0xA5).all()) and bool((sr == 0x7FC0A5A5).all()) and bool((gr == 0xA5A5 - 0x10000).all()), \
            f"{name}: an excluded row was written"
    else:
        valid = np.arange(rows_total)
    pick = torch.from_numpy(valid[np.linspace(0, valid.size - 1, min(SAMPLE_ROWS, valid.size)).astype(np.int64)]).cuda()
    xs, ds = x.reshape(rows_total, 2 * H)[pick].contiguous(), grad.reshape(rows_total, H)[pick].contiguous()
    gx32 = torch.empty(xs.shape, dtype=torch.float32, device="cuda")
    q32, sf32 = dga.silu_and_mul_backward_per_token_cast_to_fp8(xs.float(), ds.float(), grad_x_out=gx32, sync=True)
    gq, gsf = q.view(rows_total, 2 * H)[pick], sf.view(rows_total, -1)[pick]
    assert torch.equal(q32.view(torch.uint8), gq) and torch.equal(sf32.view(torch.int32), gsf.view(torch.int32)), name
    assert torch.equal(gx32.bfloat16().view(torch.int16), gx.view(rows_total, 2 * H)[pick].view(torch.int16)), name
    ref, bound = _reference(xs[:, :H], xs[:, H:], ds)
    _check_tolerance(oracle, name, gx32.cpu().numpy().astype(np.float64), gq.cpu().numpy(), gsf.cpu().numpy(), ref, bound)


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
    ap.add_argument("--trace-pass", action="store_true", help="PASSES calls of each form per case, for a rocprofv3 run")
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
        built = [forms(x, d, m) for _, x, d, m, _ in cases]
        torch.cuda.synchronize()
        for fused, fused_gx, composition, _, _, _ in built:
            for fn in (fused, fused_gx, composition):
                for _ in range(PASSES):
                    fn()
            torch.cuda.synchronize()
        return
    say(f"# {torch.cuda.get_device_name(0)}; bf16, H = {H}; fused = silu_and_mul_backward_per_token_cast_to_fp8(out=...), +gx = the same with "
        f"grad_x_out, comp = torch autograd backward of silu(gate) * up (bf16) + cat + per_token_cast_to_fp8 on all rows")
    say(f"# device events around windows of back-to-back calls (>= 150 ms each), {args.windows} windows per form, alternating; "
        f"mean [min..max] us per call; TB/s over the valid rows' own bytes ({row_bytes(False)} per row, {row_bytes(True)} with grad_x_out)")
    for name, x, grad, masked, valid in cases:
        fused, fused_gx, composition, q, sf, gx = forms(x, grad, masked)
        fused(); torch.cuda.synchronize()
        q_alone, sf_alone = q.clone(), sf.clone()
        fused_gx(); composition(); torch.cuda.synchronize()
        assert torch.equal(q_alone, q) and torch.equal(sf_alone.view(torch.int32), sf.view(torch.int32)), "grad_x_out changed (dq, dsf)"
        check(name, x, grad, masked, q, sf, gx)
        fns = (fused, fused_gx, composition)
        calls = {}
        for fn in fns:
            window_ms(fn, 20)                                       # warm-up, then a calibration window
            per_call = window_ms(fn, 50) / 50
            calls[fn] = max(50, int(150.0 / per_call) + 1)
        t = {fn: [] for fn in fns}
        for _ in range(args.windows):
            for fn in fns:
                t[fn].append(window_ms(fn, calls[fn]) * 1e3 / calls[fn])
        tf, tg, tc = (np.array(t[fn]) for fn in fns)
        tbs = lambda tt, with_gx: valid * row_bytes(with_gx) / (tt.mean() * 1e-6) / 1e12 if valid else 0.0
        say(f"{name:14s} valid rows {valid:6d} | fused {tf.mean():8.1f} [{tf.min():8.1f}..{tf.max():8.1f}] us {tbs(tf, False):5.2f} TB/s | "
            f"+gx {tg.mean():8.1f} [{tg.min():8.1f}..{tg.max():8.1f}] us {tbs(tg, True):5.2f} TB/s | "
            f"comp {tc.mean():8.1f} [{tc.min():8.1f}..{tc.max():8.1f}] us | fused / comp {tf.mean() / tc.mean():5.2f}, "
            f"+gx / comp {tg.mean() / tc.mean():5.2f}")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


def kernel_stats(args):
    """Per case from the dispatch order of the trace: the fused kernel's dispatches come PASSES at a time, twice per case (without and with
    grad_x_out), and what runs between one case's and the next one's is that case's compositions."""
    files = sorted(Path(args.kernel_stats).rglob("*kernel_trace.csv"))
    assert files, f"no *kernel_trace.csv under {args.kernel_stats}"
    rows = sorted(csv.DictReader(open(files[0])), key=lambda r: int(r["Start_Timestamp"]))
    dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    is_fused = [(KERNEL in r["Kernel_Name"]) for r in rows]
    first = is_fused.index(True)
    rows, is_fused = rows[first:], is_fused[first:]                   # (input generation and the forward graphs come before the first call)
    lines = ["# kernel time (rocprofv3 --kernel-trace --stats, one run of --trace-pass): mean over the case's dispatches; comp = all of its "
             "kernels per pass"]
    fused_us, gx_us, comp_us = ([[] for _ in CASES] for _ in range(3))
    case, seen = -1, 2 * PASSES
    for r, f in zip(rows, is_fused):
        if f:
            if seen == 2 * PASSES:
                case, seen = case + 1, 0
            (fused_us if seen < PASSES else gx_us)[case].append(dur(r))
            seen += 1
        else:
            comp_us[case].append(dur(r))
    valid = [int(m.sum()) for m in masks()] + list(FLAT_ROWS)
    for i, name in enumerate(CASES):
        tf, tg, tc = float(np.mean(fused_us[i])), float(np.mean(gx_us[i])), float(np.sum(comp_us[i])) / PASSES
        tb = lambda tt, w: f"{valid[i] * row_bytes(w) / (tt * 1e-6) / 1e12:5.2f} TB/s" if valid[i] else ""
        lines.append(f"{name:14s} kernel: fused {tf:8.1f} us {tb(tf, False)} | +gx {tg:8.1f} us {tb(tg, True)} | comp {tc:8.1f} us "
                     f"({len(comp_us[i]) // PASSES} kernels) | fused / comp {tf / tc:5.2f}, +gx / comp {tg / tc:5.2f}")
    print("\n".join(lines))
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
