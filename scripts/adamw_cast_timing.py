"""Times adamw_per_block_cast_to_fp8_transposed against the pair it replaces, to scripts/rms_norm_cast_timing.py's protocol: both forms run
alternately in one process on tensors of the same shapes, in windows of back-to-back calls between two device events (each window sized to
well over 100 ms after a calibration), after a warm-up; mean and min..max over the windows.  Before any time is reported one step of each
form from the same state is compared: w, m and v to float32 rounding of the update, the codes of the new form with the stand-alone
quantiser on the w it left behind, byte for byte.
Cases: [8, 4096, 7168], [32, 7168, 2048] and 2-D [4096, 4096], float32 gradient, with and without rowwise.
  new      adamw_per_block_cast_to_fp8_transposed(w, m, v, grad, step_scalars, rowwise=..., out=...)
  old      torch.optim.AdamW(fused=True).step() on float32 state, then per_block_cast_to_fp8_transposed(w, rowwise=..., out=...)
  bf16 m,v torch has no counterpart (its fused kernel wants the moments in the parameter's dtype): the time and the TB/s alone
TB/s: the bytes the fused kernel must move (16 in and 12 out for the update with float32 moments, 12 and 8 with bfloat16 ones, 1 out per
code layout: 30 (29) and 22 (21) per element with (without) rowwise) over the new form's mean time.
The condition: the fused call takes less time than the pair at every float32-moment case (new / old < 1.0); no ratio is fixed in advance.
Usage: python scripts/adamw_cast_timing.py [--out profiles/adamw_cast_timing.txt] [--windows N]"""
import argparse
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import deepgemm_ascend_amd as dga  # noqa: E402
from scripts.cast_transposed_timing import alternate  # noqa: E402

SHAPES = ((8, 4096, 7168), (32, 7168, 2048), (4096, 4096))
LR, BETAS, EPS, WD, STEP = 3e-4, (0.9, 0.95), 1e-8, 0.1, 3


def outputs(shape, rowwise):
    lead, (n, k) = tuple(shape[:-2]), shape[-2:]
    nb, kb = (n + 127) // 128, (k + 127) // 128
    t = (torch.empty(lead + (k, n), dtype=torch.uint8, device="cuda"), torch.empty(lead + (kb, nb), device="cuda"))
    return (t, (torch.empty(lead + (n, k), dtype=torch.uint8, device="cuda"), torch.empty(lead + (nb, kb), device="cuda"))) if rowwise else t


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
    say(f"# {torch.cuda.get_device_name(0)}; float32 w and grad; new = the fused entry, old = torch.optim.AdamW(fused=True) then "
        f"per_block_cast_to_fp8_transposed; device events around windows of back-to-back calls (>= 150 ms each), {args.windows} windows per "
        f"form, alternating; mean [min..max] us per call; TB/s of the bytes the fused kernel must move; condition: new / old < 1.00 with "
        f"float32 moments")
    slower = []
    sc = dga.adamw_step_scalars(STEP, LR, *BETAS, device="cuda")
    hyper = dict(beta1=BETAS[0], beta2=BETAS[1], eps=EPS, weight_decay=WD)
    for shape in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(sum(shape))
        w0 = torch.randn(shape, device="cuda", generator=g) * 0.05
        grad = torch.randn(shape, device="cuda", generator=g) * 1e-3
        m0 = torch.randn(shape, device="cuda", generator=g) * 5e-4
        v0 = torch.randn(shape, device="cuda", generator=g).square_() * 1e-6 + 1e-12
        elems = w0.numel()
        for rowwise in (False, True):
            name = f"{list(shape)}{' rowwise' if rowwise else '':8s}"
            # old: a parameter whose optimizer state is set to (m0, v0) at step STEP - 1
            p = torch.nn.Parameter(w0.clone())
            p.grad = grad
            opt = torch.optim.AdamW([p], lr=LR, betas=BETAS, eps=EPS, weight_decay=WD, fused=True)
            opt.state[p] = {"step": torch.tensor(float(STEP - 1), device="cuda"), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
            out_old, out_new = outputs(shape, rowwise), outputs(shape, rowwise)
            w, m, v = w0.clone(), m0.clone(), v0.clone()

            def old():
                opt.step()
                dga.per_block_cast_to_fp8_transposed(p.data, rowwise=rowwise, out=out_old)

            new = lambda: dga.adamw_per_block_cast_to_fp8_transposed(w, m, v, grad, sc, rowwise=rowwise, out=out_new, **hyper)
            old()
            new()
            torch.cuda.synchronize()
            st = opt.state[p]
            # (four times the operator's own bound against float64, DESIGN.md "Optimizer": torch forms m' as a lerp, and where v is tiny
            # the rounding of m' is divided by a tiny den)
            lr_, bc1, bc2s, _ = sc.tolist()
            den = v.sqrt() / bc2s + EPS
            bar = 2.0 ** -22 * (5 * w0.abs() + (lr_ / bc1) * (4 * (BETAS[0] * m0.abs() + (1 - BETAS[0]) * grad.abs()) + 10 * m.abs()) / den)
            excess = ((w - p.data).abs() - bar).max().item()
            assert excess <= 0, f"{name}: w differs from torch's by {excess:.3e} beyond float32 rounding"
            del den, bar
            big_m = BETAS[0] * m0.abs() + (1 - BETAS[0]) * grad.abs()
            assert bool(((m - st["exp_avg"]).abs() <= 2.0 ** -22 * 3 * big_m).all()), f"{name}: m differs"
            assert bool(((v - st["exp_avg_sq"]).abs() <= 2.0 ** -22 * 5 * v).all()), f"{name}: v differs"
            del big_m
            want = dga.per_block_cast_to_fp8_transposed(w, rowwise=rowwise)
            flat = lambda o: (o[0] + o[1]) if rowwise else o
            for a, b in zip(flat(out_new), flat(want)):
                assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), f"{name}: the codes are not the quantiser's on the new w"
            del want
            t = alternate([new, old], args.windows)
            ratio = t[new].mean() / t[old].mean()
            tb = elems * (30 if rowwise else 29) / (t[new].mean() * 1e-6) / 1e12
            say(f"{name} fp32 m, v | new {fmt(t[new])} | old {fmt(t[old])} | new / old {ratio:5.2f} | {tb:4.2f} TB/s")
            if ratio >= 1.0:
                slower.append(" ".join(name.split()))
            del opt, p, st, out_old, m, v
            torch.cuda.empty_cache()
            mb, vb = m0.bfloat16(), v0.bfloat16()
            new16 = lambda: dga.adamw_per_block_cast_to_fp8_transposed(w, mb, vb, grad, sc, rowwise=rowwise, out=out_new, **hyper)
            t = alternate([new16], args.windows)
            tb = elems * (22 if rowwise else 21) / (t[new16].mean() * 1e-6) / 1e12
            say(f"{name} bf16 m, v | new {fmt(t[new16])} | {'':31s} | {'':16s} | {tb:4.2f} TB/s")
            del mb, vb, w, out_new
            torch.cuda.empty_cache()
        del w0, grad, m0, v0
        torch.cuda.empty_cache()
    say("# float32-moment cases not faster than the pair: " + ("; ".join(slower) if slower else "none"))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
