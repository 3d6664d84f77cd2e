"""Times fp8_mqa_logits against the torch expression it replaces.  Both forms run alternately in one process on the same tensors, in windows
of back-to-back calls between two device events (each window sized to over 100 ms after a calibration, at least 3 calls), after a warm-up;
mean and min..max over the windows.  Before any time is reported the results are compared: -inf in the same places, the values to the bf16
rounding of the baseline's scores.
H = 64, fp8 operands (per_token_cast_to_fp8 of normal samples), float32 weights.  Cases:
  causal 4096 x 4096       ks = 0, ke = m + 1
  full   4096 x 4096       ks = 0, ke = N
  causal 4096 x 32768      ks = 0, ke = N - M + m + 1
  full    128 x 65536      ks = 0, ke = N
  new      fp8_mqa_logits(q, (k, kscale), weights, ks, ke, out=...)
  torch    k.bfloat16(); per chunk of 512 tokens (the [H, M, N] temporary of the whole call does not fit at the larger cases; every case is
           chunked the same way): einsum('mhd,nd->hmn') in bf16, relu, * weights in float32, sum over h, * kscale, masked_fill(-inf)
TFLOP/s: 2 * 128 * H flops per (token, key) pair inside the ranges over the new form's mean time, beside mfma_ceiling('bf16_exact'), the
register-resident figure of the same arithmetic.  The causal 4096 x 4096 case's time is also given as a share of the full one's.
The condition: the fused call is not slower than the torch expression on any case (new / torch <= 1.0); no ratio is fixed in advance.
Usage: python scripts/mqa_logits_timing.py [--out profiles/mqa_logits_timing.txt] [--windows N]"""
import argparse
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import deepgemm_ascend_amd as dga  # noqa: E402
from scripts.cast_transposed_timing import window_ms  # noqa: E402

H, D, CHUNK = 64, 128, 512
CASES = (("causal", 4096, 4096), ("full", 4096, 4096), ("causal", 4096, 32768), ("full", 128, 65536))


def alternate(fns, windows):
    """{fn: us per call, one entry per window}: warm-up and a calibration window each, then `windows` rounds over all of them in turn."""
    calls = {}
    for fn in fns:
        window_ms(fn, 2)
        calls[fn] = max(3, int(120.0 / (window_ms(fn, 3) / 3)) + 1)
    t = {fn: [] for fn in fns}
    for _ in range(windows):
        for fn in fns:
            t[fn].append(window_ms(fn, calls[fn]) * 1e3 / calls[fn])
    return {fn: np.array(v) for fn, v in t.items()}


def torch_form(q, k, kscale, weights, ks, ke, out):
    m, n = out.shape
    kf = k.to(torch.bfloat16)
    col = torch.arange(n, device=q.device, dtype=torch.int32)[None, :]
    for c in range(0, m, CHUNK):
        s = torch.einsum("mhd,nd->hmn", q[c:c + CHUNK].to(torch.bfloat16), kf).relu_()
        logits = (s * weights[c:c + CHUNK].t()[:, :, None]).sum(dim=0) * kscale[None, :]
        mask = (col >= ks[c:c + CHUNK, None]) & (col < ke[c:c + CHUNK, None])
        out[c:c + CHUNK] = logits.masked_fill_(~mask, float("-inf"))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=3)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    fmt = lambda v: f"{v.mean():9.1f} [{v.min():9.1f}..{v.max():9.1f}] us"
    ceiling = dga.mfma_ceiling("bf16_exact")
    say(f"# {torch.cuda.get_device_name(0)}; H = {H}, fp8 operands; new = fp8_mqa_logits(out=...), torch = bf16 einsum('mhd,nd->hmn'), relu, weight, "
        f"sum over h, scale, mask, in chunks of {CHUNK} tokens at every case; device events around windows of back-to-back calls (>= 100 ms "
        f"each, at least 3 calls), {args.windows} windows per form, alternating; mean [min..max] us per call")
    say(f"# TFLOP/s: 2 * 128 * H flops per in-range (token, key) pair over the new form's mean; mfma_ceiling('bf16_exact') = {ceiling:.0f} TFLOP/s "
        f"(operands in registers, same arithmetic); condition: new / torch <= 1.00 at every case")
    slower, means = [], {}
    for kind, m, n in CASES:
        g = torch.Generator(device="cuda").manual_seed(m + n)
        q, _ = dga.per_token_cast_to_fp8(torch.randn((m * H, D), device="cuda", generator=g))
        q = q.view(m, H, D)
        k, sfk = dga.per_token_cast_to_fp8(torch.randn((n, D), device="cuda", generator=g))
        kscale = sfk.reshape(n).contiguous()
        weights = torch.randn((m, H), device="cuda", generator=g)
        i = torch.arange(m, device="cuda", dtype=torch.int32)
        ks = torch.zeros_like(i)
        ke = (n - m + i + 1) if kind == "causal" else torch.full_like(i, n)
        out_new, out_old = torch.empty((m, n), device="cuda"), torch.empty((m, n), device="cuda")
        new = lambda: dga.fp8_mqa_logits(q, (k, kscale), weights, ks, ke, out=out_new)
        old = lambda: torch_form(q, k, kscale, weights, ks, ke, out_old)
        name = f"{kind:6s} {m:5d} x {n:5d}"
        new(), old()
        torch.cuda.synchronize()
        assert torch.equal(torch.isneginf(out_new), torch.isneginf(out_old)), f"{name}: -inf in other places"
        inside = ~torch.isneginf(out_new)
        diff = (out_new[inside] - out_old[inside]).abs().max().item()
        assert diff <= 2.0 ** -6 * out_old[inside].abs().max().item(), f"{name}: values differ by {diff}"
        t = alternate([new, old], args.windows)
        ratio = t[new].mean() / t[old].mean()
        pairs = int((ke - ks).clamp(min=0).sum().item())
        tf = 2.0 * D * H * pairs / (t[new].mean() * 1e-6) / 1e12
        means[(kind, m, n)] = t[new].mean()
        say(f"{name} | new {fmt(t[new])} | torch {fmt(t[old])} | new / torch {ratio:5.3f} | {tf:6.1f} TFLOP/s = {100 * tf / ceiling:4.1f} % of the ceiling")
        if ratio > 1.0:
            slower.append(" ".join(name.split()))
        del q, k, kscale, weights, out_new, out_old, inside
        torch.cuda.empty_cache()
    share = means[("causal", 4096, 4096)] / means[("full", 4096, 4096)]
    say(f"# causal 4096 x 4096 takes {100 * share:.1f} % of the full range's time")
    say("# cases slower than the torch expression: " + ("; ".join(slower) if slower else "none"))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
