"""Times sparse_mla_bwd(deterministic=True) against the atomic path (deterministic=False), in the mould of scripts/sparse_mla_bwd_timing.py
and on its two prefill cases (M = 4096, S = 32768, causal, topk = 2048, Hq = 128 and 64): the two run alternately in one process on the
same tensors, in windows of back-to-back calls between two device events (each over 150 ms after a calibration, at least 3 calls), after a
warm-up; mean and min..max over the windows.  Before any time is reported dq is compared byte for byte, dkv to fp32 rounding of the sum
(2^-16 of the largest value: sums of a few thousand terms in two orders), and a second deterministic call from zeros must give the first
one's bytes.  dkv is added into and cleared between the comparison and the timing only.
Reported beside each time: ns per valid (token, key) pair -- the atomic path's 8.2 and mla_bwd_dense's 2.0 .. 2.4 are the yardsticks --,
the fraction of the 2.5 PFLOP/s bf16 matrix rate on 2 Hq valid (2 * 576 + 3 * 512) flops per token for the atomic path and with phase A
counted twice (2 * 576 + 2 * 512 more: both passes compute the scores and dP) for the deterministic one, and the staging bytes (valid x
2304, written once and read once).
The condition, set before the run: at Hq = 128 the deterministic path's slowest window is faster than the atomic path's fastest; Hq = 64
is recorded whichever way it falls.
--profile-calls N runs N deterministic calls of the Hq = 128 case and nothing else: the per-kernel times come from a separate
`rocprofv3 --kernel-trace --stats -- python scripts/sparse_mla_bwd_det_timing.py --profile-calls 2`.
Usage: python scripts/sparse_mla_bwd_det_timing.py [--out profiles/sparse_mla_bwd_det_timing.txt] [--windows N]"""
import argparse
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import deepgemm_ascend_amd as dga  # noqa: E402
from scripts.indexer_topk_timing import alternate  # noqa: E402
from scripts.sparse_mla_timing import D, DV, PEAK_FLOPS, SCALE, TOPK, prefill_case  # noqa: E402


def operands(m, s, h, gen):
    idx = prefill_case(m, s, gen)
    q = torch.randn((m, h, D), device="cuda", generator=gen).to(torch.bfloat16)
    kv = torch.randn((s, D), device="cuda", generator=gen).to(torch.bfloat16)
    d_out = torch.randn((m, h, DV), device="cuda", generator=gen).to(torch.bfloat16)
    out, lse = dga.sparse_mla_fwd(q, kv, idx, SCALE)
    return q, kv, out, d_out, idx, lse


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--profile-calls", type=int, default=0)
    args = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(1)
    if args.profile_calls:
        ops = operands(4096, 32768, 128, gen)
        dkv = torch.zeros((32768, D), dtype=torch.float32, device="cuda")
        for _ in range(args.profile_calls):
            dga.sparse_mla_bwd(*ops, SCALE, dkv=dkv, deterministic=True)
        torch.cuda.synchronize()
        return
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    fmt = lambda v: f"{v.mean():9.1f} [{v.min():9.1f}..{v.max():9.1f}] us"
    say(f"# {torch.cuda.get_device_name(0)}; topk = {TOPK}; det = sparse_mla_bwd(deterministic=True), atomic = sparse_mla_bwd(); device events "
        f"around windows of back-to-back calls (>= 150 ms each, at least 3 calls), {args.windows} windows per form, alternating; dq compared "
        f"byte for byte, dkv to 2^-16 of its largest value, two deterministic calls byte for byte; mean [min..max] us per call")
    say("# condition: max det < min atomic at Hq = 128; Hq = 64 recorded whichever way it falls")
    verdict = []
    for name, m, s, h in (("prefill M=4096 S=32768 Hq=128", 4096, 32768, 128), ("prefill M=4096 S=32768 Hq= 64", 4096, 32768, 64)):
        q, kv, out, d_out, idx, lse = operands(m, s, h, gen)
        dq, dkv = torch.empty_like(q), torch.zeros((s, D), dtype=torch.float32, device="cuda")
        dq_a, dkv_a = torch.empty_like(q), torch.zeros((s, D), dtype=torch.float32, device="cuda")
        det = lambda: dga.sparse_mla_bwd(q, kv, out, d_out, idx, lse, SCALE, dq=dq, dkv=dkv, deterministic=True)
        atomic = lambda: dga.sparse_mla_bwd(q, kv, out, d_out, idx, lse, SCALE, dq=dq_a, dkv=dkv_a)
        det()
        atomic()
        torch.cuda.synchronize()
        assert torch.equal(dq.view(torch.int16), dq_a.view(torch.int16)), name
        d_dkv = float((dkv - dkv_a).abs().max()) / float(dkv_a.abs().max())
        assert d_dkv <= 2.0 ** -16, (name, d_dkv)
        first = dkv.clone()
        dkv.zero_()
        det()
        torch.cuda.synchronize()
        assert torch.equal(first.view(torch.int32), dkv.view(torch.int32)), name
        del first
        dkv.zero_(), dkv_a.zero_()
        t = alternate([det, atomic], args.windows)
        valid = int((idx >= 0).sum())
        flops = 2.0 * h * valid * (2 * D + 3 * DV)
        us, us_a = t[det].mean(), t[atomic].mean()
        say(f"{name:32s} | det {fmt(t[det])} | atomic {fmt(t[atomic])} | atomic / det {us_a / us:6.2f} | ns per pair {us * 1e3 / valid:5.2f} vs "
            f"{us_a * 1e3 / valid:5.2f} | matrix {(flops + 2.0 * h * valid * (2 * D + 2 * DV)) / (us * 1e-6) / PEAK_FLOPS:6.3f} vs "
            f"{flops / (us_a * 1e-6) / PEAK_FLOPS:6.3f} of peak | staging {valid * D * 4 / 1e9:5.1f} GB written and read | dkv differs by {d_dkv:.1e}")
        verdict.append(f"{' '.join(name.split())}: slowest det {'<' if t[det].max() < t[atomic].min() else '>='} fastest atomic")
        del q, kv, idx, out, lse, d_out, dq, dkv, dq_a, dkv_a
        torch.cuda.empty_cache()
    say("# " + "; ".join(verdict))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
