"""Times fp8_mqa_logits_bwd_dense against the only HIP path to the same gradients before it -- fp8_mqa_logits_bwd with the ranges written out
as [M, N] lists -- by the protocol of scripts/mqa_logits_bwd_timing.py: old, new and the forward run alternately in one process on the same
tensors, in windows of back-to-back calls between two device events (each over 150 ms after a calibration, at least 3 calls), after a
warm-up; mean and min..max over the windows.  Before any time is reported the results are compared: dq, dk and d_weights each against the
old path to 2^-5 of its largest value (the two paths round alike and sum in another order; 2^-5 is that script's bar).
Cases: M = 4096 tokens, ke = N - M + m + 1 (causal), per-token amax-quantised normal q and k, normal weights and d_logits; H = 64 and
H = 32; N = 8192 and N = 32768.
  new   fp8_mqa_logits_bwd_dense(q, (k, kscale), weights, d_logits, ks, ke, dq=..., dk=..., d_weights=...) -- dk is added into
  old   fp8_mqa_logits_bwd(q, (k, kscale), weights, lists, d_logits, ...) with lists[m, n] = n inside the range, -1 outside: int32 [M, N]
  fwd   fp8_mqa_logits on the same case
Reported beside each time: new / fwd, and the fraction of the 2.5 PFLOP/s bf16 matrix rate on 3 * 2 * H * 128 flops per in-range
(token, key) pair -- the scores both passes recompute and the residual terms count as nothing.
The condition, set before the run: at every case the slowest new window is faster than the fastest old window.
Usage: python scripts/mqa_logits_bwd_dense_timing.py [--out profiles/mqa_logits_bwd_dense_timing.txt] [--windows N]"""
import argparse
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import deepgemm_ascend_amd as dga  # noqa: E402
from scripts.indexer_topk_timing import alternate  # noqa: E402
from scripts.sparse_mla_timing import PEAK_FLOPS  # noqa: E402

M, D = 4096, 128
CASES = ((64, 8192), (32, 8192), (64, 32768), (32, 32768))


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
    say(f"# {torch.cuda.get_device_name(0)}; M = {M}, ke = N - M + m + 1; new = fp8_mqa_logits_bwd_dense(dq=..., dk=..., d_weights=...), old = "
        f"fp8_mqa_logits_bwd over int32 [M, N] lists of the ranges, fwd = fp8_mqa_logits(out=...); device events around windows of back-to-back "
        f"calls (>= 150 ms each, at least 3 calls), {args.windows} windows per form, alternating; results compared first; mean [min..max] us per call")
    say("# matrix: fraction of 2.5 PFLOP/s on 3 * 2 * H * 128 flops per in-range pair; condition: max new < min old at every case")
    failed = []
    for h, n in CASES:
        gen = torch.Generator(device="cuda").manual_seed(h + n)
        q, _ = dga.per_token_cast_to_fp8(torch.randn((M * h, D), device="cuda", generator=gen))
        q = q.view(M, h, D)
        k, sfk = dga.per_token_cast_to_fp8(torch.randn((n, D), device="cuda", generator=gen))
        kscale = sfk.reshape(n).contiguous()
        weights = torch.randn((M, h), device="cuda", generator=gen)
        t = torch.arange(M, device="cuda", dtype=torch.int32)
        ks, ke = torch.zeros_like(t), n - M + t + 1
        dl = torch.randn((M, n), device="cuda", generator=gen)
        col = torch.arange(n, device="cuda", dtype=torch.int32)[None, :]
        lists = torch.where(col < ke[:, None], col, -1).to(torch.int32).contiguous()
        logits = torch.empty((M, n), device="cuda")
        outs = [(torch.empty((M, h, D), device="cuda"), torch.zeros((n, D), device="cuda"), torch.empty((M, h), device="cuda")) for _ in range(2)]
        new = lambda: dga.fp8_mqa_logits_bwd_dense(q, (k, kscale), weights, dl, ks, ke, dq=outs[0][0], dk=outs[0][1], d_weights=outs[0][2])
        old = lambda: dga.fp8_mqa_logits_bwd(q, (k, kscale), weights, lists, dl, dq=outs[1][0], dk=outs[1][1], d_weights=outs[1][2])
        fwd = lambda: dga.fp8_mqa_logits(q, (k, kscale), weights, ks, ke, out=logits)
        new(), old(), fwd()
        torch.cuda.synchronize()
        diff = [float((a - b).abs().max()) / float(b.abs().max()) for a, b in zip(*outs)]
        assert max(diff) <= 2.0 ** -5, (h, n, diff)
        tm = alternate([new, old, fwd], args.windows)
        pairs = int(ke.sum())
        us = tm[new].mean()
        name = f"H = {h}, N = {n}"
        say(f"{name:18s} | new {fmt(tm[new])} | old {fmt(tm[old])} | old / new {tm[old].mean() / us:7.2f} | fwd {fmt(tm[fwd])} | new / fwd "
            f"{us / tm[fwd].mean():6.2f} | dq, dk, d_weights differ by {diff[0]:.1e}, {diff[1]:.1e}, {diff[2]:.1e} of the largest value | matrix "
            f"{6.0 * h * D * pairs / (us * 1e-6) / PEAK_FLOPS:6.3f} of peak")
        if not tm[new].max() < tm[old].min():
            failed.append(name)
        del q, k, dl, lists, logits, outs
        torch.cuda.empty_cache()
    say("# cases where new is not faster than old beyond the spread: " + ("; ".join(failed) if failed else "none"))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
