"""Times mla_fwd_dense against what a user had before it, under the protocol of scripts/indexer_kl_dense_timing.py: old and new run
alternately in one process on the same tensors, in windows of back-to-back calls between two device events (each over 150 ms after a
calibration, at least 3 calls), after a warm-up; mean and min..max over the windows.  Before any time is reported the results are
compared: out to 2^-5 of its largest value, lse to 2^-5 (the old path's matmul rounds the scores to bf16).
M = 4096, ks = 0, ke = N - M + m + 1, N = S in {8192, 32768}, Hq in {128, 64, 16}, bf16 normal q and kv, sm_scale = 576^-0.5.
  new     mla_fwd_dense(q, kv, ks, ke, sm_scale, out=..., lse=...): one launch, workgroups in descending order of their rows
  linear  the same with DGA_MLA_DENSE_LINEAR_GRID (ascending order)
  old     per chunk of tokens small enough to fit: matmul of q with kv^T ([chunk, Hq, N] fp32), -inf outside the ranges, logsumexp and
          exp(s - lse) in fp32 (the softmax, and the lse the new path returns), the weights in bf16 times kv[:, :512]
Reported beside each time: the fraction of the 2.5 PFLOP/s bf16 matrix rate that 2 Hq (576 + 512) flops per in-range pair amount to, and
the time per (token, key) pair beside sparse_mla_fwd's at the same Hq, taken from profiles/sparse_mla_timing.txt (M 2048 pairs a call).
The condition, set before the run: at every case the slowest new window is faster than the fastest old one (max new < min old).
Usage: python scripts/mla_dense_timing.py [--out profiles/mla_dense_timing.txt] [--windows N]"""
import argparse
import re
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import deepgemm_ascend_amd as dga  # noqa: E402
from scripts.indexer_topk_timing import alternate  # noqa: E402
from scripts.sparse_mla_timing import D, DV, PEAK_FLOPS, SCALE, TOPK  # noqa: E402

M = 4096


def old_form(q, kv, ks, ke, out, lse, chunk):
    n, h = kv.shape[0], q.shape[1]
    col = torch.arange(n, device=q.device, dtype=torch.int32)
    for lo in range(0, q.shape[0], chunk):
        sl = slice(lo, lo + chunk)
        outside = (col < ks[sl, None]) | (col >= ke[sl, None])
        s = torch.matmul(q[sl].reshape(-1, D), kv.t()).view(-1, h, n).float().mul_(SCALE).masked_fill_(outside[:, None, :], float("-inf"))
        lse[sl] = torch.logsumexp(s, dim=2)
        p = s.sub_(lse[sl, :, None]).exp_().to(torch.bfloat16)
        out[sl] = torch.matmul(p.view(-1, n), kv[:, :DV]).view(-1, h, DV)
    return out, lse


def sparse_ns_per_pair():
    """sparse_mla_fwd's time per (token, selected key) pair at its prefill cases, by Hq, from its timing file"""
    text = (ROOT / "profiles" / "sparse_mla_timing.txt").read_text()
    return {int(h): float(us) * 1e3 / (int(m) * TOPK) for m, h, us in re.findall(r"^prefill M=(\d+) S=\d+ Hq=\s*(\d+)\s*\| new\s+([0-9.]+)", text, flags=re.M)}


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
    sparse = sparse_ns_per_pair()
    say(f"# {torch.cuda.get_device_name(0)}; M = {M}, ks = 0, ke = N - M + m + 1; new = mla_fwd_dense(out=..., lse=...), linear = the same in "
        f"ascending grid order, old = matmul, -inf fill, fp32 logsumexp and exp, matmul in token chunks; device events around windows of "
        f"back-to-back calls (>= 150 ms each, at least 3 calls), {args.windows} windows per form, alternating; results compared first; "
        f"mean [min..max] us per call")
    say("# matrix: fraction of 2.5 PFLOP/s on 2 Hq (576 + 512) flops per in-range pair; ns per pair beside sparse_mla_fwd's "
        + ", ".join(f"{v:.3f} at Hq = {h}" for h, v in sorted(sparse.items())) + "; condition: max new < min old at every case")
    gen = torch.Generator(device="cuda").manual_seed(1)
    failed = []
    for n in (8192, 32768):
        tok = torch.arange(M, device="cuda", dtype=torch.int32)
        ks, ke = torch.zeros_like(tok), n - M + tok + 1
        pairs = int(ke.sum())
        for h in (128, 64, 16):
            q = torch.randn((M, h, D), device="cuda", generator=gen).to(torch.bfloat16)
            kv = torch.randn((n, D), device="cuda", generator=gen).to(torch.bfloat16)
            outs = [(torch.empty((M, h, DV), device="cuda", dtype=torch.bfloat16), torch.empty((M, h), device="cuda")) for _ in range(2)]
            new = lambda: dga.mla_fwd_dense(q, kv, ks, ke, SCALE, out=outs[0][0], lse=outs[0][1])
            linear = lambda: dga.mla_fwd_dense(q, kv, ks, ke, SCALE, out=outs[0][0], lse=outs[0][1], _flags=1)
            old = lambda: old_form(q, kv, ks, ke, *outs[1], max(1, (1 << 22) // (h * n) * 8))
            new(), old()
            torch.cuda.synchronize()
            diff = (float((outs[0][0].float() - outs[1][0].float()).abs().max()) / float(outs[1][0].float().abs().max()),
                    float((outs[0][1] - outs[1][1]).abs().max()))
            assert max(diff) <= 2.0 ** -5, (h, n, diff)
            tm = alternate([new, old, linear], args.windows)
            us, name = tm[new].mean(), f"Hq = {h:3d}, N = {n}"
            say(f"{name:20s} | new {fmt(tm[new])} | old {fmt(tm[old])} | old / new {tm[old].mean() / us:7.2f} | out differs by {diff[0]:.1e} of the "
                f"largest value, lse by {diff[1]:.1e} | matrix {2.0 * h * pairs * (D + DV) / (us * 1e-6) / PEAK_FLOPS:6.3f} of peak, "
                f"{us * 1e3 / pairs:6.3f} ns per pair | linear {fmt(tm[linear])}, {tm[linear].mean() / us:5.2f} x")
            if not tm[new].max() < tm[old].min():
                failed.append(name)
            del q, kv, outs
            torch.cuda.empty_cache()
    say("# cases where new is not faster than old beyond the spread: " + ("; ".join(failed) if failed else "none"))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
