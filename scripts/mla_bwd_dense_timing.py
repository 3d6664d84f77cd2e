"""Times mla_bwd_dense against what a user had before it, under the protocol of scripts/mla_dense_timing.py: old and new run alternately in
one process on the same tensors, in windows of back-to-back calls between two device events (each over 150 ms after a calibration, at
least 3 calls), after a warm-up; mean and min..max over the windows.  Before any time is reported the results are compared onto zeroed
dkv: dq and dkv to 2^-5 of their largest value (the old path's matmuls round their results to bf16).
M = 4096, ks = 0, ke = N - M + m + 1, N = S in {8192, 32768}, Hq in {128, 64, 16}, bf16 normal q, kv and d_out, out and lse from
mla_fwd_dense, sm_scale = 576^-0.5.
  new     mla_bwd_dense(q, kv, out, d_out, ks, ke, lse, sm_scale, dq=..., dkv=...): three launches
  old     per chunk of tokens small enough to fit: matmul of q with kv^T into fp32 [chunk, Hq, N], exp(s - lse) with 0 outside the ranges,
          delta, matmul of d_out with kv[:, :512]^T, dS, then three matmuls (dS kv, dS^T q, p^T d_out) with dkv accumulated in fp32
Reported beside each time: the fraction of the 2.5 PFLOP/s bf16 matrix rate that 2 Hq (2 576 + 3 512) flops per in-range pair amount to,
the time per (token, key) pair beside sparse_mla_bwd's (profiles/sparse_mla_bwd_timing.txt) and mla_fwd_dense's (profiles/
mla_dense_timing.txt) at the same Hq, and each launch's share of one profiled call.
The condition, set before the run: at every case the slowest new window is faster than the fastest old one (max new < min old).
Usage: python scripts/mla_bwd_dense_timing.py [--out profiles/mla_bwd_dense_timing.txt] [--windows N]"""
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


def old_form(q, kv, out, d_out, ks, ke, lse, dq, dkv, chunk):
    n, h = kv.shape[0], q.shape[1]
    col = torch.arange(n, device=q.device, dtype=torch.int32)
    for lo in range(0, q.shape[0], chunk):
        sl = slice(lo, lo + chunk)
        outside = ((col < ks[sl, None]) | (col >= ke[sl, None]))[:, None, :]
        q2, do2 = q[sl].reshape(-1, D), d_out[sl].reshape(-1, DV)
        p = torch.matmul(q2, kv.t()).view(-1, h, n).float().mul_(SCALE).sub_(lse[sl, :, None]).exp_().masked_fill_(outside, 0.0)
        delta = (out[sl].float() * d_out[sl].float()).sum(2, keepdim=True)
        ds = torch.matmul(do2, kv[:, :DV].t()).view(-1, h, n).float().sub_(delta).mul_(p).mul_(SCALE).to(torch.bfloat16).view(-1, n)
        pb = p.to(torch.bfloat16).view(-1, n)
        dq[sl] = torch.matmul(ds, kv).view(-1, h, D)
        dkv += torch.matmul(ds.t(), q2)
        dkv[:, :DV] += torch.matmul(pb.t(), do2)
    return dq, dkv


def ns_per_pair(name, pattern, pairs_of):
    """a neighbour's time per (token, key) pair by Hq, from its timing file (empty when the file or the line is not there)"""
    path = ROOT / "profiles" / name
    found = re.findall(pattern, path.read_text(), flags=re.M) if path.exists() else []
    return {int(h): float(us) * 1e3 / pairs_of(*map(int, rest)) for *rest, h, us in found}


def launch_shares(fn):
    """each kernel's share of the device time of one profiled call, or None where the profiler gives no device times"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        t = {}
        for e in prof.key_averages():
            us = getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0)
            for k in ("mdb_row_kernel", "mdb_key_kernel", "mdb_reduce_kernel"):
                if k in e.key:
                    t[k] = t.get(k, 0.0) + us
        total = sum(t.values())
        return {k: v / total for k, v in t.items()} if total > 0 and len(t) == 3 else None
    except Exception:  # noqa: BLE001  (a report without the shares is still a report)
        return None


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
    sparse = ns_per_pair("sparse_mla_bwd_timing.txt", r"^prefill M=(\d+) S=\d+ Hq=\s*(\d+)\s*\| new\s+([0-9.]+)", lambda m: m * TOPK)
    say(f"# {torch.cuda.get_device_name(0)}; M = {M}, ks = 0, ke = N - M + m + 1; new = mla_bwd_dense(dq=..., dkv=...), old = matmul, fp32 "
        f"exp(s - lse), delta, matmul, dS, three matmuls in token chunks, dkv accumulated; device events around windows of back-to-back calls "
        f"(>= 150 ms each, at least 3 calls), {args.windows} windows per form, alternating; results compared first; mean [min..max] us per call")
    say("# matrix: fraction of 2.5 PFLOP/s on 2 Hq (2 576 + 3 512) flops per in-range pair; ns per pair beside sparse_mla_bwd's "
        + ", ".join(f"{v:.3f} at Hq = {h}" for h, v in sorted(sparse.items())) + " and mla_fwd_dense's 0.39 .. 0.41; condition: max new < min old at every case")
    gen = torch.Generator(device="cuda").manual_seed(1)
    failed = []
    for n in (8192, 32768):
        tok = torch.arange(M, device="cuda", dtype=torch.int32)
        ks, ke = torch.zeros_like(tok), n - M + tok + 1
        pairs = int(ke.sum())
        for h in (128, 64, 16):
            q = torch.randn((M, h, D), device="cuda", generator=gen).to(torch.bfloat16)
            kv = torch.randn((n, D), device="cuda", generator=gen).to(torch.bfloat16)
            d_out = torch.randn((M, h, DV), device="cuda", generator=gen).to(torch.bfloat16)
            out, lse = dga.mla_fwd_dense(q, kv, ks, ke, SCALE)
            outs = [(torch.empty((M, h, D), device="cuda", dtype=torch.bfloat16), torch.zeros((n, D), device="cuda")) for _ in range(2)]
            new = lambda: dga.mla_bwd_dense(q, kv, out, d_out, ks, ke, lse, SCALE, dq=outs[0][0], dkv=outs[0][1])
            old = lambda: old_form(q, kv, out, d_out, ks, ke, lse, *outs[1], max(1, (1 << 22) // (h * n) * 8))
            new(), old()
            torch.cuda.synchronize()
            diff = [float((a.float() - b.float()).abs().max()) / float(b.float().abs().max()) for a, b in zip(*outs)]
            assert max(diff) <= 2.0 ** -5, (h, n, diff)
            share = launch_shares(new)
            tm = alternate([new, old], args.windows)
            us, name = tm[new].mean(), f"Hq = {h:3d}, N = {n}"
            say(f"{name:20s} | new {fmt(tm[new])} | old {fmt(tm[old])} | old / new {tm[old].mean() / us:7.2f} | dq differs by {diff[0]:.1e}, dkv by "
                f"{diff[1]:.1e} of the largest value | matrix {2.0 * h * pairs * (2 * D + 3 * DV) / (us * 1e-6) / PEAK_FLOPS:6.3f} of peak, "
                f"{us * 1e3 / pairs:6.3f} ns per pair | shares: "
                + ("not measured" if share is None else ", ".join(f"{k[4:-7]} {share[k]:.3f}" for k in ("mdb_row_kernel", "mdb_key_kernel", "mdb_reduce_kernel"))))
            if not tm[new].max() < tm[old].min():
                failed.append(name)
            del q, kv, d_out, out, lse, outs
            torch.cuda.empty_cache()
    say("# cases where new is not faster than old beyond the spread: " + ("; ".join(failed) if failed else "none"))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
