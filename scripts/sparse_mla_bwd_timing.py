"""Times sparse_mla_bwd against what a user had before it, in the mould of scripts/sparse_mla_timing.py: old and new run alternately in
one process on the same tensors, in windows of back-to-back calls between two device events (each over 150 ms after a calibration, at
least 3 calls), after a warm-up; mean and min..max over the windows.  Before any time is reported the results are compared: dq and dkv
each to 2^-5 of its largest value -- the old path's bmm rounds the scores, dP and its two dkv products to bf16 (2^-9 each of values of a
few units, the first of them in the exponent of p), and the two paths sum in different orders; 2^-5 is the forward script's bar for the
same roundings.
topk = 2048, bf16 normal samples, sm_scale = 576^-0.5; out and lse are sparse_mla_fwd's.  Cases: the prefill cases of that script,
M = 4096, S = 32768, causal, Hq = 128 and 64 (scripts/sparse_mla_timing.py prefill_case).
  new   sparse_mla_bwd(q, kv, out, d_out, indices, lse, sm_scale, dq=..., dkv=...) -- dkv is added into, as in a training step, and cleared
        between the comparison and the timing only
  old   per chunk of tokens small enough to fit: index_select of the rows ([chunk, 2048, 576]), bmm with q, p = exp(s - lse) (0 at
        invalid positions), delta, bmm of d_out with the first 512 columns, dS, bmm for dq, two bmm for the chunk's [chunk, 2048, 576] rows
        of dkv, index_add_ in fp32
Reported beside each time: the fraction of the 2.5 PFLOP/s bf16 matrix rate on 2 Hq valid (2 * 576 + 3 * 512) flops per token, and the
bytes added atomically per second -- valid x 2304 bytes per token and block of 32 heads, the unit that adds.
The condition, set before the run: new < old at every case, by more than the windows' spread (max new < min old).
Usage: python scripts/sparse_mla_bwd_timing.py [--out profiles/sparse_mla_bwd_timing.txt] [--windows N]"""
import argparse
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import deepgemm_ascend_amd as dga  # noqa: E402
from scripts.indexer_topk_timing import alternate  # noqa: E402
from scripts.sparse_mla_timing import D, DV, PEAK_FLOPS, SCALE, TOPK, prefill_case  # noqa: E402


def old_form(q, kv, out, d_out, idx, lse, dq, dkv, chunk):
    s_rows = kv.shape[0]
    for lo in range(0, q.shape[0], chunk):
        sl = slice(lo, lo + chunk)
        i = idx[sl].long()
        valid = (i >= 0) & (i < s_rows)
        rows = i.clamp(0, s_rows - 1).flatten()
        g = kv.index_select(0, rows).view(i.shape[0], TOPK, D)
        p = torch.bmm(q[sl], g.transpose(1, 2)).float().mul_(SCALE).sub_(lse[sl, :, None]).exp_().masked_fill_(~valid[:, None, :], 0.0)
        delta = (out[sl].float() * d_out[sl].float()).sum(-1, keepdim=True)
        ds = torch.bmm(d_out[sl], g[:, :, :DV].transpose(1, 2)).float().sub_(delta).mul_(p).mul_(SCALE).to(torch.bfloat16)
        dq[sl] = torch.bmm(ds, g)
        dg = torch.bmm(ds.transpose(1, 2), q[sl]).float()
        dg[:, :, :DV] += torch.bmm(p.to(torch.bfloat16).transpose(1, 2), d_out[sl])
        dkv.index_add_(0, rows, dg.masked_fill_(~valid[:, :, None], 0.0).view(-1, D))
    return dq, dkv


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
    say(f"# {torch.cuda.get_device_name(0)}; topk = {TOPK}; new = sparse_mla_bwd(dq=..., dkv=...), old = index_select, bmm, exp(s - lse), "
        f"delta, bmm, dS, three bmm, index_add_ in token chunks; device events around windows of back-to-back calls (>= 150 ms each, at "
        f"least 3 calls), {args.windows} windows per form, alternating; results compared first; mean [min..max] us per call")
    say("# matrix: fraction of 2.5 PFLOP/s on 2 Hq valid (2 * 576 + 3 * 512) flops per token; atomics: valid x 2304 B per token and 32-head "
        "block; condition: max new < min old at every case")
    gen = torch.Generator(device="cuda").manual_seed(1)
    failed = []
    for name, m, s, h, chunk in (("prefill M=4096 S=32768 Hq=128", 4096, 32768, 128, 32), ("prefill M=4096 S=32768 Hq= 64", 4096, 32768, 64, 64)):
        idx = prefill_case(m, s, gen)
        q = torch.randn((m, h, D), device="cuda", generator=gen).to(torch.bfloat16)
        kv = torch.randn((s, D), device="cuda", generator=gen).to(torch.bfloat16)
        d_out = torch.randn((m, h, DV), device="cuda", generator=gen).to(torch.bfloat16)
        out, lse = dga.sparse_mla_fwd(q, kv, idx, SCALE)
        dq, dkv = torch.empty_like(q), torch.zeros((s, D), dtype=torch.float32, device="cuda")
        dq_old, dkv_old = torch.empty_like(q), torch.zeros((s, D), dtype=torch.float32, device="cuda")
        new = lambda: dga.sparse_mla_bwd(q, kv, out, d_out, idx, lse, SCALE, dq=dq, dkv=dkv)
        old = lambda: old_form(q, kv, out, d_out, idx, lse, dq_old, dkv_old, chunk)
        new()
        old()
        torch.cuda.synchronize()
        d_dq = float((dq.float() - dq_old.float()).abs().max()) / float(dq_old.float().abs().max())
        d_dkv = float((dkv - dkv_old).abs().max()) / float(dkv_old.abs().max())
        assert d_dq <= 2.0 ** -5 and d_dkv <= 2.0 ** -5, (name, d_dq, d_dkv)
        dkv.zero_(), dkv_old.zero_()
        t = alternate([new, old], args.windows)
        valid = int((idx >= 0).sum())
        flops = 2.0 * h * valid * (2 * D + 3 * DV)
        nbytes = valid * D * 4 * ((h + 31) // 32)
        us = t[new].mean()
        say(f"{name:32s} | new {fmt(t[new])} | old {fmt(t[old])} | old / new {t[old].mean() / us:7.2f} | dq differs by {d_dq:.1e}, dkv by "
            f"{d_dkv:.1e} of the largest value | matrix {flops / (us * 1e-6) / PEAK_FLOPS:6.3f} of peak | atomics {nbytes / (us * 1e-6) / 1e12:6.2f} TB/s")
        if not t[new].max() < t[old].min():
            failed.append(" ".join(name.split()))
        del q, kv, idx, out, lse, d_out, dq, dkv, dq_old, dkv_old
        torch.cuda.empty_cache()
    say("# cases where new is not faster than old beyond the spread: " + ("; ".join(failed) if failed else "none"))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
