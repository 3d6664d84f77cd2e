"""Times fp8_mqa_logits_bwd against what a user had before it, in the mould of scripts/sparse_mla_bwd_timing.py: old and new run alternately
in one process on the same tensors, in windows of back-to-back calls between two device events (each over 150 ms after a calibration, at
least 3 calls), after a warm-up; mean and min..max over the windows.  Before any time is reported the results are compared: dq, dk and
d_weights each against the old path to 2^-5 of its largest value -- the old path's einsums round the scores and the two weights to bf16
and sum in another order; 2^-5 is that script's bar for the same roundings.
Case: M = 4096 tokens over N = 32768 keys, causal ranges, per-token amax-quantised normal q and k, normal weights and d_logits;
topk = 2048 from indexer_topk on fp8_mqa_logits' logits; H = 64 and H = 32.
  new   fp8_mqa_logits_bwd(q, (k, kscale), weights, indices, d_logits, dq=..., dk=..., d_weights=...) -- dk is added into, as in a training
        step, and cleared between the comparison and the timing only
  old   per chunk of tokens: index_select of the rows (their codes as bf16, converted once outside the timing), bf16 einsum for the scores
        ([chunk, H, 2048] in fp32), relu, the three derivative products, index_add_ in fp32
Reported beside each time: the fraction of the 2.5 PFLOP/s bf16 matrix rate on 3 * 2 * H * 128 flops per valid position, and the bytes
added atomically per second -- valid x 512 bytes per token.
The condition, set before the run: new < old at both cases, by more than the windows' spread (max new < min old).
Usage: python scripts/mqa_logits_bwd_timing.py [--out profiles/mqa_logits_bwd_timing.txt] [--windows N]"""
import argparse
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import deepgemm_ascend_amd as dga  # noqa: E402
from scripts.indexer_topk_timing import alternate  # noqa: E402
from scripts.sparse_mla_timing import PEAK_FLOPS  # noqa: E402

M, N, D, TOPK = 4096, 32768, 128, 2048


def old_form(qb, kb, kscale, weights, idx, dl, dq, dk, dw, chunk):
    n = kb.shape[0]
    for lo in range(0, qb.shape[0], chunk):
        sl = slice(lo, lo + chunk)
        i = idx[sl].long()
        valid = (i >= 0) & (i < n)
        rows = i.clamp(0, n - 1).flatten()
        g = kb.index_select(0, rows).view(i.shape[0], TOPK, D)
        sc = kscale.index_select(0, rows).view(i.shape[0], TOPK)
        d = dl[sl].masked_fill(~valid, 0.0)
        s = torch.einsum("chd,ctd->cht", qb[sl], g).float()
        dw[sl] = (torch.relu(s) * (d * sc)[:, None, :]).sum(-1)
        gk = (weights[sl][:, :, None] * d[:, None, :]).masked_fill_(~(s > 0), 0.0)
        dq[sl] = torch.einsum("cht,ctd->chd", (gk * sc[:, None, :]).to(torch.bfloat16), g)
        dk.index_add_(0, rows, torch.einsum("cht,chd->ctd", gk.to(torch.bfloat16), qb[sl]).float().view(-1, D))
    return dq, dk, dw


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
    say(f"# {torch.cuda.get_device_name(0)}; M = {M}, N = {N}, causal, topk = {TOPK}; new = fp8_mqa_logits_bwd(dq=..., dk=..., d_weights=...), old = "
        f"index_select, bf16 einsum, relu, three derivative products, index_add_ in token chunks; device events around windows of back-to-back "
        f"calls (>= 150 ms each, at least 3 calls), {args.windows} windows per form, alternating; results compared first; mean [min..max] us per call")
    say("# matrix: fraction of 2.5 PFLOP/s on 3 * 2 * H * 128 flops per valid position; atomics: valid x 512 B per token; condition: max new < "
        "min old at both cases")
    failed = []
    for h, chunk in ((64, 64), (32, 128)):
        gen = torch.Generator(device="cuda").manual_seed(h)
        q, _ = dga.per_token_cast_to_fp8(torch.randn((M * h, D), device="cuda", generator=gen))
        q = q.view(M, h, D)
        k, sfk = dga.per_token_cast_to_fp8(torch.randn((N, D), device="cuda", generator=gen))
        kscale = sfk.reshape(N).contiguous()
        weights = torch.randn((M, h), device="cuda", generator=gen)
        t = torch.arange(M, device="cuda", dtype=torch.int32)
        ks, ke = torch.zeros_like(t), N - M + t + 1
        idx = dga.indexer_topk(dga.fp8_mqa_logits(q, (k, kscale), weights, ks, ke), TOPK, row_starts=ks, row_ends=ke)
        dl = torch.randn((M, TOPK), device="cuda", generator=gen)
        qb, kb = q.to(torch.bfloat16), k.to(torch.bfloat16)
        outs = [(torch.empty((M, h, D), device="cuda"), torch.zeros((N, D), device="cuda"), torch.empty((M, h), device="cuda")) for _ in range(2)]
        new = lambda: dga.fp8_mqa_logits_bwd(q, (k, kscale), weights, idx, dl, dq=outs[0][0], dk=outs[0][1], d_weights=outs[0][2])
        old = lambda: old_form(qb, kb, kscale, weights, idx, dl, *outs[1], chunk)
        new(), old()
        torch.cuda.synchronize()
        diff = [float((a - b).abs().max()) / float(b.abs().max()) for a, b in zip(*outs)]
        assert max(diff) <= 2.0 ** -5, (h, diff)
        outs[0][1].zero_(), outs[1][1].zero_()
        tm = alternate([new, old], args.windows)
        valid = int(((idx >= 0) & (idx < N)).sum())
        us = tm[new].mean()
        name = f"H = {h}"
        say(f"{name:8s} | new {fmt(tm[new])} | old {fmt(tm[old])} | old / new {tm[old].mean() / us:7.2f} | dq, dk, d_weights differ by "
            f"{diff[0]:.1e}, {diff[1]:.1e}, {diff[2]:.1e} of the largest value | matrix {6.0 * h * D * valid / (us * 1e-6) / PEAK_FLOPS:6.3f} of peak | "
            f"atomics {valid * 512 / (us * 1e-6) / 1e12:6.2f} TB/s")
        if not tm[new].max() < tm[old].min():
            failed.append(name)
        del q, k, qb, kb, idx, dl, outs
        torch.cuda.empty_cache()
    say("# cases where new is not faster than old beyond the spread: " + ("; ".join(failed) if failed else "none"))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
