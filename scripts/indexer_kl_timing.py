"""Times indexer_kl_loss against what a user had before it, under the protocol of scripts/sparse_mla_bwd_timing.py: old and new run
alternately in one process on the same tensors, in windows of back-to-back calls between two device events (each over 150 ms after a
calibration, at least 3 calls), after a warm-up; mean and min..max over the windows.  Before any time is reported the results are
compared: d_logits and loss each to 2^-5 of its largest value -- the old path's bmm rounds the scores to bf16 (2^-9 of values of a few
units, in the exponent of p); 2^-5 is the siblings' bar for that rounding.
M = 4096, S = 32768, causal, topk = 2048 from indexer_topk on fp8_mqa_logits' output (64 indexer heads, amax-quantised normal samples),
bf16 normal q and kv, sm_scale = 576^-0.5, lse from sparse_mla_fwd, logits fp8_mqa_logits' [M, S]; Hq = 128 and 64.
  new   indexer_kl_loss(q, kv, indices, lse, sm_scale, logits, grad_scale=1 / M, loss=..., d_logits=...)
  old   per chunk of tokens small enough to fit: index_select of the rows ([chunk, 2048, 576]), bmm with q, exp(s - lse), the mean over
        the heads, gather of the logits, log_softmax, the KL sum and softmax - target
  fwd   sparse_mla_fwd(q, kv, indices, sm_scale, out=..., lse=...) at the same case, timed in the same alternation, for comparison only
Reported beside each time: the fraction of the 2.5 PFLOP/s bf16 matrix rate that 2 Hq valid 576 flops per token amount to.
The condition, set before the run: new < old at both cases, by more than the windows' spread (max new < min old).
Usage: python scripts/indexer_kl_timing.py [--out profiles/indexer_kl_timing.txt] [--windows N]"""
import argparse
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import deepgemm_ascend_amd as dga  # noqa: E402
from scripts.indexer_topk_timing import alternate  # noqa: E402
from scripts.sparse_mla_timing import D, PEAK_FLOPS, SCALE, TOPK  # noqa: E402

M, S, HI, DI = 4096, 32768, 64, 128


def old_form(q, kv, idx, lse, logits, grad_scale, loss, dl, chunk):
    for lo in range(0, q.shape[0], chunk):
        sl = slice(lo, lo + chunk)
        i = idx[sl].long()
        valid = (i >= 0) & (i < S)
        rows = i.clamp(0, S - 1)
        g = kv.index_select(0, rows.flatten()).view(i.shape[0], TOPK, D)
        t = torch.bmm(q[sl], g.transpose(1, 2)).float().mul_(SCALE).sub_(lse[sl, :, None]).exp_().mean(1).masked_fill_(~valid, 0.0)
        a = torch.log_softmax(logits[sl].gather(1, rows).masked_fill_(~valid, float("-inf")), dim=1)
        loss[sl] = torch.where(t > 0, t * (t.log() - a), torch.zeros_like(t)).sum(1)
        dl[sl] = (a.exp() - t).mul_(grad_scale)
    return loss, dl


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
    say(f"# {torch.cuda.get_device_name(0)}; M = {M}, S = {S}, causal, topk = {TOPK} from indexer_topk; new = indexer_kl_loss(loss=..., d_logits=...), "
        f"old = index_select, bmm, exp(s - lse), mean over heads, gather, log_softmax, KL sum, softmax - target in token chunks; fwd = sparse_mla_fwd "
        f"on the same operands; device events around windows of back-to-back calls (>= 150 ms each, at least 3 calls), {args.windows} windows per "
        f"form, alternating; results compared first; mean [min..max] us per call")
    say("# matrix: fraction of 2.5 PFLOP/s on 2 Hq valid 576 flops per token; condition: max new < min old at both cases")
    gen = torch.Generator(device="cuda").manual_seed(1)
    qi, _ = dga.per_token_cast_to_fp8(torch.randn((M * HI, DI), device="cuda", generator=gen))
    ki, sfk = dga.per_token_cast_to_fp8(torch.randn((S, DI), device="cuda", generator=gen))
    tok = torch.arange(M, device="cuda", dtype=torch.int32)
    ks, ke = torch.zeros_like(tok), S - M + tok + 1
    logits = dga.fp8_mqa_logits(qi.view(M, HI, DI), (ki, sfk.reshape(S).contiguous()), torch.randn((M, HI), device="cuda", generator=gen), ks, ke)
    idx = dga.indexer_topk(logits, TOPK, row_starts=ks, row_ends=ke)
    valid = int(((idx >= 0) & (idx < S)).sum())
    del qi, ki, sfk
    failed = []
    for h, chunk in ((128, 32), (64, 64)):
        q = torch.randn((M, h, D), device="cuda", generator=gen).to(torch.bfloat16)
        kv = torch.randn((S, D), device="cuda", generator=gen).to(torch.bfloat16)
        out, lse = dga.sparse_mla_fwd(q, kv, idx, SCALE)
        outs = [(torch.empty(M, device="cuda"), torch.empty((M, TOPK), device="cuda")) for _ in range(2)]
        new = lambda: dga.indexer_kl_loss(q, kv, idx, lse, SCALE, logits, grad_scale=1.0 / M, loss=outs[0][0], d_logits=outs[0][1])
        old = lambda: old_form(q, kv, idx, lse, logits, 1.0 / M, *outs[1], chunk)
        fwd = lambda: dga.sparse_mla_fwd(q, kv, idx, SCALE, out=out, lse=lse)
        new(), old()
        torch.cuda.synchronize()
        diff = [float((a - b).abs().max()) / float(b.abs().max()) for a, b in zip(*outs)]
        assert max(diff) <= 2.0 ** -5, (h, diff)
        tm = alternate([new, old, fwd], args.windows)
        us, name = tm[new].mean(), f"Hq = {h}"
        say(f"{name:8s} | new {fmt(tm[new])} | old {fmt(tm[old])} | old / new {tm[old].mean() / us:7.2f} | fwd {fmt(tm[fwd])} | new / fwd "
            f"{us / tm[fwd].mean():5.2f} | loss, d_logits differ by {diff[0]:.1e}, {diff[1]:.1e} of the largest value | matrix "
            f"{2.0 * h * valid * D / (us * 1e-6) / PEAK_FLOPS:6.3f} of peak")
        if not tm[new].max() < tm[old].min():
            failed.append(name)
        del q, kv, out, lse, outs
        torch.cuda.empty_cache()
    say("# cases where new is not faster than old beyond the spread: " + ("; ".join(failed) if failed else "none"))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
