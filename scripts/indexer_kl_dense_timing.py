"""Times indexer_kl_loss_dense against what a user had before it, under the protocol of scripts/indexer_kl_timing.py: old and new run
alternately in one process on the same tensors, in windows of back-to-back calls between two device events (each over 150 ms after a
calibration, at least 3 calls), after a warm-up; mean and min..max over the windows.  Before any time is reported the results are
compared: loss and d_logits each to 2^-5 of its largest value (the old path's matmul rounds the scores to bf16, in the exponent of p).
M = 4096, ks = 0, ke = N - M + m + 1, N = S in {8192, 32768}, Hq in {64, 128}, bf16 normal q and kv, sm_scale = 576^-0.5, logits
fp8_mqa_logits' [M, N] on amax-quantised normal samples of 64 indexer heads (-inf outside the ranges).
  new     indexer_kl_loss_dense(q, kv, ks, ke, sm_scale, logits, grad_scale=1 / M, loss=..., d_logits=..., lse_out=...): two launches
  given   the same with lse= what the first call returned: the loss launch alone (one case, to separate the two launches)
  old     per chunk of tokens small enough to fit: matmul of q with kv^T ([chunk, Hq, N] fp32), -inf outside the ranges, logsumexp,
          exp(s - lse), the mean over the heads, log_softmax of the masked logits, the KL sum and softmax - target
Reported beside each time: the fraction of the 2.5 PFLOP/s bf16 matrix rate that 2 2 Hq 576 flops per in-range pair amount to (both passes'
products; one pass when lse is given), and the time per scored (token, key) pair and pass beside indexer_kl_loss's, taken from
profiles/indexer_kl_timing.txt (M 2048 pairs a call, one pass).
The condition, set before the run: at every case the slowest new window is faster than the fastest old one (max new < min old).
Usage: python scripts/indexer_kl_dense_timing.py [--out profiles/indexer_kl_dense_timing.txt] [--windows N]"""
import argparse
import re
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import deepgemm_ascend_amd as dga  # noqa: E402
from scripts.indexer_topk_timing import alternate  # noqa: E402
from scripts.sparse_mla_timing import D, PEAK_FLOPS, SCALE, TOPK  # noqa: E402

M, HI, DI = 4096, 64, 128


def old_form(q, kv, ks, ke, logits, grad_scale, loss, dl, chunk):
    n, h = kv.shape[0], q.shape[1]
    col = torch.arange(n, device=q.device, dtype=torch.int32)
    for lo in range(0, q.shape[0], chunk):
        sl = slice(lo, lo + chunk)
        outside = (col < ks[sl, None]) | (col >= ke[sl, None])
        s = torch.matmul(q[sl].reshape(-1, D), kv.t()).view(-1, h, n).float().mul_(SCALE).masked_fill_(outside[:, None, :], float("-inf"))
        t = s.sub_(torch.logsumexp(s, dim=2, keepdim=True)).exp_().mean(1)
        a = torch.log_softmax(logits[sl].masked_fill(outside, float("-inf")), dim=1)
        loss[sl] = torch.where(t > 0, t * (t.log() - a), torch.zeros_like(t)).sum(1)
        dl[sl] = (a.exp() - t).mul_(grad_scale)
    return loss, dl


def sparse_ns_per_pair():
    """indexer_kl_loss's time per scored pair at Hq = 128 and 64, from its timing file"""
    text = (ROOT / "profiles" / "indexer_kl_timing.txt").read_text()
    return {int(h): float(us) * 1e3 / (M * TOPK) for h, us in re.findall(r"^Hq = (\d+)\s*\| new\s+([0-9.]+)", text, flags=re.M)}


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
    say(f"# {torch.cuda.get_device_name(0)}; M = {M}, ks = 0, ke = N - M + m + 1; new = indexer_kl_loss_dense(loss=..., d_logits=..., lse_out=...), "
        f"given = the same with lse=, old = matmul, masked logsumexp, exp, mean over heads, log_softmax, KL sum, softmax - target in token chunks; "
        f"device events around windows of back-to-back calls (>= 150 ms each, at least 3 calls), {args.windows} windows per form, alternating; "
        f"results compared first; mean [min..max] us per call")
    say("# matrix: fraction of 2.5 PFLOP/s on 2 Hq 576 flops per in-range pair and pass; ns per pair and pass beside indexer_kl_loss's "
        + ", ".join(f"{v:.3f} at Hq = {h}" for h, v in sorted(sparse.items())) + "; condition: max new < min old at every case")
    gen = torch.Generator(device="cuda").manual_seed(1)
    failed = []
    for n in (8192, 32768):
        qi, _ = dga.per_token_cast_to_fp8(torch.randn((M * HI, DI), device="cuda", generator=gen))
        ki, sfk = dga.per_token_cast_to_fp8(torch.randn((n, DI), device="cuda", generator=gen))
        tok = torch.arange(M, device="cuda", dtype=torch.int32)
        ks, ke = torch.zeros_like(tok), n - M + tok + 1
        logits = dga.fp8_mqa_logits(qi.view(M, HI, DI), (ki, sfk.reshape(n).contiguous()), torch.randn((M, HI), device="cuda", generator=gen), ks, ke)
        pairs = int(ke.sum())
        del qi, ki, sfk
        for h in (128, 64):
            q = torch.randn((M, h, D), device="cuda", generator=gen).to(torch.bfloat16)
            kv = torch.randn((n, D), device="cuda", generator=gen).to(torch.bfloat16)
            outs = [(torch.empty(M, device="cuda"), torch.empty((M, n), device="cuda")) for _ in range(2)]
            lse = torch.empty((M, h), device="cuda")
            new = lambda: dga.indexer_kl_loss_dense(q, kv, ks, ke, SCALE, logits, grad_scale=1.0 / M, loss=outs[0][0], d_logits=outs[0][1], lse_out=lse)
            given = lambda: dga.indexer_kl_loss_dense(q, kv, ks, ke, SCALE, logits, lse=lse, grad_scale=1.0 / M, loss=outs[0][0], d_logits=outs[0][1])
            old = lambda: old_form(q, kv, ks, ke, logits, 1.0 / M, *outs[1], max(1, (1 << 22) // (h * n) * 8))
            new(), old()
            torch.cuda.synchronize()
            diff = [float((a - b).abs().max()) / float(b.abs().max()) for a, b in zip(*outs)]
            assert max(diff) <= 2.0 ** -5, (h, n, diff)
            split = h == 128 and n == 8192
            tm = alternate([new, old] + ([given] if split else []), args.windows)
            us, name = tm[new].mean(), f"Hq = {h}, N = {n}"
            rate = lambda t, passes: f"matrix {passes * 2.0 * h * pairs * D / (t * 1e-6) / PEAK_FLOPS:6.3f} of peak, {t * 1e3 / pairs / passes:6.3f} ns per pair and pass"
            say(f"{name:20s} | new {fmt(tm[new])} | old {fmt(tm[old])} | old / new {tm[old].mean() / us:7.2f} | loss, d_logits differ by "
                f"{diff[0]:.1e}, {diff[1]:.1e} of the largest value | {rate(us, 2)}")
            if split:
                say(f"{name:20s} | lse given {fmt(tm[given])} | {rate(tm[given].mean(), 1)}")
            if not tm[new].max() < tm[old].min():
                failed.append(name)
            del q, kv, outs, lse
            torch.cuda.empty_cache()
        del logits
    say("# cases where new is not faster than old beyond the spread: " + ("; ".join(failed) if failed else "none"))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
