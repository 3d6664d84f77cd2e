"""Times router_balance_loss + router_balance_loss_backward against the torch expression they replace, to scripts/router_topk_timing.py's
protocol: both forms run alternately in one process on the same tensors, in windows of back-to-back calls between two device events (each
window sized to well over 100 ms after a calibration), after a warm-up; mean and min..max over the windows.  Before any time is reported
the results are compared: the counts exactly, loss, psum and the gradient added to dlogits to float32 rounding.
Cases: T = 4096 and 32768 tokens, E = 256 experts, k = 8, sigmoid scores with normalisation, one segment (B = 1, Switch / GShard's global
loss) and sequences of L = 4096 tokens (DeepSeek-V3's sequence-wise loss).
  new     router_balance_loss(scores, ids, out=...) then router_balance_loss_backward(dloss, counts, scores, add_to=dlogits, out=dlogits)
  torch   counts by scatter_add of ones, p = s / s.sum(-1), psum = p.view(B, L, E).sum(1), loss = coef (counts psum).sum(-1); autograd
          back to the scores, times s (1 - s), added to dlogits
The condition: the entries are not slower than the torch expression on any case (new / torch <= 1.0).
Usage: python scripts/router_balance_timing.py [--out profiles/router_balance_timing.txt] [--windows N]"""
import argparse
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import deepgemm_ascend_amd as dga  # noqa: E402
from scripts.cast_transposed_timing import alternate  # noqa: E402

TOKENS, E, K, SEQ, ALPHA = (4096, 32768), 256, 8, 4096, 0.01


def torch_form(scores, ids, dloss, dlogits, seq_len):
    t_n = scores.shape[0]
    b_n = t_n // seq_len
    s = scores.detach().requires_grad_()
    seg = (torch.arange(t_n, device=ids.device) // seq_len)[:, None].expand(t_n, K)
    counts = torch.zeros(b_n * E, dtype=torch.float32, device=ids.device)
    counts.scatter_add_(0, (seg * E + ids).reshape(-1), torch.ones(t_n * K, dtype=torch.float32, device=ids.device))
    counts = counts.view(b_n, E)
    p = s / s.sum(dim=-1, keepdim=True)
    psum = p.view(b_n, seq_len, E).sum(dim=1)
    loss = (ALPHA * E / (K * seq_len * seq_len)) * (counts * psum).sum(dim=-1)
    loss.backward(dloss)
    dlogits += s.grad * scores * (1.0 - scores)
    return loss.detach(), counts, psum.detach()


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
    say(f"# {torch.cuda.get_device_name(0)}; E = {E}, k = {K}, sigmoid scores, normalised; loss + backward added to dlogits; device events around "
        f"windows of back-to-back calls (>= 150 ms each), {args.windows} windows per form, alternating; mean [min..max] us per call; "
        f"condition: new / torch <= 1.00")
    slower = []
    for t_n in TOKENS:
        g = torch.Generator(device="cuda").manual_seed(t_n)
        logits = (torch.randn((t_n, E), device="cuda", generator=g) * 2.0).bfloat16()
        ids, _, scores = dga.router_topk(logits, K, score_func="sigmoid")
        long_ids = ids.long()
        for seq_len in sorted({t_n, SEQ}, reverse=True):
            b_n = t_n // seq_len
            dloss = torch.rand((b_n,), device="cuda", generator=g) + 0.5
            out = (torch.empty((b_n,), device="cuda"), torch.empty((b_n, E), dtype=torch.int32, device="cuda"), torch.empty((b_n, E), device="cuda"))
            d_new, d_old = torch.zeros((t_n, E), device="cuda"), torch.zeros((t_n, E), device="cuda")

            def new():
                dga.router_balance_loss(scores, ids, seq_len=seq_len, alpha=ALPHA, normalize=True, out=out)
                return dga.router_balance_loss_backward(dloss, out[1], scores, K, "sigmoid", seq_len=seq_len, alpha=ALPHA, normalize=True,
                                                        add_to=d_new, out=d_new)

            old = lambda: torch_form(scores, long_ids, dloss, d_old, seq_len)
            name = f"[{t_n}, {E}] B = {b_n:2d} L = {seq_len:5d}"
            new()
            loss, counts, psum = old()
            torch.cuda.synchronize()
            assert torch.equal(out[1].float(), counts), f"{name}: the counts differ"
            assert torch.allclose(out[0], loss, rtol=1e-4) and torch.allclose(out[2], psum, rtol=1e-4), f"{name}: loss or psum differ"
            assert torch.allclose(d_new, d_old, rtol=1e-3, atol=float(d_old.abs().max()) * 1e-5), f"{name}: the gradients differ"
            t = alternate([new, old], args.windows)
            ratio = t[new].mean() / t[old].mean()
            say(f"{name} | new {fmt(t[new])} | torch {fmt(t[old])} | new / torch {ratio:5.2f}")
            if ratio > 1.0:
                slower.append(name)
            del out, d_new, d_old
            torch.cuda.empty_cache()
    say("# slower than the torch expression: " + ("; ".join(" ".join(n.split()) for n in slower) if slower else "no case"))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
