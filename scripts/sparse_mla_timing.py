"""Times sparse_mla_fwd against what a user had before it.  Old and new run alternately in one process on the same operands, in windows of
back-to-back calls between two device events (each window sized to over 150 ms after a calibration, at least 3 calls), after a warm-up;
mean and min..max over the windows.  Before any time is reported the results are compared: out to 2^-5 of the largest value, lse to 2^-5
(the old path's bmm rounds the scores to bf16, about 2^-9 of a score of a few units, before its softmax).
topk = 2048, bf16 normal samples, sm_scale = 576^-0.5.  Cases:
  prefill  M = 4096, S = 32768, Hq = 128: token m sees keys 0 .. S - M + m and selects the 2048 largest of a score shared by all tokens
           plus noise of its own, so consecutive tokens select largely the same keys (what the indexer gives on real text)
  prefill  the same, Hq = 64
  decode   B = 128, next_n = 2, Hq = 128: contexts spread evenly over 1024 .. 65536 in a paged latent cache (pages of 64 rows handed
           out at random), 2048 positions drawn per token, given as physical slots (-1 padded where the context is shorter)
  decode   M = 1, S = 65536, Hq = 128
  new   sparse_mla_fwd(q, kv, indices, sm_scale, out=..., lse=...)
  old   per chunk of tokens small enough to fit: index_select of the rows (clamped; [chunk, 2048, 576]), bmm with q, the invalid
        positions filled with -inf, softmax in fp32, bmm with the first 512 columns
Reported beside each time: the fraction of the 2.5 PFLOP/s bf16 matrix rate on 2 Hq valid (576 + 512) flops per token, and the bytes
gathered per second -- valid x 1152 bytes per token and block of 64 heads, the unit that gathers.  With --grid the new path is also timed
with DGA_SPARSE_MLA_LINEAR_GRID (workgroups in grid order, not consecutive tokens on one XCD).
The condition, set before the run: new < old at every case, by more than the windows spread (max new < min old).
Usage: python scripts/sparse_mla_timing.py [--out profiles/sparse_mla_timing.txt] [--windows N] [--grid]"""
import argparse
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import deepgemm_ascend_amd as dga  # noqa: E402
from scripts.indexer_topk_timing import alternate  # noqa: E402

TOPK, D, DV, PAGE = 2048, 576, 512, 64
SCALE = D ** -0.5
PEAK_FLOPS = 2.5e15


def prefill_case(m, s, gen):
    """indices int32 [m, 2048] ascending: the 2048 best of shared + own scores among the keys token t sees"""
    shared = torch.randn((1, s), device="cuda", generator=gen)
    idx = torch.empty((m, TOPK), dtype=torch.int32, device="cuda")
    for lo in range(0, m, 512):
        rows = torch.arange(lo, min(lo + 512, m), device="cuda")
        score = shared + 0.25 * torch.randn((len(rows), s), device="cuda", generator=gen)
        score.masked_fill_(torch.arange(s, device="cuda")[None, :] > (s - m + rows)[:, None], float("-inf"))
        idx[lo:lo + len(rows)] = score.topk(TOPK, dim=1).indices.sort(dim=1).values.to(torch.int32)
    return idx


def decode_case(b, nn, lo, hi, gen):
    """(indices int32 [b nn, 2048] of physical slots, -1 padded; rows of the cache)"""
    lens = np.linspace(lo, hi, b).astype(np.int64)
    pages = (lens + PAGE - 1) // PAGE
    order = torch.randperm(int(pages.sum()), device="cuda", generator=gen)
    first = np.concatenate([[0], np.cumsum(pages)[:-1]])
    idx = torch.full((b * nn, TOPK), -1, dtype=torch.int32, device="cuda")
    for i, ctx in enumerate(lens):
        table = order[first[i]:first[i] + pages[i]]
        for j in range(nn):
            seen = int(ctx) - nn + j + 1
            take = min(seen, TOPK)
            pos = torch.randperm(seen, device="cuda", generator=gen)[:take].sort().values
            idx[i * nn + j, :take] = (table[pos // PAGE] * PAGE + pos % PAGE).to(torch.int32)
    return idx, int(pages.sum()) * PAGE


def old_form(q, kv, idx, chunk):
    m, h = q.shape[:2]
    out = torch.empty((m, h, DV), dtype=torch.bfloat16, device=q.device)
    lse = torch.empty((m, h), dtype=torch.float32, device=q.device)
    s_rows = kv.shape[0]
    for lo in range(0, m, chunk):
        i = idx[lo:lo + chunk].long()
        valid = (i >= 0) & (i < s_rows)
        g = kv.index_select(0, i.clamp(0, s_rows - 1).flatten()).view(i.shape[0], TOPK, D)
        sc = torch.bmm(q[lo:lo + chunk], g.transpose(1, 2)).float().mul_(SCALE).masked_fill_(~valid[:, None, :], float("-inf"))
        lse[lo:lo + chunk] = torch.logsumexp(sc, dim=-1)
        out[lo:lo + chunk] = torch.bmm(torch.softmax(sc, dim=-1).to(torch.bfloat16), g[:, :, :DV])
    return out, lse


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--grid", action="store_true")
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    fmt = lambda v: f"{v.mean():9.1f} [{v.min():9.1f}..{v.max():9.1f}] us"
    say(f"# {torch.cuda.get_device_name(0)}; topk = {TOPK}; new = sparse_mla_fwd(out=..., lse=...), old = index_select, bmm, -inf fill, fp32 "
        f"softmax, bmm in token chunks; device events around windows of back-to-back calls (>= 150 ms each, at least 3 calls), "
        f"{args.windows} windows per form, alternating; results compared first; mean [min..max] us per call")
    say("# matrix: fraction of 2.5 PFLOP/s on 2 Hq valid (576 + 512) flops per token; gather: valid x 1152 B per token and 64-head block; "
        "condition: max new < min old at every case")
    gen = torch.Generator(device="cuda").manual_seed(1)
    cases = (("prefill M=4096 S=32768 Hq=128", "prefill", 4096, 32768, 128, 64),
             ("prefill M=4096 S=32768 Hq= 64", "prefill", 4096, 32768, 64, 128),
             ("decode B=128 n2 ctx 1024..65536 Hq=128", "decode", 128, 0, 128, 64),
             ("decode M=1 S=65536 Hq=128", "prefill", 1, 65536, 128, 1))
    failed = []
    for name, kind, count, s, h, chunk in cases:
        if kind == "prefill":
            m, idx = count, prefill_case(count, s, gen)
        else:
            idx, s = decode_case(count, 2, 1024, 65536, gen)
            m = count * 2
        q = torch.randn((m, h, D), device="cuda", generator=gen).to(torch.bfloat16)
        kv = torch.randn((s, D), device="cuda", generator=gen).to(torch.bfloat16)
        out, lse = torch.empty((m, h, DV), dtype=torch.bfloat16, device="cuda"), torch.empty((m, h), dtype=torch.float32, device="cuda")
        new = lambda: dga.sparse_mla_fwd(q, kv, idx, SCALE, out=out, lse=lse)
        old = lambda: old_form(q, kv, idx, chunk)
        new()
        want, want_lse = old()
        torch.cuda.synchronize()
        d_out = float((out.float() - want.float()).abs().max()) / float(want.float().abs().max())
        d_lse = float((lse - want_lse).abs().max())
        assert d_out <= 2.0 ** -5 and d_lse <= 2.0 ** -5, (name, d_out, d_lse)
        del want, want_lse
        fns = [new, old]
        if args.grid:
            linear = lambda: dga.sparse_mla_fwd(q, kv, idx, SCALE, out=out, lse=lse, _flags=1)
            fns.append(linear)
        t = alternate(fns, args.windows)
        valid = int((idx >= 0).sum())
        flops = 2.0 * h * valid * (D + DV)
        nbytes = valid * D * 2 * ((h + 63) // 64)
        us = t[new].mean()
        line = (f"{name:40s} | new {fmt(t[new])} | old {fmt(t[old])} | old / new {t[old].mean() / us:7.2f} | out differs by {d_out:.1e} of the "
                f"largest value, lse by {d_lse:.1e} | matrix {flops / (us * 1e-6) / PEAK_FLOPS:6.3f} of peak | gather {nbytes / (us * 1e-6) / 1e12:6.2f} TB/s")
        if args.grid:
            line += f" | grid order {fmt(t[linear])}, {t[linear].mean() / us:5.2f} x"
        say(line)
        if not t[new].max() < t[old].min():
            failed.append(" ".join(name.split()))
        del q, kv, idx, out, lse
        torch.cuda.empty_cache()
    say("# cases where new is not faster than old beyond the spread: " + ("; ".join(failed) if failed else "none"))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
