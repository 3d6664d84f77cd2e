"""Times indexer_topk against what a user had before it.  Old and new run alternately in one process on the same logits, in windows of
back-to-back calls between two device events (each window sized to over 150 ms after a calibration, at least 3 calls), after a warm-up;
mean and min..max over the windows.  Before any time is reported the results are byte-compared; torch.topk's order among equal values is
unspecified, so a row whose indices differ must select byte-identical values (such rows are counted and reported).
k = 2048, float32 logits of normal samples.  Cases:
  prefill  4096 x 4096 causal (ks = 0, ke = m + 1)
  prefill  4096 x 32768 with ke = N - M + m + 1
  decode   B =  64, every context 32768, next_n = 2, N = 65536
  decode   B = 128, contexts spread evenly over 1024 .. 65536, next_n = 2, N = 65536
  decode   B =   1, context 65536, next_n = 1, N = 65536
  new   indexer_topk(logits, 2048, row_starts, row_ends | context_lens, next_n, out=...) on logits whose out-of-range columns hold NaN
  old   masked_fill of the out-of-range columns with -inf (the mask prepared outside the timed part), torch.topk(k, sorted=False), the
        selected out-of-range columns replaced by a sentinel, a sort of the indices, the sentinel replaced by -1
Reported without a bar: the time over the byte floor -- the in-range logits read once plus 4 k bytes per row written, at the 5.8 and 6.4 TB/s
the project measures for a plain stream -- and the time as a fraction of the scoring kernel's at the same case (profiles/mqa_logits_timing.txt,
profiles/paged_mqa_logits_timing.txt with clean_logits=False).
The condition, set before the run: new / old <= 1.0 at every case.
Usage: python scripts/indexer_topk_timing.py [--out profiles/indexer_topk_timing.txt] [--windows N]"""
import argparse
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import deepgemm_ascend_amd as dga  # noqa: E402
from scripts.cast_transposed_timing import window_ms  # noqa: E402

K, N_DECODE = 2048, 65536
STREAM_TBS = (5.8, 6.4)
# (name, kind, rows or B, N, next_n, lengths, the scoring kernel's us at the case)
CASES = (("prefill 4096 x 4096 causal", "prefill", 4096, 4096, 1, lambda m, n: np.arange(m) + 1, 193.0),
         ("prefill 4096 x 32768", "prefill", 4096, 32768, 1, lambda m, n: n - m + np.arange(m) + 1, 1870.0),
         ("decode B= 64 ctx 32768 n2", "decode", 64, N_DECODE, 2, lambda b, n: np.full(b, 32768), 90.4),
         ("decode B=128 ctx 1024..65536 n2", "decode", 128, N_DECODE, 2, lambda b, n: np.linspace(1024, 65536, b).astype(np.int64), 215.0),
         ("decode B=  1 ctx 65536 n1", "decode", 1, N_DECODE, 1, lambda b, n: np.full(b, 65536), 10.1))


def alternate(fns, windows, ms=180.0):
    calls = {}
    for fn in fns:
        window_ms(fn, 2)
        calls[fn] = max(3, int(ms / (window_ms(fn, 3) / 3)) + 1)
    t = {fn: [] for fn in fns}
    for _ in range(windows):
        for fn in fns:
            t[fn].append(window_ms(fn, calls[fn]) * 1e3 / calls[fn])
    return {fn: np.array(v) for fn, v in t.items()}


def old_form(logits, outside, k):
    n = logits.shape[1]
    idx = torch.topk(logits.masked_fill(outside, float("-inf")), k, dim=1, sorted=False).indices
    idx = torch.where(outside.gather(1, idx), n, idx)
    idx = idx.sort(dim=1).values
    return torch.where(idx == n, -1, idx).to(torch.int32)


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
    say(f"# {torch.cuda.get_device_name(0)}; k = {K}; new = indexer_topk(out=...) on logits with NaN outside the ranges, old = masked_fill(-inf), "
        f"torch.topk(sorted=False), sort of the indices, -1 pad (the mask prepared outside the timed part); device events around windows of "
        f"back-to-back calls (>= 150 ms each, at least 3 calls), {args.windows} windows per form, alternating; results byte-compared first; "
        f"mean [min..max] us per call")
    say(f"# byte floor: the in-range logits read once + 4 k bytes per row, at {STREAM_TBS[0]} and {STREAM_TBS[1]} TB/s; scoring: the scoring kernel's "
        f"time at the case (mqa_logits_timing.txt, paged_mqa_logits_timing.txt clean=F); condition: new / old <= 1.00 at every case")
    slower = []
    gen = torch.Generator(device="cuda").manual_seed(1)
    for name, kind, count, n, nn, lens_of, scoring_us in CASES:
        lens = lens_of(count, n).astype(np.int64)
        m = count * nn
        hi = np.maximum(np.repeat(lens, nn) - nn + np.arange(m) % nn + 1, 0) if kind == "decode" else lens
        logits = torch.randn((m, n), device="cuda", generator=gen)
        hi_d = torch.from_numpy(hi.astype(np.int32)).cuda()
        outside = torch.arange(n, device="cuda", dtype=torch.int32)[None, :] >= hi_d[:, None]
        logits.masked_fill_(outside, float("nan"))
        out_new = torch.full((m, K), 7, dtype=torch.int32, device="cuda")
        if kind == "decode":
            lens_d = torch.from_numpy(lens.astype(np.int32)).cuda()
            new = lambda: dga.indexer_topk(logits, K, context_lens=lens_d, next_n=nn, out=out_new)
        else:
            zeros = torch.zeros(m, dtype=torch.int32, device="cuda")
            new = lambda: dga.indexer_topk(logits, K, row_starts=zeros, row_ends=hi_d, out=out_new)
        old = lambda: old_form(logits, outside, K)
        got, want = new(), old()
        torch.cuda.synchronize()
        differ = torch.nonzero((got != want).any(dim=1)).flatten()
        for r in differ.tolist():                                         # equal values at the cut: the sets may differ, the values may not
            a, b = got[r][got[r] >= 0].long(), want[r][want[r] >= 0].long()
            va, vb = logits[r][a].view(torch.int32).sort().values, logits[r][b].view(torch.int32).sort().values
            assert torch.equal(va, vb), f"{name}: row {r} selects other values"
        del want
        t = alternate([new, old], args.windows)
        ratio = t[new].mean() / t[old].mean()
        read = int(np.where(hi > K, hi, 0).sum()) * 4                     # (a row no longer than k reads nothing)
        nbytes = read + m * K * 4
        floors = [nbytes / (r * 1e12) * 1e6 for r in STREAM_TBS]
        say(f"{name:32s} | new {fmt(t[new])} | old {fmt(t[old])} | new / old {ratio:6.4f} | rows with ties at the cut {len(differ)} | bytes "
            f"{nbytes / 1e6:7.1f} MB: byte floor {floors[1]:6.1f}..{floors[0]:6.1f} us, new = {t[new].mean() / floors[1]:6.2f}..{t[new].mean() / floors[0]:6.2f} x | "
            f"scoring {scoring_us:7.1f} us, new = {t[new].mean() / scoring_us:5.2f} of it")
        if ratio > 1.0:
            slower.append(" ".join(name.split()))
        del logits, outside, out_new
        torch.cuda.empty_cache()
    say("# cases slower than the old path: " + ("; ".join(slower) if slower else "none"))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
