"""Times fp8_paged_mqa_logits and per_token_cast_to_fp8_paged against what a user had before them.  Old and new run alternately in one
process on the same tensors, in windows of back-to-back calls between two device events (each window sized to over 100 ms after a
calibration, at least 3 calls), after a warm-up; mean and min..max over the windows (a call shorter than its launch is timed at the
rate the host can launch it: that is what a caller outside a graph sees).  Before any time is reported the results are
byte-compared.
Scoring, H = 64, N = 65536, block tables a random permutation of the blocks, the cache written by per_token_cast_to_fp8_paged from normal
samples, q per_token_cast_to_fp8 of normal samples, float32 weights.  Cases, each with clean_logits both ways:
  B =  64, every context 4096, next_n = 1
  B =  64, every context 32768, next_n = 2
  B = 128, contexts spread evenly over 1024 .. 65536, next_n = 2
  B =   1, context 65536, next_n = 1
  new   fp8_paged_mqa_logits(q, kv_cache, weights, context_lens, block_tables, None, N, clean_logits, out=...)
  old   per sequence: index_select of its pages' codes and of their scales into contiguous tensors, fp8_mqa_logits with M = next_n and
        ke = ctx - next_n + j + 1, a copy into the row slice; with clean_logits one fill of the whole output with -inf in front.  The
        lengths, page lists and ranges are prepared on the host outside the timed part, which favours the old path.
Reported without a bar: the time over the byte floor -- (sum of keys) * 132 B read plus the logits written, at the 5.8 and 6.4 TB/s grad_sumsq
reads at -- and over the matrix floor, 2 * 128 * H flop per in-range (row, key) pair at mfma_ceiling('bf16_exact').
Writer: per_token_cast_to_fp8_paged(x, cache, slots) against per_token_cast_to_fp8(x) plus two index_put_ (codes, scales) at T = 128 and
T = 8192, bf16 x, scattered slots.
The condition, set before the run: new / old <= 1.0 at every case.
Usage: python scripts/paged_mqa_logits_timing.py [--out profiles/paged_mqa_logits_timing.txt] [--windows N]"""
import argparse
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import deepgemm_ascend_amd as dga  # noqa: E402
from scripts.mqa_logits_timing import alternate  # noqa: E402

H, D, N, KV, BYTES = 64, 128, 65536, 64, 8448
CASES = (("B= 64 ctx 4096 n1", 64, 1, lambda b: np.full(b, 4096)),
         ("B= 64 ctx 32768 n2", 64, 2, lambda b: np.full(b, 32768)),
         ("B=128 ctx 1024..65536 n2", 128, 2, lambda b: np.linspace(1024, 65536, b).astype(np.int64)),
         ("B=  1 ctx 65536 n1", 1, 1, lambda b: np.full(b, 65536)))
STREAM_TBS = (5.8, 6.4)


def build_cache(num_blocks, gen):
    """a dense cache of num_blocks blocks filled through the writer, a million keys at a time"""
    cache = torch.empty((num_blocks, KV, 1, D + 4), dtype=torch.uint8, device="cuda")
    total = num_blocks * KV
    for lo in range(0, total, 1 << 20):
        hi = min(lo + (1 << 20), total)
        x = torch.randn((hi - lo, D), device="cuda", generator=gen, dtype=torch.float32).to(torch.bfloat16)
        dga.per_token_cast_to_fp8_paged(x, cache, torch.arange(lo, hi, device="cuda", dtype=torch.int64))
    torch.cuda.synchronize()
    return cache


def old_form(q, codes, scales, weights, pages, ctxs, zeros, ends, out, clean):
    b, nn = q.shape[0], q.shape[1]
    if clean:
        out.fill_(float("-inf"))
    for i in range(b):
        ctx = ctxs[i]
        k = codes.index_select(0, pages[i]).view(-1, D)[:ctx]
        s = scales.index_select(0, pages[i]).view(torch.float32).view(-1)[:ctx]
        out[i * nn:(i + 1) * nn, :ctx] = dga.fp8_mqa_logits(q[i], (k, s), weights[i * nn:(i + 1) * nn], zeros[i], ends[i])
    return out


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
    ceiling = dga.mfma_ceiling("bf16_exact")
    say(f"# {torch.cuda.get_device_name(0)}; H = {H}, N = {N}; new = fp8_paged_mqa_logits(out=...), old = per sequence index_select of codes and scales, "
        f"fp8_mqa_logits (M = next_n), copy into the row slice (clean: one -inf fill in front); device events around windows of back-to-back "
        f"calls (>= 100 ms each, at least 3 calls), {args.windows} windows per form, alternating; results byte-compared first; mean [min..max] us per call")
    say(f"# byte floor: (sum of keys) * 132 B + the logits written, at {STREAM_TBS[0]} and {STREAM_TBS[1]} TB/s (grad_sumsq's measured stream); matrix floor: "
        f"2 * 128 * H flop per in-range pair at mfma_ceiling('bf16_exact') = {ceiling:.0f} TFLOP/s; condition: new / old <= 1.00 at every case")
    slower = []
    gen = torch.Generator(device="cuda").manual_seed(1)
    for name, b, nn, lens_of in CASES:
        lens = lens_of(b).astype(np.int64)
        need = (lens + KV - 1) // KV
        num_blocks, max_blocks = int(need.sum()), N // KV
        cache = build_cache(num_blocks, gen)
        perm = np.random.default_rng(b + nn).permutation(num_blocks)
        tables = np.full((b, max_blocks), -1, np.int32)
        at = 0
        for i in range(b):
            tables[i, :need[i]] = perm[at:at + need[i]]
            at += need[i]
        tables_d = torch.from_numpy(tables).cuda()
        lens_d = torch.from_numpy(lens.astype(np.int32)).cuda()
        q, _ = dga.per_token_cast_to_fp8(torch.randn((b * nn * H, D), device="cuda", generator=gen))
        q = q.view(b, nn, H, D)
        weights = torch.randn((b * nn, H), device="cuda", generator=gen)
        flat = cache.view(num_blocks, BYTES)
        codes, scales = flat[:, :KV * D], flat[:, KV * D:]
        pages = [tables_d[i, :need[i]].long() for i in range(b)]
        ctxs = [int(v) for v in lens]
        zeros = [torch.zeros(nn, dtype=torch.int32, device="cuda") for _ in range(b)]
        ends = [torch.tensor([c - nn + j + 1 for j in range(nn)], dtype=torch.int32, device="cuda") for c in ctxs]
        pairs = sum(max(c - nn + j + 1, 0) for c in ctxs for j in range(nn))
        for clean in (True, False):
            fill = float("nan")
            out_new = torch.full((b * nn, N), fill, device="cuda")
            out_old = torch.full((b * nn, N), fill, device="cuda")
            new = lambda: dga.fp8_paged_mqa_logits(q, cache, weights, lens_d, tables_d, None, N, clean, out=out_new)
            old = lambda: old_form(q, codes, scales, weights, pages, ctxs, zeros, ends, out_old, clean)
            label = f"{name} clean={'T' if clean else 'F'}"
            new(), old()
            torch.cuda.synchronize()
            if clean:
                assert torch.equal(out_new.view(torch.int32), out_old.view(torch.int32)), f"{label}: results differ"
            else:
                for i in range(b):
                    rows = slice(i * nn, (i + 1) * nn)
                    assert torch.equal(out_new[rows, :ctxs[i]].view(torch.int32), out_old[rows, :ctxs[i]].view(torch.int32)), f"{label}: results differ"
                    assert torch.isnan(out_new[rows, int(need[i]) * KV:]).all(), f"{label}: written beyond the last page"
            t = alternate([new, old], args.windows)
            ratio = t[new].mean() / t[old].mean()
            wrote = b * nn * N * 4 if clean else int((need * KV * nn * 4).sum())
            nbytes = int(lens.sum()) * (D + 4) + wrote
            floors = [nbytes / (r * 1e12) * 1e6 for r in STREAM_TBS]
            mfloor = 2.0 * D * H * pairs / (ceiling * 1e12) * 1e6
            say(f"{label:32s} | new {fmt(t[new])} | old {fmt(t[old])} | new / old {ratio:6.4f} | bytes {nbytes / 1e6:8.1f} MB: byte floor "
                f"{floors[1]:7.1f}..{floors[0]:7.1f} us, new = {t[new].mean() / floors[1]:5.2f}..{t[new].mean() / floors[0]:5.2f} x | matrix floor "
                f"{mfloor:7.1f} us, new = {t[new].mean() / mfloor:5.2f} x")
            if ratio > 1.0:
                slower.append(" ".join(label.split()))
            del out_new, out_old
        del cache, flat, codes, scales, q, weights, pages
        torch.cuda.empty_cache()

    # the writer
    num_blocks = 4096
    for tokens in (128, 8192):
        x = torch.randn((tokens, D), device="cuda", generator=gen).to(torch.bfloat16)
        slots = torch.from_numpy(np.random.default_rng(tokens).permutation(num_blocks * KV)[:tokens].astype(np.int64)).cuda()
        blk, key = slots // KV, slots % KV
        cache_new = torch.zeros((num_blocks, BYTES), dtype=torch.uint8, device="cuda")
        cache_old = torch.zeros_like(cache_new)
        codes_old = cache_old[:, :KV * D].view(num_blocks, KV, D)
        scales_old = cache_old[:, KV * D:].view(torch.float32)

        def old():
            qx, sf = dga.per_token_cast_to_fp8(x)
            codes_old.index_put_((blk, key), qx.view(torch.uint8))
            scales_old.index_put_((blk, key), sf.view(-1))

        new = lambda: dga.per_token_cast_to_fp8_paged(x, cache_new, slots)
        new(), old()
        torch.cuda.synchronize()
        label = f"writer T = {tokens}"
        assert torch.equal(cache_new, cache_old) and int((cache_new != 0).sum()) > tokens * 100, f"{label}: caches differ"
        t = alternate([new, old], args.windows)
        ratio = t[new].mean() / t[old].mean()
        say(f"{label:32s} | new {fmt(t[new])} | old {fmt(t[old])} | new / old {ratio:6.4f}")
        if ratio > 1.0:
            slower.append(label)
    say("# cases slower than the old path: " + ("; ".join(slower) if slower else "none"))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
