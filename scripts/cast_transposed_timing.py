"""Times per_token_cast_to_fp8_transposed (one pass) against the path it replaces: per_token_cast_to_fp8(x.t().contiguous()), plus
per_token_cast_to_fp8(x) for the rowwise=True rows, plus the masked_fill of the padding rows for the m_indices case.  Both run alternately
in one process on the same tensors, in windows of back-to-back calls between two device events (each window sized to well over 100 ms after
a calibration), after a warm-up; mean and min..max over the windows.  Before any time is reported every output of the new entry is compared
with the old path's, whole tensors, byte for byte (the old path is the oracle-tested quantiser on the transpose; the masked row-wise output
on the valid rows, the sentinels on the others).
Cases (bf16): [32768, 7168], [32768, 2048], [4096, 4096], and [32768, 2048] with a random contiguous-layout m_indices (8 experts, every
segment padded to 128 rows).  TB/s = the bytes one pass needs, 3 per element (4 with rowwise), over the new entry's time.
Usage: python scripts/cast_transposed_timing.py [--out profiles/cast_transposed_timing.txt] [--windows N]"""
import argparse
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import deepgemm_ascend_amd as dga  # noqa: E402

SHAPES = [(32768, 7168, False), (32768, 2048, False), (4096, 4096, False), (32768, 2048, True)]
SENTINEL_Q, SENTINEL_SF = 0xA5, 0x7FC0A5A5


def contiguous_m_indices(t_n, experts=8, seed=7):
    """int32 [t_n]: `experts` segments of whole 128-row blocks in random proportions; each ends in 0..127 padding rows (index -1)."""
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.choice(np.arange(1, t_n // 128), size=experts - 1, replace=False)) * 128
    idx = np.full(t_n, -1, np.int32)
    for g, (lo, hi) in enumerate(zip(np.r_[0, cuts], np.r_[cuts, t_n])):
        idx[lo:hi - rng.integers(0, 128)] = g
    return idx


def forms(x, idx, rowwise):
    t_n, h = x.shape
    qt = torch.full((h, t_n), SENTINEL_Q, dtype=torch.uint8, device="cuda")
    sft = torch.full((h, t_n // 128), SENTINEL_SF, dtype=torch.int32, device="cuda").view(torch.float32)
    q = torch.full((t_n, h), SENTINEL_Q, dtype=torch.uint8, device="cuda")
    sf = torch.full((t_n, (h + 127) // 128), SENTINEL_SF, dtype=torch.int32, device="cuda").view(torch.float32)
    out = ((qt, sft), (q, sf)) if rowwise else (qt, sft)

    def new():
        dga.per_token_cast_to_fp8_transposed(x, m_indices=idx, rowwise=rowwise, out=out)

    def old():
        x0 = x if idx is None else x.masked_fill((idx < 0).unsqueeze(1), 0.0)
        r = dga.per_token_cast_to_fp8(x0.t().contiguous())
        return r + dga.per_token_cast_to_fp8(x) if rowwise else r

    return new, old, (qt, sft, q, sf)


def check(name, new, old, outs, idx, rowwise):
    qt, sft, q, sf = outs
    new()
    want = old()
    torch.cuda.synchronize()
    assert torch.equal(qt, want[0].view(torch.uint8)) and torch.equal(sft.view(torch.int32), want[1].view(torch.int32)), f"{name}: (qt, sft) differ"
    if rowwise:
        valid = torch.ones(q.shape[0], dtype=torch.bool, device="cuda") if idx is None else idx >= 0
        assert torch.equal(q[valid], want[2].view(torch.uint8)[valid]) and torch.equal(sf[valid], want[3][valid]), f"{name}: (q, sf) differ"
        assert bool((q[~valid] == SENTINEL_Q).all()) and bool((sf[~valid].view(torch.int32) == SENTINEL_SF).all()), f"{name}: an excluded row was written"


def window_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternate(fns, windows):
    """{fn: us per call, one entry per window}: warm-up and a calibration window each, then `windows` rounds over all of them in turn."""
    calls = {}
    for fn in fns:
        window_ms(fn, 20)
        calls[fn] = max(50, int(150.0 / (window_ms(fn, 50) / 50)) + 1)
    t = {fn: [] for fn in fns}
    for _ in range(windows):
        for fn in fns:
            t[fn].append(window_ms(fn, calls[fn]) * 1e3 / calls[fn])
    return {fn: np.array(v) for fn, v in t.items()}


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
    say(f"# {torch.cuda.get_device_name(0)}; bf16; new = per_token_cast_to_fp8_transposed(out=...), old = per_token_cast_to_fp8(x.t().contiguous()) "
        f"(+ per_token_cast_to_fp8(x) with rowwise, + masked_fill with m_indices)")
    say(f"# device events around windows of back-to-back calls (>= 150 ms each), {args.windows} windows per form, alternating; mean [min..max] us "
        f"per call; traffic ratio: 3/7 = 0.43, rowwise 4/10 = 0.40")
    for t_n, h, masked in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(t_n + h)
        x = (torch.randn((t_n, h), device="cuda", generator=g) * 3.0).bfloat16()
        idx = torch.from_numpy(contiguous_m_indices(t_n)).cuda() if masked else None
        if masked:
            x[idx < 0] = float("nan")
        for rowwise in (False, True):
            name = f"[{t_n}, {h}]{' m_indices' if masked else ''}{' rowwise' if rowwise else ''}"
            new, old, outs = forms(x, idx, rowwise)
            check(name, new, old, outs, idx, rowwise)
            t = alternate([new, old], args.windows)
            tb = t_n * h * (4 if rowwise else 3) / (t[new].mean() * 1e-6) / 1e12
            say(f"{name:36s} | new {fmt(t[new])} {tb:5.2f} TB/s | old {fmt(t[old])} | new / old {t[new].mean() / t[old].mean():5.2f}")
            del new, old, outs
        del x
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
