"""Times per_block_cast_to_fp8_transposed (one pass over all experts) against the path it replaces, the per-expert loop
per_block_cast_to_fp8(w[g].t().contiguous()), plus per_block_cast_to_fp8(w[g]) for the rowwise=True rows, plus the torch.stack of the
results into the [G, ., .] tensors the grouped GEMMs take (a 2-D weight has no loop and no stack).  Both run alternately in one process on
the same tensors, in windows of back-to-back calls between two device events (each window sized to at least 150 ms after a calibration),
after a warm-up; mean and min..max over the windows.  Before any time is reported every output of the new entry is compared with the old
path's, whole tensors, byte for byte (the old path is the oracle-tested quantiser on each expert's transpose).
Cases: [32, 4096, 7168] bf16 and fp32, [32, 7168, 2048] bf16, [4096, 4096] bf16 (2-D), each with and without rowwise.  TB/s = the bytes one
pass needs -- 3 per bf16 element, 4 with rowwise; 5 and 6 for fp32 -- over the new entry's time.
Usage: python scripts/block_cast_transposed_timing.py [--out profiles/block_cast_transposed_timing.txt] [--windows N]"""
import argparse
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))
import deepgemm_ascend_amd as dga  # noqa: E402
from cast_transposed_timing import alternate  # noqa: E402

CASES = [((32, 4096, 7168), torch.bfloat16), ((32, 4096, 7168), torch.float32), ((32, 7168, 2048), torch.bfloat16), ((4096, 4096), torch.bfloat16)]
SENTINEL_Q, SENTINEL_SF = 0xA5, 0x7FC0A5A5
REFERENCE = ROOT / "profiles" / "cast_transposed_timing.txt"


def forms(w, rowwise):
    lead, (n, k) = tuple(w.shape[:-2]), w.shape[-2:]
    nb, kb = (n + 127) // 128, (k + 127) // 128
    full = lambda shape: torch.full(shape, SENTINEL_Q, dtype=torch.uint8, device="cuda")
    scales = lambda shape: torch.full(shape, SENTINEL_SF, dtype=torch.int32, device="cuda").view(torch.float32)
    qt, sft = full(lead + (k, n)), scales(lead + (kb, nb))
    q, sf = (full(lead + (n, k)), scales(lead + (nb, kb))) if rowwise else (None, None)
    out = ((qt, sft), (q, sf)) if rowwise else (qt, sft)

    def new():
        dga.per_block_cast_to_fp8_transposed(w, rowwise=rowwise, out=out)

    def old():
        if not lead:
            r = dga.per_block_cast_to_fp8(w.t().contiguous())
            return r + dga.per_block_cast_to_fp8(w) if rowwise else r
        t = [dga.per_block_cast_to_fp8(w[g].t().contiguous()) for g in range(lead[0])]
        r = (torch.stack([a for a, _ in t]), torch.stack([b for _, b in t]))
        if rowwise:
            p = [dga.per_block_cast_to_fp8(w[g]) for g in range(lead[0])]
            r += (torch.stack([a for a, _ in p]), torch.stack([b for _, b in p]))
        return r

    return new, old, (qt, sft, q, sf)


def check(name, new, old, outs, rowwise):
    new()
    want = old()
    torch.cuda.synchronize()
    for got, ref, what in zip(outs, want, ("qt", "sft", "q", "sf")):
        bits = torch.uint8 if what in ("qt", "q") else torch.int32
        assert got.shape == ref.shape and torch.equal(got.view(bits), ref.view(bits)), f"{name}: {what} differs from the old path's"
    assert len(want) == (4 if rowwise else 2)


def reference_figures():
    """The transposing activation quantiser's TB/s as its profile holds them: (lowest, highest) over its [32768, .] cases."""
    tb = []
    if REFERENCE.exists():
        for line in REFERENCE.read_text().splitlines():
            if line.startswith("[32768") and "TB/s" in line:
                tb.append(float(line.split("TB/s")[0].split()[-1]))
    return (min(tb), max(tb)) if tb else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=4)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    fmt = lambda v: f"{v.mean():9.1f} [{v.min():9.1f}..{v.max():9.1f}] us"
    say(f"# {torch.cuda.get_device_name(0)}; new = per_block_cast_to_fp8_transposed(out=...), old = per expert per_block_cast_to_fp8(w[g].t().contiguous()) "
        f"(+ per_block_cast_to_fp8(w[g]) with rowwise) + torch.stack")
    say(f"# device events around windows of back-to-back calls (>= 150 ms each), {args.windows} windows per form, alternating; mean [min..max] us "
        f"per call; traffic ratio: bf16 3/7 = 0.43 (rowwise 4/10 = 0.40), fp32 5/13 = 0.38 (rowwise 6/18 = 0.33), the stacks' 2 bytes per output element not counted")
    ref = reference_figures()
    if ref:
        say(f"# for comparison: per_token_cast_to_fp8_transposed on [32768, .] bf16 runs at {ref[0]:.2f}-{ref[1]:.2f} TB/s of its one-pass bytes "
            f"(profiles/cast_transposed_timing.txt)")
    for shape, dtype in CASES:
        g = torch.Generator(device="cuda").manual_seed(sum(shape))
        w = torch.empty(shape, dtype=dtype, device="cuda")
        for part in (w if len(shape) == 3 else [w]):                     # (group by group: no fp32 temporary of the whole tensor)
            part.copy_(torch.randn(part.shape, device="cuda", generator=g) * 3.0)
        tag = {torch.bfloat16: "bf16", torch.float32: "fp32"}[dtype]
        for rowwise in (False, True):
            name = f"{list(shape)} {tag}{' rowwise' if rowwise else ''}"
            new, old, outs = forms(w, rowwise)
            check(name, new, old, outs, rowwise)
            t = alternate([new, old], args.windows)
            per_elem = w.element_size() + (2 if rowwise else 1)
            tb = w.numel() * per_elem / (t[new].mean() * 1e-6) / 1e12
            say(f"{name:34s} | new {fmt(t[new])} {tb:5.2f} TB/s | old {fmt(t[old])} | new / old {t[new].mean() / t[old].mean():5.2f}")
            del new, old, outs
            torch.cuda.empty_cache()
        del w
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
