"""Times the MoE dispatch / combine entries against what they replace, to scripts/cast_transposed_timing.py's protocol: old and new run
alternately in one process on the same tensors, in windows of back-to-back calls between two device events (each window sized to well over
100 ms after a calibration), after a warm-up; mean and min..max over the windows.  Before any time is reported the quantisers' outputs are
compared with the old path's byte for byte (whole qt / sft; (q, sf) on the valid rows, sentinels on the others); the combine and the weight
gradient are not the arithmetic of the torch expressions they replace (a stated order against torch's), so they are compared under the
bound of a float32 sum of their terms.
Cases (bf16), T tokens x H, k = 8 choices of 32 experts, contiguous layout (every expert's segment padded to 128 rows, index -1 on padding):
  dispatch   gather_per_token_cast_to_fp8_transposed(x, index, index_div=8)  against  x.index_select(0, token) + per_token_cast_to_fp8_transposed(xg, m_indices)
  identity   the same entry on the gathered tensor with index = arange        against  per_token_cast_to_fp8_transposed itself
  combine    combine_tokens(out, dest, w)                                     against  (src[dest.clamp(0)] * w[..., None]).masked_fill(dest[..., None] < 0, 0).sum(1)
  wgrad      combine_tokens_weight_grad(out, dy, dest)                        against  its einsum
Usage: python scripts/moe_permute_timing.py [--out profiles/moe_permute_timing.txt] [--windows N]"""
import argparse
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import deepgemm_ascend_amd as dga  # noqa: E402
from scripts.cast_transposed_timing import SENTINEL_Q, SENTINEL_SF, alternate  # noqa: E402

SHAPES = [(4096, 7168), (16384, 2048)]
K, EXPERTS = 8, 32


def routing(t_n, seed=7):
    """Every token picks K distinct experts.  Returns (index int64 [slots]: the pair t * K + j of a slot, -1 on the padding rows;
    m_indices int32 [slots]; dest int64 [t_n, K]: the slot of a pair)."""
    rng = np.random.default_rng(seed)
    ids = np.argsort(rng.random((t_n, EXPERTS)), axis=1)[:, :K].reshape(-1)
    order = np.argsort(ids, kind="stable")
    counts = np.bincount(ids, minlength=EXPERTS)
    padded = (counts + 127) // 128 * 128
    start = np.r_[0, np.cumsum(padded)[:-1]]
    slots = int(padded.sum())
    index, m_indices = np.full(slots, -1, np.int64), np.full(slots, -1, np.int32)
    dest = np.empty(t_n * K, np.int64)
    first = np.r_[0, np.cumsum(counts)[:-1]]
    for g in range(EXPERTS):
        pairs = order[first[g]:first[g] + counts[g]]
        index[start[g]:start[g] + counts[g]] = pairs
        m_indices[start[g]:start[g] + counts[g]] = g
        dest[pairs] = start[g] + np.arange(counts[g])
    return index, m_indices, dest.reshape(t_n, K)


def cast_outputs(slots, h):
    qt = torch.full((h, slots), SENTINEL_Q, dtype=torch.uint8, device="cuda")
    sft = torch.full((h, slots // 128), SENTINEL_SF, dtype=torch.int32, device="cuda").view(torch.float32)
    q = torch.full((slots, h), SENTINEL_Q, dtype=torch.uint8, device="cuda")
    sf = torch.full((slots, (h + 127) // 128), SENTINEL_SF, dtype=torch.int32, device="cuda").view(torch.float32)
    return qt, sft, q, sf


def check_cast(name, new, old, outs, valid, rowwise):
    qt, sft, q, sf = outs
    new()
    want = old()
    torch.cuda.synchronize()
    wt = want[0] if rowwise else want
    assert torch.equal(qt, wt[0].view(torch.uint8)) and torch.equal(sft.view(torch.int32), wt[1].view(torch.int32)), f"{name}: (qt, sft) differ"
    if rowwise:
        wq, wsf = want[1]
        assert torch.equal(q[valid], wq.view(torch.uint8)[valid]) and torch.equal(sf[valid], wsf[valid]), f"{name}: (q, sf) differ"
        assert bool((q[~valid] == SENTINEL_Q).all()) and bool((sf[~valid].view(torch.int32) == SENTINEL_SF).all()), f"{name}: an excluded row was written"


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
    say(f"# {torch.cuda.get_device_name(0)}; bf16; k = {K}, {EXPERTS} experts, contiguous layout; device events around windows of back-to-back calls "
        f"(>= 150 ms each), {args.windows} windows per form, alternating; mean [min..max] us per call")
    for t_n, h in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(t_n + h)
        x = (torch.randn((t_n, h), device="cuda", generator=g) * 3.0).bfloat16()
        index_np, mi_np, dest_np = routing(t_n)
        slots = index_np.size
        index, m_indices, dest = (torch.from_numpy(a).cuda() for a in (index_np, mi_np, dest_np))
        valid = index >= 0
        token = torch.where(valid, index // K, torch.zeros_like(index))
        say(f"## x [{t_n}, {h}]: {t_n * K} pairs in {slots} slots")
        for rowwise in (False, True):
            outs = cast_outputs(slots, h)
            out = ((outs[0], outs[1]), (outs[2], outs[3])) if rowwise else (outs[0], outs[1])
            new = lambda: dga.gather_per_token_cast_to_fp8_transposed(x, index, index_div=K, rowwise=rowwise, out=out)
            old = lambda: dga.per_token_cast_to_fp8_transposed(x.index_select(0, token), m_indices=m_indices, rowwise=rowwise)
            name = f"dispatch{' rowwise' if rowwise else ''}"
            check_cast(name, new, old, outs, valid, rowwise)
            t = alternate([new, old], args.windows)
            tb = slots * h * (4 if rowwise else 3) / (t[new].mean() * 1e-6) / 1e12
            say(f"{name:20s} | new {fmt(t[new])} {tb:5.2f} TB/s | old {fmt(t[old])} | new / old {t[new].mean() / t[old].mean():5.2f}")
            del new, old, outs, out
        xg = x.index_select(0, token)
        ident = torch.arange(slots, dtype=torch.int64, device="cuda")
        everything = torch.ones(slots, dtype=torch.bool, device="cuda")
        for rowwise in (False, True):
            outs = cast_outputs(slots, h)
            out = ((outs[0], outs[1]), (outs[2], outs[3])) if rowwise else (outs[0], outs[1])
            outs_old = cast_outputs(slots, h)
            out_old = ((outs_old[0], outs_old[1]), (outs_old[2], outs_old[3])) if rowwise else (outs_old[0], outs_old[1])
            new = lambda: dga.gather_per_token_cast_to_fp8_transposed(xg, ident, rowwise=rowwise, out=out)
            old = lambda: dga.per_token_cast_to_fp8_transposed(xg, rowwise=rowwise, out=out_old)
            name = f"identity{' rowwise' if rowwise else ''}"
            check_cast(name, new, old, outs, everything, rowwise)
            t = alternate([new, old], args.windows)
            say(f"{name:20s} | new {fmt(t[new])}            | old {fmt(t[old])} | new / old {t[new].mean() / t[old].mean():5.2f}  (condition: <= 1.10)")
            del new, old, outs, out, outs_old, out_old
        del xg
        # combine and its weight gradient on a [slots, h] expert output
        src = (torch.randn((slots, h), device="cuda", generator=g)).bfloat16()
        src[~valid] = float("nan")
        w = torch.rand((t_n, K), device="cuda", generator=g) + 0.05
        dy = torch.randn((t_n, h), device="cuda", generator=g).bfloat16()
        y = torch.empty((t_n, h), dtype=torch.float32, device="cuda")
        new = lambda: dga.combine_tokens(src, dest, w, out=y)
        old = lambda: (src[dest.clamp(0)] * w[..., None]).masked_fill(dest[..., None] < 0, 0).sum(1)
        new()
        want = old()
        bound = K * 2.0 ** -23 * (src[dest].float().abs() * w[..., None]).sum(1)
        assert bool(((y - want).abs() <= bound).all()), "combine: outside the bound of a float32 sum of k products"
        del want, bound
        t = alternate([new, old], args.windows)
        tb = (t_n * K * h * 2 + t_n * h * 4) / (t[new].mean() * 1e-6) / 1e12
        say(f"{'combine (fp32 out)':20s} | new {fmt(t[new])} {tb:5.2f} TB/s | old {fmt(t[old])} | new / old {t[new].mean() / t[old].mean():5.2f}")
        dw = torch.empty((t_n, K), dtype=torch.float32, device="cuda")
        new = lambda: dga.combine_tokens_weight_grad(src, dy, dest, out=dw)
        old = lambda: torch.einsum("tkh,th->tk", src[dest].float(), dy.float())
        new()
        want = old()
        bound = (h + 2) * 2.0 ** -23 * torch.einsum("tkh,th->tk", src[dest].float().abs(), dy.float().abs())
        assert bool(((dw - want).abs() <= bound).all()), "weight gradient: outside the bound of two float32 sums of h products"
        del want, bound
        t = alternate([new, old], args.windows)
        tb = (t_n * K * h * 2 + t_n * h * 2) / (t[new].mean() * 1e-6) / 1e12
        say(f"{'weight gradient':20s} | new {fmt(t[new])} {tb:5.2f} TB/s | old {fmt(t[old])} | new / old {t[new].mean() / t[old].mean():5.2f}")
        del new, old, x, src, w, dy, y, dw
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
