"""Times silu_and_mul_backward_per_token_cast_to_fp8_transposed(rowwise=True) (one pass over gate_up and grad_h) against the pair it
replaces: silu_and_mul_backward_per_token_cast_to_fp8(grad_x_out=dY1) followed by per_token_cast_to_fp8_transposed(dY1), same mask.  Both
run alternately in one process on the same tensors, in windows of back-to-back calls between two device events (each window sized to well
over 150 ms after a calibration), after a warm-up; mean and min..max over the windows.  Before any time is reported the outputs are
compared byte for byte: (dq, dsf) with the pair's on the valid rows (the rows a mask excludes hold their sentinels), and (dqt, dsft) with
per_token_cast_to_fp8_transposed of the fp32 gradient the existing entry writes for the up-converted inputs -- the contract by composition.
(The pair's own dY1^T operand is NOT the same bytes for the 16-bit types: it quantises a gradient rounded to 16 bits.)
Cases: bf16 [32768, 2 * 2048] plain and with a random contiguous-layout m_indices (8 experts, every segment padded to 128 rows),
bf16 [4096, 2 * 4096], fp32 [32768, 2 * 2048].  TB/s = the bytes one pass needs per (gate, up) pair, three input elements and four code bytes
(bf16: 10 H T; the scales are not counted), over the new entry's time.  A case whose slowest new window is not below the pair's fastest
is marked NOT faster.
Usage: python scripts/silu_mul_bwd_cast_transposed_timing.py [--out profiles/silu_mul_bwd_cast_transposed_timing.txt] [--windows N]"""
import argparse
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))
import deepgemm_ascend_amd as dga  # noqa: E402
from cast_transposed_timing import alternate, contiguous_m_indices  # noqa: E402

CASES = [(32768, 2048, False, torch.bfloat16), (32768, 2048, True, torch.bfloat16), (4096, 4096, False, torch.bfloat16),
         (32768, 2048, False, torch.float32)]
SENTINEL_Q, SENTINEL_SF = 0xA5, 0x7FC0A5A5


def outputs(t_n, h):
    qt = torch.full((2 * h, t_n), SENTINEL_Q, dtype=torch.uint8, device="cuda")
    sft = torch.full((2 * h, t_n // 128), SENTINEL_SF, dtype=torch.int32, device="cuda").view(torch.float32)
    q = torch.full((t_n, 2 * h), SENTINEL_Q, dtype=torch.uint8, device="cuda")
    sf = torch.full((t_n, 2 * h // 128), SENTINEL_SF, dtype=torch.int32, device="cuda").view(torch.float32)
    return qt, sft, q, sf


def forms(x, grad, idx):
    t_n, h = grad.shape
    qt, sft, q, sf = outputs(t_n, h)
    oqt, osft, oq, osf = outputs(t_n, h)
    dy1 = torch.empty_like(x)

    def new():
        dga.silu_and_mul_backward_per_token_cast_to_fp8_transposed(x, grad, m_indices=idx, rowwise=True, out=((qt, sft), (q, sf)))

    def old():
        dga.silu_and_mul_backward_per_token_cast_to_fp8(x, grad, m_indices=idx, out=(oq, osf), grad_x_out=dy1)
        dga.per_token_cast_to_fp8_transposed(dy1, m_indices=idx, out=(oqt, osft))

    return new, old, (qt, sft, q, sf), (oqt, osft, oq, osf)


def check(name, x, grad, idx, new, old, outs, old_outs):
    qt, sft, q, sf = outs
    oqt, osft, oq, osf = old_outs
    new()
    old()
    torch.cuda.synchronize()
    valid = torch.ones(q.shape[0], dtype=torch.bool, device="cuda") if idx is None else idx >= 0
    assert torch.equal(q[valid], oq[valid]) and torch.equal(sf[valid].view(torch.int32), osf[valid].view(torch.int32)), \
        f"{name}: (dq, dsf) differ from the existing entry's"
    assert bool((q[~valid] == SENTINEL_Q).all()) and bool((sf[~valid].view(torch.int32) == SENTINEL_SF).all()), f"{name}: an excluded row was written"
    big_g = torch.full(x.shape, float("nan"), dtype=torch.float32, device="cuda")
    dga.silu_and_mul_backward_per_token_cast_to_fp8(x.float(), grad.float(), m_indices=idx, grad_x_out=big_g)
    wqt, wsft = dga.per_token_cast_to_fp8_transposed(big_g, m_indices=idx, sync=True)
    assert torch.equal(qt, wqt.view(torch.uint8)) and torch.equal(sft.view(torch.int32), wsft.view(torch.int32)), \
        f"{name}: (dqt, dsft) differ from the composition"
    if x.dtype == torch.float32:      # (fp32 inputs: the pair quantises the same unrounded gradient)
        assert torch.equal(qt, oqt) and torch.equal(sft.view(torch.int32), osft.view(torch.int32)), f"{name}: (dqt, dsft) differ from the pair's"
    return float((qt != oqt).float().mean())


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
    say(f"# {torch.cuda.get_device_name(0)}; new = silu_and_mul_backward_per_token_cast_to_fp8_transposed(rowwise=True, out=...), old = "
        f"silu_and_mul_backward_per_token_cast_to_fp8(grad_x_out=dY1) -> per_token_cast_to_fp8_transposed(dY1), same mask")
    say(f"# device events around windows of back-to-back calls (>= 150 ms each), {args.windows} windows per form, alternating; mean [min..max] us "
        f"per call; TB/s over (3 s + 4) H T bytes, s the size of an input element (bf16: 10 H T; the pair moves 18 H T); codes off the pair's: "
        f"the share of dqt's bytes that differ from the pair's operand, which quantises the gradient rounded to 16 bits")
    for t_n, h, masked, dtype in CASES:
        g = torch.Generator(device="cuda").manual_seed(t_n + h)
        gate = (torch.randn((t_n, h), device="cuda", generator=g) * 3.0).clamp(-16.0, 16.0).to(dtype)
        up = (torch.randn((t_n, h), device="cuda", generator=g) * 3.0).to(dtype)
        grad = (torch.randn((t_n, h), device="cuda", generator=g) * 0.5).to(dtype).contiguous()
        x = torch.cat([gate, up], dim=-1).contiguous()
        del gate, up
        idx = torch.from_numpy(contiguous_m_indices(t_n)).cuda() if masked else None
        if masked:
            x[idx < 0] = float("nan")
            grad[idx < 0] = float("nan")
        name = f"{str(dtype)[6:]} [{t_n}, 2*{h}]{' m_indices' if masked else ''}"
        new, old, outs, old_outs = forms(x, grad, idx)
        off = check(name, x, grad, idx, new, old, outs, old_outs)
        t = alternate([new, old], args.windows)
        tb = t_n * h * (3 * x.element_size() + 4) / (t[new].mean() * 1e-6) / 1e12
        faster = "faster" if t[new].max() < t[old].min() else "NOT faster beyond the spread"
        say(f"{name:36s} | new {fmt(t[new])} {tb:5.2f} TB/s | old {fmt(t[old])} | new / old {t[new].mean() / t[old].mean():5.2f} ({faster}) | "
            f"codes off the pair's {off:.3e}")
        del new, old, outs, old_outs, x, grad
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
