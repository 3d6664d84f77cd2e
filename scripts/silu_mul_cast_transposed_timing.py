"""Times silu_and_mul_per_token_cast_to_fp8_transposed (one pass over gate_up) against the path a user had without it: torch
F.silu(gate) * up in bf16 followed by per_token_cast_to_fp8_transposed (same mask), plus silu_and_mul_per_token_cast_to_fp8 for the
rowwise=True case.  Both run alternately in one process on the same tensors, in windows of back-to-back calls between two device events
(each window sized to well over 150 ms after a calibration), after a warm-up; mean and min..max over the windows.  Before any time is
reported the new entry's outputs pass, on SAMPLE channels spread over H, checks 1 and 3 of tests/test_silu_mul_cast_transposed_gpu.py:
exact-family inputs against oracle.quant_1x128 on the transpose of fl32(gate * up) byte for byte, and tolerance-family inputs (the timed
tensor) under the forward's scale and code bounds and its cap on the share off the oracle; the row-wise output equals the forward
quantiser's on the valid rows, and the rows a mask excludes hold their sentinels.
Cases (bf16): [32768, 2 * 2048] plain, with a random contiguous-layout m_indices (8 experts, every segment padded to 128 rows) and with
rowwise; [4096, 2 * 4096].  TB/s = the bytes one pass needs, 5 per element of h (6 with rowwise), over the new entry's time.
Usage: python scripts/silu_mul_cast_transposed_timing.py [--out profiles/silu_mul_cast_transposed_timing.txt] [--windows N]"""
import argparse
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "scripts"))
import deepgemm_ascend_amd as dga  # noqa: E402
from cast_transposed_timing import alternate, contiguous_m_indices  # noqa: E402

CASES = [(32768, 2048, False, False), (32768, 2048, True, False), (32768, 2048, False, True), (4096, 4096, False, False)]
SENTINEL_Q, SENTINEL_SF = 0xA5, 0x7FC0A5A5
SAMPLE = 96


def outputs(t_n, h, rowwise):
    qt = torch.full((h, t_n), SENTINEL_Q, dtype=torch.uint8, device="cuda")
    sft = torch.full((h, t_n // 128), SENTINEL_SF, dtype=torch.int32, device="cuda").view(torch.float32)
    q = torch.full((t_n, h), SENTINEL_Q, dtype=torch.uint8, device="cuda")
    sf = torch.full((t_n, (h + 127) // 128), SENTINEL_SF, dtype=torch.int32, device="cuda").view(torch.float32)
    return qt, sft, q, sf, (((qt, sft), (q, sf)) if rowwise else (qt, sft))


def forms(x, idx, rowwise):
    t_n, h = x.shape[0], x.shape[1] // 2
    qt, sft, q, sf, out = outputs(t_n, h, rowwise)

    def new():
        dga.silu_and_mul_per_token_cast_to_fp8_transposed(x, m_indices=idx, rowwise=rowwise, out=out)

    def old():
        hh = torch.nn.functional.silu(x[:, :h]) * x[:, h:]
        r = dga.per_token_cast_to_fp8_transposed(hh, m_indices=idx)
        return r + dga.silu_and_mul_per_token_cast_to_fp8(x, m_indices=idx) if rowwise else r

    return new, old, (qt, sft, q, sf)


def check(name, x, idx, rowwise, new, outs):
    from oracle import oracle
    from test_silu_mul_cast_gpu import _check_tolerance, _exact_inputs, _h_ref, _share_off_the_oracle
    oracle.build()
    qt, sft, q, sf = outs
    t_n, h = x.shape[0], x.shape[1] // 2
    valid = torch.ones(t_n, dtype=torch.bool, device="cuda") if idx is None else idx >= 0
    pick = torch.from_numpy(np.linspace(0, h - 1, SAMPLE).astype(np.int64)).cuda()
    vnp = valid.cpu().numpy()
    # check 1: exact-family inputs of the same shape and mask, the sampled channels byte for byte
    xe, gate, up = _exact_inputs((t_n,), h, torch.bfloat16, seed=t_n + h)
    eqt, esft, _, _, eout = outputs(t_n, h, False)
    dga.silu_and_mul_per_token_cast_to_fp8_transposed(xe, m_indices=idx, out=eout, sync=True)
    prod = (gate[:, pick].float() * up[:, pick].float()).cpu().numpy()
    wq, wsf = oracle.quant_1x128(np.ascontiguousarray(np.where(vnp[:, None], prod, np.float32(0.0)).T))
    assert (eqt[pick].cpu().numpy() == wq).all() and (esft[pick].cpu().numpy().view(np.uint32) == wsf.view(np.uint32)).all(), \
        f"{name}: the exact family differs from the oracle"
    del xe, gate, up, eqt, esft, eout
    # check 3: the timed (tolerance-family) tensor, the sampled channels
    new()
    torch.cuda.synchronize()
    href = np.where(vnp[:, None], _h_ref(x[:, :h][:, pick], x[:, h:][:, pick]), np.float32(0.0))
    href_t = np.ascontiguousarray(href.T)
    gq, gsf = qt[pick].cpu().numpy(), sft[pick].cpu().numpy()
    _check_tolerance(oracle, gq, gsf, href_t, False, np.arange(SAMPLE), name)
    assert _share_off_the_oracle(oracle, gq, gsf, href_t, False, name) <= 1e-3
    if rowwise:
        fq, fsf = dga.silu_and_mul_per_token_cast_to_fp8(x, m_indices=idx, sync=True)
        assert torch.equal(q[valid], fq.view(torch.uint8)[valid]) and torch.equal(sf[valid].view(torch.int32), fsf[valid].view(torch.int32)), \
            f"{name}: (q, sf) differ from the forward quantiser's"
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
    say(f"# {torch.cuda.get_device_name(0)}; bf16; new = silu_and_mul_per_token_cast_to_fp8_transposed(out=...), old = F.silu(gate) * up (bf16) -> "
        f"per_token_cast_to_fp8_transposed (+ silu_and_mul_per_token_cast_to_fp8 with rowwise), same mask")
    say(f"# device events around windows of back-to-back calls (>= 150 ms each), {args.windows} windows per form, alternating; mean [min..max] us "
        f"per call; TB/s over 5 H T bytes (rowwise: 6 H T)")
    for t_n, h, masked, rowwise in CASES:
        g = torch.Generator(device="cuda").manual_seed(t_n + h)
        gate = (torch.randn((t_n, h), device="cuda", generator=g) * 3.0).clamp(-16.0, 16.0).bfloat16()
        up = (torch.randn((t_n, h), device="cuda", generator=g) * 3.0).bfloat16()
        x = torch.cat([gate, up], dim=-1).contiguous()
        del gate, up
        idx = torch.from_numpy(contiguous_m_indices(t_n)).cuda() if masked else None
        if masked:
            x[idx < 0] = float("nan")
        name = f"[{t_n}, 2*{h}]{' m_indices' if masked else ''}{' rowwise' if rowwise else ''}"
        new, old, outs = forms(x, idx, rowwise)
        check(name, x, idx, rowwise, new, outs)
        t = alternate([new, old], args.windows)
        tb = t_n * h * (6 if rowwise else 5) / (t[new].mean() * 1e-6) / 1e12
        say(f"{name:36s} | new {fmt(t[new])} {tb:5.2f} TB/s | old {fmt(t[old])} | new / old {t[new].mean() / t[old].mean():5.2f}")
        del new, old, outs, x
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
