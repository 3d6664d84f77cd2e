"""Times router_topk against the torch expression it replaces, to scripts/moe_permute_timing.py's protocol: both forms run alternately in
one process on the same tensors, in windows of back-to-back calls between two device events (each window sized to well over 100 ms after a
calibration), after a warm-up; mean and min..max over the windows.  Before any time is reported the results are compared: the scores
element by element, the chosen sets row by row (the two forms round their scores differently, so a row whose k-th and (k+1)-th values
nearly tie may differ: at most 0.1 % of the rows), the weights on the rows that agree.
Cases: T = 4096 and 32768 tokens, E = 256 experts, k = 8, bf16 and fp32 logits,
  softmax          softmax(logits.float()) -> topk -> normalise
  sigmoid groups   DeepSeek-V3's gate: sigmoid -> + bias -> 8 groups valued by their two largest -> the 4 largest groups -> topk of what
                   they hold -> the unbiased scores gathered and normalised, times 2.5
The condition: the entry is not slower than the torch expression on any case (new / torch <= 1.0).  The TB/s column is the entry's
E * (input bytes + 4) + 8 k bytes per token over its time.
Usage: python scripts/router_topk_timing.py [--out profiles/router_topk_timing.txt] [--windows N]"""
import argparse
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import deepgemm_ascend_amd as dga  # noqa: E402
from scripts.cast_transposed_timing import alternate  # noqa: E402

TOKENS, E, K = (4096, 32768), 256, 8
N_GROUPS, TOPK_GROUPS, SCALE = 8, 4, 2.5


def torch_softmax(logits):
    s = torch.softmax(logits.float(), dim=-1)
    v, ids = torch.topk(s, K, dim=-1)
    return ids, v / v.sum(dim=-1, keepdim=True), s


def torch_sigmoid_groups(logits, bias):
    t_n = logits.shape[0]
    s = torch.sigmoid(logits.float())
    sel = s + bias
    group_value = sel.view(t_n, N_GROUPS, -1).topk(2, dim=-1).values.sum(dim=-1)
    kept = torch.zeros_like(group_value, dtype=torch.bool).scatter_(1, group_value.topk(TOPK_GROUPS, dim=-1).indices, True)
    allowed = kept[:, :, None].expand(t_n, N_GROUPS, E // N_GROUPS).reshape(t_n, E)
    ids = sel.masked_fill(~allowed, float("-inf")).topk(K, dim=-1).indices
    r = s.gather(1, ids)
    return ids, r / r.sum(dim=-1, keepdim=True) * SCALE, s


def compare(name, new, old):
    ids, w, s = new()
    tids, tw, ts = old()
    torch.cuda.synchronize()
    assert torch.allclose(s, ts, rtol=1e-4, atol=1e-9), f"{name}: the scores differ"
    order, torder = ids.long().sort(dim=1), tids.sort(dim=1)
    same = (order.values == torder.values).all(dim=1)
    assert float((~same).float().mean()) <= 1e-3, f"{name}: {int((~same).sum())} rows choose another set"
    assert torch.allclose(w.gather(1, order.indices)[same], tw.gather(1, torder.indices)[same], rtol=1e-4, atol=1e-9), f"{name}: the weights differ"
    return int((~same).sum())


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
    say(f"# {torch.cuda.get_device_name(0)}; E = {E}, k = {K}; device events around windows of back-to-back calls (>= 150 ms each), "
        f"{args.windows} windows per form, alternating; mean [min..max] us per call; condition: new / torch <= 1.00")
    slower = []
    for t_n in TOKENS:
        for dtype in (torch.bfloat16, torch.float32):
            g = torch.Generator(device="cuda").manual_seed(t_n)
            logits = (torch.randn((t_n, E), device="cuda", generator=g) * 2.0).to(dtype)
            bias = torch.randn((E,), device="cuda", generator=g) * 0.05
            out = (torch.empty((t_n, K), dtype=torch.int32, device="cuda"), torch.empty((t_n, K), dtype=torch.float32, device="cuda"),
                   torch.empty((t_n, E), dtype=torch.float32, device="cuda"))
            forms = {"softmax": (lambda: dga.router_topk(logits, K, out=out), lambda: torch_softmax(logits)),
                     "sigmoid groups": (lambda: dga.router_topk(logits, K, score_func="sigmoid", bias=bias, n_groups=N_GROUPS,
                                                                topk_groups=TOPK_GROUPS, scale=SCALE, out=out),
                                        lambda: torch_sigmoid_groups(logits, bias))}
            for form, (new, old) in forms.items():
                name = f"[{t_n}, {E}] {str(dtype).split('.')[-1]:8s} {form:14s}"
                other = compare(name, new, old)
                t = alternate([new, old], args.windows)
                tb = t_n * (E * (logits.element_size() + 4) + 8 * K) / (t[new].mean() * 1e-6) / 1e12
                ratio = t[new].mean() / t[old].mean()
                say(f"{name} | new {fmt(t[new])} {tb:5.2f} TB/s | torch {fmt(t[old])} | new / torch {ratio:5.2f} | rows with another set: {other}")
                if ratio > 1.0:
                    slower.append(name)
            del logits, bias, out, forms
            torch.cuda.empty_cache()
    say("# slower than the torch expression: " + ("; ".join(" ".join(n.split()) for n in slower) if slower else "no case"))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
