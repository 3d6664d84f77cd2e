"""Times split-topk sparse MLA decode, by the method of scripts/sparse_mla_timing.py: the forms of a case run alternately in one process on
the same operands, in windows of back-to-back calls between two device events (each window sized to over 150 ms after a calibration, at
least 3 calls), after a warm-up; mean and min..max over the windows.  Results are compared before any time is reported: num_splits = 1 and
the rule's choice of 1 byte for byte against the one-pass operator, every other split count within 2^-6 of it (the tests hold the bound).
topk = 2048, Hq = 128, bf16 normal samples, sm_scale = 576^-0.5, both caches (the fp8 one in pages of 64 rows).
  1. sweep   sparse_mla_fwd_split(num_splits = P), P in 1, 2, 4, ..., 64, at M in 1, 4, 16, 64 tokens over S = 65536 rows, and the one-pass
             operator beside them: the table DGA_SPARSE_MLA_MIN_TILES is chosen from (2048 / 32 / P tiles a split)
  2. rule    sparse_mla_fwd_split(num_splits = None) against the one-pass operator.  Conditions, set before the run: at M = 1 and at
             decode B = 16 (next_n = 2) the slowest split window is faster than the fastest one-pass window; at decode B = 128 and at
             the prefill case the rule returns 1 and the call is the one-pass launch
  3. parent  with --parent-lib: dga_sparse_mla_fwd and dga_sparse_mla_fwd_fp8 of the parent commit's libdga_hip.so loaded beside this one,
             on the same operands: the one-pass kernels must be what they were (min new <= max parent at every case)
Usage: python scripts/sparse_mla_split_timing.py [--out profiles/sparse_mla_split_timing.txt] [--windows N] [--parent-lib PATH]"""
import argparse
import ctypes
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import deepgemm_ascend_amd as dga  # noqa: E402
from deepgemm_ascend_amd import _lib  # noqa: E402
from scripts.indexer_topk_timing import alternate  # noqa: E402
from scripts.sparse_mla_fp8_timing import write_cache  # noqa: E402
from scripts.sparse_mla_timing import D, DV, SCALE, TOPK, decode_case, prefill_case  # noqa: E402

H = 128
SPLITS = (1, 2, 4, 8, 16, 32, 64)


def random_lists(m, s, gen):
    """indices int32 [m, 2048]: 2048 distinct rows of [0, s) per token, ascending, all valid"""
    return torch.rand((m, s), device="cuda", generator=gen).topk(TOPK, dim=1).indices.sort(dim=1).values.to(torch.int32)


def outputs(m, n):
    return [(torch.empty((m, H, DV), dtype=torch.bfloat16, device="cuda"), torch.empty((m, H), dtype=torch.float32, device="cuda")) for _ in range(n)]


def same(a, b):
    return torch.equal(a[0].view(torch.int16), b[0].view(torch.int16)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def close(a, b):
    return bool(((a[0].float() - b[0].float()).abs() <= 2.0 ** -6).all()) and bool(((a[1] - b[1]).abs() <= 1e-4).all())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    fmt = lambda v: f"{v.mean():7.1f} [{v.min():7.1f}..{v.max():7.1f}]"
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    say(f"# {torch.cuda.get_device_name(0)}, {cus} CUs; topk = {TOPK}, Hq = {H}; device events around windows of back-to-back calls (>= 150 ms each, "
        f"at least 3 calls), {args.windows} windows per form, alternating; results compared first; mean [min..max] us per call")
    gen = torch.Generator(device="cuda").manual_seed(1)
    forms = (("bf16", dga.sparse_mla_fwd, dga.sparse_mla_fwd_split), ("fp8 ", dga.sparse_mla_fwd_fp8, dga.sparse_mla_fwd_fp8_split))

    say(f"# 1. sweep: sparse_mla_fwd_split(num_splits = P) over S = 65536 rows, all {TOPK} positions valid; one-pass = the one-launch operator; "
        f"rule = what sparse_mla_num_splits returns (DGA_SPARSE_MLA_MIN_TILES = 4)")
    s = 65536
    cache, deq = write_cache(torch.randn((s, D), device="cuda", generator=gen).to(torch.bfloat16))
    for m in (1, 4, 16, 64):
        q = torch.randn((m, H, D), device="cuda", generator=gen).to(torch.bfloat16)
        idx = random_lists(m, s, gen)
        for name, one, split in forms:
            kv = deq if name == "bf16" else cache
            outs = outputs(m, len(SPLITS) + 1)
            fns = [lambda o=outs[0]: one(q, kv, idx, SCALE, out=o[0], lse=o[1])]
            fns += [lambda p=p, o=o: split(q, kv, idx, SCALE, num_splits=p, out=o[0], lse=o[1]) for p, o in zip(SPLITS, outs[1:])]
            for fn in fns:
                fn()
            torch.cuda.synchronize()
            assert same(outs[1], outs[0]) and all(close(o, outs[0]) for o in outs[2:]) and not torch.isnan(outs[0][1]).any(), (m, name)
            t = alternate(fns, args.windows)
            best = min(SPLITS, key=lambda p: t[fns[1 + SPLITS.index(p)]].mean())
            say(f"M={m:3d} {name} | one-pass {fmt(t[fns[0]])} | " + " | ".join(f"P={p:2d} {fmt(t[fn])}" for p, fn in zip(SPLITS, fns[1:])) +
                f" | best P={best}, rule P={dga.sparse_mla_num_splits(m, H, TOPK, 'cuda:0')}")
        del q, idx
    del cache, deq
    torch.cuda.empty_cache()

    say("# 2. rule: sparse_mla_fwd_split(num_splits = None) against the one-pass operator.  Conditions: max split < min one-pass at M = 1 and at "
        "decode B = 16; rule = 1 and the one-pass launch (same bytes) at decode B = 128 and at the prefill case")
    parent = None
    if args.parent_lib:
        lib = ctypes.CDLL(str(args.parent_lib))
        parent = {}
        for sym in ("dga_sparse_mla_fwd", "dga_sparse_mla_fwd_fp8"):
            fn = getattr(lib, sym)
            fn.restype, fn.argtypes = _lib.SIGNATURES[sym]
            parent[sym] = fn
    cases = (("decode M=1 S=65536", "lists", 1, 65536, True), ("decode B= 16 n2 ctx 1024..65536", "decode", 16, 0, True),
             ("decode B=128 n2 ctx 1024..65536", "decode", 128, 0, False), ("prefill M=4096 S=32768", "prefill", 4096, 32768, False))
    failed, slower, parent_lines = [], [], []
    for name, kind, count, s, splits in cases:
        if kind == "decode":
            idx, s = decode_case(count, 2, 1024, 65536, gen)
            m = count * 2
        else:
            m, idx = count, (prefill_case(count, s, gen) if kind == "prefill" else random_lists(count, s, gen))
        q = torch.randn((m, H, D), device="cuda", generator=gen).to(torch.bfloat16)
        cache, deq = write_cache(torch.randn((s, D), device="cuda", generator=gen).to(torch.bfloat16))
        rule = dga.sparse_mla_num_splits(m, H, TOPK, "cuda:0")
        for form, one, split in forms:
            kv = deq if form == "bf16" else cache
            outs = outputs(m, 3)
            f_one = lambda: one(q, kv, idx, SCALE, out=outs[0][0], lse=outs[0][1])
            f_split = lambda: split(q, kv, idx, SCALE, out=outs[1][0], lse=outs[1][1])
            fns = [f_one, f_split]
            if parent:
                stream = torch.cuda.current_stream().cuda_stream
                if form == "bf16":
                    def f_parent():
                        assert parent["dga_sparse_mla_fwd"](q.data_ptr(), deq.data_ptr(), idx.data_ptr(), None, m, H, s, D, TOPK, TOPK, float(SCALE), 0,
                                                            outs[2][0].data_ptr(), outs[2][1].data_ptr(), stream) == 0
                else:
                    def f_parent():
                        assert parent["dga_sparse_mla_fwd_fp8"](q.data_ptr(), cache.data_ptr(), idx.data_ptr(), None, m, H, cache.shape[0], cache.shape[1],
                                                                cache.stride(0), TOPK, TOPK, float(SCALE), 0, outs[2][0].data_ptr(),
                                                                outs[2][1].data_ptr(), stream) == 0
                fns.append(f_parent)
            for fn in fns:
                fn()
            torch.cuda.synchronize()
            assert (close if rule > 1 else same)(outs[1], outs[0]) and not torch.isnan(outs[0][1]).any(), (name, form)
            assert not parent or same(outs[2], outs[0]), (name, form)
            t = alternate(fns, args.windows)
            ok = (rule > 1 and t[f_split].max() < t[f_one].min()) if splits else rule == 1
            if not ok:
                failed.append(f"{' '.join(name.split())} {form.strip()}")
            say(f"{name:32s} {form} | rule P={rule:2d} | one-pass {fmt(t[f_one])} | split {fmt(t[f_split])} | one-pass / split "
                f"{t[f_one].mean() / t[f_split].mean():5.2f} | " + ("split, within 2^-6" if rule > 1 else "the same launch, same bytes"))
            if parent:
                parent_lines.append(f"{name:32s} {form} | this build {fmt(t[f_one])} | parent {fmt(t[f_parent])} | this / parent "
                                    f"{t[f_one].mean() / t[f_parent].mean():6.3f}, same bytes")
                if not t[f_one].min() <= t[f_parent].max():
                    slower.append(f"{' '.join(name.split())} {form.strip()}")
        del q, cache, deq, idx
        torch.cuda.empty_cache()
    say("# cases where a condition does not hold: " + ("; ".join(failed) if failed else "none"))
    if parent:
        say("# 3. the one-pass kernels against the parent commit's build, loaded beside this one (condition: min this <= max parent at every case)")
        for line in parent_lines:
            say(line)
        say("# cases where the one-pass kernel is slower than the parent's beyond the spread: " + ("; ".join(slower) if slower else "none"))
    else:
        say("# no --parent-lib: the one-pass kernels were not timed against the parent commit's build")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
