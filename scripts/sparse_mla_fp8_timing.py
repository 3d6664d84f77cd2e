"""Times sparse_mla_fwd_fp8 and mla_kv_cast_to_fp8_paged, by the method of scripts/sparse_mla_timing.py: the forms of a case run alternately
in one process on the same operands, in windows of back-to-back calls between two device events (each window sized to over 150 ms after a
calibration, at least 3 calls), after a warm-up; mean and min..max over the windows.  Before any time is reported the results are compared
byte for byte.  topk = 2048, bf16 normal samples, sm_scale = 576^-0.5, the cache in pages of 64 rows.
Attention, per case:
  fp8     sparse_mla_fwd_fp8(q, cache, indices, ...) on the cache mla_kv_cast_to_fp8_paged wrote
  bf16    sparse_mla_fwd(q, deq(cache), indices, ...) with the same indices: what a user without the fp8 kernel runs after dequantising
  parent  with --parent-lib: dga_sparse_mla_fwd of another build of the library (the parent commit's libdga_hip.so) on the bf16 operands,
          loaded beside this one.  The bf16 kernel's text moved into code it shares with the fp8 kernel; the condition, set before the run,
          is that bf16 is not slower than parent beyond the windows' spread (min bf16 <= max parent) at every case.
Cases: the decode and prefill cases of scripts/sparse_mla_timing.py (decode B = 128, next_n = 2 over a paged cache; M = 1; prefill
M = 4096, S = 32768 at Hq = 128 and 64) and decode B = 16.  No target is set for fp8 / bf16: the ratio is reported as measured.
Writer, at 128 and 8192 tokens into a cache of 65536 rows:
  new     mla_kv_cast_to_fp8_paged(kv_c, k_pe, cache, slots)
  old     per_token_cast_to_fp8(kv_c), then three indexed assignments of codes, scales and rope bytes into the cache's rows
Usage: python scripts/sparse_mla_fp8_timing.py [--out profiles/sparse_mla_fp8_timing.txt] [--windows N] [--parent-lib PATH]"""
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
from scripts.sparse_mla_timing import D, DV, PAGE, SCALE, TOPK, decode_case, prefill_case  # noqa: E402

ROW = dga.SPARSE_MLA_FP8_ROW_BYTES


def write_cache(kv):
    """kv bf16 [s, 576], s a multiple of 64 -> (fp8 cache uint8 [s / 64, 64, 1, 656], its dequantised rows bf16 [s, 576])"""
    s = kv.shape[0]
    assert s % PAGE == 0
    cache = torch.zeros((s // PAGE, PAGE, 1, ROW), dtype=torch.uint8, device="cuda")
    dga.mla_kv_cast_to_fp8_paged(kv[:, :DV], kv[:, DV:], cache, torch.arange(s, dtype=torch.int64, device="cuda"), sync=True)
    rows = cache.view(s, ROW)
    deq = torch.empty((s, D), dtype=torch.bfloat16, device="cuda")
    for lo in range(0, s, 1 << 18):
        part = rows[lo:lo + (1 << 18)]
        scales = part[:, DV:DV + 16].contiguous().view(torch.float32)
        deq[lo:lo + len(part), :DV] = (part[:, :DV].contiguous().view(torch.float8_e4m3fn).float() * scales.repeat_interleave(128, -1)).to(torch.bfloat16)
        deq[lo:lo + len(part), DV:] = part[:, DV + 16:].contiguous().view(torch.bfloat16)
    return cache, deq


def parent_entry(path):
    lib = ctypes.CDLL(str(path))
    fn = lib.dga_sparse_mla_fwd
    fn.restype, fn.argtypes = _lib.SIGNATURES["dga_sparse_mla_fwd"]
    return fn


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

    fmt = lambda v: f"{v.mean():9.1f} [{v.min():9.1f}..{v.max():9.1f}] us"
    parent = parent_entry(args.parent_lib) if args.parent_lib else None
    say(f"# {torch.cuda.get_device_name(0)}; topk = {TOPK}; fp8 = sparse_mla_fwd_fp8 on the written cache, bf16 = sparse_mla_fwd on its dequantised rows, "
        f"parent = dga_sparse_mla_fwd of the parent commit's build on the same bf16 operands; device events around windows of back-to-back calls "
        f"(>= 150 ms each, at least 3 calls), {args.windows} windows per form, alternating; results byte-compared first; mean [min..max] us per call")
    say("# condition: bf16 not slower than parent beyond the spread (min bf16 <= max parent) at every case; fp8 / bf16 is reported, no target")
    gen = torch.Generator(device="cuda").manual_seed(1)
    cases = (("decode B=128 n2 ctx 1024..65536 Hq=128", "decode", 128, 0, 128),
             ("decode B= 16 n2 ctx 1024..65536 Hq=128", "decode", 16, 0, 128),
             ("decode M=1 S=65536 Hq=128", "prefill", 1, 65536, 128),
             ("prefill M=4096 S=32768 Hq=128", "prefill", 4096, 32768, 128),
             ("prefill M=4096 S=32768 Hq= 64", "prefill", 4096, 32768, 64))
    slower = []
    for name, kind, count, s, h in cases:
        if kind == "prefill":
            m, idx = count, prefill_case(count, s, gen)
        else:
            idx, s = decode_case(count, 2, 1024, 65536, gen)
            m = count * 2
        q = torch.randn((m, h, D), device="cuda", generator=gen).to(torch.bfloat16)
        cache, deq = write_cache(torch.randn((s, D), device="cuda", generator=gen).to(torch.bfloat16))
        outs = [(torch.empty((m, h, DV), dtype=torch.bfloat16, device="cuda"), torch.empty((m, h), dtype=torch.float32, device="cuda")) for _ in range(3)]
        fp8 = lambda: dga.sparse_mla_fwd_fp8(q, cache, idx, SCALE, out=outs[0][0], lse=outs[0][1])
        bf16 = lambda: dga.sparse_mla_fwd(q, deq, idx, SCALE, out=outs[1][0], lse=outs[1][1])
        fns = [fp8, bf16]
        if parent:
            def old():
                rc = parent(q.data_ptr(), deq.data_ptr(), idx.data_ptr(), None, m, h, s, D, TOPK, TOPK, float(SCALE), 0, outs[2][0].data_ptr(),
                            outs[2][1].data_ptr(), torch.cuda.current_stream().cuda_stream)
                assert rc == 0, rc
            fns.append(old)
        for fn in fns:
            fn()
        torch.cuda.synchronize()
        for o, l in outs[1:len(fns)]:
            assert torch.equal(o.view(torch.int16), outs[0][0].view(torch.int16)) and torch.equal(l.view(torch.int32), outs[0][1].view(torch.int32)), name
        assert not torch.isnan(outs[0][1]).any()
        t = alternate(fns, args.windows)
        valid = int((idx >= 0).sum())
        blocks = (h + 63) // 64
        line = (f"{name:40s} | fp8 {fmt(t[fp8])} | bf16 {fmt(t[bf16])} | fp8 / bf16 {t[fp8].mean() / t[bf16].mean():6.3f} | same bytes | gather "
                f"fp8 {valid * ROW * blocks / (t[fp8].mean() * 1e-6) / 1e12:5.2f} TB/s, bf16 {valid * D * 2 * blocks / (t[bf16].mean() * 1e-6) / 1e12:5.2f} TB/s")
        if parent:
            line += f" | parent {fmt(t[old])} | bf16 / parent {t[bf16].mean() / t[old].mean():6.3f}, same bytes"
            if not t[bf16].min() <= t[old].max():
                slower.append(" ".join(name.split()))
        say(line)
        del q, cache, deq, idx, outs
        torch.cuda.empty_cache()
    if parent:
        say("# cases where bf16 is slower than parent beyond the spread: " + ("; ".join(slower) if slower else "none"))
    else:
        say("# no --parent-lib: the bf16 kernel was not timed against the parent commit's build")

    s = 65536
    for tokens in (128, 8192):
        kv = torch.randn((tokens, D), device="cuda", generator=gen).to(torch.bfloat16)
        kv_c, k_pe = kv[:, :DV].contiguous(), kv[:, DV:].contiguous()
        slots = torch.randperm(s, device="cuda", generator=gen)[:tokens]
        caches = [torch.zeros((s // PAGE, PAGE, 1, ROW), dtype=torch.uint8, device="cuda") for _ in range(2)]
        flat = caches[1].view(s, ROW)

        def old():
            codes, sf = dga.per_token_cast_to_fp8(kv_c)
            flat[slots, :DV] = codes.view(torch.uint8)
            flat[slots, DV:DV + 16] = sf.view(torch.uint8)
            flat[slots, DV + 16:] = k_pe.view(torch.uint8)

        new = lambda: dga.mla_kv_cast_to_fp8_paged(kv_c, k_pe, caches[0], slots)
        new(); old()
        torch.cuda.synchronize()
        assert torch.equal(caches[0], caches[1]) and int((caches[0] != 0).sum()) > tokens * 500
        t = alternate([new, old], args.windows)
        say(f"writer T={tokens:5d} into S={s} bf16 | new {fmt(t[new])} | old {fmt(t[old])} | old / new {t[old].mean() / t[new].mean():6.2f} | same bytes")
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
