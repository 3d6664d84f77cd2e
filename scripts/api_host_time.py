"""Host time per call of the Python wrappers (deepgemm_ascend_amd/api.py), in the manner of profiles/r03_host_overhead.txt: each row issues
2000 back-to-back calls on the current stream and synchronises once at the end; "host" is the wall time of the issuing loop per call.  A row is
warmed up first (plans, scratch and the allocator's blocks exist) and measured in three such windows: the fastest is the figure, all three
are printed (their spread is this measurement's noise within one process; between two processes, run it twice).  The shapes are short on
purpose -- the device finishes a call before the host has issued the next, so the loop never waits for the queue.
--ext times the pybind extension deep_gemm_cpp (csrc/python_api_amd.cpp) in the same way: the built module in the package, or the one at
PATH (a build of another commit, to compare with; its file may have any name, and it finds libdga_hip.so beside itself).
Usage: python scripts/api_host_time.py [--calls 2000] [--windows 3]        (results: profiles/api_host_time.txt)
       python scripts/api_host_time.py --ext [PATH]                        (results: profiles/ext_host_time.txt)"""
import argparse
import importlib.util
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import deepgemm_ascend_amd as dga  # noqa: E402


def rows():
    """(label, call) for every row; the tensors live in the closures."""
    dev = "cuda"
    bf = lambda *shape: torch.randn(*shape, device=dev).to(torch.bfloat16)
    m, n, k = 64, 32768, 512
    a, b, out = dga.per_token_cast_to_fp8(bf(m, k)), dga.per_block_cast_to_fp8(bf(n, k)), torch.empty(m, n, dtype=torch.bfloat16, device=dev)
    yield f"gemm_fp8_fp8_bf16_nt {m}x{n}x{k}, tiling looked up", lambda: dga.gemm_fp8_fp8_bf16_nt(a, b, out)

    g, mmax, n, k = 4, 64, 512, 512
    qa, sfa = dga.per_token_cast_to_fp8(bf(g * mmax, k))
    qb, sfb = dga.per_block_cast_to_fp8_transposed(bf(g, k, n))   # [G, N, K] codes, [G, N/128, K/128] scales
    lhs, rhs = (qa.view(g, mmax, k), sfa.view(g, mmax, -1)), (qb, sfb)
    outg, masked = torch.empty(g, mmax, n, dtype=torch.bfloat16, device=dev), torch.tensor([64, 1, 33, 0], dtype=torch.int32, device=dev)
    yield (f"m_grouped_gemm_fp8_fp8_bf16_nt_masked G{g} Mmax{mmax} N{n} K{k}",
           lambda: dga.m_grouped_gemm_fp8_fp8_bf16_nt_masked(lhs, rhs, outg, masked, mmax))

    x = bf(64, 2 * 512)
    q_sf = dga.silu_and_mul_per_token_cast_to_fp8(x)
    yield "silu_and_mul_per_token_cast_to_fp8 64x(2x512)", lambda: dga.silu_and_mul_per_token_cast_to_fp8(x)
    yield "silu_and_mul_per_token_cast_to_fp8 64x(2x512), out=", lambda: dga.silu_and_mul_per_token_cast_to_fp8(x, out=q_sf)

    logits = torch.randn(64, 256, device=dev)
    gate = dga.router_topk(logits, 8)
    yield "router_topk T64 E256 k8", lambda: dga.router_topk(logits, 8)
    yield "router_topk T64 E256 k8, out=", lambda: dga.router_topk(logits, 8, out=gate)

    src, weights = bf(64 * 8, 512), gate[1]
    dest = torch.randperm(64 * 8, device=dev).view(64, 8)
    yield "combine_tokens T64 k8 H512", lambda: dga.combine_tokens(src, dest, weights)

    # sparse MLA decode, one token: beside a kernel of some 20 us (profiles/sparse_mla_split_timing.txt) the wrapper's checks count
    hq, topk, s = 16, 64, 64
    q, kv, cache = bf(1, hq, 576), bf(s, 576), torch.zeros(1, 64, 1, 656, dtype=torch.uint8, device=dev)
    idx = torch.randperm(s, device=dev)[:topk].to(torch.int32).view(1, topk)
    o, l = torch.empty(1, hq, 512, dtype=torch.bfloat16, device=dev), torch.empty(1, hq, dtype=torch.float32, device=dev)
    po, pl = dga.sparse_mla_fwd_partial(q, kv, idx, 0.04, 2)
    shape = f"M1 Hq{hq} topk{topk}, out="
    yield f"sparse_mla_fwd {shape}", lambda: dga.sparse_mla_fwd(q, kv, idx, 0.04, out=o, lse=l)
    yield f"sparse_mla_fwd_fp8 {shape}", lambda: dga.sparse_mla_fwd_fp8(q, cache, idx, 0.04, out=o, lse=l)
    yield f"sparse_mla_fwd_split(num_splits=None) {shape}", lambda: dga.sparse_mla_fwd_split(q, kv, idx, 0.04, out=o, lse=l)
    yield f"sparse_mla_fwd_split(num_splits=2) {shape}", lambda: dga.sparse_mla_fwd_split(q, kv, idx, 0.04, num_splits=2, out=o, lse=l)
    yield f"sparse_mla_fwd_fp8_split(num_splits=2) {shape}", lambda: dga.sparse_mla_fwd_fp8_split(q, cache, idx, 0.04, num_splits=2, out=o, lse=l)
    yield f"sparse_mla_merge P2 M1 Hq{hq}, out=", lambda: dga.sparse_mla_merge(po, pl, out=o, lse=l)


def load_ext(path):
    if not path:
        from deepgemm_ascend_amd import deep_gemm_cpp
        return deep_gemm_cpp
    spec = importlib.util.spec_from_file_location("deep_gemm_cpp", path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def ext_rows(d):
    """The same, through the bindings of the extension module d: positional tensors, outputs allocated by the caller of the GEMMs."""
    dev = "cuda"
    bf = lambda *shape: torch.randn(*shape, device=dev).to(torch.bfloat16)
    m, n, k = 64, 32768, 512
    (a, sfa), (b, sfb), out = d.per_token_cast_to_fp8(bf(m, k)), d.per_block_cast_to_fp8(bf(n, k)), torch.empty(m, n, dtype=torch.bfloat16, device=dev)
    yield f"gemm_fp8_fp8_bf16_nt {m}x{n}x{k}", lambda: d.gemm_fp8_fp8_bf16_nt(a, sfa, b, sfb, out)

    g, mmax, n, k = 4, 64, 512, 512
    qa, sa = d.per_token_cast_to_fp8(bf(g * mmax, k))
    qb, sb = d.per_block_cast_to_fp8_transposed(bf(g, k, n))
    qa, sa = qa.view(g, mmax, k), sa.view(g, mmax, -1)
    outg, masked = torch.empty(g, mmax, n, dtype=torch.bfloat16, device=dev), torch.tensor([64, 1, 33, 0], dtype=torch.int32, device=dev)
    yield (f"m_grouped_gemm_fp8_fp8_bf16_nt_masked G{g} Mmax{mmax} N{n} K{k}",
           lambda: d.m_grouped_gemm_fp8_fp8_bf16_nt_masked(qa, sa, qb, sb, outg, masked, mmax))

    m, n, k = 64, 512, 512
    (a2, sfa2), (b2, sfb2), acc = d.per_token_cast_to_fp8(bf(m, k)), d.per_block_cast_to_fp8(bf(n, k)), torch.zeros(m, n, device=dev)
    yield f"gemm_fp8_fp8_fp32_nt {m}x{n}x{k}, c=out", lambda: d.gemm_fp8_fp8_fp32_nt(a2, sfa2, b2, sfb2, acc, acc)

    x = bf(64, 2 * 512)
    yield "silu_and_mul_per_token_cast_to_fp8 64x(2x512)", lambda: d.silu_and_mul_per_token_cast_to_fp8(x)
    xt = bf(64, 512)
    yield "per_token_cast_to_fp8_transposed 64x512", lambda: d.per_token_cast_to_fp8_transposed(xt)

    src, weights = bf(64 * 8, 512), torch.rand(64, 8, device=dev)
    dest = torch.randperm(64 * 8, device=dev).view(64, 8)
    yield "combine_tokens T64 k8 H512", lambda: d.combine_tokens(src, dest, weights)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--ext", nargs="?", const="", default=None, metavar="PATH")
    args = ap.parse_args()
    torch.manual_seed(0)
    for label, call in rows() if args.ext is None else ext_rows(load_ext(args.ext)):
        for _ in range(200):
            call()
        torch.cuda.synchronize()
        us = []
        for _ in range(args.windows):
            t0 = time.perf_counter()
            for _ in range(args.calls):
                call()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            us.append((t1 - t0) / args.calls * 1e6)
        print(f"{label:<64}: host {min(us):6.2f} us/call issued   (windows: {' '.join(f'{u:.2f}' for u in us)})", flush=True)


if __name__ == "__main__":
    main()
