#!/usr/bin/env python3
"""bench.py -- the judged benchmark entry (contract in the task statement, section 4).

Default workload = BASELINE.json configs[1]: 4096 x 4096 x 4096 fp8 block-scaled NT GEMM, bf16 out,
per-1x128 A scales / per-128x128 B scales, 1 x MI355X.  One "step" = one pass of the hot path over one
batch = one operator call through the C ABI (tiling lookup included, as the reference's op consults its cache on
every call, select_kernel.cpp:371-378) with inputs already resident in HBM.

  python bench.py --gpus N --steps K --warmup W
      N > 1 without WORLD_SIZE in the environment: this process starts N ranks (one per GPU, torch.distributed.run on
      127.0.0.1) BEFORE it touches a GPU and exits with their status -- the reference's multi-card model is likewise N
      processes, one per device (benchmark_msprof/main.cpp:24-26, framework/benchmark/benchmark.py:249-253).
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...     (what the driver runs)
  python bench.py ... --dump-outputs DIR
      also writes what the last timed step returned (DIR/out.npy, float32) so that two builds can be compared output for output.

N > 1: the dense GEMM does not shard ("replicas only"): every rank runs the same
problem, `value` = N x per-replica work / max-over-ranks time (weak scaling).  The path that does shard --
the grouped masked-M GEMM with experts partitioned over ranks and an RCCL all-to-all each way -- is reported
in the extra "grouped" object of the same JSON line (tok/s with and without the exchange).

Extra objects: "roofline" (dominant kernel vs the dense fp8 MFMA peak, with the clock measured inside the kernel's
main loop, and vs `ceiling_tflops` = what this box's matrix pipe sustains on the kernel's inner step with the operands
already in registers), "parity" (every output of the timed kernel against the strict kernel, which tests pin bit for bit
to the CPU oracle), "policies" (the three arithmetic policies side by side -- fast / bf16_exact / strict: value, roofline
and parity of each; the headline `value` is the "fast" column), "shape_list" (the reference's 18 sweep shapes,
framework/benchmark/benchmark.py:24-44: time, rate, bound and parity gate of each), "reference_benchmark_fp16" (the same list through
the call the reference's own benchmark makes: run_mmad_bench, fp16 in, f32 out), "dsv3_prefill" (BASELINE configs[2], own roofline), "cpu_baseline" (the CPU oracle and the reference's
numpy formula timed on this box's host cores on a bounded row sample; rank 0, N = 1 only).
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))

PEAK_FP8_TFLOPS = 5000.0   # MI355X dense fp8 MFMA peak (/opt/skills/guides/MI355X_MICROARCH.md, chip table)
PEAK_BF16_TFLOPS = 2500.0  # dense bf16 MFMA peak: the instruction the bf16-exact policy computes on
PEAK_FP32_MATRIX_TFLOPS = 157.3   # fp32-input MFMA peak: the instruction the strict policy computes on
# the parity bar of each arithmetic policy: |d| <= 2 ulp_bf16 + eps * S on every element (README.md, Numerics)
POLICY_EPS = {"fast": 2.0 ** -15, "bf16_exact": 2.0 ** -22, "strict": 0.0}
PEAK_HBM_GBPS = 8000.0
FP8_FLOP_PER_CLK_PER_CU = 8192.0   # peak_fp8 = CUs x clk x 8192

WORKLOADS = {
    # name: (m, n, k)
    "dense_4096": (4096, 4096, 4096),         # BASELINE.json configs[1]
    "dsv3_prefill": (4096, 2048, 7168),       # configs[2]  (M=4096, K=7168, N=2048)
}


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--workload", default="dense_4096", choices=sorted(WORKLOADS))
    ap.add_argument("--policy", default="bf16_exact", choices=["bf16_exact", "fast"],
                    help="arithmetic policy of the timed steps = of `value`.  bf16_exact (default, also the operator's default): the "
                         "fastest policy inside north_star's tolerance (<= 1e-5 of the outputs beyond 2 bf16 ULP of the fp32-accumulate "
                         "result).  fast: the fp8 matrix instruction (6.7e-4 beyond 2 ULP) -- reported in the `fast` object either way")
    ap.add_argument("--detail-out", default=None,
                    help="file for the full record (every leg, every column); default gpurun_out/bench_detail.json, /tmp if that "
                         "is not writable.  stdout carries ONE compact line (< 4 KB) -- the record the driver parses")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-grouped", action="store_true")
    ap.add_argument("--no-parity", action="store_true")
    ap.add_argument("--no-prefill", action="store_true")
    ap.add_argument("--no-shape-list", action="store_true", help="skip the reference's 18-shape sweep list leg")
    ap.add_argument("--no-policies", action="store_true",
                    help="skip the side-by-side legs of the bf16-exact and strict arithmetic policies")
    ap.add_argument("--no-live-traffic", action="store_true",
                    help="roofline.traffic from the committed PMC passes instead of two rocprofv3 child runs of this invocation")
    ap.add_argument("--widen", action="store_true",
                    help="also time the rows either side of the hot path (contiguous-grouped layout, quantiser); off by "
                         "default so that the default command's kernel statistics hold the headline kernels only")
    ap.add_argument("--groups", type=int, default=256)
    ap.add_argument("--grouped-mask", default="full", choices=["full", "random"])
    ap.add_argument("--capacity-factor", type=float, default=1.25,
                    help="sharded grouped path: rows reserved per (chunk, peer) = this x the even share (parallel.py)")
    ap.add_argument("--sharded-indexed", action="store_true",
                    help="world > 1: let the grouped GEMM read the receive buffer in place (opt-in until it has run under "
                         "RCCL; the packed path is the default, parallel.py)")
    ap.add_argument("--cpu-budget", type=float, default=15.0)
    ap.add_argument("--prewarm-ms", type=float, default=300.0,
                    help="untimed clock pre-warm in front of the W warmup steps: after idle the GPU needs a few hundred "
                         "steps to reach its sustained clocks (20 warmup steps alone leave the first 200 timed steps 14 %% "
                         "slow, scripts/warm_effect.py)")
    ap.add_argument("--rehearse-shared-gpu", action="store_true",
                    help="N > 1 ranks that all use cuda:0, gloo with collectives staged through the host: runs every N > 1 "
                         "branch of this file and of parallel.py on a one-GPU box.  A rehearsal of the control flow -- the line "
                         "says so and its numbers mean nothing (the ranks time-slice one GPU)")
    ap.add_argument("--stub", action="store_true",
                    help="no GPU: gloo backend, CPU tensors and a numpy stand-in for the step -- exercises the launcher, the "
                         "rendezvous, the barrier / max-over-ranks timing and the JSON contract (tests/test_bench_launcher.py)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned to its caller as DIR/<name>.npy "
                         "(float32; rank 0): out.npy = the bf16 output matrix, whole when it fits in 32 MiB as float32, else a "
                         "fixed seeded sample of its rows in ascending order.  The inputs are seeded, so two builds run with the "
                         "same arguments can be compared output for output")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    return args


DUMP_BYTES = 32 << 20   # --dump-outputs: float32 bytes per output; a larger output is dumped as a seeded row sample


def dump_rows(out):
    """`out` (2-D torch tensor or numpy array) as the float32 array --dump-outputs writes: every row when they fit DUMP_BYTES,
    else a fixed seeded sample of rows in ascending order -- the same rows in every run of the same shape."""
    import numpy as np
    m, n = out.shape
    keep = max(1, DUMP_BYTES // (4 * n))
    if m > keep:
        idx = np.sort(np.random.default_rng(0).choice(m, keep, replace=False))
        if isinstance(out, np.ndarray):
            out = out[idx]
        else:
            import torch
            out = out.index_select(0, torch.from_numpy(idx).to(out.device))
    if not isinstance(out, np.ndarray):
        out = out.float().cpu().numpy()
    return np.ascontiguousarray(out, dtype=np.float32)


def dump_outputs(dirpath, arrays: dict) -> dict:
    """Write each array as DIR/<name>.npy; returns {name: shape} for the record."""
    import numpy as np
    d = Path(dirpath)
    d.mkdir(parents=True, exist_ok=True)
    for name, arr in arrays.items():
        np.save(d / f"{name}.npy", arr)
    return {name: list(arr.shape) for name, arr in arrays.items()}


def launch_ranks(args) -> int:
    """--gpus N outside a torchrun environment: start the N ranks as children.  Nothing in this process has touched a
    GPU (torch is not even imported yet), so no GPU-initialised process is ever re-executed."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), str(Path(__file__).resolve())] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


# --------------------------------------------------------------------------------------------------- inputs

def _rand_fp8(shape, gen):
    import torch
    x = torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=gen)
    return torch.where((x & 0x7F) == 0x7F, x & 0x80, x)  # no NaN encodings


def make_dense_inputs(m, n, k, seed, ue8m0=False):
    """Synthetic data of the SURVEY.md 8(d) shape: fp32 ~ N(0,1), amax-scaled per 1x128 / 128x128, cast to
    e4m3fn.  Generated on the device (torch casts saturate identically to the oracle for |x| <= 448).
    ue8m0: the scales rounded UP to powers of two (2^ceil(log2(amax / 448)): upstream DeepGEMM's use_ue8m0 quantisation)."""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    xa = torch.randn((m, k), device="cuda", generator=g)
    xb = torch.randn((n, k), device="cuda", generator=g)
    kb = k // 128
    pow2 = (lambda s: torch.exp2(torch.ceil(torch.log2(s)))) if ue8m0 else (lambda s: s)
    sa = pow2(xa.view(m, kb, 128).abs().amax(dim=2).clamp_min(1e-30) / 448.0)
    qa = (xa.view(m, kb, 128) / sa[..., None]).reshape(m, k).to(torch.float8_e4m3fn).view(torch.uint8)
    nb = n // 128
    sb = pow2(xb.view(nb, 128, kb, 128).abs().amax(dim=(1, 3)).clamp_min(1e-30) / 448.0)
    qb = (xb.view(nb, 128, kb, 128) / sb[:, None, :, None]).reshape(n, k).to(torch.float8_e4m3fn).view(torch.uint8)
    return qa.contiguous(), sa.contiguous().float(), qb.contiguous(), sb.contiguous().float()


TRAFFIC_FILES = ("r06_traffic.json", "r05_traffic.json", "r04_traffic.json", "r03_traffic.json", "r02_traffic.json", "r01_traffic.json")   # newest first


def pmc_traffic_source():
    for name in TRAFFIC_FILES:
        if (ROOT / "profiles" / name).exists():
            return f"profiles/{name}: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of the same kernel (a committed measurement, not this run)"
    return None


def pmc_traffic(workload: str):
    """HBM-side bytes per launch from the committed rocprofv3 PMC passes (profiles/r0N_traffic.json: FETCH_SIZE and
    WRITE_SIZE collected in separate passes and corrected as MI355X_MICROARCH.md prescribes).  PMC counters cannot be
    read from inside this process, so this is the figure of the profiled run of the same kernel, not of this run."""
    for name in TRAFFIC_FILES:
        try:
            d = json.loads((ROOT / "profiles" / name).read_text())
            return int(d[workload]["traffic_bytes"])
        except Exception:
            continue
    return None


def live_pmc_traffic(m, n, k, launches=260, skip=200, timeout_s=90, policy="bf16_exact"):
    """HBM-side bytes per launch of the dense tile kernel measured BY THIS RUN: two child processes (scripts/prof_dense.py, the
    same kernel on the same recipe) under `rocprofv3 --kernel-trace --pmc FETCH_SIZE` and `... WRITE_SIZE` -- separate passes,
    the counters' units and the gfx950 correction as MI355X_MICROARCH.md prescribes (FETCH_SIZE counts 64 B per 128-B request of
    wide coalesced reads: x 2; KB: x 1024), mean over the launches after the first `skip` (sustained clocks).  The children are
    started, not exec'ed (this process has initialised the GPU), with rocprofv3's program directly behind `--`.
    Returns (bytes or None, how / why not)."""
    import csv as _csv
    import shutil
    import tempfile
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None, "rocprofv3 not found"
    if "rocprof" in os.environ.get("LD_PRELOAD", "").lower() or any(k.startswith(("ROCPROF", "ROCP_TOOL")) for k in os.environ):
        return None, "this process runs under a profiler already: no nested rocprofv3 passes"
    mean = {}
    for counter in ("FETCH_SIZE", "WRITE_SIZE"):
        d = tempfile.mkdtemp(prefix="dga_pmc_", dir="/tmp")
        try:
            cmd = [exe, "--kernel-trace", "--pmc", counter, "--output-format", "csv", "-d", d, "-o", "p", "--", sys.executable,
                   str(ROOT / "scripts" / "prof_dense.py"), str(m), str(n), str(k), str(launches), "--policy", policy]
            # its own session: on a timeout the whole group goes (rocprofv3 AND the python child it started -- killing the
            # wrapper alone would leave 260 launches of the kernel running beside the legs timed next)
            proc = subprocess.Popen(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                    text=True, start_new_session=True)
            try:
                so, se = proc.communicate(timeout=timeout_s)
            except subprocess.TimeoutExpired:
                import signal
                try:
                    os.killpg(proc.pid, signal.SIGKILL)
                except ProcessLookupError:
                    pass
                proc.communicate()
                return None, f"rocprofv3 --pmc {counter}: timed out after {timeout_s} s (process group killed)"
            r = subprocess.CompletedProcess(cmd, proc.returncode, so, se)
            files = sorted(Path(d).rglob("*_counter_collection.csv"))
            if r.returncode != 0 or not files:
                return None, f"rocprofv3 --pmc {counter}: rc {r.returncode}, {(r.stderr or '')[-200:]!r}"
            per = {}
            with open(files[0]) as f:
                for row in _csv.DictReader(f):
                    if "gemm_fp8" in row["Kernel_Name"] and row["Counter_Name"] == counter:
                        per[int(row["Dispatch_Id"])] = per.get(int(row["Dispatch_Id"]), 0.0) + float(row["Counter_Value"])
            vals = [v for _, v in sorted(per.items())][skip:]
            if not vals:
                return None, f"no launches of the tile kernel in the {counter} pass"
            mean[counter] = sum(vals) / len(vals)
        except Exception as e:
            return None, f"{counter} pass: {e!r}"
        finally:
            shutil.rmtree(d, ignore_errors=True)
    byt = int(mean["FETCH_SIZE"] * 2 * 1024 + mean["WRITE_SIZE"] * 1024)
    return byt, (f"this run: rocprofv3 --kernel-trace --pmc FETCH_SIZE / WRITE_SIZE (separate child processes of bench.py, scripts/prof_dense.py, "
                 f"mean of launches {skip + 1}..{launches}; FETCH_SIZE {mean['FETCH_SIZE']:.0f} KB x 2 (gfx950), WRITE_SIZE {mean['WRITE_SIZE']:.0f} KB)")


# --------------------------------------------------------------------------------------------------- legs

def parity_vs_strict(dga, a, sfa, b, sfb, fast_out, policy="fast"):
    """Every output of a timed kernel (`policy` names which: its bar is reported beside the figures) against the strict kernel on the same inputs.  The strict
    kernel is the product's exact-arithmetic policy; tests/test_strict_gpu.py pins it bit for bit to the CPU oracle, so
    these figures are the fast path's distance from the oracle over ALL elements.  S = sum |scaled products| comes from
    the strict kernel run on |a|, |b|, |scales| (bf16-rounded, 2^-9 relative)."""
    import torch
    m, n = fast_out.shape
    exact = torch.empty_like(fast_out)
    s_abs = torch.empty_like(fast_out)
    dga.gemm_fp8_fp8_bf16_nt((a, sfa), (b, sfb), exact, strict=True)
    dga.gemm_fp8_fp8_bf16_nt((a & 0x7F, sfa.abs()), (b & 0x7F, sfb.abs()), s_abs, strict=True, sync=True)

    def key(t):   # monotone integer map of bf16 bit patterns (+0 / -0 coincide)
        v = t.view(torch.int16).to(torch.int32)
        mag = v & 0x7FFF
        return torch.where(v < 0, -mag, mag)
    ulps = (key(fast_out) - key(exact)).abs()
    f, e, s = fast_out.double(), exact.double(), s_abs.double()
    ulp = torch.exp2(torch.floor(torch.log2(e.abs().clamp_min(2.0 ** -126))) - 7)
    excess = ((f - e).abs() - 2 * ulp).clamp_min(0) / s.clamp_min(1e-300)
    return {
        "against": "strict policy (fp32-MFMA chain in the oracle's order; bit-identical to the CPU oracle in tests/test_strict_gpu.py)",
        "elements": int(m * n), "max_ulp": int(ulps.max()), "frac_gt_2ulp": float((ulps > 2).double().mean()),
        "elements_gt_2ulp": int((ulps > 2).sum()),
        "worst_excess_over_S": float(excess.max()),
        "bar": f"|d| <= 2 ulp_bf16 + 2^{int(__import__('math').log2(POLICY_EPS[policy])) if POLICY_EPS[policy] else '-inf'} * S (README.md, Numerics)",
        "within_bar": bool(float(excess.max()) <= POLICY_EPS[policy] * 1.01),
    }


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def cpu_baseline(m, n, k, a, sfa, b, sfb, gpu_out=None, budget_s=15.0, strict_out=None):
    """The CPU oracle (oracle/dga_oracle.c, kind "port") on a bounded row sample of the same workload: one warm-up,
    median of >= 3 passes.  Beside it the reference's own CPU path restated -- np.matmul(f32, f32) on the dequantised
    operands (/root/reference/deep_gemm_ascend/framework/benchmark/benchmark.py:362) -- as the BLAS-quality bound:
    operands dequantised once outside the timed region, one sgemm over the full K, same protocol.  The oracle rows
    computed here also check the timed GPU output (the oracle as checker)."""
    import numpy as np
    from oracle import oracle as O
    O.build()
    cores = max(1, min(os.cpu_count() or 1, 64))
    an = a.cpu().numpy(); bn = b.cpu().numpy(); san = sfa.cpu().numpy(); sbn = sfb.cpu().numpy()
    probe = min(m, cores)
    O.gemm_fp8_fp8_bf16_nt(an[:probe], san[:probe], bn, sbn, threads=cores)          # warm-up (page-in, thread start)
    t0 = time.perf_counter()
    O.gemm_fp8_fp8_bf16_nt(an[:probe], san[:probe], bn, sbn, threads=cores)
    dt = max(time.perf_counter() - t0, 1e-4)
    reps = 3
    rows = int(min(m, max(cores, probe * (0.6 * budget_s / reps) / dt)))
    rows = max(cores, rows - rows % cores)
    times, want = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        want = O.gemm_fp8_fp8_bf16_nt(an[:rows], san[:rows], bn, sbn, threads=cores)
        times.append(time.perf_counter() - t0)
    med = _median(times)
    res = {
        "value": round(2.0 * rows * n * k / med / 1e12, 6), "unit": "TFLOP/s", "cores": cores, "kind": "port",
        "reps": reps, "median_s": round(med, 4),
        "sample": f"first {rows} of {m} rows of A against all of B; 1 warm-up + {reps} passes, median {med:.2f} s (scalar "
                  f"fp32-accumulate C oracle, one thread per core)",
    }
    # the reference's golden formula on the dequantised operands, BLAS sgemm over the full K
    tab = O.e4m3fn_table()
    rb = min(m, 1024)
    kb = k // 128
    a_deq = (tab[an[:rb]].reshape(rb, kb, 128) * san[:rb, :, None]).reshape(rb, k).astype(np.float32)
    b_deq = (tab[bn].reshape(n // 128, 128, kb, 128) * sbn[:, None, :, None]).reshape(n, k).astype(np.float32)
    b_t = np.ascontiguousarray(b_deq.T)
    np.matmul(a_deq, b_t)                                                            # warm-up
    bt = []
    for _ in range(3):
        t0 = time.perf_counter()
        np.matmul(a_deq, b_t)
        bt.append(time.perf_counter() - t0)
    bmed = _median(bt)
    res.update({"blas_value": round(2.0 * rb * n * k / bmed / 1e12, 6), "blas_reps": 3, "blas_median_s": round(bmed, 4),
                "blas_note": f"reference golden formula np.matmul(f32, f32) on operands dequantised once outside the timed "
                             f"region, first {rb} rows, numpy BLAS threads"})
    if gpu_out is not None:
        got = gpu_out[:rows].view(__import__("torch").int16).cpu().numpy().view(np.uint16)
        rep = O.parity_report(got, want, an[:rows], san[:rows], bn, sbn)
        res["gpu_rows_vs_oracle"] = {"rows": rows, "max_ulp": rep["max_ulp"], "frac_gt_2ulp": rep["frac_gt_max_ulp"],
                                     "worst_excess_over_S": rep["worst_excess_over_S"]}
    if strict_out is not None:   # policy_legs leaves the strict policy's output in this buffer (it runs last)
        got = strict_out[:rows].view(__import__("torch").int16).cpu().numpy().view(np.uint16)
        res["strict_rows_vs_oracle"] = {"rows": rows, "max_ulp": int(O.bf16_ulp_diff(got, want).max(initial=0)),
                                        "bit_identical": bool(np.array_equal(got, want))}
    return res


def grouped_leg(args, rank, world, dist):
    """Grouped masked-M GEMM, experts sharded over ranks (BASELINE.json configs[3]/[4])."""
    from deepgemm_ascend_amd import parallel
    return parallel.bench_grouped(rank, world, dist, steps=max(3, min(args.steps, 20)), warmup=3,
                                  groups_total=args.groups, m_max=128, n=2048, k=7168,
                                  mask=args.grouped_mask, capacity_factor=args.capacity_factor,
                                  indexed=True if args.sharded_indexed else None, parity=not args.no_parity, policy=args.policy)


def _time_us(fn, iters, warm):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def kernel_name(t, policy):
    """Name under which the rocprofv3 kernel trace lists the launch a tiling resolves to (csrc/dga_launch.hip)."""
    if policy == "bf16_exact":
        if int(t.kernelSerial) == 6 and int(t.build) == 10:
            return "gemm_fp8_bf16x_dsk_kernel"
        if int(t.kernelSerial) == 6:
            return "gemm_fp8_wsk_dma_kernel (MATH = 1)"
        if int(t.kernelSerial) == 7:
            return "gemm_fp8_bf16x_streamk_kernel"
        if int(t.build) == 9:
            return "gemm_fp8_bf16x_grouped_kernel"
        if int(t.m1) == 128 and int(t.n1) == 256:
            return "gemm_fp8_bf16x_persistent_kernel (rasters of more than one round; gemm_fp8_blockscaled_nt_kernel<..., MATH = 1> otherwise)"
        return "gemm_fp8_blockscaled_nt_kernel<..., MATH = 1> (bf16-exact build)"
    if policy == "strict":
        return "gemm_fp8_strict_nt_kernel"
    tag = int(t.dispatchPolicyTag)
    return {5: "gemm_fp8_blockscaled_nt_persistent_kernel", 6: "gemm_fp8_cont_persistent_kernel"}.get(tag, "gemm_fp8_blockscaled_nt_kernel")


def roofline_mfma(dga, a, sfa, b, sfb, out, t, m, n, k, kernel_us, cus, policy="fast"):
    """`roofline` object of a dense launch: achieved = 2MNK / average launch time; peak = the vendor dense fp8 figure (the
    metric's own denominator, whatever instruction the policy computes on; `instruction_peak` prices it against that one);
    clock_mhz = the shader clock measured inside the kernel's main loop right after the timed region (loop-clock build of the
    same kernel, fast policy only); frac_at_measured_clock prices the same launch against CUs x clk x 8192."""
    flops = 2.0 * m * n * k
    achieved = flops / (kernel_us * 1e-6) / 1e12
    ipeak, instr, _ = POLICY_SPEC[policy]
    r = {"bound": "mfma", "achieved": round(achieved, 2), "peak": PEAK_FP8_TFLOPS, "unit": "TFLOP/s",
         "frac": round(achieved / PEAK_FP8_TFLOPS, 4), "traffic": None, "kernel_us": round(kernel_us, 3),
         "algorithmic_bytes": m * k + n * k + 2 * m * n + 4 * (sfa.numel() + sfb.numel()),
         "kernel": kernel_name(t, policy), "tile": f"{t.m1}x{t.n1}x{t.k1}", "policy": policy, "instruction": instr,
         "instruction_peak": ipeak, "frac_of_instruction_peak": round(achieved / ipeak, 4),
         "clock_mhz": None, "frac_at_measured_clock": None}
    if policy != "fast":
        return r
    try:
        # 1000 launches: the stamps of the last one are read, and after the gap behind the timed region the chip needs a few
        # hundred launches to be back at the clocks of a busy stream (with 100 the probe read 1.42 GHz where the stream
        # holds 1.67; scripts/clock_probe_check.py shows the probe's launch interval equal to the product kernel's)
        mhz, loop_us = dga.gemm_fp8_loop_clock((a, sfa), (b, sfb), out, tiling_=t, launches=1000)
        peak_clk = cus * mhz * 1e6 * FP8_FLOP_PER_CLK_PER_CU / 1e12
        r.update({"clock_mhz": round(mhz, 1), "main_loop_us": round(loop_us, 2),
                  "peak_at_measured_clock": round(peak_clk, 1), "frac_at_measured_clock": round(achieved / peak_clk, 4)})
    except Exception as e:   # a tiling without a loop-clock build: the vendor-peak fraction stands alone
        r["clock_note"] = repr(e)
    return r


def _prewarmed_us(fn, iters, prewarm_ms):
    """Average launch interval of `iters` back-to-back calls behind an untimed clock pre-warm (HIP events on the current stream)."""
    import torch
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < prewarm_ms:
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
    return _time_us(fn, iters, 0)


def _graph_us(fn, iters, replays=5, prewarm_ms=30.0):
    """Device time per call: `iters` calls captured into one HIP graph on a side stream, the graph replayed `replays` times
    between two events, behind a clock pre-warm (harness/sweep.py graph_us).  The host issues one graph launch per `iters` calls,
    so a call whose kernel is shorter than the host time of issuing it (5-8 us through Python) is timed by what the device
    spends on it."""
    from deepgemm_ascend_amd.harness import sweep
    us = sweep.graph_us(fn, iters, replays, prewarm_ms)
    if us is None:
        raise RuntimeError("graph capture failed")
    return us


POLICY_SPEC = {
    # policy: (peak of the instruction it computes on, instruction, dispatchPolicyTag)
    "fast": (PEAK_FP8_TFLOPS, "v_mfma_f32_16x16x128_f8f6f4 per scale block + fp32 promotion", "0-2, 4-6 (the tiling's schedule)"),
    "bf16_exact": (PEAK_BF16_TFLOPS, "v_mfma_f32_16x16x32_bf16 x4 per scale block on e4m3 bytes up-converted in registers", 7),
    "strict": (PEAK_FP32_MATRIX_TFLOPS, "v_mfma_f32_16x16x4_f32 x32 per scale block, the oracle's own order", 3),
}


def policy_legs(dga, a, sfa, b, sfb, m, n, k, args, headline_policy, headline, ceilings):
    """The three arithmetic policies side by side on one workload: value, roofline and parity of each.
      fast        the fp8 matrix instruction (whatever schedule the tiling names)
      bf16_exact  e4m3 -> bf16 in registers, bf16 matrix instruction (dispatchPolicyTag 7) -- the operator's default
      strict      fp32-input matrix instruction in the oracle's order (dispatchPolicyTag 3)
    `headline` = the already measured {"kernel_us", "roofline", "parity"} of `headline_policy` (the timed steps); the other two
    are timed here.  Every roofline prices the launch against the fp8 peak (the metric's denominator) AND against the peak of
    the instruction the policy computes on (`instruction_peak`), and carries `ceiling_tflops`: what this box's matrix pipe
    sustains on the policy's inner step with the operands already in registers (dga_mfma_ceiling)."""
    import torch
    flops = 2.0 * m * n * k
    out = torch.empty((m, n), dtype=torch.bfloat16, device="cuda")
    legs = {}

    def with_ceiling(roof, pol):
        if ceilings.get(pol):
            roof["ceiling_tflops"] = round(ceilings[pol], 1)
            roof["frac_of_ceiling"] = round(roof["achieved"] / ceilings[pol], 4)
        return roof
    peak, instr, tag = POLICY_SPEC[headline_policy]
    legs[headline_policy] = {"dispatchPolicyTag": tag, "value": headline["roofline"]["achieved"], "unit": "TFLOP/s",
                             "kernel_us": headline["kernel_us"], "roofline": with_ceiling(dict(headline["roofline"]), headline_policy),
                             "parity": headline.get("parity"), "timed_as": "the headline steps"}
    iters = {"fast": (max(20, min(args.steps, 200)), args.prewarm_ms), "bf16_exact": (max(20, min(args.steps, 200)), args.prewarm_ms),
             "strict": (max(5, min(args.steps, 20)), min(args.prewarm_ms, 50.0))}
    for pol in ("fast", "bf16_exact", "strict"):   # strict last: its output stays in `out` for the CPU oracle's rows
        if pol == headline_policy:
            continue
        peak, instr, tag = POLICY_SPEC[pol]
        try:
            fn = lambda: dga.gemm_fp8_fp8_bf16_nt((a, sfa), (b, sfb), out, policy=pol)
            us = _prewarmed_us(fn, *iters[pol])
            tf = flops / us / 1e6
            roof = with_ceiling({"bound": "mfma", "achieved": round(tf, 2), "peak": PEAK_FP8_TFLOPS, "unit": "TFLOP/s",
                                 "frac": round(tf / PEAK_FP8_TFLOPS, 4), "instruction_peak": peak,
                                 "frac_of_instruction_peak": round(tf / peak, 4), "kernel_us": round(us, 3), "instruction": instr}, pol)
            leg = {"dispatchPolicyTag": tag, "value": round(tf, 2), "unit": "TFLOP/s", "kernel_us": round(us, 3), "roofline": roof}
            if not args.no_parity:
                fn(); torch.cuda.synchronize()
                leg["parity"] = parity_vs_strict(dga, a, sfa, b, sfb, out, policy=pol)
                if pol == "strict":
                    leg["parity"]["against"] = "itself (a second run: determinism); the CPU oracle rows are in cpu_baseline.gpu_rows_vs_oracle"
            legs[pol] = leg
        except Exception as e:
            legs[pol] = {"error": repr(e)}
    return legs, out


def ue8m0_leg(dga, m, n, k, args):
    """configs[1] with the block scales rounded up to powers of two (2^ceil(log2(amax / 448))): policy "fast_ue8m0" (fp8 MFMA with
    the scales in its E8M0 operands, accumulate in place) and "bf16_exact_ue8m0" (in contract: scales folded into the exact
    conversions, bf16 MFMA accumulates in place), each with its parity against the strict kernel on the same inputs."""
    import torch
    a, sfa, b, sfb = make_dense_inputs(m, n, k, seed=7, ue8m0=True)
    out = torch.empty((m, n), dtype=torch.bfloat16, device="cuda")
    flops = 2.0 * m * n * k
    leg = {"recipe": "SURVEY.md 8(d) with scale = 2^ceil(log2(amax / 448)) (per_token_cast_to_fp8(..., use_ue8m0=True))"}
    for pol in ("fast_ue8m0", "bf16_exact_ue8m0"):
        fn = lambda: dga.gemm_fp8_fp8_bf16_nt((a, sfa), (b, sfb), out, policy=pol)
        us = _prewarmed_us(fn, max(20, min(args.steps, 200)), args.prewarm_ms)
        o = {"value": round(flops / us / 1e6, 2), "unit": "TFLOP/s", "kernel_us": round(us, 3), "frac_of_fp8_peak": round(flops / us / 1e6 / PEAK_FP8_TFLOPS, 4)}
        if not args.no_parity:
            fn(); torch.cuda.synchronize()
            par = parity_vs_strict(dga, a, sfa, b, sfb, out, policy="fast" if pol == "fast_ue8m0" else "bf16_exact")
            o.update({"max_ulp": par["max_ulp"], "frac_gt_2ulp": par["frac_gt_2ulp"], "within_bar": par["within_bar"]})
        leg[pol] = o
    return leg


IN_CONTRACT_FRAC = 1e-5   # at most this fraction of the outputs beyond 2 bf16 ULP of the fp32-accumulate result


def in_contract(policies):
    """The fastest arithmetic policy whose outputs stay inside north_star's tolerance -- within 2 ULP bf16 of the
    fp32-accumulate CPU path (/root/reference/deep_gemm_ascend/framework/tests/test.py:19-64) -- on all but IN_CONTRACT_FRAC of
    the elements (every output compared with the strict kernel, which tests/test_strict_gpu.py pins bit for bit to the CPU
    oracle).  The headline `value` is the fast policy's; this object says which number a caller who needs the contract gets."""
    best = None
    for pol in ("fast", "bf16_exact", "strict"):
        leg = policies.get(pol) or {}
        par = leg.get("parity") or {}
        if "value" not in leg or "frac_gt_2ulp" not in par:
            continue
        if par["frac_gt_2ulp"] <= IN_CONTRACT_FRAC and (best is None or leg["value"] > best["value"]):
            best = {"policy": pol, "value": leg["value"], "unit": "TFLOP/s", "kernel_us": leg.get("kernel_us"),
                    "frac_of_fp8_peak": round(leg["value"] / PEAK_FP8_TFLOPS, 4),
                    "frac_of_own_peak": (leg.get("roofline") or {}).get("frac"),
                    "frac_gt_2ulp": par["frac_gt_2ulp"], "max_ulp": par.get("max_ulp"),
                    "bar": f"frac_gt_2ulp <= {IN_CONTRACT_FRAC:g} over all outputs against the strict kernel"}
    return best or {"policy": None, "note": "no policy leg with a parity report (run without --no-parity / --no-policies)"}


def shape_list_leg(dga, iters=20):
    """The reference's own sweep shape list (framework/benchmark/benchmark.py:24-44: 18 shapes) through the operator as a
    caller makes it -- tiling from the cache / tuned table / predictor, fast policy -- each gated by the product's parity bar
    (harness/tolerance.py) against the fp32 matmul of the dequantised operands, then timed warm (one operand set re-launched;
    the cold-cache figures of the short-M shapes are in profiles/r03_decode_cold.txt).  Per shape: the bound that applies
    (min of the MFMA and the HBM floor), and the fraction of it reached."""
    import torch
    from deepgemm_ascend_amd.harness import sweep
    rows = []
    for (m, n, k) in sweep.SHAPE_GROUP:
        try:
            a, sfa, b, sfb, golden, s_abs = sweep.gen_data(m, n, k)
            out = torch.empty((m, n), dtype=torch.bfloat16, device="cuda")
            t = dga.tiling(m, n, k)
            fn = lambda: dga.gemm_fp8_fp8_bf16_nt((a, sfa), (b, sfb), out, tiling_=t)
            fn(); torch.cuda.synchronize()
            ok, frac = sweep.is_correct(golden, out, s_abs, short_k=k < 128)
            n_it = 3 if k % 16 else iters
            us_eager = _prewarmed_us(fn, n_it, 30.0)
            timing = "graph"
            try:
                us = _graph_us(fn, n_it)
            except Exception:
                us, timing = us_eager, "eager"
            flops, byt = 2.0 * m * n * k, m * k + n * k + 2 * m * n + 4 * (sfa.numel() + sfb.numel())
            t_mfma, t_hbm = flops / (PEAK_FP8_TFLOPS * 1e6), byt / (PEAK_HBM_GBPS * 1e3)     # us at the two peaks
            bound = "mfma" if t_mfma >= t_hbm else "hbm"
            rows.append({"m": m, "n": n, "k": k, "tile": f"{t.m1}x{t.n1}", "stages": int(t.stages), "splitk": int(t.splitkFactor),
                         "policy": int(t.dispatchPolicyTag), "us": round(us, 2), "us_eager": round(us_eager, 2), "timing": timing, "tflops": round(flops / us / 1e6, 1),
                         "gbps": round(byt / us / 1e3, 1), "bound": bound, "frac": round(max(t_mfma, t_hbm) / us, 4),
                         "parity_ok": bool(ok), "frac_gt_2ulp": frac})
            try:
                # every row under the in-contract policy (bf16-exact arithmetic, its own tiling = what a call without a policy runs):
                # decode rows stream their weights, so the exact arithmetic costs them little -- up to 16-32 rows it runs on the same
                # one-launch kernel as the fast policy; MFMA-bound rows run at the bf16 matrix rate
                tb = dga.tiling(m, n, k, policy="bf16_exact")
                fb = lambda: dga.gemm_fp8_fp8_bf16_nt((a, sfa), (b, sfb), out, tiling_=tb, policy="bf16_exact")
                fb(); torch.cuda.synchronize()
                okb, fracb = sweep.is_correct(golden, out, s_abs, policy="bf16_exact", short_k=k < 128)
                try:
                    usb = _graph_us(fb, n_it)
                except Exception:
                    usb = _prewarmed_us(fb, n_it, 30.0)
                rows[-1].update({"us_in_contract": round(usb, 2), "in_contract_tile": f"{tb.m1}x{tb.n1}", "in_contract_kernel": int(tb.kernelSerial),
                                 "in_contract_parity_ok": bool(okb), "in_contract_frac_gt_2ulp": fracb,
                                 "in_contract_frac": round(max(t_mfma, t_hbm) / usb, 4)})
            except Exception as e:
                rows[-1]["in_contract_error"] = repr(e)
            if bound == "hbm" and k % 16 == 0:
                # SURVEY 8(d)'s protocol for the HBM-bound rows: the operand sets rotated past the 256 MB Infinity Cache (a decode GEMM's
                # weights are never warm), the same calls by graph replay -- what harness/sweep.py --cold and the selector's rules go by
                try:
                    opb = m * k + n * k + 2 * m * n
                    sets = [(a, sfa, b, sfb, out)] + [(a.clone(), sfa.clone(), b.clone(), sfb.clone(), torch.empty_like(out))
                                                      for _ in range(min(16, max(3, -(-(320 << 20) // opb))) - 1)]
                    turn = [0]
                    def rot(tt, pol):
                        c = sets[turn[0] % len(sets)]
                        turn[0] += 1
                        dga.gemm_fp8_fp8_bf16_nt((c[0], c[1]), (c[2], c[3]), c[4], tiling_=tt, **({"policy": pol} if pol else {}))
                    for key, tt, pol in (("us_cold", t, None), ("us_in_contract_cold", dga.tiling(m, n, k, policy="bf16_exact"), "bf16_exact")):
                        for _ in range(len(sets)):
                            rot(tt, pol)
                        torch.cuda.synchronize()
                        rows[-1][key] = round(_graph_us(lambda: rot(tt, pol), max(n_it, len(sets))), 2)
                    rows[-1]["frac_cold"] = round(t_hbm / rows[-1]["us_cold"], 4)
                    rows[-1]["in_contract_frac_cold"] = round(t_hbm / rows[-1]["us_in_contract_cold"], 4)
                    del sets
                except Exception as e:
                    rows[-1]["cold_error"] = repr(e)
            if k % 16:
                # the same bytes in rows round_up(K, 16) apart with zero tails (what the quantisers' aligned_rows forms write):
                # read in place, no padding pass -- both operands, and the weights alone (padded once at load time)
                def aligned(x):
                    ld = (k + 127) // 128 * 128
                    buf = torch.zeros((x.shape[0], ld), dtype=torch.uint8, device="cuda")
                    buf[:, :k] = x.view(torch.uint8)
                    return buf[:, :k]
                a2, b2 = aligned(a), aligned(b)
                out2 = torch.empty_like(out)
                for key, (aa, bb, zp) in {"us_rows_aligned": (a2, b2, (True, True)), "us_weights_aligned": (a, b2, (False, True))}.items():
                    f2 = lambda: dga.gemm_fp8_fp8_bf16_nt((aa, sfa), (bb, sfb), out2, tiling_=t, zero_padded=zp)
                    f2(); torch.cuda.synchronize()
                    rows[-1][key + "_same_bytes"] = bool(torch.equal(out2.view(torch.int16), out.view(torch.int16)))
                    try:
                        rows[-1][key] = round(_graph_us(f2, n_it), 2)
                    except Exception:
                        rows[-1][key] = round(_prewarmed_us(f2, n_it, 30.0), 2)
                rows[-1]["frac_rows_aligned"] = round(max(t_mfma, t_hbm) / rows[-1]["us_rows_aligned"], 4)
                del a2, b2, out2
            del a, b, out, golden, s_abs
        except Exception as e:
            rows.append({"m": m, "n": n, "k": k, "error": repr(e)})
    return {"source": "framework/benchmark/benchmark.py:24-44 (the reference's sweep shape list)", "protocol": "warm, auto tiling; us / frac / parity_ok = the fast policy (fp8 matrix instruction), us_in_contract / in_contract_* = the operator's default "
                        "(bf16-exact) under its own tiling; us = device time per call (the calls captured into a HIP graph and replayed), "
                        "us_eager = launch interval of the same calls issued one by one from Python (host-bound below ~6 us); M <= 128 rows: us_in_contract = the "
                        "bf16-exact policy with its own tiling (in_contract_kernel 6 = the one-launch workgroup split-K); K % 16 != 0 rows: "
                        "us = contiguous operands (padding pass + tile kernel), us_rows_aligned = both operands in 16-byte aligned zero-tailed rows "
                        "(read in place), us_weights_aligned = only the weights; HBM-bound rows also COLD (SURVEY 8(d): operand sets rotated past the 256 MB "
                        "Infinity Cache, graph replay): us_cold / frac_cold, us_in_contract_cold / in_contract_frac_cold",
            "shapes": rows}


def widen_leg():
    """The rows either side of the hot path, reported beside the headline metric:
    the contiguous-grouped (prefill MoE) layout and the activation quantiser that feeds the GEMM."""
    import torch
    import deepgemm_ascend_amd as dga
    gen = torch.Generator(device="cuda").manual_seed(7)
    groups, per, n, k = 8, 1024, 4096, 7168
    msum = groups * per
    a = _rand_fp8((msum, k), gen); b = _rand_fp8((groups, n, k), gen)
    sfa = torch.rand((msum, k // 128), device="cuda") + 0.5
    sfb = torch.rand((groups, n // 128, k // 128), device="cuda") + 0.5
    idx = torch.arange(groups, device="cuda", dtype=torch.int32).repeat_interleave(per).contiguous()
    out = torch.empty((msum, n), dtype=torch.bfloat16, device="cuda")
    t = dga.tiling(msum, n, k, groups=groups, contiguous=True)
    us = _prewarmed_us(lambda: dga.m_grouped_gemm_fp8_fp8_bf16_nt_contiguous((a, sfa), (b, sfb), out, idx, tiling_=t), 20, 300.0)   # (273 us inside the clock ramp, 219 behind it)
    tf = 2.0 * msum * n * k / us / 1e6
    res = {"contiguous": {"workload": f"m_grouped_gemm_fp8_fp8_bf16_nt_contiguous G={groups} x {per} rows, N={n} K={k}",
                          "tile": f"{t.m1}x{t.n1}", "kernel_us": round(us, 1),
                          "roofline": {"bound": "mfma", "achieved": round(tf, 1), "peak": PEAK_FP8_TFLOPS,
                                       "unit": "TFLOP/s", "frac": round(tf / PEAK_FP8_TFLOPS, 4)}}}
    del a, b, out
    rows, kk = 32768, 7168
    x = torch.randn((rows, kk), device="cuda", dtype=torch.bfloat16)
    us = _prewarmed_us(lambda: dga.per_token_cast_to_fp8(x), 20, 100.0)
    byt = rows * kk * 3 + rows * (kk // 128) * 4
    res["per_token_cast"] = {"workload": f"per_token_cast_to_fp8 bf16 [{rows},{kk}] -> e4m3fn + 1x128 f32 scales",
                             "kernel_us": round(us, 1), "algorithmic_bytes": byt,
                             "roofline": {"bound": "hbm", "achieved": round(byt / us / 1e3, 1), "peak": PEAK_HBM_GBPS,
                                          "unit": "GB/s", "frac": round(byt / us / 1e3 / PEAK_HBM_GBPS, 4)}}
    del x
    res["operator_bf16"] = operator_16bit_rows()
    return res


def operator_16bit_rows():
    """The reference's operator in its own dtypes -- catlass_dynamic_matmul, bf16 in and out, mat2 stored [N,K] (op_host/
    catlass_dynamic_matmul.cpp:50-80) -- over the 18-shape list; device time by graph replay (warm)."""
    import torch
    import deepgemm_ascend_amd as dga
    from deepgemm_ascend_amd.harness import sweep
    rows = []
    for (m, n, k) in sweep.SHAPE_GROUP:
        g = torch.Generator(device="cuda").manual_seed(m + n + k)
        x = (torch.randn((m, k), device="cuda", generator=g) * 0.5).to(torch.bfloat16)
        w = (torch.randn((n, k), device="cuda", generator=g) * 0.5).to(torch.bfloat16)
        o = torch.empty((m, n), dtype=torch.bfloat16, device="cuda")
        us = _graph_us(lambda: dga.catlass_dynamic_matmul(x, w.t(), o), 10, replays=3, prewarm_ms=30.0)
        flops, byt = 2.0 * m * n * k, 2.0 * (m * k + n * k + m * n)
        t_m, t_h = flops / (PEAK_BF16_TFLOPS * 1e6), byt / (PEAK_HBM_GBPS * 1e3)
        rows.append({"shape": [m, n, k], "us": round(us, 2), "tflops": round(flops / us / 1e6, 1), "gbps": round(byt / us / 1e3, 1),
                     "bound": "mfma" if t_m >= t_h else "hbm", "frac": round(max(t_m, t_h) / us, 3)})
        del x, w, o
    return rows


def reference_benchmark_rows():
    """The reference's own benchmark as it runs it (framework/benchmark/benchmark.py:24-44, :364-377): run_mmad_bench's launch --
    x[M,K] fp16, y[K,N] fp16 read where it lies, z[M,N] f32 -- over the 18-shape list; device time by graph replay (warm)."""
    import torch
    from deepgemm_ascend_amd import _lib, api
    from deepgemm_ascend_amd.harness import sweep
    lib = _lib.lib()
    rows = []
    for (m, n, k) in sweep.SHAPE_GROUP:
        g = torch.Generator(device="cuda").manual_seed(m + n + k)
        x = (torch.randn((m, k), device="cuda", generator=g) * 0.5).to(torch.float16)
        y = (torch.randn((k, n), device="cuda", generator=g) * 0.5).to(torch.float16)
        z = torch.empty((m, n), dtype=torch.float32, device="cuda")

        def fn():
            ws_ptr, ws_bytes = api._mmad_workspace(1, m, n, k, x)
            rc = lib.dga_run_mmad_rtc_ws(x.data_ptr(), y.data_ptr(), z.data_ptr(), 1, m, n, k, api._dt16(x), ws_ptr, ws_bytes,
                                         api._stream_ptr(z))
            if rc != 0:
                raise RuntimeError(f"dga_run_mmad_rtc_ws: {rc}")
        us = _graph_us(fn, 10, replays=3, prewarm_ms=30.0)
        flops, byt = 2.0 * m * n * k, 2.0 * (m * k + n * k) + 4.0 * m * n
        t_m, t_h = flops / (PEAK_BF16_TFLOPS * 1e6), byt / (PEAK_HBM_GBPS * 1e3)
        rows.append({"shape": [m, n, k], "us": round(us, 2), "tflops": round(flops / us / 1e6, 1), "gbps": round(byt / us / 1e3, 1),
                     "bound": "mfma" if t_m >= t_h else "hbm", "frac": round(max(t_m, t_h) / us, 3)})
        del x, y, z
    return rows


class _HostStagedCollectives:
    """--rehearse-shared-gpu only: torch.distributed's interface as this file and parallel.py use it, every device tensor staged
    through the host around a gloo collective (RCCL refuses two ranks on one device)."""

    def __init__(self, dist):
        self._d = dist
        self.ReduceOp = dist.ReduceOp

    @staticmethod
    def _host(t):
        import torch
        torch.cuda.current_stream().synchronize()
        return t.detach().cpu()

    def barrier(self):
        self._d.barrier()

    def all_reduce(self, t, op=None):
        c = self._host(t)
        self._d.all_reduce(c, op=op if op is not None else self.ReduceOp.SUM)
        t.copy_(c)

    def all_gather(self, outs, t):
        c = self._host(t)
        cs = [c.new_empty(c.shape) for _ in outs]
        self._d.all_gather(cs, c)
        for o, x in zip(outs, cs):
            o.copy_(x)

    def all_to_all_single(self, out, inp):
        c = self._host(inp).contiguous()
        o = c.new_empty(tuple(out.shape))
        self._d.all_to_all_single(o, c)
        out.copy_(o)

    def all_gather_object(self, objs, obj):
        self._d.all_gather_object(objs, obj)

    def get_world_size(self):
        return self._d.get_world_size()

    def get_rank(self):
        return self._d.get_rank()

    def destroy_process_group(self):
        self._d.destroy_process_group()


# --------------------------------------------------------------------------------------------------- main

def main():
    args = parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(args))

    import torch
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE {world}: start it as `python bench.py --gpus {args.gpus}` "
              f"(it spawns the ranks) or under torch.distributed.run with --nproc-per-node {args.gpus}", file=sys.stderr)
        sys.exit(2)
    dist = None
    backend = None
    if world > 1:
        import torch.distributed as dist_mod
        dist = dist_mod
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.stub:
            backend = "gloo"
            dist.init_process_group(backend)
        elif args.rehearse_shared_gpu:
            backend = "gloo, host-staged, every rank on cuda:0 (REHEARSAL of the control flow, not a measurement)"
            local_rank = 0
            torch.cuda.set_device(0)
            dist.init_process_group("gloo")
            dist = _HostStagedCollectives(dist)
        else:
            backend = "nccl"   # RCCL on ROCm
            torch.cuda.set_device(local_rank)
            dist.init_process_group(backend, device_id=torch.device("cuda", local_rank))
    elif not args.stub:
        torch.cuda.set_device(0)
    dev = "cpu" if args.stub else "cuda"

    def sync():
        if not args.stub:
            torch.cuda.synchronize()

    m, n, k = WORKLOADS[args.workload]
    dga = None
    pol = args.policy
    if args.stub:
        import numpy as np
        xs = np.ones((64, 64), np.float32)
        out = np.empty((64, 64), np.float32)
        t = None

        def step():
            np.matmul(xs, xs, out=out)
    else:
        import deepgemm_ascend_amd as dga_mod
        dga = dga_mod
        dga.lib()  # fails loudly if libdga_hip.so is missing
        a, sfa, b, sfb = make_dense_inputs(m, n, k, seed=rank)
        out = torch.empty((m, n), dtype=torch.bfloat16, device="cuda")
        t = dga.tiling(m, n, k, policy=pol if pol == "bf16_exact" else None)

        def step():   # the operator call as a caller makes it: the plan comes from the (m,n,k) cache on every call
            dga.gemm_fp8_fp8_bf16_nt((a, sfa), (b, sfb), out, policy=pol)

    t_pre = time.perf_counter()
    while not args.stub and (time.perf_counter() - t_pre) * 1e3 < args.prewarm_ms:   # untimed: sustained clocks
        for _ in range(50):
            step()
        sync()
    for _ in range(args.warmup):
        step()
    sync()
    if dist:
        dist.barrier()
    sync()
    # HIP events on the stream the kernel is launched on (torch's current stream)
    if not args.stub:
        ev0 = torch.cuda.Event(enable_timing=True); ev1 = torch.cuda.Event(enable_timing=True)
        ev0.record()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    if not args.stub:
        ev1.record()
    sync()
    t_local = time.perf_counter() - t0
    if dist:
        dist.barrier()
    sync()
    elapsed = time.perf_counter() - t0
    kernel_us = (ev0.elapsed_time(ev1) * 1e3 / args.steps) if not args.stub else t_local * 1e6 / args.steps
    per_rank_us = [round(kernel_us, 3)]
    if dist:
        tt = torch.tensor([elapsed, kernel_us], device=dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt[0])
        gathered = [torch.zeros(1, device=dev, dtype=torch.float64) for _ in range(world)]
        dist.all_gather(gathered, torch.tensor([kernel_us], device=dev, dtype=torch.float64))
        per_rank_us = [round(float(x), 3) for x in gathered]
        kernel_us = float(tt[1])
    # what the last timed step handed its caller, taken before any later leg reuses `out`
    dumped = dump_outputs(args.dump_outputs, {"out": dump_rows(out)}) if args.dump_outputs and rank == 0 else None

    # what the ranks saw: so that the first real multi-GPU run of this line can be read without the logs
    ranks_seen = None
    if dist and not args.stub:
        mine = {"rank": rank, "local_rank": local_rank, "device": torch.cuda.get_device_name(local_rank),
                "cus": torch.cuda.get_device_properties(local_rank).multi_processor_count, "host": socket.gethostname()}
        ranks_seen = [None] * world
        dist.all_gather_object(ranks_seen, mine)
    flops = 2.0 * m * n * k
    value = world * flops * args.steps / elapsed / 1e12
    res = {
        "metric": "fp8 TFLOPS + % MFMA peak, 4096^3 block-scaled GEMM; grouped-GEMM tok/s at 1/2/4/8 GPU",
        "value": round(value, 2), "unit": "TFLOP/s", "n_gpus": dist.get_world_size() if dist else 1, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 5), "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None,
        "dtype": "bf16" if pol == "bf16_exact" else "fp8_e4m3fn",   # the arithmetic type the timed path multiplies in (operands are e4m3fn bytes either way)
        "data": "synthetic",
        "config": {"workload": f"{args.workload}: gemm_fp8_fp8_bf16_nt M={m} N={n} K={k}, e4m3fn operands, per-1x128 / per-128x128 f32 scales, bf16 out",
                   "policy": pol, "tile": f"{t.m1}x{t.n1}x{t.k1}" if t is not None else None,
                   "parallelism": "replicas" if world > 1 else "single", "prewarm_ms": args.prewarm_ms,
                   "backend": backend, "stub": bool(args.stub)},
        "per_rank_kernel_us": per_rank_us,
    }
    if dumped is not None:
        res["dumped_outputs"] = {"dir": str(args.dump_outputs), "arrays": dumped}
    if ranks_seen is not None:
        try:
            ver = torch.cuda.nccl.version()
        except Exception as e:
            ver = repr(e)
        res["distributed"] = {"backend": backend, "rccl_version": ver, "world_size": world, "ranks": ranks_seen}
    if args.stub:
        if rank == 0:
            emit(res, args)
        if dist:
            dist.barrier()
            dist.destroy_process_group()
        return

    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    res["roofline"] = roofline_mfma(dga, a, sfa, b, sfb, out, t, m, n, k, kernel_us, cus, policy=pol)
    if args.workload == "dense_4096":
        res["roofline"]["traffic"] = pmc_traffic("dense" if pol == "fast" else "dense_bf16_exact")
        res["roofline"]["traffic_source"] = "committed: " + str(pmc_traffic_source())
        if rank == 0 and world == 1 and not args.no_live_traffic:   # the counters of THIS run where rocprofv3 is there to take them
            live, how = live_pmc_traffic(m, n, k, policy=pol)
            if live is not None:
                res["roofline"]["traffic_committed"] = res["roofline"]["traffic"]
                res["roofline"]["traffic"], res["roofline"]["traffic_source"] = live, how
            else:
                res["roofline"]["traffic_live_error"] = how

    if rank == 0 and not args.no_parity:
        try:
            dga.gemm_fp8_fp8_bf16_nt((a, sfa), (b, sfb), out, policy=pol, sync=True)
            res["parity"] = parity_vs_strict(dga, a, sfa, b, sfb, out, policy=pol)
        except Exception as e:
            res["parity"] = {"error": repr(e)}

    # the three arithmetic policies side by side (rank 0; the headline above is the `pol` column)
    ceilings = {}
    strict_out = None
    if rank == 0 and not args.no_policies:
        for cp in ("fast", "bf16_exact"):
            try:
                ceilings[cp] = dga.mfma_ceiling(cp, launches=300)
            except Exception as e:
                ceilings[cp] = None
                res.setdefault("ceiling_errors", {})[cp] = repr(e)
        if ceilings.get(pol):
            res["roofline"]["ceiling_tflops"] = round(ceilings[pol], 1)
            res["roofline"]["frac_of_ceiling"] = round(res["roofline"]["achieved"] / ceilings[pol], 4)
        res["policies"], strict_out = policy_legs(dga, a, sfa, b, sfb, m, n, k, args, pol,
                                                  {"kernel_us": round(kernel_us, 3), "roofline": res["roofline"],
                                                   "parity": res.get("parity")}, ceilings)
        res["in_contract"] = in_contract(res["policies"])
        fx = res["policies"].get("fast", {}).get("roofline")
        if isinstance(fx, dict) and args.workload == "dense_4096" and pol != "fast":
            fx["traffic"] = pmc_traffic("dense")
            fx["traffic_source"] = "committed: " + str(pmc_traffic_source())
            fx["algorithmic_bytes"] = res["roofline"]["algorithmic_bytes"]

    # the same problem quantised with power-of-two ("UE8M0") scales -- upstream DeepGEMM's use_ue8m0 recipe -- under the two policies
    # that exploit them: the scales ride in the fp8 MFMA's E8M0 operands / are folded into the exact e4m3 -> bf16 conversions
    if rank == 0 and world == 1 and not args.no_policies and args.workload == "dense_4096":
        try:
            res["ue8m0_scales"] = ue8m0_leg(dga, m, n, k, args)
        except Exception as e:
            res["ue8m0_scales"] = {"error": repr(e)}

    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        res["cpu_baseline"] = cpu_baseline(m, n, k, a, sfa, b, sfb, gpu_out=out, budget_s=args.cpu_budget,
                                           strict_out=strict_out)
        # the strict leg's parity that means something: its rows against the CPU oracle (its comparison with the strict kernel is
        # a comparison with itself)
        sleg = (res.get("policies") or {}).get("strict")
        if isinstance(sleg, dict) and "strict_rows_vs_oracle" in res["cpu_baseline"]:
            sleg["parity_vs_oracle"] = res["cpu_baseline"]["strict_rows_vs_oracle"]
    del strict_out

    # BASELINE configs[2] beside the headline (every rank runs it: replicas, like the headline)
    if not args.no_prefill and args.workload == "dense_4096":
        try:
            pm, pn, pk = WORKLOADS["dsv3_prefill"]
            del a, b, out
            pa, psfa, pb, psfb = make_dense_inputs(pm, pn, pk, seed=100 + rank)
            pout = torch.empty((pm, pn), dtype=torch.bfloat16, device="cuda")
            pt = dga.tiling(pm, pn, pk, policy=pol if pol == "bf16_exact" else None)
            pstep = lambda: dga.gemm_fp8_fp8_bf16_nt((pa, psfa), (pb, psfb), pout, policy=pol)
            # the same untimed clock pre-warm as in front of the headline's steps: this leg follows the CPU baseline, i.e.
            # seconds of an idle GPU, and 200 warm launches (12 ms) alone leave it inside the clock ramp (59 us instead of 55)
            t_pre = time.perf_counter()
            while (time.perf_counter() - t_pre) * 1e3 < args.prewarm_ms:
                for _ in range(50):
                    pstep()
                torch.cuda.synchronize()
            us = _time_us(pstep, max(50, min(args.steps, 400)), 200)
            res["dsv3_prefill"] = {"workload": f"gemm_fp8_fp8_bf16_nt M={pm} N={pn} K={pk} (BASELINE configs[2])", "policy": pol,
                                   "value": round(2.0 * pm * pn * pk / us / 1e6, 2), "unit": "TFLOP/s",
                                   "roofline": roofline_mfma(dga, pa, psfa, pb, psfb, pout, pt, pm, pn, pk, us, cus, policy=pol)}
            res["dsv3_prefill"]["roofline"]["traffic"] = pmc_traffic("dsv3_prefill" if pol == "fast" else "dsv3_prefill_bf16_exact")
            res["dsv3_prefill"]["roofline"]["traffic_source"] = "committed: " + str(pmc_traffic_source())
            if rank == 0 and not args.no_parity:
                dga.gemm_fp8_fp8_bf16_nt((pa, psfa), (pb, psfb), pout, policy=pol, sync=True)
                res["dsv3_prefill"]["parity"] = parity_vs_strict(dga, pa, psfa, pb, psfb, pout, policy=pol)
            if rank == 0 and not args.no_policies:
                if ceilings.get(pol):
                    pr = res["dsv3_prefill"]["roofline"]
                    pr["ceiling_tflops"] = round(ceilings[pol], 1)
                    pr["frac_of_ceiling"] = round(pr["achieved"] / ceilings[pol], 4)
                res["dsv3_prefill"]["policies"], _ = policy_legs(
                    dga, pa, psfa, pb, psfb, pm, pn, pk, args, pol,
                    {"kernel_us": round(us, 3), "roofline": res["dsv3_prefill"]["roofline"],
                     "parity": res["dsv3_prefill"].get("parity")}, ceilings)
            del pa, pb, pout
        except Exception as e:
            res["dsv3_prefill"] = {"error": repr(e)}

    if not args.no_grouped:
        try:
            grouped = grouped_leg(args, rank, world, dist)
            if isinstance(grouped.get("roofline"), dict) and world == 1 and args.groups == 256 and args.grouped_mask == "full":
                grouped["roofline"]["traffic"] = pmc_traffic("grouped" if pol == "fast" else "grouped_bf16_exact")
                grouped["roofline"]["traffic_source"] = "committed: " + str(pmc_traffic_source())
            res["grouped"] = grouped
        except Exception as e:  # the primary metric must still be reported
            res["grouped"] = {"error": repr(e)}
    if rank == 0 and world == 1 and not args.no_shape_list:
        try:
            res["shape_list"] = shape_list_leg(dga)
        except Exception as e:
            res["shape_list"] = {"error": repr(e)}
        # the same list through the call the reference's own benchmark makes (16-bit, its own operator slot): ~5 s
        try:
            res["reference_benchmark_fp16"] = {"source": "framework/benchmark/benchmark.py:24-44, :364-377 -- run_mmad_bench(x[M,K] fp16, "
                                                         "y[K,N] fp16, z[M,N] f32); warm, device time by graph replay",
                                               "shapes": reference_benchmark_rows()}
        except Exception as e:
            res["reference_benchmark_fp16"] = {"error": repr(e)}
    if rank == 0 and world == 1 and args.widen:
        try:
            res["widen"] = widen_leg()
        except Exception as e:
            res["widen"] = {"error": repr(e)}
    if rank == 0:
        emit(res, args)
    if dist:
        dist.barrier()
        dist.destroy_process_group()


# --------------------------------------------------------------------------------------------------- output

COMPACT_LIMIT = 4096   # bytes: the driver reads the LAST stdout line; a 21 KB line went unparsed in round 4


def _pick(d, keys):
    return {k: d[k] for k in keys if isinstance(d, dict) and k in d and d[k] is not None}


def compact(res: dict) -> dict:
    """The record the driver parses: the contract's keys + `roofline` + `cpu_baseline` in full meaning but few columns, and one
    short object per side leg.  Everything else (every policy's roofline, the 18-shape list, the reference's own benchmark
    list, per-phase times ...) is in the detail file named by `detail`.  Counterpart of the reference harness's one short
    Result record per run (framework/benchmark/benchmark.py:195-225, 420-428)."""
    c = _pick(res, ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "dtype", "data"))
    c["vs_baseline"] = res.get("vs_baseline")
    cfg = res.get("config") or {}
    c["config"] = _pick(cfg, ("workload", "policy", "tile", "parallelism", "backend"))
    if cfg.get("stub"):
        c["config"]["stub"] = True
    if "roofline" in res:
        r = res["roofline"]
        c["roofline"] = _pick(r, ("bound", "achieved", "peak", "unit", "frac", "kernel_us", "algorithmic_bytes", "kernel", "policy",
                                  "instruction_peak", "frac_of_instruction_peak", "clock_mhz", "frac_at_measured_clock",
                                  "ceiling_tflops", "frac_of_ceiling"))
        c["roofline"]["traffic"] = r.get("traffic")
        if r.get("traffic_source"):
            c["roofline"]["traffic_source"] = "this run (rocprofv3 --pmc child passes)" if str(r["traffic_source"]).startswith("this run") else "committed profiles/ pass"
        if isinstance(r.get("kernel"), str) and len(r["kernel"]) > 64:
            c["roofline"]["kernel"] = r["kernel"][:61] + "..."
    if "cpu_baseline" in res:
        cb = res["cpu_baseline"]
        c["cpu_baseline"] = _pick(cb, ("value", "unit", "cores", "kind", "blas_value"))
        if cb.get("sample"):
            c["cpu_baseline"]["sample"] = str(cb["sample"])[:120]
        if isinstance(cb.get("gpu_rows_vs_oracle"), dict):
            c["cpu_baseline"]["gpu_rows_vs_oracle"] = _pick(cb["gpu_rows_vs_oracle"], ("rows", "max_ulp", "frac_gt_2ulp"))
    if isinstance(res.get("parity"), dict):
        c["parity"] = _pick(res["parity"], ("elements", "max_ulp", "frac_gt_2ulp", "elements_gt_2ulp", "worst_excess_over_S", "within_bar", "error"))
    if isinstance(res.get("in_contract"), dict):
        c["in_contract"] = _pick(res["in_contract"], ("policy", "value", "unit", "kernel_us", "frac_of_fp8_peak", "frac_gt_2ulp", "max_ulp"))
    pols = res.get("policies") or {}
    for name in ("fast", "bf16_exact", "strict"):
        leg = pols.get(name)
        if isinstance(leg, dict) and name != (res.get("config") or {}).get("policy"):
            o = _pick(leg, ("value", "kernel_us", "error"))
            if isinstance(leg.get("roofline"), dict):
                o["frac_of_fp8_peak"] = leg["roofline"].get("frac")
            if isinstance(leg.get("parity"), dict):
                o.update(_pick(leg["parity"], ("max_ulp", "frac_gt_2ulp")))
            if isinstance(leg.get("parity_vs_oracle"), dict):
                o["bit_identical_to_cpu_oracle"] = leg["parity_vs_oracle"].get("bit_identical")
            c[name] = o
    if isinstance(res.get("ue8m0_scales"), dict):
        c["ue8m0_scales"] = {kk: (_pick(vv, ("value", "kernel_us", "frac_of_fp8_peak", "frac_gt_2ulp", "max_ulp")) if isinstance(vv, dict) else vv)
                             for kk, vv in res["ue8m0_scales"].items() if kk != "recipe"}
    if isinstance(res.get("dsv3_prefill"), dict):
        dp = res["dsv3_prefill"]
        o = _pick(dp, ("policy", "value", "unit", "error"))
        if isinstance(dp.get("roofline"), dict):
            o.update(_pick(dp["roofline"], ("frac", "kernel_us")))
        if isinstance(dp.get("parity"), dict):
            o.update(_pick(dp["parity"], ("max_ulp", "frac_gt_2ulp")))
        fl = (dp.get("policies") or {}).get("fast")
        if isinstance(fl, dict) and dp.get("policy") != "fast":
            o["fast"] = _pick(fl, ("value", "kernel_us"))
        c["dsv3_prefill"] = o
    if isinstance(res.get("grouped"), dict):
        g = res["grouped"]
        o = _pick(g, ("policy", "n_gpus", "tokens", "tok_per_s_gemm_only", "tok_per_s_with_alltoall", "ms_gemm", "ms_end_to_end", "error"))
        if isinstance(g.get("roofline"), dict):
            o["roofline"] = _pick(g["roofline"], ("bound", "achieved", "peak", "unit", "frac", "kernel_us", "algorithmic_bytes", "traffic"))
        for side in ("fast", "in_contract"):
            if isinstance(g.get(side), dict):
                o[side] = _pick(g[side], ("policy", "tok_per_s_gemm_only", "ms_gemm", "frac_of_8TBps"))
        if isinstance(g.get("parity"), dict):
            o["parity"] = {kk: _pick(vv, ("max_ulp", "frac_gt_2ulp")) for kk, vv in g["parity"].items() if isinstance(vv, dict)}
        # the GEMM alone under SURVEY 8(d)'s second mask, randint(0, m_max + 1): where the rows that do not exist are skipped
        if isinstance(g.get("random_mask"), dict) and isinstance(g["random_mask"].get("roofline"), dict):
            o["random_mask"] = {"tok_per_s_gemm_only": g["random_mask"].get("tok_per_s_gemm_only"),
                                **_pick(g["random_mask"]["roofline"], ("kernel_us", "frac"))}
        if isinstance(g.get("dropped_tokens"), dict):
            o["dropped_tokens"] = g["dropped_tokens"].get("timed_steps")
        c["grouped"] = o
    if isinstance(res.get("shape_list"), dict) and isinstance(res["shape_list"].get("shapes"), list):
        rows = [r for r in res["shape_list"]["shapes"] if "frac" in r]
        if rows:
            fr = sorted(r["frac"] for r in rows)
            fi = sorted(r["in_contract_frac"] for r in rows if "in_contract_frac" in r) or [None]
            c["shape_list"] = {"shapes": len(res["shape_list"]["shapes"]),
                               "in_contract": {"parity_ok": sum(1 for r in rows if r.get("in_contract_parity_ok")), "frac_of_bound_min": fi[0],
                                               "frac_of_bound_median": fi[len(fi) // 2], "frac_of_bound_max": fi[-1]},
                               "fast": {"parity_ok": sum(1 for r in rows if r.get("parity_ok")), "frac_of_bound_min": fr[0],
                                        "frac_of_bound_median": fr[len(fr) // 2], "frac_of_bound_max": fr[-1]}}
            cold = sorted(r["in_contract_frac_cold"] for r in rows if "in_contract_frac_cold" in r)
            if cold:     # the HBM-bound rows by SURVEY 8(d)'s protocol (operands rotated past the Infinity Cache)
                c["shape_list"]["in_contract"]["hbm_rows_cold"] = {"rows": len(cold), "frac_of_bound_min": cold[0], "frac_of_bound_median": cold[len(cold) // 2]}
    if "detail" in res:
        c["detail"] = res["detail"]
    if "per_rank_kernel_us" in res and (res.get("n_gpus") or 1) > 1:
        c["per_rank_kernel_us"] = res["per_rank_kernel_us"]
    line = json.dumps(c)
    for drop in ("shape_list", "ue8m0_scales", "dsv3_prefill", "strict", "parity", "cpu_baseline.sample"):   # never expected: a guard, not a plan
        if len(line) < COMPACT_LIMIT:
            break
        if "." in drop:
            a_, b_ = drop.split(".")
            (c.get(a_) or {}).pop(b_, None)
        else:
            c.pop(drop, None)
        line = json.dumps(c)
    return c


def emit(res: dict, args) -> None:
    """Full record -> the detail file (and stderr); ONE compact line -> stdout, last."""
    path = None
    for cand in ([args.detail_out] if args.detail_out else [str(ROOT / "gpurun_out" / "bench_detail.json"), "/tmp/dga_bench_detail.json"]):
        try:
            Path(cand).parent.mkdir(parents=True, exist_ok=True)
            Path(cand).write_text(json.dumps(res, indent=1))
            path = cand
            break
        except OSError:
            continue
    res = dict(res)
    res["detail"] = path
    print("bench.py: full record (every leg and column) in " + str(path), file=sys.stderr, flush=True)
    sys.stdout.flush()
    print(json.dumps(compact(res)), flush=True)


if __name__ == "__main__":
    main()
