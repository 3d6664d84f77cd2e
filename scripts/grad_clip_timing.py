"""Times the device-side gradient norm, clip and skip, to scripts/adamw_cast_timing.py's protocol: the forms of a comparison run alternately
in one process on the same tensors, in windows of back-to-back calls between two device events (each window sized to over 150 ms after
a calibration), after a warm-up; mean and min..max over the windows.  Results are compared before any time is reported.
Cases: gradients [8, 4096, 7168] and [32, 7168, 2048] in float32 and in bfloat16, and a list of 64 float32 tensors [1024, 1024].
  1  clip_grad_norm_step_scalars(tensors, step_scalars, max_norm, out=...) against the torch expression it replaces:
     torch._foreach_norm -> stack -> norm -> coefficient -> copy_ into step_scalars[3].  Condition: new / old < 1.0 on the two grouped
     float32 cases; no ratio is fixed in advance.
  2  TB/s of the bytes grad_sumsq reads (4 or 2 per element) over its own mean time.  Yardstick: per_block_cast_to_fp8_transposed's
     5.3 - 5.6 TB/s on the grouped cases.
  3  adamw_per_block_cast_to_fp8_transposed's C entry (no flag) of this build against the same entry of the parent commit's library
     (--parent-lib: its libdga_hip.so built into a scratch directory, loaded beside this one), on the two grouped float32 cases without
     rowwise, and this build's entry with a flag that is zero.  Condition: new - parent <= the min..max spread of the parent's own windows.
Usage: python scripts/grad_clip_timing.py [--out profiles/grad_clip_timing.txt] [--windows N] [--parent-lib PATH]"""
import argparse
import ctypes
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import deepgemm_ascend_amd as dga  # noqa: E402
from deepgemm_ascend_amd import _lib  # noqa: E402
from scripts.cast_transposed_timing import alternate  # noqa: E402

GROUPED = ((8, 4096, 7168), (32, 7168, 2048))
MAX_NORM, EPS = 1.0, 1e-6
LR, BETAS, ADAM_EPS, WD, STEP = 3e-4, (0.9, 0.95), 1e-8, 0.1, 3
PLAIN = "dga_adamw_cast_to_fp8_128x128_transposed"


def torch_clip(tensors, sc):
    norms = torch._foreach_norm(tensors)
    total = torch.linalg.vector_norm(torch.stack(norms).float())
    sc[3:4].copy_(torch.clamp(MAX_NORM / (total + EPS), max=1.0))
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--windows", type=int, default=4)
    ap.add_argument("--parent-lib", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    fmt = lambda v: f"{v.mean():8.1f} [{v.min():8.1f}..{v.max():8.1f}] us"
    say(f"# {torch.cuda.get_device_name(0)}; device events around windows of back-to-back calls (>= 150 ms each), {args.windows} windows per "
        f"form, alternating; mean [min..max] us per call")
    say("# 1, 2: new = clip_grad_norm_step_scalars(out=...), old = torch._foreach_norm -> stack -> norm -> coefficient -> copy_ into "
        "step_scalars[3]; sumsq = grad_sumsq(out=...) alone, TB/s of the bytes it reads; condition: new / old < 1.00 on the grouped float32 cases")
    cases = [(f"{list(s)} {name}", [s], dt) for s in GROUPED for name, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16))]
    cases.append(("64 x [1024, 1024] fp32", [(1024, 1024)] * 64, torch.float32))
    missed = []
    for name, shapes, dt in cases:
        g = torch.Generator(device="cuda").manual_seed(len(name))
        tensors = [(torch.randn(s, device="cuda", generator=g) * 1e-3).to(dt) for s in shapes]
        elems = sum(t.numel() for t in tensors)
        sc_new, sc_old = (torch.tensor([LR, 0.5, 0.5, 7.0], device="cuda") for _ in range(2))
        outs = (torch.empty(1, device="cuda"), torch.empty(1, device="cuda"), torch.empty(1, dtype=torch.int32, device="cuda"),
                torch.empty(1, dtype=torch.float64, device="cuda"))
        new = lambda: dga.clip_grad_norm_step_scalars(tensors, sc_new, MAX_NORM, eps=EPS, out=outs)
        old = lambda: torch_clip(tensors, sc_old)
        sumsq = lambda: dga.grad_sumsq(tensors, out=outs[3])
        new()
        total = old()
        torch.cuda.synchronize()
        exact = sum(t.double().square().sum() for t in tensors).sqrt().item()
        tol = 1e-4 if dt == torch.float32 else 1e-2                      # torch's norms are float32 (bfloat16) sums
        assert abs(outs[0].item() - exact) <= 1e-6 * exact, f"{name}: norm {outs[0].item()} against float64 {exact}"
        assert abs(total.item() - exact) <= tol * exact, f"{name}: torch's norm {total.item()} against float64 {exact}"
        assert abs(sc_new[3].item() - sc_old[3].item()) <= tol * sc_new[3].item() and outs[2].item() == 0, f"{name}: step_scalars[3] differs"
        t = alternate([new, old, sumsq], args.windows)
        ratio = t[new].mean() / t[old].mean()
        tb = elems * tensors[0].element_size() / (t[sumsq].mean() * 1e-6) / 1e12
        say(f"{name:28s} | new {fmt(t[new])} | old {fmt(t[old])} | new / old {ratio:5.2f} | sumsq {fmt(t[sumsq])} {tb:4.2f} TB/s")
        if ratio >= 1.0 and dt == torch.float32 and len(shapes) == 1:
            missed.append(name)
        del tensors
        torch.cuda.empty_cache()
    say("# grouped float32 cases where the new form is not faster: " + ("; ".join(missed) if missed else "none"))

    say(f"# 3: {PLAIN}, float32 w, m, v and grad, no rowwise, through the C entry of each library; parent = the parent commit's "
        f"build; flag = this build's _skip entry with a device flag that is 0; condition: new - parent <= max - min of the parent's windows")
    if args.parent_lib is None:
        say("# (no --parent-lib given: not measured)")
    else:
        L = _lib.lib()
        P = ctypes.CDLL(str(Path(args.parent_lib).resolve()))
        res, argtypes = _lib.SIGNATURES[PLAIN]
        getattr(P, PLAIN).restype, getattr(P, PLAIN).argtypes = res, argtypes
        assert not hasattr(P, PLAIN + "_skip"), "--parent-lib is not the parent's build"
        sc = dga.adamw_step_scalars(STEP, LR, *BETAS, device="cuda")
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        regress = []
        for shape in GROUPED:
            g = torch.Generator(device="cuda").manual_seed(sum(shape))
            w0 = torch.randn(shape, device="cuda", generator=g) * 0.05
            grad = torch.randn(shape, device="cuda", generator=g) * 1e-3
            m0 = torch.randn(shape, device="cuda", generator=g) * 5e-4
            v0 = torch.randn(shape, device="cuda", generator=g).square_() * 1e-6 + 1e-12
            groups, n, k = shape
            state = {}
            for who in ("new", "parent", "flag"):
                state[who] = (w0.clone(), m0.clone(), v0.clone(), torch.empty((groups, k, n), dtype=torch.uint8, device="cuda"),
                              torch.empty((groups, (k + 127) // 128, (n + 127) // 128), device="cuda"))

            def entry(lib, who, skip):
                w, m, v, qt, sft = state[who]
                head = (w.data_ptr(), m.data_ptr(), v.data_ptr(), _lib.DT_FP32, grad.data_ptr(), _lib.DT_FP32, sc.data_ptr(), BETAS[0], BETAS[1],
                        ADAM_EPS, WD, groups, n, k, qt.data_ptr(), sft.data_ptr(), None, None, 0)
                if skip is None:
                    fn = getattr(lib, PLAIN)
                    return lambda: fn(*head, stream)
                fn = getattr(lib, PLAIN + "_skip")
                return lambda: fn(*head, skip.data_ptr(), stream)

            new, parent, flagged = entry(L, "new", None), entry(P, "parent", None), entry(L, "flag", flag)
            for fn in (new, parent, flagged):
                assert fn() == 0
            torch.cuda.synchronize()
            for who in ("parent", "flag"):
                for a, b in zip(state["new"], state[who]):
                    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), f"{list(shape)}: new and {who} differ after one step"
            t = alternate([new, parent, flagged], args.windows)
            spread = t[parent].max() - t[parent].min()
            diff = t[new].mean() - t[parent].mean()
            say(f"{str(list(shape)):20s} | new {fmt(t[new])} | parent {fmt(t[parent])} | flag = 0 {fmt(t[flagged])} | new - parent {diff:+6.1f} us, "
                f"parent's spread {spread:5.1f} us")
            if diff > spread:
                regress.append(str(list(shape)))
            del state, w0, grad, m0, v0
            torch.cuda.empty_cache()
        say("# cases slower than the parent by more than the parent's own spread: " + ("; ".join(regress) if regress else "none"))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
