#!/usr/bin/env python3
"""Compare the gfx950 device code of the fp8 units of two source trees, kernel by kernel.

    python scripts/isa_compare.py PARENT_TREE BRANCH_TREE [--work DIR] [--jobs N] [--units a.hip b.hip ...] [--kernels REGEX] > table.txt

Every unit is compiled in both trees with the flags its Makefile gives it (taken from `make -n`, as tests/test_build.py does),
`--cuda-device-only -S -Rpass-analysis=kernel-resource-usage`.  Comment lines, trailing comments, .file / .loc / .ident and blank
lines are dropped; what is left of every kernel function whose mangled name matches --kernels (default gemm_; the quantiser units:
--units dga_cast.hip dga_silu_mul_cast.hip dga_silu_mul_bwd_cast.hip --kernels cast_) is compared line for line, labels included.  The table has one
row per kernel: identical yes/no and VGPRs / SGPRs / AGPRs / SGPR spill / VGPR spill / scratch / LDS / occupancy before -> after.
A kernel that differs also gets its instruction counts for the mnemonics the main loops are made of.  Assembly already present
under --work is reused (delete the directory to recompile).  Exit status 1 if any kernel differs."""
import argparse
import re
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

UNITS = ["dga_launch.hip", "dga_diag.hip"] + [f"dga_launch_menu_{c}.hip" for c in "abcdefghijklmnop"]
FIELDS = [("VGPRs", "VGPRs"), ("TotalSGPRs", "SGPRs"), ("AGPRs", "AGPRs"), ("SGPRs Spill", "sspill"), ("VGPRs Spill", "vspill"),
          ("ScratchSize [bytes/lane]", "scratch"), ("LDS Size [bytes/block]", "LDS"), ("Occupancy [waves/SIMD]", "occ")]
MNEMONICS = ["v_mfma", "v_cvt_scalef32", "ds_read", "buffer_load", "v_fma", "s_waitcnt", "s_barrier"]


def ship_flags(csrc, unit):
    obj = f"../../build/csrc/{Path(unit).stem}.o"
    out = subprocess.run(["make", "-n", "-B", "-C", str(csrc), obj], capture_output=True, text=True, check=True).stdout
    words = [l for l in out.splitlines() if "hipcc" in l and f" {unit} " in l + " "][-1].split()
    keep, skip = [], False
    for w in words:
        if skip or w in ("-c", unit):
            skip = False
        elif w == "-o":
            skip = True
        else:
            keep.append(w)
    return keep


def compile_unit(tree, unit, work):
    asm, rem = work / (Path(unit).stem + ".s"), work / (Path(unit).stem + ".remarks")
    if not (asm.exists() and rem.exists()):
        csrc = Path(tree) / "deepgemm_ascend_amd" / "csrc"
        cmd = ship_flags(csrc, unit) + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", unit, "-o", str(asm.resolve())]
        r = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True)
        if r.returncode:
            sys.exit(f"{tree}: {unit} does not compile\n{r.stderr[-3000:]}")
        rem.write_text(r.stderr)
    return asm.read_text(), rem.read_text()


def kernels(asm, pattern):
    """name -> normalised lines of every function whose mangled name matches `pattern`"""
    out, name = {}, None
    for line in asm.splitlines():
        m = re.match(r"^(_Z\w*(?:" + pattern + r")\w*):", line)
        if m:
            name = m.group(1)
            out[name] = []
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end"):
            name = None
            continue
        s = line.split(";")[0].rstrip()
        if s.strip() and not re.match(r"\s*\.(file|loc|ident)\b", s):
            out[name].append(s)
    return out


def resources(remarks):
    out, name = {}, None
    for line in remarks.splitlines():
        m = re.search(r"remark: +(?:Function Name: (\S+)|([A-Za-z][A-Za-z /\[\]]*?): (\d+)) \[-Rpass", line)
        if not m:
            continue
        if m.group(1):
            name = m.group(1)
            out[name] = {}
        elif name:
            out[name][m.group(2)] = int(m.group(3))
    return out


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    short = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True).stdout.splitlines() if tool else names
    return {n: s.replace("void dga::", "").replace("(dga::GemmParams)", "") for n, s in zip(names, short)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("--work", default="build/isa_compare")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--units", nargs="*", default=UNITS)
    ap.add_argument("--kernels", default="gemm_", help="regular expression a kernel's mangled name must contain")
    a = ap.parse_args()
    work = {k: Path(a.work) / k for k in ("parent", "branch")}
    for w in work.values():
        w.mkdir(parents=True, exist_ok=True)
    with ThreadPoolExecutor(a.jobs) as ex:
        jobs = {(k, u): ex.submit(compile_unit, getattr(a, k), u, work[k]) for u in a.units for k in work}
        built = {key: f.result() for key, f in jobs.items()}
    differ = total = 0
    print("unit  kernel  identical  " + "  ".join(f"{s}(parent->branch)" for _, s in FIELDS))
    for u in a.units:
        (asm0, rem0), (asm1, rem1) = built[("parent", u)], built[("branch", u)]
        k0, k1, r0, r1 = kernels(asm0, a.kernels), kernels(asm1, a.kernels), resources(rem0), resources(rem1)
        names = demangle(sorted(set(k0) | set(k1)))
        for n in sorted(names):
            same = k0.get(n) == k1.get(n)
            total += 1
            differ += not same
            cols = [f"{r0.get(n, {}).get(f, '-')}->{r1.get(n, {}).get(f, '-')}" for f, _ in FIELDS]
            print(f"{Path(u).stem}  {names[n]}  {'yes' if same else 'NO'}  " + "  ".join(cols))
            if not same:
                for mn in MNEMONICS:
                    c = [sum(1 for l in k.get(n, []) if l.strip().startswith(mn)) for k in (k0, k1)]
                    print(f"    {mn}*: {c[0]} -> {c[1]}")
    print(f"# {total} kernels in {len(a.units)} units, {total - differ} identical, {differ} different")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
