"""Cross-compiles csrc/dga_sparse_mla.hip and csrc/dga_sparse_mla_merge.hip with the library's flags and prints, per kernel, the resource usage the compiler reports and the
instruction counts of the kernel's whole text: the two table lines per kernel of profiles/sparse_mla_isa.txt.  No device is needed.
Usage: python scripts/sparse_mla_isa.py [--hipcc /opt/rocm/bin/hipcc] [--keep out.s]"""
import argparse
import re
import subprocess
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "deepgemm_ascend_amd" / "csrc"
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{ROOT / 'include'}", f"-I{CSRC}", "-fno-slp-vectorize", "-mllvm",
         "-amdgpu-mfma-vgpr-form=1", "-x", "hip", "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage"]
COUNTED = ("v_mfma_f32_16x16x32_bf16", "ds_read_b128", "ds_read_b64_tr_b16", "ds_write_b128", "ds_write_b32", "global_load_dwordx4",
           "global_load_dword", "global_store_dwordx2", "global_store_dword", "v_exp_f32", "v_log_f32", "v_cvt_pk_bf16_f32", "v_cvt_pk_f32_fp8",
           "v_mul_f32", "v_pk_mul_f32", "ds_bpermute_b32", "s_barrier", "v_accvgpr_write_b32", "v_accvgpr_read_b32", "scratch_", "global_atomic")
# (the one-pass instantiations keep the names they had before the PARTIAL axis existed)
NAMES = {"SmlaBf16RowsELb0": "sparse_mla_fwd_kernel<SmlaBf16Rows>", "SmlaFp8RowsELb0": "sparse_mla_fwd_kernel<SmlaFp8Rows>",
         "SmlaBf16RowsELb1": "sparse_mla_fwd_kernel<SmlaBf16Rows, PARTIAL>", "SmlaFp8RowsELb1": "sparse_mla_fwd_kernel<SmlaFp8Rows, PARTIAL>",
         "sparse_mla_merge_kernel": "sparse_mla_merge_kernel"}
SPLIT_COUNTED = ("global_store_dwordx4",)                    # counted for the split kernels only: the one-pass lines stay as they were
ONE_PASS = ("sparse_mla_fwd_kernel<SmlaBf16Rows>", "sparse_mla_fwd_kernel<SmlaFp8Rows>")
UNITS = ("dga_sparse_mla.hip", "dga_sparse_mla_merge.hip")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hipcc", default="/opt/rocm/bin/hipcc")
    ap.add_argument("--keep", default=None)
    args = ap.parse_args()
    text, remarks = "", ""
    with tempfile.TemporaryDirectory() as tmp:
        for unit in UNITS:                                     # (--keep names the first unit's assembly; the merge's goes beside it)
            asm = Path(args.keep + ("" if unit == UNITS[0] else ".merge")) if args.keep else Path(tmp) / (unit + ".s")
            run = subprocess.run([args.hipcc] + FLAGS + ["-o", str(asm), str(CSRC / unit)], capture_output=True, text=True, check=True)
            text += asm.read_text()
            remarks += run.stderr
    usage = {}
    for block in remarks.split("Function Name: ")[1:]:
        sym = block.split()[0]
        get = lambda key: int(re.search(re.escape(key) + r": (\d+)", block).group(1))
        usage[sym] = [get("VGPRs"), get("AGPRs"), get("TotalSGPRs"), get("ScratchSize [bytes/lane]"), get("SGPRs Spill"), get("VGPRs Spill"),
                      get("LDS Size [bytes/block]"), get("Occupancy [waves/SIMD]")]
    print("kernel  VGPRs  AGPRs  SGPRs  scratch[B/lane]  sspill  vspill  LDS[B]  occupancy[waves/SIMD]")
    for sym, row in usage.items():
        name = next(v for k, v in NAMES.items() if k in sym)
        print(name + "  " + "  ".join(map(str, row)))
        body = text[text.index("\n" + sym + ":"):text.index(".Lfunc_end", text.index("\n" + sym + ":"))]
        ops = [line.split()[0] for line in body.splitlines() if line.startswith("\t") and not line.lstrip().startswith((".", ";"))]
        counts = []
        for op in COUNTED + (() if name in ONE_PASS else SPLIT_COUNTED):
            whole = (op, op + "_e32", op + "_e64", op + "_sdwa", op + "_dpp")
            n = sum(o.startswith(op) for o in ops) if op.endswith("_") or op == "global_atomic" else sum(o in whole for o in ops)
            counts.append(f"{op} {n}")
        print(name + " instructions: " + ", ".join(counts))


if __name__ == "__main__":
    main()
