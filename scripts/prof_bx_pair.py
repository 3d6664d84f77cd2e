"""Launch the dense bf16-exact GEMM with one body of the persistent kernel forced (for rocprofv3 A/B runs of the paired body).
  prof_bx_pair.py m n k iters body     body: 0 = one tile at a time, 1 = two stacked tiles at a time, -1 = the launcher's rule
The clock pre-warm (50 launches) is followed by `iters` launches; with --time the script prints the mean of those by events."""
import sys
from pathlib import Path
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch
import deepgemm_ascend_amd as dga
import bench

argv = [x for x in sys.argv[1:] if x != "--time"]
m, n, k, iters, body = (int(x) for x in argv[:5])
a, sfa, b, sfb = bench.make_dense_inputs(m, n, k, seed=0)
out = torch.empty((m, n), dtype=torch.bfloat16, device="cuda")
L = dga.lib()
L.dga_diag_bf16x_pair_force(body, 0)


def launch():
    dga.gemm_fp8_fp8_bf16_nt((a, sfa), (b, sfb), out, policy="bf16_exact")


for _ in range(50):
    launch()
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(iters):
    launch()
e1.record()
torch.cuda.synchronize()
took = L.dga_diag_bf16x_pair_last()
line = f"done {m} {n} {k} body={body} last_launch_paired={took}"
if "--time" in sys.argv:
    line += f" mean_us={e0.elapsed_time(e1) * 1e3 / iters:.2f}"
print(line)
