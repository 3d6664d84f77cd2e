// fp8 tile-kernel menu, part H: the persistent form of the bf16-exact policy's 128 x 256 in-register build
// (gemm_fp8_bf16x_persistent_kernel.hpp, dispatchPolicyTag 7): one workgroup per CU walks the raster, the LDS ring runs across tiles.
#include "dga_fp8_menu_impl.hpp"
#include "gemm_fp8_bf16x_persistent_kernel.hpp"
#include <atomic>
namespace dga {

// ---- which body walks a dense bf16 raster: one tile at a time (this unit) or two stacked tiles at a time
//      (gemm_fp8_bf16x_pair_kernel.hpp, dga_launch_menu_q.hip; same bits).  The paired body runs where pairing adds no raster
//      quantisation: 2 * ceil(pairs / CUs) == ceil(tiles / CUs) -- 4096^3 (256 pairs on 256 CUs) and 8192^3 yes,
//      4096 x 2048 x 7168 (128 pairs would idle half the CUs) no.
static std::atomic<int> pair_force{-1}, pair_grid{0}, pair_last{-1};
static bool bf16x_pair_rule(int64_t tiles_m, int64_t tiles_n, int64_t cus)
{
    const int64_t tiles = tiles_m * tiles_n, pairs = ((tiles_m + 1) / 2) * tiles_n;
    return 2 * ((pairs + cus - 1) / cus) == (tiles + cus - 1) / cus;
}

template <int OUT, int SFB_ROWS>
static int launch_bf16x_persistent_one(const GemmParams &p, hipStream_t stream)
{
    typedef GemmCfg<128, 256, 2, 4, 3> Cfg;
    const int64_t tiles = p.launch_tiles > 0 ? p.launch_tiles : static_cast<int64_t>(p.groups) * p.tiles_m * p.tiles_n;
    const unsigned grid = static_cast<unsigned>(std::min<int64_t>(tiles, device_cus()));
    return (p.k % 128) ? launch_kernel<gemm_fp8_bf16x_persistent_kernel<true, OUT, SFB_ROWS>>(grid, Cfg::NT, Cfg::LDS_BYTES, stream, p)
                       : launch_kernel<gemm_fp8_bf16x_persistent_kernel<false, OUT, SFB_ROWS>>(grid, Cfg::NT, Cfg::LDS_BYTES, stream, p);
}

// Rasters of at least two k blocks.  Bf16 rows: dense and masked-grouped rasters (launch_tiles > 0: the first tiles of a dense raster --
// the whole rounds in front of a quarter-tile tail).  The fp32 forms: dense rasters.  Split-K, the quarter tiles themselves, indexed
// rows and the contiguous layout keep the one-tile build.
int launch_bf16x_persistent(const GemmParams &p, Out out, hipStream_t stream)
{
    if (p.tail_sub || p.m_indices || p.row_index || p.splitk > 1 || p.kb_n < 2) return DGA_E_TILING;
    if (out == Out::Bf16 && p.groups == 1 && !p.masked_m && p.launch_tiles == 0 && p.k % 128 == 0) {
        const int force = pair_force.load(std::memory_order_relaxed);
        if (force >= 0 ? force != 0 : bf16x_pair_rule(p.tiles_m, p.tiles_n, device_cus())) {
            const int grid = pair_grid.load(std::memory_order_relaxed);
            GemmParams q = p;
            if (grid > 0) q.xcd_remap = 0;   // (a grid of any size walks the raster in plain order)
            const int rc = launch_bf16x_pair(q, grid > 0 ? static_cast<unsigned>(grid) : 0u, stream);
            if (rc != DGA_E_TILING) {
                pair_last.store(1, std::memory_order_relaxed);
                return rc;
            }
        }
    }
    pair_last.store(0, std::memory_order_relaxed);
    if (out == Out::Bf16) return (p.launch_tiles > 0 && p.groups != 1) ? DGA_E_TILING : launch_bf16x_persistent_one<0, 0>(p, stream);
    if (p.masked_m || p.groups != 1) return DGA_E_TILING;
    return out == Out::F32 ? launch_bf16x_persistent_one<1, 0>(p, stream) : launch_bf16x_persistent_one<1, 1>(p, stream);
}
}

// Diagnostics (not part of include/dga_hip.h; scripts and tests reach them through the loaded library).
// force: -1 the launcher's rule, 0 never the paired body, 1 the paired body wherever it can run; grid > 0: that many workgroups for
// the paired body.  Returns the previous `force`.
extern "C" __attribute__((visibility("default"))) int dga_diag_bf16x_pair_force(int force, int grid)
{
    dga::pair_grid.store(grid > 0 ? grid : 0, std::memory_order_relaxed);
    return dga::pair_force.exchange(force < 0 ? -1 : (force != 0), std::memory_order_relaxed);
}
// 1: the launcher's rule gives a dense M x N raster of 128 x 256 tiles to the paired body on this device (K permitting)
extern "C" __attribute__((visibility("default"))) int dga_diag_bf16x_pair_rule(int m, int n)
{
    if (m < 1 || n < 1) return 0;
    return dga::bf16x_pair_rule((m + 127) / 128, (n + 255) / 256, dga::device_cus()) ? 1 : 0;
}
// the body of the last launch through launch_bf16x_persistent: 1 paired, 0 one tile at a time, -1 none yet
extern "C" __attribute__((visibility("default"))) int dga_diag_bf16x_pair_last(void)
{
    return dga::pair_last.load(std::memory_order_relaxed);
}
