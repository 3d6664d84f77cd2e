// fp8 tile-kernel menu, part P: the k-grouped weight-gradient builds (KGROUP = 1; dga_k_grouped_wgrad_gemm_fp8_fp8_fp32_nt) -- the
// bf16-exact one-tile tiles (gemm_fp8_kernel.hpp MATH = 1, OUT = 1, SFB_ROWS = 1), the persistent 128 x 256 build
// (gemm_fp8_bf16x_persistent_kernel.hpp) and the strict kernel (gemm_fp8_strict_kernel.hpp).  The raster is G x tiles(M, N); every
// tile reads its group's K from the device counts.  Built with part O's pragma-unroll budget (Makefile FLAGS_dga_launch_menu_p).
#include "dga_fp8_menu_impl.hpp"
#include "gemm_fp8_bf16x_persistent_kernel.hpp"
namespace dga {

// the k-grouped raster only: p.ks set, K_total a whole number of k blocks, no split-K, no tail, no row tables
static bool kgroup_params(const GemmParams &p)
{
    return p.ks && p.k % 128 == 0 && p.splitk <= 1 && !p.tail_sub && p.launch_tiles == 0 && !p.m_indices && !p.row_index;
}

template <class Cfg>
int launch_bf16x_kgroup(const GemmParams &p, hipStream_t stream)
{
    if (!kgroup_params(p)) return DGA_E_TILING;
    const int64_t tiles = static_cast<int64_t>(p.groups) * p.tiles_m * p.tiles_n;
    return launch_kernel<gemm_fp8_blockscaled_nt_kernel<Cfg, 0, false, false, 1, false, 1, 1, 1>>(static_cast<unsigned>(tiles), Cfg::NT,
                                                                                                   StageCfg<Cfg, 1>::LDS_BYTES, stream, p);
}
#define DGA_MENU_INSTANTIATE_BX_KGROUP(BM, BN, WM, WN, ST, PP) \
    template int launch_bf16x_kgroup<GemmCfg<BM, BN, WM, WN, ST>>(const GemmParams &, hipStream_t);
DGA_MENU_BX(DGA_MENU_INSTANTIATE_BX_KGROUP)

int launch_bf16x_persistent_kgroup(const GemmParams &p, hipStream_t stream)
{
    if (!kgroup_params(p)) return DGA_E_TILING;
    typedef GemmCfg<128, 256, 2, 4, 3> Cfg;
    const int64_t tiles = static_cast<int64_t>(p.groups) * p.tiles_m * p.tiles_n;
    const unsigned grid = static_cast<unsigned>(std::min<int64_t>(tiles, device_cus()));
    return launch_kernel<gemm_fp8_bf16x_persistent_kernel<false, 1, 1, 1>>(grid, Cfg::NT, Cfg::LDS_BYTES, stream, p);
}

// strict: 64-row tiles (TM = 2) where they fill the CUs, else 32-row tiles (p.tiles_m counts rows of bm)
int launch_strict_kgroup(const GemmParams &p, int bm, hipStream_t stream)
{
    const StrictKernel kfn = strict_kernel<1>(bm, Out::F32Rows);
    if (!kgroup_params(p) || !kfn) return DGA_E_TILING;
    const unsigned grid = static_cast<unsigned>(static_cast<int64_t>(p.groups) * p.tiles_m * p.tiles_n);
    hipLaunchKernelGGL(kfn, dim3(grid), dim3(256), 0, stream, p);
    return record_hip(hipGetLastError());
}
}
