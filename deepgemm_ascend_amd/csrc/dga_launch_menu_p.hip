// fp8 tile-kernel menu, part P: the k-grouped weight-gradient builds (KGROUP = 1; dga_k_grouped_wgrad_gemm_fp8_fp8_fp32_nt) -- the
// bf16-exact one-tile tiles (gemm_fp8_kernel.hpp MATH = 1, OUT = 1, SFB_ROWS = 1), the persistent 128 x 256 build
// (gemm_fp8_bf16x_persistent_kernel.hpp) and the strict kernel (gemm_fp8_strict_kernel.hpp).  The raster is G x tiles(M, N); every
// tile reads its group's K from the device counts.  Built with part O's pragma-unroll budget (Makefile FLAGS_dga_launch_menu_p).
#include "dga_fp8_menu_impl.hpp"
#include "gemm_fp8_bf16x_persistent_kernel.hpp"
#include "gemm_fp8_strict_kernel.hpp"
namespace dga {

template <class Kfn>
static int launch_kgroup(Kfn kfn, int lds, unsigned grid, unsigned threads, const GemmParams &p, hipStream_t stream)
{
    static std::once_flag once[64];
    static hipError_t attr_err[64];
    int dev = 0;
    if (int rc = record_hip(hipGetDevice(&dev))) return rc;
    if (dev < 0 || dev >= 64) return DGA_E_HIP;
    if (lds > 0)
        std::call_once(once[dev], [&] {
            attr_err[dev] = hipFuncSetAttribute(reinterpret_cast<const void *>(kfn), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        });
    if (int rc = record_hip(attr_err[dev])) return rc;
    if (grid == 0) return DGA_OK;
    hipLaunchKernelGGL(kfn, dim3(grid), dim3(threads), lds, stream, p);
    return record_hip(hipGetLastError());
}

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
    return launch_kgroup(gemm_fp8_blockscaled_nt_kernel<Cfg, 0, false, false, 1, false, 1, 1, 1>, StageCfg<Cfg, 1>::LDS_BYTES,
                         static_cast<unsigned>(tiles), Cfg::NT, p, stream);
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
    return launch_kgroup(gemm_fp8_bf16x_persistent_kernel<false, 1, 1, 1>, Cfg::LDS_BYTES, grid, Cfg::NT, p, stream);
}

// strict: 64-row tiles (TM = 2) where they fill the CUs, else 32-row tiles (p.tiles_m counts rows of bm)
int launch_strict_kgroup(const GemmParams &p, int bm, hipStream_t stream)
{
    if (!kgroup_params(p)) return DGA_E_TILING;
    const unsigned grid = static_cast<unsigned>(static_cast<int64_t>(p.groups) * p.tiles_m * p.tiles_n);
    if (bm == 64) return launch_kgroup(gemm_fp8_strict_nt_kernel<2, 1, 1, 1>, 0, grid, 256, p, stream);
    if (bm == 32) return launch_kgroup(gemm_fp8_strict_nt_kernel<1, 1, 1, 1>, 0, grid, 256, p, stream);
    return DGA_E_TILING;
}
}
