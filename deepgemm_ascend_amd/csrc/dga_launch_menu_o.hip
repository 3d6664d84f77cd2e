// fp8 tile-kernel menu, part O: the bf16-exact builds with fp32 rows and per-row sfb (dga_fp8_menu.hpp; gemm_fp8_kernel.hpp MATH = 1,
// OUT = 1, SFB_ROWS = 1: dga_wgrad_gemm_fp8_fp8_fp32_nt).  A unit of its own: the per-element promotion scale takes the 64-gap k-block
// body of the 8 x 16 x 16 wave tiles past the default pragma-unroll budget (rolled, its register arrays went to scratch), and the
// budget raised for part E would move the schedule of the builds there (Makefile FLAGS_dga_launch_menu_o).
#include "dga_fp8_menu_impl.hpp"
namespace dga {

template <class Cfg, bool KTAIL>
static int launch_bf16x_rows_one(const GemmParams &p, hipStream_t stream)
{
    constexpr int kLds = StageCfg<Cfg, 1>::LDS_BYTES;
    const unsigned grid = p.launch_tiles > 0 ? static_cast<unsigned>(p.launch_tiles)
                                             : static_cast<unsigned>(p.groups) * p.tiles_m * p.tiles_n;
    return launch_kernel<gemm_fp8_blockscaled_nt_kernel<Cfg, 0, KTAIL, false, 1, false, 1, 1>>(grid, Cfg::NT, kLds, stream, p);
}

// dense rasters, the quarter tiles of the tail pair, and the slab pass of the two-launch split-K (promoted partial sums into the
// slabs; the fp32 combine adds C)
template <class Cfg>
int launch_bf16x_rows(const GemmParams &p, hipStream_t stream)
{
    if (p.m_indices || p.masked_m || p.row_index || (p.splitk <= 1 && p.groups != 1)) return DGA_E_TILING;
    return (p.k % 128) ? launch_bf16x_rows_one<Cfg, true>(p, stream) : launch_bf16x_rows_one<Cfg, false>(p, stream);
}

#define DGA_MENU_INSTANTIATE_BX_ROWS(BM, BN, WM, WN, ST, PP) \
    template int launch_bf16x_rows<GemmCfg<BM, BN, WM, WN, ST>>(const GemmParams &, hipStream_t);
DGA_MENU_BX(DGA_MENU_INSTANTIATE_BX_ROWS)
}
