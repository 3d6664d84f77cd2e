// fp8 tile-kernel menu, part E: the bf16-exact builds (dga_fp8_menu.hpp; gemm_fp8_kernel.hpp MATH = 1, dispatchPolicyTag 7), bf16 and
// fp32 rows (OUT = 1).
#include "dga_fp8_menu_impl.hpp"
namespace dga {

template <class Cfg, bool KTAIL, int OUT>
static int launch_bf16x_one(const GemmParams &p, hipStream_t stream)
{
    const unsigned grid = p.launch_tiles > 0 ? static_cast<unsigned>(p.launch_tiles)
                                             : static_cast<unsigned>(p.groups) * p.tiles_m * p.tiles_n;
    return launch_kernel<gemm_fp8_blockscaled_nt_kernel<Cfg, 0, KTAIL, false, 1, false, OUT>>(grid, Cfg::NT, Cfg::LDS_BYTES, stream, p);
}

template <class Cfg>
int launch_bf16x(const GemmParams &p, hipStream_t stream)
{
    // tiles no taller than the contiguous layout's segment alignment (no second pass)
    if (p.m_indices && Cfg::kBM > DGA_CONTIGUOUS_M_ALIGNMENT) return DGA_E_TILING;
    return (p.k % 128) ? launch_bf16x_one<Cfg, true, 0>(p, stream) : launch_bf16x_one<Cfg, false, 0>(p, stream);
}

// fp32 rows (+ C): dense rasters only (the fp32 entry has no grouped form)
template <class Cfg>
int launch_bf16x_f32(const GemmParams &p, hipStream_t stream)
{
    if (p.m_indices || p.masked_m || p.row_index || p.groups != 1 || p.splitk > 1) return DGA_E_TILING;
    return (p.k % 128) ? launch_bf16x_one<Cfg, true, 1>(p, stream) : launch_bf16x_one<Cfg, false, 1>(p, stream);
}

#define DGA_MENU_INSTANTIATE_BX(BM, BN, WM, WN, ST, PP) \
    template int launch_bf16x<GemmCfg<BM, BN, WM, WN, ST>>(const GemmParams &, hipStream_t);
DGA_MENU_BX(DGA_MENU_INSTANTIATE_BX)
#define DGA_MENU_INSTANTIATE_BX_F32(BM, BN, WM, WN, ST, PP) \
    template int launch_bf16x_f32<GemmCfg<BM, BN, WM, WN, ST>>(const GemmParams &, hipStream_t);
DGA_MENU_BX(DGA_MENU_INSTANTIATE_BX_F32)
}
