// fp8 tile-kernel menu, part H: the persistent form of the bf16-exact policy's 128 x 256 in-register build
// (gemm_fp8_bf16x_persistent_kernel.hpp, dispatchPolicyTag 7): one workgroup per CU walks the raster, the LDS ring runs across tiles.
#include "dga_fp8_menu_impl.hpp"
#include "gemm_fp8_bf16x_persistent_kernel.hpp"
namespace dga {

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
    if (out == Out::Bf16) return (p.launch_tiles > 0 && p.groups != 1) ? DGA_E_TILING : launch_bf16x_persistent_one<0, 0>(p, stream);
    if (p.masked_m || p.groups != 1) return DGA_E_TILING;
    return out == Out::F32 ? launch_bf16x_persistent_one<1, 0>(p, stream) : launch_bf16x_persistent_one<1, 1>(p, stream);
}
}
