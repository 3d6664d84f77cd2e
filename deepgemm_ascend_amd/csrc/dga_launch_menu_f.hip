// fp8 tile-kernel menu, part F: the image build of the bf16-exact policy (gemm_fp8_bf16x_image_kernel.hpp, dispatchPolicyTag 7):
// 128 x 256 tile, both operands converted once per workgroup into a bf16 LDS image; 8 waves (two per SIMD) or 4 (one per SIMD);
// and the A-image build (gemm_fp8_bf16x_aimage_kernel.hpp): only the A-matrix tile goes through the image, 8 waves.
#include "dga_fp8_menu_impl.hpp"
#include "gemm_fp8_bf16x_aimage_kernel.hpp"
namespace dga {

template <class Cfg, bool KTAIL, bool AIMAGE = false>
static int launch_bf16x_image_one(const GemmParams &p, hipStream_t stream)
{
    static_assert(Cfg::LDS_BYTES <= 160 * 1024, "LDS of one CU");
    const unsigned grid = p.launch_tiles > 0 ? static_cast<unsigned>(p.launch_tiles)
                                             : static_cast<unsigned>(p.groups) * p.tiles_m * p.tiles_n;
    if constexpr (AIMAGE) return launch_kernel<gemm_fp8_bf16x_aimage_kernel<KTAIL>>(grid, Cfg::NT, Cfg::LDS_BYTES, stream, p);
    else return launch_kernel<gemm_fp8_bf16x_image_kernel<Cfg, KTAIL>>(grid, Cfg::NT, Cfg::LDS_BYTES, stream, p);
}

int launch_bf16x_image(const GemmParams &p, int waves, hipStream_t stream)
{
    // dense and masked-grouped rasters (and their split-K form); the contiguous and indexed layouts keep the in-register builds
    if (p.tail_sub || p.m_indices || p.row_index || p.launch_tiles > 0) return DGA_E_TILING;
    if (waves == 1)   // the A-image build
        return (p.k % 128) ? launch_bf16x_image_one<BxAImageCfg, true, true>(p, stream) : launch_bf16x_image_one<BxAImageCfg, false, true>(p, stream);
    if (waves == 4)
        return (p.k % 128) ? launch_bf16x_image_one<BxImageCfg<4>, true>(p, stream) : launch_bf16x_image_one<BxImageCfg<4>, false>(p, stream);
    return (p.k % 128) ? launch_bf16x_image_one<BxImageCfg<8>, true>(p, stream) : launch_bf16x_image_one<BxImageCfg<8>, false>(p, stream);
}
}
