// fp8 tile-kernel menu, part Q: the paired body of the bf16-exact policy's dense persistent kernel
// (gemm_fp8_bf16x_pair_kernel.hpp): one workgroup per CU walks the raster two stacked 128 x 256 tiles at a time.  A unit of its own:
// the body unrolls a whole k block (128 MFMA gaps) and takes the unroll budget that goes with it (Makefile), which the builds of
// part H must not see.  The rule that picks this body over the one-tile-at-a-time one is part H's (launch_bf16x_persistent).
#include "dga_fp8_menu_impl.hpp"
#include "gemm_fp8_bf16x_pair_kernel.hpp"
namespace dga {

// grid 0: one workgroup per CU, at most one per pair
int launch_bf16x_pair(const GemmParams &p, unsigned grid, hipStream_t stream)
{
    if (p.groups != 1 || p.masked_m || p.m_indices || p.row_index || p.splitk > 1 || p.launch_tiles > 0 || p.tail_sub || p.kb_n < 2 ||
        (p.k % 128))
        return DGA_E_TILING;
    const int64_t pairs = static_cast<int64_t>((p.tiles_m + 1) / 2) * p.tiles_n;
    if (grid == 0) grid = static_cast<unsigned>(std::min<int64_t>(pairs, device_cus()));
    return launch_kernel<gemm_fp8_bf16x_pair_kernel>(grid, PairCfg::NT, PairCfg::LDS_BYTES, stream, p);
}
}
