// Definitions behind dga_fp8_menu.hpp; included by the units that launch kernels (the dga_launch_menu_*.hip units instantiate their share).
#pragma once
#include <hip/hip_runtime.h>
#include <mutex>

#include "dga_fp8_menu.hpp"
#include "gemm_fp8_strict_kernel.hpp"

namespace dga {

// Launch Kernel<<<grid, threads, lds, stream>>>(args...): the dynamic-LDS attribute set once per device and kernel (where lds > 0),
// nothing launched for an empty grid.
template <auto Kernel, class... Args>
int launch_kernel(unsigned grid, unsigned threads, int lds, hipStream_t stream, const Args &...args)
{
    static std::once_flag once[64];
    static hipError_t attr_err[64];
    int dev = 0;
    if (int rc = record_hip(hipGetDevice(&dev))) return rc;
    if (dev < 0 || dev >= 64) return DGA_E_HIP;
    if (lds > 0) {
        std::call_once(once[dev], [&] {
            attr_err[dev] = hipFuncSetAttribute(reinterpret_cast<const void *>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        });
        if (int rc = record_hip(attr_err[dev])) return rc;
    }
    if (grid == 0) return DGA_OK;
    hipLaunchKernelGGL(Kernel, dim3(grid), dim3(threads), lds, stream, args...);
    return record_hip(hipGetLastError());
}

// the strict kernel's build for a tile height of bm rows (32, 64, 128) and an output form; nullptr: none.  KGROUP: the k-grouped
// form (dga_launch_menu_p.hip), which exists for 32 and 64 rows with per-row sfb only
typedef void (*StrictKernel)(const GemmParams);
template <int TM, int KGROUP>
static StrictKernel strict_kernel_tm(Out out)
{
    if constexpr (KGROUP) return out == Out::F32Rows ? gemm_fp8_strict_nt_kernel<TM, 1, 1, 1> : nullptr;
    else return out == Out::F32Rows ? gemm_fp8_strict_nt_kernel<TM, 1, 1> : out == Out::F32 ? gemm_fp8_strict_nt_kernel<TM, 1> : gemm_fp8_strict_nt_kernel<TM>;
}
template <int KGROUP = 0>
static StrictKernel strict_kernel(int bm, Out out)
{
    if (bm == 32) return strict_kernel_tm<1, KGROUP>(out);
    if (bm == 64) return strict_kernel_tm<2, KGROUP>(out);
    if constexpr (!KGROUP)
        if (bm == 128) return strict_kernel_tm<4, 0>(out);
    return nullptr;
}

template <class Cfg, int PP, bool KTAIL, bool CLK>
static int launch_one(const GemmParams &p, hipStream_t stream)
{
    unsigned grid = p.launch_tiles > 0 ? static_cast<unsigned>(p.launch_tiles)
                                       : static_cast<unsigned>(p.groups) * p.tiles_m * p.tiles_n;
    if (p.m_indices && Cfg::kBM > DGA_CONTIGUOUS_M_ALIGNMENT) grid *= 2;  // pass-1 copies for straddling tiles
    return launch_kernel<gemm_fp8_blockscaled_nt_kernel<Cfg, PP, KTAIL, CLK>>(grid, Cfg::NT, Cfg::LDS_BYTES, stream, p);
}

template <class Cfg, int PP, bool CLK>
int launch_cfg(const GemmParams &p, hipStream_t stream)
{
    if constexpr (CLK) {
        if (p.k % 128) return DGA_E_TILING;
        return launch_one<Cfg, PP, false, true>(p, stream);
    } else {
        return (p.k % 128) ? launch_one<Cfg, PP, true, false>(p, stream) : launch_one<Cfg, PP, false, false>(p, stream);
    }
}

#define DGA_MENU_INSTANTIATE(BM, BN, WM, WN, ST, PP) \
    template int launch_cfg<GemmCfg<BM, BN, WM, WN, ST>, PP, false>(const GemmParams &, hipStream_t);
#define DGA_MENU_INSTANTIATE_LC(BM, BN, WM, WN, ST, PP) \
    template int launch_cfg<GemmCfg<BM, BN, WM, WN, ST, 4>, PP, false>(const GemmParams &, hipStream_t);
#define DGA_MENU_INSTANTIATE_CLK_LC(BM, BN, WM, WN, ST, PP) \
    template int launch_cfg<GemmCfg<BM, BN, WM, WN, ST, 4>, PP, true>(const GemmParams &, hipStream_t);
#define DGA_MENU_INSTANTIATE_CLK(BM, BN, WM, WN, ST, PP) \
    template int launch_cfg<GemmCfg<BM, BN, WM, WN, ST>, PP, true>(const GemmParams &, hipStream_t);

}  // namespace dga
