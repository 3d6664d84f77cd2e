// What the fp8 tiling selectors (dga_tiling.cpp, dga_predictor.cpp) and the fp8 launcher (dga_launch.hip and its menu units) both
// decide, written once: which kernelSerial values exist, how many workgroups a raster has, when the last partial round runs in
// quarter tiles, and the splits and workspaces of the kernels that meet in the caller's workspace.  Host arithmetic only; nothing
// here launches.
#pragma once
#include <cstdint>

#include "dga_hip.h"

namespace dga {

// the kernelSerial values the library has builds for (the reference's type 3, PaddingStreamK, has none)
inline bool known_kernel_serial(unsigned serial)
{
    return serial == DGA_KERNEL_COMMON || serial == DGA_KERNEL_SMALL || serial == DGA_KERNEL_PADDING_COMMON || serial == DGA_KERNEL_STREAMK ||
           serial == DGA_KERNEL_STREAMK_TAIL || serial == DGA_KERNEL_SPLITK_WORKGROUP || serial == DGA_KERNEL_STREAMK_ONE_LAUNCH;
}

// workgroups of the plain raster: groups x tile rows x tile columns (a zero tile -- a malformed cache row -- divides by one)
inline uint64_t raster_tiles(uint64_t groups, uint32_t m, uint32_t n, uint32_t bm, uint32_t bn)
{
    return groups * ((m + bm - 1) / (bm ? bm : 1)) * ((n + bn - 1) / (bn ? bn : 1));
}

// LDS bytes of one stage of a tile (dga_device_common.hpp GemmCfg with 256 DMA threads; the 8-wave tile gives the same figure)
inline uint32_t fp8_stage_bytes(uint32_t bm, uint32_t bn) { return (bm > 32 ? bm : 32) * 128 + bn * 128 + ((bm + 8 + 255) / 256) * 1024; }

// "The last partial round runs in quarter tiles" (kernelSerial 5): a dense raster of more than one round whose remainder `tail` fills at
// most 1 / share_den of the CUs runs its whole rounds as they are and the tail as four quarter tiles per parent tile in a second launch.
// share_den: 4 where the fast selector names the pair for its 256 x 256 tile, 2 for the bf16-exact 128 x 256 tile and for what the
// launcher takes from a caller's tiling under either policy (two quarter tiles to a CU).  Empty (tail == 0): the rule does not apply.
struct PartialRound {
    uint64_t main_tiles = 0, tail = 0;
    explicit operator bool() const { return tail != 0; }
    uint64_t launch_tiles() const { return main_tiles + 4 * tail; }   // both launches: blockDim of the tiling
};
inline PartialRound partial_round(uint64_t tiles, uint32_t cus, uint32_t share_den)
{
    const uint64_t tail = cus ? tiles % cus : 0;
    if (tiles <= cus || tail == 0 || tail * share_den > cus) return {};
    return {tiles - tail, tail};
}

// ---- the one-launch decode split-K of the bf16-exact policy (gemm_fp8_bf16x_dsk_kernel.hpp, DGA_BUILD_BX_DECODE)
// (SLOT_FLOATS: one workgroup's partial tile; MAX_S: workgroups per tile at most)
struct DskTile { static constexpr int BM = 64, BN = 128, SLOT_FLOATS = BM * BN, MAX_S = 8; };
// the splits a launch of `tiles` 64 x 128 tiles over kb k blocks runs with, given the tiling's splitkFactor: every workgroup resident
// at once (`cus`), every k slice at least two blocks, at most DskTile::MAX_S workgroups per tile
inline int bx_dsk_splits(int64_t tiles, int kb, int want, int cus)
{
    if (tiles <= 0 || tiles > cus) return 0;
    int s = want > 0 ? want : 1;
    if (s > DskTile::MAX_S) s = DskTile::MAX_S;
    if (s > cus / tiles) s = static_cast<int>(cus / tiles);
    if (s > kb / 4) s = kb / 4;
    return s;      // 0: the problem is too short along K (fewer than four k blocks)
}
// one fp32 partial tile per tile and split but the first + the flags
inline size_t bx_dsk_workspace_bytes(int64_t tiles, int splits)
{
    if (splits <= 1) return 0;
    return static_cast<size_t>(tiles) * (splits - 1) * (DskTile::SLOT_FLOATS * 4 + 8) + 256;
}

// ---- the one-launch Stream-K kernels: one fp32 partial tile per workgroup (one per CU) + the flags.  256 x 256 floats on the fast
//      path (gemm_fp8_streamk_kernel.hpp), 128 x 256 under the bf16-exact policy (gemm_fp8_bf16x_streamk_kernel.hpp)
inline size_t streamk_workspace_bytes(uint32_t cus) { return static_cast<size_t>(cus) * (256 * 256 * 4 + 8) + 256; }
inline size_t bx_streamk_workspace_bytes(uint32_t cus) { return static_cast<size_t>(cus) * (128 * 256 * 4 + 8) + 256; }

}  // namespace dga
