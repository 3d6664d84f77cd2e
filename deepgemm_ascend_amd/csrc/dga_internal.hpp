// Internal (non-ABI) declarations shared by the host translation units.
#pragma once
#include <hip/hip_runtime_api.h>

#include "dga_hip.h"
#include <cstdint>
#include <cstdlib>

namespace dga {
int record_hip(hipError_t e);
// CUs of the current device (cached); the MI355X constant 256 when no device is visible (host-only tiling calls)
uint32_t device_cus();
// $DGA_DEFAULT_POLICY, read once: the arithmetic of a GEMM call that names no tiling.  1 = bf16-exact (the default: inside the
// operator's 2-ULP contract), 0 = "fast" (fp8 matrix instruction), 2 = "strict".
int default_policy();
// indexed masked-grouped form: flat row buffers + slot -> row table (dga_m_grouped_gemm_fp8_fp8_bf16_nt_masked_indexed)
struct Fp8Indexed {
    const int64_t *row_index;   // device int64[groups * m_max]
    int64_t lda;                // bytes between rows of the flat A source
    int64_t sfa_ld;             // floats between rows of the scale source
    int64_t ldc;                // bf16 elements between rows of the flat destination
    int64_t rows;               // rows of the flat A source (bounds the buffer descriptor)
};
// row-strided dense form (dga_gemm_fp8_fp8_bf16_nt_strided): bytes between the rows of A and of B, DGA_ROWS_* flags
struct Fp8Strided {
    int64_t lda, ldb;
    int flags;
};
// the output form of an fp8 GEMM: bf16 rows, fp32 rows (+ C; dga_gemm_fp8_fp8_fp32_nt), or fp32 rows with per-row sfb (sfb is [N, KB],
// one scale per row of B; dga_wgrad_gemm_fp8_fp8_fp32_nt).  One-to-one with the kernels' (OUT, SFB_ROWS) template pairs (0, 0), (1, 0), (1, 1)
enum class Out { Bf16, F32, F32Rows };
// one call of the fp8 launcher (run_fp8): the operands first, then what only some entry points set
struct Fp8Call {
    const void *a;
    const float *sfa;
    const void *b;
    const float *sfb;
    void *out;
    int m, n, k;
    const dga_tiling_t *tiling;     // nullptr: the entry's own selector picks one
    void *workspace;
    size_t workspace_bytes;
    hipStream_t stream;
    int groups = 1, b_groups = 1, expected_m = 0;
    const int32_t *masked_m = nullptr;     // masked grouped layout
    // contiguous-grouped layout: one A/out matrix of m rows (groups == 1 on that side), b_groups B matrices picked per row block
    const int32_t *m_indices = nullptr;
    const Fp8Indexed *ix = nullptr;        // indexed masked-grouped form: a / sfa / out are flat row buffers addressed through ix->row_index
    const Fp8Strided *sd = nullptr;        // dense operands with their own row strides
    Out kind = Out::Bf16;                  // the fp32 forms are dense only
    const float *c_in = nullptr;           // fp32 forms: the optional fp32 addend (may be out)
    unsigned long long *clock_stamps = nullptr;   // dga_gemm_fp8_loop_clock only: the loop-clock build, two words per wave
};
// the fp8 launcher behind the C-ABI GEMM entry points (dga_launch.hip); clock_stamps: see dga_diag.hip
int run_fp8(const Fp8Call &c);
// $NAME as an integer, `dflt` when unset
inline int env_int(const char *name, int dflt)
{
    const char *e = std::getenv(name);
    return e ? std::atoi(e) : dflt;
}
// compiled fp8 kernel menu (dga_launch.hip)
int variant_count();
void variant_info(int i, int *bm, int *bn, int *wm, int *wn, int *lds);
int variant_stages(int i);
bool variant_has_loader_waves(int i);   // a dispatchPolicyTag-4 build of that menu entry exists
// a 3-stage tiling on the plain loop whose tile has a loader-wave build takes it (same bits, 9-17 % less time)
void prefer_loader_waves(dga_tiling_t &t, bool upgrade_plain = true);
// odd-K re-layout pass (dga_rows.hip): rows of src_row_bytes at any byte alignment -> 16-byte aligned rows of dst_row_bytes, zero tail;
// two operands in one launch (rows1 == 0: one)
int pad_rows(const void *src0, void *dst0, int64_t rows0, const void *src1, void *dst1, int64_t rows1, int64_t src_row_bytes,
             int64_t dst_row_bytes, hipStream_t stream);
// the same with the sources' own row strides (bytes between rows, >= src_row_bytes)
int pad_rows_strided(const void *src0, int64_t stride0, void *dst0, int64_t rows0, const void *src1, int64_t stride1, void *dst1,
                     int64_t rows1, int64_t src_row_bytes, int64_t dst_row_bytes, hipStream_t stream);
// dense 256x256 tilings: turn a small last partial wave into a K-split tail (dga_tiling.cpp)
void apply_tail_split(dga_tiling_t &t, uint32_t cus);
// the wave grid and LDS bytes of a tiling that names a tile, a stage count and a schedule only (a cache row, the predictor's pick)
namespace tiling {
void complete_from_menu(dga_tiling_t &t);
// the compiled menu's first build of a tile (stages 0: of any stage count; loaders: one with loader waves); nullptr: none
struct MenuEntry;
const MenuEntry *find_build(int bm, int bn, int stages = 0, bool loaders = false);
}

// What the sparse MLA attention entries (dga_sparse_mla.hip: the four forward forms; dga_sparse_mla_bwd.hip: the backward) hand to the one
// check below and to their launches: the call without its row source and outputs, the row source, and the outputs of either kind.  A new
// row source is one more maker of SmlaSource with its clauses in the four questions the check asks.
struct SmlaCall {
    const void *q;
    const int32_t *indices, *index_offsets;
    int64_t m;
    int heads;
    int64_t topk, idx_stride;
    double sm_scale;
    int flags;
    void *stream;
};

// count units of page_size rows each, `stride` apart: bf16 rows (s of them, one a unit, kv_stride elements apart) or the blocks of the
// paged fp8 cache (block_stride bytes apart).  The range clauses divide by what the shape clause has vouched for.
struct SmlaSource {
    bool fp8;
    const void *rows;
    int64_t count, page_size, stride;
    // (stride / 656 < page_size says block_stride < 656 page_size without the product)
    bool shape() const
    {
        return count >= 1 && page_size >= 1 && (fp8 ? stride / DGA_SPARSE_MLA_FP8_ROW_BYTES >= page_size : stride >= DGA_SPARSE_MLA_D_QK);
    }
    bool aligned() const { return reinterpret_cast<uintptr_t>(rows) % 16 == 0 && stride % (fp8 ? 16 : 8) == 0; }
    bool rows_in_range() const { return count <= 0x7FFFFFFFll / page_size; }
    bool bytes_in_range() const { return stride <= 0x7FFFFFFFFFFFFFFFll / (fp8 ? 1 : 2) / count; }
};

// The checks of every entry, in the documented order: flags, shape, m == 0, null, alignment, range; *launch is set when a launch is
// to follow (not for m == 0).  out and lse are the one-pass forward entries' (null and unchecked for the partial ones and the backward,
// which check their own outputs afterwards).
inline int check_sparse_mla(const SmlaCall &c, const SmlaSource &src, bool outputs, const void *out, const void *lse, bool *launch)
{
    *launch = false;
    if (c.flags & ~DGA_SPARSE_MLA_LINEAR_GRID) return DGA_E_RANGE;
    if (c.m < 0 || c.heads < 16 || c.heads > DGA_SPARSE_MLA_MAX_HEADS || c.heads % 16 || !src.shape() || c.topk < 1 || c.idx_stride < c.topk)
        return DGA_E_SHAPE;
    if (c.m == 0) return DGA_OK;
    if (!c.q || !src.rows || !c.indices || (outputs && (!out || !lse))) return DGA_E_NULL;
    if (reinterpret_cast<uintptr_t>(c.q) % 16 || !src.aligned() || reinterpret_cast<uintptr_t>(out) % 16 ||
        reinterpret_cast<uintptr_t>(c.indices) % 4 || reinterpret_cast<uintptr_t>(c.index_offsets) % 4 || reinterpret_cast<uintptr_t>(lse) % 4)
        return DGA_E_ALIGN;
    const int head_blocks = (c.heads + 63) / 64;
    if (!src.rows_in_range() || c.topk > 0x7FFFFFFFll - DGA_SPARSE_MLA_TILE || c.m > (0x7FFFFFFFll - 8) / head_blocks) return DGA_E_RANGE;
    if (!src.bytes_in_range() || c.idx_stride > 0x7FFFFFFFFFFFFFFFll / 4 / c.m) return DGA_E_RANGE;
    *launch = true;
    return DGA_OK;
}

// What the two backward entries (dga_sparse_mla_bwd.hip; dga_sparse_mla_bwd_det.hip) take beside SmlaCall, the checks they share in the
// documented order, and the launch of the backward kernel: with phase C and its atomic adds onto dkv, or dq alone (dkv is not looked at).
// Both are defined in dga_sparse_mla_bwd.hip.
struct SmlaBwdCall {
    SmlaCall c;
    const void *kv;
    int64_t s, kv_stride;
    const void *out, *d_out;
    const float *lse;
    void *dq;
    float *dkv;
    int64_t dkv_stride;
};
int check_sparse_mla_bwd(const SmlaBwdCall &b, bool *launch);
int launch_sparse_mla_bwd(const SmlaBwdCall &b, bool with_dkv);
}  // namespace dga
