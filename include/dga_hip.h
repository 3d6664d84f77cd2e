/*
 * dga_hip.h -- C ABI of libdga_hip.so: the MI355X (gfx950) drop-in for the
 * DeepGEMM_Ascend hot path.  Plain pointers and sizes only; every entry point
 * returns an int status (0 = DGA_OK, negative = error) and never throws.
 * Device pointers are caller-owned; nothing here allocates device memory.
 * `stream` is a hipStream_t passed as void* (NULL = the default stream).
 *
 * Each declaration cites the reference interface it replaces
 * (paths relative to /root/reference).
 */
#ifndef DGA_HIP_H
#define DGA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DGA_ABI_VERSION 7

/* ---- status codes (reference: DGA_HOST_ASSERT throws DGAException,
 *      deep_gemm_ascend/framework/csrc/utils/exception.hpp:9-33; op hooks return
 *      ge::GRAPH_FAILED, aclnn_catlass_dynamic_matmul/op_host/catlass_dynamic_matmul_tiling.cpp:86-100) */
enum {
    DGA_OK = 0,
    DGA_E_NULL = -1,      /* required pointer is NULL */
    DGA_E_SHAPE = -2,     /* rank / dimension mismatch (InferShape / TilingFunc checks) */
    DGA_E_DTYPE = -3,     /* dtype mismatch (InferDataType) */
    DGA_E_ALIGN = -4,     /* pointer / stride alignment the kernel cannot take */
    DGA_E_HIP = -5,       /* a HIP runtime call failed (see dga_last_hip_error) */
    DGA_E_TILING = -6,    /* tiling not supported by any compiled kernel variant */
    DGA_E_WORKSPACE = -7, /* workspace too small */
    DGA_E_IO = -8,        /* harness / cache file error */
    DGA_E_RANGE = -9      /* masked_m / knob out of range */
};

/* dtypes (the values the aclnn op proto uses are ge::DataType; we keep our own small enum) */
enum { DGA_DT_FP16 = 1, DGA_DT_BF16 = 2, DGA_DT_FP8_E4M3FN = 3, DGA_DT_FP32 = 4 };

/* LayoutTag / PaddingTag: aclnn_catlass_dynamic_matmul/op_host/op_tiling/tiling_params.h:16-17 */
enum { DGA_LAYOUT_ROW_MAJOR = 0, DGA_LAYOUT_COLUMN_MAJOR = 1 };
enum { DGA_PADDING_NONE = 0, DGA_PADDING_ND = 1, DGA_PADDING_BLOCK_ND = 2, DGA_PADDING_NZ = 3 };

/* kernelSerial menu, same numbering as the reference
 * (op_kernel/kernel/kernel_utils.h:31-37, select_kernel.cpp:270-331):
 *   0 Common, 1 Small, 2 PaddingCommon (K % 16 != 0 read in place by the loader waves of the 128 x 256 tile: the re-layout fused
 *   with the matmul as in the reference's kernel of that name; without it odd K takes a padding pass), 4 StreamK/split-K. */
enum { DGA_KERNEL_COMMON = 0, DGA_KERNEL_SMALL = 1, DGA_KERNEL_PADDING_COMMON = 2, DGA_KERNEL_STREAMK = 4,
       DGA_KERNEL_STREAMK_TAIL = 5 /* whole waves of 256x256 tiles, the last partial wave covered by 128x128 tiles in a second launch;
                                      under DGA_POLICY_BF16_EXACT: whole waves of 128x256 tiles + 64x128 quarter tiles.  Same bytes as
                                      the single launch; a tail longer than half the CUs runs as the single launch */,
       DGA_KERNEL_SPLITK_WORKGROUP = 6 /* M <= 64: the 8 waves of a workgroup are the 8 K slices of one output tile, partial tiles
                                          combined in LDS -- one launch, no slab (the reference's single-core split-K kernel types,
                                          op_kernel/catlass_dynamic_matmul_tiling_key.h:30-36); the bits of split-K with factor 8.
                                          M <= 32: operands staged through per-wave LDS-DMA rings (tiling.stages = 1 names the
                                          older build that streams fragments global -> registers instead) */,
       DGA_KERNEL_STREAMK_ONE_LAUNCH = 7 /* Stream-K proper (the reference's kernel type 4, padding_streamk_matmul_kernel.h:94-98): ONE
                                          launch of one workgroup per CU; the raster's (tile, k block) units are cut evenly over the
                                          workgroups, a run that ends inside a tile leaves an fp32 partial tile in the workspace and the
                                          workgroup holding the tile's first k blocks adds the partials in k order.  256 x 256 tile, dense,
                                          M and N multiples of 256, K of 128; anything else runs the tiling's tile kernel.  Needs
                                          dga_workspace_bytes() of workspace (256 KB per CU) */ };

/* dispatchPolicyTag of the fp8 tile kernels (the reference's field selects a catlass dispatch policy,
 * op_tiling/tiling_params.h:19-66; here it selects the main-loop schedule or the exact-arithmetic kernel):
 *   0 plain (one barrier per k block), 1 ping-pong, 2 continuous pipeline -- the same results, bit for bit;
 *   3 strict: fp32-input MFMA chain in the reference CPU path's own order (fp32 products, fp32 running sum, k ascending:
 *     framework/tests/test.py:37) -- bit-identical to the oracle, any shape, at the fp32 matrix rate (1/32 of the fp8
 *     rate).  $DGA_STRICT=1 forces it for every fp8 call of the process.
 *   4 loader waves: the plain loop with four extra waves that only issue the LDS-DMA (128x256 tile, 3 stages): the masked
 *     grouped weight stream (-2 % time) and dense problems of about one such tile per CU (BASELINE configs[2]: -9 %);
 *     same bits as policy 0; a tile without such a build runs policy 0.
 *   5 persistent loader waves: policy 4 with one workgroup per CU that walks its share of the tiles, the LDS ring running
 *     across tile boundaries (the next tile's first k blocks are in flight while this one is stored) -- what the
 *     reference's one-block-per-AI-core kernel is by construction (framework/csrc/jit/generate_code.hpp:160-198); same
 *     bits as policy 0; whole rasters only (split-K and the quarter-tile tail run policy 4).
 *   6 persistent continuous pipeline: policy 2 (256x256 tile) with one workgroup per CU walking its tiles, the refill slots
 *     of a tile's last two k blocks fetching the next tile's first two; dense rasters of full tiles (M, N multiples of 256,
 *     K of 128, at least two k blocks) -- anything else runs policy 2; same bits.
 *   7 bf16-exact: the e4m3 bytes are up-converted to bf16 in registers (exact) and every 128-wide scale block is summed by four
 *     chained v_mfma_f32_16x16x32_bf16 -- exact products, fp32-class sums (2^-25 of the block's sum of magnitudes, against
 *     2^-16 on the fp8 matrix instruction), the same fp32 promotion.  The policy between the fast path (policies 0-2, 4-6) and
 *     the strict one: within 2 bf16 ULP of the reference CPU path (framework/tests/test.py:19-64) on all but ~1e-6 of the
 *     outputs of BASELINE configs[1] (every one a sum that cancels to < 2^-21 of its terms), at the bf16 matrix rate.  Takes
 *     every layout the tile kernels take (dense, masked, contiguous, indexed, split-K); the tile comes from the tiling's
 *     (m1, n1) mapped onto the policy's own menu (wave tiles of at most 64 x 64).  $DGA_BF16_EXACT=1 forces it for every fp8
 *     call of the process.
 *   | 16 (DGA_POLICY_UE8M0_SCALES, a FLAG on the fast-path schedules 0, 2, 4, 5, 6): the caller's promise that every value of sfa
 *     and sfb is an exact power of two in the normal fp32 range ("UE8M0" scales: 2^ceil(log2(amax / 448)), what upstream DeepGEMM's
 *     per_token_cast_to_fp8(..., use_ue8m0=True) writes).  The scales then ride in the E8M0 operands of
 *     v_mfma_scale_f32_16x16x128_f8f6f4 and the MFMA accumulates in place, as the reference's Mmad(c1Local, ..., init on first)
 *     does (framework/csrc/jit/generate_code.hpp:320-335): no promotion on the vector pipe.  Outputs equal the promotion form's up
 *     to fp32 rounding order (profiles/r05_probe_scale_acc.txt: identical bf16 on 76 800 of 76 800 outputs); a tile without such a
 *     build runs the promotion form.  A scale that is NOT a power of two is read as its exponent alone (mantissa dropped); zero
 *     reads as 2^-127.  Ignored by policy 3.
 *     On policy 7 (7 | 16): the bf16-exact arithmetic with the scales folded into the e4m3 -> bf16 conversions of the A fragments (a
 *     power of two times an e4m3 value is a bf16 value: exact) -- the bf16 MFMA chain then accumulates through every k block in
 *     place, no promotion; 128 x 256 and 64 x 256 tiles, every layout; other tiles run policy 7 as it is. */
enum { DGA_POLICY_PLAIN = 0, DGA_POLICY_PINGPONG = 1, DGA_POLICY_CONTINUOUS = 2, DGA_POLICY_STRICT = 3,
       DGA_POLICY_LOADER_WAVES = 4, DGA_POLICY_PERSISTENT = 5, DGA_POLICY_CONTINUOUS_PERSISTENT = 6,
       DGA_POLICY_BF16_EXACT = 7, DGA_POLICY_UE8M0_SCALES = 16 };

/* dga_tiling_t.build: the compiled build a caller (a sweep, a test, a tuned CSV row) names beside the tile and the schedule.  0 lets
 * the dispatcher choose (what every selector of this library writes unless it says otherwise below).  No reference counterpart: the
 * reference compiles one kernel per tiling key (op_kernel/catlass_dynamic_matmul_tiling_key.h:30-36).
 *   fast path     DGA_BUILD_WSK_REGISTER with kernelSerial 6 only: fragments global -> registers (M <= 64) instead of the LDS-DMA rings
 *   bf16-exact    DGA_BUILD_BX_AIMAGE / _IMAGE8 / _IMAGE4: the 128 x 256 tile with A (8 waves) or both operands (8 / 4 waves) converted
 *                 once per workgroup into a bf16 LDS image;  DGA_BUILD_BX_PERSISTENT / _ONE_TILE: one workgroup per CU walking the raster /
 *                 one workgroup per tile (0: persistent on rasters of more than one round);  DGA_BUILD_BX_GROUPED: the masked grouped
 *                 layout's kernel (two k blocks of the ring in flight, the loop unrolled for the m-tiles that hold rows) -- what
 *                 dga_tiling_bf16_exact names for masked grouped problems;  DGA_BUILD_BX_DECODE with kernelSerial 6 and the 64 x 128 tile
 *                 only: the one-launch split-K for a few 64-row tiles (two k groups per workgroup, splitkFactor <= 8 workgroups per tile
 *                 whose fp32 partial tiles meet in the workspace -- dga_workspace_bytes counts them; a launch it does not take, e.g. no
 *                 workspace or more tiles than CUs, runs the two-launch split-K of the same tiling);  DGA_BUILD_WSK_REGISTER as above.
 * The values are the magic `stages` values of ABI <= 6, so a CSV row written then (stages 1, 4..8) maps onto (build = stages,
 * stages = 3) when it is read. */
enum { DGA_BUILD_DEFAULT = 0, DGA_BUILD_WSK_REGISTER = 1, DGA_BUILD_BX_AIMAGE = 4, DGA_BUILD_BX_IMAGE8 = 5, DGA_BUILD_BX_IMAGE4 = 6,
       DGA_BUILD_BX_PERSISTENT = 7, DGA_BUILD_BX_ONE_TILE = 8, DGA_BUILD_BX_GROUPED = 9, DGA_BUILD_BX_DECODE = 10 };

/* Platform description: the CDNA4 retarget of PlatformInfo
 * (op_tiling/platform_info.h:16-41; Python mirror get_best_config/tiling_calculator.py:25-30).
 * The same struct carries the Ascend numbers when the reference's own arithmetic is
 * replayed for parity (tests only). */
typedef struct dga_platform_t {
    uint32_t coreNum;   /* Ascend: AI cores (24/20).  MI355X: CUs (256) */
    uint64_t ubSize;    /* Ascend UB 192 KiB.       MI355X: unused (0) */
    uint64_t l1Size;    /* Ascend L1 512 KiB.       MI355X: LDS per CU (160 KiB) */
    uint64_t l0ASize;   /* Ascend 64 KiB.           MI355X: VGPR bytes per SIMD lane-set usable for A fragments */
    uint64_t l0BSize;
    uint64_t l0CSize;   /* Ascend L0C 128 KiB.      MI355X: fp32 accumulator bytes per workgroup (8 waves x 128 regs x 64 lanes x 4) */
    uint32_t xcdNum;    /* MI355X: 8 (Ascend: 1) */
    uint32_t waveSize;  /* MI355X: 64 */
} dga_platform_t;

/* Host-side superset of the kernel tiling data: TilingParams
 * (op_tiling/tiling_params.h:19-66) + CatlassDynamicMatmulTilingData
 * (op_kernel/catlass_dynamic_matmul_tiling_data.h:19-33) + CDNA4 fields. */
typedef struct dga_tiling_t {
    uint64_t strideA, strideB, strideC;
    uint32_t m, n, k;
    uint16_t m1, n1, k1;         /* workgroup tile BM x BN x BK */
    uint8_t swizzleOffset;       /* tile-rows rastered together (tiling_params.h:63) */
    uint8_t swizzleDirection;    /* (m > n) ? 0 : 1 (tiling_params.h:64) */
    uint16_t splitkFactor;
    uint8_t layoutTagA, layoutTagB, layoutTagC;
    uint8_t paddingTagA, paddingTagB, paddingTagC;
    uint8_t kernelSerial;
    uint8_t dispatchPolicyTag;
    uint8_t build;               /* DGA_BUILD_*: which compiled build of (kernelSerial, dispatchPolicyTag, tile) runs; 0 = the
                                    dispatcher's rule.  ABI 7: until ABI 6 these names rode on magic values of `stages` */
    uint8_t reserved0;           /* 0 */
    uint32_t blockDim;           /* workgroups launched (reference: uint8 AI-core count) */
    /* CDNA4 */
    uint8_t wavesM, wavesN;      /* wave grid inside the workgroup */
    uint8_t stages;              /* LDS stages, as in the reference's tiling data (op_kernel/catlass_dynamic_matmul_tiling_data.h:19-33
                                    has none: the catlass dispatch policy fixes them): 0 = the tile's default, 2 or 3 */
    uint8_t contiguous;          /* 1 = contiguous-grouped layout (groups = number of B matrices) */
    uint32_t ldsBytes;
    uint32_t groups;             /* 1 = dense */
} dga_tiling_t;

typedef struct dga_problem_t {
    uint32_t m, n, k;
    uint32_t groups;             /* 1 = dense; >1 = grouped masked-M with m = m_max */
    uint32_t expected_m;         /* grouped: hint for tile choice (0 = m) */
    uint8_t layoutTagA, layoutTagB, layoutTagC;
    uint8_t dtype;               /* DGA_DT_* of the inputs */
    uint32_t flags;              /* DGA_PROBLEM_* */
} dga_problem_t;

#define DGA_PROBLEM_CONTIGUOUS_M 1u   /* contiguous-grouped layout: tile height <= DGA_CONTIGUOUS_M_ALIGNMENT */
#define DGA_CONTIGUOUS_M_ALIGNMENT 128

/* ---- operator hooks -------------------------------------------------------------------- */

/* InferShape: aclnn_catlass_dynamic_matmul/op_host/catlass_dynamic_matmul.cpp:16-35.
 * self [m,k], mat2 logical [k,n] -> out [m,n]; both ranks must be 2. */
int dga_infer_shape(const int64_t *self_shape, int self_rank, const int64_t *mat2_shape, int mat2_rank,
                    int64_t *out_shape /*[2]*/);

/* InferDataType: catlass_dynamic_matmul.cpp:37-46 (inputs must match; out = in).
 * fp8 inputs are the extension: out = bf16. */
int dga_infer_dtype(int self_dtype, int mat2_dtype, int *out_dtype);

/* TilingFunc: catlass_dynamic_matmul_tiling.cpp:77-122 = shape checks + TilingParams ctor +
 * SelectKernelWithCache (select_kernel.cpp:371-378).  Consults the (m,n,k)-keyed tiling cache,
 * optionally CSV-backed through $CACHE_FILE_PATH / $DGA_CACHE_FILE_PATH (cache.cpp:22-101).  A cached row's
 * DGA_POLICY_UE8M0_SCALES flag is dropped: the flag is the caller's promise about its scales, not a row's. */
int dga_tiling(const dga_problem_t *problem, dga_tiling_t *out);

/* TilingFunc of the bf16-exact arithmetic policy (dispatchPolicyTag 7): dga_tiling, then -- for dense problems -- the tile and
 * split-K factor picked from that policy's own menu by its own cost model (wave tiles <= 64 x 64, one 8-wave build; the fast path's
 * tuned tile is 10-40 % off there on mid-M shapes).  A tiling-cache row of this policy's class (dispatchPolicyTag 7, with or without
 * DGA_POLICY_UE8M0_SCALES) is taken first if dga_tiling_check accepts it, and passed over for the rules otherwise; no build name of a
 * fast-class row survives.  Whatever any cache row says, the result for M, N > 0 passes dga_tiling_check and carries
 * dispatchPolicyTag = DGA_POLICY_BF16_EXACT exactly: never DGA_POLICY_UE8M0_SCALES, which only the caller's policy (or process
 * default) adds.  No reference counterpart. */
int dga_tiling_bf16_exact(const dga_problem_t *problem, dga_tiling_t *out);

/* Does the compiled kernel menu hold this tiling?  DGA_OK, or the error every fp8 GEMM entry returns for it BEFORE any launch
 * (they call the same check first): DGA_E_TILING for a (kernelSerial, dispatchPolicyTag, m1 x n1, wavesM x wavesN, stages) no build
 * answers to, DGA_E_RANGE for a split factor beyond 1024.  A caller-written dga_tiling_t is data from outside; the counterpart of
 * CatlassDynamicMatmulTilingFunc returning GRAPH_FAILED (op_host/catlass_dynamic_matmul_tiling.cpp:86-100).  What the fields may
 * hold:  kernelSerial 0, 1, 2, 4, 5, 6, 7;  k1 0 or 128;  dispatchPolicyTag 0..7, optionally | DGA_POLICY_UE8M0_SCALES;  stages 0, 2 or 3;
 * reserved0 0;
 *   policy 3 (strict): any tile, stages and build (the kernel picks its own);
 *   policy 7 (bf16-exact): any m1, n1 > 0 (mapped onto that policy's menu); build 0 or a DGA_BUILD_BX_* name (DGA_BUILD_WSK_REGISTER only
 *     with kernelSerial 6; DGA_BUILD_BX_DECODE only with kernelSerial 6 on m1 x n1 = 64 x 128);
 *   fast path: m1 x n1 a tile of the menu, wavesM x wavesN either 0 x 0 or a wave grid that tile is built with; build 0
 *     (DGA_BUILD_WSK_REGISTER only with kernelSerial 6); policy 1 and kernelSerial 5 / 7: 256 x 256 only. */
int dga_tiling_check(const dga_tiling_t *tiling);

/* TilingFunc of dga_gemm_fp8_fp8_fp32_nt (host only): what dga_tiling_bf16_exact returns, except that a tiling naming a build without
 * an fp32 epilogue -- a bf16 image build (DGA_BUILD_BX_AIMAGE / _IMAGE8 / _IMAGE4) or DGA_BUILD_BX_GROUPED (a cache row) -- comes back
 * as the same tile with build = DGA_BUILD_DEFAULT and dispatchPolicyTag = DGA_POLICY_BF16_EXACT;
 * with $DGA_DEFAULT_POLICY = "strict" the strict tag.  DGA_E_RANGE: $DGA_DEFAULT_POLICY names no policy.  No reference counterpart. */
int dga_tiling_fp32_out(const dga_problem_t *problem, dga_tiling_t *out);
/* dga_tiling_check plus the fp32 entry's refusals (host only): DGA_E_TILING for a dispatchPolicyTag other than DGA_POLICY_BF16_EXACT or
 * DGA_POLICY_STRICT (the fast schedules), DGA_POLICY_UE8M0_SCALES, and the builds DGA_BUILD_BX_AIMAGE / _IMAGE8 / _IMAGE4 / _GROUPED.
 * Every other bf16-exact build -- the one-tile and persistent tiles, the two-launch split-K, the quarter-tile tail, the one-launch decode
 * split-K, Stream-K and workgroup split-K -- has an fp32 epilogue. */
int dga_tiling_check_fp32_out(const dga_tiling_t *tiling);

/* TilingFunc of dga_wgrad_gemm_fp8_fp8_fp32_nt (host only): what dga_tiling_fp32_out returns, with every build that has no per-row-sfb
 * form mapped onto the same tile: kernelSerial 6 (the workgroup split-K, and with it DGA_BUILD_BX_DECODE / DGA_BUILD_WSK_REGISTER)
 * becomes the two-launch split-K of the same splitkFactor (kernelSerial 4; 0 where splitkFactor is 1), kernelSerial 7 (one-launch
 * Stream-K) kernelSerial 0, those build names DGA_BUILD_DEFAULT.  With $DGA_DEFAULT_POLICY = "strict" the strict tag.  No reference
 * counterpart. */
int dga_tiling_wgrad(const dga_problem_t *problem, dga_tiling_t *out);
/* dga_tiling_check_fp32_out plus the weight-gradient entry's refusals (host only): DGA_E_TILING for kernelSerial 6 or 7 and the builds
 * DGA_BUILD_BX_DECODE / DGA_BUILD_WSK_REGISTER under the bf16-exact tag.  The one-tile and persistent tiles, the two-launch split-K, the
 * quarter-tile tail and the strict kernel have a per-row-sfb form. */
int dga_tiling_check_wgrad(const dga_tiling_t *tiling);

/* TilingFunc of dga_k_grouped_wgrad_gemm_fp8_fp8_fp32_nt (host only; problem->k = K_total, problem->groups = G): a rule on the raster of
 * G x tiles(M, N) alone -- the persistent 128 x 256 build (DGA_BUILD_BX_PERSISTENT) where those tiles fill the CUs and every group has at
 * least eight (one per XCD), otherwise the
 * tallest, then widest one-tile tile (DGA_BUILD_BX_ONE_TILE of 128 x 128, 64 x 256, 64 x 128, 32 x 128) whose raster does, else 32 x 128;
 * kernelSerial 0, splitkFactor 1, so dga_workspace_bytes() is 0.  Tag 7; with $DGA_DEFAULT_POLICY = "strict" the strict tag.  Does not
 * consult the tiling cache (no cache row, sweep or predictor covers this entry).  No reference counterpart. */
int dga_tiling_k_grouped_wgrad(const dga_problem_t *problem, dga_tiling_t *out);
/* dga_tiling_check_wgrad plus the k-grouped entry's refusals (host only): DGA_E_TILING for splitkFactor > 1 (no split-K inside a
 * group, under any tag) and, under the bf16-exact tag, for kernelSerial 4, 5, 6 and 7 (the two-launch split-K, the quarter-tile tail,
 * the workgroup split-K, the one-launch Stream-K), every build but 0, DGA_BUILD_BX_PERSISTENT and DGA_BUILD_BX_ONE_TILE, a tile (m1, n1)
 * that is not exactly one of 128 x 256, 128 x 128, 64 x 256, 64 x 128, 32 x 128, and DGA_BUILD_BX_PERSISTENT off 128 x 256.  The fast
 * tags and the UE8M0 flag are refused as by dga_tiling_check_fp32_out. */
int dga_tiling_check_k_grouped_wgrad(const dga_tiling_t *tiling);

/* The arithmetic of an fp8 call that names neither a policy nor a tiling: $DGA_DEFAULT_POLICY, parsed and validated ONCE per process,
 * here, for every front end (the C entry points with tiling == NULL, deepgemm_ascend_amd/api.py, the deep_gemm_cpp extension).
 * Names: "bf16_exact" (the default: inside the operator's 2-ULP contract), "fast", "strict", "fast_ue8m0", "bf16_exact_ue8m0" (the
 * caller's promise of power-of-two scales for every call), "auto" (bf16-exact where the decode kernel carries it, fast elsewhere).
 * Writes the NUL-terminated name to name_out[cap] (nullable) and returns DGA_OK -- or DGA_E_RANGE for a value that is none of these
 * (an unset or empty variable is "bf16_exact"): a typo must not silently change the arithmetic; every fp8 entry that needs the default
 * returns the same error.  No reference counterpart (its one kernel has one arithmetic). */
int dga_default_policy(char *name_out, int cap);

/* SelectKernel without the cache, on an explicit platform (select_kernel.cpp:333-369).
 * platform == NULL -> MI355X.  With dga_platform_ascend910b() it replays the reference's
 * DoTilingLayout01 + handler chain for parity tests. */
int dga_select_kernel(const dga_problem_t *problem, const dga_platform_t *platform, dga_tiling_t *out);

void dga_platform_mi355x(dga_platform_t *out);
void dga_platform_ascend910b(dga_platform_t *out, uint32_t core_num /*24 C++ default, 20 Python default*/);

/* Learned predictor (get_best_config/get_best_config.py:166-670 TilingPredictor + model.py TimePredictMLP; C++ hook
 * op_tiling/predictor.cpp:107-157, SelectKernelWithPredictor select_kernel.cpp:380-388).  The weights file is the
 * text export of harness/train_predictor.py; tuned/predictor_mi355x.txt next to the library is loaded on first use
 * unless $DGA_NO_PREDICTOR is set.  dga_tiling() consults it on a cache miss for dense fp8 problems.
 *   dga_predictor_load(NULL) = the default file; DGA_E_IO if the file is missing or malformed.
 *   dga_select_kernel_with_predictor: native tiling (dga_select_kernel) unless the model's greedy pick over the
 *   compiled candidates promises >= 20 % over it (the reference: 3 %; raised by measurement against the fitted selector) and there are >= 4 candidates (the reference's two fallbacks,
 *   get_best_config.py:587-621); *predicted_us / *native_us = the model's times for the result / the native tiling
 *   (0 when no model is loaded or the problem is outside what the model covers). */
int dga_predictor_load(const char *path);
void dga_predictor_unload(void);
int dga_predictor_loaded(void);
int dga_predict_time_us(const dga_problem_t *problem, const dga_tiling_t *tiling, float *us);
/* Selection strategies of the predictor (get_best_config.py:431-525 select_tiling_strategy): greedy, topk_median, topk_dbscan.
 * preds[count] = predicted times, tiles[count][3] = (mTile, nTile, kTile) of every candidate (used by topk_dbscan only).
 * *picked_index = the candidate taken; topk_dbscan also returns the winning cluster (cluster_members[<= count], *cluster_count;
 * both nullable) -- the reference draws a random member of it (random.Random(random_state).choice), this library takes its fastest
 * member (random_state == 0) or member random_state % size, so that a pick is reproducible. */
enum { DGA_PICK_GREEDY = 0, DGA_PICK_TOPK_MEDIAN = 1, DGA_PICK_TOPK_DBSCAN = 2 };
int dga_select_tiling_strategy(const float *preds, const int32_t *tiles, int count, int method, int topk, float dbscan_eps,
                               int dbscan_min_samples, uint64_t random_state, int *picked_index, int *cluster_members, int *cluster_count);
/* dga_select_kernel_with_predictor with the strategy named (method: DGA_PICK_*, topk as in the reference: 10). */
int dga_select_kernel_with_predictor_ex(const dga_problem_t *problem, dga_tiling_t *out, float *predicted_us, float *native_us,
                                        int method, int topk);
int dga_select_kernel_with_predictor(const dga_problem_t *problem, dga_tiling_t *out, float *predicted_us,
                                     float *native_us);

/* Tiling cache control (TilingCache, cache.cpp:69-100; CSV::Document, csv.cpp:31-140). */
int dga_tiling_cache_open(const char *csv_path);  /* NULL/"" = memory only */
int dga_tiling_cache_clear(void);
int dga_tiling_cache_size(void);

/* workspace: the reference asks the runtime for a fixed 200 MB
 * (catlass_dynamic_matmul_tiling.cpp:115-120); we size it from the tiling (0 unless split-K). */
size_t dga_workspace_bytes(const dga_tiling_t *tiling);

/* ---- the hot path ---------------------------------------------------------------------- */

/* gemm_fp8_fp8_bf16_nt: out[M,N] (bf16) = dequant(A[M,K] e4m3fn, sfa[M,ceil(K/128)] f32)
 *                                       . dequant(B[N,K] e4m3fn, sfb[ceil(N/128),ceil(K/128)] f32)^T
 * Replaces the launch half of run_mmad_rtc / mmad_rtc
 * (deep_gemm_ascend/framework/csrc/python_api.cpp:18, jit_kernels/impls/gemm.hpp:68-111) and of the
 * aclnn op's device entry (op_kernel/catlass_dynamic_matmul.cpp:16-45), NT layout as in
 * catlass_dynamic_matmul_tiling.cpp:83-84.  All rows contiguous (lda = ldb = K, ldc = N).
 * tiling == NULL -> dga_tiling() is called.  Asynchronous on `stream`. */
int dga_gemm_fp8_fp8_bf16_nt(const void *a, const float *sfa, const void *b, const float *sfb, void *out,
                             int m, int n, int k, const dga_tiling_t *tiling, void *workspace,
                             size_t workspace_bytes, void *stream);

/* The same with the operands' own row strides (bytes between rows: lda, ldb >= K, each either K or a multiple of 16; out and the
 * scales stay contiguous) -- what a framework hands over when its tensors are views of padded buffers (the reference's Python
 * entry takes torch tensors, strides and all: deep_gemm_ascend/framework/csrc/python_api.cpp:18).  An operand whose rows start
 * on 16-byte boundaries is read in place.  For K % 16 != 0 that needs the bytes from K to the next 16-byte boundary of every row to
 * be zero, which the caller states per operand with DGA_ROWS_A_ZERO_PADDED / DGA_ROWS_B_ZERO_PADDED (dga_cast_to_fp8_*_ld writes
 * such rows; make the stride a multiple of 128 where possible -- rows that start inside a cache line cost two line requests per
 * 128-byte piece and give the gain back, profiles/r04_odd_k_rows.txt); an operand without the promise goes through the padding
 * pass ALONE -- weights padded once at load time leave only
 * the activations to re-lay out, and operands that both come from the _ld quantisers need no pass at all (the reference fuses
 * its re-layout into the matmul launch instead: op_kernel/kernel/padding_common_matmul_kernel.h:33-107).
 * DGA_E_ALIGN: a stride that is neither K nor a multiple of 16; DGA_E_SHAPE: a stride below K. */
#define DGA_ROWS_A_ZERO_PADDED 1
#define DGA_ROWS_B_ZERO_PADDED 2
int dga_gemm_fp8_fp8_bf16_nt_strided(const void *a, int64_t lda, const float *sfa, const void *b, int64_t ldb, const float *sfb,
                                     void *out, int m, int n, int k, int flags, const dga_tiling_t *tiling, void *workspace,
                                     size_t workspace_bytes, void *stream);

/* gemm_fp8_fp8_fp32_nt: out[M,N] (fp32) = C[M,N] (fp32, optional) + dequant(A) . dequant(B)^T -- the fp32 result the reference's
 * run_mmad_rtc writes into its caller-allocated z[B,M,N] (deep_gemm_ascend/framework/csrc/python_api.cpp:18,
 * jit_kernels/impls/gemm.hpp:68-111; its golden is the fp32 np.matmul, scripts/gen_golden.py:14-15), with upstream DeepGEMM's fp32-output
 * accumulation on top.  Operands, scales, strides and flags exactly as in dga_gemm_fp8_fp8_bf16_nt_strided (lda = ldb = K: contiguous
 * rows).  out and c are contiguous [M,N] fp32 (ldc = N).
 *   c == NULL: no addend; every element of out is written and its old contents are never read.  c == out: in-place accumulation;
 *   a c that partially overlaps out: DGA_E_SHAPE.  The addend goes in with one fp32 add after the product is complete,
 *   out = fl(acc + c) -- never into a partial sum (split-K adds it once, in its combine).  K = 0: out = c (or zeros).
 *   Arithmetic: bf16-exact (dispatchPolicyTag 7: the accumulator the bf16 entry rounds, bit for bit) or strict (3: the oracle's fp32).
 *   tiling == NULL -> dga_tiling_fp32_out(): bf16-exact, or strict when $DGA_DEFAULT_POLICY is "strict"; any other process default
 *   ("fast", "auto", the _ue8m0 forms) gives bf16-exact for this entry.  A tiling is checked by dga_tiling_check_fp32_out before
 *   anything is launched.  The workspace is what the bf16 call on the same tiling needs.  Asynchronous on `stream`. */
int dga_gemm_fp8_fp8_fp32_nt(const void *a, int64_t lda, const float *sfa, const void *b, int64_t ldb, const float *sfb, const float *c,
                             float *out, int m, int n, int k, int flags, const dga_tiling_t *tiling, void *workspace,
                             size_t workspace_bytes, void *stream);

/* wgrad_gemm_fp8_fp8_fp32_nt: upstream DeepGEMM's weight-gradient GEMM, out[M,N] (fp32) = C[M,N] (fp32, optional) +
 * dequant(A) . dequant(B)^T with per-1x128 scales on BOTH operands ("1D1D"): sfa [M, ceil(K/128)] and sfb [N, ceil(K/128)], row-major --
 * one scale per row of B per 128-wide k block, what per_token_cast_to_fp8 writes for an activation.  For dW = dY^T . X: A = dY^T
 * [out_features, tokens], B = X^T [in_features, tokens], K = tokens, and out accumulated across micro-batches with c == out.
 * Everything else -- strides, DGA_ROWS_*_ZERO_PADDED, c == NULL / c == out / partial overlap (DGA_E_SHAPE), K = 0 (out = c),
 * workspace, asynchrony -- is dga_gemm_fp8_fp8_fp32_nt's.  The promotion scale of an output is fl(sfa[m, kb] * sfb[n, kb]); with every
 * row of a 128-row block of B on one scale the result is that of dga_gemm_fp8_fp8_fp32_nt on the same tiling, bit for bit.
 * tiling == NULL -> dga_tiling_wgrad(); a tiling is checked by dga_tiling_check_wgrad before anything is launched.  No reference
 * counterpart: the Ascend reference has no weight-gradient path. */
int dga_wgrad_gemm_fp8_fp8_fp32_nt(const void *a, int64_t lda, const float *sfa, const void *b, int64_t ldb, const float *sfb,
                                   const float *c, float *out, int m, int n, int k, int flags, const dga_tiling_t *tiling,
                                   void *workspace, size_t workspace_bytes, void *stream);

/* k_grouped_wgrad_gemm_fp8_fp8_fp32_nt: upstream DeepGEMM's MoE weight-gradient GEMM, G problems whose groups lie along K (the tokens):
 *   out[g] (fp32 [M,N]) = C[g] (fp32, optional) + dequant(A[:, k0_g : k0_g + K_g]) . dequant(B[:, k0_g : k0_g + K_g])^T
 * with A [M, K_total] fp8 (row stride lda), sfa [M, K_total/128], B [N, K_total] fp8 (row stride ldb), sfb [N, K_total/128] -- the
 * per-1x128 scales of dga_wgrad_gemm_fp8_fp8_fp32_nt on both operands -- and K_g = ks[g], k0_g = sum_{h<g} K_g.  ks is a device
 * int32[groups], read while the call executes (a captured graph replays with the counts of the moment); every K_g a multiple of 128
 * (DGA_CONTIGUOUS_M_ALIGNMENT: the contiguous forward layout's segments, transposed), 0 allowed, sum <= K_total (columns past the sum
 * are never read).  Counts that break this give unspecified numbers, never a read outside A, B, sfa, sfb or a write outside out: the
 * kernels clamp every group to [0, K_total).  K_g = 0: out[g] = C[g] exactly, or zeros.  out and C are [G, M, N] contiguous; C may be
 * out itself, a partial overlap is DGA_E_SHAPE.  K_total % 128, negative sizes: DGA_E_SHAPE; lda / ldb below K_total: DGA_E_SHAPE, not
 * a multiple of 16: DGA_E_ALIGN; NULL pointers where there is work: DGA_E_NULL -- all before any launch.  flags: 0 or
 * DGA_ROWS_*_ZERO_PADDED (no effect: rows of whole k blocks).  One launch; no workspace (workspace may be NULL, any size is ignored).
 * Numerics: tag 7 -- group g is, bit for bit, dga_wgrad_gemm_fp8_fp8_fp32_nt on contiguous copies of its slices with the same tile and
 * no split-K, then + C[g]; tag 3 -- the oracle's fp32 result, bit for bit.  tiling == NULL -> dga_tiling_k_grouped_wgrad(); a tiling is
 * checked by dga_tiling_check_k_grouped_wgrad before anything is launched.  No reference counterpart. */
int dga_k_grouped_wgrad_gemm_fp8_fp8_fp32_nt(const void *a, int64_t lda, const float *sfa, const void *b, int64_t ldb, const float *sfb,
                                             const float *c, float *out, const int32_t *ks, int groups, int m, int n, int k_total,
                                             int flags, const dga_tiling_t *tiling, void *workspace, size_t workspace_bytes,
                                             void *stream);

/* m_grouped_gemm_fp8_fp8_bf16_nt_masked: G independent problems
 *   a [G,m_max,K], sfa [G,m_max,KB], b [G,N,K], sfb [G,NB,KB], out [G,m_max,N];
 *   only rows < masked_m[g] (device int32[G]) of out[g] are written.  masked_m is read on the device while the call
 *   executes (like every operand it must not be written concurrently).
 * No reference counterpart beyond the uniform batch loop (generate_code.hpp:149-153); SURVEY.md 8(b). */
int dga_m_grouped_gemm_fp8_fp8_bf16_nt_masked(const void *a, const float *sfa, const void *b, const float *sfb,
                                              void *out, const int32_t *masked_m, int groups, int m_max, int n,
                                              int k, int expected_m, const dga_tiling_t *tiling, void *workspace,
                                              size_t workspace_bytes, void *stream);

/* The masked grouped GEMM on rows that stay where they are: instead of a packed [G, m_max, K] activation tensor, row r of
 * group g is row row_index[g * m_max + r] of ONE flat source -- a (rows x lda bytes, lda % 16 == 0, rows * lda < 2 GiB),
 * its scales at sfa + row * sfa_ld floats (they may ride inside the same payload rows) -- and its result goes to row
 * row_index[g * m_max + r] of the flat destination out (ldc bf16 elements per row).  Only entries r < masked_m[g] of the
 * table are read.  This removes the pack / unpack copies either side of the GEMM in the expert-sharded forward (the
 * tokens are gathered by the kernel's own tile loads and scattered by its stores); dga_route_slots builds the table.
 * K % 16 != 0 runs the element-wise kernel.  No reference counterpart (row 8(e)). */
int dga_m_grouped_gemm_fp8_fp8_bf16_nt_masked_indexed(const void *a, int64_t lda, const float *sfa, int64_t sfa_ld,
                                                      const void *b, const float *sfb, void *out, int64_t ldc,
                                                      const int64_t *row_index, int64_t rows, const int32_t *masked_m,
                                                      int groups, int m_max, int n, int k, int expected_m,
                                                      const dga_tiling_t *tiling, void *workspace, size_t workspace_bytes,
                                                      void *stream);

/* The aclnn operator in its own dtypes (CatlassDynamicMatmul, op_host/catlass_dynamic_matmul.cpp:50-80; device entry
 * op_kernel/catlass_dynamic_matmul.cpp:16-45): out[M,N] = self[M,K] . mat2, self row-major, mat2 logical [K,N] stored
 * column-major = physical [N,K] (NT, catlass_dynamic_matmul_tiling.cpp:83-84), all three of `dtype` (DGA_DT_FP16 or
 * DGA_DT_BF16; fp32 accumulate, one RNE rounding at the end).  workspace: dga_catlass_dynamic_matmul_workspace_bytes()
 * (padded operand copies when K % 64 != 0 or a base is not 16-byte aligned; split-K slabs for small M); NULL is legal
 * (single pass, element-wise kernel for unaligned shapes). */
size_t dga_catlass_dynamic_matmul_workspace_bytes(int m, int n, int k, const void *self, const void *mat2);
int dga_catlass_dynamic_matmul(const void *self, const void *mat2, void *out, int m, int n, int k, int dtype,
                               void *workspace, size_t workspace_bytes, void *stream);

/* m_grouped_gemm_fp8_fp8_bf16_nt_contiguous: the prefill-side MoE layout.
 *   a [m_sum,K], sfa [m_sum,KB], b [G,N,K], sfb [G,NB,KB], out [m_sum,N], m_indices device int32[m_sum].
 * Row r is multiplied with b[m_indices[r]]; rows with m_indices[r] < 0 are padding and are not written.
 * Layout contract: the rows of one group are consecutive, every group segment starts at a multiple of
 * DGA_CONTIGUOUS_M_ALIGNMENT rows, and a segment's padding rows (-1) follow its valid rows.
 * No reference counterpart (the reference has only the uniform batch loop, generate_code.hpp:149-153). */
int dga_m_grouped_gemm_fp8_fp8_bf16_nt_contiguous(const void *a, const float *sfa, const void *b, const float *sfb,
                                                  void *out, const int32_t *m_indices, int m_sum, int groups, int n,
                                                  int k, const dga_tiling_t *tiling, void *workspace,
                                                  size_t workspace_bytes, void *stream);

/* Quantisers upstream of the GEMM: x [rows,k] contiguous, x_dtype in
 * {DGA_DT_FP32, DGA_DT_BF16, DGA_DT_FP16} -> q [rows,k] e4m3fn bytes and fp32 scales
 *   1x128:    sf [rows, ceil(k/128)]              (the A-operand / activation format)
 *   128x128:  sf [ceil(rows/128), ceil(k/128)]    (the B-operand / weight format)
 * scale = amax/448 (1 when the block is all zero), q = RNE-satfinite(x / scale).  The reference's inputs are fp16
 * files from numpy (scripts/gen_data.py:10-30); it has no quantiser. */
int dga_cast_to_fp8_1x128(const void *x, int x_dtype, int64_t rows, int64_t k, void *q, float *sf, void *stream);
int dga_cast_to_fp8_128x128(const void *x, int x_dtype, int64_t rows, int64_t k, void *q, float *sf, void *stream);
/* The same writing rows ldq bytes apart (k <= ldq <= 128 * ceil(k/128)) with ZEROS from byte k to the end of each row: with
 * ldq = round_up(k, 128) (whole cache lines; round_up(k, 16) is the minimum) the result is an operand
 * dga_gemm_fp8_fp8_bf16_nt_strided reads in place (DGA_ROWS_*_ZERO_PADDED). */
int dga_cast_to_fp8_1x128_ld(const void *x, int x_dtype, int64_t rows, int64_t k, void *q, int64_t ldq, float *sf, void *stream);
int dga_cast_to_fp8_128x128_ld(const void *x, int x_dtype, int64_t rows, int64_t k, void *q, int64_t ldq, float *sf, void *stream);
/* The same with flags (ABI 6).  DGA_CAST_UE8M0: every block scale is rounded UP to a power of two, 2^ceil(log2(amax / 448)) -- the
 * "UE8M0" scales of upstream DeepGEMM's per_token_cast_to_fp8(..., use_ue8m0=True); still written as fp32.  GEMM calls on such
 * operands may set DGA_POLICY_UE8M0_SCALES (the scales then ride in the matrix instruction's E8M0 operands).  ldq as in the _ld forms
 * (ldq = k: contiguous rows).  DGA_E_RANGE: an unknown flag. */
#define DGA_CAST_UE8M0 1
int dga_cast_to_fp8_1x128_ex(const void *x, int x_dtype, int64_t rows, int64_t k, void *q, int64_t ldq, float *sf, int flags, void *stream);
int dga_cast_to_fp8_128x128_ex(const void *x, int x_dtype, int64_t rows, int64_t k, void *q, int64_t ldq, float *sf, int flags, void *stream);

/* The activation of a MoE expert MLP fused into the 1x128 quantiser that feeds its second GEMM:
 *   (q, sf) = cast_to_fp8_1x128( silu(x[..., :h]) * x[..., h:] ),   silu(g) = g / (1 + exp(-g)),
 * x [groups, rows, 2h] contiguous (gate = the first h columns of a row, up = the last h: the silu_and_mul convention),
 * x_dtype as above, q [groups, rows, h] e4m3fn bytes, sf [groups, rows, ceil(h/128)] fp32.  The product is formed in fp32 and never
 * rounded to 16 bits; q and sf are what dga_cast_to_fp8_1x128_ex gives on that fp32 product (flags: DGA_CAST_UE8M0).  Accuracy of the
 * product: for gate >= 20 it is fl32(gate * up) exactly (1 + exp(-g) rounds to 1), for |gate| <= 16 it is within relative 2^-18 of
 * the real-number value (hardware base-2 exponential and a refined reciprocal, not the IEEE division), for gate <= -88.8 exp(-g)
 * overflows and the product is +-0 (so for gate <= -120, where the real value is below the smallest fp32 subnormal per unit of up).
 * Row masks, read on the device (a captured graph follows the routing); at most one may be given:
 *   masked_m  int32[groups]  rows r >= masked_m[g] of group g are neither read nor written, in q and in sf alike (the layout of
 *                            dga_m_grouped_gemm_fp8_fp8_bf16_nt_masked)
 *   m_indices int32[rows]    groups = 1; rows with a negative index are neither read nor written (the tensor
 *                            dga_m_grouped_gemm_fp8_fp8_bf16_nt_contiguous takes)
 * DGA_E_RANGE: an unknown flag, or more 1x128 blocks than one grid holds (2^31 - 1 workgroups of 16 blocks);  DGA_E_SHAPE: a negative
 * size, groups < 1, both masks, m_indices with groups != 1;  a zero size is DGA_OK with nothing done;  then DGA_E_NULL, DGA_E_DTYPE. */
int dga_silu_mul_cast_to_fp8_1x128(const void *x, int x_dtype, int64_t groups, int64_t rows, int64_t h,
                                   const int32_t *masked_m, const int32_t *m_indices,
                                   void *q, float *sf, int flags, void *stream);

/* Its backward, fused into the 1x128 quantiser that feeds the dgrad of the first GEMM (K = 2h):
 *   dgate = grad_h * up * silu'(gate),   dup = grad_h * silu(gate),   silu'(g) = s + g s (1 - s),  s = 1 / (1 + exp(-g)),
 *   (dq, dsf) = cast_to_fp8_1x128( [dgate | dup] ),
 * x [groups, rows, 2h] as above (the tensor the forward read), grad_h [groups, rows, h], both contiguous and of `dtype`;
 * dq [groups, rows, 2h] e4m3fn bytes (dgate in the first h columns of a row, dup in the last h), dsf [groups, rows, 2h/128] fp32.
 * h % 128 == 0 is required: no 1x128 block of the [2h] axis straddles the two halves.  grad_x (may be NULL): [groups, rows, 2h] of
 * `dtype`, receives the unquantised fp32 gradient in the same pass (rounded to nearest even for the 16-bit types), on the rows that
 * are written; what dga_cast_to_fp8_1x128_transposed (same mask) turns into the operand of dga_k_grouped_wgrad_gemm_fp8_fp8_fp32_nt.  Both gradients are formed in
 * fp32 and never rounded to 16 bits before they are quantised; dq and dsf are what dga_cast_to_fp8_1x128_ex gives on them (flags:
 * DGA_CAST_UE8M0).  Accuracy: for gate >= 20 dgate = fl32(grad_h * up) and dup = fl32(grad_h * gate) exactly; for |gate| <= 16 dup is
 * within relative 2^-18 and dgate within 2^-17 |grad_h up| (s + |g| s (1 - s)) of the real-number value (silu' has a root at
 * g = -1.2785: no relative bound there); for gate <= -88.8 both are +-0.  A NaN in gate or grad_h gives NaN codes in both halves, a
 * NaN in up in dgate alone.  masked_m, m_indices: as above; a row a mask excludes is neither read nor written, in dq, dsf and grad_x.
 * DGA_E_RANGE: an unknown flag, or more blocks than one grid holds;  DGA_E_SHAPE: a negative size, h % 128 != 0, groups < 1, both
 * masks, m_indices with groups != 1;  a zero size is DGA_OK with nothing done;  then DGA_E_NULL (x, grad_h, dq, dsf), DGA_E_DTYPE. */
int dga_silu_mul_bwd_cast_to_fp8_1x128(const void *x, const void *grad_h, int dtype, int64_t groups, int64_t rows, int64_t h,
                                       const int32_t *masked_m, const int32_t *m_indices,
                                       void *dq, float *dsf, void *grad_x, int flags, void *stream);

/* The 1x128 quantiser of the TRANSPOSE of token-major activations, in one pass -- the operands of dga_wgrad_gemm_fp8_fp8_fp32_nt and
 * dga_k_grouped_wgrad_gemm_fp8_fp8_fp32_nt (K along the tokens) from the [T, h] tensors the forward and the fused quantisers work on:
 *   (qt, sft) = cast_to_fp8_1x128_ex( where(valid, x, 0)^T ),   byte for byte and bit for bit,
 * x [groups, rows, h] contiguous of x_dtype (as above), T = groups * rows, qt [h, T] e4m3fn bytes in rows ldqt bytes apart,
 * T <= ldqt <= round_up(T, 128), with zeros from byte T to the end of each row (the _ld forms' rule), sft [h, ceil(T/128)] fp32.
 * masked_m, m_indices: as above, with the other meaning for the output: a row they exclude is not read (NaN or garbage in it changes
 * nothing) and counts as zeros -- its codes are 0x00, and a 128-token block without a valid row has scale 1.  Every byte of qt and every
 * scale of sft is written.  q_row, sf_row (both NULL or both set): (q_row [T, h], sf_row [T, ceil(h/128)]) = cast_to_fp8_1x128_ex(x)
 * from the same read of x, on the valid rows; the rows a mask excludes are not written there.  T and h may be any value.
 * flags: DGA_CAST_UE8M0.  DGA_E_RANGE: an unknown flag;  DGA_E_SHAPE: a negative size, groups < 1, both masks, m_indices with
 * groups != 1, ldqt outside its range, exactly one of q_row / sf_row;  T == 0 or h == 0 is DGA_OK with nothing touched;  then
 * DGA_E_NULL (x, qt, sft), DGA_E_DTYPE, and DGA_E_RANGE for more 128 x 128 tiles than one grid holds. */
int dga_cast_to_fp8_1x128_transposed(const void *x, int x_dtype, int64_t groups, int64_t rows, int64_t h,
                                     const int32_t *masked_m, const int32_t *m_indices,
                                     void *qt, int64_t ldqt, float *sft, void *q_row, float *sf_row,
                                     int flags, void *stream);

/* The same quantiser with the rows read through a table -- the dispatch of an MoE layer fused into the quantiser, driven by
 * dga_route_slots' slot -> pair table (`inverse`) as it is:
 *   xg[r] = src[index[r] / index_div]                                        (row_scale == NULL; xg has src_dtype)
 *   xg[r] = fl32(row_scale[index[r]] * fl32(src[index[r] / index_div]))      (row_scale: fp32 [src_rows * index_div]; xg is fp32;
 *                                                                             one multiplication, no special cases)
 * src [src_rows, h] contiguous of src_dtype (as above), index int64 [groups, rows], T = groups * rows, P = src_rows * index_div the number
 * of (token, choice) pairs.  Row r is valid iff masked_m does not exclude it and 0 <= index[r] < P.  An index that masked_m excludes is NOT
 * READ (dga_route_slots leaves stale values there); a value outside [0, P) excludes the row and dereferences nothing.  The result is
 * dga_cast_to_fp8_1x128_transposed's on xg with the excluded rows masked, byte for byte and bit for bit, and that entry's contract carries
 * over: an excluded row counts as zeros and is never read, every byte of qt [h, T] (rows ldqt bytes apart) and every scale of sft is
 * written, a 128-token block without a valid row has scale 1, and (q_row, sf_row) -- both NULL or both set -- are written on the valid rows
 * only.  xg itself is never written.  The uses on dga_route_slots(keys = the top-k ids, cap = rows): index = inverse, index_div = k,
 * masked_m = counts for the forward's lhs; the same with src = dY and row_scale = the routing weights for the backward's; groups = 1 and
 * index with -1 on the padding rows for the contiguous layout.  flags: DGA_CAST_UE8M0.  Checks, in dga_cast_to_fp8_1x128_transposed's
 * order: DGA_E_RANGE: an unknown flag;  DGA_E_SHAPE: a negative size, groups < 1, index_div < 1, src_rows * index_div beyond int64,
 * groups != 1 without masked_m, ldqt outside its range, exactly one of q_row / sf_row;  T == 0 or h == 0 is DGA_OK with nothing touched;
 * then DGA_E_NULL (src unless src_rows == 0, index, qt, sft), DGA_E_DTYPE, and DGA_E_RANGE for more 128 x 128 tiles than one grid holds
 * or src_rows * h beyond int64. */
int dga_gather_cast_to_fp8_1x128_transposed(const void *src, int src_dtype, int64_t src_rows, int64_t h, const int64_t *index,
                                            int64_t index_div, const float *row_scale, int64_t groups, int64_t rows,
                                            const int32_t *masked_m, void *qt, int64_t ldqt, float *sft, void *q_row, float *sf_row,
                                            int flags, void *stream);

/* The same quantiser on h = silu(gate) * up -- the operand of the weight gradient of an expert MLP's second GEMM, dW2[g] = dout_g^T . h_g,
 * from the tensor dga_silu_mul_cast_to_fp8_1x128 read, in one pass and without h ever leaving fp32 registers:
 *   (qt, sft) = cast_to_fp8_1x128_ex( where(valid, silu(gate) * up, 0)^T ),
 * x [groups, rows, 2h] contiguous of x_dtype (gate in the first h columns of a row, up in the last h), T = groups * rows, qt [h, T] e4m3fn
 * bytes in rows ldqt bytes apart, T <= ldqt <= round_up(T, 128), zeros from byte T to the end of each row, sft [h, ceil(T/128)] fp32.
 * The product is dga_silu_mul_cast_to_fp8_1x128's, with its accuracy: fl32(gate * up) exactly for gate >= 20 -- there qt and sft are
 * dga_cast_to_fp8_1x128_transposed's on that product byte for byte --, within relative 2^-18 for |gate| <= 16, +-0 for gate <= -88.8; the
 * amax of every 128-token block is rounded from an fp64 value of its largest element, as the forward's block amax is.  A NaN in gate or
 * up gives code sign | 0x7F and is ignored by the amax.  masked_m, m_indices: as in dga_cast_to_fp8_1x128_transposed -- a row they
 * exclude is not read and counts as h = +0 (code 0x00; a 128-token block without a valid row has scale 1), and every byte of qt and every
 * scale of sft is written.  q_row, sf_row (both NULL or both set): (q_row [T, h], sf_row [T, ceil(h/128)]) are
 * dga_silu_mul_cast_to_fp8_1x128's outputs, bit for bit, from the same read of x, on the valid rows; the rows a mask excludes are not
 * written there -- a training forward gets both operands in one pass.  T and h may be any value.  flags: DGA_CAST_UE8M0.  Checks, in
 * dga_cast_to_fp8_1x128_transposed's order: DGA_E_RANGE: an unknown flag;  DGA_E_SHAPE: a negative size, groups < 1, both masks,
 * m_indices with groups != 1, ldqt outside its range, exactly one of q_row / sf_row;  T == 0 or h == 0 is DGA_OK with nothing touched;
 * then DGA_E_NULL (x, qt, sft), DGA_E_DTYPE, and DGA_E_RANGE for more 128 x 128 tiles than one grid holds. */
int dga_silu_mul_cast_to_fp8_1x128_transposed(const void *x, int x_dtype, int64_t groups, int64_t rows, int64_t h,
                                              const int32_t *masked_m, const int32_t *m_indices,
                                              void *qt, int64_t ldqt, float *sft, void *q_row, float *sf_row,
                                              int flags, void *stream);

/* The same quantiser on the backward of that activation -- the operand of the weight gradient of an expert MLP's first GEMM,
 * dW1[g] = dY1_g^T . x_g with dY1 = [dgate | dup], from the tensors dga_silu_mul_bwd_cast_to_fp8_1x128 reads, in one pass and without dY1
 * ever leaving fp32 registers:
 *   (qt, sft) = cast_to_fp8_1x128_ex( where(valid, [dgate | dup], 0)^T ),
 * x [groups, rows, 2h] and grad_h [groups, rows, h] contiguous of `dtype`, h % 128 == 0, T = groups * rows, qt [2h, T] e4m3fn bytes in rows
 * ldqt bytes apart (dgate^T in the first h rows, dup^T in the last h), T <= ldqt <= round_up(T, 128), zeros from byte T to the end of each
 * row, sft [2h, ceil(T/128)] fp32.  The contract is by composition: with G the fp32 grad_x that dga_silu_mul_bwd_cast_to_fp8_1x128 writes
 * for the fp32 up-conversion of (x, grad_h) under the same mask, (qt, sft) are dga_cast_to_fp8_1x128_transposed's on G byte for byte and
 * bit for bit, for every `dtype` and on every input (NaN, infinities and gate <= -88.8 included); the gradients have that entry's accuracy.
 * The amax of a 128-token block is the plain fp32 maximum of those gradients (no NaN enters), not an fp64 re-evaluation.  masked_m,
 * m_indices: as in dga_cast_to_fp8_1x128_transposed -- a row they exclude is not read and counts as zeros (code 0x00; a 128-token block
 * without a valid row has scale 1), and every byte of qt and every scale of sft is written.  q_row, sf_row (both NULL or both set):
 * (q_row [T, 2h], sf_row [T, 2h/128]) are dga_silu_mul_bwd_cast_to_fp8_1x128's (dq, dsf) on (x, grad_h) as given, bit for bit, from the
 * same read, on the valid rows; the rows a mask excludes are not written there.  There is no grad_x: not writing it is the point.
 * flags: DGA_CAST_UE8M0.  Checks, in dga_cast_to_fp8_1x128_transposed's order: DGA_E_RANGE: an unknown flag;  DGA_E_SHAPE: a negative
 * size, h % 128 != 0, groups < 1, both masks, m_indices with groups != 1, ldqt outside its range, exactly one of q_row / sf_row;  T == 0
 * or h == 0 is DGA_OK with nothing touched;  then DGA_E_NULL (x, grad_h, qt, sft), DGA_E_DTYPE, and DGA_E_RANGE for more tile halves
 * (2 per 128 tokens x 128 channels of h) than one grid holds. */
int dga_silu_mul_bwd_cast_to_fp8_1x128_transposed(const void *x, const void *grad_h, int dtype, int64_t groups, int64_t rows, int64_t h,
                                                  const int32_t *masked_m, const int32_t *m_indices,
                                                  void *qt, int64_t ldqt, float *sft, void *q_row, float *sf_row,
                                                  int flags, void *stream);

/* The 128x128 quantiser of grouped expert weights and of their transposes, in one pass -- the rhs of fprop (W) and of dgrad (W^T) from
 * the master weights, with no loop over the experts, no transposing copy and no stacking:
 *   (qt[g], sft[g]) = cast_to_fp8_128x128_ex( w[g]^T ),   byte for byte and bit for bit, for every group g,
 * w [groups, n, k] contiguous of w_dtype (DGA_DT_FP32 / BF16 / FP16), qt [groups, k, n] e4m3fn bytes, sft [groups, ceil(k/128),
 * ceil(n/128)] fp32, both contiguous.  A 128x128 block's amax does not change under transposition, so these are the codes and scales of
 * cast_to_fp8_128x128_ex(w[g]) transposed; no scale block mixes two groups, whatever n is.  q_row, sf_row (both NULL or both set):
 * (q_row[g] [n, k], sf_row[g] [ceil(n/128), ceil(k/128)]) = cast_to_fp8_128x128_ex(w[g]) from the same read of w.  Every byte of every
 * output and every scale is written; n and k may be any value.  flags: DGA_CAST_UE8M0.  DGA_E_RANGE: an unknown flag;  DGA_E_SHAPE: a
 * negative size, exactly one of q_row / sf_row;  groups, n or k zero is DGA_OK with nothing touched;  then DGA_E_NULL (w, qt, sft),
 * DGA_E_DTYPE, and DGA_E_RANGE for more 128 x 128 tiles than one grid holds (2^31 - 1). */
int dga_cast_to_fp8_128x128_transposed(const void *w, int w_dtype, int64_t groups, int64_t n, int64_t k,
                                       void *qt, float *sft, void *q_row, float *sf_row, int flags, void *stream);

/* The optimizer step of those weights fused into that quantiser (csrc/dga_adamw_cast.hip): AdamW on the fp32 master weights w [groups,
 * n, k] with their moments m and v (same shape, both of moment_dtype = DGA_DT_FP32 or DGA_DT_BF16) and the weight gradient grad (same
 * shape, grad_dtype = DGA_DT_FP32 or DGA_DT_BF16, read only), all contiguous; w, m and v are updated in place, and no two of w, m, v and
 * grad may overlap in memory (not checked here: the entry sees pointers; the Python wrapper refuses it).  step_scalars: four fp32
 * values on the device, {lr, bc1, bc2s, grad_scale}, read by the kernel -- bc1 = 1 - beta1^step, bc2s = sqrt(1 - beta2^step); nothing of
 * a step's changing state is a launch argument, so one captured graph serves every step.  Per element, every operation in fp32 and
 * rounded on its own (fl), sqrt and / the IEEE correctly rounded ones, subnormals kept:
 *   g   = fl(grad * grad_scale)
 *   m'  = fl(fl(beta1 * m) + fl(fl(1 - beta1) * g))
 *   v'  = fl(fl(beta2 * v) + fl(fl(fl(1 - beta2) * g) * g))
 *   den = fl(fl(sqrt(v') / bc2s) + eps)
 *   w1  = fl(w * fl(1 - fl(lr * weight_decay)))
 *   w'  = fl(w1 - fl(fl(lr / bc1) * fl(m' / den)))
 * w' is stored as fp32, m' and v' RNE in moment_dtype; the update uses the unrounded m' and v'.  A float32 reference reproduces all
 * three bit for bit (a NaN is a NaN: its sign and payload are the hardware's).  The codes are an exact function of the w left behind:
 *   (qt, sft) and, if given, (q_row, sf_row) = what dga_cast_to_fp8_128x128_transposed writes for that w with the same flags, byte
 *   for byte and bit for bit;  shapes, the pairing of q_row / sf_row and flags as there, every element of every output written.
 * A NaN or infinite gradient poisons its own element of w, m and v and no other (the tile's amax ignores NaN; the element's code is
 * sign | 0x7F); eps = 0 with v' = 0 gives 0 / 0 = NaN; grad_scale = 0 and lr = 0 are ordinary inputs.  Rows at and beyond n and
 * columns at and beyond k are neither read nor written; k % 8 != 0 or a pointer short of 16 (codes: 8) bytes takes the bounded
 * element-wise path for that tensor.  One launch, nothing allocated, nothing read back (capturable).  Checks in this order:
 * DGA_E_RANGE: an unknown flag;  DGA_E_SHAPE: a negative size, exactly one of q_row / sf_row;  groups, n or k zero is DGA_OK with
 * nothing launched;  then DGA_E_NULL (w, m, v, grad, step_scalars, qt, sft), DGA_E_DTYPE (fp16 moments or gradient included), and
 * DGA_E_RANGE for a beta outside [0, 1), an eps or weight_decay that is negative, NaN or infinite, and more tiles than one grid holds. */
int dga_adamw_cast_to_fp8_128x128_transposed(void *w, void *m, void *v, int moment_dtype, const void *grad, int grad_dtype,
                                             const float *step_scalars, float beta1, float beta2, float eps, float weight_decay,
                                             int64_t groups, int64_t n, int64_t k, void *qt, float *sft, void *q_row, float *sf_row,
                                             int flags, void *stream);

/* The same step behind a device flag: skip (int32 [1] on the device, NULL = no flag; dga_grad_clip_scalars writes one) is read by the
 * kernel, one uniform branch.  Where skip[0] != 0 nothing is stored to w, m and v -- their bits after the call are their bits before,
 * whatever grad holds, NaN and infinities included -- and the codes are formed from the unchanged w: (qt, sft) and (q_row, sf_row) are
 * dga_cast_to_fp8_128x128_transposed(w) byte for byte, every element of every output written, so the GEMMs behind it in a captured graph
 * read valid operands.  Where skip[0] == 0, and with skip == NULL, every bit of every result is the entry's above, which forwards here
 * with NULL.  The step number stays the caller's: it reads skip back when convenient and does not advance step after a skipped one. */
int dga_adamw_cast_to_fp8_128x128_transposed_skip(void *w, void *m, void *v, int moment_dtype, const void *grad, int grad_dtype,
                                                  const float *step_scalars, float beta1, float beta2, float eps, float weight_decay,
                                                  int64_t groups, int64_t n, int64_t k, void *qt, float *sft, void *q_row, float *sf_row,
                                                  int flags, const int32_t *skip, void *stream);

/* The global gradient norm on the device (csrc/dga_grad_norm.hip): sumsq[0] = sum_i sum_e x_i[e]^2 over `count` contiguous tensors of
 * numel[i] elements (0 allowed) and dtypes[i] = DGA_DT_FP32 or DGA_DT_BF16 (they may be mixed; fp16 is refused, as by the optimizer),
 * all on one device.  accumulate != 0: sumsq[0] = fl(sumsq[0] + sum), added last, so that several calls build one sum.  Every product and
 * every sum is float64: the inputs convert exactly and their squares are exact (48 significant bits) and can neither overflow nor
 * underflow; subnormals are kept; the only roundings are the additions':  |sumsq - exact| <= (n + 1) 2^-53 exact  for n elements.  A NaN
 * or an infinity anywhere makes sumsq non-finite and nothing else can: isfinite(sumsq) is the overflow check of a loss-scaled step.
 * The order of the additions is fixed by the list of (numel, dtype) alone -- not by the pointers, their alignment, the device or the
 * stream -- without floating-point atomics: two runs give the same bits.  Stage 1: one workgroup per chunk of DGA_GRAD_SUMSQ_CHUNK
 * consecutive elements of one tensor (a chunk never spans two), each lane its fixed elements in ascending order, the lanes by a fixed
 * tree, one float64 partial per chunk into the workspace; the tensor table is a kernel argument, 64 list entries per launch, longer
 * lists take more stage-1 launches into disjoint partial ranges.  Stage 2: one workgroup adds the partials in a fixed order and writes
 * sumsq.  A pointer short of 16 bytes takes bounded loads for that tensor alone: the same bits.  dga_grad_sumsq_workspace_bytes: 8 bytes
 * per chunk (0 for a list the entry refuses or an empty one).  Nothing is allocated or read back (capturable).  Checks in this order,
 * every code before the first launch: DGA_E_SHAPE: a negative count or numel;  DGA_E_NULL: sumsq, the three arrays with count > 0, a
 * tensor with numel > 0, the workspace when there is a chunk;  DGA_E_DTYPE;  DGA_E_RANGE: more chunks than a 31-bit grid holds, a
 * workspace that is too small or not 8-byte aligned.  count == 0, or all tensors empty, still writes sumsq = accumulate ? sumsq : 0. */
#define DGA_GRAD_SUMSQ_CHUNK 16384
int64_t dga_grad_sumsq_workspace_bytes(int count, const int64_t *numel);
int dga_grad_sumsq(const void *const *tensors, const int64_t *numel, const int *dtypes, int count, double *sumsq, int accumulate,
                   void *workspace, int64_t workspace_bytes, void *stream);

/* From the sum of squares (possibly all-reduced across ranks in between) to what the optimizer reads.  One lane, float64, one rounding
 * to fp32 on store:
 *   finite = isfinite(sumsq[0])
 *   normd  = pre_scale * sqrt(sumsq[0])               the norm of the unscaled gradients; pre_scale = 1 / loss_scale
 *   q      = max_norm / (normd + eps);  coefd = q < 1 ? q : 1     torch.nn.utils.clip_grad_norm_'s; +inf never clips; 0 / 0 gives 1
 *   norm[0] = f32(normd) (non-finite as it comes);  coef[0] = finite ? f32(coefd) : 0;  step_scalars[3] = finite ? f32(pre_scale coefd) : 0
 *   skip[0] = finite ? 0 : 1                          int32, overwritten at every call
 * step_scalars is the optimizer's fp32 [4]; elements 0 .. 2 are not touched.  DGA_E_NULL: any pointer;  DGA_E_RANGE: max_norm negative or
 * NaN, pre_scale not a finite number > 0, eps negative, NaN or infinite.  One launch, nothing read back (capturable). */
int dga_grad_clip_scalars(const double *sumsq, double max_norm, double pre_scale, double eps, float *step_scalars, float *norm,
                          float *coef, int32_t *skip, void *stream);

/* ---- the framework's 28-int Config (deep_gemm_ascend/framework/csrc/jit/get_best_config.hpp) ---- */

/* struct Config in declaration order (get_best_config.hpp:12-31), 28 uint32. */
int dga_get_best_config(uint32_t batch, uint32_t m, uint32_t n, uint32_t k, uint32_t out[28]);
int dga_get_bench_config(uint32_t m, uint32_t n, uint32_t k, uint32_t m_sections, uint32_t n_sections,
                         uint32_t m_sec_o_blocks, uint32_t n_sec_o_blocks, uint32_t k_o_iter_blocks,
                         uint32_t db_o_blocks, uint32_t out[28]);
/* run_mmad_bench's host write-back: slots 0..5 are the knobs in, slots 6..27 are filled in the
 * Python-binding order of gemm_bench.hpp:68-81 (m,n,k,batch,k_iters,...,r_db_num). */
int dga_bench_params_fill(uint32_t m, uint32_t n, uint32_t k, int32_t params[28]);
/* benchmark_msprof's order (benchmark_util.h:78-85): m,n,k,6 knobs,batch,k_iters,... */
int dga_bbit_params(uint32_t m, uint32_t n, uint32_t k, uint32_t m_sections, uint32_t n_sections,
                    uint32_t m_sec_o_blocks, uint32_t n_sec_o_blocks, uint32_t k_o_iter_blocks,
                    uint32_t db_o_blocks, uint32_t out[28]);

/* ---- the framework's 16-bit path (what the reference ships today) ----------------------- */

/* run_mmad_rtc (python_api.cpp:18, gemm.hpp:68-111): z[B,M,N] f32 = x[B,M,K] . y[B,K,N], x/y bf16 or fp16. */
int dga_run_mmad_rtc(const void *x, const void *y, float *z, int batch, int m, int n, int k, int dtype,
                     void *stream);
/* run_mmad_bench (python_api.cpp:23, gemm_bench.hpp:49-113): z[M,N] f32 = x[M,K] . y[K,N];
 * params_host = the 28 ints after dga_bench_params_fill (the knobs only steer the Ascend kernel). */
int dga_run_mmad_bench(const void *x, const void *y, float *z, int m, int n, int k, int dtype,
                       const int32_t *params_host, void *stream);

/* The same with a caller-provided workspace of dga_mmad_workspace_bytes(): y is transposed (and x padded when K is not
 * a multiple of 64) into it and the LDS-DMA / MFMA tile kernel runs; without a workspace the entry points above gather
 * fragments straight from global memory (same results, much slower). */
size_t dga_mmad_workspace_bytes(int batch, int m, int n, int k, const void *x);
int dga_run_mmad_rtc_ws(const void *x, const void *y, float *z, int batch, int m, int n, int k, int dtype,
                        void *workspace, size_t workspace_bytes, void *stream);
int dga_run_mmad_bench_ws(const void *x, const void *y, float *z, int m, int n, int k, int dtype,
                          const int32_t *params_host, void *workspace, size_t workspace_bytes, void *stream);

/* ---- expert sharding helper (the reference has no routing or collective of any kind) ------- */

/* Token routing for the dispatch: counts[g] = number of t with expert_ids[t] == g (int64, zeroed here) and pos[t] =
 * position of token t in the expert-sorted order (an expert's tokens are contiguous, their relative order is
 * unspecified; ids outside [0, groups) get pos -1 and are not counted).  One pass of atomics in place of a device sort
 * and a histogram.  No reference counterpart (row 8(e)). */
int dga_route_tokens(const int64_t *expert_ids, int64_t tokens, int groups, int64_t *counts, int64_t *pos, void *stream);

/* Capacity-bounded slot assignment, the routing step of the sharded forward that needs no host round trip (static
 * shapes: the whole forward is capturable in a HIP graph).  Row r carries an int32 key at keys + r * key_stride_bytes
 * (an expert id; negative = unused row).  hi = key / key_div, lo = key % key_div;
 *   bucket = hi                                        (key_sub == 0)
 *   bucket = (lo / key_sub) * key_mul + hi             (key_sub > 0: expert chunk, then destination rank)
 * dest[r] = bucket * cap + (next free slot of the bucket, one atomic), or -1 for an unused row / an unknown bucket; a
 * full bucket gives -1 and adds 1 to *overflow per dropped row (device int32 counter, sticky -- the caller reads and clears it).
 * counts (device int32[buckets]) end as the rows placed per bucket (zeroed first when zero_counts != 0); tags != NULL:
 * the int32 at tags + dest[r] * tag_stride_bytes receives lo (the payload header the receiving rank routes by).
 * Slot order inside a bucket is the atomics' arrival order.  No reference counterpart (row 8(e)).
 * inverse != NULL (device int64[buckets * cap]): inverse[dest[r]] = r + inverse_base, the slot -> row table of
 * dga_m_grouped_gemm_fp8_fp8_bf16_nt_masked_indexed. */
int dga_route_slots(const void *keys, int64_t key_stride_bytes, int64_t rows, int key_div, int key_sub, int key_mul,
                    int buckets, int cap, int32_t *counts, int zero_counts, int64_t *dest, void *tags,
                    int64_t tag_stride_bytes, int32_t *overflow, int64_t *inverse, int64_t inverse_base, void *stream);

/* Indexed row copy on the device: for r in [0, rows):
 *   dst[(dst_index ? dst_index[r] : r) * dst_row_stride .. +row_bytes) = src[(src_index ? src_index[r] : r) * src_row_stride ..)
 * (strides in bytes; index arrays are device int64).  Packs token rows for the dispatch all-to-all, scatters the
 * received rows into the masked [G, m_max, K] layout, and the reverse for the combine. */
int dga_copy_rows(void *dst, int64_t dst_row_stride, const int64_t *dst_index, const void *src, int64_t src_row_stride,
                  const int64_t *src_index, int64_t row_bytes, int64_t rows, void *stream);
/* Two row streams with shared indices in one launch: dst0[di] = src0[si] (row_bytes0) and dst1[di] = src1[si]
 * (row_bytes1) -- the dispatch's pack (fp8 bytes + scales -> one payload row) and unpack. */
int dga_copy_rows2(void *dst0, int64_t dst0_row_stride, const void *src0, int64_t src0_row_stride, int64_t row_bytes0,
                   void *dst1, int64_t dst1_row_stride, const void *src1, int64_t src1_row_stride, int64_t row_bytes1,
                   const int64_t *dst_index, const int64_t *src_index, int64_t rows, void *stream);

/* The combine of an MoE layer on dga_route_slots' pair -> slot table (dest int64 [tokens, k], k >= 1; a dropped choice holds -1):
 *   acc = +0;  for j = 0 .. k - 1 in that order, where 0 <= dest[t, j] < src_rows:
 *       acc = fl32(acc + fl32(weights[t, j] * fl32(src[dest[t, j], c])))       (two roundings, never a fused multiply-add;
 *                                                                                weights == NULL: the product is the value itself)
 *   out[t, c] = RNE(acc)
 * src [src_rows, h] contiguous of src_dtype (DGA_DT_FP32 / BF16 / FP16), weights fp32 [tokens, k] or NULL, out [tokens, h] contiguous of
 * out_dtype = src_dtype or DGA_DT_FP32.  A choice whose dest is outside [0, src_rows) is skipped whatever its weight, a token without a
 * valid choice gets a row of +0, and every element of out is written.  This is float32 arithmetic in a stated order: a host reference
 * reproduces it bit for bit.  weights == NULL is the backward of the dispatch, dX[t] = sum_j dX_slots[dest[t, j]].  One pass: every valid
 * choice's row is read once and out is written once.  DGA_E_SHAPE: a negative size, k < 1, tokens * k beyond int64;  tokens == 0 or h == 0
 * is DGA_OK with nothing touched;  then DGA_E_NULL (src unless src_rows == 0, dest, out), DGA_E_DTYPE, and DGA_E_RANGE for k beyond
 * 2^31 - 1, rows * h beyond int64 or more workgroups than one grid holds. */
int dga_combine_rows(const void *src, int src_dtype, int64_t src_rows, int64_t h, const int64_t *dest, const float *weights,
                     int64_t tokens, int64_t k, void *out, int out_dtype, void *stream);

/* The gradient of the combine with respect to its weights: dw[t, j] = sum_c src[dest[t, j], c] * grad[t, c], fp32 [tokens, k], products and
 * sums in fp32 in a fixed order (no floating-point atomics: two runs on the same inputs give the same bits), +0 for a choice whose dest is
 * outside [0, src_rows).  src [src_rows, h] and grad [tokens, h] contiguous of `dtype`; grad[t] is read once for every 8 choices of a
 * token.  Every element of dw is written.  Checks as in dga_combine_rows (DGA_E_NULL: src unless src_rows == 0, grad, dest, dw); h == 0 is
 * DGA_OK with nothing touched, dw included. */
int dga_combine_rows_weight_grad(const void *src, const void *grad, int dtype, int64_t src_rows, int64_t h, const int64_t *dest,
                                 int64_t tokens, int64_t k, float *dw, void *stream);

/* The gate of an MoE layer in one launch: logits [tokens, experts] contiguous of logits_dtype (DGA_DT_FP32 / BF16 / FP16; the 16-bit
 * types convert exactly) -> scores fp32 [tokens, experts], ids int32 [tokens, k], weights fp32 [tokens, k]; every element of the three is
 * written.  ids is what dga_route_slots takes as keys (key_stride_bytes 4, pair t * k + j), weights what dga_combine_rows and the
 * gathering quantiser's row_scale take, scores what dga_router_topk_backward and a balance loss read.  Two contracts:
 *  (1) scores, against float64.  DGA_ROUTER_SOFTMAX: m = max x (exact), e_i = exp(x_i - m), p_i = e_i / sum e,
 *      |p - p64| <= (experts + 128) 2^-24 p64 where |x_i - m| <= 16.  DGA_ROUTER_SIGMOID: s = 1 / (1 + exp(-x)),
 *      |s - s64| <= 2^-18 s64 where |x| <= 16.  A row that holds a NaN or +inf, or nothing but -inf, may give NaN scores and weights.
 *  (2) ids and weights are exact fp32 functions of the scores written, which a host reference in float32 reproduces bit for bit:
 *      sel_i = fl32(scores_i + bias_i) (bias fp32 [experts], selection only; NULL: sel_i = scores_i); a NaN sel counts as -inf.
 *      Comparisons are IEEE >: equal values (+0 and -0 too) tie, and the lower index wins.  n_groups > 1 (DeepSeek-V3's group-limited
 *      routing): the experts form n_groups consecutive groups; a group's value is fl32(largest sel + second largest sel) of the group
 *      (a NaN value counts as -inf); the topk_groups groups of largest value stay, ties to the lower group; no expert of another group is
 *      chosen.  ids[t, 0 .. k-1] = the k largest sel among the experts that may be chosen, in descending order, ties to the lower index:
 *      always k distinct values in [0, experts), whatever the logits hold.  r_j = scores[t, ids[t, j]] (no bias in a weight).
 *      DGA_ROUTER_RENORMALIZE: D = ((r_0 + r_1) + ...) + r_{k-1} in that order, w_j = fl32(fl32(r_j / D) * scale), the division
 *      correctly rounded; else w_j = fl32(r_j * scale).
 * One wave per token, the row in registers, wave reductions only: no LDS, no atomics, nothing read back -- capturable.  It moves
 * experts * (input bytes + 4) + 8 k bytes per token, once.
 * DGA_E_SHAPE: a negative size, k < 1, k > experts, n_groups < 1, experts % n_groups != 0, topk_groups outside [1, n_groups],
 * topk_groups * (experts / n_groups) < k, n_groups > 1 with groups of one expert;  tokens == 0 is DGA_OK with nothing touched;  then
 * DGA_E_NULL (logits, ids, weights, scores), DGA_E_DTYPE, and DGA_E_RANGE for experts > DGA_ROUTER_MAX_EXPERTS, k > DGA_ROUTER_MAX_TOPK,
 * an unknown score_func or flag, or more tokens than one grid holds (4 (2^31 - 1)). */
enum { DGA_ROUTER_SOFTMAX = 0, DGA_ROUTER_SIGMOID = 1 };   /* score_func */
#define DGA_ROUTER_RENORMALIZE 1                           /* flags */
#define DGA_ROUTER_MAX_EXPERTS 1024
#define DGA_ROUTER_MAX_TOPK 64
int dga_router_topk(const void *logits, int logits_dtype, int64_t tokens, int64_t experts, int64_t k, int score_func, const float *bias,
                    int64_t n_groups, int64_t topk_groups, int flags, float scale, int32_t *ids, float *weights, float *scores,
                    void *stream);

/* The backward of dga_router_topk: dw fp32 [tokens, k] (dga_combine_rows_weight_grad's output), scores and ids as the forward wrote them
 * -> dlogits [tokens, experts] of dlogits_dtype (DGA_DT_FP32, or a 16-bit type rounded to nearest even); every element is written.  The
 * bias and the choice of groups get no gradient.  r_j = scores[t, ids[t, j]], D and w_j as in the forward,
 *   g_j = (scale dw_j - sum_l dw_l w_l) / D   (DGA_ROUTER_RENORMALIZE;  else g_j = scale dw_j),   ds_i = g_j at i = ids[t, j], else 0
 *   DGA_ROUTER_SIGMOID: dlogits_i = ds_i s_i (1 - s_i), +0 off the selection;   DGA_ROUTER_SOFTMAX: dlogits_i = s_i (ds_i - sum_l ds_l s_l).
 * fp32 in a fixed order, no floating-point atomics: two runs give the same bits.  Against float64 on the same fp32 scores:
 * |dlogits - ref64| <= (experts + k + 8) 2^-24 M, M the same expression with every term replaced by its absolute value and (1 - s_i) by 1.
 * An id outside [0, experts) reads nothing and contributes nothing.  Checks as in dga_router_topk (no group conditions; DGA_E_NULL: dw,
 * scores, ids, dlogits). */
int dga_router_topk_backward(const float *dw, const float *scores, const int32_t *ids, int64_t tokens, int64_t experts, int64_t k,
                             int score_func, int flags, float scale, void *dlogits, int dlogits_dtype, void *stream);

/* The load-balancing loss of a router over dga_router_topk's outputs: scores fp32 [tokens, experts] and ids int32 [tokens, k], both
 * contiguous; the tokens form B = tokens / seq_len segments of seq_len consecutive tokens (seq_len = tokens: Switch / GShard's global
 * loss; seq_len = a sequence: DeepSeek-V3's sequence-wise loss).  For segment b, with u = 2^-24 and gamma(n) = n u / (1 - n u):
 *   counts[b, e] = #{(t, j) : t in b, ids[t, j] == e}                   int32 [B, experts], exact; an id outside [0, experts) counts nowhere
 *   p[t, e]      = scores[t, e] / S_t, S_t = sum_e scores[t, e]         (DGA_ROUTER_BALANCE_NORMALIZE;  else p = scores)
 *   psum[b, e]   = sum_{t in b} p[t, e]                                 fp32 [B, experts], |psum - P64| <= gamma(seq_len + experts + 1) P64
 *   loss[b]      = coef * sum_e counts[b, e] * psum[b, e]               fp32 [B], |loss - loss64| <= gamma(seq_len + 2 experts + 4) loss64
 * against float64 on the same fp32 scores (scores >= 0).  coef is the caller's: alpha * experts / (k seq_len^2) gives
 * alpha sum_e f_e P_e with f_e = experts / (k seq_len) counts and P_e = psum / seq_len.  Every element of the three outputs is written.
 * A NaN score makes its own segment's psum (that expert's) and loss NaN and touches no other segment.  Two launches, no floating-point
 * atomics, nothing read back (capturable): a workgroup adds a chunk of max(16, 4 ceil(tokens / 2048)) consecutive tokens of one segment
 * into a partial of the workspace, fp32 and int32 [B, chunks, experts] with chunks = ceil(seq_len / that); one workgroup per segment
 * then adds the partials in an order the shape alone fixes, so two runs give the same bits.  The callee never allocates:
 * dga_router_balance_loss_workspace_bytes gives the size, 8 B chunks experts (0 for a shape the entry refuses or an empty one).
 * DGA_E_SHAPE: a negative size, k < 1, k > experts, seq_len < 1, tokens % seq_len != 0;  tokens == 0 is DGA_OK with nothing touched;
 * then DGA_E_NULL (scores, ids, loss, counts, psum, workspace), and DGA_E_RANGE for experts > DGA_ROUTER_MAX_EXPERTS,
 * k > DGA_ROUTER_MAX_TOPK, an unknown flag, more than 2^31 - 1 partials, or a workspace that is too small or not 4-byte aligned. */
#define DGA_ROUTER_BALANCE_NORMALIZE 1                     /* flags */
size_t dga_router_balance_loss_workspace_bytes(int64_t tokens, int64_t experts, int64_t seq_len);
int dga_router_balance_loss(const float *scores, const int32_t *ids, int64_t tokens, int64_t experts, int64_t k, int64_t seq_len, int flags,
                            float coef, float *loss, int32_t *counts, float *psum, void *workspace, size_t workspace_bytes, void *stream);

/* The backward of dga_router_balance_loss into the logits: dloss fp32 [B], counts and scores as above (the counts carry no gradient) ->
 * dlogits [tokens, experts] of dlogits_dtype (DGA_DT_FP32, or a 16-bit type rounded to nearest even); every element is written.  For a
 * token t of segment b, in fp32, every operation rounded on its own:
 *   q_e  = fl(fl(dloss[b] * coef) * fl(counts[b, e]))
 *   ds_i = (q_i - sum_e q_e p_e) / S_t   (DGA_ROUTER_BALANCE_NORMALIZE;  else ds_i = q_i)
 *   DGA_ROUTER_SIGMOID: aux_i = ds_i s_i (1 - s_i);   DGA_ROUTER_SOFTMAX: aux_i = s_i (ds_i - sum_e ds_e s_e)
 * |aux - ref64| <= gamma(4 experts + 8) M against float64 on the same inputs, M the same expression with every term replaced by its
 * absolute value and (1 - s_i) by 1.  add_to (fp32 [tokens, experts] or NULL; it may be dlogits itself): the result is
 * fl(add_to + aux), bit for bit the sum of add_to and what the entry writes as fp32 without it -- dga_router_topk_backward's output
 * becomes the step's whole dlogits without another pass.  One wave per token, fixed order, no atomics: two runs give the same bits.
 * Checks as in dga_router_balance_loss (DGA_E_NULL: dloss, counts, scores, dlogits; then DGA_E_DTYPE; DGA_E_RANGE also for an unknown
 * score_func and for more tokens than one grid holds). */
int dga_router_balance_loss_backward(const float *dloss, const int32_t *counts, const float *scores, int64_t tokens, int64_t experts, int64_t k,
                                     int64_t seq_len, int score_func, int flags, float coef, const float *add_to, void *dlogits,
                                     int dlogits_dtype, void *stream);

/* DeepSeek-V3's auxiliary-loss-free balancing step, in place on bias fp32 [experts] (what dga_router_topk adds for the selection), from
 * counts int32 [segments, experts]:  n_e = sum_b counts[b, e] (int64),  sgn_e = sign(sum_e' n_e' - experts * n_e), compared as integers --
 * +1 for an expert below the mean load, -1 above, 0 exactly at it --,  bias[e] = fl(bias[e] + fl(rate * sgn_e)).  A host reference in
 * float32 reproduces it bit for bit.  One launch of one workgroup, capturable.  DGA_E_SHAPE: a negative size;  segments == 0 or
 * experts == 0 is DGA_OK with nothing touched;  then DGA_E_NULL (bias, counts) and DGA_E_RANGE for experts > DGA_ROUTER_MAX_EXPERTS. */
int dga_router_bias_update(float *bias, const int32_t *counts, int64_t segments, int64_t experts, float rate, void *stream);

/* The norm in front of an MoE block fused into the quantiser of everything that reads it: n = rms_norm(x + residual) * weight and
 * per-token 1x128 codes of n in one pass over the row (csrc/dga_rms_norm.hip).  x and residual (or NULL) [rows, h] contiguous of x_dtype
 * (DGA_DT_FP32 / BF16 / FP16; T below), weight [h] of w_dtype = x_dtype or DGA_DT_FP32, 1 <= h <= DGA_RMS_NORM_MAX_H, eps >= 0 finite.
 * Per row, every operation in fp32 and rounded on its own (fl):
 *   z[i]            = x[i]                                       without residual;
 *   residual_out[i] = RNE_T(fl(x[i] + residual[i])),  z[i] = that stored value     with it (residual_out may be residual or x)
 *   rstd            ~ (mean(z^2) + eps)^(-1/2),  |rstd - exact| <= (h / 2 + 6) 2^-24 exact against float64 on the same z; the sum of
 *                   squares runs in an order that (h, x_dtype) alone fixes -- never the row count, the row's place or an atomic
 *   y[i]            = fl(fl(z[i] * rstd) * weight[i]), a NaN replaced by the one NaN 0x7FC00000;  norm_out[i] = RNE_T(y[i])
 *   (q, sf)         = what dga_cast_to_fp8_1x128_ex gives on the fp32 tensor y with the same flags, byte for byte and bit for bit;
 *                   y is never rounded to 16 bits in front of the quantiser
 * everything below rstd an exact function of the rstd [rows] fp32 the call returns (always written).  Nothing is rescaled: where the
 * squares overflow rstd = 0 and y = +-0 (NaN at an infinite z), as in an fp32 torch expression; a NaN in a row makes that row's rstd NaN
 * and its codes 0x7F, and touches no other row; subnormals are kept.  q and sf are both given or both NULL; one of (q, sf) and norm_out must
 * be given (norm_out alone: a plain fused add + RMSNorm); residual_out is given iff residual is.  One launch, nothing read back
 * (capturable).  Checks, in dga_cast_to_fp8_1x128_ex's order: DGA_E_RANGE: an unknown flag;  DGA_E_SHAPE: a negative size,
 * h > DGA_RMS_NORM_MAX_H (the row no longer fits in registers);  rows == 0 or h == 0 is DGA_OK with nothing launched;  then DGA_E_NULL
 * (x, weight, rstd, and the pairings above), DGA_E_DTYPE, and DGA_E_RANGE for a negative, NaN or infinite eps and for more rows than one
 * grid holds. */
#define DGA_RMS_NORM_MAX_H 16384
int dga_rms_norm_cast_to_fp8_1x128(const void *x, const void *residual, int x_dtype, const void *weight, int w_dtype, int64_t rows, int64_t h,
                                   float eps, void *q, float *sf, void *norm_out, void *residual_out, float *rstd, int flags, void *stream);

/* Its backward.  grad_y and z [rows, h] contiguous of dtype, z what the forward normalised (x, or residual_out), weight as above, rstd the
 * forward's own output.  With x^ = fl(z rstd), g = fl(grad_y w), c = fl(sum_i g_i x^_i / h), all in fp32:
 *   dx[t, i]   = fl(rstd * fl(g_i - fl(x^_i c)))                  dx_dtype = dtype or DGA_DT_FP32; the 16-bit dx is RNE of the fp32 one
 *   dweight[j] = sum_t grad_y[t, j] x^[t, j]                      fp32 [h], overwritten; NULL: not computed
 * grad_residual (NULL, or [rows, h] of dx_dtype; it may be dx itself): dx = RNE(fl(dx + grad_residual)), bit for bit the separate sum.
 * Against float64 on the same inputs with rstd as given, u = 2^-24, A = sum_i |g_i x^_i| / h:
 *   |dx - exact| <= u rstd (4 |g| + |x^| (6 |c| + (h + 8) A))   (fp32 dx),     |dweight[j] - exact| <= (rows + 4) u sum_t |grad_y x^|.
 * Every sum runs in an order (rows, h, dtype) alone fixes, without floating-point atomics: two runs give the same bits, and a row's dx
 * does not depend on where the row sits.  dweight takes two launches: groups of lanes add chunks of max(8, ceil(rows / 1024)) consecutive
 * rows into the workspace, fp32 [chunks, h]; a second kernel adds a column's partials in ascending order (four runs, then the runs).
 * dga_rms_norm_backward_workspace_bytes gives the size (0 for a shape the entry refuses or an empty one); the workspace is needed only
 * with dweight.  DGA_E_SHAPE: a negative size, h > DGA_RMS_NORM_MAX_H;  rows == 0 or h == 0 is DGA_OK with nothing launched;  then
 * DGA_E_NULL (grad_y, z, weight, rstd, dx; workspace with dweight), DGA_E_DTYPE, DGA_E_RANGE for more rows than one grid holds, and
 * DGA_E_WORKSPACE for a workspace that is too small or not 16-byte aligned. */
int dga_rms_norm_backward(const void *grad_y, const void *z, int dtype, const void *weight, int w_dtype, const float *rstd,
                          const void *grad_residual, int64_t rows, int64_t h, void *dx, int dx_dtype, float *dweight, void *workspace,
                          int64_t workspace_bytes, void *stream);
int64_t dga_rms_norm_backward_workspace_bytes(int64_t rows, int64_t h);

/* The scoring kernel of the lightning indexer of DeepSeek sparse attention, upstream DeepGEMM's fp8_mqa_logits (csrc/dga_mqa_logits.hip):
 *   s[m,h,n]     = sum_d q[m,h,d] k[n,d]                                          e4m3 codes, d < head_dim = 128
 *   logits[m,n]  = kscale[n] * sum_h weights[m,h] * max(s[m,h,n], 0)               for lo[m] <= n < hi[m]
 *                = -inf                                                            elsewhere
 * q [m, heads, 128] and k [n, 128] contiguous e4m3fn codes (q carries no scale: the caller folds it into weights, as upstream), kscale
 * fp32 [n], weights fp32 [m, heads], ks and ke int32 [m] on the device, logits fp32 [m, n] contiguous.  lo = min(max(ks, 0), n) and hi
 * likewise of ke are formed on the device, so a captured graph follows new ranges; hi <= lo is a row of -inf.  Every element of logits is
 * written on every call, by exactly one lane and without atomics: two runs give the same bits, and logits needs no pre-fill.
 * Arithmetic (the default policy's): the codes go to bf16 exactly, s is four chained v_mfma_f32_16x16x32_bf16 over d ascending in fp32,
 * the ReLU is s < 0 ? 0 : s on that fp32 value (a NaN stays one), each product weights * relu(s) enters an fp32 fused multiply-add chain,
 * the head sum runs in an order heads alone fixes ("Sparse-attention indexer"), kscale multiplies once after it.  Against the exact value, on every
 * element inside its range:
 *   |logits - exact| <= (2^-22 + (heads + 3) 2^-24) kscale[n] sum_h |weights[m,h]| sum_d |q[m,h,d] k[n,d]|.
 * A NaN code (0x7F, 0xFF) in q[m,h,:] makes every in-range element of row m NaN, one in k[n,:] every in-range element of column n;
 * elements outside the ranges are -inf whatever the operands hold.  A (token, block of DGA_MQA_LOGITS_BLOCK_N keys) pair whose keys lie
 * wholly outside the token's range is neither loaded nor multiplied.  No row of k or kscale at or beyond n and no row of q, weights, ks
 * or ke at or beyond m is read.  One launch, nothing read back (capturable).
 * DGA_E_SHAPE: m < 0, n < 1, head_dim != 128, heads other than 32 or 64;  m == 0 is DGA_OK with nothing launched;  then DGA_E_NULL (any
 * pointer), DGA_E_ALIGN (q or k not 8-byte, weights not 16-byte, kscale or logits not 4-byte aligned), and DGA_E_RANGE for
 * n > DGA_MQA_LOGITS_MAX_N or more (token run, key block) pairs than one grid holds (2^31 - 1). */
#define DGA_MQA_LOGITS_HEAD_DIM 128
#define DGA_MQA_LOGITS_BLOCK_N 256        /* keys of one workgroup */
#define DGA_MQA_LOGITS_BLOCK_M 64         /* consecutive tokens one workgroup walks */
#define DGA_MQA_LOGITS_MAX_N 0x7FFFFF00
int dga_fp8_mqa_logits(const void *q, const void *k, const float *kscale, const float *weights, const int32_t *ks, const int32_t *ke,
                       int64_t m, int64_t n, int heads, int head_dim, float *logits, void *stream);

/* The decode half of that scoring, upstream DeepGEMM's fp8_paged_mqa_logits (csrc/dga_paged_mqa_logits.hip): each of `batch` sequences
 * scores its next_n (1 or 2) newest tokens against its whole context, whose keys live in a paged cache reached through a block table.
 *   kv_cache      block b is DGA_PAGED_MQA_LOGITS_BLOCK_BYTES = 8448 bytes at b * block_stride: bytes 0 .. 8191 the e4m3 codes of its
 *                 DGA_PAGED_MQA_LOGITS_BLOCK_KV = 64 keys, key-major (64 x 128), bytes 8192 .. 8447 their 64 fp32 scales (upstream's fused
 *                 layout: codes first, then scales).  block_stride >= 8448 and a multiple of 16, the base 16-byte aligned, num_blocks >= 1.
 *   q             [batch, next_n, heads, 128] contiguous e4m3fn codes, no scale;  weights fp32 [batch next_n, heads]
 *   context_lens  int32 [batch], block_tables int32 [batch, max_blocks] (max_blocks >= 1), both on the device and read there, so a
 *                 captured graph follows new lengths and tables
 *   logits        fp32 [batch next_n, max_model_len] contiguous
 *   ctx_i        = min(max(context_lens[i], 0), max_model_len, 64 max_blocks)
 *   hi_r         = max(ctx_i - next_n + j + 1, 0)                                       row r = i next_n + j, j < next_n
 *   key n of sequence i = key n % 64 of block block_tables[i, n / 64]
 *   logits[r,n]  = kscale * sum_h weights[r,h] * max(sum_d q[i,j,h,d] k[d], 0)          for n < hi_r
 *                = -inf                                                                  for hi_r <= n < max_model_len
 * A table entry is read only for pages p < ceil(ctx_i / 64); the others may hold anything.  An entry of a needed page outside
 * [0, num_blocks) dereferences nothing: that page's columns are -inf in the sequence's rows.  Two sequences may name the same block.
 * clean_logits != 0: every element of logits is written on every call.  clean_logits == 0: the rows of sequence i are written only in
 * columns n < min(64 ceil(ctx_i / 64), max_model_len) -- values below hi_r, -inf from there -- and no byte at or beyond that column is
 * touched.  The arithmetic, the order of the head sum and the bound are dga_fp8_mqa_logits': with kg / sg the keys and scales gathered
 * through a sequence's table, its rows are bit for bit dga_fp8_mqa_logits(q[i], kg, sg, weights[rows], ks = 0, ke = hi_r) in the columns
 * below ctx_i.  No atomics, one writer per element, two runs give the same bits; a NaN code in a key poisons its column in every
 * sequence whose table names the block, one in q[i, j] row r, inside the ranges only.  A workgroup owns one sequence and
 * DGA_PAGED_MQA_LOGITS_CHUNK_N columns; the grid, batch x ceil(max_model_len / CHUNK_N), depends on the shapes alone and no workgroup
 * waits for another, so there is no scheduling table to pass (upstream's schedule_metadata has no counterpart).  No byte outside a
 * named block's 8448 is read, and no row of q / weights / context_lens / block_tables at or beyond batch.  One launch (capturable).
 * DGA_E_SHAPE: batch < 0, next_n other than 1 or 2, heads other than 32 or 64, head_dim != 128, num_blocks < 1, block_stride < 8448,
 * max_blocks < 1, max_model_len < 1;  batch == 0 is DGA_OK with nothing launched and no pointer looked at;  then DGA_E_NULL (any pointer),
 * DGA_E_ALIGN (q not 8-byte, kv_cache or weights not 16-byte, the others not 4-byte aligned, block_stride not a multiple of 16), and
 * DGA_E_RANGE for max_model_len > DGA_PAGED_MQA_LOGITS_MAX_N, a cache, table or output whose size leaves int64, or more workgroups than
 * one grid holds (2^31 - 1). */
#define DGA_PAGED_MQA_LOGITS_BLOCK_KV 64          /* keys of a block of the cache */
#define DGA_PAGED_MQA_LOGITS_BLOCK_BYTES 8448     /* 64 * 128 codes + 64 fp32 scales */
#define DGA_PAGED_MQA_LOGITS_CHUNK_N 512          /* columns of one workgroup */
#define DGA_PAGED_MQA_LOGITS_MAX_N 0x7FFFFC00
int dga_fp8_paged_mqa_logits(const void *q, const void *kv_cache, const float *weights, const int32_t *context_lens,
                             const int32_t *block_tables, int64_t batch, int next_n, int heads, int head_dim, int64_t num_blocks,
                             int64_t block_stride, int64_t max_blocks, int64_t max_model_len, int clean_logits, float *logits, void *stream);

/* The writer of that cache (csrc/dga_cast_paged.hip): x [tokens, 128] of x_dtype (DGA_DT_FP32 / _BF16 / _FP16) contiguous, slot_mapping
 * int64 [tokens] on the device.  Token t with 0 <= slot_mapping[t] < 64 num_blocks: its 128 codes go to bytes 128 (slot % 64) .. of block
 * slot / 64 and its scale to bytes 8192 + 4 (slot % 64) .. of that block -- dga_cast_to_fp8_1x128_ex(x, flags)'s codes and scale of row t,
 * byte for byte.  Any other slot value (-1 on padding) skips the token: its row is not read and nothing is dereferenced.  No other byte of the
 * cache is touched.  Two tokens with one valid slot are the caller's error (each byte is then one writer's).  flags: DGA_CAST_UE8M0.
 * The quantisers' order of checks: DGA_E_RANGE (flag), DGA_E_SHAPE (tokens < 0, num_blocks < 1, block_stride < 8448), tokens == 0 ->
 * DGA_OK with nothing launched, DGA_E_NULL, DGA_E_DTYPE, DGA_E_ALIGN (x or kv_cache not 16-byte, slot_mapping not 8-byte aligned,
 * block_stride not a multiple of 16), DGA_E_RANGE (the cache's size leaves int64, the grid).  One launch (capturable). */
int dga_cast_to_fp8_1x128_paged(const void *x, int x_dtype, int64_t tokens, void *kv_cache, int64_t num_blocks, int64_t block_stride,
                                const int64_t *slot_mapping, int flags, void *stream);

/* The selecting half of the indexer (csrc/dga_indexer_topk.hip): per row of the logits of dga_fp8_mqa_logits / dga_fp8_paged_mqa_logits,
 * the indices of the k highest-scoring columns inside the row's range, in ascending column order.
 *   logits        fp32 [m, n], the last dimension contiguous, rows `stride` elements apart (stride >= n: a column slice of a wider
 *                 buffer is accepted), 4-byte aligned;  out int32 [m, k] contiguous, every element written at every call
 *   [lo, hi) of row r, formed on the device from exactly one of
 *     row_starts, row_ends  int32 [m] (both or neither): lo = min(max(ks[r], 0), n), hi = min(max(ke[r], 0), n); hi <= lo: an empty row
 *     context_lens          int32 [m / next_n], next_n 1 or 2: ctx = min(max(context_lens[r / next_n], 0), n), lo = 0,
 *                           hi = max(ctx - next_n + r % next_n + 1, 0)  (dga_fp8_paged_mqa_logits' rule)
 *     neither               lo = 0, hi = n
 *   key(x)        = bits(x) ^ (bits(x) >> 31 ? 0xFFFFFFFF : 0x80000000) as uint32, every NaN 0xFFFFFFFF (above +inf; -0 below +0)
 *   order         column a precedes column b iff key is greater, or key is equal and a < b  (total)
 *   c = min(hi - lo, k);  out[r, 0 .. c) = the first c columns of [lo, hi) in that order, sorted ascending by column, then mapped;
 *   out[r, c .. k) = -1
 *   mapping of a selected column col: col itself;  relative != 0: col - lo;  block_tables int32 [m / next_n, max_blocks] (lengths form
 *   only, page_size >= 1, num_blocks page_size < 2^31): block_tables[r / next_n, col / page_size] * page_size + col % page_size, and -1 where
 *   col / page_size >= max_blocks or the entry lies outside [0, num_blocks).  Entries of unselected columns are not read.
 * Membership is by column, never by value: an in-range -inf is a candidate.  No byte of logits outside [lo, hi) is read -- a buffer that
 * dga_fp8_paged_mqa_logits left unwritten beyond a sequence's last page (clean_logits == 0) is valid input -- and a row with
 * hi - lo <= k reads no logits at all.  The result is a pure function of the in-range bits: two runs give the same bytes.
 * One workgroup owns one row (a radix select on key in LDS, then one ordered pass that writes; no workgroup waits for another, no
 * atomics on global memory); a bin that fits DGA_INDEXER_TOPK_CANDIDATES keys is finished inside LDS.  One launch (capturable), and a
 * captured graph follows new ranges, lengths and tables.
 * Checks, all before the launch: DGA_E_SHAPE (m < 0, n < 1, stride < n);  m == 0 -> DGA_OK with nothing touched;  DGA_E_NULL (logits,
 * out, one of row_starts / row_ends without the other);  DGA_E_ALIGN (a pointer not 4-byte aligned);  DGA_E_RANGE (k outside
 * [1, DGA_INDEXER_TOPK_MAX_K], n > DGA_INDEXER_TOPK_MAX_N, m >= 2^31, ranges beside lengths, relative beside block_tables, block_tables
 * without context_lens, next_n other than 1 or 2, page_size / max_blocks / num_blocks < 1, num_blocks page_size >= 2^31, m stride or
 * the table's size beyond int64);  DGA_E_SHAPE for m not a multiple of next_n. */
#define DGA_INDEXER_TOPK_MAX_K 2048
#define DGA_INDEXER_TOPK_CANDIDATES 8192          /* keys of the LDS candidate buffer */
#define DGA_INDEXER_TOPK_MAX_N 0x7FFF0000
int dga_indexer_topk(const float *logits, int64_t m, int64_t n, int64_t stride, int k, const int32_t *row_starts, const int32_t *row_ends,
                     const int32_t *context_lens, int next_n, int relative, const int32_t *block_tables, int64_t max_blocks, int page_size,
                     int64_t num_blocks, int32_t *out, void *stream);

/* What the indexer selects for (csrc/dga_sparse_mla.hip): sparse MLA attention, forward, in MLA's absorbed (MQA) form -- every kv row is
 * key (all 576 columns: 512 latent + 64 rope) and value (its first 512 columns) of every head.
 *   q             bf16 [m, heads, 576] contiguous, 16-byte aligned; heads a multiple of 16 in [16, DGA_SPARSE_MLA_MAX_HEADS]
 *   kv            bf16 [s, 576], rows kv_stride elements apart (kv_stride >= 576 and a multiple of 8), 16-byte aligned, 1 <= s < 2^31:
 *                 a flat view of a paged bf16 latent cache, which dga_indexer_topk's physical slots index directly
 *   indices       int32 [m, topk], rows idx_stride elements apart (idx_stride >= topk >= 1: a column slice of a wider tensor is accepted)
 *   index_offsets int32 [m] or NULL: the kv row of position j of token t is r = indices[t, j] + index_offsets[t]
 *                 (dga_fp8_mqa_logits' row_starts beside dga_indexer_topk(relative))
 *   a position is valid iff indices[t, j] >= 0 and 0 <= r < s; an invalid one (the -1 padding, any other negative, anything >= s)
 *   dereferences nothing and contributes nothing; duplicates count once per position; no other kv row and no column >= 576 is read
 *   over the valid positions:  s_j = sm_scale sum_d q[t, h, d] kv[r_j, d];  lse[t, h] = ln sum_j exp(s_j)  (fp32 [m, heads]);
 *   out[t, h, :] = sum_j exp(s_j - lse) kv[r_j, :512]  (bf16 [m, heads, 512], 16-byte aligned)
 *   a token without a valid position: out = +0, lse = -inf.  Every element of out and lse is written at every call.
 * Arithmetic: the bf16 products exact, summed in fp32 by v_mfma_f32_16x16x32_bf16 over d ascending, times (float)(sm_scale log2 e) -- the
 * one rounding of the scale, which is why it arrives as a double; an online softmax over tiles of
 * DGA_SPARSE_MLA_TILE positions in list order (running maximum, and a running sum l of the unrounded fp32 weights p); p rounded to bf16
 * (RNE) for the second product, its sums fp32 in list order; one multiplication by 1 / l at the end.  One writer per output, no
 * atomics: two runs give the same bits.  One launch (capturable); a captured graph follows new indices, offsets, kv and q.
 * flags: DGA_SPARSE_MLA_LINEAR_GRID takes the workgroups in grid order (the default walks consecutive tokens on one XCD); same bits.
 * Checks, all before the launch: DGA_E_RANGE (an unknown flag);  DGA_E_SHAPE (m < 0, heads, s < 1, topk < 1, kv_stride < 576,
 * idx_stride < topk);  m == 0 -> DGA_OK with nothing touched;  DGA_E_NULL (q, kv, indices, out, lse);  DGA_E_ALIGN (q, kv or out not
 * 16-byte, indices, index_offsets or lse not 4-byte aligned, kv_stride not a multiple of 8);  DGA_E_RANGE (s >= 2^31, topk or the grid
 * beyond int32, s kv_stride or m idx_stride beyond int64). */
#define DGA_SPARSE_MLA_D_QK 576
#define DGA_SPARSE_MLA_D_V 512
#define DGA_SPARSE_MLA_MAX_HEADS 128
#define DGA_SPARSE_MLA_TILE 32
#define DGA_SPARSE_MLA_LINEAR_GRID 1
int dga_sparse_mla_fwd(const void *q, const void *kv, const int32_t *indices, const int32_t *index_offsets, int64_t m, int heads, int64_t s,
                       int64_t kv_stride, int64_t topk, int64_t idx_stride, double sm_scale, int flags, void *out, float *lse, void *stream);

/* The same over a paged fp8 latent cache, read in place (csrc/dga_sparse_mla.hip, the same kernel text instantiated on the cache).  A row
 * is DGA_SPARSE_MLA_FP8_ROW_BYTES = 656 bytes (FlashMLA's layout of this model's cache):
 *   bytes 0 .. 511     512 OCP e4m3fn codes of the latent part
 *   bytes 512 .. 527   4 fp32 scales, one per 128 codes
 *   bytes 528 .. 655   64 bf16 values, the rope part, not quantised
 * and row r, 0 <= r < s = num_blocks page_size, lives at byte (r / page_size) block_stride + (r % page_size) 656 of kv_cache (16-byte
 * aligned; block_stride a multiple of 16 and >= 656 page_size; any page_size >= 1 -- page_size 1 is a flat [s, 656] array with rows
 * block_stride apart).  The value a row stands for is defined on the bits:
 *   deq[r, d] = RNE_bf16(fl32(e4m3(code[r, d]) scale[r, d / 128])), d < 512: the code converted exactly, one fp32 multiplication and one
 *   rounding to bf16, subnormals kept in both; codes 0x7F / 0xFF are NaN;  deq[r, 512 + i] = the i-th rope value as stored.
 * Contract: dga_sparse_mla_fwd_fp8(kv_cache) is dga_sparse_mla_fwd(deq) -- out and lse byte for byte wherever the latter is not NaN, NaN in
 * exactly the same elements -- so that entry's validity rule, arithmetic, bounds and determinism hold unchanged; every other argument is
 * that entry's.  No byte of an unselected row and no byte between a block's last row and the next block is read.  One launch.
 * Checks, all before the launch, in that entry's order: DGA_E_RANGE (an unknown flag);  DGA_E_SHAPE (m < 0, heads, num_blocks < 1,
 * page_size < 1, topk < 1, block_stride < 656 page_size, idx_stride < topk);  m == 0 -> DGA_OK;  DGA_E_NULL;  DGA_E_ALIGN (q, kv_cache or
 * out not 16-byte, indices, index_offsets or lse not 4-byte aligned, block_stride not a multiple of 16);  DGA_E_RANGE (s >= 2^31, topk or
 * the grid beyond int32, num_blocks block_stride or m idx_stride beyond int64). */
#define DGA_SPARSE_MLA_FP8_ROW_BYTES 656
int dga_sparse_mla_fwd_fp8(const void *q, const void *kv_cache, const int32_t *indices, const int32_t *index_offsets, int64_t m, int heads,
                           int64_t num_blocks, int64_t page_size, int64_t block_stride, int64_t topk, int64_t idx_stride, double sm_scale,
                           int flags, void *out, float *lse, void *stream);

/* Split-topk sparse MLA decode: the same attention as several workgroups a token and a merge (csrc/dga_sparse_mla.hip, the same kernel
 * text; csrc/dga_sparse_mla_merge.hip).  With tiles = ceil(topk / DGA_SPARSE_MLA_TILE) and P = min(num_splits, tiles) splits, split p owns
 * the contiguous tiles [p tiles / P, (p + 1) tiles / P) of every token's list and writes, in fp32 and not rounded to bf16,
 *   partial_out[p, t, h, :] = O (1 / l)  (fp32 [P, m, heads, 512] contiguous, 16-byte aligned)
 *   partial_lse[p, t, h]    = ln sum over the split's valid positions of exp(s_j)  (fp32 [P, m, heads] contiguous)
 * a split without a valid position +0 and -inf.  Every element of both is written at every call, nothing of a split >= P is touched.
 * The grid is m head_blocks P workgroups, the splits of one token and head block adjacent; everything else -- arguments, validity rule,
 * arithmetic per tile, flags -- is dga_sparse_mla_fwd's / dga_sparse_mla_fwd_fp8's, and the fp8 entry's partials are the bf16 entry's on
 * the dequantised rows, byte for byte.  *effective_splits (may be NULL) receives P.
 * Checks: the one-pass entry's, in its order (out and lse apart), with the grid's range counting P;  then DGA_E_RANGE (num_splits < 1 or
 * > DGA_SPARSE_MLA_MAX_SPLITS; num_splits > tiles is clamped to tiles);  DGA_E_NULL (partial_out, partial_lse);  DGA_E_ALIGN (partial_out
 * not 16-byte, partial_lse not 4-byte aligned).  m == 0 -> DGA_OK with nothing touched.
 *
 * dga_sparse_mla_merge: partial_out fp32 [num_splits, m, heads, 512], partial_lse fp32 [num_splits, m, heads] -> out bf16 [m, heads, 512],
 * lse fp32 [m, heads].  Per (t, h), fp32, nothing contracted, p ascending, L2E = (float)log2 e, LN2 = (float)ln 2:
 *   M = fmax_p partial_lse[p] from -inf (a NaN is passed over);  mu = M, or 0 when M = -inf;  w_p = v_exp_f32((partial_lse[p] - mu) L2E);
 *   L = ((w_0 + w_1) + w_2) + ...;  N[c] = ((w_0 po_0[c] + w_1 po_1[c]) + w_2 po_2[c]) + ...;
 *   L == 0 (a NaN is not 0): out = +0, lse = -inf;  else out[c] = RNE_bf16(N[c] (1 / L)), lse = mu + LN2 v_log_f32(L).
 * With num_splits = 1 that is out = RNE_bf16(po) and lse = partial_lse: partial + merge reproduces the one-pass entry byte for byte.
 * One writer per output, no atomics, nothing of a split >= num_splits is read.  One launch; m == 0 returns without one.
 * Checks: DGA_E_SHAPE (m < 0, heads, num_splits outside [1, DGA_SPARSE_MLA_MAX_SPLITS]);  m == 0 -> DGA_OK;  DGA_E_NULL;  DGA_E_ALIGN
 * (partial_out or out not 16-byte, partial_lse or lse not 4-byte aligned);  DGA_E_RANGE (the grid beyond int32, the partials beyond int64).
 *
 * dga_sparse_mla_splits: the number of splits worth launching, max(1, min(cus / (m head_blocks), tiles / DGA_SPARSE_MLA_MIN_TILES,
 * DGA_SPARSE_MLA_MAX_SPLITS)) -- as many as there are idle CUs for, none shorter than DGA_SPARSE_MLA_MIN_TILES tiles.  A pure function;
 * cus <= 0 asks the current device; m, heads or topk < 1 give 1. */
#define DGA_SPARSE_MLA_MAX_SPLITS 64
#define DGA_SPARSE_MLA_MIN_TILES 4
int dga_sparse_mla_fwd_partial(const void *q, const void *kv, const int32_t *indices, const int32_t *index_offsets, int64_t m, int heads,
                               int64_t s, int64_t kv_stride, int64_t topk, int64_t idx_stride, double sm_scale, int flags, int num_splits,
                               int *effective_splits, float *partial_out, float *partial_lse, void *stream);
int dga_sparse_mla_fwd_fp8_partial(const void *q, const void *kv_cache, const int32_t *indices, const int32_t *index_offsets, int64_t m,
                                   int heads, int64_t num_blocks, int64_t page_size, int64_t block_stride, int64_t topk, int64_t idx_stride,
                                   double sm_scale, int flags, int num_splits, int *effective_splits, float *partial_out, float *partial_lse,
                                   void *stream);
int dga_sparse_mla_merge(const float *partial_out, const float *partial_lse, int num_splits, int64_t m, int heads, void *out, float *lse,
                         void *stream);
int dga_sparse_mla_splits(int64_t m, int heads, int64_t topk, int cus);

/* The writer of the paged fp8 latent cache (csrc/dga_cast_mla_paged.hip).  kv_c [tokens, 512] and k_pe [tokens, 64], both of dtype x_dtype (DGA_DT_FP32 /
 * BF16 / FP16), rows ld_c and ld_pe elements apart (>= 512, >= 64; base and row pitch multiples of 16 bytes: two column slices of one
 * [tokens, 576] tensor are valid), slot_mapping int64 [tokens].  For every t with 0 <= slot_mapping[t] < num_blocks page_size, row slot
 * of the cache receives the 512 codes and 4 scales of dga_cast_to_fp8_1x128 on kv_c's row t (flags: DGA_CAST_UE8M0), byte for byte, and
 * RNE_bf16(k_pe[t]) (bf16 input: its bits).  Any other slot value skips the token, whose inputs are not read; no other byte of the cache
 * is written.  Duplicate valid slots are the caller's error.
 * Checks, all before the launch: DGA_E_RANGE (an unknown flag);  DGA_E_SHAPE (tokens < 0, num_blocks < 1, page_size < 1,
 * block_stride < 656 page_size, ld_c < 512, ld_pe < 64);  tokens == 0 -> DGA_OK;  DGA_E_NULL;  DGA_E_DTYPE;  DGA_E_ALIGN;  DGA_E_RANGE
 * (num_blocks page_size >= 2^31, num_blocks block_stride or tokens times a row pitch beyond int64, the grid). */
int dga_cast_mla_kv_to_fp8_paged(const void *kv_c, int64_t ld_c, const void *k_pe, int64_t ld_pe, int x_dtype, int64_t tokens, void *kv_cache,
                                 int64_t num_blocks, int64_t page_size, int64_t block_stride, const int64_t *slot_mapping, int flags,
                                 void *stream);

/* ---- the expert-sharded forward behind the C ABI (csrc/dga_sharded.cpp) ----------------------------------
 * What a C++ host (the reference's host language: framework/csrc/python_api.cpp) calls to run BASELINE configs[4]: expert g
 * lives on rank g / (groups_total / world), one all-to-all of payload rows each way, every shape static, nothing read back.
 * The library computes the buffer layout, the fixed step sequence ("plan") and executes it on the caller's streams; the two
 * collectives are the caller's (a callback), so the library does not link RCCL.  The reference has no counterpart ("multi-card"
 * = independent processes: benchmark_msprof/main.cpp:24-26, framework/benchmark/benchmark.py:249-253). */
typedef struct dga_sharded_shape_t {
    int32_t world, rank;
    int32_t groups_total;     /* experts over all ranks (a multiple of world) */
    int32_t m_max, n, k;      /* rows per expert (capacity), output columns, reduction length */
    int32_t chunks;           /* a rank's experts are processed in this many chunks, whose dispatch / GEMM / combine overlap on
                                 three streams; <= 0: 2 when world > 1 and the experts per rank allow it, else 1 */
    int32_t max_tokens;       /* the largest number of tokens one rank brings to a forward (sizes the exchange slices: the same
                                 on every rank); <= 0: groups_local * m_max */
    float capacity_factor;    /* rows reserved per (chunk, destination rank) = this x the even share, rounded up to 16;
                                 <= 0: the provable bound min(max_tokens, experts per chunk x m_max) */
    int32_t indexed;          /* 1: the GEMM gathers its rows from the receive buffer and scatters results into the buffer that
                                 travels back (no unpack / gather copy); 0: packed masked layout */
    int32_t policy;           /* dispatchPolicyTag of the GEMM (DGA_POLICY_STRICT, DGA_POLICY_BF16_EXACT, ...); -1 = the library's default
                                 arithmetic (dga_default_policy); -3 = the fast policy's tiling | DGA_POLICY_UE8M0_SCALES; -2 = the fast policy's
                                 own tiling, schedule included */
} dga_sharded_shape_t;

/* Payload row of the dispatch exchange: [K fp8 bytes][ceil(K/128) fp32 scales][int32 header = expert index on its owner, -1 =
 * unused row], padded to a multiple of 128 bytes.  Exchange buffers hold chunks x world x pair_capacity rows; a rank sends
 * peer p the rows [c * rows_per_chunk + p * pair_capacity, + pair_capacity) of chunk c (EQUAL splits: a static shape). */
typedef struct dga_sharded_layout_t {
    int32_t groups_local, groups_per_chunk, chunks, kb, nb;
    int32_t indexed;          /* the shape's flag after the limits are applied (32-bit tile offsets, K % 4) */
    int64_t hdr_offset, row_bytes, pair_capacity, rows_per_chunk, rows_total, max_tokens;
    uint64_t send_bytes, recv_bytes;       /* payload rows out / in */
    uint64_t osend_bytes, oback_bytes;     /* bf16 [rows_total, n] result rows out / back */
    uint64_t slot_bytes;                   /* int64 [max_tokens]: slot of every token */
    uint64_t rdest_bytes;                  /* int64 [rows_total]: row of every received row in the masked layout */
    uint64_t row_of_slot_bytes;            /* int64 [groups_local * m_max]: slot -> source row (indexed only) */
    uint64_t pair_cnt_bytes;               /* int32 [chunks * world] */
    uint64_t masked_m_bytes;               /* int32 [groups_local]: rows every local expert received (the GEMM's masked_m) */
    uint64_t packed_a_bytes, packed_sfa_bytes, packed_out_bytes;   /* the masked layout [Gl, m_max, .] (packed path only) */
    int32_t events;           /* events the executor needs (dga_sharded_events_create) */
    int32_t steps;            /* length of the plan */
} dga_sharded_layout_t;

typedef struct dga_sharded_buffers_t {
    void *send, *recv, *osend, *oback;
    int64_t *slot, *rdest, *row_of_slot;
    int32_t *pair_cnt, *masked_m;
    int32_t *overflow;        /* sticky device counter of rows dropped by a full expert / pair slice (the caller reads and clears it) */
    void *packed_a; float *packed_sfa; void *packed_out;
    const void *b;            /* resident weights of this rank: [groups_local, n, k] e4m3fn */
    const float *sfb;         /* [groups_local, ceil(n/128), ceil(k/128)] */
    void *workspace; size_t workspace_bytes;   /* dga_workspace_bytes of the grouped tiling (may be NULL) */
} dga_sharded_buffers_t;

/* Steps of the plan.  stream: 0 = the caller's, 1 = dispatch side stream, 2 = combine side stream. */
enum { DGA_STEP_WAIT_EVENT = 0,          /* stream waits for event */
       DGA_STEP_RECORD_EVENT = 1,        /* event recorded on stream */
       DGA_STEP_CLEAR_HEADERS = 2,       /* header of every send row = -1 */
       DGA_STEP_ROUTE_SOURCE = 3,        /* dga_route_slots on the tokens' expert ids (+ header tags) */
       DGA_STEP_PACK = 4,                /* dga_copy_rows2: token bytes + scales into their slots */
       DGA_STEP_ZERO_COUNTS = 5,         /* masked_m = 0 */
       DGA_STEP_ZERO_DROPPED = 6,        /* result rows of the tokens that found no slot = 0 (nothing else ever writes them) */
       DGA_STEP_ALL_TO_ALL_DISPATCH = 7, /* the callback, direction 0: payload rows of one chunk */
       DGA_STEP_ROUTE_RECEIVED = 8,      /* dga_route_slots keyed by the received headers: masked_m and the row tables */
       DGA_STEP_UNPACK = 9,              /* packed path: received rows into the masked layout */
       DGA_STEP_GEMM = 10,               /* the grouped masked-M GEMM of a chunk's experts */
       DGA_STEP_GATHER_OUT = 11,         /* packed path: result rows into the buffer that travels back */
       DGA_STEP_ALL_TO_ALL_COMBINE = 12, /* the callback, direction 1: bf16 result rows of one chunk */
       DGA_STEP_RESTORE_ORDER = 13,      /* result[t] = returned row slot[t] */
       DGA_STEP_ZERO_UNROUTED = 14 };    /* returning rows of the received rows that found no place in their expert = 0 */
typedef struct dga_sharded_step_t {
    int32_t op, stream, chunk, event;
    int64_t row_begin, rows;             /* slice of the exchange buffers */
    int32_t group_begin, groups;         /* local experts of the step */
} dga_sharded_step_t;

/* The collective: send peer p the `bytes_per_peer` bytes at send + p * bytes_per_peer, receive its slice at recv + p *
 * bytes_per_peer, asynchronously on `stream` (ncclGroupStart; ncclSend/ncclRecv x world; ncclGroupEnd -- or ncclAllToAll).
 * direction 0 = dispatch, 1 = combine.  Returns 0 on success. */
typedef int (*dga_all_to_all_fn)(void *user, int direction, int chunk, const void *send, void *recv, size_t bytes_per_peer,
                                 void *stream);

int dga_sharded_layout(const dga_sharded_shape_t *shape, dga_sharded_layout_t *out);
/* steps == NULL: *count = the plan's length.  Pure host arithmetic (no device is touched). */
int dga_sharded_plan(const dga_sharded_shape_t *shape, dga_sharded_step_t *steps, int capacity, int *count);
/* One forward: tok_q [tokens, k] e4m3fn, tok_sf [tokens, ceil(k/128)] f32, expert_ids int64 [tokens] (global expert of every
 * token), all device memory -> result bf16 [tokens, n] in token order.  streams[3]: hipStream_t (they may all be the same one);
 * events: layout.events handles (dga_sharded_events_create).  Asynchronous; nothing is read back; capturable in a HIP graph.
 * world == 1: no exchange, all_to_all and events may be NULL. */
int dga_sharded_forward(const dga_sharded_shape_t *shape, const dga_sharded_buffers_t *buffers, const void *tok_q,
                        const float *tok_sf, const int64_t *expert_ids, int tokens, void *result, int expected_m,
                        void *const *streams, void *const *events, dga_all_to_all_fn all_to_all, void *user);
/* hipEvent_t handles (timing disabled) for the executor: host objects, no device memory. */
int dga_sharded_events_create(int count, void **events);
int dga_sharded_events_destroy(int count, void **events);

/* ---- diagnostics ------------------------------------------------------------------------- */

/* The shader clock held inside the dense kernel's main loop ("record the measured clock" beside the
 * vendor peak).  Runs `launches` back-to-back launches of the loop-clock build of the kernel `tiling` selects -- the
 * product kernel plus one s_memtime / s_memrealtime pair either side of the k loop -- synchronises `stream`, and returns
 * the median over waves of shader ticks / 100 MHz ticks (clock_mhz) and of the loop's duration (loop_us, nullable).
 * Compiled for the kernels of BASELINE configs[1] / [2] (256x256 continuous, 128x256 3-stage with loader waves); other tilings,
 * split-K, K % 128 != 0: DGA_E_TILING.  scratch: device memory, 16 bytes per wave (128 per tile).  The reference times
 * with msprof from outside (framework/benchmark/benchmark.py:400-418) and has no counterpart. */
int dga_gemm_fp8_loop_clock(const void *a, const float *sfa, const void *b, const float *sfb, void *out, int m, int n,
                            int k, const dga_tiling_t *tiling, void *scratch, size_t scratch_bytes, int launches,
                            void *stream, float *clock_mhz, float *loop_us);

/* What the matrix pipe of this device sustains with the operands already in registers: `launches` back-to-back launches of
 * a loop of the policy's matrix instruction with the fp32 promotion beside it (mode 0: v_mfma_scale_f32_16x16x128_f8f6f4 + 4
 * FMAs -- the fast path; mode 1: 4 chained v_mfma_f32_16x16x32_bf16 + 4 FMAs + 8 e4m3 -> bf16 conversions -- the bf16-exact
 * policy's 64 x 64 wave tile), two waves per SIMD on every CU, random e4m3 bytes; *tflops = the last launch's rate.  The
 * ceiling bench.py prices the product kernels against beside the vendor peak (`roofline.ceiling_tflops`).
 * scratch: device memory, >= 16 KiB + 2 KiB per CU.  A diagnostic (it synchronises); no reference counterpart. */
int dga_mfma_ceiling(int mode, int launches, void *scratch, size_t scratch_bytes, void *stream, float *tflops);

/* ---- misc -------------------------------------------------------------------------------- */
const char *dga_status_string(int status);
int dga_last_hip_error(void);
int dga_abi_version(void);
/* fills coreNum etc. from hipDeviceProp of the current device */
int dga_device_platform(dga_platform_t *out);

#ifdef __cplusplus
}
#endif
#endif /* DGA_HIP_H */
