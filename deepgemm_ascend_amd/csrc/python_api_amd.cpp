// deep_gemm_cpp -- the reference's pybind11 torch extension, rebuilt on the C ABI of libdga_hip.so.
// Same module name and the same three entry points as deep_gemm_ascend/framework/csrc/python_api.cpp:13-36
// (run_mmad_custom / run_mmad_rtc / run_mmad_bench over at::Tensor, void return, output written in place, current device
// stream, synchronous as gemm.hpp:110), plus the fp8 operators of BASELINE.json's north star.  torch types stay on this
// side of the boundary; everything below it is plain pointers and sizes (include/dga_hip.h).
// Layout: the shared check, problem, workspace and output helpers first, then the bindings in their order of registration; a binding
// states its shapes, its C entry and its label, and takes everything else from the helpers.
// Built in-tree by deepgemm_ascend_amd/build_ext.py (hipcc, host code only -- there is no device code in this file).
#include <cstdlib>
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime_api.h>

#include <c10/core/DeviceGuard.h>

#include <initializer_list>
#include <string>
#include <tuple>
#include <vector>

#include "dga_hip.h"

namespace {

using Shape = std::initializer_list<int64_t>;
using OptTensor = c10::optional<at::Tensor>;
using TensorPair = std::tuple<at::Tensor, at::Tensor>;

void check(int rc, const char *what)   // DGA_HOST_ASSERT / DGAException (framework/csrc/utils/exception.hpp:9-33)
{
    TORCH_CHECK(rc == DGA_OK, what, ": ", dga_status_string(rc), rc == DGA_E_HIP ? " (hipError " : "",
                rc == DGA_E_HIP ? std::to_string(dga_last_hip_error()) + ")" : std::string());
}
void *cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }   // gemm.hpp:72: the current device stream
void sync_stream() { TORCH_CHECK(hipStreamSynchronize(static_cast<hipStream_t>(cur_stream())) == hipSuccess, "stream sync"); }
void on_device(const at::Tensor &t, const char *name)
{
    TORCH_CHECK(t.is_cuda(), name, " must live on a HIP device (there is no CPU path)");
    TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}
int dt16(const at::Tensor &t)
{
    TORCH_CHECK(t.scalar_type() == at::kBFloat16 || t.scalar_type() == at::kHalf, "expected bfloat16 / float16");
    return t.scalar_type() == at::kBFloat16 ? DGA_DT_BF16 : DGA_DT_FP16;
}
// The 16-bit / fp32 element types of the quantisers and the combine -> DGA_DT_*
int input_dtype(const at::Tensor &t, const char *name)
{
    const at::ScalarType st = t.scalar_type();
    TORCH_CHECK(st == at::kFloat || st == at::kBFloat16 || st == at::kHalf, name, " must be float32 / bfloat16 / float16");
    return st == at::kFloat ? DGA_DT_FP32 : st == at::kBFloat16 ? DGA_DT_BF16 : DGA_DT_FP16;
}
// caller-owned workspace: the binding plays the op runtime.  Allocate it under the device guard, after the tiling is known
struct Workspace {
    size_t bytes;
    at::Tensor buffer;
    Workspace(const at::Tensor &like, size_t bytes_)
        : bytes(bytes_), buffer(at::empty({static_cast<int64_t>(bytes_ ? bytes_ : 1)}, like.options().dtype(at::kByte))) {}
    void *ptr() const { return bytes ? buffer.data_ptr() : nullptr; }
};
// the arithmetic policy of an fp8 call (api.py ARITHMETIC_POLICIES): strict = true or policy = "strict" -> dispatchPolicyTag 3;
// "bf16_exact" -> 7; "fast" -> whatever schedule the fast tiling names (-1); "fast_ue8m0" -> that schedule | 16 (-2);
// "bf16_exact_ue8m0" -> 7 | 16; "" -> the operator's default: $DGA_DEFAULT_POLICY, else bf16-exact (inside the 2-ULP contract)
int policy_tag(bool strict, const std::string &policy_in)
{
    std::string policy = policy_in;
    if (policy.empty() && !strict) {   // the library's default, parsed and validated once in the C library (dga_default_policy)
        char name[32] = {0};
        TORCH_CHECK(dga_default_policy(name, sizeof name) == DGA_OK, "$DGA_DEFAULT_POLICY names no arithmetic policy");
        policy = name;
        TORCH_CHECK(policy != "auto", "$DGA_DEFAULT_POLICY=auto is a policy of the Python API (deepgemm_ascend_amd.api); name one here");
    }
    TORCH_CHECK(policy.empty() || policy == "fast" || policy == "bf16_exact" || policy == "strict" || policy == "fast_ue8m0" ||
                    policy == "bf16_exact_ue8m0",
                "policy must be one of 'fast', 'bf16_exact', 'strict', 'fast_ue8m0', 'bf16_exact_ue8m0'");
    TORCH_CHECK(!(strict && !policy.empty() && policy != "strict"), "strict=True contradicts policy='", policy, "'");
    if (strict || policy == "strict") return DGA_POLICY_STRICT;
    if (policy == "bf16_exact") return DGA_POLICY_BF16_EXACT;
    if (policy == "bf16_exact_ue8m0") return DGA_POLICY_BF16_EXACT | DGA_POLICY_UE8M0_SCALES;
    if (policy == "fast_ue8m0") return -2;
    return -1;
}
// the problem of every fp8 entry: row-major A, column-major B (NT), row-major C, e4m3 codes
dga_problem_t fp8_problem(int64_t m, int64_t n, int64_t k, int64_t groups, int expected_m = 0, unsigned flags = 0)
{
    dga_problem_t p{};
    p.m = m; p.n = n; p.k = k; p.groups = groups; p.expected_m = expected_m;
    p.layoutTagA = DGA_LAYOUT_ROW_MAJOR; p.layoutTagB = DGA_LAYOUT_COLUMN_MAJOR; p.layoutTagC = DGA_LAYOUT_ROW_MAJOR;
    p.dtype = DGA_DT_FP8_E4M3FN; p.flags = flags;
    return p;
}
dga_tiling_t tiling_for(const dga_problem_t &p, int tag)   // the tiling of a bf16-output call under policy_tag's answer
{
    dga_tiling_t t{};
    if (tag >= 0 && (tag & 7) == DGA_POLICY_BF16_EXACT) {   // that policy's own tile / split-K pick
        check(dga_tiling_bf16_exact(&p, &t), "tiling_bf16_exact");
        t.dispatchPolicyTag = static_cast<uint8_t>(tag);
        return t;
    }
    check(dga_tiling(&p, &t), "tiling");
    if (tag >= 0) t.dispatchPolicyTag = static_cast<uint8_t>(tag);
    if (tag == -2) t.dispatchPolicyTag |= DGA_POLICY_UE8M0_SCALES;
    return t;
}
// Operand checks of the fp8 operators -- the same the ctypes mirror makes (api.py _require): full shapes, dtypes, contiguity,
// one device.  Shapes and dtypes are checked BEFORE the device (so that a host-side test can see them), nothing is launched
// unless every check passed: an undersized out or scale tensor would otherwise be an out-of-bounds device access.
void want_shape(const at::Tensor &t, Shape shape, const char *name)
{
    TORCH_CHECK(t.dim() == static_cast<int64_t>(shape.size()), name, " must have rank ", shape.size(), ", got ", t.dim());
    int64_t i = 0;
    for (int64_t d : shape) {
        TORCH_CHECK(t.size(i) == d, name, " must be ", at::IntArrayRef(shape), ", got ", t.sizes());
        ++i;
    }
}
void want_fp8(const at::Tensor &t, const char *name)
{
    TORCH_CHECK(t.scalar_type() == at::kFloat8_e4m3fn || t.scalar_type() == at::kByte, name,
                " must be float8_e4m3fn or uint8 bytes, got ", t.scalar_type());
}
void want_dtype(const at::Tensor &t, at::ScalarType st, const char *name)
{
    TORCH_CHECK(t.scalar_type() == st, name, " must be ", st, ", got ", t.scalar_type());
}
// ... of the five tensors every fp8 GEMM takes, in the order every binding reports them; a's shape is where the sizes come from
void want_fp8_operands(const at::Tensor &a, const at::Tensor &b, Shape b_shape, const at::Tensor &out, Shape out_shape, at::ScalarType out_dtype,
                       const at::Tensor &sfa, Shape sfa_shape, const at::Tensor &sfb, Shape sfb_shape)
{
    want_fp8(a, "a"); want_fp8(b, "b");
    want_shape(b, b_shape, "b");
    want_shape(out, out_shape, "out"); want_dtype(out, out_dtype, "out");
    want_shape(sfa, sfa_shape, "sfa"); want_dtype(sfa, at::kFloat, "sfa");
    want_shape(sfb, sfb_shape, "sfb"); want_dtype(sfb, at::kFloat, "sfb");
}
// ... of the optional fp32 accumuland c of out's shape (may be out itself) -> what same_device takes: the tensor, or null without one
const at::Tensor *want_c(const OptTensor &c, Shape shape)
{
    if (!c.has_value()) return nullptr;
    want_shape(*c, shape, "c"); want_dtype(*c, at::kFloat, "c");
    return &*c;
}
const float *c_ptr(const at::Tensor *c) { return c ? c->data_ptr<float>() : nullptr; }
void same_device(std::initializer_list<const at::Tensor *> ts)   // (a null entry: an optional tensor that was not given)
{
    const at::Tensor *first = *ts.begin();
    for (const at::Tensor *t : ts) {
        if (!t) continue;
        on_device(*t, "operand");
        TORCH_CHECK(t->device() == first->device(), "all operands must live on one device");
    }
}
// An optional side tensor of a quantiser or combine binding, which check the device first: on a device and contiguous, then what
// `ok` asks of it (`what`: the tensor's one message for that), then on `like`'s device -> its data, or null without one
template <typename Ok>
void *side_tensor(const OptTensor &t, const char *name, const at::Tensor &like, Ok ok, const char *what)
{
    if (!t.has_value()) return nullptr;
    on_device(*t, name);
    TORCH_CHECK(ok(*t), what);
    TORCH_CHECK(t->device() == like.device(), "all tensors must live on one device");
    return t->data_ptr();
}
// (qt [H, T], sft [H, ceil(T/128)]): what the quantisers of a transpose return
TensorPair transposed_outputs(const at::Tensor &like, int64_t h, int64_t t_n)
{
    return {at::empty({h, t_n}, like.options().dtype(at::kFloat8_e4m3fn)), at::empty({h, (t_n + 127) / 128}, like.options().dtype(at::kFloat))};
}

// ---- the reference's three entry points -------------------------------------------------------------------------
void run_mmad_rtc(const at::Tensor &x, const at::Tensor &y, at::Tensor &z)   // gemm.hpp:68-111
{
    on_device(x, "x"); on_device(y, "y"); on_device(z, "z");
    TORCH_CHECK(x.dim() == 3 && y.dim() == 3 && z.dim() == 3 && z.scalar_type() == at::kFloat, "x [B,M,K], y [B,K,N], z [B,M,N] f32");
    const int batch = x.size(0), m = x.size(1), k = y.size(1), n = y.size(2);
    TORCH_CHECK(x.size(2) == k && y.size(0) == batch && z.size(0) == batch && z.size(1) == m && z.size(2) == n, "shape mismatch");
    TORCH_CHECK(x.device() == y.device() && x.device() == z.device(), "all operands must live on one device");
    const c10::OptionalDeviceGuard guard(at::device_of(z));
    const Workspace ws(x, dga_mmad_workspace_bytes(batch, m, n, k, x.data_ptr()));
    check(dga_run_mmad_rtc_ws(x.data_ptr(), y.data_ptr(), z.data_ptr<float>(), batch, m, n, k, dt16(x), ws.ptr(), ws.bytes, cur_stream()),
          "run_mmad_rtc");
    sync_stream();                                                             // gemm.hpp:110
}

void run_mmad_bench(const at::Tensor &x, const at::Tensor &y, at::Tensor &z, at::Tensor &params)   // gemm_bench.hpp:49-113
{
    on_device(x, "x"); on_device(y, "y"); on_device(z, "z");
    TORCH_CHECK(x.dim() == 2 && y.dim() == 2 && z.dim() == 2 && z.scalar_type() == at::kFloat, "x [M,K], y [K,N], z [M,N] f32");
    TORCH_CHECK(params.scalar_type() == at::kInt && params.numel() == 28, "params must be int32[28]");
    const int m = x.size(0), k = y.size(0), n = y.size(1);
    TORCH_CHECK(x.size(1) == k && z.size(0) == m && z.size(1) == n, "shape mismatch");
    TORCH_CHECK(x.device() == y.device() && x.device() == z.device(), "all operands must live on one device");
    const c10::OptionalDeviceGuard guard(at::device_of(z));
    at::Tensor host = params.to(at::kCPU).contiguous();                        // the reference does 6 .item() syncs (:52-57)
    check(dga_bench_params_fill(m, n, k, host.data_ptr<int32_t>()), "bench_params_fill");
    params.copy_(host);                                                        // write-back of slots 6..27 (:68-81)
    const Workspace ws(x, dga_mmad_workspace_bytes(1, m, n, k, x.data_ptr()));
    check(dga_run_mmad_bench_ws(x.data_ptr(), y.data_ptr(), z.data_ptr<float>(), m, n, k, dt16(x), host.data_ptr<int32_t>(), ws.ptr(), ws.bytes,
                                cur_stream()),
          "run_mmad_bench");
    sync_stream();
}

// ---- the fp8 block-scaled operators (names from upstream DeepGEMM) -----------------------------
void gemm_fp8_fp8_bf16_nt(const at::Tensor &a, const at::Tensor &sfa, const at::Tensor &b, const at::Tensor &sfb,
                          at::Tensor &out, bool strict, const std::string &policy)
{
    const int tag = policy_tag(strict, policy);
    TORCH_CHECK(a.dim() == 2 && b.dim() == 2, "a [M,K], b [N,K]");
    const int64_t m = a.size(0), n = b.size(0), k = a.size(1), kb = (k + 127) / 128, nb = (n + 127) / 128;
    want_fp8_operands(a, b, {n, k}, out, {m, n}, at::kBFloat16, sfa, {m, kb}, sfb, {nb, kb});
    same_device({&a, &sfa, &b, &sfb, &out});
    const c10::OptionalDeviceGuard guard(at::device_of(out));   // stream, tiling (CU count) and scratch on the tensors' device
    const dga_tiling_t t = tiling_for(fp8_problem(m, n, k, 1), tag);
    const Workspace ws(out, dga_workspace_bytes(&t));
    check(dga_gemm_fp8_fp8_bf16_nt(a.data_ptr(), sfa.data_ptr<float>(), b.data_ptr(), sfb.data_ptr<float>(), out.data_ptr(),
                                   m, n, k, &t, ws.ptr(), ws.bytes, cur_stream()), "gemm_fp8_fp8_bf16_nt");
}

// What the two dense fp32-output bindings are (fp32_out_entry in dga_launch.hip, _fp32_out_call in api.py): fp32 rows, optional addend c
// (may be out itself), the entry's default tiling; sfb per 128 rows of b, or per row
void dense_fp32_out(const at::Tensor &a, const at::Tensor &sfa, const at::Tensor &b, const at::Tensor &sfb, at::Tensor &out, const OptTensor &c,
                    bool sfb_per_row, decltype(&dga_tiling_fp32_out) tiling, const char *tiling_label,
                    decltype(&dga_gemm_fp8_fp8_fp32_nt) entry, const char *label)
{
    TORCH_CHECK(a.dim() == 2 && b.dim() == 2, "a [M,K], b [N,K]");
    const int64_t m = a.size(0), n = b.size(0), k = a.size(1), kb = (k + 127) / 128;
    want_fp8_operands(a, b, {n, k}, out, {m, n}, at::kFloat, sfa, {m, kb}, sfb, {sfb_per_row ? n : (n + 127) / 128, kb});
    const at::Tensor *addend = want_c(c, {m, n});
    same_device({&a, &sfa, &b, &sfb, &out, addend});
    const c10::OptionalDeviceGuard guard(at::device_of(out));
    const dga_problem_t p = fp8_problem(m, n, k, 1);
    dga_tiling_t t{};
    check(tiling(&p, &t), tiling_label);
    const Workspace ws(out, dga_workspace_bytes(&t));
    check(entry(a.data_ptr(), k, sfa.data_ptr<float>(), b.data_ptr(), k, sfb.data_ptr<float>(), c_ptr(addend), out.data_ptr<float>(), m, n, k, 0,
                &t, ws.ptr(), ws.bytes, cur_stream()),
          label);
}
// sfb [ceil(N/128), KB]: dga_gemm_fp8_fp8_fp32_nt, default tiling (dga_tiling_fp32_out)
void gemm_fp8_fp8_fp32_nt(const at::Tensor &a, const at::Tensor &sfa, const at::Tensor &b, const at::Tensor &sfb, at::Tensor &out,
                          const OptTensor &c)
{
    dense_fp32_out(a, sfa, b, sfb, out, c, false, dga_tiling_fp32_out, "tiling_fp32_out", dga_gemm_fp8_fp8_fp32_nt, "gemm_fp8_fp8_fp32_nt");
}
// per-row sfb [N, KB] (both operands per-1x128, the weight gradient): dga_wgrad_gemm_fp8_fp8_fp32_nt, default tiling (dga_tiling_wgrad)
void wgrad_gemm_fp8_fp8_fp32_nt(const at::Tensor &a, const at::Tensor &sfa, const at::Tensor &b, const at::Tensor &sfb, at::Tensor &out,
                                const OptTensor &c)
{
    dense_fp32_out(a, sfa, b, sfb, out, c, true, dga_tiling_wgrad, "tiling_wgrad", dga_wgrad_gemm_fp8_fp8_fp32_nt, "wgrad_gemm_fp8_fp8_fp32_nt");
}

// the MoE weight gradient with the groups along K: out[g] = c[g] + A[:, k0_g : k0_g + ks[g]] . B[:, ...]^T, ks a device int32 [G]
// read by the kernel; dga_k_grouped_wgrad_gemm_fp8_fp8_fp32_nt, default tiling (dga_tiling_k_grouped_wgrad).  The counts are not
// checked here (they stay on the device): the kernel clamps them to K_total
void k_grouped_wgrad_gemm_fp8_fp8_fp32_nt(const at::Tensor &a, const at::Tensor &sfa, const at::Tensor &b, const at::Tensor &sfb,
                                          at::Tensor &out, const at::Tensor &ks, const OptTensor &c)
{
    TORCH_CHECK(a.dim() == 2 && b.dim() == 2 && out.dim() == 3, "a [M,K_total], b [N,K_total], out [G,M,N]");
    const int64_t g = out.size(0), m = a.size(0), n = b.size(0), k = a.size(1), kb = k / 128;
    TORCH_CHECK(k % 128 == 0, "K_total must be a multiple of 128");
    want_fp8_operands(a, b, {n, k}, out, {g, m, n}, at::kFloat, sfa, {m, kb}, sfb, {n, kb});
    want_shape(ks, {g}, "ks"); want_dtype(ks, at::kInt, "ks");
    const at::Tensor *addend = want_c(c, {g, m, n});
    same_device({&a, &sfa, &b, &sfb, &out, &ks, addend});
    const c10::OptionalDeviceGuard guard(at::device_of(out));
    const dga_problem_t p = fp8_problem(m, n, k, g);
    dga_tiling_t t{};
    check(dga_tiling_k_grouped_wgrad(&p, &t), "tiling_k_grouped_wgrad");
    check(dga_k_grouped_wgrad_gemm_fp8_fp8_fp32_nt(a.data_ptr(), k, sfa.data_ptr<float>(), b.data_ptr(), k, sfb.data_ptr<float>(), c_ptr(addend),
                                                   out.data_ptr<float>(), ks.data_ptr<int32_t>(), g, m, n, k, 0, &t, nullptr, 0, cur_stream()),
          "k_grouped_wgrad_gemm_fp8_fp8_fp32_nt");
}

void m_grouped_gemm_fp8_fp8_bf16_nt_masked(const at::Tensor &a, const at::Tensor &sfa, const at::Tensor &b,
                                           const at::Tensor &sfb, at::Tensor &out, const at::Tensor &masked_m,
                                           int64_t expected_m, bool strict, const std::string &policy)
{
    const int tag = policy_tag(strict, policy);
    TORCH_CHECK(a.dim() == 3 && b.dim() == 3, "a [G,Mmax,K], b [G,N,K]");
    const int64_t g = a.size(0), mmax = a.size(1), n = b.size(1), k = a.size(2), kb = (k + 127) / 128, nb = (n + 127) / 128;
    want_fp8_operands(a, b, {g, n, k}, out, {g, mmax, n}, at::kBFloat16, sfa, {g, mmax, kb}, sfb, {g, nb, kb});
    want_shape(masked_m, {g}, "masked_m"); want_dtype(masked_m, at::kInt, "masked_m");
    same_device({&a, &sfa, &b, &sfb, &out, &masked_m});
    const c10::OptionalDeviceGuard guard(at::device_of(out));
    const dga_tiling_t t = tiling_for(fp8_problem(mmax, n, k, g, static_cast<int>(expected_m)), tag);
    check(dga_m_grouped_gemm_fp8_fp8_bf16_nt_masked(a.data_ptr(), sfa.data_ptr<float>(), b.data_ptr(), sfb.data_ptr<float>(),
                                                    out.data_ptr(), masked_m.data_ptr<int32_t>(), g, mmax, n, k,
                                                    static_cast<int>(expected_m), &t, nullptr, 0, cur_stream()),
          "m_grouped_gemm_fp8_fp8_bf16_nt_masked");
}

void m_grouped_gemm_fp8_fp8_bf16_nt_contiguous(const at::Tensor &a, const at::Tensor &sfa, const at::Tensor &b,
                                               const at::Tensor &sfb, at::Tensor &out, const at::Tensor &m_indices, bool strict,
                                               const std::string &policy)
{
    const int tag = policy_tag(strict, policy);
    TORCH_CHECK(a.dim() == 2 && b.dim() == 3, "a [Msum,K], b [G,N,K]");
    const int64_t msum = a.size(0), g = b.size(0), n = b.size(1), k = a.size(1), kb = (k + 127) / 128, nb = (n + 127) / 128;
    want_fp8_operands(a, b, {g, n, k}, out, {msum, n}, at::kBFloat16, sfa, {msum, kb}, sfb, {g, nb, kb});
    want_shape(m_indices, {msum}, "m_indices"); want_dtype(m_indices, at::kInt, "m_indices");
    same_device({&a, &sfa, &b, &sfb, &out, &m_indices});
    const c10::OptionalDeviceGuard guard(at::device_of(out));
    const dga_tiling_t t = tiling_for(fp8_problem(msum, n, k, g, 0, DGA_PROBLEM_CONTIGUOUS_M), tag);
    const Workspace ws(out, dga_workspace_bytes(&t));
    check(dga_m_grouped_gemm_fp8_fp8_bf16_nt_contiguous(a.data_ptr(), sfa.data_ptr<float>(), b.data_ptr(),
                                                        sfb.data_ptr<float>(), out.data_ptr(), m_indices.data_ptr<int32_t>(),
                                                        msum, g, n, k, &t, ws.ptr(), ws.bytes, cur_stream()),
          "m_grouped_gemm_fp8_fp8_bf16_nt_contiguous");
}

TensorPair cast_to_fp8(const at::Tensor &x, int block_rows)
{
    on_device(x, "x");
    TORCH_CHECK(x.dim() == 2, "x must be [rows, k]");
    const int dt = input_dtype(x, "x");
    const c10::OptionalDeviceGuard guard(at::device_of(x));
    at::Tensor q = at::empty(x.sizes(), x.options().dtype(at::kFloat8_e4m3fn));
    at::Tensor sf = at::empty({(x.size(0) + block_rows - 1) / block_rows, (x.size(1) + 127) / 128}, x.options().dtype(at::kFloat));
    check((block_rows == 1 ? dga_cast_to_fp8_1x128 : dga_cast_to_fp8_128x128)(x.data_ptr(), dt, x.size(0), x.size(1), q.data_ptr(),
                                                                               sf.data_ptr<float>(), cur_stream()),
          "cast_to_fp8");
    return {q, sf};
}

// What the two fused quantiser entries share.  The layout: x [rows, 2H], or [G, Mmax, 2H] with masked_m int32 [G] on x's device, of one of the
// three input types, the last dimension a multiple of `multiple` (last_dim: what to say when it is not).
struct FusedLayout {
    int64_t h, groups, rows;
    int dt;
    const int32_t *masked_m;
};
FusedLayout fused_layout(const at::Tensor &x, const OptTensor &masked_m, int64_t multiple, const char *last_dim)
{
    on_device(x, "x");
    const bool masked = masked_m.has_value();
    TORCH_CHECK(x.dim() == (masked ? 3 : 2), masked ? "x must be [G, Mmax, 2H] with masked_m" : "x must be [rows, 2H]");
    const int dt = input_dtype(x, "x");
    TORCH_CHECK(x.size(-1) % multiple == 0, last_dim);
    const int64_t groups = masked ? x.size(0) : 1;
    const void *counts = side_tensor(
        masked_m, "masked_m", x, [&](const at::Tensor &t) { return t.scalar_type() == at::kInt && t.dim() == 1 && t.size(0) == groups; },
        "masked_m must be int32 [G]");
    return {x.size(-1) / 2, groups, masked ? x.size(1) : x.size(0), dt, static_cast<const int32_t *>(counts)};
}
// ... and the outputs: (codes [..., width], scales [..., blocks]) with x's leading dimensions, at::empty (the rows a mask excludes are not
// written: they hold no value)
TensorPair fused_outputs(const at::Tensor &x, int64_t width, int64_t blocks)
{
    std::vector<int64_t> shape(x.sizes().begin(), x.sizes().end());
    shape.back() = width;
    at::Tensor q = at::empty(shape, x.options().dtype(at::kFloat8_e4m3fn));
    shape.back() = blocks;
    return {q, at::empty(shape, x.options().dtype(at::kFloat))};
}

// silu(x[..., :H]) * x[..., H:] -> the per-token quantiser, one pass (dga_silu_mul_cast_to_fp8_1x128).
TensorPair silu_and_mul_per_token_cast_to_fp8(const at::Tensor &x, const OptTensor &masked_m)
{
    const FusedLayout l = fused_layout(x, masked_m, 2, "the last dimension of x must be even (gate and up halves)");
    const c10::OptionalDeviceGuard guard(at::device_of(x));
    auto [q, sf] = fused_outputs(x, l.h, (l.h + 127) / 128);
    check(dga_silu_mul_cast_to_fp8_1x128(x.data_ptr(), l.dt, l.groups, l.rows, l.h, l.masked_m, nullptr, q.data_ptr(), sf.data_ptr<float>(), 0,
                                         cur_stream()),
          "silu_and_mul_per_token_cast_to_fp8");
    return {q, sf};
}

// The backward of that activation -> the per-token quantiser, one pass (dga_silu_mul_bwd_cast_to_fp8_1x128): grad_h [..., H] beside x; H % 128 == 0.
// (dq [.., 2H], dsf [.., 2H/128]) = the 1x128 quantiser on [dgate | dup]; grad_x_out (x's shape and dtype) receives the unquantised gradient.
TensorPair silu_and_mul_backward_per_token_cast_to_fp8(const at::Tensor &x, const at::Tensor &grad_h, const OptTensor &masked_m,
                                                       const OptTensor &grad_x_out)
{
    const FusedLayout l = fused_layout(x, masked_m, 256, "the last dimension of x must be 2H with H a multiple of 128");
    on_device(grad_h, "grad_h");
    std::vector<int64_t> shape(x.sizes().begin(), x.sizes().end());
    shape.back() = l.h;
    TORCH_CHECK(grad_h.sizes() == at::IntArrayRef(shape) && grad_h.scalar_type() == x.scalar_type(), "grad_h must be [..., H] of x's dtype");
    TORCH_CHECK(x.is_contiguous() && grad_h.is_contiguous(), "x and grad_h must be contiguous");
    TORCH_CHECK(grad_h.device() == x.device(), "all tensors must live on one device");
    void *grad_x = side_tensor(
        grad_x_out, "grad_x_out", x,
        [&](const at::Tensor &t) { return t.sizes() == x.sizes() && t.scalar_type() == x.scalar_type() && t.is_contiguous(); },
        "grad_x_out must be contiguous, of x's shape and dtype");
    const c10::OptionalDeviceGuard guard(at::device_of(x));
    auto [q, sf] = fused_outputs(x, 2 * l.h, 2 * l.h / 128);
    check(dga_silu_mul_bwd_cast_to_fp8_1x128(x.data_ptr(), grad_h.data_ptr(), l.dt, l.groups, l.rows, l.h, l.masked_m, nullptr, q.data_ptr(),
                                             sf.data_ptr<float>(), grad_x, 0, cur_stream()),
          "silu_and_mul_backward_per_token_cast_to_fp8");
    return {q, sf};
}

// What the two per-token quantisers of a transpose are: x [T, halves * H] -> (qt [H, T], sft [H, ceil(T/128)]) in one pass; rows with a
// negative m_indices (int32 [T]) are not read and count as zeros.  layout: what to say of an x that is not 2-D
TensorPair cast_transposed(const at::Tensor &x, const OptTensor &m_indices, int64_t halves, const char *layout,
                           decltype(&dga_cast_to_fp8_1x128_transposed) entry, const char *label)
{
    on_device(x, "x");
    TORCH_CHECK(x.dim() == 2 && x.is_contiguous(), layout);
    const int dt = input_dtype(x, "x");
    TORCH_CHECK(x.size(1) % halves == 0, "the last dimension of x must be even (gate and up halves)");
    const int64_t t_n = x.size(0), h = x.size(1) / halves;
    const void *indices = side_tensor(
        m_indices, "m_indices", x,
        [&](const at::Tensor &t) { return t.scalar_type() == at::kInt && t.dim() == 1 && t.size(0) == t_n && t.is_contiguous(); },
        "m_indices must be a contiguous int32 [T]");
    const c10::OptionalDeviceGuard guard(at::device_of(x));
    auto [qt, sft] = transposed_outputs(x, h, t_n);
    check(entry(x.data_ptr(), dt, 1, t_n, h, nullptr, static_cast<const int32_t *>(indices), qt.data_ptr(), t_n, sft.data_ptr<float>(), nullptr,
                nullptr, 0, cur_stream()),
          label);
    return {qt, sft};
}
// per_token_cast_to_fp8 of x^T (dga_cast_to_fp8_1x128_transposed)
TensorPair per_token_cast_to_fp8_transposed(const at::Tensor &x, const OptTensor &m_indices)
{
    return cast_transposed(x, m_indices, 1, "x must be a contiguous [T, H] tensor", dga_cast_to_fp8_1x128_transposed,
                           "per_token_cast_to_fp8_transposed");
}
// The same on h = silu(x[..., :H]) * x[..., H:] (dga_silu_mul_cast_to_fp8_1x128_transposed): x [T, 2H], the operand of dW2
TensorPair silu_and_mul_per_token_cast_to_fp8_transposed(const at::Tensor &x, const OptTensor &m_indices)
{
    return cast_transposed(x, m_indices, 2, "x must be a contiguous [T, 2H] tensor", dga_silu_mul_cast_to_fp8_1x128_transposed,
                           "silu_and_mul_per_token_cast_to_fp8_transposed");
}

// per_block_cast_to_fp8 of every w[g]^T in one pass (dga_cast_to_fp8_128x128_transposed): w [G, N, K] or [N, K] -> (qt [G, K, N],
// sft [G, ceil(K/128), ceil(N/128)]), 2-D for a 2-D w: the rhs of dgrad from the master weights.
TensorPair per_block_cast_to_fp8_transposed(const at::Tensor &w)
{
    on_device(w, "w");
    TORCH_CHECK((w.dim() == 2 || w.dim() == 3) && w.is_contiguous(), "w must be a contiguous [N, K] or [G, N, K] tensor");
    const int dt = input_dtype(w, "w");
    const int64_t groups = w.dim() == 3 ? w.size(0) : 1, n = w.size(-2), k = w.size(-1);
    const c10::OptionalDeviceGuard guard(at::device_of(w));
    std::vector<int64_t> shape(w.sizes().begin(), w.sizes().end());
    shape[shape.size() - 2] = k;
    shape.back() = n;
    at::Tensor qt = at::empty(shape, w.options().dtype(at::kFloat8_e4m3fn));
    shape[shape.size() - 2] = (k + 127) / 128;
    shape.back() = (n + 127) / 128;
    at::Tensor sft = at::empty(shape, w.options().dtype(at::kFloat));
    check(dga_cast_to_fp8_128x128_transposed(w.data_ptr(), dt, groups, n, k, qt.data_ptr(), sft.data_ptr<float>(), nullptr, nullptr, 0,
                                             cur_stream()),
          "per_block_cast_to_fp8_transposed");
    return {qt, sft};
}

// per_token_cast_to_fp8_transposed of the rows src[index[r] / index_div] (times row_scale[index[r]]) in one pass
// (dga_gather_cast_to_fp8_1x128_transposed): src [S, H], index int64 [T] -> (qt [H, T], sft [H, ceil(T/128)]); a row whose index is outside
// [0, S * index_div) is not read and counts as zeros.
TensorPair gather_per_token_cast_to_fp8_transposed(const at::Tensor &src, const at::Tensor &index, int64_t index_div, const OptTensor &row_scale)
{
    on_device(src, "src"); on_device(index, "index");
    TORCH_CHECK(src.dim() == 2 && src.is_contiguous(), "src must be a contiguous [S, H] tensor");
    const int dt = input_dtype(src, "src");
    TORCH_CHECK(index.scalar_type() == at::kLong && index.dim() == 1 && index.is_contiguous(), "index must be a contiguous int64 [T] tensor");
    TORCH_CHECK(index.device() == src.device(), "all tensors must live on one device");
    TORCH_CHECK(index_div >= 1, "index_div must be >= 1");
    const int64_t s_n = src.size(0), h = src.size(1), t_n = index.size(0);
    const void *scale = side_tensor(
        row_scale, "row_scale", src,
        [&](const at::Tensor &t) { return t.scalar_type() == at::kFloat && t.numel() == s_n * index_div && t.is_contiguous(); },
        "row_scale must be contiguous float32 with S * index_div elements");
    const c10::OptionalDeviceGuard guard(at::device_of(src));
    auto [qt, sft] = transposed_outputs(src, h, t_n);
    check(dga_gather_cast_to_fp8_1x128_transposed(src.data_ptr(), dt, s_n, h, index.data_ptr<int64_t>(), index_div, static_cast<const float *>(scale), 1,
                                                  t_n, nullptr, qt.data_ptr(), t_n, sft.data_ptr<float>(), nullptr, nullptr, 0, cur_stream()),
          "gather_per_token_cast_to_fp8_transposed");
    return {qt, sft};
}

// What the two combine bindings take: src [S, H] of one of the three input types (-> its DGA_DT_*), dest int64 [T, k] on src's device
int combine_layout(const at::Tensor &src, const at::Tensor &dest)
{
    on_device(src, "src"); on_device(dest, "dest");
    TORCH_CHECK(src.dim() == 2 && src.is_contiguous(), "src must be a contiguous [S, H] tensor");
    TORCH_CHECK(dest.scalar_type() == at::kLong && dest.dim() == 2 && dest.is_contiguous() && dest.size(1) >= 1,
                "dest must be a contiguous int64 [T, k] tensor with k >= 1");
    TORCH_CHECK(dest.device() == src.device(), "all tensors must live on one device");
    return input_dtype(src, "src");
}
// y[t] = sum_j weights[t, j] * src[dest[t, j]] (dga_combine_rows): src [S, H], dest int64 [T, k], weights float32 [T, k] or None -> y [T, H] of
// src's dtype; a dest outside [0, S) is skipped.
at::Tensor combine_tokens(const at::Tensor &src, const at::Tensor &dest, const OptTensor &weights)
{
    const int dt = combine_layout(src, dest);
    const void *w = side_tensor(
        weights, "weights", src, [&](const at::Tensor &t) { return t.scalar_type() == at::kFloat && t.sizes() == dest.sizes() && t.is_contiguous(); },
        "weights must be contiguous float32 [T, k]");
    const c10::OptionalDeviceGuard guard(at::device_of(src));
    at::Tensor out = at::empty({dest.size(0), src.size(1)}, src.options());
    check(dga_combine_rows(src.data_ptr(), dt, src.size(0), src.size(1), dest.data_ptr<int64_t>(), static_cast<const float *>(w), dest.size(0),
                           dest.size(1), out.data_ptr(), dt, cur_stream()),
          "combine_tokens");
    return out;
}

// dw[t, j] = <src[dest[t, j]], grad[t]> (dga_combine_rows_weight_grad): float32 [T, k], +0 for a dest outside [0, S).
at::Tensor combine_tokens_weight_grad(const at::Tensor &src, const at::Tensor &grad, const at::Tensor &dest)
{
    const int dt = combine_layout(src, dest);
    on_device(grad, "grad");
    TORCH_CHECK(grad.dim() == 2 && grad.size(0) == dest.size(0) && grad.size(1) == src.size(1) && grad.is_contiguous() &&
                grad.scalar_type() == src.scalar_type(), "grad must be contiguous [T, H] of src's dtype");
    TORCH_CHECK(grad.device() == src.device(), "all tensors must live on one device");
    const c10::OptionalDeviceGuard guard(at::device_of(src));
    at::Tensor dw = src.size(1) == 0 ? at::zeros(dest.sizes(), src.options().dtype(at::kFloat)) : at::empty(dest.sizes(), src.options().dtype(at::kFloat));
    check(dga_combine_rows_weight_grad(src.data_ptr(), grad.data_ptr(), dt, src.size(0), src.size(1), dest.data_ptr<int64_t>(), dest.size(0),
                                       dest.size(1), dw.data_ptr<float>(), cur_stream()),
          "combine_tokens_weight_grad");
    return dw;
}

}  // namespace

PYBIND11_MODULE(deep_gemm_cpp, m)   // the reference's module name (python_api.cpp:30)
{
    m.doc() = "MI355X drop-in for deep_gemm_ascend's deep_gemm_cpp (C ABI: include/dga_hip.h)";
    m.def("run_mmad_custom", [](const at::Tensor &, const at::Tensor &, at::Tensor &) {},
          "the reference's static kernel returns at once (include/impls/mmad.cpp:79): a no-op, kept for API parity");
    m.def("run_mmad_rtc", &run_mmad_rtc, "run_mmad_rtc");
    m.def("run_mmad_bench", &run_mmad_bench, "run_mmad_bench");
    m.def("gemm_fp8_fp8_bf16_nt", &gemm_fp8_fp8_bf16_nt, py::arg("a"), py::arg("sfa"), py::arg("b"), py::arg("sfb"),
          py::arg("out"), py::arg("strict") = false, py::arg("policy") = "");
    m.def("gemm_fp8_fp8_fp32_nt", &gemm_fp8_fp8_fp32_nt, py::arg("a"), py::arg("sfa"), py::arg("b"), py::arg("sfb"), py::arg("out"),
          py::arg("c") = py::none());
    m.def("wgrad_gemm_fp8_fp8_fp32_nt", &wgrad_gemm_fp8_fp8_fp32_nt, py::arg("a"), py::arg("sfa"), py::arg("b"), py::arg("sfb"),
          py::arg("out"), py::arg("c") = py::none());
    m.def("k_grouped_wgrad_gemm_fp8_fp8_fp32_nt", &k_grouped_wgrad_gemm_fp8_fp8_fp32_nt, py::arg("a"), py::arg("sfa"), py::arg("b"),
          py::arg("sfb"), py::arg("out"), py::arg("ks"), py::arg("c") = py::none());
    m.def("m_grouped_gemm_fp8_fp8_bf16_nt_masked", &m_grouped_gemm_fp8_fp8_bf16_nt_masked, py::arg("a"), py::arg("sfa"),
          py::arg("b"), py::arg("sfb"), py::arg("out"), py::arg("masked_m"), py::arg("expected_m"), py::arg("strict") = false,
          py::arg("policy") = "");
    m.def("m_grouped_gemm_fp8_fp8_bf16_nt_contiguous", &m_grouped_gemm_fp8_fp8_bf16_nt_contiguous, py::arg("a"),
          py::arg("sfa"), py::arg("b"), py::arg("sfb"), py::arg("out"), py::arg("m_indices"), py::arg("strict") = false,
          py::arg("policy") = "");
    m.def("get_m_alignment_for_contiguous_layout", [] { return DGA_CONTIGUOUS_M_ALIGNMENT; });
    m.def("per_token_cast_to_fp8", [](const at::Tensor &x) { return cast_to_fp8(x, 1); });
    m.def("per_block_cast_to_fp8", [](const at::Tensor &x) { return cast_to_fp8(x, 128); });
    m.def("silu_and_mul_per_token_cast_to_fp8", &silu_and_mul_per_token_cast_to_fp8, py::arg("x"), py::arg("masked_m") = py::none());
    m.def("silu_and_mul_backward_per_token_cast_to_fp8", &silu_and_mul_backward_per_token_cast_to_fp8, py::arg("x"), py::arg("grad_h"),
          py::arg("masked_m") = py::none(), py::arg("grad_x_out") = py::none());
    m.def("per_token_cast_to_fp8_transposed", &per_token_cast_to_fp8_transposed, py::arg("x"), py::arg("m_indices") = py::none());
    m.def("silu_and_mul_per_token_cast_to_fp8_transposed", &silu_and_mul_per_token_cast_to_fp8_transposed, py::arg("x"),
          py::arg("m_indices") = py::none());
    m.def("per_block_cast_to_fp8_transposed", &per_block_cast_to_fp8_transposed, py::arg("w"));
    m.def("gather_per_token_cast_to_fp8_transposed", &gather_per_token_cast_to_fp8_transposed, py::arg("src"), py::arg("index"),
          py::arg("index_div") = 1, py::arg("row_scale") = py::none());
    m.def("combine_tokens", &combine_tokens, py::arg("src"), py::arg("dest"), py::arg("weights") = py::none());
    m.def("combine_tokens_weight_grad", &combine_tokens_weight_grad, py::arg("src"), py::arg("grad"), py::arg("dest"));
    m.def("abi_version", [] { return dga_abi_version(); });
}
