"""GPU: k_grouped_wgrad_gemm_fp8_fp8_fp32_nt -- the MoE weight gradient with the groups along K.  Every group equals the dense weight-gradient
entry on contiguous copies of its slices (same tile, plain raster) bit for bit under bf16_exact, the per-column oracle under strict; empty
groups give c exactly; a captured call replays with rewritten device counts."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KS = [256, 0, 128, 640, 0, 384, 128, 1024]   # 0, 128, 256 and larger, next to each other; sum 2560


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _assert_same_bits(got, want, what):
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaN positions differ"
    g, w = np.where(gn, 0, got).astype(np.float32), np.where(wn, 0, want).astype(np.float32)
    bad = g.view(np.uint32) != w.view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {got.size} outputs differ in their bits"


def _inputs(oracle, m, n, k_total, seed):
    """A [M, K_total] / B [N, K_total] fp8 with per-1x128 scales that differ per row on both operands."""
    a, sfa, _, _ = oracle.make_inputs(m, 128, k_total, seed=seed)
    b, sfb, _, _ = oracle.make_inputs(n, 128, k_total, seed=seed + 1)
    rng = np.random.default_rng(seed)
    sfb = (sfb * np.exp2(rng.integers(-3, 4, size=sfb.shape)) * rng.uniform(0.5, 2.0, size=sfb.shape)).astype(np.float32)
    return np.ascontiguousarray(a), np.ascontiguousarray(sfa), np.ascontiguousarray(b), sfb


def _tile(dga, m, n, k, m1, n1, build, tag=7):
    t = dga.tiling(m, n, max(k, 128), policy="bf16_exact")
    t.m1, t.n1, t.kernelSerial, t.build, t.splitkFactor, t.dispatchPolicyTag = m1, n1, 0, build, 1, tag
    t.stages, t.wavesM, t.wavesN = 3, 0, 0
    return t


def _kg(dga, a, sfa, b, sfb, ks, t=None, c=None, out=None, **kw):
    g, m, n = len(ks), a.shape[0], b.shape[0]
    if out is None:
        out = torch.full((g, m, n), float("nan"), dtype=torch.float32, device="cuda")
    dga.k_grouped_wgrad_gemm_fp8_fp8_fp32_nt((_dev(a), _dev(sfa)), (_dev(b), _dev(sfb)), out, ks, c=c, tiling_=t, sync=True, **kw)
    return out.cpu().numpy()


def _slices(a, sfa, b, sfb, ks):
    k0 = 0
    for kg in ks:
        yield (np.ascontiguousarray(a[:, k0:k0 + kg]), np.ascontiguousarray(sfa[:, k0 // 128:(k0 + kg) // 128]),
               np.ascontiguousarray(b[:, k0:k0 + kg]), np.ascontiguousarray(sfb[:, k0 // 128:(k0 + kg) // 128]))
        k0 += kg


def _dense(dga, a, sfa, b, sfb, t):
    out = torch.full((a.shape[0], b.shape[0]), float("nan"), dtype=torch.float32, device="cuda")
    dga.wgrad_gemm_fp8_fp8_fp32_nt((_dev(a), _dev(sfa)), (_dev(b), _dev(sfb)), out, tiling_=t, sync=True)
    return out.cpu().numpy()


TILES = [("one_tile_128x256", 128, 256, 8), ("one_tile_128x128", 128, 128, 8), ("one_tile_64x256", 64, 256, 8),
         ("one_tile_64x128", 64, 128, 8), ("one_tile_32x128", 32, 128, 8), ("persistent", 128, 256, 7)]


@pytest.mark.parametrize("name,m1,n1,build", TILES, ids=[t[0] for t in TILES])
@pytest.mark.parametrize("m,n", [(300, 257), (129, 127)])
def test_every_group_is_the_dense_entry_on_its_slices(dga, oracle, name, m1, n1, build, m, n):
    ks = KS
    a, sfa, b, sfb = _inputs(oracle, m, n, sum(ks) + 256, seed=m + n)
    got = _kg(dga, a, sfa, b, sfb, ks, _tile(dga, m, n, sum(ks), m1, n1, build))
    for g, (sa, ssa, sb, ssb) in enumerate(_slices(a, sfa, b, sfb, ks)):
        if ks[g] == 0:
            assert not got[g].any() and not np.signbit(got[g]).any(), f"{name}: empty group {g} is not +0"
            continue
        want = _dense(dga, sa, ssa, sb, ssb, _tile(dga, m, n, ks[g], m1, n1, 8))
        _assert_same_bits(got[g], want, f"{name} group {g}")


def test_persistent_one_block_groups_next_to_large_ones(dga, oracle):
    """Many tiles per CU on the persistent build with KB_g of 1 and 0 between long groups: the ring across tile boundaries."""
    ks = [128, 2048, 128, 0, 1536, 128, 128, 256, 0, 1024, 128]
    m, n = 1024, 2048
    a, sfa, b, sfb = _inputs(oracle, m, n, sum(ks), seed=5)
    got = _kg(dga, a, sfa, b, sfb, ks, _tile(dga, m, n, sum(ks), 128, 256, 7))
    for g, (sa, ssa, sb, ssb) in enumerate(_slices(a, sfa, b, sfb, ks)):
        if ks[g]:
            _assert_same_bits(got[g], _dense(dga, sa, ssa, sb, ssb, _tile(dga, m, n, ks[g], 128, 256, 8)), f"group {g}")
        else:
            assert not got[g].any()


def test_strict_is_the_per_column_oracle(dga, oracle):
    ks = [256, 0, 128, 384]
    m, n = 70, 45
    a, sfa, b, sfb = _inputs(oracle, m, n, sum(ks) + 128, seed=11)
    got = _kg(dga, a, sfa, b, sfb, ks, strict=True)
    for g, (sa, ssa, sb, ssb) in enumerate(_slices(a, sfa, b, sfb, ks)):
        if ks[g] == 0:
            assert not got[g].any()
            continue
        want = np.concatenate([oracle.gemm_fp8_fp8_bf16_nt(sa, ssa, sb[j:j + 1], ssb[j:j + 1], threads=8, want_f32=True)[1]
                               for j in range(n)], axis=1)
        _assert_same_bits(got[g], want, f"strict group {g}")


def test_strict_64_row_tiles_are_the_dense_strict_entry(dga, oracle):
    """G x tiles64 >= CUs: the 64-row strict build (the small cases above run the 32-row one).  The dense strict entry on each group's
    slices is the oracle's result (tests/test_wgrad_gpu.py), so device against device, bit for bit."""
    rng = np.random.default_rng(7)
    ks = [int(v) for v in rng.choice([0, 128, 256], size=64)]
    m, n = 128, 256
    a, sfa, b, sfb = _inputs(oracle, m, n, sum(ks) + 128, seed=13)
    got = _kg(dga, a, sfa, b, sfb, ks, strict=True)
    for g, (sa, ssa, sb, ssb) in enumerate(_slices(a, sfa, b, sfb, ks)):
        if ks[g] == 0:
            assert not got[g].any()
            continue
        out = torch.full((m, n), float("nan"), dtype=torch.float32, device="cuda")
        dga.wgrad_gemm_fp8_fp8_fp32_nt((_dev(sa), _dev(ssa)), (_dev(sb), _dev(ssb)), out, strict=True, sync=True)
        _assert_same_bits(got[g], out.cpu().numpy(), f"strict group {g}")


def test_ks_tensor_on_another_device_is_refused(dga):
    lhs = (torch.zeros(64, 256, dtype=torch.uint8, device="cuda"), torch.ones(64, 2, device="cuda"))
    rhs = (torch.zeros(32, 256, dtype=torch.uint8, device="cuda"), torch.ones(32, 2, device="cuda"))
    out = torch.zeros(2, 64, 32, device="cuda")
    with pytest.raises(dga.DGAError, match="ks_tensor must live on the operands' device"):
        dga.k_grouped_wgrad_gemm_fp8_fp8_fp32_nt(lhs, rhs, out, [128, 128], ks_tensor=torch.tensor([128, 128], dtype=torch.int32))


def test_bf16_exact_within_the_bar_of_the_exact_result(dga, oracle):
    ks = [384, 128, 0, 512]
    m, n = 300, 257
    a, sfa, b, sfb = _inputs(oracle, m, n, sum(ks), seed=3)
    got = _kg(dga, a, sfa, b, sfb, ks).astype(np.float64)
    tab = oracle.e4m3fn_table().astype(np.float64)
    for g, (sa, ssa, sb, ssb) in enumerate(_slices(a, sfa, b, sfb, ks)):
        da = tab[sa] * np.repeat(ssa.astype(np.float64), 128, axis=1)
        db = tab[sb] * np.repeat(ssb.astype(np.float64), 128, axis=1)
        ref, S = da @ db.T, np.abs(da) @ np.abs(db).T
        excess = np.abs(got[g] - ref) - (2.0 ** -22 * S + 2.0 ** -24 * np.abs(ref))
        assert (excess <= 0).all(), f"group {g}: {int((excess > 0).sum())} outputs beyond the bar"


@pytest.mark.parametrize("mode", ["separate", "inplace"])
def test_c_is_added_and_empty_groups_give_c_exactly(dga, oracle, mode):
    ks = [256, 0, 128, 0]
    m, n = 129, 127
    a, sfa, b, sfb = _inputs(oracle, m, n, sum(ks), seed=17)
    c_np = np.random.default_rng(1).standard_normal((len(ks), m, n)).astype(np.float32)
    c_np[1, 0, :4] = -0.0
    plain = _kg(dga, a, sfa, b, sfb, ks)
    c = _dev(c_np)
    out = c if mode == "inplace" else None
    got = _kg(dga, a, sfa, b, sfb, ks, c=c, out=out)
    for g in range(len(ks)):
        want = c_np[g] if ks[g] == 0 else (plain[g] + c_np[g]).astype(np.float32)
        _assert_same_bits(got[g], want, f"{mode} group {g}")


@pytest.mark.parametrize("build", ["default", "persistent"])
def test_graph_replay_reads_the_rewritten_counts(dga, oracle, build):
    m, n, k_total = 300, 257, 2048
    a, sfa, b, sfb = _inputs(oracle, m, n, k_total, seed=23)
    splits = [[512, 256, 1024, 256], [1024, 512, 128, 384], [768, 0, 640, 640]]
    lhs, rhs = (_dev(a), _dev(sfa)), (_dev(b), _dev(sfb))
    ks_t = torch.tensor(splits[0], dtype=torch.int32, device="cuda")
    c0 = np.random.default_rng(2).standard_normal((4, m, n)).astype(np.float32)
    out = _dev(c0)
    t = _tile(dga, m, n, k_total, 128, 256, 7) if build == "persistent" else None
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):   # (warm-up: plan and module loads outside the capture)
        dga.k_grouped_wgrad_gemm_fp8_fp8_fp32_nt(lhs, rhs, out, splits[0], ks_tensor=ks_t, c=out, tiling_=t)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dga.k_grouped_wgrad_gemm_fp8_fp8_fp32_nt(lhs, rhs, out, splits[0], ks_tensor=ks_t, c=out, tiling_=t)
    for ks in splits[1:]:
        out.copy_(_dev(c0))
        ks_t.copy_(torch.tensor(ks, dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        want = _dev(c0)
        dga.k_grouped_wgrad_gemm_fp8_fp8_fp32_nt(lhs, rhs, want, ks, c=want, tiling_=t, sync=True)
        _assert_same_bits(out.cpu().numpy(), want.cpu().numpy(), f"replay {ks}")


def test_end_to_end_from_the_contiguous_forward_layout(dga, oracle):
    """dY [T, M] and X [T, N] in the contiguous layout (every expert's segment padded to 128 rows with zeros), quantised per token of
    the transposes, against the float64 dY_g^T X_g of the dequantised operands."""
    torch.manual_seed(0)
    tokens = [200, 0, 77, 300]
    m, n = 256, 384
    seg = [(t + 127) // 128 * 128 for t in tokens]
    T = sum(seg) + 128
    dy = torch.zeros(T, m, dtype=torch.bfloat16)
    x = torch.zeros(T, n, dtype=torch.bfloat16)
    r = 0
    for t, s in zip(tokens, seg):
        dy[r:r + t] = torch.randn(t, m).to(torch.bfloat16)
        x[r:r + t] = torch.randn(t, n).to(torch.bfloat16)
        r += s
    a, sfa = dga.per_token_cast_to_fp8(dy.t().contiguous().cuda())
    b, sfb = dga.per_token_cast_to_fp8(x.t().contiguous().cuda())
    out = torch.full((len(tokens), m, n), float("nan"), dtype=torch.float32, device="cuda")
    dga.k_grouped_wgrad_gemm_fp8_fp8_fp32_nt((a, sfa), (b, sfb), out, seg, sync=True)
    tab = oracle.e4m3fn_table().astype(np.float64)
    da = tab[a.view(torch.uint8).cpu().numpy()] * np.repeat(sfa.cpu().numpy().astype(np.float64), 128, axis=1)
    db = tab[b.view(torch.uint8).cpu().numpy()] * np.repeat(sfb.cpu().numpy().astype(np.float64), 128, axis=1)
    got = out.cpu().numpy().astype(np.float64)
    k0 = 0
    for g, s in enumerate(seg):
        ref = da[:, k0:k0 + s] @ db[:, k0:k0 + s].T
        S = np.abs(da[:, k0:k0 + s]) @ np.abs(db[:, k0:k0 + s]).T
        assert (np.abs(got[g] - ref) <= 2.0 ** -22 * S + 2.0 ** -24 * np.abs(ref)).all(), f"expert {g}"
        k0 += s


def test_pybind_matches_the_python_entry(dga, oracle):
    from deepgemm_ascend_amd import deep_gemm_cpp
    ks = [256, 0, 384]
    m, n = 300, 257
    a, sfa, b, sfb = _inputs(oracle, m, n, sum(ks) + 128, seed=29)
    want = _kg(dga, a, sfa, b, sfb, ks)
    out = torch.full((len(ks), m, n), float("nan"), dtype=torch.float32, device="cuda")
    deep_gemm_cpp.k_grouped_wgrad_gemm_fp8_fp8_fp32_nt(_dev(a), _dev(sfa), _dev(b), _dev(sfb), out,
                                                        torch.tensor(ks, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    _assert_same_bits(out.cpu().numpy(), want, "pybind")


def test_full_size_skewed(dga):
    """G = 8, (M, N) = (4096, 7168), skewed counts summing to 32768: device against device, group by group."""
    m, n, ks = 4096, 7168, [16384, 8192, 4096, 2048, 1024, 0, 896, 128]
    k_total = sum(ks)
    g = torch.Generator(device="cuda").manual_seed(0)
    a = (torch.randn(m, k_total, device="cuda", generator=g) * 8).to(torch.float8_e4m3fn)
    b = (torch.randn(n, k_total, device="cuda", generator=g) * 8).to(torch.float8_e4m3fn)
    sfa = torch.rand(m, k_total // 128, device="cuda", generator=g) + 0.5
    sfb = torch.rand(n, k_total // 128, device="cuda", generator=g) + 0.5
    out = torch.full((len(ks), m, n), float("nan"), dtype=torch.float32, device="cuda")
    t = dga.tiling_k_grouped_wgrad(m, n, k_total, len(ks))
    dga.k_grouped_wgrad_gemm_fp8_fp8_fp32_nt((a, sfa), (b, sfb), out, ks, tiling_=t, sync=True)
    k0 = 0
    for i, kg in enumerate(ks):
        if kg == 0:
            assert not out[i].any().item()
            continue
        want = torch.full((m, n), float("nan"), dtype=torch.float32, device="cuda")
        dt = _tile(dga, m, n, kg, t.m1, t.n1, 8)
        dga.wgrad_gemm_fp8_fp8_fp32_nt((a[:, k0:k0 + kg].contiguous(), sfa[:, k0 // 128:(k0 + kg) // 128].contiguous()),
                                       (b[:, k0:k0 + kg].contiguous(), sfb[:, k0 // 128:(k0 + kg) // 128].contiguous()), want,
                                       tiling_=dt, sync=True)
        assert torch.equal(out[i].view(torch.int32), want.view(torch.int32)), f"group {i}"
        k0 += kg
