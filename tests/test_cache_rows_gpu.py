"""GPU: the default-policy entries run the tiling a cache row leads them to, on general (not power-of-two) scales, against the oracle.

Each case opens one tiling-cache file (rows as harness/sweep.py writes them, or as a hand-written file holds them) and calls the entries
that name no tiling: the C entry with tiling == NULL (the only front end that keeps the tiling's tag as the selector returns it), the
Python operators with no policy and with policy="auto", the masked grouped operator, the fp32 and weight-gradient entries, and the
deep_gemm_cpp binding.  The rows: fast sweep winners whose register workgroup split-K name (`build` 1, legacy `stages` 1) used to leak
into the bf16-exact tiling, bf16-exact rows with the UE8M0 flag (the power-of-two-scales builds on general scales), bf16-exact rows
the menu does not hold, and one good row per branch of dga_tiling_bf16_exact.  The CPU contract: tests/test_cache_rows.py."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
WS_BYTES = 128 << 20      # more than any tiling of these shapes asks for (one Stream-K slot per CU is 64 MiB)


def _sweep():
    from deepgemm_ascend_amd.harness import sweep
    return sweep


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _bits(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _bf16x_bar(oracle, got, want, a, sfa, b, sfb, k):
    """tests/test_fuzz_gpu.py's bar: 2 ulp on all but 1e-5 of the elements, the rest within 2 ulp + 2^-22 S (2^-19 below K = 128)."""
    rep = oracle.parity_report(got, want, a, sfa, b, sfb)
    size = int(np.asarray(got).size)
    assert rep["nan_positions_equal"], rep
    lam = 1e-5 * size
    assert rep["frac_gt_max_ulp"] * size <= max(lam + 3.0 * lam ** 0.5, 2), rep
    assert rep["worst_excess_over_S"] <= (2.0 ** -22 if k >= 128 else 2.0 ** -19), rep


def _fp32_bar(got, ref, S):
    """tests/test_fp32_out_gpu.py::test_bf16_exact_within_the_bar_of_the_exact_result's bar."""
    assert not np.isnan(got).any(), "an output was not written"
    excess = np.abs(got.astype(np.float64) - ref) - (2.0 ** -22 * S + 2.0 ** -24 * np.abs(ref))
    assert (excess <= 0).all(), f"{int((excess > 0).sum())} outputs beyond the bar"


def _per_row_sfb(sfb2d, n, seed):
    """sfb [N, KB] that differs per row: the block's scale times 2^-3..2^3 times an arbitrary factor in [0.5, 2)."""
    rng = np.random.default_rng(seed)
    f = np.exp2(rng.integers(-3, 4, size=(n, 1))) * rng.uniform(0.5, 2.0, size=(n, 1))
    return (np.repeat(sfb2d, 128, axis=0)[:n] * f).astype(np.float32)


def _exact_rows(oracle, a, sfa, b, sfb_rows):
    """(float64 product, sum of its terms' magnitudes) with one sfb per row of B."""
    tab = oracle.e4m3fn_table().astype(np.float64)
    k = a.shape[1]
    da = tab[np.asarray(a, np.uint8)] * np.repeat(sfa.astype(np.float64), 128, axis=1)[:, :k]
    db = tab[np.asarray(b, np.uint8)] * np.repeat(sfb_rows.astype(np.float64), 128, axis=1)[:, :k]
    return da @ db.T, np.abs(da) @ np.abs(db).T


def _null_tiling_call(dga, a, sfa, b, sfb, out, m, n, k):
    """dga_gemm_fp8_fp8_bf16_nt with tiling == NULL: the tiling the library itself resolves, tag included."""
    from deepgemm_ascend_amd import _lib
    ws = torch.empty(WS_BYTES, dtype=torch.uint8, device="cuda")
    rc = _lib.lib().dga_gemm_fp8_fp8_bf16_nt(a.data_ptr(), sfa.data_ptr(), b.data_ptr(), sfb.data_ptr(), out.data_ptr(), m, n, k,
                                             None, ws.data_ptr(), WS_BYTES, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


class _Cache:
    def __init__(self, dga, path, head, rows):
        self.dga, self.path = dga, path
        path.write_text(head + "".join(rows))

    def __enter__(self):
        self.dga.tiling_cache_open(str(self.path))
        self.dga.api._PLANS.clear()
        return self

    def __exit__(self, *exc):
        self.dga.tiling_cache_open(None)
        self.dga.tiling_cache_clear()
        self.dga.api._PLANS.clear()
        return False


def _bx(m, n, k, tag=7, **p):
    sweep = _sweep()
    row = sweep.bx_row(m, n, k, dict({"raster": 1, "stages": 3, "splitk": 1, "policy": 7}, **p))
    cells = row.strip().split(",")
    cells[16] = str(tag)
    return sweep.FULL_CSV_HEAD, ",".join(cells) + "\n"


def _bx_candidate(m, n, k, **want):
    """The sweep's own bf16-exact candidate of this shape that has every (key, value) of want, as the row it writes."""
    sweep = _sweep()
    for p in sweep.candidates_bx(m, n, k):
        if all(p.get(key) == v for key, v in want.items()):
            return sweep.FULL_CSV_HEAD, sweep.bx_row(m, n, k, p)
    raise AssertionError(f"no bf16-exact candidate {want} for {m}x{n}x{k}")


def _fast_wsk_register(m, n, k):
    """The fast sweep's register workgroup split-K candidate (build name in legacy `stages` 1), as its row writer appends it."""
    sweep = _sweep()
    p = [c for c in sweep.candidates(m, n, k, rasters=[0]) if c.get("wsk") == 1]
    assert p, (m, n, k)
    return sweep.FAST_CSV_HEAD, sweep.fast_row(m, n, k, p[0])


# (name, m, n, k, row maker): the defects, then one good row per branch
DENSE_CASES = [
    ("leak_40x512x1024", 40, 512, 1024, lambda m, n, k: _fast_wsk_register(m, n, k)),
    ("leak_64x1024x4096", 64, 1024, 4096, lambda m, n, k: _fast_wsk_register(m, n, k)),
    ("leak_build1_row", 48, 512, 2048, lambda m, n, k: (_sweep().FULL_CSV_HEAD, f"{m},{n},{k},64,128,128,6,0,0,0,4,1,3,1,0,0,0,1,0,1\n")),
    ("ue8m0_dense", 256, 1024, 2048, lambda m, n, k: _bx(m, n, k, tag=23, m1=128, n1=256)),
    ("ue8m0_decode", 24, 1024, 2048, lambda m, n, k: _bx(m, n, k, tag=23, m1=32, n1=128, wsk=2)),
    ("decode_build_off_its_tile", 300, 520, 1024, lambda m, n, k: _bx(m, n, k, m1=128, n1=128, splitk=2, build=10)),
    ("tail_off_its_tile", 300, 520, 1024, lambda m, n, k: _bx(m, n, k, m1=64, n1=256, tail=1)),
    ("good_wsk", 8, 1024, 1024, lambda m, n, k: _bx_candidate(m, n, k, wsk=2, build=None)),
    ("good_dsk", 128, 1024, 2048, lambda m, n, k: _bx_candidate(m, n, k, build=10)),
    ("good_split", 300, 520, 1024, lambda m, n, k: _bx_candidate(m, n, k, m1=64, n1=256, splitk=2)),
    ("good_streamk", 300, 520, 1024, lambda m, n, k: _bx_candidate(m, n, k, streamk=1)),
    ("good_tail", 2176, 4096, 256, lambda m, n, k: _bx_candidate(m, n, k, tail=1)),
    ("good_odd_k", 100, 520, 1000, lambda m, n, k: _bx_candidate(m, n, k, m1=64, n1=256, splitk=1)),
]


@pytest.mark.parametrize("name,m,n,k,make", DENSE_CASES, ids=[c[0] for c in DENSE_CASES])
def test_dense_default_entries_under_a_cache_row(dga, oracle, tmp_path, name, m, n, k, make):
    head, row = make(m, n, k)
    a, sfa, b, sfb = oracle.make_inputs(m, n, k, seed=m + 3 * n + k)
    want = oracle.gemm_fp8_fp8_bf16_nt(a, sfa, b, sfb, threads=8)
    da, dsfa, db, dsfb = (_dev(x) for x in (a, sfa, b, sfb))
    with _Cache(dga, tmp_path / "rows.csv", head, [row]):
        # (first the call whose outputs show a wrong tag: the selector's own result is checked after it)
        out = torch.full((m, n), float("nan"), dtype=torch.bfloat16, device="cuda")
        assert _null_tiling_call(dga, da, dsfa, db, dsfb, out, m, n, k) == 0
        _bf16x_bar(oracle, _bits(out), want, a, sfa, b, sfb, k)
        t = dga.tiling(m, n, k, policy="bf16_exact")
        assert t.dispatchPolicyTag == 7 and dga.tiling_check(t) == 0, t.as_dict()
        for policy in (None, "auto"):
            out = torch.full((m, n), float("nan"), dtype=torch.bfloat16, device="cuda")
            dga.gemm_fp8_fp8_bf16_nt((da, dsfa), (db, dsfb), out, sync=True, policy=policy)
            if policy is None:
                _bf16x_bar(oracle, _bits(out), want, a, sfa, b, sfb, k)
            else:   # "auto": the fast path's wider bar where it is not the decode kernel
                assert not np.isnan(out.float().cpu().numpy()).any()
                oracle.assert_parity(_bits(out), want, a, sfa, b, sfb)
        # fp32 rows: the bar of the exact result
        ref, S = oracle.gemm_fp8_fp8_f64_nt(a, sfa, b, sfb).astype(np.float64), np.asarray(oracle.abs_term_sum(a, sfa, b, sfb), np.float64)
        out32 = torch.full((m, n), float("nan"), dtype=torch.float32, device="cuda")
        dga.gemm_fp8_fp8_fp32_nt((da, dsfa), (db, dsfb), out32, sync=True)
        _fp32_bar(out32.cpu().numpy(), ref, S)
        # the weight gradient: per-row sfb
        sfb_r = _per_row_sfb(sfb, n, seed=n)
        ref_r, S_r = _exact_rows(oracle, a, sfa, b, sfb_r)
        out32.fill_(float("nan"))
        dga.wgrad_gemm_fp8_fp8_fp32_nt((da, dsfa), (db, _dev(sfb_r)), out32, sync=True)
        _fp32_bar(out32.cpu().numpy(), ref_r, S_r)
        # the deep_gemm_cpp binding: its own default tilings
        from deepgemm_ascend_amd import deep_gemm_cpp as ext
        out = torch.full((m, n), float("nan"), dtype=torch.bfloat16, device="cuda")
        ext.gemm_fp8_fp8_bf16_nt(da, dsfa, db, dsfb, out)
        out32.fill_(float("nan"))
        ext.gemm_fp8_fp8_fp32_nt(da, dsfa, db, dsfb, out32)
        torch.cuda.synchronize()
        _bf16x_bar(oracle, _bits(out), want, a, sfa, b, sfb, k)
        _fp32_bar(out32.cpu().numpy(), ref, S)
        out32.fill_(float("nan"))
        ext.wgrad_gemm_fp8_fp8_fp32_nt(da, dsfa, db, _dev(sfb_r), out32)
        torch.cuda.synchronize()
        _fp32_bar(out32.cpu().numpy(), ref_r, S_r)


# (name, groups, m_max, n, k, expected_m, row maker): masked grouped problems under fast-class rows of the grouped key
def _grouped_sweep_row(g, mm, n, k):
    sweep = _sweep()
    prob = {"m": mm, "n": n, "k": k, "groups": g, "layout": "masked", "rows_per_group": mm}
    return sweep.GROUPED_CSV_HEAD, sweep.grouped_row(prob, sweep.grouped_candidates(prob)[0])


GROUPED_CASES = [
    ("leak_build1", 4, 64, 1024, 1024, 64, lambda g, mm, n, k: (_sweep().FULL_CSV_HEAD, f"{mm},{n},{k},64,128,128,0,0,0,0,32,1,3,1,0,0,0,{g},0,1\n")),
    ("leak_legacy_stages1", 4, 64, 1024, 1024, 64, lambda g, mm, n, k: (_sweep().GROUPED_CSV_HEAD, f"{mm},{n},{k},64,128,128,0,0,0,0,32,1,1,1,0,0,0,{g},0\n")),
    ("leak_build10", 4, 64, 1024, 1024, 64, lambda g, mm, n, k: (_sweep().FULL_CSV_HEAD, f"{mm},{n},{k},64,128,128,0,0,0,0,32,1,3,1,0,0,4,{g},0,10\n")),
    ("good_tall", 4, 128, 256, 1024, 128, _grouped_sweep_row),
    ("good_hint", 4, 128, 256, 192, 32, _grouped_sweep_row),
]


@pytest.mark.parametrize("name,g,mm,n,k,expected_m,make", GROUPED_CASES, ids=[c[0] for c in GROUPED_CASES])
def test_masked_grouped_default_under_a_cache_row(dga, oracle, tmp_path, name, g, mm, n, k, expected_m, make):
    head, row = make(g, mm, n, k)
    parts = [oracle.make_inputs(mm, n, k, seed=40 + i) for i in range(g)]
    A, SFA, B, SFB = (np.stack([p[j] for p in parts]) for j in range(4))
    masked = np.array([0, 1, mm // 2 + 1, mm][:g], np.int32)
    sentinel = np.full((g, mm, n), 0x7FC1, np.uint16)      # a NaN no kernel writes
    want = oracle.m_grouped_gemm_fp8_fp8_bf16_nt_masked(A, SFA, B, SFB, sentinel, masked, threads=4)
    with _Cache(dga, tmp_path / "rows.csv", head, [row]):
        t = dga.tiling(mm, n, k, groups=g, expected_m=expected_m, policy="bf16_exact")
        assert t.dispatchPolicyTag == 7 and dga.tiling_check(t) == 0, t.as_dict()
        out = torch.from_numpy(sentinel.copy().view(np.int16)).cuda().view(torch.bfloat16)
        dga.m_grouped_gemm_fp8_fp8_bf16_nt_masked((_dev(A), _dev(SFA)), (_dev(B), _dev(SFB)), out, _dev(masked), expected_m=expected_m,
                                                  sync=True)
        got = _bits(out)
    for i in range(g):
        r = int(masked[i])
        assert (got[i, r:] == 0x7FC1).all(), f"group {i}: rows >= masked_m were written"
        if r:
            _bf16x_bar(oracle, got[i, :r], want[i, :r], A[i, :r], SFA[i, :r], B[i], SFB[i], k)


STRICT_CODE = r"""
import sys, numpy as np, torch
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import deepgemm_ascend_amd as dga
from oracle import oracle as O
import test_cache_rows_gpu as G
assert dga.api.default_policy() == "strict"
for m, n, k in %(shapes)r:
    a, sfa, b, sfb = O.make_inputs(m, n, k, seed=m + n + k)
    out = torch.full((m, n), float("nan"), dtype=torch.bfloat16, device="cuda")
    rc = G._null_tiling_call(dga, *(G._dev(x) for x in (a, sfa, b, sfb)), out, m, n, k)
    same = rc == 0 and np.array_equal(G._bits(out), O.gemm_fp8_fp8_bf16_nt(a, sfa, b, sfb, threads=8))
    print(m, n, k, rc, same)
"""


def test_a_strict_process_default_is_bit_exact_under_the_same_rows(dga, oracle, tmp_path):
    """$DGA_DEFAULT_POLICY=strict in a child of its own, the defect rows as its $DGA_CACHE_FILE_PATH: the NULL-tiling C entry
    returns the oracle's bits whatever the rows name."""
    cases = [c for c in DENSE_CASES if c[0] in ("leak_64x1024x4096", "ue8m0_dense", "ue8m0_decode", "tail_off_its_tile")]
    path = tmp_path / "rows.csv"
    rows = []
    for _, m, n, k, make in cases:
        head, row = make(m, n, k)
        cells = row.strip().split(",")
        # (one file, the full header: a fast row's missing cells read as 0 -- groups 1, build 0, its legacy `stages` 1 still the build name)
        rows.append(",".join(cells + ["0"] * (20 - len(cells))) + "\n")
    path.write_text(_sweep().FULL_CSV_HEAD + "".join(rows))
    env = dict(os.environ, PYTHONPATH=str(ROOT), DGA_DEFAULT_POLICY="strict", DGA_CACHE_FILE_PATH=str(path))
    env.pop("CACHE_FILE_PATH", None)
    code = STRICT_CODE % {"root": str(ROOT), "tests": str(ROOT / "tests"), "shapes": [(m, n, k) for _, m, n, k, _ in cases]}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300, cwd=str(ROOT))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(cases) and all(ln.endswith(" 0 True") for ln in lines), r.stdout
