"""CPU: split-topk sparse MLA decode.  The float64 reference of partials and merge (tests/sparse_mla_split_ref.py) against the one-pass
reference, the split ranges and the split rule, the four C entries declared, exported and in the ctypes table, their refusals in the
documented order (none of which launches), every refusal the wrappers make, the resources of the new kernels, and the checkers the GPU tests
use, each fed a corrupted result it must reject."""
import ctypes
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import sparse_mla_ref as R
import sparse_mla_split_ref as X
from sparse_mla_support import _aligned, _bad_caches, _cache, _refused
from sparse_mla_support import _args as _short_args

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "deepgemm_ascend_amd" / "csrc"
MIN_TILES = 4                                                           # DGA_SPARSE_MLA_MIN_TILES


# ---- the reference -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", (1, 2, 3, 10))
def test_merged_partials_are_the_one_pass_reference(p):
    q, kv, idx = R.random_case(16)
    ref = R.reference(q, kv, idx, R.SCALE4)
    parts = X.partials(q, kv, idx, R.SCALE4, p)
    assert parts["P"] == p and parts["out"].shape == (p, R.M4, 16, R.D_V) and parts["lse"].shape == (p, R.M4, 16)
    merged = X.merge(parts["out"], parts["lse"])
    assert np.allclose(merged["out"], ref["out"], rtol=1e-12, atol=1e-13) and np.allclose(merged["lse"], ref["lse"], rtol=1e-13, atol=0)
    assert np.allclose((np.exp(parts["lse"] - ref["lse"])[..., None] * parts["A"]).sum(axis=0), ref["A"], rtol=1e-12)   # sum_p W_p A_p = A
    assert (merged["A"] <= ref["A"] * (1 + 1e-12)).all()
    # a list whose second half is padding: the second split is empty and weighs nothing
    half = idx.copy()
    half[:, 160:] = -1
    parts = X.partials(q, kv, half, R.SCALE4, 2)
    merged, first = X.merge(parts["out"], parts["lse"]), R.reference(q, kv, half[:, :160], R.SCALE4)
    assert np.isneginf(parts["lse"][1]).all() and not parts["out"][1].any()
    assert np.array_equal(merged["out"], first["out"]) and np.array_equal(merged["lse"], first["lse"])


def test_merge_of_nothing_is_plus_zero_and_minus_infinity():
    po, pl = np.zeros((3, 2, 16, R.D_V)), np.full((3, 2, 16), -np.inf)
    pl[1, 0], po[1, 0] = 2.0, 7.0
    m = X.merge(po, pl)
    assert np.isneginf(m["lse"][1]).all() and not m["out"][1].any() and not np.signbit(m["out"][1]).any()
    assert (m["lse"][0] == 2.0).all() and (m["out"][0] == 7.0).all()


def test_split_ranges_cover_every_tile_once():
    for tiles in range(1, 71):
        for p in range(1, min(tiles, 64) + 1):
            r = X.split_ranges(tiles, p)
            assert r[0][0] == 0 and r[-1][1] == tiles and all(a[1] == b[0] for a, b in zip(r, r[1:])) and all(lo < hi for lo, hi in r)
            assert max(hi - lo for lo, hi in r) == -(-tiles // p)
    assert X.effective_splits(160, 64) == 5 and X.effective_splits(161, 64) == 6 and X.effective_splits(2048, 64) == 64


# ---- the rule ------------------------------------------------------------------------------------------------------------------------

RULE_TABLE = [(m, heads, topk, cus) for m in (1, 2, 3, 4, 7, 16, 17, 64, 128, 129, 256, 300) for heads in (16, 64, 80, 128)
              for topk in (1, 32, 100, 128, 255, 256, 2048, 2049, 8192) for cus in (1, 64, 256, 304)]


def test_the_split_rule(dga):
    from deepgemm_ascend_amd import _lib
    L = _lib.lib()
    for m, heads, topk, cus in RULE_TABLE:
        got = L.dga_sparse_mla_splits(m, heads, topk, cus)
        hb, tiles = -(-heads // 64), X.tiles_of(topk)
        assert got == X.num_splits_rule(m, heads, topk, cus, MIN_TILES), (m, heads, topk, cus)
        assert 1 <= got <= min(tiles, 64)
        if m * hb >= cus or tiles < 2 * MIN_TILES:
            assert got == 1
        if m > 1:
            assert got <= L.dga_sparse_mla_splits(m - 1, heads, topk, cus)                 # monotone non-increasing in m
    assert L.dga_sparse_mla_splits(1, 128, 2048, 256) == 16 and L.dga_sparse_mla_splits(16, 128, 2048, 256) == 8
    assert L.dga_sparse_mla_splits(64, 128, 2048, 256) == 2 and L.dga_sparse_mla_splits(128, 128, 2048, 256) == 1
    assert L.dga_sparse_mla_splits(1, 16, 1 << 20, 1 << 20) == 64
    assert L.dga_sparse_mla_splits(0, 128, 2048, 256) == 1 == L.dga_sparse_mla_splits(1, 0, 2048, 256) == L.dga_sparse_mla_splits(1, 16, 0, 256)
    assert L.dga_sparse_mla_splits(1 << 62, 128, 1 << 62, 256) == 1
    # without a device the library's CU count is the whole MI355X's; the wrapper applies the same rule
    assert dga.sparse_mla_num_splits(300, 128, 2048) == 1 and 1 <= dga.sparse_mla_num_splits(1, 128, 2048) <= 16
    for bad in ((0, 16, 32), (1, 16, 0), (1.0, 16, 32)):
        with pytest.raises(dga.DGAError):
            dga.sparse_mla_num_splits(*bad)


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------

ENTRIES = {"dga_sparse_mla_fwd_partial": 17, "dga_sparse_mla_fwd_fp8_partial": 18, "dga_sparse_mla_merge": 8, "dga_sparse_mla_splits": 4}


def test_symbols_are_declared_exported_and_in_the_table(dga):
    from deepgemm_ascend_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "dga_hip.h").read_text(), flags=re.S)
    so = ctypes.CDLL(str(_lib.LIB_PATH))
    for name, n in ENTRIES.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(", text) and hasattr(so, name), name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == n, name
    assert re.search(r"#define\s+DGA_SPARSE_MLA_MAX_SPLITS\s+64\b", text) and re.search(r"#define\s+DGA_SPARSE_MLA_MIN_TILES\s+%d\b" % MIN_TILES, text)
    for name in ("sparse_mla_fwd_partial", "sparse_mla_fwd_fp8_partial", "sparse_mla_merge", "sparse_mla_num_splits", "sparse_mla_fwd_split",
                 "sparse_mla_fwd_fp8_split"):
        assert name in dga.__all__ and callable(getattr(dga, name)), name
    assert dga.SPARSE_MLA_MAX_SPLITS == 64 == X.MAX_SPLITS
    assert _lib.lib().dga_abi_version() == 7                            # the change only adds


def test_partial_c_entries_check_in_the_documented_order_before_any_launch(dga):
    """the one-pass entries' refusals with their statuses, then num_splits, then the partial pointers; none touches a device"""
    from deepgemm_ascend_amd import _lib
    L = _lib.lib()
    buf, p = _aligned()
    eff = ctypes.c_int(-7)

    def bf16(q=p, kv=p, idx=p, off=None, m=1, heads=16, s=4, kv_stride=576, topk=2, idx_stride=2, flags=0, splits=1, po=p, pl=p):
        return L.dga_sparse_mla_fwd_partial(q, kv, idx, off, m, heads, s, kv_stride, topk, idx_stride, 0.1, flags, splits, ctypes.byref(eff), po, pl, None)

    def fp8(q=p, kv=p, idx=p, off=None, m=1, heads=16, nb=2, page=4, stride=4 * 656, topk=2, idx_stride=2, flags=0, splits=1, po=p, pl=p):
        return L.dga_sparse_mla_fwd_fp8_partial(q, kv, idx, off, m, heads, nb, page, stride, topk, idx_stride, 0.1, flags, splits,
                                                ctypes.byref(eff), po, pl, None)

    one = lambda **kw: L.dga_sparse_mla_fwd(kw.get("q", p), kw.get("kv", p), p, None, kw.get("m", 1), kw.get("heads", 16), kw.get("s", 4), 576, 2, 2,
                                            0.1, kw.get("flags", 0), p, p, None)
    shape, null, align, rng = one(heads=8), one(q=None), one(kv=p + 8), one(flags=2)
    assert len({0, shape, null, align, rng}) == 5
    for call, shapes, aligns, ranges in (
            (bf16, (dict(m=-1), dict(heads=8), dict(heads=144), dict(heads=24), dict(s=0), dict(topk=0), dict(kv_stride=575), dict(idx_stride=1)),
             (dict(kv=p + 8), dict(q=p + 2), dict(off=p + 1), dict(kv_stride=580), dict(idx=p + 2)), (dict(flags=2), dict(s=1 << 31))),
            (fp8, (dict(m=-1), dict(heads=8), dict(nb=0), dict(page=0), dict(topk=0), dict(stride=4 * 656 - 16), dict(idx_stride=1), dict(page=1 << 62)),
             (dict(kv=p + 8), dict(q=p + 2), dict(off=p + 1), dict(stride=4 * 656 + 8)), (dict(flags=2), dict(nb=1 << 29, page=4)))):
        assert {call(**kw) for kw in shapes} == {shape}
        assert call(m=0) == 0 and call(m=0, q=None, kv=None, po=None, pl=None, splits=0) == 0           # M == 0 before anything else
        assert {call(q=None), call(idx=None), call(kv=None)} == {null}
        assert {call(**kw) for kw in aligns} == {align}
        assert {call(**kw) for kw in ranges} == {rng}
        # the order: a bad flag before a bad shape before a null before a misalignment before the one-pass ranges before num_splits ...
        assert call(flags=2, heads=8) == rng and call(heads=8, q=None) == shape and call(q=None, kv=p + 8) == null
        assert call(kv=p + 8, splits=0) == align
        assert call(splits=0) == rng == call(splits=65) == call(splits=-1) == call(splits=0, po=None)
        # ... before the partial pointers: null, then alignment
        assert call(po=None) == null == call(pl=None) == call(po=None, pl=p + 2)
        assert call(po=p + 8) == align == call(pl=p + 2) == call(po=p + 4)
        assert eff.value == -7                                           # (nothing was written on the way)
    assert bf16(m=(1 << 31) // 4, splits=64, topk=64 * 32, idx_stride=64 * 32) == rng       # the grid counts the splits
    assert bf16(m=(1 << 31) // 4, splits=64, topk=2, idx_stride=2, q=None) == null         # ... the effective ones: topk = 2 is one tile


def test_merge_c_entry_checks_shape_null_alignment_range(dga):
    from deepgemm_ascend_amd import _lib
    L = _lib.lib()
    buf, p = _aligned()

    def call(po=p, pl=p, splits=2, m=1, heads=16, out=p, lse=p):
        return L.dga_sparse_mla_merge(po, pl, splits, m, heads, out, lse, None)

    shape = call(m=-1)
    assert shape != 0 and {call(heads=8), call(heads=144), call(heads=24), call(splits=0), call(splits=65)} == {shape}
    assert call(m=0) == 0 and call(m=0, po=None, pl=None, out=None, lse=None) == 0
    null = call(po=None)
    assert null not in (0, shape) and null == call(pl=None) == call(out=None) == call(lse=None) == call(po=None, pl=p + 2)
    assert call(po=None, heads=8) == shape
    align = call(po=p + 8)
    assert align not in (0, shape, null) and align == call(out=p + 8) == call(pl=p + 2) == call(lse=p + 2)
    rng = call(m=1 << 40)
    assert rng not in (0, shape, null, align) and rng == call(m=1 << 52, splits=64, heads=128) and call(m=1 << 40, po=p + 8) == align


# ---- the wrappers --------------------------------------------------------------------------------------------------------------------

def _args(m=2, h=16, s=8, topk=70):                                     # (three tiles: num_splits up to 3 is the effective P)
    return _short_args(m, h, s, topk)


def _operand_refusals(fn, q, kv, idx, bad_kv, *more):
    """what every one of the attention forms refuses about q, kv, indices and offsets; fn(q, kv, idx, scale, *more, **kw)"""
    bad = {
        "q dtype": lambda: fn(q.float(), kv, idx, 0.1, *more),
        "q rank": lambda: fn(q[0], kv, idx, 0.1, *more),
        "q not contiguous": lambda: fn(torch.zeros((2, 32, 576), dtype=torch.bfloat16)[:, ::2], kv, idx, 0.1, *more),
        "Hq = 24": lambda: fn(_args(h=24)[0], kv, idx, 0.1, *more),
        "Hq = 144": lambda: fn(_args(h=144)[0], kv, idx, 0.1, *more),
        "d_v": lambda: fn(q, kv, idx, 0.1, *more, d_v=576),
        "sm_scale": lambda: fn(q, kv, idx, "0.1", *more),
        "indices dtype": lambda: fn(q, kv, idx.long(), 0.1, *more),
        "indices rows": lambda: fn(q, kv, idx[:1], 0.1, *more),
        "indices empty": lambda: fn(q, kv, idx[:, :0], 0.1, *more),
        "indices last dimension strided": lambda: fn(q, kv, torch.zeros((2, 140), dtype=torch.int32)[:, ::2], 0.1, *more),
        "offsets dtype": lambda: fn(q, kv, idx, 0.1, *more, index_offsets=torch.zeros(2, dtype=torch.int64)),
        "offsets shape": lambda: fn(q, kv, idx, 0.1, *more, index_offsets=torch.zeros(3, dtype=torch.int32)),
    }
    for what, c in bad_kv.items():
        bad[what] = (lambda c: lambda: fn(q, c, idx, 0.1, *more))(c)
    return bad


BAD_KV = {"kv dtype": torch.zeros((8, 576), dtype=torch.float16), "kv d": torch.zeros((8, 512), dtype=torch.bfloat16),
          "kv stride 580": torch.zeros((8, 580), dtype=torch.bfloat16)[:, :576], "kv empty": torch.zeros((0, 576), dtype=torch.bfloat16),
          "an fp8 cache": _cache()}
BAD_CACHE = {**_bad_caches(), "a bf16 cache": torch.zeros((8, 576), dtype=torch.bfloat16)}


@pytest.mark.parametrize("cache", ("bf16", "fp8"))
def test_every_partial_and_split_refusal_comes_from_the_wrapper(dga, cache):
    q, kv, idx = _args()
    if cache == "fp8":
        kv, bad_kv, partial, split = _cache(), BAD_CACHE, dga.sparse_mla_fwd_fp8_partial, dga.sparse_mla_fwd_fp8_split
    else:
        bad_kv, partial, split = BAD_KV, dga.sparse_mla_fwd_partial, dga.sparse_mla_fwd_split
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32)
    bad = _operand_refusals(partial, q, kv, idx, bad_kv, 2)
    bad.update({
        "num_splits 0": lambda: partial(q, kv, idx, 0.1, 0),
        "num_splits 65": lambda: partial(q, kv, idx, 0.1, 65),
        "num_splits 2.0": lambda: partial(q, kv, idx, 0.1, 2.0),
        "num_splits True": lambda: partial(q, kv, idx, 0.1, True),
        "num_splits None": lambda: partial(q, kv, idx, 0.1, None),
        "partial_out dtype": lambda: partial(q, kv, idx, 0.1, 2, partial_out=torch.zeros((2, 2, 16, 512), dtype=torch.bfloat16)),
        "partial_out too few splits": lambda: partial(q, kv, idx, 0.1, 3, partial_out=f32(2, 2, 16, 512)),
        "partial_out shape": lambda: partial(q, kv, idx, 0.1, 2, partial_out=f32(2, 2, 16, 576)),
        "partial_out rank": lambda: partial(q, kv, idx, 0.1, 2, partial_out=f32(2, 16, 512)),
        "partial_out strided": lambda: partial(q, kv, idx, 0.1, 2, partial_out=f32(4, 2, 16, 512)[::2]),
        "partial_lse dtype": lambda: partial(q, kv, idx, 0.1, 2, partial_lse=torch.zeros((2, 2, 16), dtype=torch.float64)),
        "partial_lse shape": lambda: partial(q, kv, idx, 0.1, 2, partial_lse=f32(2, 2, 16, 1)),
        "partial_lse too few splits": lambda: partial(q, kv, idx, 0.1, 3, partial_lse=f32(2, 2, 16)),
    })
    for what, call in _operand_refusals(split, q, kv, idx, bad_kv).items():                  # num_splits=None: the rule, then the one-pass checks
        bad["split, " + what] = call
    for what, call in _operand_refusals(lambda *a, **kw: split(*a, num_splits=3, **kw), q, kv, idx, bad_kv).items():
        bad["split 3, " + what] = call
    bad.update({
        "split num_splits 0": lambda: split(q, kv, idx, 0.1, num_splits=0),
        "split num_splits 65": lambda: split(q, kv, idx, 0.1, num_splits=65),
        "split num_splits 1.5": lambda: split(q, kv, idx, 0.1, num_splits=1.5),
        "split out shape": lambda: split(q, kv, idx, 0.1, num_splits=2, out=torch.zeros((2, 16, 576), dtype=torch.bfloat16)),
        "split out dtype": lambda: split(q, kv, idx, 0.1, num_splits=1, out=f32(2, 16, 512)),
        "split lse shape": lambda: split(q, kv, idx, 0.1, num_splits=2, lse=f32(2, 16, 1)),
        "split lse dtype": lambda: split(q, kv, idx, 0.1, lse=torch.zeros((2, 16), dtype=torch.bfloat16)),
    })
    _refused(dga, bad, (lambda: partial(q, kv, idx, 0.1, 2),
                        lambda: partial(q, kv, idx, 0.1, 64, 512, torch.zeros(2, dtype=torch.int32), f32(64, 2, 16, 512), f32(3, 2, 16)),   # 3 tiles
                        lambda: partial(q, kv, idx.view(2, 1, 70), 0.1, 1),
                        lambda: split(q, kv, idx, 0.1),
                        lambda: split(q, kv, idx, 0.1, num_splits=1),
                        lambda: split(q, kv, idx, 0.1, 512, torch.zeros(2, dtype=torch.int32), 64, torch.zeros((2, 16, 512), dtype=torch.bfloat16),
                                      f32(2, 16))))


def test_every_merge_refusal_comes_from_the_wrapper(dga):
    f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32)
    po, pl = f32(3, 2, 16, 512), f32(3, 2, 16)
    bad = {
        "partial_out dtype": lambda: dga.sparse_mla_merge(po.double(), pl),
        "partial_out rank": lambda: dga.sparse_mla_merge(po[0], pl),
        "partial_out width": lambda: dga.sparse_mla_merge(f32(3, 2, 16, 576), pl),
        "partial_out strided": lambda: dga.sparse_mla_merge(f32(6, 2, 16, 512)[::2], pl),
        "no split": lambda: dga.sparse_mla_merge(po[:0], pl[:0]),
        "65 splits": lambda: dga.sparse_mla_merge(torch.empty((65, 2, 16, 512), dtype=torch.float32, device="meta"), f32(65, 2, 16)),
        "Hq = 24": lambda: dga.sparse_mla_merge(f32(3, 2, 24, 512), f32(3, 2, 24)),
        "Hq = 144": lambda: dga.sparse_mla_merge(f32(1, 1, 144, 512), f32(1, 1, 144)),
        "partial_lse dtype": lambda: dga.sparse_mla_merge(po, pl.double()),
        "partial_lse splits": lambda: dga.sparse_mla_merge(po, f32(2, 2, 16)),
        "partial_lse strided": lambda: dga.sparse_mla_merge(po, f32(3, 2, 32)[..., ::2]),
        "partial_out misaligned": lambda: dga.sparse_mla_merge(f32(3 * 2 * 16 * 512 + 1)[1:].view(3, 2, 16, 512), pl),
        "out shape": lambda: dga.sparse_mla_merge(po, pl, out=torch.zeros((2, 16, 576), dtype=torch.bfloat16)),
        "out dtype": lambda: dga.sparse_mla_merge(po, pl, out=f32(2, 16, 512)),
        "lse shape": lambda: dga.sparse_mla_merge(po, pl, lse=f32(3, 2, 16)),
        "lse dtype": lambda: dga.sparse_mla_merge(po, pl, lse=torch.zeros((2, 16), dtype=torch.float16)),
    }
    _refused(dga, bad, (lambda: dga.sparse_mla_merge(po, pl), lambda: dga.sparse_mla_merge(po[:1], pl[:1]),
                        lambda: dga.sparse_mla_merge(f32(64, 1, 128, 512), f32(64, 1, 128), torch.zeros((1, 128, 512), dtype=torch.bfloat16), f32(1, 128))))


# ---- resources -----------------------------------------------------------------------------------------------------------------------

def test_the_new_kernels_have_no_scratch_no_spills_and_at_most_256_vgprs():
    """The kernel text has two caches and the PARTIAL axis: four instantiations, of which the two PARTIAL ones are new; and the merge."""
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{ROOT / 'include'}", f"-I{CSRC}", "-fno-slp-vectorize", "-mllvm",
             "-amdgpu-mfma-vgpr-form=1", "-x", "hip", "--cuda-device-only", "-S", "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"]
    make = (CSRC / "Makefile").read_text()
    assert "dga_sparse_mla.hip" in make and "dga_sparse_mla_merge.hip" in make and "NOFORM_dga_sparse_mla" not in make and "FLAGS_dga_sparse_mla" not in make
    seen = {}
    for unit in ("dga_sparse_mla.hip", "dga_sparse_mla_merge.hip"):
        r = subprocess.run(["/opt/rocm/bin/hipcc", *flags, str(CSRC / unit)], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        for block in r.stderr.split("Function Name: ")[1:]:
            get = lambda key: int(re.search(re.escape(key) + r": (\d+)", block).group(1))
            seen[block.split()[0]] = (get("VGPRs"), get("ScratchSize [bytes/lane]"), get("SGPRs Spill"), get("VGPRs Spill"))
    new = {k: v for k, v in seen.items() if "ELb1E" in k or "sparse_mla_merge_kernel" in k}
    assert len(seen) == 5 and len(new) == 3 and sum("SmlaBf16Rows" in k for k in new) == 1 and sum("SmlaFp8Rows" in k for k in new) == 1
    for name, (vgprs, scratch, sspill, vspill) in new.items():
        assert vgprs <= 256 and scratch == 0 and sspill == 0 and vspill == 0, (name, vgprs, scratch, sspill, vspill)


# ---- the GPU tests' checkers reject corrupted results ---------------------------------------------------------------------------------

def test_the_bound_checkers_reject_corrupted_results():
    h, p = 16, 3
    q, kv, idx = R.random_case(h)
    ref = R.reference(q, kv, idx, R.SCALE4)
    parts = X.partials(q, kv, idx, R.SCALE4, p)
    merged = X.merge(parts["out"], parts["lse"])
    bo = X.bound_out(ref, R.SCALE4, R.TOPK4, p, merged["maxlse"])
    bl = X.bound_lse(ref, R.SCALE4, R.TOPK4, p, merged["maxlse"])
    assert bo.shape == ref["out"].shape and bl.shape == ref["lse"].shape
    # the addition to the one-pass bars is what the derivation says: a few hundred u, far below 2^-8
    assert (bo >= R.bound_out(ref, R.SCALE4, R.TOPK4)).all() and 100 * X.U < X.c_merge(R.TOPK4, p, merged["maxlse"]).max() < 2.0 ** -12
    assert 500 * X.U < np.max(X.c_merge(2048, 2, 20.0)) < 2500 * X.U
    good_out, good_lse = R.bf16_round(merged["out"].astype(np.float32)), merged["lse"].astype(np.float32)
    assert X.worst_ratio(good_out, ref["out"], bo) < 1 and X.worst_ratio(good_lse, ref["lse"], bl) < 1
    # two splits swapped in partial_lse alone: each split's rows weighed with the other's weight
    swapped = X.merge(parts["out"], parts["lse"][[1, 0, 2]])
    assert X.worst_ratio(swapped["out"], ref["out"], bo) > 1
    # one partial's lse off by an ulp of a weight (2^-8, a bf16 ulp): lse moves by W_p 2^-8, far outside its bar
    off = parts["lse"].copy()
    off[1] += 2.0 ** -8
    moved = X.merge(parts["out"], off)
    assert X.worst_ratio(moved["lse"], ref["lse"], bl) > 1
    # one head's row moved to its neighbour
    rolled = good_out.copy()
    rolled[3, [4, 5]] = good_out[3, [5, 4]]
    assert X.worst_ratio(rolled, ref["out"], bo) > 1
    # -inf and NaN must stand where the reference has them
    bad = good_lse.copy()
    bad[0, 0] = -np.inf
    assert X.worst_ratio(bad, ref["lse"], bl) == np.inf
    bad = good_out.copy()
    bad[0, 0, 0] = np.nan
    assert X.worst_ratio(bad, ref["out"], bo) == np.inf
    # the merge's own share, on exact partials
    po32, pl32 = parts["out"].astype(np.float32), parts["lse"].astype(np.float32)
    m32 = X.merge(po32, pl32)
    assert X.worst_ratio(R.bf16_round(m32["out"].astype(np.float32)), m32["out"], X.merge_bound_out(m32, p)) < 1
    assert X.worst_ratio(X.merge(po32[[1, 0, 2]], pl32)["out"], m32["out"], X.merge_bound_out(m32, p)) > 1
    assert X.worst_ratio(m32["lse"] + 2.0 ** -16, m32["lse"], X.merge_bound_lse(m32, p)) > 1


@pytest.mark.parametrize("p", (2, 3, 5))
def test_the_winning_split_checker_rejects_swapped_splits_and_heads(p):
    h = 48
    q, kv, idx, scale, win = R.winners_case(h)
    ws = X.winner_splits(idx, win, p)
    assert ws.shape == (R.WIN_M, h) and set(np.unique(ws)) == set(range(p))                  # every split holds somebody's winner
    parts = X.partials(q, kv, idx, scale, p)
    pl = X.f32_bits(parts["lse"])
    lse = X.f32_bits(np.take_along_axis(parts["lse"], ws[None], axis=0)[0])
    assert (np.take_along_axis(parts["lse"], ws[None], axis=0)[0] == 512.0).all()           # the winner's split: exactly 512
    others = parts["lse"][np.arange(p)[:, None, None] != ws[None]]
    assert (others <= np.log(R.WIN_TOPK)).all() and np.exp(np.float32(np.log(R.WIN_TOPK) - 512.0)) == 0           # weights exactly 0 in fp32
    assert X.heads_off_their_winning_split(lse, pl, ws) == []
    assert len(X.heads_off_their_winning_split(lse, pl[np.roll(np.arange(p), 1)], ws)) == R.WIN_M * h             # the splits rotated
    bad = lse.copy()
    bad[1, [3, 7]] = pl[(ws[1, 3] + 1) % p, 1, 3], lse[1, 7] ^ 1                              # another split's slot; one bit
    assert X.heads_off_their_winning_split(bad, pl, ws) == [(1, 3), (1, 7)]
    # and the row checker of the one-pass tests tells a row in another split's, head's or token's slot apart
    bits = R.winner_bits(kv, win)
    moved = bits.copy()
    moved[0, [1, 2]] = bits[0, [2, 1]]
    assert R.heads_off_their_winner(moved, kv, win) == [(0, 1), (0, 2)]
