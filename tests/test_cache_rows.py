"""CPU: the default-policy tiling entries under every kind of (m,n,k) tiling-cache row.

A call that names no tiling reads the tiling cache first (tuned/mi355x.csv, $DGA_CACHE_FILE_PATH, dga_tiling_cache_open), and
dga_tiling_bf16_exact, dga_tiling_fp32_out and dga_tiling_wgrad build their tiling from that row.  Whatever the row says -- a fast-path
sweep winner, a bf16-exact one, a file from before the `build` column, a reference-format file, a row with the UE8M0 flag, a row
written by hand -- each entry must hand back a tiling its own check accepts (a row the policy's menu does not hold falls back to the
rules), with dispatchPolicyTag 7 and never the power-of-two-scales flag, which only the process default may add.  The rows are the
ones harness/sweep.py writes, through its own candidate enumerators and row writers.  Their GPU results: tests/test_cache_rows_gpu.py."""
import ctypes
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import deepgemm_ascend_amd as dga
from deepgemm_ascend_amd import _lib
from deepgemm_ascend_amd.api import Tiling
from deepgemm_ascend_amd.harness import sweep

ROOT = Path(__file__).resolve().parent.parent
UE8M0 = 16
REF_HEAD = "m,n,k,m1,n1,k1,kernelSerial,paddingTagA,paddingTagB,paddingTagC,blockDim\n"

# shapes named for the branch of dga_tiling_bf16_exact each takes without a cache row (the first test pins that): (name, m, n, k),
# and for the grouped layouts (name, m or m_max, n, k, groups, expected_m, contiguous)
DENSE = [("wsk", 8, 2112, 7168), ("wsk32", 24, 4096, 2048), ("dsk", 128, 4096, 7168), ("dsk320", 320, 2112, 7168),
         ("cost", 48, 2112, 7168), ("cost_split", 64, 1024, 4096), ("cost_small", 40, 512, 1024), ("cost_mid", 300, 520, 1024),
         ("cost_big", 1024, 4096, 4096), ("tail", 2304, 4096, 7168), ("streamk", 3511, 6151, 8191), ("odd_k", 100, 520, 1000)]
GROUPED = [("masked_tall", 128, 256, 1024, 4, 128, False), ("masked_hint", 128, 256, 192, 4, 32, False),
           ("masked_short", 64, 4096, 1024, 4, 64, False), ("contiguous", 512, 256, 1024, 4, 0, True)]


def _problem(m, n, k, groups=1, expected_m=0, contiguous=False):
    return dga.api._problem(m, n, k, groups, expected_m, contiguous=contiguous)


def _call(fn, p):
    t = Tiling()
    rc = getattr(_lib.lib(), fn)(ctypes.byref(p), ctypes.byref(t))
    return rc, t


def _check(fn, t):
    return int(getattr(_lib.lib(), fn)(ctypes.byref(t)))


def test_the_shapes_reach_every_branch_of_the_bf16_exact_tiling():
    """Without a cache row each shape lands where its name says: the rows below are laid over all of dga_tiling_bf16_exact."""
    dga.tiling_cache_open(None)
    dga.tiling_cache_clear()
    try:
        got = {name: dga.tiling(m, n, k, policy="bf16_exact") for name, m, n, k in DENSE}
        assert got["wsk"].kernelSerial == 6 and got["wsk"].build == 0 and got["wsk"].m1 == 16
        assert got["wsk32"].kernelSerial == 6 and got["wsk32"].m1 == 32
        for name in ("dsk", "dsk320"):
            assert (got[name].kernelSerial, got[name].build, got[name].m1, got[name].n1) == (6, 10, 64, 128), name
        for name in ("cost", "cost_small", "cost_mid", "cost_big", "odd_k"):
            assert got[name].kernelSerial in (0, 4) and got[name].build == 0, name
        assert got["cost_split"].splitkFactor > 1 or got["cost_mid"].splitkFactor > 1
        assert got["tail"].kernelSerial == 5 and got["streamk"].kernelSerial == 7
        g = {name: dga.tiling(m, n, k, groups=gr, expected_m=em, contiguous=c, policy="bf16_exact") for name, m, n, k, gr, em, c in GROUPED}
        assert g["masked_tall"].build == 9                                   # DGA_BUILD_BX_GROUPED
        assert (g["masked_hint"].m1, g["masked_hint"].n1, g["masked_hint"].build) == (32, 128, 0)
        assert g["masked_short"].m1 == 64 and g["contiguous"].contiguous == 1
    finally:
        dga.tiling_cache_clear()


# ---- the rows ---------------------------------------------------------------------------------------------------------------------

def _fast_sweep_rows(m, n, k):
    """Every dense fast-path candidate, as harness/sweep.py appends its winner (17 columns; a register workgroup split-K is `stages` 1)."""
    return [(sweep.FAST_CSV_HEAD, sweep.fast_row(m, n, k, p)) for p in sweep.candidates(m, n, k, rasters=[0])]


def _bx_sweep_rows(m, n, k):
    """Every bf16-exact candidate, as `sweep.py --arith bf16_exact` writes it (the full header, the build column)."""
    return [(sweep.FULL_CSV_HEAD, sweep.bx_row(m, n, k, p)) for p in sweep.candidates_bx(m, n, k)]


def _legacy(head, row):
    """The same row in a file from before the build column: a build name rides in `stages` (1, 4..9), build 10 has no such name."""
    cells = row.strip().split(",")
    build = int(cells[19]) if len(cells) > 19 else 0
    if build not in (0, 1, 4, 5, 6, 7, 8, 9):
        return None
    if build:
        cells[12] = str(build)
    return sweep.GROUPED_CSV_HEAD, ",".join(cells[:19]) + "\n"


def _tag23(head, row):
    cells = row.strip().split(",")
    cells[16] = str(int(cells[16]) | UE8M0)
    return head, ",".join(cells) + "\n"


def _grouped_sweep_rows(m, n, k, groups, contiguous):
    prob = {"m": m, "n": n, "k": k, "groups": groups, "layout": "contiguous" if contiguous else "masked", "rows_per_group": m // groups if contiguous else m}
    return [(sweep.GROUPED_CSV_HEAD, sweep.grouped_row(prob, c)) for c in sweep.grouped_candidates(prob)]


def _reference_rows(m, n, k):
    """Reference-format rows (11 columns): k1 = 256 on its tiles, kernel type 3 (PaddingStreamK), which has no build here."""
    out = []
    for m1, n1, k1, serial in ((128, 256, 256, 0), (256, 256, 256, 1), (128, 256, 512, 3), (256, 128, 1024, 4), (128, 128, 256, 0),
                               (64, 256, 256, 3), (16, 128, 256, 2)):
        out.append((REF_HEAD, f"{m},{n},{k},{m1},{n1},{k1},{serial},0,0,0,24\n"))
    return out


def _random_rows(m, n, k, groups, contiguous, count, seed):
    """Hand-written rows: any tile, schedule, split, stage count, wave grid, tag and build, in either class."""
    rng = np.random.default_rng(seed)
    tiles = sweep.TILES + [(64, 64), (512, 128)]
    out = []
    for _ in range(count):
        m1, n1 = tiles[int(rng.integers(len(tiles)))]
        serial = int(rng.choice([0, 1, 3, 4, 5, 6, 7, 9]))
        splitk = int(rng.choice([0, 1, 2, 4, 6, 8]))
        stages = int(rng.integers(0, 11))
        wm, wn = [(0, 0), (2, 2), (1, 4), (4, 2), (2, 4), (3, 3)][int(rng.integers(6))]
        tag = int(rng.choice([0, 1, 2, 3, 4, 5, 6, 7, 16, 18, 21, 23, 39]))
        build = int(rng.choice([0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 11]))
        k1 = int(rng.choice([0, 128, 256]))
        out.append((sweep.FULL_CSV_HEAD, f"{m},{n},{k},{m1},{n1},{k1},{serial},0,0,0,{int(rng.integers(0, 600))},{splitk},{stages},"
                                         f"{int(rng.integers(0, 9))},{wm},{wn},{tag},{groups},{1 if contiguous else 0},{build}\n"))
    return out


def _dense_rows(m, n, k, seed):
    fast = _fast_sweep_rows(m, n, k)
    fast += [(sweep.FULL_CSV_HEAD, r) for _, r in fast]
    bx = _bx_sweep_rows(m, n, k)
    legacy = [r for r in (_legacy(*x) for x in bx) if r]
    tag23 = [_tag23(*x) for x in bx]
    return {"fast": fast, "bx": bx, "legacy": legacy, "tag23": tag23, "reference": _reference_rows(m, n, k),
            "random": _random_rows(m, n, k, 1, False, 120, seed)}


class _Rows:
    """One row at a time as the open cache file; the global state is restored whatever happens."""
    def __init__(self, path):
        self.path = path

    def open(self, head, row):
        self.path.write_text(head + row)
        dga.tiling_cache_open(str(self.path))
        assert dga.tiling_cache_size() == 1, (head, row)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        dga.tiling_cache_open(None)
        dga.tiling_cache_clear()
        dga.api._PLANS.clear()
        return False


def _expected_fp32_tag():
    return 3 if dga.api.default_policy() == "strict" else 7


def _bad_default_entries(p, dense):
    """(entry, rc, check, tag, tiling) of every default-policy entry that hands back what its own check refuses or a tag it must not carry."""
    bad = []
    rc, t = _call("dga_tiling_bf16_exact", p)
    chk = _check("dga_tiling_check", t) if rc == 0 else None
    if rc or chk or t.dispatchPolicyTag != 7:
        bad.append(("bf16_exact", rc, chk, t.dispatchPolicyTag, t.as_dict()))
    if dense:
        for fn, check in (("dga_tiling_fp32_out", "dga_tiling_check_fp32_out"), ("dga_tiling_wgrad", "dga_tiling_check_wgrad")):
            rc, t = _call(fn, p)
            chk = _check(check, t) if rc == 0 else None
            if rc or chk or t.dispatchPolicyTag != _expected_fp32_tag():
                bad.append((fn, rc, chk, t.dispatchPolicyTag, t.as_dict()))
    return bad


@pytest.mark.parametrize("name,m,n,k", DENSE, ids=[d[0] for d in DENSE])
def test_every_cache_row_gives_the_dense_default_entries_a_tiling_they_accept(tmp_path, name, m, n, k):
    p = _problem(m, n, k)
    failures = {}
    with _Rows(tmp_path / "rows.csv") as rows:
        for kind, lst in _dense_rows(m, n, k, seed=m * 7 + n + k).items():
            assert lst, kind
            for head, row in lst:
                rows.open(head, row)
                bad = _bad_default_entries(p, dense=True)
                if bad:
                    failures.setdefault(kind, []).append((row.strip(), bad[0]))
    assert not failures, {kind: (len(v), v[:3]) for kind, v in failures.items()}


@pytest.mark.parametrize("name,m,n,k,groups,expected_m,contiguous", GROUPED, ids=[g[0] for g in GROUPED])
def test_every_cache_row_gives_the_grouped_bf16_exact_entry_a_tiling_it_accepts(tmp_path, name, m, n, k, groups, expected_m, contiguous):
    p = _problem(m, n, k, groups, expected_m, contiguous)
    kinds = {"fast": _grouped_sweep_rows(m, n, k, groups, contiguous)}
    # the register workgroup split-K's names (build 1 / legacy stages 1) and the decode build (10) on the grouped key
    c = 1 if contiguous else 0
    kinds["build_names"] = [(sweep.FULL_CSV_HEAD, f"{m},{n},{k},64,128,128,0,0,0,0,64,1,3,1,0,0,{tag},{groups},{c},{b}\n")
                            for tag in (0, 4, 7, 23) for b in (1, 10, 8, 9)]
    kinds["legacy"] = [(sweep.GROUPED_CSV_HEAD, f"{m},{n},{k},{m1},{n1},128,0,0,0,0,64,1,{st},1,0,0,{tag},{groups},{c}\n")
                       for (m1, n1) in ((64, 128), (128, 256), (16, 128)) for st in (1, 4, 5, 6, 7, 8, 9) for tag in (0, 7, 23)]
    kinds["random"] = _random_rows(m, n, k, groups, contiguous, 150, seed=groups * 31 + m + n)
    failures = {}
    with _Rows(tmp_path / "rows.csv") as rows:
        for kind, lst in kinds.items():
            assert lst, kind
            for head, row in lst:
                rows.open(head, row)
                bad = _bad_default_entries(p, dense=False)
                if bad:
                    failures.setdefault(kind, []).append((row.strip(), bad[0]))
    assert not failures, {kind: (len(v), v[:3]) for kind, v in failures.items()}


@pytest.mark.parametrize("name,m,n,k", DENSE, ids=[d[0] for d in DENSE])
def test_the_fast_tiling_of_a_swept_or_reference_row_passes_the_check(tmp_path, name, m, n, k):
    """The opt-in fast policy keeps a well-formed row's pick; what it hands back for a row a sweep wrote (now or before the build
    column) or for a reference-format row is a tiling the launcher takes."""
    p = _problem(m, n, k)
    fast = _fast_sweep_rows(m, n, k)
    # (a fast sweep appends its 17 columns to a file with the full header, too: the missing cells read as 0)
    kinds = {"fast": fast, "fast_in_full_file": [(sweep.FULL_CSV_HEAD, r) for _, r in fast], "reference": _reference_rows(m, n, k)}
    failures = {}
    with _Rows(tmp_path / "rows.csv") as rows:
        for kind, lst in kinds.items():
            for head, row in lst:
                rows.open(head, row)
                rc, t = _call("dga_tiling", p)
                chk = _check("dga_tiling_check", t) if rc == 0 else None
                if rc or chk or (t.dispatchPolicyTag & 15) in (3, 7):
                    failures.setdefault(kind, []).append((row.strip(), rc, chk, t.as_dict()))
    assert not failures, {kind: (len(v), v[:3]) for kind, v in failures.items()}


def test_a_bf16_exact_row_the_menu_holds_is_still_taken(tmp_path):
    """A well-formed tag-7 row is what the default call runs (the fallback is for rows the check refuses): tile, split, schedule, build."""
    with _Rows(tmp_path / "rows.csv") as rows:
        for (m, n, k), row, want in (
                ((300, 520, 1024), "64,256,128,4,0,0,0,30,2,3,1,0,0,7,1,0,0", (64, 256, 4, 2, 0)),
                ((128, 4096, 7168), "64,128,128,6,0,0,0,256,4,3,1,0,0,7,1,0,10", (64, 128, 6, 4, 10)),
                ((2304, 4096, 7168), "128,256,128,5,0,0,0,352,1,3,1,0,0,7,1,0,0", (128, 256, 5, 1, 0)),
                ((1024, 4096, 4096), "128,256,128,0,0,0,0,128,1,3,2,0,0,23,1,0,8", (128, 256, 0, 1, 8))):
            rows.open(sweep.FULL_CSV_HEAD, f"{m},{n},{k},{row}\n")
            t = dga.tiling(m, n, k, policy="bf16_exact")
            assert (t.m1, t.n1, t.kernelSerial, t.splitkFactor, t.build) == want, (row, t.as_dict())
            assert t.dispatchPolicyTag == 7 and dga.tiling_check(t) == 0


# ---- null-tiling resolution under each process default ----------------------------------------------------------------------------

# (m, n, k, row): a tag-23 decode row the "auto" policy takes, a tag-23 dense row, a fast sweep row of the register workgroup split-K
# (legacy stages 1), fast rows with the UE8M0 flag (and build 1), a bf16-exact row naming build 10 off its tile
PLAN_ROWS = [(24, 4096, 2048, "32,128,128,6,0,0,0,256,1,3,1,0,0,23,1,0,0"),
             (1024, 4096, 4096, "128,256,128,0,0,0,0,512,1,3,2,0,0,23,1,0,0"),
             (64, 1024, 4096, "64,128,128,6,0,0,0,8,1,1,1,0,0,0,1,0,0"),
             (40, 512, 1024, "32,128,128,6,0,0,0,4,1,3,1,0,0,16,1,0,1"),
             (300, 520, 1024, "128,128,128,0,0,0,0,15,1,3,1,0,0,20,1,0,0"),
             (256, 1024, 2048, "128,128,128,6,0,0,0,32,4,3,1,0,0,7,1,0,10")]

PLAN_CODE = r"""
import json, deepgemm_ascend_amd as d
from deepgemm_ascend_amd import api
shapes = json.loads(%r)
out = []
for m, n, k in shapes:
    t = api._planned(0, m, n, k, 1, 0, False, False, None)
    a = api._planned(0, m, n, k, 1, 0, False, False, "auto")
    f = api._planned_fp32_out(0, m, n, k, False, None, False)
    w = api._planned_fp32_out(0, m, n, k, False, None, True)
    out.append({"tag": t.dispatchPolicyTag, "check": api.tiling_check(t), "auto": a.dispatchPolicyTag, "auto_serial": a.kernelSerial,
                "auto_check": api.tiling_check(a), "fp32": f.dispatchPolicyTag, "fp32_check": api.tiling_check_fp32_out(f),
                "wgrad": w.dispatchPolicyTag, "wgrad_check": api.tiling_check_wgrad(w)})
print(json.dumps(out))
"""


@pytest.mark.parametrize("policy", [None, "fast", "bf16_exact", "strict", "fast_ue8m0", "bf16_exact_ue8m0", "auto"])
def test_null_tiling_plans_carry_the_process_default_never_the_row(tmp_path, policy):
    """Each process default in a child of its own ($DGA_DEFAULT_POLICY is read once), with the rows as its $DGA_CACHE_FILE_PATH:
    the planned tilings of the bf16, fp32 and wgrad entries carry the tag of the process default (or of "auto"), pass their checks,
    and never carry the UE8M0 flag or a schedule tag a cache row imposed."""
    import json
    path = tmp_path / "rows.csv"
    path.write_text(sweep.FULL_CSV_HEAD + "".join(f"{m},{n},{k},{row}\n" for m, n, k, row in PLAN_ROWS))
    env = dict(os.environ, PYTHONPATH=str(ROOT), DGA_CACHE_FILE_PATH=str(path))
    env.pop("DGA_DEFAULT_POLICY", None)
    env.pop("CACHE_FILE_PATH", None)
    if policy is not None:
        env["DGA_DEFAULT_POLICY"] = policy
    shapes = [[m, n, k] for m, n, k, _ in PLAN_ROWS]
    r = subprocess.run([sys.executable, "-c", PLAN_CODE % json.dumps(shapes)], capture_output=True, text=True, env=env, timeout=300,
                       cwd=str(ROOT))
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    name = policy or "bf16_exact"
    for (m, n, k, row), g in zip(PLAN_ROWS, got):
        ctx = (name, (m, n, k), row, g)
        assert g["check"] == 0 and g["auto_check"] == 0 and g["fp32_check"] == 0 and g["wgrad_check"] == 0, ctx
        assert g["fp32"] == g["wgrad"] == (3 if name == "strict" else 7), ctx
        fast_class = lambda tag: (tag & 15) not in (3, 7)
        if name == "bf16_exact":
            assert g["tag"] == 7, ctx
        elif name == "bf16_exact_ue8m0":
            assert g["tag"] == 7 | UE8M0, ctx
        elif name == "strict":
            assert g["tag"] == 3, ctx
        elif name == "fast":
            assert fast_class(g["tag"]) and not g["tag"] & UE8M0, ctx
        elif name == "fast_ue8m0":
            assert fast_class(g["tag"]) and g["tag"] & UE8M0, ctx
        # policy="auto" (and an "auto" process default): bf16-exact on the decode kernel, the fast path elsewhere -- never the flag
        if g["auto_serial"] == 6 and (g["auto"] & 15) == 7:
            assert g["auto"] == 7, ctx
        else:
            assert fast_class(g["auto"]) and not g["auto"] & UE8M0, ctx
        if name == "auto":
            assert g["tag"] == g["auto"], ctx
