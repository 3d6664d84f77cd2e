"""What the fp8 tiling selectors return, case by case (tests/test_selector_golden.py compares it with tests/golden/selector_golden.json).
A helper module, not a conftest: the case lists, the dump (run in a child process of its own, since the selectors latch their environment
switches once per process) and the fixture's encoding.

  python -m tests.selector_cases --write      rewrite the fixture from the library as built

Sections (the fixture holds one list of results per section and call, in the order of the section's cases):
  dense        M x N x K grid, five calls, the tiling cache cleared before each
  masked       masked grouped layout (groups, m_max, n, k, expected_m), fast and bf16-exact
  contiguous   contiguous grouped layout (groups, m, n, k), fast and bf16-exact
  kgw          dga_tiling_k_grouped_wgrad (groups, m, n, k_total)
  tuned        every row of tuned/mi355x.csv as the preloaded table (a child without $DGA_NO_TUNED_TABLE)
  rows         one cache-file row at a time: the shapes and row generators of tests/test_cache_rows.py
A result is (rc, every field of dga_tiling_t, dga_workspace_bytes of it); the workspace is left out of `tuned` and `rows`."""
import ctypes
import json
import os
import subprocess
import sys
import tempfile
from pathlib import Path

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent
for _p in (str(ROOT), str(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

GOLDEN = HERE / "golden" / "selector_golden.json"
GOLDEN_CUS = 256

# About half of the values the grid was first drawn from on each axis (29 x 14 x 15): trimmed, for the fixture's size, to the smallest sub-grid on which the
# selectors still return every combination of (call, tile, kernelSerial, dispatchPolicyTag, build, stages, wave grid, split-K or not) that they
# return on the full one (129 of them); the odd and off-tile sizes stay.  tests/test_selector_golden.py asserts the classes by name.
DENSE_M = [1, 16, 17, 32, 33, 65, 128, 129, 256, 257, 513, 1279, 2048, 3511, 8192]
DENSE_N = [128, 512, 4096, 5003, 7168, 8192, 16384, 18432, 24576, 32768]
DENSE_K = [128, 256, 2048, 7168, 7681, 8191, 16384, 18432, 32768]
DENSE_CALLS = ["dga_select_kernel", "dga_tiling", "dga_tiling_bf16_exact", "dga_tiling_fp32_out", "dga_tiling_wgrad"]
GROUPED_CALLS = ["dga_tiling", "dga_tiling_bf16_exact"]
ROW_CALLS = ["dga_tiling", "dga_tiling_bf16_exact", "dga_tiling_fp32_out", "dga_tiling_wgrad"]

# (groups, m_max, n, k, expected_m); the four K < 256 cases reach the hint tiles of dga_tiling_bf16_exact (the grouped kernel takes every
# K >= 256 of an expert of more than 64 rows); the last is K % 16 != 0
MASKED = [(256, 128, 7168, 2048, 0), (256, 128, 7168, 2048, 16), (256, 128, 7168, 2048, 64), (64, 16, 3072, 8192, 0), (16, 64, 1536, 4096, 0),
          (8, 64, 4096, 7168, 32), (8, 64, 512, 2048, 16), (8, 128, 512, 128, 16), (8, 128, 512, 192, 48), (8, 128, 512, 192, 0),
          (8, 128, 512, 256, 16), (8, 64, 4096, 7161, 32)]
# (groups, m, n, k); the last is K % 16 != 0
CONTIGUOUS = [(32, 4096, 2048, 7168), (8, 8192, 4096, 7168), (4, 4096, 2048, 4096), (3, 384, 4096, 7168), (256, 32768, 7168, 2048),
              (4, 32768, 7168, 2048), (4, 4096, 2048, 4090)]
# (groups, m, n, k_total); the last five take the five tiles of the rule in turn (128 x 256 persistent, 128 x 128, 64 x 256, 64 x 128, 32 x 128)
KGW = [(8, 4096, 7168, 16384), (4, 128, 128, 2048), (32, 2048, 7168, 131072), (2, 64, 256, 512), (64, 7168, 2048, 65536),
       (1, 4096, 4096, 8192), (1, 2048, 2048, 8192), (100, 192, 128, 25600), (1, 1024, 2048, 8192), (1, 512, 2048, 8192)]
ROWS_RANDOM = 8     # hand-written rows per shape (tests/test_cache_rows.py runs 120 / 150 of the same generator)


def dense_cases():
    return [(m, n, k) for m in DENSE_M for n in DENSE_N for k in DENSE_K]


# ---- the dump: runs in the child ----------------------------------------------------------------------------------------------------

def _result(lib, fn, p, workspace=True, platform_arg=False):
    from deepgemm_ascend_amd.api import Tiling
    t = Tiling()
    args = (ctypes.byref(p), None, ctypes.byref(t)) if platform_arg else (ctypes.byref(p), ctypes.byref(t))
    rc = int(getattr(lib, fn)(*args))
    out = {"rc": rc, **t.as_dict()}
    if workspace:
        out["workspace"] = int(lib.dga_workspace_bytes(ctypes.byref(t)))
    return out


def _dump_section(lib, calls, problems, workspace=True):
    out = {}
    for fn in calls:
        res = []
        for p in problems:
            lib.dga_tiling_cache_clear()
            res.append(_result(lib, fn, p, workspace, platform_arg=fn == "dga_select_kernel"))
        out[fn] = res
    return out


def tuned_shapes():
    """(m, n, k, groups, contiguous) of every row of the shipped table."""
    import csv
    with open(ROOT / "deepgemm_ascend_amd" / "tuned" / "mi355x.csv") as f:
        return [(int(r["m"]), int(r["n"]), int(r["k"]), int(r.get("groups") or 1), int(r.get("contiguous") or 0)) for r in csv.DictReader(f)]


def row_cases():
    """(shape, kind, head, row) for the cache-file section: tests/test_cache_rows.py's shapes, generators and seeds."""
    import test_cache_rows as R
    out = []
    for name, m, n, k in R.DENSE:
        fast = R._fast_sweep_rows(m, n, k)
        bx = R._bx_sweep_rows(m, n, k)
        kinds = {"fast": fast, "fast_in_full_file": [(R.sweep.FULL_CSV_HEAD, r) for _, r in fast], "bx": bx,
                 "legacy": [r for r in (R._legacy(*x) for x in bx) if r], "tag23": [R._tag23(*x) for x in bx],
                 "reference": R._reference_rows(m, n, k), "random": R._random_rows(m, n, k, 1, False, ROWS_RANDOM, m * 7 + n + k)}
        out += [((name, m, n, k, 1, 0, False), kind, head, row) for kind, lst in kinds.items() for head, row in lst]
    for name, m, n, k, groups, expected_m, contiguous in R.GROUPED:
        kinds = {"fast": R._grouped_sweep_rows(m, n, k, groups, contiguous),
                 "random": R._random_rows(m, n, k, groups, contiguous, ROWS_RANDOM, groups * 31 + m + n)}
        out += [((name, m, n, k, groups, expected_m, contiguous), kind, head, row) for kind, lst in kinds.items() for head, row in lst]
    return out


def dump(phase):
    """phase "rules": the sections that need $DGA_NO_TUNED_TABLE (and the cache-file rows); "tuned": the preloaded table."""
    import deepgemm_ascend_amd as dga
    from deepgemm_ascend_amd import _lib
    lib = _lib.lib()
    pf = _lib.Platform()
    lib.dga_device_platform(ctypes.byref(pf))
    out = {"cus": int(pf.coreNum)}
    problem = dga.api._problem
    if phase == "tuned":
        res = {fn: [_result(lib, fn, problem(m, n, k, g, 0, contiguous=bool(c)), workspace=False) for m, n, k, g, c in tuned_shapes()]
               for fn in GROUPED_CALLS}
        out["tuned"] = res
        return out
    out["dense"] = _dump_section(lib, DENSE_CALLS, [problem(m, n, k) for m, n, k in dense_cases()])
    out["masked"] = _dump_section(lib, GROUPED_CALLS, [problem(m, n, k, g, em) for g, m, n, k, em in MASKED])
    out["contiguous"] = _dump_section(lib, GROUPED_CALLS, [problem(m, n, k, g, 0, contiguous=True) for g, m, n, k in CONTIGUOUS])
    out["kgw"] = _dump_section(lib, ["dga_tiling_k_grouped_wgrad"], [problem(m, n, k, g) for g, m, n, k in KGW])
    rows = {fn: [] for fn in ROW_CALLS}
    with tempfile.TemporaryDirectory() as tmp:
        path = Path(tmp) / "rows.csv"
        for (name, m, n, k, g, em, c), kind, head, row in row_cases():
            p = problem(m, n, k, g, em, contiguous=c)
            for fn in ROW_CALLS:     # (a miss appends to the open file: every call gets the file with the one row)
                path.write_text(head + row)
                assert lib.dga_tiling_cache_open(str(path).encode()) == 0 and lib.dga_tiling_cache_size() == 1, (head, row)
                rows[fn].append(_result(lib, fn, p, workspace=False))
        lib.dga_tiling_cache_open(None)
        lib.dga_tiling_cache_clear()
    out["rows"] = rows
    return out


# ---- the parent's side ---------------------------------------------------------------------------------------------------------------

def run_child(phase):
    """dump(phase) in a fresh process without any DGA_* switch of the caller's."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("DGA_") and k != "CACHE_FILE_PATH"}
    env["PYTHONPATH"] = str(ROOT)
    if phase == "rules":
        env["DGA_NO_TUNED_TABLE"] = "1"
    r = subprocess.run([sys.executable, "-m", "tests.selector_cases", "--dump", phase], capture_output=True, text=True, env=env,
                       cwd=str(ROOT), timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def section_cases():
    """section -> the case of every result, as the failure messages name it."""
    return {"dense": dense_cases(), "masked": MASKED, "contiguous": CONTIGUOUS, "kgw": KGW, "tuned": tuned_shapes(),
            "rows": [(shape, kind, row.strip()) for shape, kind, head, row in row_cases()]}


def section_problems():
    """section -> (m, n, k, groups) of every case: what a result's echo fields are stored against."""
    return {"dense": [(m, n, k, 1) for m, n, k in dense_cases()], "masked": [(m, n, k, g) for g, m, n, k, em in MASKED],
            "contiguous": [(m, n, k, g) for g, m, n, k in CONTIGUOUS], "kgw": [(m, n, k, g) for g, m, n, k in KGW],
            "tuned": [(m, n, k, g) for m, n, k, g, c in tuned_shapes()],
            "rows": [(shape[1], shape[2], shape[3], shape[4]) for shape, kind, head, row in row_cases()]}


# The fixture: one table of distinct results and, per section and call, one index into it for every case ("results") and the non-zero
# workspaces by case number.  A call whose answers mostly repeat an earlier call's of the section names it ("as") and lists only the cases
# that differ.  So that the table stays small, the fields that echo the problem are stored as their difference from it (swizzleDirection
# from m > n ? 0 : 1), and blockDim as its difference from the plain raster (groups x tile rows x tile columns x split-K) of the result's
# own tile; decode() adds them back, nothing is lost.  A field that then has one value in the whole table is stored once ("constant").
ECHO = {"m": 0, "n": 1, "k": 2, "groups": 3, "strideA": 2, "strideB": 2, "strideC": 1}


def _raster(r):
    if not r["m1"] or not r["n1"]:
        return 0
    groups = 1 if r["contiguous"] else max(1, r["groups"])
    return groups * -(-r["m"] // r["m1"]) * -(-r["n"] // r["n1"]) * max(1, r["splitkFactor"])


def _relative(r, prob, sign):
    r = dict(r)
    if sign < 0:
        r["blockDim"] -= _raster(r)
    for f, i in ECHO.items():
        r[f] += sign * prob[i]
    r["swizzleDirection"] += sign * (0 if prob[0] > prob[1] else 1)
    if sign > 0:
        r["blockDim"] += _raster(r)
    return r


def encode(results):
    fields = None
    table, index = {}, {}
    problems = section_problems()
    for section in ("dense", "masked", "contiguous", "kgw", "tuned", "rows"):
        index[section] = {}
        prev = None
        for fn, res in results[section].items():
            ids, work = [], []
            assert len(res) == len(problems[section]), (section, fn)
            for r, prob in zip(res, problems[section]):
                r = _relative(r, prob, -1)
                work.append(r.pop("workspace", 0))
                if fields is None:
                    fields = list(r)
                assert list(r) == fields
                ids.append(table.setdefault(tuple(r.values()), len(table)))
            enc = {"results": ids, "workspace": {str(i): w for i, w in enumerate(work) if w}}
            if prev and 2 * sum(a != b for a, b in zip(ids, prev[1])) < len(ids):
                enc = {"as": prev[0], "results": {str(i): a for i, (a, b) in enumerate(zip(ids, prev[1])) if a != b},
                       "workspace": {str(i): a for i, (a, b) in enumerate(zip(work, prev[2])) if a != b}}
            index[section][fn] = enc
            prev = (fn, ids, work)
    const = {f: v for f, v, col in zip(fields, next(iter(table)), zip(*table)) if len(set(col)) == 1}
    return {"cus": results["cus"], "constant": const, "fields": [f for f in fields if f not in const],
            "table": [[v for f, v in zip(fields, t) if f not in const] for t in table], "index": index}


def decode(fixture):
    """section -> call -> list of results (dicts, `workspace` included where the section records it)."""
    problems = section_problems()
    out = {}
    for section, calls in fixture["index"].items():
        out[section], flat = {}, {}
        for fn, enc in calls.items():
            if "as" in enc:
                ids = [enc["results"].get(str(i), tid) for i, tid in enumerate(flat[enc["as"]][0])]
                work = [enc["workspace"].get(str(i), w) for i, w in enumerate(flat[enc["as"]][1])]
            else:
                ids = enc["results"]
                work = [enc["workspace"].get(str(i), 0) for i in range(len(ids))]
            flat[fn] = (ids, work)
            assert len(ids) == len(problems[section]), (section, fn, "the case list and the fixture differ in length")
            res = []
            for tid, w, prob in zip(ids, work, problems[section]):
                r = _relative(dict(fixture["constant"], **dict(zip(fixture["fields"], fixture["table"][tid]))), prob, +1)
                if section not in ("tuned", "rows"):
                    r["workspace"] = w
                res.append(r)
            out[section][fn] = res
    return out


def collect():
    """Both children's results, merged (the two run side by side)."""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(2) as pool:
        results, tuned = pool.map(run_child, ("rules", "tuned"))
    assert tuned["cus"] == results["cus"]
    results["tuned"] = tuned["tuned"]
    return results


def write_fixture(fixture, path=GOLDEN):
    lines = ['{"cus": %d,' % fixture["cus"], ' "constant": %s,' % json.dumps(fixture["constant"]), ' "fields": %s,' % json.dumps(fixture["fields"]),
             ' "table": [']
    rows = [json.dumps(t, separators=(",", ":")) for t in fixture["table"]]
    lines += ["  " + ", ".join(rows[i:i + 4]) + ("," if i + 4 < len(rows) else "") for i in range(0, len(rows), 4)]
    lines += [" ],", ' "index": {']
    sections = list(fixture["index"].items())
    for si, (section, calls) in enumerate(sections):
        lines.append('  "%s": {' % section)
        for ci, (fn, enc) in enumerate(calls.items()):
            head = '"as": "%s", ' % enc["as"] if "as" in enc else ""
            lines.append('   "%s": {%s"results": %s,' % (fn, head, json.dumps(enc["results"], separators=(",", ":"))))
            lines.append('    "workspace": %s}%s' % (json.dumps(enc["workspace"], separators=(",", ":")), "," if ci + 1 < len(calls) else ""))
        lines.append("  }%s" % ("," if si + 1 < len(sections) else ""))
    lines += [" }", "}"]
    path.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--dump":
        print(json.dumps(dump(sys.argv[2])))
    elif sys.argv[1:] == ["--write"]:
        got = collect()
        assert got["cus"] == GOLDEN_CUS, "the fixture is a %d-CU fixture; this device reports %d" % (GOLDEN_CUS, got["cus"])
        write_fixture(encode(got))
        print("wrote %s (%d bytes)" % (GOLDEN, GOLDEN.stat().st_size))
    else:
        sys.exit(__doc__)
