"""CPU: every fp8 tiling selector returns, field for field, what tests/golden/selector_golden.json records (tests/selector_cases.py: the
cases, the dump in a child process, `python -m tests.selector_cases --write`).  The fixture is a 256-CU fixture: on a device that reports
another CU count the selectors legitimately answer differently, and the tests skip."""
import json

import pytest

import selector_cases as S


@pytest.fixture(scope="module")
def golden():
    return S.decode(json.loads(S.GOLDEN.read_text()))


@pytest.fixture(scope="module")
def got():
    res = S.collect()
    if res["cus"] != S.GOLDEN_CUS:
        pytest.skip("dga_device_platform reports %d CUs; the fixture records the selectors' answers for %d" % (res["cus"], S.GOLDEN_CUS))
    return res


@pytest.mark.parametrize("section", ["dense", "masked", "contiguous", "kgw", "tuned", "rows"])
def test_the_selectors_return_the_recorded_tilings(golden, got, section):
    cases = S.section_cases()[section]
    assert set(got[section]) == set(golden[section])
    bad, count = [], 0
    for fn, want_list in golden[section].items():
        got_list = got[section][fn]
        assert len(got_list) == len(want_list) == len(cases), (section, fn)
        for case, want, have in zip(cases, want_list, got_list):
            if want != have:
                count += 1
                if len(bad) < 10:
                    bad.append((fn, case, {f: (want[f], have.get(f)) for f in want if want[f] != have.get(f)}))
    assert not bad, "%d results differ; (call, case, {field: (recorded, returned)}): %s" % (count, bad)


def _rows(results, fn):
    return [r for r in results[fn] if r["rc"] == 0]


def test_the_dense_grid_reaches_every_rule(golden):
    """A trimmed grid must not quietly lose a rule: each class the selectors have on dense problems has a row in the fixture."""
    bx = _rows(golden["dense"], "dga_tiling_bf16_exact")
    assert {r["kernelSerial"] for r in bx} >= {0, 4, 5, 6, 7}
    assert {r["build"] for r in bx} >= {0, 10}
    assert {(r["m1"], r["n1"]) for r in bx} >= {(128, 256), (128, 128), (64, 256), (64, 128), (32, 128)}
    assert {(r["m1"], r["n1"]) for r in bx if r["kernelSerial"] == 6 and r["build"] == 0} >= {(16, 128), (32, 128)}
    fast = _rows(golden["dense"], "dga_tiling") + _rows(golden["dense"], "dga_select_kernel")
    assert {r["kernelSerial"] for r in fast} >= {0, 1, 4, 5, 6, 7}
    assert {r["dispatchPolicyTag"] for r in fast} >= {0, 2, 4, 5, 6}
    assert {r["stages"] for r in fast} >= {2, 3}
    assert golden["dense"]["dga_tiling"] != golden["dense"]["dga_select_kernel"]          # the predictor changes picks


def test_the_grouped_cases_reach_their_rules(golden):
    bx = dict(zip(S.MASKED, golden["masked"]["dga_tiling_bf16_exact"]))
    hint = [(bx[c]["m1"], bx[c]["n1"], bx[c]["build"]) for c in ((8, 128, 512, 128, 16), (8, 128, 512, 192, 48), (8, 128, 512, 192, 0), (8, 128, 512, 256, 16))]
    assert hint == [(32, 128, 0), (64, 256, 0), (128, 128, 0), (128, 256, 9)]
    kgw = golden["kgw"]["dga_tiling_k_grouped_wgrad"]
    assert {(r["m1"], r["n1"]) for r in kgw} == {(128, 256), (128, 128), (64, 256), (64, 128), (32, 128)}
    assert {r["build"] for r in kgw} == {7, 8}
