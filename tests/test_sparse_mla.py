"""CPU: sparse_mla_fwd's reference against the definition written as a loop, the entry declared, exported and in the ctypes table, and
every refusal the wrapper makes before a launch (there is no CPU path, so a call with nothing to refuse is refused for its device)."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import sparse_mla_ref as R
from sparse_mla_support import _args

ROOT = Path(__file__).resolve().parent.parent


def test_reference_matches_the_definition_as_a_loop():
    rng = np.random.default_rng(3)
    m, h, s, topk = 3, 2, 9, 7
    q = R.bf16_round(rng.standard_normal((m, h, R.D_QK)).astype(np.float32))
    kv = R.bf16_round(rng.standard_normal((s, R.D_QK + 8)).astype(np.float32))
    kv[:, R.D_QK:] = np.nan                                            # columns a row does not have
    kv[5] = np.nan                                                     # a row nobody selects
    idx = np.array([[0, 3, -1, 3, 8, 9, -7], [-1] * 7, [2, 1, 0, 4, 6, 3, 8]], np.int32)
    # (offsets: a -1 that an offset would bring into range stays invalid; 8 + 1 and 0 - 2 leave the range; row 5 is never named)
    for off in (None, np.zeros(3, np.int32), np.array([1, 3, -2], np.int32)):
        i = idx
        ref = R.reference(q, kv, i, 0.05, off)
        out, lse = R.direct(q, kv, i, 0.05, off)
        assert np.isfinite(ref["out"]).all() and np.allclose(ref["out"], out, rtol=1e-12, atol=1e-13)
        assert np.array_equal(np.isneginf(ref["lse"]), np.isneginf(lse))
        fin = np.isfinite(lse)
        assert np.allclose(ref["lse"][fin], lse[fin], rtol=1e-12, atol=1e-13)
        assert (ref["A"] >= np.abs(ref["out"]) - 1e-12).all()
    ref = R.reference(q, kv, idx, 0.05)
    assert ref["count"].tolist() == [4, 0, 7] and np.isneginf(ref["lse"][1]).all() and not ref["out"][1].any()
    # duplicates count once per position: the list [3, 3] weighs row 3 twice against row 0
    two = R.reference(q[:1], kv, np.array([[0, 3, 3]], np.int32), 0.05)
    one = R.reference(q[:1], kv, np.array([[0, 3]], np.int32), 0.05)
    assert not np.allclose(two["out"], one["out"])


def test_bf16_rounding_is_to_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -7 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -3.0, 0.0], np.float32)
    assert R.bf16_round(x).tolist() == [1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -3.0, 0.0]
    t = torch.from_numpy(np.random.default_rng(0).standard_normal(4096).astype(np.float32))
    assert np.array_equal(R.bf16_bits(t.numpy()), t.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))


def test_symbol_is_declared_exported_and_in_the_table(dga):
    from deepgemm_ascend_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "dga_hip.h").read_text(), flags=re.S)
    assert re.search(r"\bint\s+dga_sparse_mla_fwd\s*\(", text)
    assert re.search(r"#define\s+DGA_SPARSE_MLA_D_QK\s+576\b", text) and re.search(r"#define\s+DGA_SPARSE_MLA_D_V\s+512\b", text)
    assert hasattr(ctypes.CDLL(str(_lib.LIB_PATH)), "dga_sparse_mla_fwd")
    restype, argtypes = _lib.SIGNATURES["dga_sparse_mla_fwd"]
    assert restype is ctypes.c_int and len(argtypes) == 15
    assert dga.SPARSE_MLA_D_QK == 576 and dga.SPARSE_MLA_D_V == 512 and callable(dga.sparse_mla_fwd)
    assert _lib.lib().dga_abi_version() == 7


def test_c_entry_checks_before_any_launch(dga):
    """the C entry's own refusals and M == 0, none of which touches a device"""
    from deepgemm_ascend_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(4096 + 64)
    p = (ctypes.addressof(buf) + 63) & ~63

    def call(q=p, kv=p, idx=p, off=None, m=1, heads=16, s=4, kv_stride=576, topk=2, idx_stride=2, flags=0, out=p, lse=p):
        return L.dga_sparse_mla_fwd(q, kv, idx, off, m, heads, s, kv_stride, topk, idx_stride, 0.1, flags, out, lse, None)

    codes = {call(m=-1), call(heads=8), call(heads=144), call(heads=24), call(s=0), call(topk=0), call(kv_stride=575), call(idx_stride=1)}
    assert len(codes) == 1 and 0 not in codes                                      # one status: the shape
    assert call(m=0) == 0 and call(m=0, q=None, out=None) == 0
    assert call(q=None) == call(lse=None) == call(idx=None) != 0 and call(q=None) not in codes
    a = call(kv=p + 8)
    assert a != 0 and a == call(q=p + 2) == call(out=p + 4) == call(lse=p + 2) == call(off=p + 1) == call(kv_stride=580)
    r = call(flags=2)
    assert r != 0 and r == call(s=1 << 31) and r not in codes and r != a


def test_every_refusal_comes_from_the_wrapper(dga):
    q, kv, idx = _args()
    bad = {
        "q dtype": lambda: dga.sparse_mla_fwd(q.float(), kv, idx, 0.1),
        "q rank": lambda: dga.sparse_mla_fwd(q[0], kv, idx, 0.1),
        "q d": lambda: dga.sparse_mla_fwd(torch.zeros((2, 16, 512), dtype=torch.bfloat16), kv, idx, 0.1),
        "q not contiguous": lambda: dga.sparse_mla_fwd(torch.zeros((2, 32, 576), dtype=torch.bfloat16)[:, ::2], kv, idx, 0.1),
        "Hq = 8": lambda: dga.sparse_mla_fwd(_args(h=8)[0], kv, idx, 0.1),
        "Hq = 24": lambda: dga.sparse_mla_fwd(_args(h=24)[0], kv, idx, 0.1),
        "Hq = 144": lambda: dga.sparse_mla_fwd(_args(h=144)[0], kv, idx, 0.1),
        "d_v": lambda: dga.sparse_mla_fwd(q, kv, idx, 0.1, 576),
        "kv dtype": lambda: dga.sparse_mla_fwd(q, kv.half(), idx, 0.1),
        "kv rank": lambda: dga.sparse_mla_fwd(q, kv.view(2, 4, 576), idx, 0.1),
        "kv d": lambda: dga.sparse_mla_fwd(q, torch.zeros((8, 512), dtype=torch.bfloat16), idx, 0.1),
        "kv empty": lambda: dga.sparse_mla_fwd(q, kv[:0], idx, 0.1),
        "kv last dimension strided": lambda: dga.sparse_mla_fwd(q, torch.zeros((8, 1152), dtype=torch.bfloat16)[:, ::2], idx, 0.1),
        "kv stride 580": lambda: dga.sparse_mla_fwd(q, torch.zeros((8, 580), dtype=torch.bfloat16)[:, :576], idx, 0.1),
        "kv misaligned": lambda: dga.sparse_mla_fwd(q, torch.zeros((8 * 584 + 4,), dtype=torch.bfloat16)[4:].view(8, 584)[:, :576], idx, 0.1),
        "indices dtype": lambda: dga.sparse_mla_fwd(q, kv, idx.long(), 0.1),
        "indices rank": lambda: dga.sparse_mla_fwd(q, kv, idx[0], 0.1),
        "indices rows": lambda: dga.sparse_mla_fwd(q, kv, idx[:1], 0.1),
        "indices empty": lambda: dga.sparse_mla_fwd(q, kv, idx[:, :0], 0.1),
        "indices last dimension strided": lambda: dga.sparse_mla_fwd(q, kv, torch.zeros((2, 8), dtype=torch.int32)[:, ::2], 0.1),
        "offsets dtype": lambda: dga.sparse_mla_fwd(q, kv, idx, 0.1, index_offsets=torch.zeros(2, dtype=torch.int64)),
        "offsets shape": lambda: dga.sparse_mla_fwd(q, kv, idx, 0.1, index_offsets=torch.zeros(3, dtype=torch.int32)),
        "out shape": lambda: dga.sparse_mla_fwd(q, kv, idx, 0.1, out=torch.zeros((2, 16, 576), dtype=torch.bfloat16)),
        "out dtype": lambda: dga.sparse_mla_fwd(q, kv, idx, 0.1, out=torch.zeros((2, 16, 512), dtype=torch.float32)),
        "lse shape": lambda: dga.sparse_mla_fwd(q, kv, idx, 0.1, lse=torch.zeros((2, 16, 1), dtype=torch.float32)),
        "lse dtype": lambda: dga.sparse_mla_fwd(q, kv, idx, 0.1, lse=torch.zeros((2, 16), dtype=torch.bfloat16)),
    }
    for what, call in bad.items():
        with pytest.raises(dga.DGAError) as e:
            call()
        assert "HIP device" not in str(e.value), what                  # refused for what it is, not for where it lives
    # nothing to refuse but the device: CPU tensors, in each accepted layout
    for call in (lambda: dga.sparse_mla_fwd(q, kv, idx, 0.1),
                 lambda: dga.sparse_mla_fwd(q, kv.view(8, 1, 576), idx.view(2, 1, 4), 0.1, 512, torch.zeros(2, dtype=torch.int32)),
                 lambda: dga.sparse_mla_fwd(q, torch.zeros((8, 640), dtype=torch.bfloat16)[:, :576], torch.zeros((2, 9), dtype=torch.int32)[:, :4],
                                            0.1)):
        with pytest.raises(dga.DGAError) as e:
            call()
        assert "HIP device" in str(e.value)


@pytest.mark.parametrize("h", R.ALL_HEADS)
def test_winners_case_tells_every_head_apart(h):
    """what the GPU test of the same case relies on"""
    q, kv, idx, scale, win = R.winners_case(h)
    assert q.shape == (R.WIN_M, h, R.D_QK) and idx.shape == (R.WIN_M, R.WIN_TOPK) and win.shape == (R.WIN_M, h) and scale == 2.0 ** -3
    assert np.array_equal(R.bf16_round(q), q) and np.array_equal(R.bf16_round(kv), kv)          # bf16 holds the operands
    rows, valid = R.rows_of(idx, R.WIN_S)
    assert (valid.sum(axis=1) == R.WIN_TOPK - R.WIN_INVALID).all() and (idx[~valid] == -1).all() and not valid[:, -3:].any()
    for t, sc in enumerate(R.scores(q, kv, idx, scale)):
        top = np.sort(sc, axis=1)
        assert (top[:, -1] == 512).all() and (top[:, -1] - top[:, -2] >= 256).all()              # the top score, the margin
        assert set(np.unique(sc)) <= {-512.0, 0.0, 512.0}
        assert np.array_equal(rows[t][valid[t]][sc.argmax(axis=1)], win[t])                       # the winner is the row it says
        assert len(set(win[t])) == h                                                              # distinct within the token
        where = np.flatnonzero(np.isin(rows[t], win[t]) & valid[t])
        assert len(where) == h and len(set(where // R.TILE)) == R.WIN_TOPK // R.TILE >= 3          # once each, in every tile
    assert len({tuple(w) for w in win}) == R.WIN_M                                               # a fresh map per token
    assert len(np.unique(R.winner_bits(kv, win).reshape(-1, R.D_V), axis=0)) == len(np.unique(win))   # distinct rows, distinct bits
    # the float64 reference is the winner's row, and its lse is 512
    ref = R.reference(q, kv, idx, scale)
    assert np.array_equal(ref["out"].astype(np.float32), kv[win][:, :, :R.D_V]) and np.array_equal(ref["lse"], np.full((R.WIN_M, h), 512.0))
    assert R.heads_off_their_winner(R.winner_bits(kv, win), kv, win) == []


def test_the_winner_check_rejects_two_swapped_heads():
    for h in (16, 80):
        q, kv, idx, scale, win = R.winners_case(h)
        bits = R.winner_bits(kv, win)
        bad = bits.copy()
        bad[1, [3, h - 2]] = bits[1, [h - 2, 3]]                        # two heads of one token swapped: a head in the wrong lane or wave
        assert R.heads_off_their_winner(bad, kv, win) == [(1, 3), (1, h - 2)]
        bad = bits.copy()
        bad[2, 5, 511] ^= 0x8000                                        # one sign bit (the -0 the float64 out would round to)
        assert R.heads_off_their_winner(bad, kv, win) == [(2, 5)]


def test_the_peaked_cases_keep_every_weight_in_fp32s_normal_range():
    for h in R.PEAK_HEADS:
        q, kv, idx = R.random_case(h)
        flat = R.score_spread(q, kv, idx, R.SCALE4)
        for sign in (1, -1):
            spread = R.score_spread(q, kv, idx, sign * R.PEAK * R.SCALE4)
            assert np.isclose(spread, R.PEAK * flat) and 20 < spread < R.SPREAD_MAX, (h, sign, spread)
        for order in ("ascending", "descending"):                      # the order changes the list, not the set
            assert R.score_spread(q, kv, R.ordered(q, kv, idx, order), R.PEAK * R.SCALE4) == R.score_spread(q, kv, idx, R.PEAK * R.SCALE4)
    # every head count's list has the counts the GPU test asserts
    for h in R.ALL_HEADS:
        _, _, idx = R.random_case(h)
        assert R.rows_of(idx, R.S4)[1].sum(axis=1).tolist() == [318, 298, 318, 318, 318]
    q, kv, idx = R.long_case(16)
    rows, valid = R.rows_of(idx, kv.shape[0])
    assert idx.shape == (2, 2048) and valid.all() and all(len(set(r)) == 2048 for r in rows) and R.score_spread(q, kv, idx, R.SCALE4) < R.SPREAD_MAX


def test_the_int32_extremes_name_the_rows_they_should():
    s = 40
    idx, off, want = R.extremes_case(s)
    assert idx.dtype == np.int32 and off.dtype == np.int32 and off.tolist() == [-(2 ** 31 - 1) + 5, 2 ** 31 - 1, -2 ** 31, 0, 7]
    rows, valid = R.rows_of(idx, s, off)
    assert [rows[t][valid[t]].tolist() for t in range(5)] == want
    # every extreme the case is about is in it; the sums of tokens 1 and 2 leave the int32 range
    assert idx[0, 0] == R.INT_MAX and rows[0, 0] == 5 and (idx == R.INT_MIN).any(axis=1).all()
    assert idx[1, 0] == R.INT_MAX and rows[1, 0] == 2 ** 32 - 2 and idx[2, 2] == 5 and rows[2, 39] == -2 ** 32 and not valid[1:3].any()
    assert [len(w) for w in want] == [4, 0, 0, 8, 2]                    # powers of two where there is a count
