"""Not a test file: the float64 references and element bounds of the fused SiLU-and-multiply quantisers' tolerance family (DESIGN.md "Fused
SiLU-and-multiply quantiser" and "... backward quantiser"), shared by tests/test_silu_mul_cast_gpu.py, tests/test_silu_mul_bwd_cast_gpu.py
and tests/test_moe_mlp_step_gpu.py.  Imports no GPU code; the tensor arguments are torch tensors on any device."""
import numpy as np

EPS = 2.0 ** -18                    # forward: |h32 - h| <= EPS |h|
EPS_GATE = 2.0 ** -17               # |dgate32 - dgate| <= EPS_GATE |d u| (s + |g| s (1 - s))
EPS_UP = 2.0 ** -18                 # |dup32 - dup| <= EPS_UP |dup|


def _h_ref(gate, up):
    """fl32 of the float64 value of g / (1 + exp(-g)) * u, rows flattened."""
    g = gate.double().cpu().numpy().reshape(-1, gate.shape[-1])
    u = up.double().cpu().numpy().reshape(-1, up.shape[-1])
    return (g / (1.0 + np.exp(-g)) * u).astype(np.float32)


def _e4m3_rne_satfinite(oracle, y):
    """float64 -> the e4m3fn value nearest to it (ties to the even code, |y| > 448 to +-448), from the oracle's code table."""
    vals = oracle.e4m3fn_table()[:0x7F].astype(np.float64)          # codes 0x00..0x7E: 0 .. 448, increasing with the code
    assert (np.diff(vals) > 0).all() and vals[0] == 0.0 and vals[-1] == 448.0
    a = np.minimum(np.abs(y), 448.0)
    hi = np.clip(np.searchsorted(vals, a, side="left"), 1, len(vals) - 1)
    lo = hi - 1
    dlo, dhi = a - vals[lo], vals[hi] - a
    code = np.where(dlo < dhi, lo, np.where(dhi < dlo, hi, np.where(lo % 2 == 0, lo, hi)))
    return np.copysign(vals[code], y)


def _reference(gate, up, grad):
    """In float64 from the (rounded) inputs [rows, H]: the reference [dgate | dup] and its element bounds, EPS_GATE |d u| (s + |g| s (1 - s))
    and EPS_UP |dup|.  1 - s is taken as exp(-g) s: no cancellation at large g."""
    G, U, D = (t.double().cpu().numpy() for t in (gate, up, grad))
    e = np.exp(-G)
    s = 1.0 / (1.0 + e)
    one_minus_s = e * s
    dup = D * G * s
    dgate = D * U * (s + G * s * one_minus_s)
    mag = np.abs(D * U) * (s + np.abs(G) * s * one_minus_s)
    ref = np.concatenate([dgate, dup], axis=1)
    bound = np.concatenate([EPS_GATE * mag, EPS_UP * np.abs(dup)], axis=1)
    ref.setflags(write=False); bound.setflags(write=False)
    return ref, bound
