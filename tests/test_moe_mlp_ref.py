"""CPU: the float64 reference of the expert-MLP training step (tests/moe_mlp_ref.py) that tests/test_moe_mlp_step_gpu.py holds the device
to.  step_exact against torch.autograd in float64; step_emulated without its roundings is step_exact; with them it stays a small
perturbation of it; and the caps the GPU test puts on the share of codes excused near a rounding boundary hold when the float64
reference itself is moved by the whole element bound."""
import numpy as np
import pytest
import torch

import moe_mlp_ref as R
from fused_bounds import EPS, _reference

KEYS = ("Y1", "h", "Out", "grad_h", "dY1", "dX", "dW1", "dW2")


def _autograd(case):
    out = {k: [] for k in KEYS}
    for x, w1, w2, do in zip(case["X"], case["W1"], case["W2"], case["dOut"]):
        x, w1, w2 = (torch.from_numpy(v).clone().requires_grad_(True) for v in (x, w1, w2))
        y1 = x @ w1.t()
        h = torch.nn.functional.silu(y1[:, :R.H]) * y1[:, R.H:]
        o = h @ w2.t()
        y1.retain_grad(); h.retain_grad()
        (o * torch.from_numpy(do)).sum().backward()
        zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad          # (an empty expert)
        for k, v in (("Y1", y1), ("h", h), ("Out", o), ("grad_h", zero(h)), ("dY1", zero(y1)), ("dX", zero(x)), ("dW1", zero(w1)),
                     ("dW2", zero(w2))):
            out[k].append(v.detach().numpy())
    return out


@pytest.mark.parametrize("seed", [0, 1])
def test_step_exact_is_autograd_in_float64(seed):
    """Both are float64 and differ only in summation order: relative Frobenius difference <= 1e-12, per tensor and per expert (the
    one-token expert is not averaged away under the 200-token one)."""
    case = R.make_case(seed)
    got, want = R.step_exact(case), _autograd(case)
    for k in KEYS:
        for g, t in enumerate(case["tokens"]):
            if t == 0:
                assert not np.asarray(got[k][g]).any() and not want[k][g].any(), (k, g)
                continue
            err = R.rel_error([got[k][g]], [want[k][g]])
            assert err <= 1e-12, (k, g, err)
    assert got["dW1"].shape == (R.G, 2 * R.H, R.D) and got["dW2"].shape == (R.G, R.D, R.H)


def test_emulated_without_roundings_is_step_exact():
    """The emulation has the step's structure and nothing else.  The dgrads multiply with a contiguous copy of W^T where step_exact takes W,
    so the two differ by summation order alone: the autograd test's 1e-12, per tensor and per expert."""
    case = R.make_case(0)
    got, want = R.step_emulated(case, None), R.step_exact(case)
    for k in KEYS:
        for g, t in enumerate(case["tokens"]):
            if t == 0:
                assert not np.asarray(got[k][g]).any() and np.asarray(got[k][g]).shape == np.asarray(want[k][g]).shape, (k, g)
                continue
            err = R.rel_error([got[k][g]], [want[k][g]])
            assert err <= 1e-12, (k, g, err)


def test_emulated_is_a_small_perturbation_of_exact(oracle):
    """An e4m3 rounding moves an element by at most 2^-4 relative, about 0.026 rms; an output has at most seven of them behind it (dX: X, W1,
    dOut, W2^T, the gate's path through Y1, dY1, W1^T), 0.026 sqrt(7) = 0.07.  A transposed operand, a swapped half or a wrong scale axis in
    the emulation gives an error of order 1."""
    case = R.make_case(0)
    emu, exact = R.step_emulated(case, oracle), R.step_exact(case)
    for k in KEYS:
        err = R.rel_error(emu[k], exact[k])
        print(f"{k}: emulated against exact {err:.4f}")
        assert 1e-3 < err < 0.1, (k, err)
    assert not emu["dW1"][1].any() and not emu["dW2"][1].any() and emu["dW1"][3].any() and emu["dW2"][3].any()


def test_seed_0_is_not_the_largest_emulated_error(oracle):
    """The condition the whole-step error test on the GPU rests on (moe_mlp_ref.ERROR_SEEDS): for every output the largest emulated error
    of the eight seeds exceeds seed 0's by more than 2^-10 of it."""
    errs = np.array([R.emulated_errors(oracle, seed) for seed in R.ERROR_SEEDS])
    for j, k in enumerate(R.ERROR_KEYS):
        margin = errs[:, j].max() / errs[0, j] - 1.0
        print(f"{k}: seed 0 {errs[0, j]:.7f}, largest {errs[:, j].max():.7f} (seed {R.ERROR_SEEDS[int(errs[:, j].argmax())]}), margin {margin:.2e}")
        assert margin > 2.0 ** -10, (k, margin)


def _shares(oracle, ref, bound):
    """Row-wise 1x128 quantisation of fl32(ref): the share of elements with two admissible codes when ref moves by +-bound, and the expected
    share of elements within their bound of a boundary."""
    _, sf = oracle.quant_1x128(ref.astype(np.float32))
    scale = np.repeat(sf.astype(np.float64), 128, axis=1)[:, :ref.shape[1]]
    lo, hi = R.code_interval(oracle, ref, bound, scale)
    return float((lo != hi).mean()), R.expected_boundary_share(ref, bound, scale), R.dgate_cap(ref, bound, scale)


@pytest.mark.parametrize("seed", [0, 1])
def test_the_caps_hold_for_the_reference_moved_by_the_whole_bound(oracle, seed):
    """What the GPU test relies on, for its seed (0) and another: the share of elements of the emulated step's h, dup and dgate for which
    RNE((ref - bound) / s) and RNE((ref + bound) / s) differ -- every element a device that uses its whole bound could be excused for --
    is inside the cap, along the rows and (h) along the tokens."""
    case = R.make_case(seed)
    emu = R.step_emulated(case, oracle)
    y1 = np.concatenate(emu["Y1"]); grad_h = np.concatenate(emu["grad_h"])
    h = R.act(y1)
    for name, ref in (("h", h), ("h^T", np.ascontiguousarray(np.concatenate([R._pad128(R.act(v)) for v in emu["Y1"]]).T))):
        two, expect, _ = _shares(oracle, ref, EPS * np.abs(ref))
        print(f"seed {seed} {name}: {two:.3e} of the elements have two admissible codes (expected {expect:.3e}, cap {R.CAP_RELATIVE:.3e})")
        assert two <= R.CAP_RELATIVE and expect <= 2.0 ** -13
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v))
    ref, bound = _reference(t(y1[:, :R.H]), t(y1[:, R.H:]), t(grad_h))
    assert np.array_equal(ref, R.act_bwd(y1, grad_h))                  # the shared bound helper and this module state one dY1
    two, expect, _ = _shares(oracle, ref[:, R.H:], bound[:, R.H:])
    print(f"seed {seed} dup: {two:.3e} (expected {expect:.3e}, cap {R.CAP_RELATIVE:.3e})")
    assert two <= R.CAP_RELATIVE and expect <= 2.0 ** -13
    two, expect, cap = _shares(oracle, ref[:, :R.H], bound[:, :R.H])
    print(f"seed {seed} dgate: {two:.3e} (expected {expect:.3e}, cap {cap:.3e} = 8 x expected)")
    assert two <= cap
    assert 2.0 ** -14 <= expect <= 2.0 ** -9                           # the derivation's estimate: 2^-12 for g >= 0 plus about 1.5 * 2^-10
