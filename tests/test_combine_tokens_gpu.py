"""GPU: combine_tokens bit for bit against the numpy float32 reference of tests/combine_ref.py (its definition), and
combine_tokens_weight_grad against float64 under the derived any-order bar.

T = 37 tokens, k in {1, 2, 8}, S = 300 source rows, H in {384, 100, 7176}: the vector path, the bounded path, and a row long enough to be split
over workgroups.  Some choices are -1, S, S + 5, 2^62 or -2^63, token 5 has no valid choice and gets a row of +0; the source rows no valid
choice names hold NaN, and so do the weights of the dropped choices.  out is pre-filled with NaN: every element is written."""
import numpy as np
import pytest
import torch

import combine_ref as C

pytestmark = pytest.mark.gpu

_DEV = {}


def _device_case(k, h, dtype):
    """(case, src, grad, dest, weights on the device), once per process."""
    key = (k, h, dtype)
    if key not in _DEV:
        c = C.make_case(k, h, dtype)
        to = lambda a: torch.from_numpy(a).to(C.TORCH_DT[dtype]).cuda()
        _DEV[key] = (c, to(c["src"]), to(c["grad"]), torch.from_numpy(c["dest"]).cuda(), torch.from_numpy(c["w"]).cuda())
    return _DEV[key]


def _out_bits(t):
    return (t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)).cpu().numpy().view(np.uint32 if t.dtype == torch.float32 else np.uint16)


@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("h", C.HS)
@pytest.mark.parametrize("k", C.KS)
def test_combine_is_the_float32_definition_bit_for_bit(dga, k, h, dtype):
    c, src, _, dest, w = _device_case(k, h, dtype)
    assert np.isnan(c["src"]).any() and (~C.valid(c["dest"], C.S)).any()
    for weights, w_np in ((None, None), (w, c["w"])):
        want = C.combine_ref(c["src"], c["dest"], w_np)
        assert np.isfinite(want).all() and not want[C.EMPTY_TOKEN].any()
        for odt in (dtype, "fp32"):
            what = f"weights={weights is not None} out={odt}"
            out = torch.full((C.T, h), float("nan"), dtype=C.TORCH_DT[odt], device="cuda")
            got = dga.combine_tokens(src, dest, weights, out=out)
            torch.cuda.synchronize()
            assert got is out
            assert np.array_equal(_out_bits(out), C.round_to(want, odt)), what
            assert not _out_bits(out)[C.EMPTY_TOKEN].any(), what               # +0, not -0
        got = dga.combine_tokens(src, dest, weights, sync=True)                # without out=: src's dtype
        assert got.dtype == C.TORCH_DT[dtype] and np.array_equal(_out_bits(got), C.round_to(want, dtype))


@pytest.mark.parametrize("dtype", C.DTYPES)
@pytest.mark.parametrize("h", C.HS)
@pytest.mark.parametrize("k", C.KS)
def test_weight_grad_is_within_the_any_order_bar_and_repeats_its_bits(dga, k, h, dtype):
    c, src, grad, dest, _ = _device_case(k, h, dtype)
    ref, bar = C.weight_grad_ref(c["src"], c["grad"], c["dest"])
    out = torch.full((C.T, k), float("nan"), dtype=torch.float32, device="cuda")
    assert dga.combine_tokens_weight_grad(src, grad, dest, out=out) is out
    again = dga.combine_tokens_weight_grad(src, grad, dest, sync=True)
    got = out.cpu().numpy()
    ok = C.valid(c["dest"], C.S)
    err = np.abs(got.astype(np.float64) - ref)
    print(f"k={k} h={h} {dtype}: largest error / bar = {np.max(err[ok] / bar[ok]):.4f}")
    assert np.isfinite(got).all() and (err <= bar).all()
    assert not got.view(np.uint32)[~ok].any()                                  # a dropped choice: exactly +0
    assert np.array_equal(got.view(np.uint32), again.cpu().numpy().view(np.uint32))


def test_unaligned_pointers_take_the_bounded_path_with_the_same_result(dga):
    """H = 384 would take 16-byte accesses; a source, a gradient and an output that start 2 bytes into an allocation may not."""
    c, src, grad, dest, w = _device_case(2, 384, "bf16")
    off = lambda t: torch.cat([t.new_zeros(1), t.reshape(-1)])[1:].view(t.shape)
    src1, grad1 = off(src), off(grad)
    assert src1.data_ptr() % 16 == 2 and src1.is_contiguous()
    out1 = off(torch.full((C.T, 384), float("nan"), dtype=torch.bfloat16, device="cuda"))
    dga.combine_tokens(src1, dest, w, out=out1, sync=True)
    assert np.array_equal(_out_bits(out1), C.round_to(C.combine_ref(c["src"], c["dest"], c["w"]), "bf16"))
    ref, bar = C.weight_grad_ref(c["src"], c["grad"], c["dest"])
    got = dga.combine_tokens_weight_grad(src1, grad1, dest, sync=True).cpu().numpy()
    assert (np.abs(got.astype(np.float64) - ref) <= bar).all()
