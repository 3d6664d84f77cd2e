"""GPU: what the wrappers' shared helpers own and no single test states for all of them.  Every wrapper that takes out= writes into the
caller's own storage and hands it back -- the same data pointers, codes given as uint8 returned as float8_e4m3fn views of them, no
_dga_zero_padded mark left on a tensor of the caller's --, and without out= returns tensors of the same shapes with float8_e4m3fn codes.
sync=True leaves the stream idle on return.  The smallest shapes with a ragged tail: 3 rows of H = 128 for the fused quantisers, T = 130 tokens
of H = 136 channels for the transposing ones (a second 128-token block, and aligned_rows pads), T 5 / E 8 / k 2 for the router, two segments
of 3 tokens for the balance loss.  The values are the other GPU tests' business."""
import pytest
import torch

pytestmark = pytest.mark.gpu

U8, F32, I32, BF16 = torch.uint8, torch.float32, torch.int32, torch.bfloat16
T, H = 130, 136


def e(*shape, dtype=F32):
    return torch.empty(*shape, dtype=dtype, device="cuda")


def r(*shape, dtype=BF16):
    return torch.randn(*shape, device="cuda").to(dtype)


def _transposed_out():
    return (e(H, 256, dtype=U8)[:, :T], e(H, 2)), (e(T, H, dtype=U8), e(T, 2))


def _cases(dga):
    """name -> (call(out, sync) -> the wrapper's result, make_out() -> the caller's tensors in out='s nesting)."""
    x3, g3, xt, x2t, w = r(3, 256), r(3, 128), r(T, H), r(T, 2 * H), r(H, T)
    index = torch.arange(T, device="cuda")
    src, dest, grad = r(8, H), torch.tensor([[0, 7], [3, -1], [2, 2], [9, 1], [4, 5]], device="cuda"), r(5, H)
    logits = r(5, 8, dtype=F32)
    ids5, w5, s5 = dga.router_topk(logits, 2)
    s6 = torch.softmax(r(6, 8, dtype=F32), dim=1)
    ids6 = torch.tensor([[0, 1], [2, 3], [7, 0], [1, 2], [5, 6], [6, 7]], dtype=I32, device="cuda")
    _, counts, _ = dga.router_balance_loss(s6, ids6, seq_len=3)
    return {
        "silu_and_mul_per_token_cast_to_fp8": (lambda out, sync: dga.silu_and_mul_per_token_cast_to_fp8(x3, out=out, sync=sync),
                                               lambda: (e(3, 128, dtype=U8), e(3, 1))),
        "silu_and_mul_backward_per_token_cast_to_fp8": (
            lambda out, sync: dga.silu_and_mul_backward_per_token_cast_to_fp8(x3, g3, out=out, sync=sync), lambda: (e(3, 256, dtype=U8), e(3, 2))),
        "per_token_cast_to_fp8_transposed": (
            lambda out, sync: dga.per_token_cast_to_fp8_transposed(xt, rowwise=True, aligned_rows=True, out=out, sync=sync), _transposed_out),
        "silu_and_mul_per_token_cast_to_fp8_transposed": (
            lambda out, sync: dga.silu_and_mul_per_token_cast_to_fp8_transposed(x2t, rowwise=True, aligned_rows=True, out=out, sync=sync),
            _transposed_out),
        "gather_per_token_cast_to_fp8_transposed": (
            lambda out, sync: dga.gather_per_token_cast_to_fp8_transposed(xt, index, rowwise=True, aligned_rows=True, out=out, sync=sync),
            _transposed_out),
        "per_token_cast_to_fp8_transposed-flat": (
            lambda out, sync: dga.per_token_cast_to_fp8_transposed(xt, out=out, sync=sync), lambda: (e(H, T, dtype=U8), e(H, 2))),
        "per_block_cast_to_fp8_transposed": (lambda out, sync: dga.per_block_cast_to_fp8_transposed(w, rowwise=True, out=out, sync=sync),
                                             lambda: ((e(T, H, dtype=U8), e(2, 2)), (e(H, T, dtype=U8), e(2, 2)))),
        "combine_tokens": (lambda out, sync: dga.combine_tokens(src, dest, w5, out=out, sync=sync), lambda: e(5, H, dtype=BF16)),
        "combine_tokens_weight_grad": (lambda out, sync: dga.combine_tokens_weight_grad(src, grad, dest, out=out, sync=sync), lambda: e(5, 2)),
        "router_topk": (lambda out, sync: dga.router_topk(logits, 2, out=out, sync=sync), lambda: (e(5, 2, dtype=I32), e(5, 2), e(5, 8))),
        "router_topk_backward": (lambda out, sync: dga.router_topk_backward(w5, s5, ids5, "softmax", out=out, sync=sync), lambda: e(5, 8)),
        "router_balance_loss": (lambda out, sync: dga.router_balance_loss(s6, ids6, seq_len=3, out=out, sync=sync),
                                lambda: (e(2), e(2, 8, dtype=I32), e(2, 8))),
        "router_balance_loss_backward": (
            lambda out, sync: dga.router_balance_loss_backward(torch.ones(2, device="cuda"), counts, s6, 2, "softmax", seq_len=3, out=out, sync=sync),
            lambda: e(6, 8)),
    }


NAMES = ["silu_and_mul_per_token_cast_to_fp8", "silu_and_mul_backward_per_token_cast_to_fp8", "per_token_cast_to_fp8_transposed",
         "silu_and_mul_per_token_cast_to_fp8_transposed", "gather_per_token_cast_to_fp8_transposed", "per_token_cast_to_fp8_transposed-flat",
         "per_block_cast_to_fp8_transposed", "combine_tokens", "combine_tokens_weight_grad", "router_topk", "router_topk_backward",
         "router_balance_loss", "router_balance_loss_backward"]


@pytest.fixture(scope="module")
def cases(dga):
    torch.manual_seed(0)
    got = _cases(dga)
    assert sorted(got) == sorted(NAMES)
    return got


def flat(o):
    return [o] if isinstance(o, torch.Tensor) else [t for m in o for t in flat(m)]


def retag(o):
    if isinstance(o, torch.Tensor):
        return o.view(torch.float8_e4m3fn) if o.dtype == U8 else o
    return tuple(retag(m) for m in o)


def nesting(o):
    return None if isinstance(o, torch.Tensor) else tuple(nesting(m) for m in o)


@pytest.mark.parametrize("name", NAMES)
def test_out_is_the_callers_own_storage(cases, name):
    call, make_out = cases[name]
    mine = make_out()
    got = call(mine, True)
    assert nesting(got) == nesting(mine)
    for g, m in zip(flat(got), flat(mine)):
        assert g.data_ptr() == m.data_ptr() and g.shape == m.shape and g.stride() == m.stride()
        assert g.dtype == (torch.float8_e4m3fn if m.dtype == U8 else m.dtype)
        assert g is m or m.dtype == U8                      # (only the codes are re-tagged)
        assert not hasattr(m, "_dga_zero_padded")           # the promise of zero tails goes on new tensor objects only
    fresh = call(None, True)
    assert nesting(fresh) == nesting(mine)
    for f, m in zip(flat(fresh), flat(mine)):
        assert f.shape == m.shape and f.dtype == (torch.float8_e4m3fn if m.dtype == U8 else m.dtype)
        assert all(f.data_ptr() != other.data_ptr() for other in flat(mine))
    if name in ("silu_and_mul_per_token_cast_to_fp8", "silu_and_mul_backward_per_token_cast_to_fp8", "per_block_cast_to_fp8_transposed"):
        typed = retag(make_out())          # contiguous codes the caller already holds as float8_e4m3fn come back as they are
        for g, m in zip(flat(call(typed, True)), flat(typed)):
            assert g is m


@pytest.mark.parametrize("name", ["silu_and_mul_per_token_cast_to_fp8", "per_token_cast_to_fp8_transposed", "per_block_cast_to_fp8_transposed",
                                  "combine_tokens", "router_topk", "router_balance_loss"])
def test_sync_leaves_the_stream_idle(cases, name):
    """One wrapper of each family.  A few milliseconds of matrix products are queued first: without the synchronise the stream is still busy
    when the wrapper returns."""
    call, _ = cases[name]
    big = torch.ones(4096, 4096, device="cuda")
    torch.cuda.synchronize()
    for _ in range(8):
        big = (big @ big) * 2.0 ** -12
    call(None, True)
    assert torch.cuda.current_stream().query()
