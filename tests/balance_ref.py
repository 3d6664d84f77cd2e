"""Not a test file: the float64 references of router_balance_loss and router_balance_loss_backward with the M of the backward's bound, the
three bars, a numpy router_bias_update, and the cases tests/test_router_balance.py (CPU), tests/test_router_balance_gpu.py and
tests/test_router_balance_layer_gpu.py share.  Imports no GPU code.

The bars are the interface's any-order bounds (u = 2^-24, gamma(n) = n u / (1 - n u)), which hold for every order of summation, so for
the kernels' as well.  Their roundings, counted for the order the kernels use: a normalised score costs at most V + 6 (the row sum: V - 1
inside a lane and 6 across the lanes; one division), psum adds one rounding per addition of a chain that is always shorter than L, the
loss one for float(count), one per product, at most E - 1 for the sum over the experts, one for coef as a float and one for the last
product: below L + E + 1 and L + 2 E + 4.  No tighter bar is claimed: the depth of the kernels' chains depends on the chunking, and the
tests hold them to the any-order figures."""
import numpy as np

import router_ref as R

SEGMENTS = 3                                     # B
SEQ_LENS = (1, 37, 50)                           # L; at 50 a segment spans four stage-one chunks, the last of two tokens
ALPHA = 1.5
U = 2.0 ** -24


def gamma(n):
    return n * U / (1.0 - n * U)


def psum_bar(seq_len, e):
    return gamma(seq_len + e + 1)


def loss_bar(seq_len, e):
    return gamma(seq_len + 2 * e + 4)


def backward_bar(e):
    return gamma(4 * e + 8)


def chunk_tokens(tokens):
    """The tokens of a segment one stage-one workgroup takes, as include/dga_hip.h states it."""
    return max(16, 4 * -(-tokens // 2048))


def coef(alpha, e, k, seq_len):
    return alpha * e / (k * seq_len * seq_len)


def counts_ref(ids, e, seq_len):
    """int64 [B, e]: the pairs of each segment per expert; an id outside [0, e) counts nowhere."""
    ids = np.asarray(ids, np.int64)
    t_n = ids.shape[0]
    seg = np.repeat(np.arange(t_n) // seq_len, ids.shape[1])
    flat = ids.reshape(-1)
    ok = (flat >= 0) & (flat < e)
    counts = np.zeros((t_n // seq_len, e), np.int64)
    np.add.at(counts, (seg[ok], flat[ok]), 1)
    return counts


def forward_ref(scores, ids, seq_len, alpha=1.0, normalize=False):
    """(loss float64 [B], counts int64 [B, e], psum float64 [B, e]) on the float64 values of the scores given."""
    s = np.asarray(scores, np.float64)
    t_n, e = s.shape
    counts = counts_ref(ids, e, seq_len)
    with np.errstate(invalid="ignore", divide="ignore"):
        p = s / s.sum(axis=1, keepdims=True) if normalize else s
        psum = p.reshape(t_n // seq_len, seq_len, e).sum(axis=1)
        loss = coef(alpha, e, np.shape(ids)[1], seq_len) * (counts * psum).sum(axis=1)
    return loss, counts, psum


def backward_ref(dloss, counts, scores, k, func, seq_len, alpha=1.0, normalize=False):
    """(ref64 [T, e], M [T, e]): the float64 backward, and the same expression with every term replaced by its absolute value and
    (1 - s) by 1."""
    s = np.asarray(scores, np.float64)
    t_n, e = s.shape
    q = np.asarray(dloss, np.float64)[:, None] * coef(alpha, e, k, seq_len) * np.asarray(counts, np.float64)
    q = np.repeat(q, seq_len, axis=0)                                      # [T, e]: the row of the token's segment
    mq = np.abs(q)
    if normalize:
        tot = s.sum(axis=1, keepdims=True)
        p = s / tot
        ds = (q - (q * p).sum(axis=1, keepdims=True)) / tot
        mds = (mq + (mq * np.abs(p)).sum(axis=1, keepdims=True)) / np.abs(tot)
    else:
        ds, mds = q, mq
    if func == "sigmoid":
        return ds * s * (1.0 - s), mds * np.abs(s)
    return s * (ds - (ds * s).sum(axis=1, keepdims=True)), np.abs(s) * (mds + (mds * np.abs(s)).sum(axis=1, keepdims=True))


def bias_update_ref(bias, counts, rate):
    """float32 [e]: every operation a numpy float32 one, the comparison on integers."""
    n = np.asarray(counts, np.int64).sum(axis=0)
    sgn = np.sign(n.sum() - n.shape[0] * n).astype(np.float32)
    return np.add(np.asarray(bias, np.float32), np.multiply(np.float32(rate), sgn, dtype=np.float32), dtype=np.float32)


def synthetic_case(e, k, seq_len, seed=0):
    """(scores float32 [B L, e] in (0, 1), ids int32 [B L, k] in [-1, e], in no order, with repeats; both ends occur)."""
    rng = np.random.default_rng([seed, e, k, seq_len])
    t_n = SEGMENTS * seq_len
    scores = (rng.random((t_n, e)) * 0.98 + 0.01).astype(np.float32)
    ids = rng.integers(-1, e + 1, size=(t_n, k)).astype(np.int32)
    ids[0, 0], ids[-1, -1] = -1, e
    return scores, ids


def logits_case(e, seq_len, seed=0):
    """float32 [B L, e], exact in bfloat16: what router_topk turns into the scores and ids of the other cases."""
    rng = np.random.default_rng([seed, e, seq_len, 5])
    return R.to_dtype(rng.standard_normal((SEGMENTS * seq_len, e)) * 2.0, "bf16")
