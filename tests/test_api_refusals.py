"""CPU: the argument checks of the Python wrappers that no other test pins, message by message.  Every wrapper runs all of its checks before
the device guard, which refuses host tensors ("no CPU path"), so a table of (wrapper, valid arguments with one fault, the whole message) needs
no GPU: the valid arguments alone reach the guard -- each fault is refused by its own check --, and two faults at once show which check runs
first.  Messages are compared as whole strings.  The last tests hold the helpers to the rule at the top of api.py: a check that passes formats
nothing."""
import inspect
import re

import pytest
import torch

import deepgemm_ascend_amd as dga
from deepgemm_ascend_amd import _lib, api

I32, I64, F32, F64, BF16, F16, U8 = torch.int32, torch.int64, torch.float32, torch.float64, torch.bfloat16, torch.float16, torch.uint8


def z(*shape, dtype=F32):
    return torch.zeros(*shape, dtype=dtype)


FP8_MSG = "fp8 operand must be float8_e4m3fn or uint8 bytes, got torch.float32"
STRIDE_MSG = "operands must be row-major with unit inner stride (row-strided views are accepted)"
DTYPES_MSG = "float32, bfloat16 or float16"
SCORES_MSG = "scores must be a contiguous float32 [T, E] tensor"
FUNC_MSG = 'score_func must be "softmax" or "sigmoid"'

# wrapper -> its valid arguments (host tensors, the smallest shapes the checks tell apart): lhs / rhs pairs are split into a, sfa, b, sfb
VALID = {
    "gemm_fp8_fp8_bf16_nt": lambda: dict(a=z(4, 256, dtype=U8), sfa=z(4, 2), b=z(8, 256, dtype=U8), sfb=z(1, 2), out=z(4, 8, dtype=BF16)),
    "gemm_fp8_fp8_fp32_nt": lambda: dict(a=z(4, 256, dtype=U8), sfa=z(4, 2), b=z(8, 256, dtype=U8), sfb=z(1, 2), out=z(4, 8)),
    "wgrad_gemm_fp8_fp8_fp32_nt": lambda: dict(a=z(4, 256, dtype=U8), sfa=z(4, 2), b=z(8, 256, dtype=U8), sfb=z(8, 2), out=z(4, 8)),
    "k_grouped_wgrad_gemm_fp8_fp8_fp32_nt": lambda: dict(a=z(4, 256, dtype=U8), sfa=z(4, 2), b=z(8, 256, dtype=U8), sfb=z(8, 2), out=z(2, 4, 8),
                                                         ks=[128, 128]),
    "m_grouped_gemm_fp8_fp8_bf16_nt_masked": lambda: dict(a=z(2, 4, 256, dtype=U8), sfa=z(2, 4, 2), b=z(2, 8, 256, dtype=U8), sfb=z(2, 1, 2),
                                                          out=z(2, 4, 8, dtype=BF16), masked_m=z(2, dtype=I32), expected_m=4),
    "m_grouped_gemm_fp8_fp8_bf16_nt_masked_indexed": lambda: dict(
        a_rows=z(8, 256, dtype=U8), sfa_src=z(8, 2), sfa_byte_offset=0, sfa_ld=2, b=z(2, 8, 256, dtype=U8), sfb=z(2, 1, 2),
        out_rows=z(8, 8, dtype=BF16), row_index=z(8, dtype=I64), masked_m=z(2, dtype=I32), m_max=4),
    "m_grouped_gemm_fp8_fp8_bf16_nt_contiguous": lambda: dict(a=z(8, 256, dtype=U8), sfa=z(8, 2), b=z(2, 8, 256, dtype=U8), sfb=z(2, 1, 2),
                                                              out=z(8, 8, dtype=BF16), m_indices=z(8, dtype=I32)),
    "catlass_dynamic_matmul": lambda: dict(self_=z(4, 16, dtype=BF16), mat2=z(8, 16, dtype=BF16).t(), out=z(4, 8, dtype=BF16)),
    "per_token_cast_to_fp8": lambda: dict(x=z(3, 130)),
    "per_block_cast_to_fp8": lambda: dict(x=z(3, 130)),
    "silu_and_mul_per_token_cast_to_fp8": lambda: dict(x=z(3, 256), out=(z(3, 128, dtype=U8), z(3, 1))),
    "route_tokens": lambda: dict(expert_ids=z(5, dtype=I64), groups=4),
    "route_slots": lambda: dict(keys=z(6, dtype=I32), key_stride_bytes=4, rows=6, buckets=2, cap=4, counts=z(2, dtype=I32), dest=z(6, dtype=I64),
                                overflow=z(1, dtype=I32), inverse=z(8, dtype=I64)),
    "copy_rows": lambda: dict(dst=z(4, 16, dtype=U8), src=z(4, 16, dtype=U8), dst_index=z(4, dtype=I64), src_index=z(4, dtype=I64)),
    "copy_rows2": lambda: dict(dst0=z(4, 16, dtype=U8), src0=z(4, 16, dtype=U8), bytes0=16, dst1=z(4, 8, dtype=U8), src1=z(4, 8, dtype=U8),
                               bytes1=8, dst_index=z(4, dtype=I64)),
    "router_topk": lambda: dict(logits=z(5, 8), k=2, bias=z(8), out=(z(5, 2, dtype=I32), z(5, 2), z(5, 8))),
    "router_topk_backward": lambda: dict(dw=z(5, 2), scores=z(5, 8), ids=z(5, 2, dtype=I32), score_func="softmax", out=z(5, 8, dtype=BF16)),
    "router_balance_loss": lambda: dict(scores=z(6, 8), ids=z(6, 2, dtype=I32), seq_len=3, out=(z(2), z(2, 8, dtype=I32), z(2, 8))),
    "router_balance_loss_backward": lambda: dict(dloss=z(2), counts=z(2, 8, dtype=I32), scores=z(6, 8), k=2, score_func="sigmoid", seq_len=3,
                                                 add_to=z(6, 8), out=z(6, 8, dtype=F16)),
    "router_bias_update": lambda: dict(bias=z(8), counts=z(2, 8, dtype=I32), rate=0.5),
    "mla_kv_cast_to_fp8_paged": lambda: dict(kv_c=z(3, 512, dtype=BF16), k_pe=z(3, 64, dtype=BF16), kv_cache=z(2, 2, 1, 656, dtype=U8),
                                             slot_mapping=z(3, dtype=I64)),
    "sparse_mla_merge": lambda: dict(partial_out=z(2, 2, 16, 512), partial_lse=z(2, 2, 16), out=z(2, 16, 512, dtype=BF16), lse=z(2, 16)),
}


def _smla_valid(fp8, outputs):
    """the attention forms of sparse MLA: M = 2, Hq = 16, 4 rows, topk = 40 (two tiles, so that num_splits = 2 is P = 2)"""
    rows = dict(kv_cache=z(2, 2, 1, 656, dtype=U8)) if fp8 else dict(kv=z(4, 576, dtype=BF16))
    return lambda: dict(q=z(2, 16, 576, dtype=BF16), **rows, indices=z(2, 40, dtype=I32), sm_scale=0.1, index_offsets=z(2, dtype=I32),
                        **outputs())


SMLA_OUT = lambda: dict(out=z(2, 16, 512, dtype=BF16), lse=z(2, 16))
SMLA_PARTIAL = lambda: dict(num_splits=2, partial_out=z(2, 2, 16, 512), partial_lse=z(2, 2, 16))
SMLA_SPLIT = lambda: dict(num_splits=2, **SMLA_OUT())
SMLA_FORMS = [("sparse_mla_fwd", False, SMLA_OUT), ("sparse_mla_fwd_fp8", True, SMLA_OUT), ("sparse_mla_fwd_partial", False, SMLA_PARTIAL),
              ("sparse_mla_fwd_fp8_partial", True, SMLA_PARTIAL), ("sparse_mla_fwd_split", False, SMLA_SPLIT),
              ("sparse_mla_fwd_fp8_split", True, SMLA_SPLIT)]
VALID.update({name: _smla_valid(fp8, outputs) for name, fp8, outputs in SMLA_FORMS})


def call(name, kw):
    kw = dict(kw)
    if "sfa" in kw:
        kw["lhs"] = (kw.pop("a"), kw.pop("sfa"))
    if "sfb" in kw:
        kw["rhs"] = (kw.pop("b"), kw.pop("sfb"))
    return getattr(dga, name)(**kw)


DENSE = [   # _dense_fp8_operands, in its order; {out}: the output's dtype by name
    (dict(a=z(4, 256)), FP8_MSG), (dict(b=z(8, 256)), FP8_MSG), (dict(a=z(1, 4, 256, dtype=U8)), "rank must be 2"),
    (dict(b=z(8, 128, dtype=U8)), "self dimk is not equal with mat2 dimk"), (dict(out="[4,9]"), "out must be [4,8]"),
    (dict(out=z(4, 8, dtype=F16)), "out must be {out}"), (dict(sfa=z(4, 2, dtype=F64)), "scales must be float32"),
    (dict(sfb=z(1, 2, dtype=F64)), "scales must be float32"), (dict(sfa=z(4, 3)), "sfa must be [4,2]"), (dict(sfa=z(8)), "sfa must be [4,2]"),
    (dict(sfb=z(2, 3)), "sfb must be {sfb}"), (dict(sfa=z(4, 4)[:, :2]), "scales and out must be contiguous"),
    (dict(a=z(4, 512, dtype=U8)[:, ::2]), STRIDE_MSG), (dict(b=z(8, 512, dtype=U8)[:, ::2]), STRIDE_MSG),
    (dict(b=z(256, 8, dtype=U8).t()), STRIDE_MSG),
    # two faults: the earlier check reports
    (dict(a=z(4, 256), out=z(4, 8, dtype=F16)), FP8_MSG), (dict(out=z(4, 8, dtype=F16), sfa=z(4, 3)), "out must be {out}"),
]
FP32_C = [  # the accumuland of the fp32-output entries, after the operands
    (dict(policy="fast"), "{name}: policy must be one of ['bf16_exact', 'strict']"),
    (dict(strict=True, policy="bf16_exact"), "strict=True contradicts policy='bf16_exact'"),
    (dict(c=z(4, 8, dtype=BF16)), "c must be float32"), (dict(c=z(4, 9)), "c must be [4,8]"), (dict(c=z(32)), "c must be [4,8]"),
    (dict(c=z(4, 16)[:, :8]), "c must be contiguous"), (dict(c="overlap"), "c must be out itself or not overlap it"),
    (dict(policy="fast", a=z(4, 256)), "{name}: policy must be one of ['bf16_exact', 'strict']"), (dict(c=z(4, 9, dtype=BF16)), "c must be float32"),
    (dict(sfa=z(4, 3), c=z(4, 9)), "sfa must be [4,2]"),
]


def _dense(name, out, sfb, more=()):
    rows = []
    for fault, msg in list(DENSE) + list(more):
        fault = dict(fault)
        if isinstance(fault.get("out"), str):
            fault["out"] = z(4, 9, dtype=VALID[name]()["out"].dtype)
        rows.append((name, fault, msg.format(out=out, sfb=sfb, name=name)))
    return rows


# Sparse MLA: six attention forms (one-pass, partial, split; over bf16 rows or the paged fp8 cache), the merge, and the cache's writer.
# The forms check in one order -- q, the rows, indices, num_splits, the outputs -- and share the wording of each part.
Q_MSG = "q must be a contiguous bfloat16 [M, Hq, 576] tensor"
KV_MSG = "kv must be a bfloat16 [S, 576] or [S, 1, 576] tensor"
KV_STRIDE_MSG = "kv must have a contiguous last dimension and a stride(0) >= 576 that is a multiple of 8, got %d"
QKV_ALIGN_MSG = "q and kv must be 16-byte aligned"
CACHE_ROWS_MSG = "kv_cache must have contiguous rows, 656 bytes apart inside a block (stride(1) == 656)"
CACHE_STRIDE_MSG = "kv_cache blocks must be at least %d bytes apart and a multiple of 16, got stride(0) = %d"
IDX_MSG = "indices must be an int32 [M, topk] or [M, 1, topk] tensor with topk >= 1"
IDX_STRIDE_MSG = "indices must have a contiguous last dimension and stride(0) >= topk"
SPLITS_MSG = "num_splits must be an int in [1, 64], got %s"
OUT_MSG, LSE_MSG = "out must be contiguous bfloat16 [2, 16, 512]", "lse must be contiguous float32 [2, 16]"
PO_MSG, PL_MSG = "partial_out must be contiguous float32 [>= 2, 2, 16, 512]", "partial_lse must be contiguous float32 [>= 2, 2, 16]"


def misaligned(*shape, dtype, by=8):
    """a contiguous tensor that starts `by` bytes past a 16-byte boundary"""
    skip, n = by // z(1, dtype=dtype).element_size(), 1
    for d in shape:
        n *= d
    return z(skip + n, dtype=dtype)[skip:].view(*shape)


SMLA_QUERY = [
    (dict(q=z(2, 16, 576)), Q_MSG), (dict(q=z(16, 576, dtype=BF16)), Q_MSG), (dict(q=z(2, 16, 512, dtype=BF16)), Q_MSG),
    (dict(q=z(2, 32, 576, dtype=BF16)[:, ::2]), Q_MSG), (dict(q=z(2, 8, 576, dtype=BF16)), "Hq must be a multiple of 16 in [16, 128], got 8"),
    (dict(q=z(2, 144, 576, dtype=BF16)), "Hq must be a multiple of 16 in [16, 128], got 144"), (dict(d_v=576), "d_v must be 512"),
    (dict(sm_scale="0.1"), "sm_scale must be a number"),
]
SMLA_BF16_ROWS = [
    (dict(kv=z(4, 576, dtype=F16)), KV_MSG), (dict(kv=z(2, 2, 576, dtype=BF16)), KV_MSG), (dict(kv=z(4, 512, dtype=BF16)), KV_MSG),
    (dict(kv=z(0, 576, dtype=BF16)), "kv must have between 1 and 2^31 - 1 rows, got 0"),
    (dict(kv=torch.empty((1 << 31, 576), dtype=BF16, device="meta")), "kv must have between 1 and 2^31 - 1 rows, got 2147483648"),
    (dict(kv=z(4, 1152, dtype=BF16)[:, ::2]), KV_STRIDE_MSG % 1152), (dict(kv=z(4, 580, dtype=BF16)[:, :576]), KV_STRIDE_MSG % 580),
    (dict(kv=z(4 * 576, dtype=BF16).as_strided((4, 576), (568, 1))), KV_STRIDE_MSG % 568),
    (dict(kv=misaligned(4, 576, dtype=BF16)), QKV_ALIGN_MSG), (dict(q=misaligned(2, 16, 576, dtype=BF16)), QKV_ALIGN_MSG),
    # two faults: q before the rows, the rows before indices
    (dict(q=z(2, 16, 576), kv=z(4, 512, dtype=BF16)), Q_MSG), (dict(sm_scale=None, kv=z(0, 576, dtype=BF16)), "sm_scale must be a number"),
    (dict(kv=z(4, 580, dtype=BF16)[:, :576], indices=z(2, 40, dtype=I64)), KV_STRIDE_MSG % 580),
    (dict(q=misaligned(2, 16, 576, dtype=BF16), indices=z(2, 0, dtype=I32)), QKV_ALIGN_MSG),
]
MLA_FP8_CACHE = [   # _mla_fp8_cache, in its order: the attention forms' and the writer's
    (dict(kv_cache=z(2, 2, 1, 656, dtype=torch.int8)), "kv_cache must be uint8, got torch.int8"),
    (dict(kv_cache=z(2, 2, 656, dtype=U8)), "kv_cache must be [num_blocks, page_size, 1, 656] or [S, 656], got [2, 2, 656]"),
    (dict(kv_cache=z(4, 576, dtype=U8)), "kv_cache must be [num_blocks, page_size, 1, 656] or [S, 656], got [4, 576]"),
    (dict(kv_cache=z(2, 1, 2, 656, dtype=U8)), "kv_cache must be [num_blocks, page_size, 1, 656] or [S, 656], got [2, 1, 2, 656]"),
    (dict(kv_cache=z(0, 2, 1, 656, dtype=U8)), "kv_cache must have at least one row"), (dict(kv_cache=z(2, 0, 1, 656, dtype=U8)), "kv_cache must have at least one row"),
    (dict(kv_cache=z(2, 2, 1, 672, dtype=U8)[..., :656]), CACHE_ROWS_MSG), (dict(kv_cache=z(4, 1312, dtype=U8)[:, ::2]), CACHE_ROWS_MSG),
    (dict(kv_cache=z(2, 2 * 656 + 8, dtype=U8)[:, :2 * 656].view(2, 2, 1, 656)), CACHE_STRIDE_MSG % (1312, 1320)),
    (dict(kv_cache=z(4, 664, dtype=U8)[:, :656]), CACHE_STRIDE_MSG % (656, 664)),
    (dict(kv_cache=z(2 * 2 * 656, dtype=U8).as_strided((2, 2, 1, 656), (656 + 16, 656, 656, 1))), CACHE_STRIDE_MSG % (1312, 672)),
    (dict(kv_cache=torch.empty((1 << 25, 64, 1, 656), dtype=U8, device="meta")), "kv_cache must have fewer than 2^31 rows, got 33554432 x 64"),
    (dict(kv_cache=misaligned(2, 2, 1, 656, dtype=U8)), "kv_cache must be 16-byte aligned"),
    # two faults inside the cache: the shape before the stride before the alignment
    (dict(kv_cache=z(2, 2 * 656 + 8, dtype=torch.int8)[:, :2 * 656].view(2, 2, 1, 656)), "kv_cache must be uint8, got torch.int8"),
    (dict(kv_cache=misaligned(2, 2 * 656 + 8, dtype=U8)[:, :2 * 656].view(2, 2, 1, 656)), CACHE_STRIDE_MSG % (1312, 1320)),
]
SMLA_FP8_ROWS = MLA_FP8_CACHE + [
    (dict(q=misaligned(2, 16, 576, dtype=BF16)), "q must be 16-byte aligned"),
    # two faults: q before the cache, the cache before q's alignment before indices
    (dict(q=z(2, 16, 576), kv_cache=z(4, 576, dtype=U8)), Q_MSG), (dict(d_v=256, kv_cache=z(0, 2, 1, 656, dtype=U8)), "d_v must be 512"),
    (dict(kv_cache=misaligned(2, 2, 1, 656, dtype=U8), q=misaligned(2, 16, 576, dtype=BF16)), "kv_cache must be 16-byte aligned"),
    (dict(kv_cache=z(4, 664, dtype=U8)[:, :656], indices=z(2, 40, dtype=I64)), CACHE_STRIDE_MSG % (656, 664)),
    (dict(q=misaligned(2, 16, 576, dtype=BF16), indices=z(2, 0, dtype=I32)), "q must be 16-byte aligned"),
]
SMLA_INDICES = [
    (dict(indices=z(2, 40, dtype=I64)), IDX_MSG), (dict(indices=z(40, dtype=I32)), IDX_MSG), (dict(indices=z(1, 40, dtype=I32)), IDX_MSG),
    (dict(indices=z(2, 0, dtype=I32)), IDX_MSG), (dict(indices=z(2, 2, 40, dtype=I32)), IDX_MSG),
    (dict(indices=z(2, 80, dtype=I32)[:, ::2]), IDX_STRIDE_MSG), (dict(indices=z(2 * 40, dtype=I32).as_strided((2, 40), (32, 1))), IDX_STRIDE_MSG),
    (dict(index_offsets=z(2, dtype=I64)), "index_offsets must be contiguous int32 [2]"),
    (dict(index_offsets=z(3, dtype=I32)), "index_offsets must be contiguous int32 [2]"),
    (dict(indices=z(2, 40, dtype=I64), index_offsets=z(3, dtype=I32)), IDX_MSG),
]
SMLA_NUM_SPLITS = [
    (dict(num_splits=0), SPLITS_MSG % "0"), (dict(num_splits=65), SPLITS_MSG % "65"), (dict(num_splits=2.0), SPLITS_MSG % "2.0"),
    (dict(num_splits=True), SPLITS_MSG % "True"),
    # two faults: indices before num_splits
    (dict(indices=z(2, 80, dtype=I32)[:, ::2], num_splits=0), IDX_STRIDE_MSG), (dict(index_offsets=z(3, dtype=I32), num_splits=65), "index_offsets must be contiguous int32 [2]"),
]
SMLA_OUTPUTS = {
    SMLA_OUT: [
        (dict(out=z(2, 16, 576, dtype=BF16)), OUT_MSG), (dict(out=z(2, 16, 512)), OUT_MSG), (dict(out=z(2, 16, 1024, dtype=BF16)[..., ::2]), OUT_MSG),
        (dict(lse=z(2, 16, 1)), LSE_MSG), (dict(lse=z(2, 16, dtype=BF16)), LSE_MSG),
        # two faults: indices before the outputs, out before lse
        (dict(index_offsets=z(3, dtype=I32), out=z(2, 16, 512)), "index_offsets must be contiguous int32 [2]"),
        (dict(out=z(2, 16, 512), lse=z(2, 16, 1)), OUT_MSG),
    ],
    SMLA_PARTIAL: SMLA_NUM_SPLITS + [
        (dict(num_splits=None), SPLITS_MSG % "None"),
        (dict(partial_out=z(2, 2, 16, 512, dtype=BF16)), PO_MSG), (dict(partial_out=z(1, 2, 16, 512)), PO_MSG),
        (dict(partial_out=z(2, 2, 16, 576)), PO_MSG), (dict(partial_out=z(2, 16, 512)), PO_MSG), (dict(partial_out=z(4, 2, 16, 512)[::2]), PO_MSG),
        (dict(partial_lse=z(2, 2, 16, dtype=F64)), PL_MSG), (dict(partial_lse=z(2, 2, 16, 1)), PL_MSG), (dict(partial_lse=z(1, 2, 16)), PL_MSG),
        # a list of one tile: P = min(num_splits, 1), and the buffers need hold no more
        (dict(indices=z(2, 32, dtype=I32), partial_out=z(1, 2, 16, 576)), "partial_out must be contiguous float32 [>= 1, 2, 16, 512]"),
        # two faults: num_splits before partial_out before partial_lse
        (dict(num_splits=0, partial_out=z(2, 16, 512)), SPLITS_MSG % "0"), (dict(partial_out=z(2, 16, 512), partial_lse=z(1, 2, 16)), PO_MSG),
    ],
    SMLA_SPLIT: SMLA_NUM_SPLITS + [
        (dict(out=z(2, 16, 576, dtype=BF16)), OUT_MSG), (dict(lse=z(2, 16, dtype=BF16)), LSE_MSG),
        # two faults: num_splits before out before lse
        (dict(num_splits=65, out=z(2, 16, 512)), SPLITS_MSG % "65"), (dict(out=z(2, 16, 512), lse=z(2, 16, 1)), OUT_MSG),
    ],
}


def _smla(name, fp8, outputs):
    rows = SMLA_QUERY + (SMLA_FP8_ROWS if fp8 else SMLA_BF16_ROWS) + SMLA_INDICES + SMLA_OUTPUTS[outputs]
    if outputs is SMLA_SPLIT:
        # num_splits=None checks what an explicit num_splits checks, in the same order.  NEW ORDER: the rows with one fault in q's alignment
        # or the row source and one in indices report the former since the forms share one checker; until then None alone checked indices
        # first, and reported the latter.
        rows = rows + [({**fault, "num_splits": None}, msg) for fault, msg in rows if "num_splits" not in fault]
    return [(name, fault, msg) for fault, msg in rows]


PO4_MSG = "partial_out must be a contiguous float32 [P, M, Hq, 512] tensor"
SMLA_CASES = [row for form in SMLA_FORMS for row in _smla(*form)] + [
    ("sparse_mla_merge", dict(partial_out=z(2, 2, 16, 512, dtype=F64)), PO4_MSG), ("sparse_mla_merge", dict(partial_out=z(2, 16, 512)), PO4_MSG),
    ("sparse_mla_merge", dict(partial_out=z(2, 2, 16, 576)), PO4_MSG), ("sparse_mla_merge", dict(partial_out=z(4, 2, 16, 512)[::2]), PO4_MSG),
    ("sparse_mla_merge", dict(partial_out=z(0, 2, 16, 512), partial_lse=z(0, 2, 16)), "partial_out must hold between 1 and 64 splits, got 0"),
    ("sparse_mla_merge", dict(partial_out=torch.empty((65, 2, 16, 512), device="meta")), "partial_out must hold between 1 and 64 splits, got 65"),
    ("sparse_mla_merge", dict(partial_out=z(2, 2, 24, 512)), "Hq must be a multiple of 16 in [16, 128], got 24"),
    ("sparse_mla_merge", dict(partial_lse=z(2, 2, 16, dtype=F64)), "partial_lse must be contiguous float32 [2, 2, 16]"),
    ("sparse_mla_merge", dict(partial_lse=z(1, 2, 16)), "partial_lse must be contiguous float32 [2, 2, 16]"),
    ("sparse_mla_merge", dict(partial_lse=z(2, 2, 32)[..., ::2]), "partial_lse must be contiguous float32 [2, 2, 16]"),
    ("sparse_mla_merge", dict(partial_out=misaligned(2, 2, 16, 512, dtype=F32)), "partial_out must be 16-byte aligned"),
    ("sparse_mla_merge", dict(out=z(2, 16, 576, dtype=BF16)), OUT_MSG), ("sparse_mla_merge", dict(out=z(2, 16, 512)), OUT_MSG),
    ("sparse_mla_merge", dict(lse=z(2, 2, 16)), LSE_MSG), ("sparse_mla_merge", dict(lse=z(2, 16, dtype=F16)), LSE_MSG),
    # two faults: partial_out before partial_lse before its alignment before out before lse
    ("sparse_mla_merge", dict(partial_out=z(2, 2, 16, 576), partial_lse=z(1, 2, 16)), PO4_MSG),
    ("sparse_mla_merge", dict(partial_out=misaligned(2, 2, 16, 512, dtype=F32), partial_lse=z(1, 2, 16)), "partial_lse must be contiguous float32 [2, 2, 16]"),
    ("sparse_mla_merge", dict(partial_lse=z(1, 2, 16), out=z(2, 16, 512)), "partial_lse must be contiguous float32 [2, 2, 16]"),
    ("sparse_mla_merge", dict(partial_out=misaligned(2, 2, 16, 512, dtype=F32), out=z(2, 16, 512)), "partial_out must be 16-byte aligned"),
    ("sparse_mla_merge", dict(out=z(2, 16, 512), lse=z(2, 2, 16)), OUT_MSG),
] + [("mla_kv_cast_to_fp8_paged", fault, msg) for fault, msg in [
    (dict(kv_c=z(3, 576, dtype=BF16)), "kv_c must be a [T, 512] tensor"), (dict(kv_c=z(512, dtype=BF16)), "kv_c must be a [T, 512] tensor"),
    (dict(k_pe=z(3, 128, dtype=BF16)), "k_pe must be a [T, 64] tensor with kv_c's T"), (dict(k_pe=z(2, 64, dtype=BF16)), "k_pe must be a [T, 64] tensor with kv_c's T"),
    (dict(kv_c=z(3, 512, dtype=F64), k_pe=z(3, 64, dtype=F64)), "kv_c must be float32, bfloat16 or float16"),
    (dict(k_pe=z(3, 64, dtype=F16)), "kv_c and k_pe must have one dtype, got torch.bfloat16 and torch.float16"),
    (dict(kv_c=z(3, 1024, dtype=BF16)[:, ::2]), "kv_c must have a contiguous last dimension, a 16-byte aligned base and rows a multiple of 16 bytes apart"),
    (dict(kv_c=z(3, 516, dtype=BF16)[:, :512]), "kv_c must have a contiguous last dimension, a 16-byte aligned base and rows a multiple of 16 bytes apart"),
    (dict(k_pe=z(3, 72, dtype=BF16)[:, 4:68]), "k_pe must have a contiguous last dimension, a 16-byte aligned base and rows a multiple of 16 bytes apart"),
    (dict(slot_mapping=z(3, dtype=I32)), "slot_mapping must be contiguous int64 [3]"), (dict(slot_mapping=z(2, dtype=I64)), "slot_mapping must be contiguous int64 [3]"),
    (dict(slot_mapping=z(6, dtype=I64)[::2]), "slot_mapping must be contiguous int64 [3]"),
    # two faults: the inputs before the cache before slot_mapping
    (dict(k_pe=z(3, 72, dtype=BF16)[:, 4:68], kv_cache=z(4, 576, dtype=U8)), "k_pe must have a contiguous last dimension, a 16-byte aligned base and rows a multiple of 16 bytes apart"),
    (dict(kv_cache=z(0, 2, 1, 656, dtype=U8), slot_mapping=z(3, dtype=I32)), "kv_cache must have at least one row"),
] + MLA_FP8_CACHE]

CASES = _dense("gemm_fp8_fp8_bf16_nt", "bfloat16", "[1,2]") + _dense("gemm_fp8_fp8_fp32_nt", "float32", "[1,2]", FP32_C) + \
    _dense("wgrad_gemm_fp8_fp8_fp32_nt", "float32", "[8,2]", FP32_C) + [
    ("k_grouped_wgrad_gemm_fp8_fp8_fp32_nt", dict(policy="auto"), "k_grouped_wgrad_gemm_fp8_fp8_fp32_nt: policy must be one of ['bf16_exact', 'strict']"),
    ("k_grouped_wgrad_gemm_fp8_fp8_fp32_nt", dict(strict=True, policy="bf16_exact"), "strict=True contradicts policy='bf16_exact'"),
    ("k_grouped_wgrad_gemm_fp8_fp8_fp32_nt", dict(b=z(8, 256)), FP8_MSG),
    ("k_grouped_wgrad_gemm_fp8_fp8_fp32_nt", dict(a=z(1, 4, 256, dtype=U8)), "A and B must be rank 2"),
    ("k_grouped_wgrad_gemm_fp8_fp8_fp32_nt", dict(out=z(4, 8)), "out must be a contiguous float32 [G, M, N]"),
    ("k_grouped_wgrad_gemm_fp8_fp8_fp32_nt", dict(out=z(2, 4, 8, dtype=BF16)), "out must be a contiguous float32 [G, M, N]"),
    ("k_grouped_wgrad_gemm_fp8_fp8_fp32_nt", dict(out=z(2, 4, 9)), "A must be [4, K_total] and B [9, K_total] with out [2, 4, 9]"),
    ("k_grouped_wgrad_gemm_fp8_fp8_fp32_nt", dict(a=z(4, 200, dtype=U8), b=z(8, 200, dtype=U8)), "K_total must be a multiple of 128"),
    ("k_grouped_wgrad_gemm_fp8_fp8_fp32_nt", dict(sfb=z(8, 2, dtype=F64)), "scales must be float32"),
    ("k_grouped_wgrad_gemm_fp8_fp8_fp32_nt", dict(sfa=z(4, 3)), "sfa must be [4,2]"),
    ("k_grouped_wgrad_gemm_fp8_fp8_fp32_nt", dict(sfb=z(1, 2)), "sfb must be [8,2] (one scale per row of B: per_token_cast_to_fp8)"),
    ("k_grouped_wgrad_gemm_fp8_fp8_fp32_nt", dict(sfb=z(8, 4)[:, :2]), "scales must be contiguous"),
    ("k_grouped_wgrad_gemm_fp8_fp8_fp32_nt", dict(a=z(4, 512, dtype=U8)[:, ::2]), STRIDE_MSG),
    ("k_grouped_wgrad_gemm_fp8_fp8_fp32_nt", dict(a=z(4, 264, dtype=U8)[:, :256]), "row strides of A and B must be multiples of 16 bytes"),
    ("k_grouped_wgrad_gemm_fp8_fp8_fp32_nt", dict(ks=[128]), "ks must hold 2 counts, one per group"),
    ("k_grouped_wgrad_gemm_fp8_fp8_fp32_nt", dict(ks=[100, 128]), "every ks[g] must be >= 0 and a multiple of 128"),
    ("k_grouped_wgrad_gemm_fp8_fp8_fp32_nt", dict(ks=[256, 128]), "sum(ks) = 384 exceeds K_total = 256"),
    ("k_grouped_wgrad_gemm_fp8_fp8_fp32_nt", dict(ks_tensor=z(2, dtype=I64)), "ks_tensor must be a contiguous int32 [2]"),
    ("k_grouped_wgrad_gemm_fp8_fp8_fp32_nt", dict(c=z(2, 4, 8, dtype=BF16)), "c must be a contiguous float32 [2, 4, 8]"),
    ("k_grouped_wgrad_gemm_fp8_fp8_fp32_nt", dict(c=z(4, 8)), "c must be a contiguous float32 [2, 4, 8]"),
    ("k_grouped_wgrad_gemm_fp8_fp8_fp32_nt", dict(c="overlap"), "c must be out itself or not overlap it"),
    ("k_grouped_wgrad_gemm_fp8_fp8_fp32_nt", dict(sfa=z(4, 3), ks=[128]), "sfa must be [4,2]"),
    ("k_grouped_wgrad_gemm_fp8_fp8_fp32_nt", dict(ks=[128], c=z(4, 8)), "ks must hold 2 counts, one per group"),

    ("m_grouped_gemm_fp8_fp8_bf16_nt_masked", dict(a=z(2, 4, 256)), FP8_MSG),
    ("m_grouped_gemm_fp8_fp8_bf16_nt_masked", dict(a=z(8, 256, dtype=U8)), "rank must be 3"),
    ("m_grouped_gemm_fp8_fp8_bf16_nt_masked", dict(b=z(3, 8, 256, dtype=U8)), "group / k mismatch"),
    ("m_grouped_gemm_fp8_fp8_bf16_nt_masked", dict(b=z(2, 8, 128, dtype=U8)), "group / k mismatch"),
    ("m_grouped_gemm_fp8_fp8_bf16_nt_masked", dict(out=z(2, 4, 8)), "out must be [G,Mmax,N] bfloat16"),
    ("m_grouped_gemm_fp8_fp8_bf16_nt_masked", dict(out=z(2, 4, 9, dtype=BF16)), "out must be [G,Mmax,N] bfloat16"),
    ("m_grouped_gemm_fp8_fp8_bf16_nt_masked", dict(sfa=z(2, 4, 3)), "sfa must be [2,4,2] f32"),
    ("m_grouped_gemm_fp8_fp8_bf16_nt_masked", dict(sfb=z(2, 1, 2, dtype=F64)), "sfb must be [2,1,2] f32"),
    ("m_grouped_gemm_fp8_fp8_bf16_nt_masked", dict(masked_m=z(2, dtype=I64)), "masked_m must be int32 [G]"),
    ("m_grouped_gemm_fp8_fp8_bf16_nt_masked", dict(masked_m=z(3, dtype=I32)), "masked_m must be int32 [G]"),
    ("m_grouped_gemm_fp8_fp8_bf16_nt_masked", dict(out=z(2, 4, 16, dtype=BF16)[:, :, :8]), "operands must be contiguous"),
    ("m_grouped_gemm_fp8_fp8_bf16_nt_masked", dict(a=z(8, 256, dtype=U8), out=z(2, 4, 8)), "rank must be 3"),
    ("m_grouped_gemm_fp8_fp8_bf16_nt_masked", dict(sfb=z(2, 2, 2), masked_m=z(2, dtype=I64)), "sfb must be [2,1,2] f32"),

    ("m_grouped_gemm_fp8_fp8_bf16_nt_masked_indexed", dict(b=z(2, 8, 256)), FP8_MSG),
    ("m_grouped_gemm_fp8_fp8_bf16_nt_masked_indexed", dict(a_rows=z(2, 4, 256, dtype=U8)), "2-D row tensors"),
    ("m_grouped_gemm_fp8_fp8_bf16_nt_masked_indexed", dict(out_rows=z(8, 8)), "row widths"),
    ("m_grouped_gemm_fp8_fp8_bf16_nt_masked_indexed", dict(a_rows=z(8, 128, dtype=U8)), "row widths"),
    ("m_grouped_gemm_fp8_fp8_bf16_nt_masked_indexed", dict(out_rows=z(4, 8, dtype=BF16)), "out_rows must have a row for every source row"),
    ("m_grouped_gemm_fp8_fp8_bf16_nt_masked_indexed", dict(sfb=z(2, 2, 2)), "sfb must be [2,1,2] f32"),
    ("m_grouped_gemm_fp8_fp8_bf16_nt_masked_indexed", dict(row_index=z(8, dtype=I32)), "row_index int64[G*m_max]"),
    ("m_grouped_gemm_fp8_fp8_bf16_nt_masked_indexed", dict(masked_m=z(2, dtype=I64)), "masked_m must be int32 [G]"),
    ("m_grouped_gemm_fp8_fp8_bf16_nt_masked_indexed", dict(sfa_byte_offset=2), "scale rows must be float-aligned"),
    ("m_grouped_gemm_fp8_fp8_bf16_nt_masked_indexed", dict(sfa_src=z(8, 2, dtype=F64)),
     "sfa_src must be a 2-D float32 (or uint8 payload) row tensor with unit inner stride"),
    ("m_grouped_gemm_fp8_fp8_bf16_nt_masked_indexed", dict(sfa_ld=3), "sfa_ld must be sfa_src's row stride in floats"),
    ("m_grouped_gemm_fp8_fp8_bf16_nt_masked_indexed", dict(sfa_src=z(4, 2)),
     "sfa_src must hold ceil(K/128) floats at sfa_byte_offset of each of the source's rows"),
    ("m_grouped_gemm_fp8_fp8_bf16_nt_masked_indexed", dict(a_rows=z(2, 4, 256, dtype=U8), sfb=z(2, 2, 2)), "2-D row tensors"),
    ("m_grouped_gemm_fp8_fp8_bf16_nt_masked_indexed", dict(row_index=z(8, dtype=I32), sfa_byte_offset=2), "row_index int64[G*m_max]"),

    ("m_grouped_gemm_fp8_fp8_bf16_nt_contiguous", dict(a=z(8, 256)), FP8_MSG),
    ("m_grouped_gemm_fp8_fp8_bf16_nt_contiguous", dict(b=z(8, 256, dtype=U8)), "a/out rank 2, b rank 3"),
    ("m_grouped_gemm_fp8_fp8_bf16_nt_contiguous", dict(b=z(2, 8, 128, dtype=U8)), "k mismatch"),
    ("m_grouped_gemm_fp8_fp8_bf16_nt_contiguous", dict(out=z(8, 8)), "out must be [Msum,N] bfloat16"),
    ("m_grouped_gemm_fp8_fp8_bf16_nt_contiguous", dict(sfa=z(8, 3)), "sfa must be [8,2] f32"),
    ("m_grouped_gemm_fp8_fp8_bf16_nt_contiguous", dict(sfb=z(2, 1, 3)), "sfb must be [2,1,2] f32"),
    ("m_grouped_gemm_fp8_fp8_bf16_nt_contiguous", dict(m_indices=z(8, dtype=I64)), "m_indices must be int32 [Msum]"),
    ("m_grouped_gemm_fp8_fp8_bf16_nt_contiguous", dict(m_indices=z(16, dtype=I32)[::2]), "operands must be contiguous"),
    ("m_grouped_gemm_fp8_fp8_bf16_nt_contiguous", dict(b=z(8, 256, dtype=U8), out=z(8, 8)), "a/out rank 2, b rank 3"),
    ("m_grouped_gemm_fp8_fp8_bf16_nt_contiguous", dict(sfa=z(8, 3), m_indices=z(8, dtype=I64)), "sfa must be [8,2] f32"),

    ("catlass_dynamic_matmul", dict(out=z(1, 4, 8, dtype=BF16)), "rank must be 2"),
    ("catlass_dynamic_matmul", dict(mat2=z(8, 32, dtype=BF16).t()), "self dimk is not equal with mat2 dimk"),
    ("catlass_dynamic_matmul", dict(out=z(4, 8, dtype=F16)), "self, mat2 and out must share one 16-bit dtype"),
    ("catlass_dynamic_matmul", dict(out=z(4, 9, dtype=BF16)), "self / out must be contiguous"),
    ("catlass_dynamic_matmul", dict(mat2=z(16, 8, dtype=BF16)), "mat2 must be the transposed view of a contiguous [N,K] tensor (NT)"),
    ("catlass_dynamic_matmul", dict(mat2=z(8, 32, dtype=BF16).t(), out=z(4, 8, dtype=F16)), "self dimk is not equal with mat2 dimk"),
    ("catlass_dynamic_matmul", dict(out=z(4, 9, dtype=F16), mat2=z(16, 8, dtype=BF16)), "self, mat2 and out must share one 16-bit dtype"),
] + [row for name in ("per_token_cast_to_fp8", "per_block_cast_to_fp8") for row in [
    (name, dict(x=z(1, 3, 130)), "x must be a contiguous [rows, k] tensor"), (name, dict(x=z(3, 260)[:, :130]), "x must be a contiguous [rows, k] tensor"),
    (name, dict(x=z(3, 130, dtype=F64)), "x must be float32, bfloat16 or float16"),
    (name, dict(x=z(1, 3, 130, dtype=F64)), "x must be a contiguous [rows, k] tensor"),
    (name, dict(x=z(3, 260, dtype=I32)[:, :130]), "x must be a contiguous [rows, k] tensor"),
]] + [
    ("silu_and_mul_per_token_cast_to_fp8", dict(out=(z(3, 128, dtype=U8),)), "out must be (q, sf)"),
    ("silu_and_mul_per_token_cast_to_fp8", dict(out=(z(3, 128), z(3, 1))), FP8_MSG),
    ("silu_and_mul_per_token_cast_to_fp8", dict(out=(z(3, 256, dtype=U8)[:, :128], z(3, 1))), "out q must be contiguous [3, 128]"),
    ("silu_and_mul_per_token_cast_to_fp8", dict(out=(z(3, 128, dtype=U8), z(3, 2))), "out sf must be contiguous float32 [3, 1]"),
    ("silu_and_mul_per_token_cast_to_fp8", dict(masked_m=z(3, dtype=I32), out=(z(3, 128, dtype=U8),)), "x must be a contiguous [G, Mmax, 2H] tensor with masked_m"),
    ("silu_and_mul_per_token_cast_to_fp8", dict(out=(z(4, 128, dtype=U8), z(3, 2))), "out q must be contiguous [3, 128]"),

    ("route_tokens", dict(expert_ids=z(5, dtype=I32)), "expert_ids int64 [T]"),
    ("route_tokens", dict(expert_ids=z(5, 1, dtype=I64)), "expert_ids int64 [T]"),

    ("route_slots", dict(inverse=z(4, dtype=I64)), "inverse int64[buckets * cap]"),
    ("route_slots", dict(counts=z(2, dtype=I64)), "counts int32[buckets]"),
    ("route_slots", dict(dest=z(3, dtype=I64)), "dest int64[rows]"),
    ("route_slots", dict(overflow=z(1, dtype=I64)), "overflow int32[1]"),
    ("route_slots", dict(inverse=z(8, dtype=I32), counts=z(1, dtype=I32)), "inverse int64[buckets * cap]"),
    ("route_slots", dict(counts=z(1, dtype=I32), dest=z(6, dtype=I32)), "counts int32[buckets]"),

    ("copy_rows", dict(dst=z(64, dtype=U8)), "2-D row tensors"),
    ("copy_rows", dict(src=z(4, 32, dtype=U8)[:, ::2]), "2-D row tensors"),
    ("copy_rows", dict(dst_index=z(4, dtype=I32)), "index must be int64[rows]"),
    ("copy_rows", dict(src_index=z(2, dtype=I64)), "index must be int64[rows]"),
    ("copy_rows", dict(dst=z(64, dtype=U8), dst_index=z(4, dtype=I32)), "2-D row tensors"),
    ("copy_rows", dict(src=z(4, 32, dtype=U8)[:, ::2], src_index=z(4, dtype=I32)), "2-D row tensors"),

    ("copy_rows2", dict(dst1=z(32, dtype=U8)), "2-D row tensors"),
    ("copy_rows2", dict(src0=z(4, 32, dtype=U8)[:, ::2]), "2-D row tensors"),

    ("router_topk", dict(logits=z(1, 5, 8)), "logits must be a contiguous [T, E] tensor"),
    ("router_topk", dict(logits=z(5, 16)[:, :8]), "logits must be a contiguous [T, E] tensor"),
    ("router_topk", dict(logits=z(5, 8, dtype=F64)), "logits must be float32, bfloat16 or float16"),
    ("router_topk", dict(score_func="tanh"), FUNC_MSG),
    ("router_topk", dict(k=2.0), "k, n_groups and topk_groups must be integers"),
    ("router_topk", dict(topk_groups=None), "k, n_groups and topk_groups must be integers"),
    ("router_topk", dict(bias=z(7)), "bias must be contiguous float32 [8]"),
    ("router_topk", dict(bias=z(8, dtype=BF16)), "bias must be contiguous float32 [8]"),
    ("router_topk", dict(k=0, out=None), "k must be >= 1"),
    ("router_topk", dict(out=(z(5, 2, dtype=I32), z(5, 2))), "out must hold (ids, weights, scores)"),
    ("router_topk", dict(out=(z(5, 2, dtype=I32), z(5, 2), None)), "out must hold (ids, weights, scores)"),
    ("router_topk", dict(out=(z(5, 2, dtype=I64), z(5, 2), z(5, 8))), "out ids must be contiguous int32 [5, 2]"),
    ("router_topk", dict(out=(z(5, 2, dtype=I32), z(5, 3), z(5, 8))), "out weights must be contiguous float32 [5, 2]"),
    ("router_topk", dict(out=(z(5, 2, dtype=I32), z(5, 2), z(5, 16)[:, :8])), "out scores must be contiguous float32 [5, 8]"),
    ("router_topk", dict(logits=z(5, 8, dtype=F64), score_func="tanh"), "logits must be float32, bfloat16 or float16"),
    ("router_topk", dict(bias=z(7), out=(z(5, 2),)), "bias must be contiguous float32 [8]"),
    ("router_topk", dict(out=(z(5, 3, dtype=I32), z(5, 3), z(5, 9))), "out ids must be contiguous int32 [5, 2]"),

    ("router_topk_backward", dict(score_func="tanh"), FUNC_MSG),
    ("router_topk_backward", dict(scores=z(5, 8, dtype=BF16)), SCORES_MSG),
    ("router_topk_backward", dict(ids=z(4, 2, dtype=I32)), "ids must be a contiguous int32 [5, k] tensor"),
    ("router_topk_backward", dict(ids=z(5, 2, dtype=I64)), "ids must be a contiguous int32 [5, k] tensor"),
    ("router_topk_backward", dict(dw=z(5, 3)), "dw must be contiguous float32 [5, 2]"),
    ("router_topk_backward", dict(out=z(5, 8, dtype=F64)), "out must be contiguous [5, 8], float32, bfloat16 or float16"),
    ("router_topk_backward", dict(out=z(5, 9)), "out must be contiguous [5, 8], float32, bfloat16 or float16"),
    ("router_topk_backward", dict(score_func="tanh", scores=z(5, 8, dtype=BF16)), FUNC_MSG),
    ("router_topk_backward", dict(ids=z(4, 2, dtype=I32), dw=z(5, 3)), "ids must be a contiguous int32 [5, k] tensor"),

    ("router_balance_loss", dict(ids=z(6, 2, dtype=I64)), "ids must be a contiguous int32 [T, k] tensor"),
    ("router_balance_loss", dict(scores=z(6, 8, dtype=BF16)), SCORES_MSG),
    ("router_balance_loss", dict(seq_len=0), "k and seq_len must be integers >= 1"),
    ("router_balance_loss", dict(seq_len=3.0), "k and seq_len must be integers >= 1"),
    ("router_balance_loss", dict(ids=z(6, 0, dtype=I32)), "k and seq_len must be integers >= 1"),
    ("router_balance_loss", dict(seq_len=4), "seq_len must divide the 6 tokens"),
    ("router_balance_loss", dict(ids=z(3, 2, dtype=I32)), "ids must hold 6 rows"),
    ("router_balance_loss", dict(out=(z(2), z(2, 8, dtype=I32))), "out must hold (loss, counts, psum)"),
    ("router_balance_loss", dict(out=(z(3), z(2, 8, dtype=I32), z(2, 8))), "out loss must be contiguous float32 [2]"),
    ("router_balance_loss", dict(out=(z(2), z(2, 8), z(2, 8))), "out counts must be contiguous int32 [2, 8]"),
    ("router_balance_loss", dict(out=(z(2), z(2, 8, dtype=I32), z(2, 9))), "out psum must be contiguous float32 [2, 8]"),
    ("router_balance_loss", dict(ids=z(3, 2, dtype=I64), seq_len=4), "ids must be a contiguous int32 [T, k] tensor"),
    ("router_balance_loss", dict(seq_len=4, ids=z(3, 2, dtype=I32)), "seq_len must divide the 6 tokens"),

    ("router_balance_loss_backward", dict(score_func="tanh"), FUNC_MSG),
    ("router_balance_loss_backward", dict(scores=z(6, 16)[:, :8]), SCORES_MSG),
    ("router_balance_loss_backward", dict(k=0), "k and seq_len must be integers >= 1"),
    ("router_balance_loss_backward", dict(seq_len=5), "seq_len must divide the 6 tokens"),
    ("router_balance_loss_backward", dict(dloss=z(3)), "dloss must be contiguous float32 [2]"),
    ("router_balance_loss_backward", dict(counts=z(2, 8)), "counts must be contiguous int32 [2, 8]"),
    ("router_balance_loss_backward", dict(add_to=z(6, 8, dtype=BF16)), "add_to must be contiguous float32 [6, 8]"),
    ("router_balance_loss_backward", dict(out=z(6, 8, dtype=F64)), "out must be contiguous [6, 8], float32, bfloat16 or float16"),
    ("router_balance_loss_backward", dict(score_func="tanh", k=0), FUNC_MSG),
    ("router_balance_loss_backward", dict(dloss=z(3), add_to=z(6, 9)), "dloss must be contiguous float32 [2]"),

    ("router_bias_update", dict(bias=z(8, dtype=F64)), "bias must be a contiguous float32 [E] tensor"),
    ("router_bias_update", dict(bias=z(2, 4)), "bias must be a contiguous float32 [E] tensor"),
    ("router_bias_update", dict(counts=z(2, 7, dtype=I32)), "counts must be a contiguous int32 [B, 8] tensor"),
    ("router_bias_update", dict(counts=z(2, 8)), "counts must be a contiguous int32 [B, 8] tensor"),
    ("router_bias_update", dict(bias=z(2, 4), counts=z(2, 8)), "bias must be a contiguous float32 [E] tensor"),
    ("router_bias_update", dict(bias=z(7), counts=z(2, 8, dtype=I32)), "counts must be a contiguous int32 [B, 7] tensor"),
] + SMLA_CASES


def whole(msg: str) -> str:
    return "^" + re.escape(f"host assert: status -2 ({_lib.status_string(-2)}) {msg}") + "$"


@pytest.mark.parametrize("name,fault,msg", CASES, ids=[f"{i}-{c[0]}-{'+'.join(c[1])}" for i, c in enumerate(CASES)])
def test_one_fault_gets_its_own_message(name, fault, msg):
    kw = {**VALID[name](), **fault}
    if isinstance(kw.get("c"), str):      # a c that starts inside out without being it
        shape, n = kw["out"].shape, kw["out"].numel()
        both = z(2 * n)
        kw["out"], kw["c"] = both[:n].view(shape), both[4:4 + n].view(shape)
    with pytest.raises(dga.DGAError, match=whole(msg)):
        call(name, kw)


@pytest.mark.parametrize("name", sorted(VALID))
def test_the_valid_arguments_reach_the_device_guard(name):
    """... so that every case above is refused by its own check.  The optional arguments once present, once absent."""
    kw, params = VALID[name](), inspect.signature(getattr(dga, name)).parameters
    optional = [k for k in kw if k in params and params[k].default is None and not isinstance(kw[k], int)]
    for drop in ((), optional):
        with pytest.raises(dga.DGAError, match=whole("tensors must be on a HIP device (there is no CPU path)")):
            call(name, {k: v for k, v in kw.items() if k not in drop})
    if "c" in params:
        with pytest.raises(dga.DGAError, match=whole("tensors must be on a HIP device (there is no CPU path)")):
            call(name, {**kw, "c": kw["out"]})   # c = out: in-place accumulation


def test_with_policy_refuses_what_it_cannot_tag():
    t = dga.Tiling()
    names = sorted(api.ARITHMETIC_POLICIES)
    with pytest.raises(dga.DGAError, match=whole(f"policy must be one of {names}")):
        api._with_policy(t, False, "exact")
    with pytest.raises(dga.DGAError, match=whole("strict=True contradicts policy='fast'")):
        api._with_policy(t, True, "fast")
    with pytest.raises(dga.DGAError, match=whole(f"policy must be one of {names}")):
        api._with_policy(t, True, "exact")                       # both faults: the name is checked first
    t.dispatchPolicyTag = api.POLICY_BF16_EXACT
    with pytest.raises(dga.DGAError, match=whole("policy='fast_ue8m0' needs a fast-path tiling")):
        api._with_policy(t, False, "fast_ue8m0")
    assert api._with_policy(t, False, None) is t and api._with_policy(t, True, "strict").dispatchPolicyTag == api.POLICY_STRICT


class Unprintable:
    """A name that cannot be formatted: whoever builds a message with it raises."""
    def __str__(self):
        raise AssertionError("a passing check formatted its message")
    __repr__ = __str__

    def __format__(self, spec):
        raise AssertionError("a passing check formatted its message")


def test_passing_checks_format_nothing():
    name = Unprintable()
    t, codes = z(2, 3), z(2, 3, dtype=U8)
    api._want(t, name, F32, (2, 3))
    api._want(t, name, None, (2, 3))
    api._want(t, name, api._CAST_DT, (2, 3))
    api._require(True, name)
    api._require(True, "%s", name)
    got = api._outputs((codes, t), ((name, U8, (2, 3)), (name, F32, (2, 3))), t.device, name)
    assert got[0] is codes and got[1] is t
    got = api._outputs((codes.view(torch.float8_e4m3fn), t), ((name, U8, (2, 3)), (name, F32, (2, 3))), t.device, name)
    assert got[0].dtype == torch.float8_e4m3fn
    fresh = api._outputs(None, ((name, U8, (2, 3)), (name, I32, (4,))), t.device, name)
    assert [(f.dtype, tuple(f.shape)) for f in fresh] == [(U8, (2, 3)), (I32, (4,))]
    with pytest.raises(AssertionError, match="formatted"):      # ... and a failing one does
        api._want(t, name, F32, (2, 4))


def test_failing_checks_word_their_message_one_way():
    t = z(2, 6)[:, :3]
    with pytest.raises(dga.DGAError, match=whole("x must be contiguous float32 [2, 3]")):
        api._want(t, "x", F32, (2, 3))
    with pytest.raises(dga.DGAError, match=whole("x must be contiguous [2, 4]")):
        api._want(z(2, 3), "x", None, (2, 4))
    with pytest.raises(dga.DGAError, match=whole("out x must be contiguous int32 [2, 3]")):
        api._outputs((z(2, 3),), (("x", I32, (2, 3)),), t.device, "out must hold (x)")
    with pytest.raises(dga.DGAError, match=whole("out must hold (x)")):
        api._outputs((z(2, 3), z(2, 3)), (("x", I32, (2, 3)),), t.device, "out must hold (x)")
    with pytest.raises(dga.DGAError, match=whole("out must hold (x)")):
        api._outputs((None,), (("x", I32, (2, 3)),), t.device, "out must hold (x)")
