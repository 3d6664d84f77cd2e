"""The paged fp8 latent cache of sparse_mla_fwd_fp8 in numpy: its rows packed and unpacked under both accepted shapes, the value a row
stands for, and what mla_kv_cast_to_fp8_paged writes.

    row r        656 bytes at (r // page_size) block_stride + (r % page_size) 656 of the buffer:
                 bytes 0 .. 511 the e4m3fn codes, 512 .. 527 four float32 scales (one per 128 codes), 528 .. 655 64 bf16 rope values
    deq[r, d]    RNE_bf16(fl32(e4m3(code[r, d]) scale[r, d // 128])) for d < 512 -- the code's value from a 256-entry table, one float32
                 multiplication and one rounding to bf16, subnormals kept in both -- and the rope value as stored for d >= 512

The flat shape [S, 656] with rows `stride` bytes apart is page_size = 1 with block_stride = stride.  sparse_mla_fwd_fp8(q, cache, ...) is
sparse_mla_fwd(q, deq(cache), ...) byte for byte, which is all its GPU tests hold it to (tests/sparse_mla_ref.py has the reference and the
bounds of that function)."""
import numpy as np

ROW, LATENT, GROUPS, ROPE = 656, 512, 4, 64
SCALES_AT, ROPE_AT = 512, 528
D_QK = LATENT + ROPE
NAN_CODES = (0x7F, 0xFF)


def _e4m3_table():
    t = np.zeros(256, np.float64)
    for c in range(256):
        e, m = (c >> 3) & 15, c & 7
        v = m / 8 * 2.0 ** -6 if e == 0 else (1 + m / 8) * 2.0 ** (e - 7)
        t[c] = np.nan if (c & 0x7F) == 0x7F else (-v if c & 0x80 else v)
    return t.astype(np.float32)


E4M3 = _e4m3_table()                                                   # every value is exact in float32
E4M3.setflags(write=False)


def bf16_bits(x):
    """float32 -> the 16 bits of its round-to-nearest-even bf16, subnormals kept, overflow to inf; NaN as 0x7FC0 | sign"""
    f = np.ascontiguousarray(x, dtype=np.float32)
    b = f.view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(f), ((b >> 16) & 0x8000 | 0x7FC0).astype(np.uint16), r)


def bits_to_f32(bits):
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def deq_bits(codes, scales, rope_bits):
    """codes uint8 [S, 512], scales float32 [S, 4], rope_bits uint16 [S, 64] -> uint16 [S, 576]: the bf16 bits of the rows' values"""
    codes, scales = np.asarray(codes, np.uint8), np.asarray(scales, np.float32)
    with np.errstate(all="ignore"):
        prod = E4M3[codes] * np.repeat(scales, LATENT // GROUPS, axis=-1)      # float32 x float32 -> float32: one rounding
    return np.concatenate([bf16_bits(prod), np.asarray(rope_bits, np.uint16)], axis=-1)


def deq(codes, scales, rope_bits):
    """float32 [S, 576]: the values (each exact in bf16; NaN where the row holds one)"""
    return bits_to_f32(deq_bits(codes, scales, rope_bits))


def geometry(s, page_size, block_stride=None):
    """(num_blocks, block_stride) of a cache of at least s rows"""
    nb = -(-s // page_size)
    stride = page_size * ROW if block_stride is None else block_stride
    assert stride >= page_size * ROW and stride % 16 == 0
    return nb, stride


def row_at(r, page_size, block_stride):
    r = np.asarray(r, np.int64)
    return r // page_size * block_stride + r % page_size * ROW


def pack(codes, scales, rope_bits, page_size=1, block_stride=None, fill=0):
    """-> uint8 [num_blocks, block_stride]: rows 0 .. S - 1 in place, every other byte (rows beyond S, the padding between blocks) `fill`"""
    codes, scales, rope_bits = np.asarray(codes, np.uint8), np.asarray(scales, np.float32), np.asarray(rope_bits, np.uint16)
    s = codes.shape[0]
    assert codes.shape == (s, LATENT) and scales.shape == (s, GROUPS) and rope_bits.shape == (s, ROPE)
    nb, stride = geometry(s, page_size, block_stride)
    buf = np.full(nb * stride, fill, np.uint8)
    rows = np.concatenate([codes, np.ascontiguousarray(scales).view(np.uint8).reshape(s, 16), np.ascontiguousarray(rope_bits).view(np.uint8).reshape(s, 128)],
                          axis=1)
    at = row_at(np.arange(s), page_size, stride)
    buf[at[:, None] + np.arange(ROW)[None, :]] = rows
    return buf.reshape(nb, stride)


def unpack(buf, page_size=1, s=None):
    """the inverse: (codes [S, 512], scales [S, 4], rope_bits [S, 64]) of the first s rows (all of them by default)"""
    buf = np.asarray(buf, np.uint8)
    nb, stride = buf.shape
    s = nb * page_size if s is None else s
    at = row_at(np.arange(s), page_size, stride)
    rows = buf.reshape(-1)[at[:, None] + np.arange(ROW)[None, :]]
    return (rows[:, :LATENT].copy(), np.ascontiguousarray(rows[:, SCALES_AT:ROPE_AT]).view(np.float32).reshape(s, GROUPS),
            np.ascontiguousarray(rows[:, ROPE_AT:]).view(np.uint16).reshape(s, ROPE))


def row_bytes_mask(rows, nb, page_size, block_stride):
    """bool [nb, block_stride]: the bytes of the named rows"""
    mask = np.zeros(nb * block_stride, bool)
    rows = np.asarray(rows, np.int64).reshape(-1)
    if len(rows):
        mask[row_at(rows, page_size, block_stride)[:, None] + np.arange(ROW)[None, :]] = True
    return mask.reshape(nb, block_stride)


def written(buf, kv_c, rope_bits, slots, page_size, quant_1x128, ue8m0=False):
    """What mla_kv_cast_to_fp8_paged leaves in a copy of buf: kv_c float32 [T, 512] (the values the input tensor holds), rope_bits uint16
    [T, 64] (bf16_bits of k_pe's values; a bf16 k_pe's own bits), slots int64 [T]; quant_1x128 is the quantisers' reference
    (oracle.quant_1x128: codes [T, 512], scales [T, 4]).
    Tokens whose slot lies outside [0, num_blocks page_size) are skipped; valid slots must be distinct."""
    out = np.array(buf, np.uint8, copy=True)
    nb, stride = out.shape
    slots = np.asarray(slots, np.int64)
    keep = (slots >= 0) & (slots < nb * page_size)
    assert len(np.unique(slots[keep])) == int(keep.sum())
    if keep.any():
        codes, scales = quant_1x128(np.ascontiguousarray(np.asarray(kv_c, np.float32)[keep]), ue8m0=ue8m0)
        rope = np.asarray(rope_bits, np.uint16)[keep]
        rows = np.concatenate([np.asarray(codes, np.uint8).reshape(-1, LATENT), np.ascontiguousarray(scales, np.float32).view(np.uint8).reshape(-1, 16),
                               np.ascontiguousarray(rope).view(np.uint8).reshape(-1, 128)], axis=1)
        out.reshape(-1)[row_at(slots[keep], page_size, stride)[:, None] + np.arange(ROW)[None, :]] = rows
    return out


def quantise(kv, quant_1x128):
    """kv float32 [S, 576] (bf16 values) -> (codes, scales, rope_bits): what the writer makes of the latent and rope parts of each row"""
    kv = np.asarray(kv, np.float32)
    codes, scales = quant_1x128(np.ascontiguousarray(kv[:, :LATENT]))
    return np.asarray(codes, np.uint8).reshape(-1, LATENT), np.asarray(scales, np.float32).reshape(-1, GROUPS), bf16_bits(kv[:, LATENT:])
