"""The reconstruction's row pass on paired 16-bit halves, as a numpy model, against the plain row of idct8 (CPU).

amv_reconstruct.hip takes the row pass of a records frame without a ten-bit AC as dot products: the dequantising
multiply writes the low 16 bits of coefficient x step into one half of a pair register, (n0, n4), (n1, n7), (n5, n3),
(n2, n6) of a row, and each of the eight linear forms in front of the row's butterflies is one v_dot2_i32_i16 over a
pair -- a.lo * w.lo + a.hi * w.hi + accumulator, the low 32 bits.  The model below restates the half write and the
dot products with 32-bit wrap; the reference is idctrow (AmvJpeg.c:1082-1128) in wrapping int arithmetic, in the three
forms the kernel's rows leave it in: shifted (rows 1-3, 5-7), masked with the column pass's 8192 on top (row 0, whose
first input is the DC as a 32-bit number) and masked (row 4).

The claim: equal for every input a scan without a ten-bit AC can carry -- |coefficient| <= 511 times a step of either
table, any DC.  And the reason the entropy stage marks frames: the first ten-bit value whose product leaves an int16.
"""
import os
import re

import numpy as np

from coef_builder import QUANT

W1, W2, W3, W5, W6, W7 = 2841, 2676, 2408, 1609, 1108, 565
PAIR_COL = ((0, 4), (1, 7), (5, 3), (2, 6))
SEED = (64 * pow(181, -1, 1 << 32)) & 0x7FFFFFFF          # 181 * 2 * SEED == 128 modulo 2^32
PLAIN, ROW0, ROW4 = "plain", "row0", "row4"
STEPS = sorted({int(q) for t in QUANT for q in np.asarray(t).ravel()})
DC_STEPS = sorted({int(np.asarray(t).ravel()[0]) for t in QUANT})


def wrap32(x):
    return ((np.asarray(x, np.int64) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def wrap16(x):
    return ((np.asarray(x, np.int64) + (1 << 15)) & 0xFFFF) - (1 << 15)


def reference_row(n, kind):
    """idctrow on [rows, 8] int64 inputs (already dequantised), every step wrapped to 32 bits"""
    n = np.asarray(n, np.int64)
    x0 = wrap32(wrap32(n[:, 0] << 11) + 128)
    x1 = wrap32(n[:, 4] << 11)
    x2, x3, x4, x5, x6, x7 = n[:, 6], n[:, 2], n[:, 1], n[:, 7], n[:, 5], n[:, 3]
    x8 = wrap32(W7 * wrap32(x4 + x5))
    x4 = wrap32(x8 + wrap32((W1 - W7) * x4))
    x5 = wrap32(x8 - wrap32((W1 + W7) * x5))
    x8 = wrap32(W3 * wrap32(x6 + x7))
    x6 = wrap32(x8 - wrap32((W3 - W5) * x6))
    x7 = wrap32(x8 - wrap32((W3 + W5) * x7))
    x8 = wrap32(x0 + x1)
    x0 = wrap32(x0 - x1)
    x1 = wrap32(W6 * wrap32(x3 + x2))
    x2 = wrap32(x1 - wrap32((W2 + W6) * x2))
    x3 = wrap32(x1 + wrap32((W2 - W6) * x3))
    x1 = wrap32(x4 + x6)
    x4 = wrap32(x4 - x6)
    x6 = wrap32(x5 + x7)
    x5 = wrap32(x5 - x7)
    x7 = wrap32(x8 + x3)
    x8 = wrap32(x8 - x3)
    x3 = wrap32(x0 + x2)
    x0 = wrap32(x0 - x2)
    x2 = wrap32(wrap32(181 * wrap32(x4 + x5)) + 128) >> 8
    x4 = wrap32(wrap32(181 * wrap32(x4 - x5)) + 128) >> 8
    out = np.stack([wrap32(x7 + x1), wrap32(x3 + x2), wrap32(x0 + x4), wrap32(x8 + x6),
                    wrap32(x8 - x6), wrap32(x0 - x4), wrap32(x3 - x2), wrap32(x7 - x1)], 1) >> 8
    if kind == PLAIN:
        return out
    # what the column pass takes from rows 0 and 4: 256 * v (+ 8192 in row 0), modulo 2^32
    return wrap32(wrap32(out << 8) + (8192 if kind == ROW0 else 0))


def half_write(coef, step):
    """v_mul_i32_i24_sdwa into half a register: the low 16 bits of the product, read back signed"""
    return wrap16(np.asarray(coef, np.int64) * np.asarray(step, np.int64))


def dot2(lo, hi, wlo, whi, acc):
    return wrap32(lo * wlo + hi * whi + acc)


def model_row(coef, step, kind):
    """the kernel's row: [rows, 8] quantised coefficients and their steps -> what idct8_row_pairs leaves"""
    coef, step = np.asarray(coef, np.int64), np.asarray(step, np.int64)
    h = half_write(coef, step)
    pair = [(h[:, a], h[:, b]) for a, b in PAIR_COL]
    even = np.full(len(coef), 128, np.int64)
    if kind == ROW0:   # the DC is a 32-bit product of its own; its pair's low half is zero
        pair[0] = (np.zeros(len(coef), np.int64), pair[0][1])
        even = wrap32(wrap32(wrap32(coef[:, 0] * step[:, 0]) * 2048) + (128 + 8192))
    t = dot2(*pair[0], 2048, 2048, even)
    a0 = dot2(*pair[0], 2048, -2048, even)
    a4 = dot2(*pair[1], W1, W7, SEED)
    a5 = dot2(*pair[1], W7, -W1, 0)
    a6 = dot2(*pair[2], W5, W3, -SEED)
    a7 = dot2(*pair[2], W3, -W5, 0)
    a2 = dot2(*pair[3], W6, -W2, 0)
    a3 = dot2(*pair[3], W2, W6, 0)
    a1 = wrap32(a4 + a6)
    a4 = wrap32(a4 - a6)
    a6 = wrap32(a5 + a7)
    a5 = wrap32(a5 - a7)
    a7 = wrap32(t + a3)
    t = wrap32(t - a3)
    a3 = wrap32(a0 + a2)
    a0 = wrap32(a0 - a2)
    a2 = wrap32(181 * wrap32(a4 + a5)) >> 8      # (the 128 came in with the seeds)
    a4 = wrap32(181 * wrap32(a4 - a5)) >> 8
    out = np.stack([wrap32(a7 + a1), wrap32(a3 + a2), wrap32(a0 + a4), wrap32(t + a6),
                    wrap32(t - a6), wrap32(a0 - a4), wrap32(a3 - a2), wrap32(a7 - a1)], 1)
    return out >> 8 if kind == PLAIN else out & ~255


def _same(coef, step, kind):
    coef, step = np.asarray(coef, np.int64), np.asarray(step, np.int64)
    got, want = model_row(coef, step, kind), reference_row(coef * step, kind)
    bad = np.nonzero((got != want).any(1))[0]
    assert bad.size == 0, (kind, coef[bad[0]], step[bad[0]], got[bad[0]], want[bad[0]])


def test_the_model_is_the_kernels():
    """the pairing, the seed and the weights as amv_reconstruct.hip has them"""
    src = open(os.path.join(os.path.dirname(__file__), "..", "amv-codec-tools_amd", "csrc", "amv_reconstruct.hip")).read()
    m = re.search(r"kPairCol\[4\]\[2\] = \{\{(\d), (\d)\}, \{(\d), (\d)\}, \{(\d), (\d)\}, \{(\d), (\d)\}\}", src)
    assert m and tuple(map(int, m.groups())) == tuple(c for p in PAIR_COL for c in p)
    assert "W1 = 2841, W2 = 2676, W3 = 2408, W5 = 1609, W6 = 1108, W7 = 565" in src
    assert (181 * 2 * SEED) % (1 << 32) == 128
    assert max(STEPS) == 61 and 511 * 61 == 31171


def test_every_product_of_nine_bits_is_an_int16_and_rides_every_position():
    c, q = np.meshgrid(np.arange(-511, 512), np.array(STEPS), indexing="ij")
    c, q = c.ravel(), q.ravel()
    assert (half_write(c, q) == c * q).all()
    assert (c * q).max() == 31171 and (c * q).min() == -31171
    for kind in (PLAIN, ROW0, ROW4):
        for pos in range(1 if kind == ROW0 else 0, 8):
            coef = np.zeros((c.size, 8), np.int64)
            step = np.ones((c.size, 8), np.int64)
            coef[:, pos], step[:, pos] = c, q
            _same(coef, step, kind)


def test_all_four_pairs_at_the_extremes():
    signs = np.array([[1 if (k >> j) & 1 else -1 for j in range(8)] for k in range(256)], np.int64)
    step = np.full((256, 8), 61, np.int64)
    for kind in (PLAIN, ROW4):
        _same(511 * signs, step, kind)
    for dc in (-32768, -1, 0, 1, 32767):
        for dq in DC_STEPS:
            coef, st = 511 * signs, step.copy()
            coef[:, 0], st[:, 0] = dc, dq
            _same(coef, st, ROW0)


def test_every_dc_in_row_0():
    dc = np.arange(-32768, 32768)
    rng = np.random.default_rng(0xDC)
    for dq in DC_STEPS:
        for ac in (0, 511, -511):
            coef = np.full((dc.size, 8), ac, np.int64)
            step = np.full((dc.size, 8), 61, np.int64)
            coef[:, 0], step[:, 0] = dc, dq
            _same(coef, step, ROW0)
        coef = rng.integers(-511, 512, (dc.size, 8))
        step = rng.choice(STEPS, (dc.size, 8))
        coef[:, 0], step[:, 0] = dc, dq
        _same(coef, step, ROW0)


def test_random_rows():
    rng = np.random.default_rng(0x0D07)
    for kind in (PLAIN, ROW0, ROW4):
        coef = rng.integers(-511, 512, (100000, 8))
        step = rng.choice(STEPS, (100000, 8))
        if kind == ROW0:
            coef[:, 0] = rng.integers(-32768, 32768, 100000)
            step[:, 0] = rng.choice(DC_STEPS, 100000)
        _same(coef, step, kind)


def test_the_first_ten_bit_value_that_breaks_the_half():
    """why frames with a ten-bit AC are marked: from 538 x 61 on the product is no int16, and the row differs"""
    broken = [(c, q) for c in range(512, 1024) for q in STEPS if half_write(c, q) != c * q]
    assert broken[0] == (538, 61) and 537 * 61 == 32757 and 538 * 61 == 32818
    assert half_write(-537, 61) == -537 * 61 and half_write(-538, 61) != -538 * 61
    assert all(half_write(c, q) == c * q for c in range(512, 538) for q in STEPS)   # (512 x 61 itself still fits)
    for kind in (PLAIN, ROW4):
        coef = np.zeros((1, 8), np.int64)
        step = np.full((1, 8), 61, np.int64)
        coef[0, 1] = 538
        assert (model_row(coef, step, kind) != reference_row(coef * step, kind)).any()
        coef[0, 1] = 537
        _same(coef, step, kind)
