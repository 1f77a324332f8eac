"""Models of two rewrites in amv_reconstruct.hip, checked on the CPU in NumPy.

(a) idct8's row pass takes the + 128 of its two 181-products in on the addends of the odd products' multiply-adds
    (+ s on W1 x4 + W7 x5, - s on W5 x6 + W3 x7, s = 64 / 181 modulo 2^31).  The eight outputs of a row must be the same
    32-bit words with and without the seeds, for the plain rows (>> 8) and for rows 0 and 4, which leave masked.
(b) Stage D forms the twelve bytes of a patch row as six byte pairs in output order -- (B0 G0)(R0 B1)(G1 R1)(B2 G2)
    (R2 B3)(G3 R3), one packed add and one saturating pack each, the second pack of a dword into its high half -- where
    it formed pixel pairs of one channel and interleaved them with byte permutes.  Both are modelled on 16-bit lanes.
(c) The frames of tests/test_gpu_stage_d_pairs.py put every byte of a patch row, in both rows, on 0 from below, on 255
    from above and in between: checked here on the oracle's output, so that it fails without a GPU.
"""
import numpy as np
import pytest

import coef_builder as cb
import stage_d_frames as sd

W1, W2, W3, W5, W6, W7 = 2841, 2676, 2408, 1609, 1108, 565
M32 = (1 << 32) - 1
SEED = 64 * pow(181, -1, 1 << 31) % (1 << 31)


def _i32(x):
    """int64 array -> the same numbers wrapped to int32, still as int64"""
    return ((x + (1 << 31)) & M32) - (1 << 31)


def _row(v, kind, seeded):
    """idct8<false, kind> of amv_reconstruct.hip on int64 arrays of 24-bit inputs [..., 8] -> uint32 [..., 8]"""
    v = [v[..., i].astype(np.int64) for i in range(8)]
    bias = 128 + 8192 if kind == "row0" else 128
    s = SEED if seeded else 0
    half = 0 if seeded else 128
    a0 = _i32(v[0] * 2048 + bias)
    a1 = _i32(v[4] * 2048)
    i2, i3, i4, i5, i6, i7 = v[6], v[2], v[1], v[7], v[5], v[3]
    a4 = _i32(i4 * W1 + _i32(i5 * W7 + s))
    a5 = _i32(i4 * W7 + _i32(i5 * -W1))
    a6 = _i32(i6 * W5 + _i32(i7 * W3 - s))
    a7 = _i32(i6 * W3 + _i32(i7 * -W5))
    t = _i32(a0 + a1)
    a0 = _i32(a0 - a1)
    a2 = _i32(i3 * W6 + _i32(i2 * -W2))
    a3 = _i32(i3 * W2 + _i32(i2 * W6))
    a1 = _i32(a4 + a6)
    a4 = _i32(a4 - a6)
    a6 = _i32(a5 + a7)
    a5 = _i32(a5 - a7)
    a7 = _i32(t + a3)
    t = _i32(t - a3)
    a3 = _i32(a0 + a2)
    a0 = _i32(a0 - a2)
    a2 = _i32(181 * _i32(a4 + a5) + half) >> 8
    a4 = _i32(181 * _i32(a4 - a5) + half) >> 8
    out = np.stack([a7 + a1, a3 + a2, a0 + a4, t + a6, t - a6, a0 - a4, a3 - a2, a7 - a1], -1)
    out = _i32(out)
    out = out >> 8 if kind == "plain" else out & ~255
    return (out & M32).astype(np.uint32)


def _row_inputs():
    top = (1 << 23) - 1
    big_step = int(max(cb.QUANT[0].max(), cb.QUANT[1].max()))
    edges = [0, 1, -1, top, -top, -top - 1, cb.AC_BOUND, -cb.AC_BOUND, cb.AC_BOUND - 1, 1 - cb.AC_BOUND,
             32767 * big_step, -32768 * big_step, 32767 * 9, -32768 * 9, 32767 * 8, -32768 * 8, 1023 * big_step, -1023 * big_step]
    edges = [e for e in edges if -top - 1 <= e <= top]
    rng = np.random.default_rng(0x181)
    rows = [rng.integers(-top - 1, top + 1, (200000, 8))]                       # the whole 24-bit range
    rows.append(rng.choice(edges, (50000, 8)))                                  # every slot on an edge
    one = np.zeros((len(edges) * 8, 8), np.int64)                               # one slot on an edge, the others zero
    for i, e in enumerate(edges):
        one[8 * i + np.arange(8), np.arange(8)] = e
    rows.append(one)
    rows.append(rng.integers(-cb.AC_BOUND, cb.AC_BOUND + 1, (50000, 8)))        # what the stage accessor promises
    return np.concatenate(rows)


def test_seed_is_what_the_kernel_uses():
    assert 181 * 2 * SEED % (1 << 32) == 128 and 0 <= SEED < 1 << 31


@pytest.mark.parametrize("kind", ["plain", "row0", "row4"])
def test_seeded_row_pass_equals_plain(kind):
    v = _row_inputs()
    assert (np.abs(v) == (1 << 23) - 1).any() and (v == -(1 << 23)).any() and (np.abs(v) == cb.AC_BOUND).any()
    plain, seeded = _row(v, kind, False), _row(v, kind, True)
    bad = np.argwhere(plain != seeded)
    assert bad.size == 0, "row %s: input %s: plain %#x, seeded %#x" % (
        kind, v[bad[0][0]], plain[tuple(bad[0])], seeded[tuple(bad[0])])


# ---------------------------------------------------------------------------------------------- (b) the packing

def _perm(a, b, sel):
    """v_perm_b32 as __builtin_amdgcn_perm(a, b, sel) for selectors 0..7: bytes 0-3 are b's, 4-7 a's"""
    pool = [(b >> (8 * i)) & 255 for i in range(4)] + [(a >> (8 * i)) & 255 for i in range(4)]
    out = np.zeros_like(a)
    for i in range(4):
        out |= pool[(sel >> (8 * i)) & 7] << (8 * i)
    return out


def _halves(x):
    lo = (x & 0xffff).astype(np.int64)
    hi = ((x >> 16) & 0xffff).astype(np.int64)
    return lo, hi


def _pk_add(x, xsel, c):
    """v_pk_add_i16 with the first operand's halves chosen by xsel = (low result's, high result's): 16-bit wrap"""
    xh, ch = _halves(x), _halves(c)
    lo = (xh[xsel[0]] + ch[0]) & 0xffff
    hi = (xh[xsel[1]] + ch[1]) & 0xffff
    return (lo | (hi << 16)).astype(np.uint32)


def _sat_u8(h):
    s = np.where(h >= 0x8000, h - 0x10000, h)
    return np.clip(s, 0, 255)


def _sat_pk(x):
    """v_sat_pk_u8_i16: both halves clamped to 0..255, in bytes 0 and 1; the rest of the dword zero"""
    lo, hi = _halves(x)
    return (_sat_u8(lo) | (_sat_u8(hi) << 8)).astype(np.uint32)


def _sat_pk_high(d, x):
    """... its SDWA form writing the high half of d and keeping the low half"""
    return ((d & 0xffff) | (_sat_pk(x) << 16)).astype(np.uint32)


def _pixel_pairs(yy, dots):
    """the row as it was formed: terms doubled into both halves, pixel pairs of one channel, three interleaving permutes"""
    c = {}
    for e in range(2):
        for name in "bgr":
            d = dots[name][e]
            c[name, e] = _perm(d, d, 0x02010201)
    pair = lambda y, t: _sat_pk(_pk_add(y, (0, 1), t))
    b01, g01, r01 = pair(yy[0], c["b", 0]), pair(yy[0], c["g", 0]), pair(yy[0], c["r", 0])
    b23, g23, r23 = pair(yy[1], c["b", 1]), pair(yy[1], c["g", 1]), pair(yy[1], c["r", 1])
    gr = g01 | (r01 << 16)
    bg = b23 | (g23 << 16)
    return [_perm(gr, b01, 0x01060400), _perm(bg, gr, 0x06040301), _perm(bg, r23, 0x01070500)]


def _channel_pairs(yy, dots):
    """the row as it is formed now: (b, g), (r, b), (g, r) of a chroma sample, six brackets in output order"""
    bg, rb, gr = [], [], []
    for e in range(2):
        b, g, r = dots["b"][e], dots["g"][e], dots["r"][e]
        bg.append(_perm(g, b, 0x06050201))
        rb.append(_perm(b, r, 0x06050201))
        gr.append(_perm(r, g, 0x06050201))
    quad = lambda lo, hi: _sat_pk_high(_sat_pk(lo), hi)
    return [quad(_pk_add(yy[0], (0, 0), bg[0]), _pk_add(yy[0], (0, 1), rb[0])),
            quad(_pk_add(yy[0], (1, 1), gr[0]), _pk_add(yy[1], (0, 0), bg[1])),
            quad(_pk_add(yy[1], (0, 1), rb[1]), _pk_add(yy[1], (1, 1), gr[1]))]


def test_channel_pairs_equal_pixel_pairs():
    Y, C = np.meshgrid(np.arange(-300, 301), np.arange(-450, 451), indexing="ij")
    Y, C = Y.reshape(-1), C.reshape(-1)
    # every luma slot and every term slot runs over its whole range against every value of the other (a turn of the
    # range is a bijection), and no two slots hold the same value at once
    y = [((Y + 300 + 150 * i) % 601 - 300) for i in range(4)]
    terms = [((C + 450 + 130 * j) % 901 - 450) for j in range(6)]
    junk = np.arange(Y.size) * 37 % 256                                       # the dot product's low byte: not part of the term
    pack = lambda lo, hi: ((lo & 0xffff) | ((hi & 0xffff) << 16)).astype(np.uint32)
    yy = [pack(y[0], y[1]), pack(y[2], y[3])]
    dot = lambda t: (((t << 8) | junk) & M32).astype(np.uint32)
    dots = {"b": [dot(terms[0]), dot(terms[3])], "g": [dot(terms[1]), dot(terms[4])], "r": [dot(terms[2]), dot(terms[5])]}
    old, new = _pixel_pairs(yy, dots), _channel_pairs(yy, dots)
    # and both are the row: B G R of pixel i is clamp(y[i] + term of sample i / 2)
    want = np.stack([np.clip(y[i] + terms[3 * (i // 2) + ch], 0, 255) for i in range(4) for ch in range(3)], -1)
    for k in range(3):
        assert (old[k] == new[k]).all(), "dword %d" % k
        for byte in range(4):
            assert (((new[k] >> (8 * byte)) & 255) == want[:, 4 * k + byte]).all(), (k, byte)
    assert (want == 0).any(0).all() and (want == 255).any(0).all()


# ---------------------------------------------------------------------------------------------- (c) the frames

@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("w,h", sd.SIZES)
def test_frames_cover_every_byte_place(orc, w, h, flags):
    coefs = sd.frames(w, h)
    assert len(coefs) <= 3
    sd.assert_covered(orc, coefs, [sd.mcus(w, h)] * len(coefs), w, h, flags)
