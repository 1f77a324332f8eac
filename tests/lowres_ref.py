"""The reduced-size decode (lowres 1, 2, 3: pictures of 1/2, 1/4, 1/8 the size), restated in numpy: a helper of the tests.

Per block, the reference's `-lowres` arithmetic: decode_block's dequantisation (mjpegdec.c:388-430,805: (int16)(level * q),
1024 on the DC), j_rev_dct4 / j_rev_dct2 / j_rev_dct1 (jrevdct.c:952-1156) over the top-left 4x4 / 2x2 / 1x1 coefficients
with every store into the block wrapped to int16 as DCTELEM is, and the 0..255 clamp of put_pixels_clamped4_c / 2_c /
ff_jref_idct1_put (dsputil.c:461-493, 3774-3801).  tests/golden/ref_lowres.json pins this part to the reference itself.

Per frame, the library's placement rule (include/amvhip.h): with `start` the full-size start row of the component
(mjpegdec.c:675), start_L = ((start + 1 + (1 << L) - 1) >> L) - 1 and reduced canvas row r lands at plane row
start_L - r; or, for the stills of the fixture, the reference's ordinary top-down MJPEG placement (mjpegdec.c:709-711).

Coefficients come as the entropy stage hands them out ([blocks, 64] int16 lines in scan order, six to an MCU, the DC
summed: `entropy_blocks` of the oracle); the quantiser tables are a parameter (`q60_tables(orc)` for AMV, `header_tables`
for a still)."""
import numpy as np

# scan position of each natural (row-major) position: the standard zig-zag (dsputil.c:50-59)
SCAN_OF_NATURAL = np.array([0, 1, 5, 6, 14, 15, 27, 28, 2, 4, 7, 13, 16, 26, 29, 42, 3, 8, 12, 17, 25, 30, 41, 43, 9, 11, 18, 24,
                            31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50,
                            56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63])
FIX_0_541196100, FIX_0_765366865, FIX_1_306562965, FIX_1_847759065 = 4433, 6270, 10703, 15137     # jrevdct.c:183-206
CONST_BITS, PASS1_BITS = 13, 2


def wrap16(x):
    return ((np.asarray(x, np.int64) + 32768) & 0xffff) - 32768


def dim(full, L):
    return (full + (1 << L) - 1) >> L


def sizes_420(wl, hl):
    """[(width, height)] of Y, Cb, Cr of a wl x hl picture"""
    return [(wl, hl), ((wl + 1) // 2, (hl + 1) // 2), ((wl + 1) // 2, (hl + 1) // 2)]


def plane_sizes(w, h, L):
    """... of the reduced picture of a w x h one"""
    return sizes_420(dim(w, L), dim(h, L))


def frame_bytes(w, h, L):
    return sum(a * b for a, b in plane_sizes(w, h, L))


def q60_tables(orc):
    """(luma, chroma) of sp5x's Q60, scan order, from the oracle"""
    out = []
    for chroma in (0, 1):
        t = np.zeros(64, np.uint8)
        orc.lib().amvo_q60_table(chroma, t.ctypes.data)
        out.append(t.astype(np.int64))
    return tuple(out)


def header_tables(jpeg):
    """the (luma, chroma) DQT tables a JPEG header carries (8-bit, scan order as they lie in the segment)"""
    jpeg = bytes(jpeg)
    tabs, at = {}, 2
    while at + 4 <= len(jpeg) and jpeg[at] == 0xFF and jpeg[at + 1] != 0xDA:
        size = (jpeg[at + 2] << 8) | jpeg[at + 3]
        if jpeg[at + 1] == 0xDB:
            seg = jpeg[at + 4: at + 2 + size]
            while len(seg) >= 65:
                assert seg[0] >> 4 == 0, "8-bit tables"
                tabs[seg[0] & 15] = np.frombuffer(seg[1:65], np.uint8).astype(np.int64)
                seg = seg[65:]
        at += 2 + size
    return tabs[0], tabs[1]


def dequantise(coef, tables):
    """[blocks, 64] lines -> [blocks, 8, 8] natural order, wrapped to int16: decode_block (1024 on the DC)"""
    coef = np.asarray(coef, np.int64)
    steps = np.stack([tables[1 if k >= 4 else 0] for k in range(6)])[np.arange(coef.shape[0]) % 6]
    prod = coef * steps
    prod[:, 0] += 1024
    return wrap16(prod[:, SCAN_OF_NATURAL]).reshape(-1, 8, 8)


def _even4(d0, d2, d4, d6, folded=False):
    """the even part of j_rev_dct4 (rows :1003-1048, columns :1081-1126): its four branches, selected as the reference does.
    folded: the general branch for every shape -- NOT the reference (tests use it to show that a case tells the two apart)"""
    z1 = (d2 + d6) * FIX_0_541196100
    both = (z1 - d6 * FIX_1_847759065, z1 + d2 * FIX_0_765366865)               # d2 != 0, d6 != 0
    if folded:
        tmp0, tmp1 = (d0 + d4) << CONST_BITS, (d0 - d4) << CONST_BITS
        return tmp0 + both[1], tmp1 + both[0], tmp1 - both[0], tmp0 - both[1]
    only6 = (-d6 * FIX_1_306562965, d6 * FIX_0_541196100)                        # d2 == 0, d6 != 0
    only2 = (d2 * FIX_0_541196100, d2 * FIX_1_306562965)                         # d2 != 0, d6 == 0
    zero = np.zeros_like(d0)                                                     # d2 == 0, d6 == 0
    tmp2 = np.where(d6 != 0, np.where(d2 != 0, both[0], only6[0]), np.where(d2 != 0, only2[0], zero))
    tmp3 = np.where(d6 != 0, np.where(d2 != 0, both[1], only6[1]), np.where(d2 != 0, only2[1], zero))
    tmp0, tmp1 = (d0 + d4) << CONST_BITS, (d0 - d4) << CONST_BITS
    return tmp0 + tmp3, tmp1 + tmp2, tmp1 - tmp2, tmp0 - tmp3                     # tmp10, tmp11, tmp12, tmp13


def rev_dct4(block, folded=False):
    """j_rev_dct4 on [n, 8, 8] int16-valued blocks -> the [n, 4, 4] it leaves in the top-left corner (int16 values)"""
    d = np.array(block, np.int64)[:, :4, :4]
    d[:, 0, 0] = wrap16(d[:, 0, 0] + 4)                                          # :965
    d0, d2, d4, d6 = (d[:, :, k] for k in range(4))                              # pass 1: rows
    dc_only = (d2 | d4 | d6) == 0
    flat = wrap16(d0 << PASS1_BITS)                                              # :986-999
    half = 1 << (CONST_BITS - PASS1_BITS - 1)
    rows = np.stack([np.where(dc_only, flat, wrap16((t + half) >> (CONST_BITS - PASS1_BITS))) for t in _even4(d0, d2, d4, d6, folded)], -1)
    c0, c2, c4, c6 = (rows[:, k, :] for k in range(4))                           # pass 2: columns, no shortcut
    return np.stack([wrap16(t >> (CONST_BITS + PASS1_BITS + 3)) for t in _even4(c0, c2, c4, c6, folded)], 1)


def rev_dct2(block):
    """j_rev_dct2 (:1139-1152) -> [n, 2, 2]"""
    d = np.array(block, np.int64)[:, :2, :2]
    d[:, 0, 0] = wrap16(d[:, 0, 0] + 4)
    d00, d01, d10, d11 = d[:, 0, 0] + d[:, 0, 1], d[:, 0, 0] - d[:, 0, 1], d[:, 1, 0] + d[:, 1, 1], d[:, 1, 0] - d[:, 1, 1]
    out = np.stack([(d00 + d10) >> 3, (d01 + d11) >> 3, (d00 - d10) >> 3, (d01 - d11) >> 3], -1)
    return wrap16(out).reshape(-1, 2, 2)


def rev_dct1(block):
    """ff_jref_idct1_put's (block[0] + 4) >> 3 (dsputil.c:3800): int arithmetic, nothing wraps -> [n, 1, 1]"""
    return ((np.array(block, np.int64)[:, :1, :1] + 4) >> 3)


def block_pixels(coef, L, tables):
    """[blocks, 64] lines -> [blocks, bs, bs] uint8: dequantise, reduced IDCT, ff_cropTbl's clamp"""
    nat = dequantise(coef, tables)
    out = {1: rev_dct4, 2: rev_dct2, 3: rev_dct1}[L](nat)
    return np.clip(out, 0, 255).astype(np.uint8)


def canvas(px, mcw, mch, nmcu_ok):
    """[mcus * 6, bs, bs] block pixels -> the three reduced canvases (Y [mch * 2bs, mcw * 2bs], Cb, Cr [mch * bs, mcw * bs]),
    MCUs at or after nmcu_ok zero"""
    bs = px.shape[-1]
    px = px.reshape(mch, mcw, 6, bs, bs) * (np.arange(mcw * mch) < nmcu_ok).reshape(mch, mcw, 1, 1, 1).astype(np.uint8)
    y = np.empty((mch, 2, bs, mcw, 2, bs), np.uint8)
    for k in range(4):
        y[:, k >> 1, :, :, k & 1, :] = px[:, :, k].transpose(0, 2, 1, 3)
    chroma = [px[:, :, k].transpose(0, 2, 1, 3).reshape(mch * bs, mcw * bs) for k in (4, 5)]
    return [y.reshape(mch * 2 * bs, mcw * 2 * bs)] + chroma


def start_row(h, L, chroma):
    """start_L of the component"""
    mch = (h + 15) // 16
    start = (1 if chroma else 2) * (8 * mch - ((h // 2) & 7)) - 1                # mjpegdec.c:675
    return ((start + 1 + (1 << L) - 1) >> L) - 1


def picture(coef, w, h, L, nmcu_ok, tables, flip=True):
    """one frame -> uint8 [frame_bytes(w, h, L)]: Y, Cb, Cr tight.  flip: the library's rule for AMV; False: the reference's
    top-down placement of an ordinary MJPEG picture"""
    mcw, mch = (w + 15) // 16, (h + 15) // 16
    planes = canvas(block_pixels(coef, L, tables), mcw, mch, nmcu_ok)
    out = []
    for c, (s, (pw, ph)) in enumerate(zip(planes, plane_sizes(w, h, L))):
        plane = np.zeros((ph, pw), np.uint8)
        if flip:
            src = start_row(h, L, c > 0) - np.arange(ph)                          # the canvas row each plane row shows
            inside = (src >= 0) & (src < s.shape[0])
            plane[inside] = s[src[inside], :pw]
        else:
            plane[:] = s[:ph, :pw]
        out.append(plane.reshape(-1))
    return np.concatenate(out)


def split(frame, sizes):
    """a frame's bytes -> its three planes (sizes: plane_sizes or sizes_420)"""
    out, at = [], 0
    for pw, ph in sizes:
        out.append(np.asarray(frame)[at: at + pw * ph].reshape(ph, pw))
        at += pw * ph
    return out


def fnv1a64(data):
    h = 0xCBF29CE484222325
    for b in bytes(data):
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h
