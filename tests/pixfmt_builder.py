"""Crafted pictures for the pixel-format kernels (amv_pixfmt.hip): inputs that sit on the rounding steps, the clamps and
the dropped bits of the reference's img_convert arithmetic.  TEST INFRASTRUCTURE, for BUILDING inputs only: the
expectation of every GPU test stays img_convert_ref.convert (itself pinned to the real reference by test_img_convert.py).
The searches below restate the numerators of img_convert_ref._rgb_in / _rgb_out to FIND inputs; test_pixfmt_builder.py
asserts that the inputs found do in img_convert_ref what they were sought for.

rgb_in (imgconvert_template.h:218-323): luma = (yr r + yg g + yb b + 512 [+ 16 << 10]) >> 10 a pixel; chroma =
((ur R + ug G + ub B + 2047) >> 12) + 128 on the sums R, G, B of a 2 x 2 patch -- the numerator is negative for half of
all colours and the shift is arithmetic.  Sought, for each of the four (source, destination) weight sets: triples whose
luma numerator is 1023 and 0 mod 1024, patches of four different pixels whose Cb and Cr numerators are 4095 and 0 mod 4096
with the numerator positive and negative: 10 thresholds a pair, RGB_IN_THRESHOLDS = 40 in all, of which
RGB_IN_THRESHOLDS_MET = 34 are met.  The six that cannot be: towards YUV420P the Cb weights (-152, -298, 450) are all even,
so the Cb numerator (+ 2047) is odd and never 0 mod 4096, for either sign, in each of the three sources.

rgb_out (imgconvert_template.h:30-216): channel = cm((y + c_b (Cb - 128) + c_r (Cr - 128) + 512) >> 10).  Sought, from both
source ranges and for each of r, g, b: a value before the clamp of -1, 0, 255 and 256, one below -100 and one above 355, a
negative numerator that is 1023 and one that is 0 mod 1024 (8 a channel), and every channel value 0..255 after the clamp
(so that RGB565 / RGB555 see both sides of every dropped-bit boundary: 7|8 ... 247|248, and 3|4 ... 251|252 for the six-bit
green); and the six colours with one channel at 255 and the others at 0, or the reverse: RGB_OUT_THRESHOLDS of each kind.
Met: every channel value; 43 of the 48 steps -- r and b depend on two samples only and were searched exhaustively: from
YUV420P their numerators are even (1192 (Y - 16), 1634 Cr', 2066 Cb', 512), from YUVJ420P r's is a multiple of 4, so none is
ever 1023 mod 1024, and from YUVJ420P no negative b numerator is 1023 or 0 mod 1024 within Cb' = -128..127; 10 of the 12
colours -- from YUVJ420P pure red and pure blue are out of reach (r = 255 wants Y >= 77 at Cr = 255, and then g <= 0 and
b <= 0 ask for Cb' >= -39 and Cb' <= -44), which a search over every Y and every third Cb, Cr bears out."""
import numpy as np

import img_convert_ref as R

RGB_IN_PAIRS = [(R.RGB24, R.YUV420P), (R.BGR24, R.YUV420P), (R.RGB32, R.YUV420P), (R.RGB24, R.YUVJ420P)]
RGB_IN_THRESHOLDS, RGB_IN_THRESHOLDS_MET = 40, 34
RGB_OUT_SOURCES = [R.YUV420P, R.YUVJ420P]
# per source range: 3 channels x 8 sought values, 3 x 256 channel values, 6 saturated colours
RGB_OUT_THRESHOLDS = {"steps": 48, "values": 1536, "colours": 12}
RGB_OUT_THRESHOLDS_MET = {"steps": 43, "values": 1536, "colours": 10}
CORNERS = [(r, g, b) for r in (0, 255) for g in (0, 255) for b in (0, 255)]

_CACHE = {}


# ---- rgb_in ----------------------------------------------------------------------------------------------------------------

def rgb_in_weights(dst):
    """(y weights, y add, u weights, v weights) on (r, g, b), as img_convert_ref._rgb_in has them"""
    F = R.FIX
    ys, cs, yadd = (1.0, 1.0, 0) if dst == R.YUVJ420P else (219.0 / 255.0, 224.0 / 255.0, 16 << R.SCALEBITS)
    return ((F(0.29900 * ys), F(0.58700 * ys), F(0.11400 * ys)), R.ONE_HALF + yadd,
            (-F(0.16874 * cs), -F(0.33126 * cs), F(0.50000 * cs)), (F(0.50000 * cs), -F(0.41869 * cs), -F(0.08131 * cs)))


def rgb_in_numerators(dst, patch):
    """patch int [..., 4, 3] (four pixels of r, g, b) -> (luma numerators [..., 4], Cb numerator, Cr numerator)"""
    wy, yadd, wu, wv = rgb_in_weights(dst)
    patch = patch.astype(np.int64)
    s = patch.sum(axis=-2)
    rnd = (R.ONE_HALF << 2) - 1
    return (patch * np.array(wy)).sum(axis=-1) + yadd, (s * np.array(wu)).sum(axis=-1) + rnd, (s * np.array(wv)).sum(axis=-1) + rnd


def rgb_in_patches(dst):
    """(patches uint8 [n, 4, 3], met): the sought patches of a weight set, the eight corner colours, patches of the corners
    mixed; met = the names of the thresholds found"""
    key = ("rgb_in", dst)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(9000 + dst)
    pool = rng.integers(0, 256, (1 << 18, 4, 3), dtype=np.int64)
    # half of the pool near grey, where the chroma numerators are small and of either sign
    pool[1::2] = np.clip(pool[1::2, :1, :1] + rng.integers(-6, 7, (1 << 17, 4, 3)), 0, 255)
    different = np.ones(len(pool), bool)                             # four different pixels
    for i in range(4):
        for j in range(i + 1, 4):
            different &= (pool[:, i] != pool[:, j]).any(axis=1)
    yn, un, vn = rgb_in_numerators(dst, pool)
    found, met = [], []
    for res in (1023, 0):
        hit = np.flatnonzero((yn % 1024 == res).any(axis=1))
        if hit.size:
            met.append("y%d" % res)
            found += hit[:3].tolist()
    for name, num in (("u", un), ("v", vn)):
        for res in (4095, 0):
            for sign in (1, -1):
                ok = (num % 4096 == res) & ((num > 0) if sign > 0 else (num < 0)) & different
                hit = np.flatnonzero(ok)
                if hit.size:
                    met.append("%s%d%s" % (name, res, "+" if sign > 0 else "-"))
                    found += hit[:3].tolist()
    corners = np.array(CORNERS, np.int64)
    flat = np.repeat(corners[:, None, :], 4, axis=1)
    mixed = np.stack([corners[[k, (k + 1) % 8, (k + 3) % 8, (k + 6) % 8]] for k in range(8)])
    patches = np.concatenate([pool[found], flat, mixed]).astype(np.uint8)
    _CACHE[key] = (patches, met)
    return _CACHE[key]


def patch_planes(patches, w):
    """patches [n, 4, c] laid out two rows a patch row in a picture w wide (w even; the list is repeated to fill whole
    rows): int planes [c][h, w]"""
    per_row = w // 2
    n = -(-len(patches) // per_row) * per_row
    p = patches[np.arange(n) % len(patches)].reshape(n // per_row, per_row, 2, 2, -1)   # [patch row, patch, y, x, channel]
    pic = p.transpose(0, 2, 1, 3, 4).reshape(2 * (n // per_row), w, -1)
    return [pic[:, :, c] for c in range(pic.shape[2])]


def rgb_picture(fmt, patches, w):
    """the patches as a packed picture of the format: ([plane [h, w * bpp]], h)"""
    r, g, b = patch_planes(patches, w)
    if fmt == R.RGB24:
        q = np.stack([r, g, b], axis=2)
    elif fmt == R.BGR24:
        q = np.stack([b, g, r], axis=2)
    else:                                                            # RGB32: B G R A in memory; alpha is not read
        q = np.stack([b, g, r, (r * 7 + b) & 255], axis=2)
    return [q.astype(np.uint8).reshape(r.shape[0], -1)], r.shape[0]


# ---- rgb_out ---------------------------------------------------------------------------------------------------------------

def rgb_out_numerators(src, y, cb, cr):
    """the three numerators (before >> 10 and the clamp) of r, g, b, as img_convert_ref._rgb_out has them"""
    F = R.FIX
    y, cb, cr = np.asarray(y, np.int64), np.asarray(cb, np.int64) - 128, np.asarray(cr, np.int64) - 128
    if src == R.YUVJ420P:
        yy, s = y << R.SCALEBITS, 1.0
    else:
        yy, s = (y - 16) * F(255.0 / 219.0), 255.0 / 224.0
    return (yy + F(1.40200 * s) * cr + R.ONE_HALF, yy - F(0.34414 * s) * cb - F(0.71414 * s) * cr + R.ONE_HALF,
            yy + F(1.77200 * s) * cb + R.ONE_HALF)


def rgb_out_triples(src):
    """(triples uint8 [n, 3] of (Y, Cb, Cr), met): met = {"steps": [...], "values": count, "colours": [...]} of what was found"""
    key = ("rgb_out", src)
    if key in _CACHE:
        return _CACHE[key]
    g = np.arange(256)
    yy, cc = np.meshgrid(g, g, indexing="ij")
    flat128 = np.full_like(yy, 128)
    # r depends on (Y, Cr), b on (Y, Cb): those searches are exhaustive.  g depends on all three: the planes through
    # Cb = 128 and Cr = 128, and every (Cb, Cr) at a dozen luma values
    some = np.unique(np.concatenate([np.arange(0, 256, 32), [1, 2, 3, 255]]))
    grids = {0: [(yy, flat128, cc)], 1: [(yy, flat128, cc), (yy, cc, flat128), np.meshgrid(some, g, g, indexing="ij")], 2: [(yy, cc, flat128)]}
    triples, steps, values = [], [], 0
    for ch in range(3):
        ys = np.concatenate([a[0].ravel() for a in grids[ch]])
        cbs = np.concatenate([a[1].ravel() for a in grids[ch]])
        crs = np.concatenate([a[2].ravel() for a in grids[ch]])
        num = rgb_out_numerators(src, ys, cbs, crs)[ch]
        val = num >> R.SCALEBITS
        wanted = [("=-1", val == -1), ("=0", val == 0), ("=255", val == 255), ("=256", val == 256), ("<-100", val < -100),
                  (">355", val > 355), ("neg%1023", (num < 0) & (num % 1024 == 1023)), ("neg%0", (num < 0) & (num % 1024 == 0))]
        for name, ok in wanted:
            hit = np.flatnonzero(ok)
            if hit.size:
                steps.append("%s%s" % ("rgb"[ch], name))
                pick = hit[[0, hit.size // 2, -1]] if name[0] in "<>" else hit[:2]
                if name == "<-100":
                    pick = [int(np.argmin(val))]
                if name == ">355":
                    pick = [int(np.argmax(val))]
                triples += [(ys[k], cbs[k], crs[k]) for k in pick]
        for v in range(256):
            hit = np.flatnonzero(val == v)
            if hit.size:
                values += 1
                triples.append((ys[hit[0]], cbs[hit[0]], crs[hit[0]]))
    colours = []
    sub = np.unique(np.concatenate([np.arange(0, 256, 3), [255]]))
    y3, cb3, cr3 = np.meshgrid(g, sub, sub, indexing="ij")
    n3 = [np.clip(n >> R.SCALEBITS, 0, 255) for n in rgb_out_numerators(src, y3, cb3, cr3)]
    for ch in range(3):
        for hi in (255, 0):
            ok = np.ones(y3.shape, bool)
            for k in range(3):
                ok &= n3[k] == (hi if k == ch else 255 - hi)
            hit = np.argwhere(ok)
            if hit.size:
                colours.append("%s=%d" % ("rgb"[ch], hi))
                i = hit[len(hit) // 2]
                triples.append((y3[tuple(i)], cb3[tuple(i)], cr3[tuple(i)]))
    _CACHE[key] = (np.array(triples, np.uint8), {"steps": steps, "values": values, "colours": colours})
    return _CACHE[key]


def yuv_picture(triples, w):
    """(Y, Cb, Cr) triples as 2 x 2 blocks (a chroma sample serves four pixels) of a 4:2:0 picture w wide: ([Y, Cb, Cr], h)"""
    blocks = np.repeat(triples[:, None, :], 4, axis=1)
    y, cb, cr = patch_planes(blocks, w)
    return [y.astype(np.uint8), cb[0::2, 0::2].astype(np.uint8), cr[0::2, 0::2].astype(np.uint8)], y.shape[0]


# ---- planes routes ---------------------------------------------------------------------------------------------------------

def value_picture(src, w, h, turn=0):
    """a planar picture whose every plane holds all 256 values (w * h >= 1024 for the 4:2:0 destinations' chroma), the chroma
    constant over what a shrinking route averages, so that the averaged sample is the value itself"""
    cw, ch = (w + 1) // 2, (h + 1) // 2
    assert cw * ch >= 256
    y = ((np.arange(w * h) + turn) % 256).reshape(h, w).astype(np.uint8)
    out = [y]
    for k in (1, 2):
        c = ((np.arange(cw * ch) * (1 if k == 1 else 255) + 37 * k + turn) % 256).reshape(ch, cw).astype(np.uint8)
        if src in R.P422 or src in R.P444:
            c = np.repeat(c, 2, axis=0)[:h]
        if src in R.P444:
            c = np.repeat(c, 2, axis=1)[:, :w]
        out.append(c)
    return out


SHRINK12_PAIRS = [(0, 0), (0, 1), (1, 0), (1, 1), (254, 255), (255, 254), (255, 255), (127, 128)]
# sums 0..3, 508..515 (both sides of 510 + 2 = 512), 1017..1020
SHRINK22_QUADS = ([(0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 1, 0), (1, 1, 0, 1)] +
                  [(127, 127, 127, 127 + k) for k in range(4)] + [(128, 128, 128, 128 + k) for k in range(4)] +
                  [(254, 254, 254, 255), (255, 254, 254, 255), (255, 255, 254, 255), (255, 255, 255, 255)])


def shrink_picture(src, w, turn=0):
    """a 4:2:2 / 4:4:4 picture w x 2 whose chroma columns go through the pairs / quads above (luma: a ramp)"""
    y = ((np.arange(2 * w) * 5 + turn) % 256).reshape(2, w).astype(np.uint8)
    out = [y]
    for k in (1, 2):
        if src in R.P422:
            cols = np.array([SHRINK12_PAIRS[(i + k + turn) % len(SHRINK12_PAIRS)] for i in range(w // 2)], np.uint8)   # [col, (top, bottom)]
            out.append(cols.T.copy())
        else:
            quads = np.array([SHRINK22_QUADS[(i + k + turn) % len(SHRINK22_QUADS)] for i in range(w // 2)], np.uint8)  # [col, (tl, tr, bl, br)]
            out.append(quads.reshape(w // 2, 2, 2).transpose(1, 0, 2).reshape(2, w).copy())
    return out
