"""Crafted coefficient blocks for the reconstruction kernels (a helper of the tests, imported as scan_builder is).

The entropy stage hands the reconstruction `[blocks, 64] int16` lines in scan order, six to an MCU (Y0 Y1 Y2 Y3 Cb Cr),
the DC already summed.  Decoded pictures hold small coefficients and pixels far from every clamp; random blocks do not
land on thresholds.  Here frames are written block by block so that each threshold of the two kernels is met on purpose:

  1  one coefficient at each of the 64 scan positions (the zig-zag, amvlib's [3][4] entry, each quantiser step);
  2  the shapes the reference's IDCT shortcuts look for: all-zero, DC only, only row 0, only column 0, every subset of
     rows holding only their first element;
  3  IDCT outputs of 254 .. 257 and -255 .. -258 before the iclp clamp, through the general path and every shortcut;
  4  flat MCUs over a (y, u, v) grid and triples that put each of R, G, B on -1 / 0 / 255 / 256 before its clamp; MCUs
     whose Y blocks and chroma samples are all different (placement, chroma sampling, byte order);
  5  every AC at +-1023 in sign patterns with the DC at the ends of int16: the largest sums a scan can make;
  6  FFmpeg-compat: products that wrap the int16 store (to +-32767, -32768, 0), `dc << 3` at its wrap, column sums on
     both sides of the crop at 0 / 255 and beyond the crop table;
  7  nmcu_ok at every place of a ten-MCU segment, widths whose last MCU keeps 1 .. 15 pixels, partial bottom MCU rows,
     9 MCU rows next to 8, 16x16 and 8x8.

Every case has a domain.  D: DC any int16, every AC within +-1023 -- all a scan can carry (AC sizes end at 10).  E: any
int16 anywhere, reachable through amvhip_reconstruct_dev only.  `in_bound` says whether the case lies inside what
include/amvhip.h promises for the amvlib modes (every |AC * step| <= AC_BOUND); D is inside it.

The expectation comes from the oracle's per-block primitives (amvo_dequant_idct_block, amvo_ffmpeg_dequant_block,
amvo_simple_idct_put); only the placement of the blocks and the colour conversion (AmvJpeg.c:805-831, three integer
lines) are whole-frame numpy here, and tests/test_coef_builder.py pins both against amvo_decode_frame,
amvo_decode_frame_ffmpeg and amvo_yuv_to_bgr.  The tables below are data of the wire format; the same test pins them.
"""
import numpy as np

import scan_builder as sb

D, E = "D", "E"
FLAG_FIXED = 1
COMP_OF = sb.COMP_OF
# what include/amvhip.h states for amvhip_reconstruct_dev in the amvlib modes ("What the stage accessor promises")
AC_BOUND = 100000

QUANT = (np.array([8, 6, 6, 7, 6, 5, 8, 7, 7, 7, 9, 9, 8, 10, 12, 20, 13, 12, 11, 11, 12, 25, 18, 19, 15, 20, 29, 26, 31, 30,
                   29, 26, 28, 28, 32, 36, 46, 39, 32, 34, 44, 39, 28, 28, 40, 55, 41, 44, 48, 49, 52, 52, 52, 31, 39, 57,
                   61, 56, 50, 60, 46, 51, 52, 50], np.int64),
         np.array([9, 9, 9, 12, 11, 12, 24, 13, 13, 24, 50, 33, 28, 33] + [50] * 50, np.int64))
Q60 = (np.array([13, 9, 10, 11, 10, 8, 13, 11, 10, 11, 14, 14, 13, 15, 19, 32, 21, 19, 18, 18, 19, 39, 28, 30, 23, 32, 46, 41,
                 49, 48, 46, 41, 45, 44, 51, 58, 74, 62, 51, 54, 70, 55, 44, 45, 64, 87, 65, 70, 76, 78, 82, 83, 82, 50, 62,
                 90, 97, 90, 80, 96, 74, 81, 82, 79], np.int64),
       np.array([14, 14, 14, 19, 17, 19, 38, 21, 21, 38, 79, 53, 45, 53] + [79] * 50, np.int64))
# scan position of each natural (row-major) position: the standard zig-zag
SCAN_OF_NATURAL = np.array([0, 1, 5, 6, 14, 15, 27, 28, 2, 4, 7, 13, 16, 26, 29, 42, 3, 8, 12, 17, 25, 30, 41, 43, 9, 11, 18, 24,
                            31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50,
                            56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63])
QUIRK_NATURAL, QUIRK_SCAN, QUIRK_STD = 3 * 8 + 4, 37, 31      # amvlib reads scan 37 at natural (3,4); the standard says 31


def stride(w):
    return (w * 24 + 31) // 32 * 4


def yuv420_bytes(w, h):
    return w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)


def line_of(nat):
    """an 8x8 block in natural order -> its scan-order line"""
    line = np.zeros(64, np.int64)
    line[SCAN_OF_NATURAL] = np.asarray(nat, np.int64).reshape(64)
    return line


def one(s, v, dc=None):
    line = np.zeros(64, np.int64)
    if dc is not None:
        line[0] = dc
    line[s] = v
    return line


def steps_of(nblocks, table=QUANT):
    """[nblocks, 64] the step of every coefficient, the component by the block's place in its MCU"""
    return np.stack([table[1 if k >= 4 else 0] for k in range(6)])[np.arange(nblocks) % 6]


def dequantised(coef, flags=0, table=QUANT):
    """[blocks, 64] lines -> [blocks, 8, 8] int64 natural-order products coef * step (no wrap): the INPUT of the
    reference's IDCT.  For building cases and for counting what they reach, never for the expectation."""
    coef = np.asarray(coef, np.int64)
    prod = coef * steps_of(coef.shape[0], table)
    nat = prod[:, SCAN_OF_NATURAL]
    if table is QUANT and not flags & FLAG_FIXED:
        nat[:, QUIRK_NATURAL] = prod[:, QUIRK_SCAN]
    return nat.reshape(-1, 8, 8)


# ------------------------------------------------------------------------------------------------ the expectation

def idct_blocks(orc, coef, flags):
    """amvo_dequant_idct_block of every line -> [blocks, 64] int32 (luma with its +128)"""
    coef = np.ascontiguousarray(coef, np.int16)
    out = np.empty((coef.shape[0], 64), np.int32)
    fn, cp, op = orc.lib().amvo_dequant_idct_block, coef.ctypes.data, out.ctypes.data
    for b in range(coef.shape[0]):
        fn(cp + 128 * b, COMP_OF[b % 6], flags, op + 256 * b)
    return out


def ffmpeg_blocks(orc, coef, put=True):
    """amvo_ffmpeg_dequant_block + amvo_simple_idct_put of every line -> [blocks, 64] uint8; put=False: amvo_simple_idct,
    the int16 values in front of the crop"""
    coef = np.ascontiguousarray(coef, np.int16)
    L = orc.lib()
    blk = np.empty((coef.shape[0], 64), np.int16)
    px = np.empty((coef.shape[0], 64), np.uint8)
    cp, bp, pp = coef.ctypes.data, blk.ctypes.data, px.ctypes.data
    for b in range(coef.shape[0]):
        L.amvo_ffmpeg_dequant_block(cp + 128 * b, COMP_OF[b % 6], bp + 128 * b)
        if put:
            L.amvo_simple_idct_put(pp + 64 * b, 8, bp + 128 * b)
        else:
            L.amvo_simple_idct(bp + 128 * b)
    return px if put else blk


def colour_terms(y, u, v):
    """StoreBuffer's three sums in front of their clamps (AmvJpeg.c:808-810), int32 arrays -> (bb, gg, rr)"""
    y, u, v = (np.asarray(a, np.int32) for a in (y, u, v))
    return ((y * 256 + 411 * u - 29 * v) >> 8, (y * 256 - 159 * u - 220 * v) >> 8, (y * 256 + 18 * u + 367 * v) >> 8)


def yuv_to_bgr(y, u, v):
    """... clamped to bytes (:812-831) -> uint8 [..., 3] in the order B, G, R"""
    return np.stack([np.clip(t, 0, 255) for t in colour_terms(y, u, v)], -1).astype(np.uint8)


def _planes(px, mcw, mch):
    """[mcus * 6, 64] block values -> the three planes in scan coordinates: Y [mch*16, mcw*16], Cb, Cr [mch*8, mcw*8]
    (GetYUV, AmvJpeg.c:754-787: Y0 Y1 over Y2 Y3)"""
    px = px.reshape(mch, mcw, 6, 8, 8)
    y = np.empty((mch, 2, 8, mcw, 2, 8), px.dtype)
    for k in range(4):
        y[:, k >> 1, :, :, k & 1, :] = px[:, :, k].transpose(0, 2, 1, 3)
    cb = px[:, :, 4].transpose(0, 2, 1, 3).reshape(mch * 8, mcw * 8)
    cr = px[:, :, 5].transpose(0, 2, 1, 3).reshape(mch * 8, mcw * 8)
    return y.reshape(mch * 16, mcw * 16), cb, cr


def _decoded(nmcu_ok, mcw, mch, scale):
    """which samples of a plane belong to MCUs in front of nmcu_ok"""
    ok = (np.arange(mcw * mch) < nmcu_ok).reshape(mch, mcw)
    return np.repeat(np.repeat(ok, scale, 0), scale, 1)


def picture(orc, coef, w, h, nmcu_ok, flags):
    """the amvlib modes: what amvo_decode_frame stores for these coefficients -> uint8 [h, stride(w)], bottom-up BGR,
    zero where nothing was decoded and in the row padding"""
    mcw, mch = (w + 15) // 16, (h + 15) // 16
    y, cb, cr = _planes(idct_blocks(orc, coef, flags), mcw, mch)
    up = lambda c: np.repeat(np.repeat(c, 2, 0), 2, 1)                    # sample (i >> 1, j >> 1), :805-807
    bgr = yuv_to_bgr(y, up(cb), up(cr))
    bgr[~_decoded(nmcu_ok, mcw, mch, 16)] = 0
    out = np.zeros((h, stride(w)), np.uint8)
    out[:, : w * 3] = bgr[:h, :w][::-1].reshape(h, w * 3)                 # picture row r is stored as row h-1-r, :800
    return out


def picture_ffmpeg(orc, coef, w, h, nmcu_ok):
    """FFmpeg-compat: what amvo_decode_frame_ffmpeg stores -> uint8 [yuv420_bytes(w, h)]: plane row p of a component
    with vertical factor v holds scan row v * (8 * mcu_rows - ((h / 2) & 7)) - 1 - p (mjpegdec.c:672-677); rows the
    formula sends outside stay zero"""
    mcw, mch = (w + 15) // 16, (h + 15) // 16
    planes = _planes(ffmpeg_blocks(orc, coef), mcw, mch)
    out = []
    for c, s in enumerate(planes):
        v = 2 if c == 0 else 1
        s = s * _decoded(nmcu_ok, mcw, mch, 8 * v)
        pw, ph = (w, h) if c == 0 else ((w + 1) // 2, (h + 1) // 2)
        plane = np.zeros((ph, pw), np.uint8)
        start = v * (8 * mch - ((h // 2) & 7)) - 1
        p = np.arange(ph)
        inside = start - p >= 0
        plane[p[inside]] = s[start - p[inside], :pw]
        out.append(plane.reshape(-1))
    return np.concatenate(out)


def preclamp(orc, line, comp, flags=0):
    """the 64 IDCT outputs of a block IN FRONT of the iclp clamp (without luma's +128), measured with the oracle alone:
    8 more in the dequantised DC is exactly 1 more in every output before the clamp -- 64 after the row pass
    ((dc * 2048 + 128) >> 8, or the shortcut's 8 * dc), 64 * 256 = 1 << 14 in every column sum, or the column shortcut's
    (x + 32) >> 6 -- so the block is decoded with its DC moved down and up by 304 and 600 coefficients (as many levels
    in luma, 9 / 8 as many in chroma) and the move is added back where the moved output sits strictly inside the clamp.
    None where an output is inside the clamp under none of the moves (beyond +-850: not what this is for)."""
    moves = (0, -304, 304, -600, 600)
    slots = np.zeros((6 * len(moves), 64), np.int64)
    at = [6 * i + (0 if comp == 0 else 4) for i in range(len(moves))]
    slots[at] = line
    slots[at, 0] += moves
    assert abs(slots[:, 0]).max() < 32768
    out = idct_blocks(orc, slots, flags)[at].astype(np.int64) - (128 if comp == 0 else 0)
    pre, found = np.zeros(64, np.int64), np.zeros(64, bool)
    for o, m in zip(out, moves):
        free = (o > -256) & (o < 255) & ~found
        pre[free] = o[free] - (m if comp == 0 else m * 9 // 8)
        found |= free
    return pre if found.all() else None


# ------------------------------------------------------------------------------------------------ the corpus

class Case:
    """one corpus frame: name, geometry, coef [blocks, 64] int16, nmcu_ok, domain (D / E), in_bound (inside what the header
    promises for the amvlib modes), dense_only (not a frame a scan can carry as it stands: an E case, an nmcu_ok in front
    of the frame's end, or a DC more than +-2047 from the component's DC before it) with the reason in `why`"""

    def __init__(self, name, w, h, coef, nmcu_ok=None, domain=None):
        self.name, self.w, self.h = name, w, h
        self.nmcu = sb.mcus(w, h)
        coef = np.asarray(coef, np.int64)
        assert coef.shape == (self.nmcu * 6, 64) and coef.min() >= -32768 and coef.max() <= 32767, name
        self.coef = np.ascontiguousarray(coef.astype(np.int16))
        self.nmcu_ok = self.nmcu if nmcu_ok is None else nmcu_ok
        in_d = int(np.abs(coef[:, 1:]).max()) <= 1023
        self.domain = domain or (D if in_d else E)
        assert self.domain == E or in_d, name
        self.in_bound = int((np.abs(coef) * steps_of(coef.shape[0]))[:, 1:].max()) <= AC_BOUND
        assert self.in_bound or self.domain == E, name
        self.why = None
        if self.domain == E:
            self.why = "E: an AC beyond +-1023"
        elif self.nmcu_ok != self.nmcu:
            self.why = "nmcu_ok in front of the frame's end"
        else:
            for c in range(3):
                dc = coef[[b for b in range(coef.shape[0]) if COMP_OF[b % 6] == c], 0]
                if np.abs(np.diff(np.concatenate([[0], dc]))).max() > 2047:
                    self.why = "a DC difference beyond +-2047"
        self.dense_only = self.why is not None

    def chunk(self):
        """the frame as a scan (valid frames only)"""
        assert not self.dense_only, (self.name, self.why)
        return sb.assemble(sb.blocks_from_coefficients(self.coef)).chunk


def ordinary(rng, w, h):
    """a frame of ordinary content: small DCs, a few small ACs at the low scan positions"""
    nb = sb.mcus(w, h) * 6
    coef = np.zeros((nb, 64), np.int64)
    coef[:, 0] = np.cumsum(rng.integers(-6, 7, nb)) % 97 - 48
    coef[:, 1:12] = rng.integers(-12, 13, (nb, 11)) * (rng.random((nb, 11)) < 0.35)
    return coef


def _pack(cases, name, luma, chroma, w=160, h=120):
    """lines into whole 160x120 frames -- D lines, E lines inside the bound (Ei) and E lines beyond it (Eo) apart: an MCU
    takes four of the luma list and two of the chroma list; a list that runs out starts again one place on, so that its
    lines meet the other block slots"""
    nm = sb.mcus(w, h)

    def kind(line, comp):
        if int(np.abs(line[1:]).max()) <= 1023:
            return D
        return "Ei" if int((np.abs(line) * QUANT[comp])[1:].max()) <= AC_BOUND else "Eo"

    for dom in (D, "Ei", "Eo"):
        lu, ch = [l for l in luma if kind(l, 0) == dom], [l for l in chroma if kind(l, 1) == dom]
        if not lu and not ch:
            continue
        lu = lu or [np.zeros(64, np.int64)]
        ch = ch or [np.zeros(64, np.int64)]
        need = max((len(lu) + 3) // 4, (len(ch) + 1) // 2)
        for f in range((need + nm - 1) // nm):
            coef = np.zeros((nm * 6, 64), np.int64)
            for m in range(nm):
                g = f * nm + m
                for k in range(6):
                    src, i = (lu, 4 * g + k) if k < 4 else (ch, 2 * g + k - 4)
                    coef[m * 6 + k] = src[(i + i // len(src)) % len(src)]
            cases.append(Case("%s_%s%d" % (name, dom, f), w, h, coef, domain=dom[0]))
            assert cases[-1].in_bound == (dom != "Eo")
            if dom == D and cases[-1].dense_only:
                # ... and once more as a frame a scan can carry: every DC as near to its value as +-2047 from the
                # component's DC before it allows
                dc = [0, 0, 0]
                for b in range(nm * 6):
                    c = COMP_OF[b % 6]
                    dc[c] += int(np.clip(coef[b, 0] - dc[c], -2047, 2047))
                    coef[b, 0] = dc[c]
                cases.append(Case("%s_%s%d_scan" % (name, dom, f), w, h, coef, domain=D))


def _placement(comp):
    q, out = QUANT[comp], []
    for s in range(64):
        t = 802500 // int(q[s])       # the smallest single dequantised coefficient a model of the kernel got wrong
        vals = [1, -1, 1023, -1023, 32767, -32767, -32768] + [v for v in (t, t + 1, -t, -t - 1) if -32768 <= v <= 32767]
        out += [one(s, v) for v in vals]
        if s:
            t = AC_BOUND // int(q[s])      # the last coefficient inside what the header promises, the first beyond it
            out += [one(s, v) for v in (t, -t, t + 1, -t - 1)]
            out += [one(s, v, dc=-37) for v in (1023, -1023)]
    return out


def _signs(rng, n, kind):
    if kind == "rand":
        return rng.integers(1, 1024, n) * rng.choice([-1, 1], n)
    return np.full(n, 1023) * {"+": np.ones(n, np.int64), "-": -np.ones(n, np.int64), "alt": np.where(np.arange(n) % 2, -1, 1)}[kind]


def _shortcuts(rng, comp):
    q, out = QUANT[comp], [np.zeros(64, np.int64)]
    out += [one(0, dc) for dc in (1, -1, 255, -256, 1023, -1024, 4095, 32767, -32767, -32768)]
    for kind in ("rand", "+", "-", "alt"):
        for dc in (0, int(rng.integers(-32768, 32768))):
            for axis in (0, 1):
                nat = np.zeros((8, 8), np.int64)
                if axis == 0:
                    nat[0, :] = _signs(rng, 8, kind)       # only row 0: every column is top-element-only after the row pass
                else:
                    nat[:, 0] = _signs(rng, 8, kind)       # only column 0: every row holds only its first element
                nat[0, 0] = dc
                out.append(line_of(nat))
    for subset in range(256):        # the rows of the subset hold only their first element, the others are general
        rows = [r for r in range(8) if subset >> r & 1]
        for kind in ("rand", "+", "alt"):
            nat = _signs(rng, 64, kind).reshape(8, 8)
            nat[rows, 1:] = 0
            nat[0, 0] = int(rng.integers(-32768, 32768))
            out.append(line_of(nat))
            if 3 in rows and kind == "alt":
                out[-1][QUIRK_SCAN] = 0      # amvlib's table puts scan 37 into row 3: first-element-only under it too
        # E: first elements at and around 2^20 / step, where the row formula's dc * 2048 leaves 32 bits and the shortcut's
        # 8 * dc does not (steps too small for that: the ends of int16)
        nat = _signs(rng, 64, "rand").reshape(8, 8)
        nat[rows, 1:] = 0
        for r in rows:
            t = (1 << 20) // int(q[SCAN_OF_NATURAL[8 * r]])
            near = [v for v in (t - 1, t, t + 1, -t + 1, -t, -t - 1, -t - 2) if -32768 <= v <= 32767 and r]
            nat[r, 0] = int(rng.choice(near or [32767, -32768, -32767, 20000]))
        if not rows or rows == [0]:
            nat[1, 1] = 32767      # (an E line all the same)
        out.append(line_of(nat))
    # E: only row 0, its results at and around 2^23 - 32 where the column formula's x * 256 + 8192 leaves 32 bits and the
    # shortcut's (x + 32) >> 6 does not: with coefficients at natural (0,0) and (0,4) alone the row pass gives
    # 8 * (dc * step0 + c * step14) in columns 0, 3, 4, 7
    for c14 in (20970, 20971, -20971, -20972, 32767, -32768):
        for dc in range(4, 12):
            out.append(one(14, c14, dc=dc if c14 > 0 else -dc))
    return out


def _aim(orc, rng, comp, shape, target):
    """a block of the given shape whose largest (target > 0) or smallest IDCT output in front of the clamp is `target`"""
    for _ in range(200):
        nat = np.zeros((8, 8), np.int64)
        if shape == "general":
            at = rng.choice(63, 12, replace=False) + 1
            nat.reshape(64)[at] = rng.integers(-9, 10, 12)
        elif shape == "rows_shortcut":
            nat[1:, 0] = rng.integers(-25, 26, 7)
        elif shape == "columns_shortcut":
            nat[0, 1:] = rng.integers(-25, 26, 7)
        line = line_of(nat)
        pre = preclamp(orc, line, comp)
        ext = int(pre.max() if target > 0 else pre.min())
        guess = target - ext if comp == 0 else int(round((target - ext) * 8 / 9))
        for dc in ([guess] if comp == 0 else range(guess - 2, guess + 3)):
            line[0] = dc
            pre = preclamp(orc, line, comp)
            if int(pre.max() if target > 0 else pre.min()) == target:
                return line.copy()
        if shape == "dc_only":
            return None      # chroma's DC step is 9 against 8: a flat block skips one level in nine
    raise ValueError("no %s block reaches %d" % (shape, target))


ICLP_EDGES = (254, 255, 256, 257, -255, -256, -257, -258)
ICLP_SHAPES = ("general", "rows_shortcut", "columns_shortcut", "dc_only")


def _iclp(orc, rng, comp):
    out = [_aim(orc, rng, comp, shape, t) for shape in ICLP_SHAPES for t in ICLP_EDGES for _ in range(1 if shape == "dc_only" else 3)]
    return [line for line in out if line is not None]


def _flat_levels(orc):
    """chroma value -> a DC coefficient of a DC-only chroma block that gives it (the step is 9: not every value exists)"""
    cs = np.arange(-300, 301)
    lines = np.zeros((cs.size * 6, 64), np.int64)
    lines[4::6, 0] = cs
    val = idct_blocks(orc, lines, 0)[4::6, 0]
    return {int(v): int(c) for v, c in zip(val[::-1], cs[::-1])}


def _colour(orc, rng, cases):
    level = _flat_levels(orc)
    assert min(level) == -256 and max(level) == 255
    us = np.array(sorted(level), np.int32)
    triples = [(y, u, v) for y in (-128, -1, 0, 255, 256, 383) for u in (-256, -1, 0, 255) for v in (-256, -1, 0, 255)]
    # triples that put each channel on each side of each clamp
    yy, uu, vv = np.meshgrid(np.arange(-128, 384, dtype=np.int32), us[::7], us[::5], indexing="ij")
    for t in colour_terms(yy, uu, vv):
        for edge in (-1, 0, 255, 256):
            hit = np.argwhere(t == edge)
            for i in hit[np.linspace(0, len(hit) - 1, 3).astype(int)]:
                triples.append((int(yy[tuple(i)]), int(uu[tuple(i)]), int(vv[tuple(i)])))
    mcus = []
    for y, u, v in triples:
        m = np.zeros((6, 64), np.int64)
        m[:4, 0] = y - 128            # a DC-only luma block is its DC coefficient (step 8), clamped to -256 .. 255, + 128
        m[4, 0], m[5, 0] = level[u], level[v]
        mcus.append(m)
    # MCUs whose four Y blocks differ and whose 64 Cb and 64 Cr samples are all different: chroma blocks by search
    distinct = []
    for _ in range(1500):
        m = np.zeros((60, 64), np.int64)
        m[:, 0] = rng.integers(-20, 21, 60)
        m[:, 1:10] = rng.integers(-40, 41, (60, 9))
        px = idct_blocks(orc, m, 0)
        distinct += [m[b] for b in range(4, 60, 6) if len(set(px[b].tolist())) == 64]
        if len(distinct) >= 16:
            break
    else:
        raise ValueError("the search found %d chroma blocks of 64 different samples" % len(distinct))
    for i in range(8):
        m = np.zeros((6, 64), np.int64)
        m[:4, 0] = rng.permutation(81)[:4] - 40
        m[:4, 1:10] = rng.integers(-14, 15, (4, 9))
        m[4], m[5] = distinct[2 * i], distinct[2 * i + 1]
        mcus.append(m)
    nm = sb.mcus(160, 120)
    for f in range((len(mcus) + nm - 1) // nm):
        coef = np.concatenate([mcus[(f * nm + m) % len(mcus)] for m in range(nm)])
        cases.append(Case("colour_%d" % f, 160, 120, coef))
    return triples


PATTERNS = ("plus", "minus", "by_row", "by_column", "checkerboard")


def _pattern(kind):
    r, c = np.indices((8, 8))
    sign = {"plus": np.ones((8, 8), np.int64), "minus": -np.ones((8, 8), np.int64), "by_row": 1 - 2 * (r & 1),
            "by_column": 1 - 2 * (c & 1), "checkerboard": 1 - 2 * ((r + c) & 1)}[kind]
    return line_of(1023 * sign)


def _large_sums(cases):
    lines = []
    for kind in PATTERNS:
        for dc in (32767, -32767, -32768, 0):
            line = _pattern(kind)
            line[0] = dc
            lines.append(line)
    _pack(cases, "large_sums", lines, lines)
    # the same as a frame a scan can carry: 63 ACs at +-1023 in every block of every segment, each component's DC
    # walking between the ends of int16 in steps of 2047
    nb = sb.mcus(160, 120) * 6
    coef = np.stack([_pattern(PATTERNS[(b // 6 + b) % 5]) for b in range(nb)])
    dc, step = [0, 0, 0], [2047, -2047, 2047]
    for b in range(nb):
        c = COMP_OF[b % 6]
        nxt = dc[c] + step[c]
        if not -32768 <= nxt <= 32767:
            nxt = 32767 if nxt > 0 else -32768
            step[c] = -step[c]
        dc[c] = nxt
        coef[b, 0] = nxt
    cases.append(Case("large_sums_walk", 160, 120, coef))


def wrap16(x):
    return (np.asarray(x, np.int64) + 32768) % 65536 - 32768


def _ffmpeg_wraps(orc, rng, comp):
    q, out = Q60[comp], []
    cs = np.arange(-32768, 32768, dtype=np.int64)
    for s in range(64):
        prod = cs * int(q[s]) + (1024 if s == 0 else 0)
        first = int(SCAN_OF_NATURAL[8 * (int(np.nonzero(SCAN_OF_NATURAL == s)[0][0]) // 8)])   # the row's first element
        for target in (32767, -32768, 0, 32766, -32767):
            hit = cs[(wrap16(prod) == target) & (prod != target)]                # lands there through the wrap alone
            if hit.size:
                line = one(s, int(hit[np.argmin(np.abs(hit))]), dc=7 if s else None)
                if target == 0 and first not in (s, 0):
                    line[first] = 3      # the row holds only its first element once the product has wrapped to 0
                out.append(line)
            hit = cs[prod == target]
            if hit.size and target:
                out.append(one(s, int(hit[0]), dc=7 if s else None))
    # flat = (int16)(first << 3) at its wrap: first elements either side of +-4096, in row 0 (the DC, + 1024) and below
    for r in range(8):
        s = int(SCAN_OF_NATURAL[8 * r])
        for edge in (4095, 4096, -4096, -4097):
            c = (edge - (1024 if s == 0 else 0)) // int(q[s])
            out += [one(s, c + d) for d in (0, 1)]
    # DC-only blocks whose outputs sit on both sides of the crop at 0 and 255 and beyond the crop table (-1024 .. 1279)
    cand = np.arange(-1300, 1301)
    at = 0 if comp == 0 else 4
    lines = np.zeros((cand.size * 6, 64), np.int64)
    lines[at::6, 0] = cand
    val = ffmpeg_blocks(orc, lines, put=False)[at::6, 0]
    for want in (-1, 0, 1, 254, 255, 256, -1025, -1024, 1279, 1280):
        hit = cand[val == want]
        if hit.size:
            out.append(one(0, int(hit[0])))
    # ... and through the general path
    for _ in range(24):
        line = np.zeros(64, np.int64)
        line[0] = int(rng.choice([-79, 78, -40, 40, -700, 700]))
        line[1:20] = rng.integers(-30, 31, 19)
        out.append(line)
    return out


GEOMETRIES = ((176, 144), (176, 128), (16, 16), (8, 8)) + tuple((160 + k, 24) for k in (2, 4, 6, 8, 10, 12, 14)) + \
             ((161, 24), (163, 18), (175, 40), (32, 17))


def _edges(rng, cases):
    W, H = 160, 120
    busy = lambda w, h: ordinary(rng, w, h) * 3 + rng.integers(-2, 3, (sb.mcus(w, h) * 6, 64)) * (np.arange(64) < 6)
    for ok in [0, 1, 9] + list(range(10, 21)) + [79]:
        cases.append(Case("nmcu_ok_%d" % ok, W, H, busy(W, H), nmcu_ok=ok))
    for w, h in GEOMETRIES:
        nm = sb.mcus(w, h)
        mcw = (w + 15) // 16
        cases.append(Case("whole_%dx%d" % (w, h), w, h, busy(w, h)))
        for ok in sorted({0, mcw - 1, mcw, nm - 1} - {nm, -1}):
            cases.append(Case("nmcu_ok_%d_%dx%d" % (ok, w, h), w, h, busy(w, h), nmcu_ok=ok))


def corpus(orc, seed=0xC0EF):
    """-> (cases, the (y, u, v) triples of class 4)"""
    rng = np.random.default_rng(seed)
    cases = []
    _pack(cases, "placement", _placement(0), _placement(1))
    _pack(cases, "shortcuts", _shortcuts(rng, 0), _shortcuts(rng, 1))
    _pack(cases, "iclp", _iclp(orc, rng, 0), _iclp(orc, rng, 1))
    triples = _colour(orc, rng, cases)
    _large_sums(cases)
    _pack(cases, "ffmpeg_wraps", _ffmpeg_wraps(orc, rng, 0), _ffmpeg_wraps(orc, rng, 1))
    _edges(rng, cases)
    assert len({c.name for c in cases}) == len(cases)
    return cases, triples


def batches(cases, seed=0xBA7C):
    """per geometry: the cases, each between two ordinary frames -> [{w, h, cases, where (their places in the batch),
    coef [n, blocks, 64] int16, nmcu_ok [n] uint32}]"""
    rng = np.random.default_rng(seed)
    by_geom = {}
    for c in cases:
        by_geom.setdefault((c.w, c.h), []).append(c)
    out = []
    for (w, h), cs in by_geom.items():
        frames, oks, where = [ordinary(rng, w, h)], [sb.mcus(w, h)], []
        for c in cs:
            where.append(len(frames))
            frames += [c.coef, ordinary(rng, w, h)]
            oks += [c.nmcu_ok, sb.mcus(w, h)]
        out.append({"w": w, "h": h, "cases": cs, "where": where, "coef": np.stack(frames).astype(np.int16),
                    "nmcu_ok": np.array(oks, np.uint32)})
    return out
