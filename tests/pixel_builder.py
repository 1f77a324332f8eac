"""Crafted pictures for the video encoder kernels (a helper of the tests, imported as scan_builder and coef_builder are).

The encoder has no entry that takes coefficients: pixels are the only handle.  Through the YUVJ420P entry a sample is the
byte minus 128, so a block of the transform's input can be written exactly.  Blocks are made by a clipped, rounded
inverse DCT of a target coefficient pattern; the oracle's per-block primitives (amvo_fdct_islow, amvo_quantize_block)
then say what the block really quantises to, and it is kept only where that is what was meant.  Ordinary content --
synthetic frames, noise -- sits far from the thresholds the kernels depend on; here every case is one frame written
block by block (or pixel by pixel) so that a named threshold is met on purpose:

  1  symbols   every AC symbol 8-bit samples can reach, both tables, both signs, with the smallest and the largest
               magnitude of its size that a block reaches; every DC difference size 0 .. 8, both signs, each predictor
  2  runs      zero runs of 16 .. 62 (one, two, three ZRLs), coefficient 63 alone and with others (no EOB), 63 non-zero
               ACs, the non-zero positions {31} {32} {31, 32} {63} {31, 63} (the halves of the mask, the shifts that wrap)
  3  split     segments of fewer than 64, of 64 and of 65 symbols; a lane's run starting inside a block at its second
               symbol, its last coefficient, its EOB and just behind coefficient 31; runs on both sides of 256 bits
  4  predictor 176x80 (6 + 5 MCUs, 10 segments, 3 rounds) and 336x16 (3 segments of 7): large DC steps at the first MCU
               of every segment, on Y0, Cb and Cr apart and together
  5  window    a non-final flush with each of 0 .. 7 bits carried over; a last round, and a first round, that does not
               fit (the frame is handed back); a round that fits only after the flush
  6  ff        FF at each byte of a window word, FF runs, FF on both sides of byte 1024 of a flush, FF as the last whole
               byte, tails of 0 .. 7 bits, a padded last byte that is FF (searched with the oracle)
  7  range     for each of the 64 outputs the 127 / -128 sign pattern that maximises it and the one that minimises it,
               checkerboard, stripes, flat 127 and flat -128 -- in chroma blocks and in all four luma blocks of an MCU
  8  quantiser DC sums on both sides of a rounding step (t = 0, 1, the largest; both signs; divisors 64 and 72); the
               transform's output on the last value that quantises to 0 and on the first that quantises to +-1, for every
               position, both tables, both signs, qbias 0 and 128: 504 thresholds, of which the +-1 search over single
               pixels meets 504 exactly on both sides (AC_THRESHOLDS_MET; tests/test_pixel_builder.py asserts it)
  9  rgb       RGB24 / BGR24 pixels: triples that put the luma sum and the 2x2 chroma sums on both sides of a rounding
               step, 0 and 255 in every channel, 2x2 patches of four different pixels, widths whose last MCU keeps 2, 6,
               10, 14 pixels, heights that end 2 and 14 rows into an MCU row, every row and column unlike its neighbour

What 8-bit samples cannot reach: AC sizes 9 and 10 (the largest |AC| a block gave is under 256), DC differences of
sizes 9 .. 11 (a DC is -128 .. 127).

The expectation is never made here: it is the oracle's amvo_encode_frame / amvo_encode_frame_yuv420 of the case's
source.  The models below -- the symbol numbering, the split into lanes, the bits per run, the window -- restate
amv_encode_par.hip for building cases and for counting what they reach only.
"""
import numpy as np

import coef_builder as cb
import scan_builder as sb

QUANT = cb.QUANT
SCAN_OF_NATURAL = cb.SCAN_OF_NATURAL
NATURAL_OF_SCAN = np.argsort(SCAN_OF_NATURAL)
COMP_OF = sb.COMP_OF
SEED = 0xA11CE
POISON = 0xEE
# amv_encode_par.hip: the bit-string window, a lane's scratch, MCUs per segment, waves per frame, bytes per flush tile
WINDOW_BITS, OWN_BITS, SEG_MCUS, WAVES, TILE_BYTES = 1280 * 32, 256, 10, 4, 1024
AC_THRESHOLDS, AC_THRESHOLDS_MET = 504, 504
BIG, TALL = (176, 80), (336, 16)

_C = np.array([[(np.sqrt(0.125) if u == 0 else 0.5) * np.cos((2 * x + 1) * u * np.pi / 16) for x in range(8)] for u in range(8)])
# BASIS[natural position u * 8 + v, sample row * 8 + column]: the orthonormal DCT; the transform's outputs are 8 times it
BASIS = np.einsum("ux,vy->uvxy", _C, _C).reshape(64, 64)


# ------------------------------------------------------------------------------------------------ oracle primitives

def fdct(orc, samples):
    """[n, 64] samples of -128 .. 127 (row-major) -> [n, 64] int16 amvo_fdct_islow outputs, natural order"""
    blk = np.array(samples, np.int16).reshape(-1, 64)
    fn, p = orc.lib().amvo_fdct_islow, blk.ctypes.data
    for b in range(blk.shape[0]):
        fn(p + 128 * b)
    return blk


def quantise(orc, dct, comp, qbias=0):
    """[n, 64] transform outputs -> [n, 64] int16 lines in scan order (amvo_quantize_block); comp: 0 luma, else chroma, one
    for all or one per block"""
    dct = np.ascontiguousarray(dct, np.int16).reshape(-1, 64)
    comp = np.broadcast_to(np.asarray(comp), (dct.shape[0],))
    out = np.empty_like(dct)
    fn, dp, op = orc.lib().amvo_quantize_block, dct.ctypes.data, out.ctypes.data
    for b in range(dct.shape[0]):
        fn(dp + 128 * b, int(comp[b]), qbias, op + 128 * b)
    return out


def lines_of(orc, samples, comp, qbias=0):
    return quantise(orc, fdct(orc, samples), comp, qbias)


def samples_of(lines, comp, gain=1.0):
    """the clipped, rounded inverse DCT of [n, 64] lines (scan order, in quantiser steps; fractions allowed)"""
    target = (np.asarray(lines, np.float64).reshape(-1, 64) * QUANT[1 if comp else 0])[:, SCAN_OF_NATURAL] * gain
    return np.clip(np.rint(target @ BASIS), -128, 127).astype(np.int16)


# ------------------------------------------------------------------------------------------------ frames

def mcu_grid(w, h):
    return (w + 15) // 16, (h + 15) // 16


def planes_of_blocks(blocks, w, h):
    """[mcus * 6, 64] sample blocks in scan coordinates (w, h multiples of 16) -> the picture's (Y, Cb, Cr) uint8 planes:
    bitstream row k is picture row h - 1 - k"""
    assert w % 16 == 0 and h % 16 == 0
    y, u, v = cb._planes(np.asarray(blocks, np.int16), w // 16, h // 16)
    return tuple(np.ascontiguousarray((p[::-1] + 128).astype(np.uint8)) for p in (y, u, v))


def blocks_of_planes(Y, Cb, Cr, w, h):
    """the sample blocks the encoder transforms, MCU order: rows below and columns right of the picture repeat the nearest
    edge sample (row 0 of the picture, its last column).  A model of the placement; test_pixel_builder pins it."""
    mcw, mch = mcu_grid(w, h)
    out = []
    for plane, pw, ph, n in ((Y, w, h, 16), (Cb, w // 2, h // 2, 8), (Cr, w // 2, h // 2, 8)):
        r, c = np.arange(mch * n), np.arange(mcw * n)
        s = plane[np.where(r < ph, ph - 1 - r, 0)][:, np.minimum(c, pw - 1)].astype(np.int16) - 128
        if n == 16:
            out.append(s.reshape(mch, 2, 8, mcw, 2, 8).transpose(0, 3, 1, 4, 2, 5).reshape(mch, mcw, 4, 64))
        else:
            out.append(s.reshape(mch, 8, mcw, 8).transpose(0, 2, 1, 3).reshape(mch, mcw, 1, 64))
    return np.concatenate(out, 2).reshape(-1, 64)


def to_planes(orc, pix, w, h, bgr):
    """the oracle's rgb24_to_yuvj420p of [h, w, 3] pixels"""
    pix = np.ascontiguousarray(pix, np.uint8)
    Y, Cb, Cr = np.zeros((h, w), np.uint8), np.zeros((h // 2, w // 2), np.uint8), np.zeros((h // 2, w // 2), np.uint8)
    orc.lib().amvo_rgb24_to_yuvj420p(pix.ctypes.data, w * 3, w, h, 1 if bgr else 0, Y.ctypes.data, Cb.ctypes.data, Cr.ctypes.data)
    return Y, Cb, Cr


class Case:
    """one corpus frame: name, group, geometry, kind ("yuv", "rgb", "bgr"), the qbias it was built for, its source --
    planes (Y, Cb, Cr) for every kind (an RGB case's are the oracle's conversion), pix [h, w, 3] for rgb / bgr -- and
    `meta`: what the builder aimed at, for test_pixel_builder to check against the oracle"""

    def __init__(self, name, group, w, h, planes=None, pix=None, kind="yuv", qbias=0, meta=None):
        self.name, self.group, self.w, self.h, self.kind, self.qbias = name, group, w, h, kind, qbias
        self.planes, self.pix, self.meta = planes, pix, meta or {}
        assert w % 2 == 0 and h % 2 == 0 and (pix is None) == (kind == "yuv")

    def chunk(self, orc, qbias=None):
        """the expectation: the oracle's chunk"""
        q = self.qbias if qbias is None else qbias
        if self.kind == "yuv":
            return orc.encode_frame_yuv(*self.planes, self.w, self.h, qbias=q)
        return orc.encode_frame(self.pix, self.w, self.h, bgr=self.kind == "bgr", qbias=q)

    def lines(self, orc, qbias=None):
        """the oracle's coefficients: amvo_encode_frame's own for pixels; for planes amvo_quantize_block of amvo_fdct_islow
        of the blocks (test_pixel_builder: they are what the oracle's chunk decodes to)"""
        q = self.qbias if qbias is None else qbias
        if self.kind != "yuv":
            return orc.encode_frame(self.pix, self.w, self.h, bgr=self.kind == "bgr", qbias=q, want_coef=True)[1]
        blocks = blocks_of_planes(*self.planes, self.w, self.h)
        return lines_of(orc, blocks, [0, 0, 0, 0, 1, 1] * (len(blocks) // 6), q)


def _yuv_case(name, group, w, h, blocks, meta=None, qbias=0):
    return Case(name, group, w, h, planes=planes_of_blocks(blocks, w, h), qbias=qbias, meta=meta)


# ------------------------------------------------------------------------------------------------ models of the one-kernel coder

def segments(w, h):
    """[(first block, blocks)] of the frame's segments in the order the waves take them (balanced split of an MCU row)"""
    mcw, mch = mcu_grid(w, h)
    nseg = (mcw + SEG_MCUS - 1) // SEG_MCUS
    per = (mcw + nseg - 1) // nseg
    out = []
    for my in range(mch):
        for i in range(nseg):
            m0 = i * per
            cnt = max(0, min(per, mcw - m0))
            out.append(((my * mcw + m0) * 6, cnt * 6))
    return out


def kernel_symbols(lines):
    """per block the symbols as the one-kernel coder numbers them: [(kind, position, bits)] with kind dc / ac / eob; the
    ZRLs in front of a coefficient belong to its symbol"""
    out = []
    for b, blk in enumerate(sb.blocks_from_coefficients(lines)):
        at = iter((np.nonzero(lines[b][1:])[0] + 1).tolist())
        syms, zrl = [], 0
        for table, sym, bits in sb.block_symbols(blk, b % 6):
            if table < 2:
                syms.append(("dc", 0, len(bits)))
            elif sym == sb.ZRL:
                zrl += len(bits)
            elif sym == sb.EOB:
                syms.append(("eob", 0, len(bits)))
            else:
                syms.append(("ac", next(at), len(bits) + zrl))
                zrl = 0
        out.append(syms)
    return out


def window_walk(round_bits):
    """the window over a frame's rounds -> {handed_back: the round that did not fit or None, wrote_before: whole bytes had
    left when it was handed back, flushes: [(round, window bits, bits carried over, final)], fits_after_flush: rounds that
    fitted only because what waited left first, windows: [(first scan byte, bytes)] of every flush}"""
    pending, done, flushes, windows, after = 0, 0, [], [], []
    for r, bits in enumerate(round_bits):
        final = r == len(round_bits) - 1
        if pending + bits > WINDOW_BITS:
            if pending >= 8:
                flushes.append((r, pending, pending & 7, False))
                windows.append((done, pending >> 3))
                done += pending >> 3
                pending &= 7
                if pending + bits <= WINDOW_BITS:
                    after.append(r)
            if pending + bits > WINDOW_BITS:
                return {"handed_back": r, "wrote_before": done > 0, "flushes": flushes, "fits_after_flush": after, "windows": windows}
        total = pending + bits
        pending = total
        if final or total > WINDOW_BITS // 2:
            nbytes = (total + 7) >> 3 if final else total >> 3
            flushes.append((r, total, 0 if final else total & 7, final))
            windows.append((done, nbytes))
            done += nbytes
            pending = 0 if final else total & 7
    return {"handed_back": None, "wrote_before": False, "flushes": flushes, "fits_after_flush": after, "windows": windows}


def frame_model(lines, w, h):
    """what a frame of these coefficients makes the one-kernel coder do -> {segments: [{symbols, per, runs: bits per lane,
    starts: where each lane's run begins}], round_bits, nbits, raw (the scan bytes before stuffing), + window_walk}"""
    syms = kernel_symbols(lines)
    segs = []
    for first, nb in segments(w, h):
        flat = [(b, p, s) for b in range(first, first + nb) for p, s in enumerate(syms[b])]
        n = len(flat)
        per = (n + 63) // 64
        runs, starts = [], []
        for lane in range(64):
            j0 = min(n, lane * per)
            j1 = min(n, j0 + per)
            runs.append(sum(s[2] for _, _, s in flat[j0:j1]))
            if j0 < j1:
                b, p, s = flat[j0]
                kinds = set()
                if p == 1:
                    kinds.add("second")
                if s[0] == "eob" and p > 1:
                    kinds.add("eob")
                if s[0] == "ac" and p > 1 and (p + 1 == len(syms[b]) or syms[b][p + 1][0] == "eob"):
                    kinds.add("last_coefficient")
                if p > 1 and syms[b][p - 1][0] == "ac" and syms[b][p - 1][1] == 31:
                    kinds.add("behind_31")
                starts.append(kinds)
        segs.append({"symbols": n, "per": per, "runs": runs, "starts": starts})
    bits = [sum(seg["runs"]) for seg in segs]
    out = {"segments": segs, "round_bits": [sum(bits[i:i + WAVES]) for i in range(0, len(bits), WAVES)], "nbits": sum(bits)}
    out.update(window_walk(out["round_bits"]))
    return out


def scan_of(chunk):
    """a chunk's scan bytes with the stuffing taken out (FF D8 and FF D9 removed)"""
    return bytes(chunk[2:-2]).replace(b"\xff\x00", b"\xff")


# ------------------------------------------------------------------------------------------------ the pool of blocks

def _pattern(line):
    return tuple((int(k), int(line[k])) for k in np.nonzero(line[1:])[0] + 1)


class Pool:
    """blocks of one or two coefficients, per table: pattern ((position, value), ...) -> samples.  Candidates are the
    clipped inverse DCT of the pattern at several gains; the key is what the oracle says they quantise to (qbias 0).
    `holding`: (run, value) -> a candidate that clipping gave up to two coefficients more than were meant but that holds
    the symbol -- taken only where no block of the exact pattern exists (the largest values of a size, mostly)."""

    PAIRS = [(a, a + r + 1) for a in (1, 2, 3, 4, 5, 6, 12, 13, 20) for r in range(16)] + [(1, r + 2) for r in range(16, 62)] + [(31, 32), (31, 63), (2, 63)]

    def __init__(self, orc):
        self.by, self.holding = [{}, {}], [{}, {}]
        for comp in (0, 1):
            q = QUANT[comp]
            lines = []
            for p in range(1, 64):
                top = int(2300 // q[p]) + 1
                for v in range(1, top):
                    for g in (0.5, 0.25, 0.75):
                        for sgn in (1, -1):
                            line = np.zeros(64)
                            line[p] = sgn * (v + g)
                            lines.append(line)
            for a, b in self.PAIRS:
                vbs = range(1, min(256, int(1500 // q[b]) + 1)) if b - a <= 16 and a != 31 else (1, 2, 3)
                for vb in vbs:
                    for sa in (1, -1):
                        for sgn in (1, -1):
                            line = np.zeros(64)
                            line[a], line[b] = sa * 1.5, sgn * (vb + 0.5)
                            lines.append(line)
            samples = samples_of(np.array(lines), comp)
            got = lines_of(orc, samples, comp)
            by = self.by[comp]
            for s, line in zip(samples, got):
                if line[0] == 0:
                    pat = _pattern(line)
                    by.setdefault(pat, s)
                    if len(pat) <= 4:                  # a few coefficients more than were meant: the symbol is there all the same
                        last = 0
                        for k, v in pat:
                            self.holding[comp].setdefault((k - last - 1, v), s)
                            last = k

    def single(self, comp, p, v):
        return self.by[comp].get(((p, v),))

    def pair(self, comp, a, b, vb):
        for va in (1, -1, 2, -2):
            s = self.by[comp].get(((a, va), (b, vb)))
            if s is not None:
                return s
        return None

    def symbol(self, comp, run, v):
        """a block that codes (run, size of v) with the value v -> samples or None"""
        s = self.single(comp, run + 1, v)
        if s is None:
            for a in (1, 2, 3):
                s = self.pair(comp, a, a + run + 1, v)
                if s is not None:
                    break
        return s if s is not None else self.holding[comp].get((run, v))


def _flat(v):
    return np.full(64, v, np.int16)


def _fill(w, h, luma, chroma, rest=0):
    """frames of w x h whose luma blocks are the list `luma` and chroma blocks the list `chroma`, in order, the rest flat"""
    nm = mcu_grid(w, h)[0] * mcu_grid(w, h)[1]
    frames = []
    while luma or chroma:
        blocks = np.full((nm * 6, 64), rest, np.int16)
        for m in range(nm):
            for k in range(6):
                src = luma if k < 4 else chroma
                if src:
                    blocks[m * 6 + k] = src.pop(0)
        frames.append(blocks)
    return frames


# ------------------------------------------------------------------------------------------------ the groups

def _symbols(orc, pool, cases):
    reach = {}
    for comp in (0, 1):
        blocks = []
        for run in range(16):
            for size in range(1, 9):
                for sgn in (1, -1):
                    lo = next((v for v in range(1 << (size - 1), 1 << size) if pool.symbol(comp, run, sgn * v) is not None), None)
                    if lo is None:
                        continue
                    hi = next(v for v in range((1 << size) - 1, lo - 1, -1) if pool.symbol(comp, run, sgn * v) is not None)
                    reach[(comp, run, size, sgn)] = (lo, hi)
                    blocks += [pool.symbol(comp, run, sgn * v) for v in sorted({lo, hi})]
        frames = _fill(*BIG, blocks if comp == 0 else [], blocks if comp else [])
        for i, f in enumerate(frames):
            cases.append(_yuv_case("symbols_%s_%d" % (("luma", "chroma")[comp], i), 1, *BIG, f))
    # DC differences: flat blocks; a flat luma block of value s has the DC s, a chroma one round(64 s / 72)
    wants = [0] + [sgn * v for size in range(1, 9) for v in sorted({1 << (size - 1), (1 << size) - 1}) for sgn in (1, -1)]
    def walk(lo, hi, steps):
        at, out = 0, []
        for d in steps:
            d = max(lo - hi, min(hi - lo, d))      # (chroma DCs span 227: its largest step is that)
            if not lo <= at + d <= hi:
                at = lo if d > 0 else hi            # (a step of its own, on the way)
                out.append(at)
            at += d
            out.append(at)
        return out

    chroma_sample = {}
    for s in range(-128, 128):
        chroma_sample.setdefault(int(np.sign(s) * ((abs(64 * s) + 36) // 72)), s)
    luma = [_flat(v) for v in walk(-128, 127, wants)]
    cb_ = [_flat(chroma_sample[v]) for v in walk(-114, 113, wants)]
    cr_ = [_flat(chroma_sample[v]) for v in walk(-114, 113, [-d for d in wants])]
    chroma = [x for pair in zip(cb_, cr_) for x in pair]
    for i, f in enumerate(_fill(*BIG, luma, chroma)):
        cases.append(_yuv_case("dc_differences_%d" % i, 1, *BIG, f, meta={"wants": wants}))
    return reach


def _dense_block(orc, rng, comp, with_63):
    """a block whose ACs 1 .. 62 are all non-zero, coefficient 63 too (no EOB) or not (an EOB at position 63)"""
    for _ in range(4000):
        line = rng.choice([-1.0, 1.0], 64) * rng.uniform(1.15, 1.9)
        line[0] = 0
        if not with_63:
            line[63] = 0
        s = samples_of(line[None], comp)
        got = lines_of(orc, s, comp)[0]
        if (got[1:63] != 0).all() and (got[63] != 0) == with_63:
            return s[0]
    raise ValueError("no block of %d non-zero ACs, table %d" % (63 if with_63 else 62, comp))


def _runs(orc, rng, pool, cases):
    luma, chroma, reach = [], [], {"runs": set(), "masks": set()}
    for comp, dst in ((0, luma), (1, chroma)):
        for p in range(17, 64):                       # a single coefficient behind 16 .. 62 zeros
            s = next(x for x in (pool.single(comp, p, v) for v in (1, -1, 2, -2)) if x is not None)
            dst.append(s)
        for a, b in ((31, 32), (31, 63), (2, 63)) + tuple((1, r + 2) for r in range(16, 62)):
            s = next((x for x in (pool.pair(comp, a, b, v) for v in (1, -1, 2, -2)) if x is not None), None)
            if s is not None:
                dst.append(s)
            reach["masks" if a != 1 else "runs"].add((comp, a, b) if s is not None else None)
        dst += [_dense_block(orc, rng, comp, True), _dense_block(orc, rng, comp, False)]
    for i, f in enumerate(_fill(*BIG, luma, chroma)):
        cases.append(_yuv_case("runs_%d" % i, 2, *BIG, f))
    return reach


def _split(orc, rng, pool, cases):
    w, h = 80, 16                                    # one segment of five MCUs: 30 blocks, 60 symbols when all are flat
    one = [pool.single(0, 1, 1), pool.single(0, 2, -1), pool.single(0, 1, -2), pool.single(0, 3, 1), pool.single(0, 5, 1)]
    for extra, name in ((0, "60_symbols"), (2, "62_symbols"), (4, "64_symbols"), (5, "65_symbols")):
        blocks = np.zeros((30, 64), np.int16)
        for i in range(extra):
            blocks[6 * i + i % 4] = one[i]
        cases.append(_yuv_case("split_" + name, 3, w, h, blocks, meta={"symbols": 60 + extra}))
    # full blocks beside empty ones: `lead` one-coefficient blocks in front move every later run one symbol on
    full = {(comp, w63): _dense_block(orc, rng, comp, w63) for comp in (0, 1) for w63 in (True, False)}
    for lead in range(4):
        blocks = np.zeros((30, 64), np.int16)
        for i in range(lead):
            blocks[i] = one[i]
        blocks[6 + 1], blocks[6 + 4] = full[(0, False)], full[(1, True)]
        blocks[18 + 2], blocks[18 + 5], blocks[24 + 3] = full[(0, True)], full[(1, False)], full[(0, False)]
        cases.append(_yuv_case("split_full_beside_empty_%d" % lead, 3, w, h, blocks))
    # runs on both sides of 256 bits: noise blocks in front of flat ones, ten MCUs to the segment
    w = 160
    best = []
    for trial in range(48):
        nbin = 4 + trial                              # saturated noise in front, plain noise behind it
        blocks = rng.integers(-128, 128, (60, 64)).astype(np.int16)
        blocks[:nbin] = rng.choice(np.array([-128, 127], np.int16), (nbin, 64))
        runs = frame_model(lines_of(orc, blocks, [0, 0, 0, 0, 1, 1] * 10), w, h)["segments"][0]["runs"]
        under, over = [r for r in runs if r <= OWN_BITS], [r for r in runs if r > OWN_BITS]
        if under and over:
            best.append((min(over) - max(under), trial, blocks, max(under), min(over)))
    best.sort(key=lambda t: t[:2])
    for gap, trial, blocks, under, over in best[:3]:
        cases.append(_yuv_case("split_scratch_%d_%d_%d" % (under, over, trial), 3, w, h, blocks, meta={"under": under, "over": over}))


def _predictor(cases):
    for w, h in (BIG, TALL):
        nm = mcu_grid(w, h)[0] * mcu_grid(w, h)[1]
        firsts = [first // 6 for first, nb in segments(w, h)]
        for name, ks in (("y0", (0,)), ("cb", (4,)), ("cr", (5,)), ("all", (0, 1, 2, 3, 4, 5))):
            blocks = np.zeros((nm * 6, 64), np.int16)
            for m in range(nm):
                blocks[m * 6: m * 6 + 6] = [[(3 * m + 5 * k) % 23 - 11] for k in range(6)]     # small steps everywhere
            for i, m in enumerate(firsts):
                for k in ks:
                    # the first MCU of every segment far from the MCU in front of it, the last MCU of every segment too
                    blocks[m * 6 + k] = 127 if i % 2 == 0 else -128
                    if m:
                        blocks[(m - 1) * 6 + (3 if k < 4 else k)] = -128 if i % 2 == 0 else 127
            cases.append(_yuv_case("predictor_%s_%dx%d" % (name, w, h), 4, w, h, blocks, meta={"blocks": ks}))


def _noise_frame(rng, amps, w=BIG[0], h=BIG[1]):
    """noise of amplitude amps[r] in the blocks of round r"""
    segs = segments(w, h)
    blocks = np.zeros((segs[-1][0] + segs[-1][1], 64), np.int16)
    for i, (first, nb) in enumerate(segs):
        a = amps[i // WAVES]
        if a >= 128:
            blocks[first: first + nb] = rng.choice(np.array([-128, 127], np.int16), (nb, 64))
        elif a:
            blocks[first: first + nb] = rng.integers(-a, a + 1, (nb, 64))
    return blocks


def _round_bits(orc, blocks, w=BIG[0], h=BIG[1]):
    return frame_model(lines_of(orc, blocks, [0, 0, 0, 0, 1, 1] * (len(blocks) // 6)), w, h)


def _window(orc, rng, cases):
    # noise amplitude -> bits per block, measured once; the amplitude for a wanted load by interpolation
    amps = (6, 10, 16, 24, 34, 48, 64, 90, 127)
    load = []
    for a in amps:
        blocks = rng.integers(-a, a + 1, (60, 64))
        load.append(frame_model(lines_of(orc, blocks, [0, 0, 0, 0, 1, 1] * 10), 160, 16)["nbits"] / 60.0)
    amp_for = lambda bits_per_block: int(round(np.interp(bits_per_block, load, amps)))
    per_round = [sum(nb for _, nb in segments(*BIG)[i:i + WAVES]) for i in range(0, 10, WAVES)]   # 132, 132, 66 blocks
    seen = {}
    for trial in range(200):                          # a non-final flush with each count of bits carried over
        blocks = _noise_frame(rng, (amp_for(25000 / per_round[0]), 8, 8))
        m = _round_bits(orc, blocks)
        early = [f for f in m["flushes"] if not f[3]]
        if m["handed_back"] is None and early and early[0][2] not in seen:
            seen[early[0][2]] = blocks
        if len(seen) == 8:
            break
    for k in sorted(seen):
        cases.append(_yuv_case("window_flush_carries_%d" % k, 5, *BIG, seen[k], meta={"carried": k}))
    # a round of saturated noise is ~320 bits a block: only a round of more than 128 blocks can miss the window, so the
    # frames handed back are 160x128 (two rounds of 240 blocks); one 176x80 frame's first round (132 blocks) just misses it
    wide = (160, 128)
    subs = (("window_last_round_handed_back", wide, (amp_for(24000 / 240), 128), "last"),
            ("window_first_round_handed_back", wide, (128, 8), "first"), ("window_first_round_just_over", BIG, (128, 8, 8), "first"),
            ("window_fits_after_flush", BIG, (amp_for(15000 / per_round[0]), amp_for(30000 / per_round[1]), 8), "after"))
    for name, (w, h), a, sub in subs:
        for i in range(2):
            cases.append(_yuv_case("%s_%d" % (name, i), 5, w, h, _noise_frame(rng, a, w, h), meta={"sub": sub}))


FF_PROPERTIES = tuple("ff_at_byte_%d" % i for i in range(4)) + ("ff_run_2", "ff_both_sides_of_byte_1024", "ff_last_whole_byte", "padding_makes_ff") + \
    tuple("tail_%d" % i for i in range(8))


def ff_properties(model, raw):
    """which of FF_PROPERTIES a frame reaches: from the scan bytes (the oracle's, unstuffed), its length in bits and the
    windows the model flushes"""
    got = set()
    tail = model["nbits"] & 7
    got.add("tail_%d" % tail)
    if tail and raw[-1] == 0xFF:
        got.add("padding_makes_ff")
    if tail and len(raw) > 1 and raw[-2] == 0xFF:
        got.add("ff_last_whole_byte")
    if b"\xff\xff" in raw:
        got.add("ff_run_2")
    if model["handed_back"] is None:
        for first, nbytes in model["windows"]:
            win = raw[first: first + nbytes]
            for i in range(4):
                if 0xFF in win[i::4]:
                    got.add("ff_at_byte_%d" % i)
            for t in range(TILE_BYTES, nbytes - 3, TILE_BYTES):
                if 0xFF in win[t - 4: t] and 0xFF in win[t: t + 4]:
                    got.add("ff_both_sides_of_byte_1024")
    return got


def longest_ff_run(raw):
    best = run = 0
    for b in raw:
        run = run + 1 if b == 0xFF else 0
        best = max(best, run)
    return best


def _ff(orc, rng, pool, cases):
    """frames of blocks that hold long codes and all-ones mantissas, kept where the oracle's scan reaches something new"""
    long_codes = [[s for pat, s in pool.by[comp].items() if len(pat) >= 1 and pat[-1][0] - (pat[-2][0] if len(pat) > 1 else 0) > 6
                   and pat[-1][1] in (1, 3, 7, 15)] for comp in (0, 1)]
    have, kept = set(), 0
    for trial in range(400):
        heavy = trial % 3 == 2
        w, h = (160, 32) if heavy else (80, 32)
        blocks = np.zeros((w // 16 * 12, 64), np.int16)
        for b in range(len(blocks)):
            comp = 0 if b % 6 < 4 else 1
            if heavy:                                  # several coefficients far apart: many 16-bit codes to the block
                line = np.zeros(64)
                at = rng.choice(np.arange(6, 64), 7, replace=False)
                line[at] = rng.choice([1.5, 3.5, -1.5, 7.5], 7)
                blocks[b] = samples_of(line[None], comp)[0]
            elif rng.random() < 0.8:
                blocks[b] = long_codes[comp][int(rng.integers(len(long_codes[comp])))]
            blocks[b] = np.clip(blocks[b] + int(rng.integers(-20, 21)), -128, 127)
        case = _yuv_case("ff_%d" % kept, 6, w, h, blocks)
        new = ff_properties(frame_model(case.lines(orc), w, h), scan_of(case.chunk(orc))) - have
        if new:
            case.meta["reaches"] = sorted(new)
            cases.append(case)
            have |= new
            kept += 1
        if len(have) == len(FF_PROPERTIES):
            break
    return have


def range_patterns():
    """[(name, 64 samples)]: per output the pattern that maximises it and the one that minimises it, then the plain ones"""
    out = []
    for n in range(64):
        up = BASIS[n] > 0
        out.append(("max_%d" % n, np.where(up, 127, -128)))
        out.append(("min_%d" % n, np.where(up, -128, 127)))
    r, c = np.indices((8, 8))
    for name, m in (("checkerboard", (r + c) & 1), ("column_stripes", c & 1), ("row_stripes", r & 1)):
        out.append((name, np.where(m.reshape(64) == 1, 127, -128)))
        out.append((name + "_inverse", np.where(m.reshape(64) == 1, -128, 127)))
    out += [("flat_127", np.full(64, 127)), ("flat_-128", np.full(64, -128))]
    return [(name, s.astype(np.int16)) for name, s in out]


def _range(cases):
    pats = [s for _, s in range_patterns()]
    nm = 55
    for f in range((len(pats) + nm - 1) // nm):
        blocks = np.zeros((nm * 6, 64), np.int16)
        for m in range(nm):
            i = f * nm + m
            blocks[m * 6: m * 6 + 4] = pats[i % len(pats)]                      # all four luma blocks of the MCU
            blocks[m * 6 + 4], blocks[m * 6 + 5] = pats[(2 * i) % len(pats)], pats[(2 * i + 1) % len(pats)]
        cases.append(_yuv_case("range_%d" % f, 7, *BIG, blocks))


def dc_ties():
    """[(comp, sum of the samples, the DC it must quantise to)]: the last sum that rounds to t and the first that rounds
    to t + 1, for t = 0, 1 and the largest, both signs"""
    out = []
    for comp, q, tops in ((0, 64, (126, -127)), (1, 72, (112, -113))):
        for sgn in (1, -1):
            for t in (0, 1, abs(tops[0 if sgn > 0 else 1])):
                out += [(comp, sgn * (q * t + q // 2 - 1), sgn * t), (comp, sgn * (q * t + q // 2), sgn * (t + 1))]
    return out


def _block_of_sum(total):
    base = total // 64 if total >= 0 else -((-total) // 64)
    s = np.full(64, base, np.int16)
    rest = total - 64 * base
    step = 1 if rest > 0 else -1
    s[[(i * 27) % 64 for i in range(abs(rest))]] += step        # (27 is odd: 64 different places)
    assert int(s.sum()) == total and s.min() >= -128 and s.max() <= 127
    return s


def ac_threshold(orc, comp, scan, qbias):
    """the first transform output (> 0) that quantises to 1 at this position -- asked of the oracle"""
    nat = int(NATURAL_OF_SCAN[scan])
    x = np.zeros((600, 64), np.int16)
    x[:, nat] = np.arange(600)
    return int(np.argmax(quantise(orc, x, comp, qbias)[:, scan] != 0))


def _aim_output(orc, rng, comp, scan, target):
    """a block whose transform output at `scan` is exactly `target`: the inverse DCT of that alone, then single pixels
    moved by +-1 (rounding to pixels moves the output in steps of about ten)"""
    nat = int(NATURAL_OF_SCAN[scan])
    s = np.clip(np.rint(target / 8.0 * BASIS[nat]), -128, 127).astype(np.int16)
    for _ in range(60):
        err = target - int(fdct(orc, s[None])[0, nat])
        if err == 0:
            return s
        gain = 8.0 * BASIS[nat]                          # what +1 on a pixel adds to the output
        moves = [(abs(d * gain[i] - err), i, d) for i in range(64) for d in (1, -1) if -128 <= s[i] + d <= 127]
        moves.sort()
        tried = []
        for _, i, d in moves[:5] + [moves[int(rng.integers(len(moves)))]]:
            t = s.copy()
            t[i] += d
            tried.append((abs(target - int(fdct(orc, t[None])[0, nat])), rng.random(), t))
        s = min(tried, key=lambda x: x[:2])[2]
    return None


def _quantiser(orc, rng, cases):
    ties = dc_ties()
    luma = [_block_of_sum(t) for comp, t, _ in ties if comp == 0]
    chroma = [_block_of_sum(t) for comp, t, _ in ties if comp == 1]
    cases.append(_yuv_case("quantiser_dc_ties", 8, 64, 32, _fill(64, 32, luma, chroma)[0]))
    met = 0
    blocks = {0: ([], []), 128: ([], [])}
    for qbias in (0, 128):
        for comp in (0, 1):
            for scan in range(1, 64):
                thr = ac_threshold(orc, comp, scan, qbias)
                for sgn in (1, -1):
                    under, on = _aim_output(orc, rng, comp, scan, sgn * (thr - 1)), _aim_output(orc, rng, comp, scan, sgn * thr)
                    met += under is not None and on is not None
                    blocks[qbias][comp].extend(b for b in (under, on) if b is not None)
    for qbias in (0, 128):
        for i, f in enumerate(_fill(*BIG, *blocks[qbias])):
            cases.append(_yuv_case("quantiser_ac_thresholds_q%d_%d" % (qbias, i), 8, *BIG, f, qbias=qbias))
    return met


RGB_GEOMETRIES = ((34, 18), (38, 30), (42, 18), (46, 30), (64, 32))     # last MCU keeps 2, 6, 10, 14; rows end 2 and 14 in


def rgb_terms(patch, bgr):
    """the sums in front of the shifts (colorspace.h:78-88) for [..., 2, 2, 3] patches -> (luma [..., 2, 2], cb, cr)"""
    p = np.asarray(patch, np.int64)
    r, g, b = (p[..., 2], p[..., 1], p[..., 0]) if bgr else (p[..., 0], p[..., 1], p[..., 2])
    r1, g1, b1 = r.sum((-1, -2)), g.sum((-1, -2)), b.sum((-1, -2))
    return 306 * r + 601 * g + 117 * b + 512, -173 * r1 - 339 * g1 + 512 * b1 + 2047, 512 * r1 - 429 * g1 - 83 * b1 + 2047


def _rgb(orc, rng, cases):
    # patches of four different pixels whose sums sit on the last value in front of a rounding step or on the first behind it
    found = {}
    for _ in range(60):
        p = rng.integers(0, 256, (20000, 2, 2, 3))
        for bgr in (False, True):
            y, u, v = rgb_terms(p, bgr)
            for key, hit in (("y_under", (y % 1024 == 1023).any((1, 2))), ("y_on", (y % 1024 == 0).any((1, 2))),
                             ("u_under", u % 4096 == 4095), ("u_on", u % 4096 == 0), ("v_under", v % 4096 == 4095), ("v_on", v % 4096 == 0)):
                have = found.setdefault((key, bgr), [])
                if len(have) < 6:
                    have.extend(p[hit][: 6 - len(have)])
        if all(len(v) >= 6 for v in found.values()) and len(found) == 12:
            break
    edges = [np.array(c, np.int64) for c in np.ndindex(2, 2, 2)]
    patches = [q for v in found.values() for q in v]
    patches += [np.broadcast_to(e * 255, (2, 2, 3)) for e in edges]               # 0 and 255 in every channel, flat
    patches += [np.array([[edges[i] * 255, edges[(i + 3) % 8] * 255], [edges[(i + 5) % 8] * 255, edges[(i + 6) % 8] * 255]]) for i in range(8)]
    for w, h in RGB_GEOMETRIES:
        grid = np.zeros((h, w, 3), np.uint8)
        order = rng.permutation(len(patches) * ((h // 2) * (w // 2) // len(patches) + 1))
        for i, (r, c) in enumerate(np.ndindex(h // 2, w // 2)):
            grid[2 * r: 2 * r + 2, 2 * c: 2 * c + 2] = patches[order[i] % len(patches)]
        # every row and column unlike its neighbours: a wrong replication at the right or lower edge shows
        r, c = np.indices((h, w))
        loud = np.stack([(r * 37 + c * 91) % 256, (r * 113 + c * 29 + 128 * (r & 1)) % 256, (r * 59 + c * 151 + 128 * (c & 1)) % 256], -1).astype(np.uint8)
        for name, pix in (("patches", grid), ("loud", loud)):
            for kind in ("rgb", "bgr"):
                cases.append(Case("rgb_%s_%s_%dx%d" % (name, kind, w, h), 9, w, h, planes=to_planes(orc, pix, w, h, kind == "bgr"), pix=pix, kind=kind,
                                  qbias=128 if name == "loud" else 0))
    return found


_CORPUS = {}


def corpus(orc, seed=0x91C5):
    """-> (cases, reach): reach holds what the searches found, for test_pixel_builder's floors.  Built once per process."""
    if seed in _CORPUS:
        return _CORPUS[seed]
    rng = np.random.default_rng(seed)
    pool = Pool(orc)
    cases, reach = [], {}
    reach["symbols"] = _symbols(orc, pool, cases)
    reach["runs"] = _runs(orc, rng, pool, cases)
    _split(orc, rng, pool, cases)
    _predictor(cases)
    _window(orc, rng, cases)
    reach["ff"] = _ff(orc, rng, pool, cases)
    _range(cases)
    reach["ac_thresholds_met"] = _quantiser(orc, rng, cases)
    reach["rgb"] = _rgb(orc, rng, cases)
    assert len({c.name for c in cases}) == len(cases)
    _CORPUS[seed] = (cases, reach)
    return cases, reach


def batches(orc, cases):
    """per geometry and kind: the cases, each between two ordinary synth_frame frames -> [{w, h, kind, cases, where (their
    places in the batch), n, planes: (Y [n, h, ys], Cb, Cr [n, h / 2, cs]) with rows padded by POISON, ys, cs, and for rgb /
    bgr pix [n, h, stride] padded the same way, stride; frames: a Case per frame, the ordinary ones included}]"""
    by = {}
    for c in cases:
        by.setdefault((c.w, c.h, c.kind), []).append(c)
    out = []
    for (w, h, kind), cs in by.items():
        t = [0]

        def ordinary():
            pix = orc.synth_frame(SEED, 7 * t[0] + w, w, h)
            t[0] += 1
            if kind == "bgr":
                pix = np.ascontiguousarray(pix[..., ::-1])
            planes = to_planes(orc, pix, w, h, kind == "bgr")
            return Case("ordinary frame #%d" % (2 * (t[0] - 1)), 0, w, h, planes=planes, pix=None if kind == "yuv" else pix, kind=kind)

        frames, where = [ordinary()], []
        for c in cs:
            where.append(len(frames))
            frames += [c, ordinary()]
        n, ys, cs_ = len(frames), w + 24, w // 2 + 8
        Y, Cb, Cr = np.full((n, h, ys), POISON, np.uint8), np.full((n, h // 2, cs_), POISON, np.uint8), np.full((n, h // 2, cs_), POISON, np.uint8)
        for i, f in enumerate(frames):
            Y[i, :, :w], Cb[i, :, : w // 2], Cr[i, :, : w // 2] = f.planes
        b = {"w": w, "h": h, "kind": kind, "cases": cs, "where": where, "n": n, "frames": frames, "planes": (Y, Cb, Cr), "ys": ys, "cs": cs_}
        if kind != "yuv":
            b["stride"] = w * 3 + 7
            b["pix"] = np.full((n, h, b["stride"]), POISON, np.uint8)
            for i, f in enumerate(frames):
                b["pix"][i, :, : w * 3] = f.pix.reshape(h, w * 3)
        out.append(b)
    return out
