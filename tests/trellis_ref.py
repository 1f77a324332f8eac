"""The video encoder's trellis quantiser restated in Python (a helper of the tests, imported as nr_ref and scan_builder are).

    dct_quantize_trellis_c   libavcodec/mpegvideo_enc.c:2961-3247   per 8x8 block, the levels of least distortion + lambda * bits

One walk (`walk`: the survivors, the candidates in order, strict comparison, the pruning rule of :3163-3173, the search for
the end, the way back) serves two modes, which differ in what they feed it:

    product mode     what the product codes (amv_trellis_plan.h): this encoder's fdct outputs (samples - 128) in scan order,
                     AMV's fixed steps Q[i], qmat = (1 << 22) / (8 Q), bias = qbias << 14, the reconstruction every AMV
                     decoder applies (level * Q, so level * Q * 8 in the fdct's scale), the rate of AMV's fixed AC code
                     itself -- ZRLs, run/size code, magnitude bits, no escape -- and an end-of-block term that is the EOB
                     code's length where one is written (none behind position 63).  The DC is amvo_quantize_block's.
    reference mode   dct_quantize_trellis_c as it is, fed as tests/golden/make_ref_trellis_golden.py feeds the real one:
                     un-shifted samples, the MPEG-1 intra matrix at a qscale, bias 0, MPEG-1's reconstruction
                     ((a * qscale * M[j] >> 3) - 1 | 1) << 3, a caller's length[UNI_AC_ENC_INDEX(run, level + 64)] table
                     with esc_length beyond +-64, the flat 2 * lambda at the end.  (The FMT_H263 branches and the
                     FMT_MPEG1 bias are not reached by the amv encoder's setting and are left out.)

Python ints do not wrap: the model is the C code wherever its int arithmetic does not wrap, which is what the product's
bound on lambda guarantees (amv_trellis_plan.h).
"""
import numpy as np

import coef_builder as cb
import nr_ref as N
import scan_builder as sb
from nr_ref import orc

NO_SCORE = 256 * 256 * 256 * 120
QMAT_SHIFT = 22
LAST_NARROW = 27
QUANT = cb.QUANT                       # (luma, chroma) steps in scan order
ZIGZAG = N.ZIGZAG                      # scan position -> row-major index
# amv_trellis_plan.h's bound: 63 * ((8 * 61 + 2)^2 + 59 * lambda) stays below NO_SCORE
LAMBDA_MAX = ((NO_SCORE - 1) // 63 - (8 * 61 + 2) ** 2) // 59


def lambda_of_qscale(qscale):
    """lambda = qscale * FF_QP2LAMBDA, lambda2 = (lambda^2 + 64) >> 7 (:144-147); the trellis takes lambda2 >> 1 (:2985)"""
    lam = qscale * 118
    return ((lam * lam + 64) >> 7) >> 1


_LEN = {}


def ac_lengths(comp):
    """len[symbol] of the AC code of class comp (0 luma, 1 chroma): the oracle's amvo_huffman_codes(2 + comp)"""
    if comp not in _LEN:
        _LEN[comp] = [int(x) for x in orc.huffman_codes(2 + comp)[0]]
    return _LEN[comp]


def nbits(a):
    return int(a).bit_length()


def product_bits(length, run, a):
    return (run >> 4) * length[0xF0] + length[((run & 15) << 4) | nbits(a)] + nbits(a)


# ---- the walk both modes share -----------------------------------------------------------------------------------------------

def walk(last, cands, rate, lam, end_term, narrow_rule=True, newest_first=True, strict=True, trace=None):
    """cands[i] (i = 1 .. last) = [(level, distortion), ...] in the order they are tried; rate(run, level) -> bits;
    end_term(i) -> what ending with position i - 1 as the last coded one adds.  -> {position: level} of the path.
    narrow_rule=False prunes by `> best + lambda` whatever `last` is, newest_first=False walks the survivors oldest first,
    strict=False lets an equal score win: the three variants the fixture's maker tells apart.
    trace: a dict that receives steps (inner steps taken) and survivors (the longest list)"""
    better = (lambda s, best: s < best) if strict else (lambda s, best: s <= best)
    score = {1: 0}
    survivors = [1]
    run_tab, level_tab = {}, {}
    steps = longest = 0
    for i in range(1, last + 1):
        best = NO_SCORE
        for level, d in cands[i]:
            for frm in (reversed(survivors) if newest_first else survivors):
                run = i - frm
                s = d + rate(run, level) * lam + score[frm]
                steps += 1
                if better(s, best):
                    best, run_tab[i + 1], level_tab[i + 1] = s, run, level
        score[i + 1] = best
        slack = 0 if (narrow_rule and last <= LAST_NARROW) else lam
        while survivors and score[survivors[-1]] > best + slack:
            survivors.pop()
        survivors.append(i + 1)
        longest = max(longest, len(survivors))
    best, end = NO_SCORE, 1
    for i in range(survivors[0], last + 2):
        s = score[i] + end_term(i)
        if better(s, best):
            best, end = s, i
    if trace is not None:
        trace["steps"], trace["survivors"] = steps, longest
    out = {}
    i = end
    while i > 1:
        out[i - 1] = level_tab[i]
        i -= run_tab[i] + 1
    return out


def _candidates(c, qmat, bias, dist):
    """-> (last, cands): steps 1 and 2 of the text over c[1 .. 63] (scan order); dist(i, |level|) -> distortion"""
    t1 = (1 << QMAT_SHIFT) - bias - 1
    L = [int(c[i]) * int(qmat[i]) for i in range(64)]
    last = max([i for i in range(1, 64) if abs(L[i]) > t1], default=0)
    cands = {}
    for i in range(1, last + 1):
        sign = -1 if L[i] < 0 else 1
        if abs(L[i]) > t1:
            a = (abs(L[i]) + bias) >> QMAT_SHIFT
            levels = [a, a - 1] if a >= 2 else [a]
        else:
            levels = [1]
        cands[i] = [(sign * a, dist(i, a)) for a in levels]
    return last, cands


# ---- product mode ------------------------------------------------------------------------------------------------------------

def product_distortion(c, a, q):
    return (a * q * 8 - abs(c)) ** 2 - c * c


def trellis_block(c, comp, qbias, lam, trace=None, **variant):
    """c: the block's fdct outputs in scan order (position 0 is not looked at) -> the 63 AC levels, scan order, as a list of
    64 with position 0 = 0"""
    q, length = QUANT[comp], ac_lengths(comp)
    qmat = [(1 << QMAT_SHIFT) // (8 * int(q[i])) for i in range(64)]
    last, cands = _candidates(c, qmat, qbias << 14, lambda i, a: product_distortion(int(c[i]), a, int(q[i])))
    out = [0] * 64
    if trace is not None:
        trace["last"], trace["steps"], trace["survivors"] = last, 0, 0
    if last:
        path = walk(last, cands, lambda run, level: product_bits(length, run, abs(level)), lam,
                    lambda i: length[0x00] * lam if i - 1 < 63 else 0, trace=trace, **variant)
        for p, v in path.items():
            out[p] = v
    return out


def block_cost(c, levels, comp, lam):
    """distortion + lambda * bits of the AC levels (scan order) of one block as the text defines them, the EOB included"""
    q, length = QUANT[comp], ac_lengths(comp)
    total, prev = 0, 0
    for i in range(1, 64):
        if levels[i]:
            total += product_distortion(int(c[i]), abs(int(levels[i])), int(q[i])) + product_bits(length, i - prev - 1, abs(int(levels[i]))) * lam
            prev = i
    return total + (length[0x00] * lam if prev < 63 else 0)


def quantize_trellis(coef, qbias, lam, **variant):
    """[B, 64] fdct outputs (row-major, MCU order: Y0 Y1 Y2 Y3 Cb Cr) -> zig-zag lines: the DC amvo_quantize_block's, the AC
    levels the walk's"""
    coef = np.asarray(coef, np.int64)
    zz = N.quantize_product(coef, qbias).astype(np.int64)
    for b in range(coef.shape[0]):
        zz[b, 1:] = trellis_block(coef[b][ZIGZAG], 0 if b % 6 < 4 else 1, qbias, lam, **variant)[1:]
    return zz.astype(np.int16)


def frame_coefficients(y, cb_, cr, w, h):
    return N.fdct(N.frame_blocks(y, cb_, cr, w, h, 128))


def encode_frames(frames, w, h, qbias, lam, want_coef=False):
    """frames: [(y, cb, cr)] -> the chunks (or the zig-zag lines per frame) of the trellis entries"""
    out = []
    for y, cb_, cr in frames:
        zz = quantize_trellis(frame_coefficients(y, cb_, cr, w, h), qbias, lam)
        out.append(zz if want_coef else N._chunk(zz))
    return out


def encode_frames_plain(frames, w, h, qbias, want_coef=False):
    out = []
    for y, cb_, cr in frames:
        zz = N.quantize_product(frame_coefficients(y, cb_, cr, w, h), qbias)
        out.append(zz if want_coef else N._chunk(zz))
    return out


# ---- reference mode ----------------------------------------------------------------------------------------------------------

def uni_ac_enc_index(run, level):
    return run * 128 + level


def reference_qmat(qscale):
    """convert_matrix for ff_jpeg_fdct_islow (mpegvideo_enc.c:80-91): (1 << 22) / (qscale * M[j]), row-major"""
    return (1 << QMAT_SHIFT) // (qscale * N.MPEG1_INTRA)


def trellis_block_reference(block, qscale, lam, length, esc_length, **variant):
    """block: 64 fdct outputs of un-shifted samples, row-major (the fdct done) -> (64 levels row-major, last_non_zero) as
    dct_quantize_trellis_c leaves them with mb_intra = 1, y_dc_scale = 8, n < 4, out_format FMT_MJPEG"""
    block = [int(x) for x in block]
    M = [int(x) for x in N.MPEG1_INTRA]
    qm = reference_qmat(qscale)
    c = [block[ZIGZAG[i]] for i in range(64)]
    qmat = [int(qm[ZIGZAG[i]]) for i in range(64)]

    def dist(i, a):
        u = (((a * qscale * M[ZIGZAG[i]]) >> 3) - 1 | 1) << 3
        return (u - abs(c[i])) ** 2 - c[i] * c[i]

    last, cands = _candidates(c, qmat, 0, dist)
    out = [0] * 64
    out[0] = (block[0] + 32) // 64                     # q = y_dc_scale << 3; block[0] is not negative
    if not last:
        return out, 0

    def rate(run, level):
        return length[uni_ac_enc_index(run, level + 64)] if 0 <= level + 64 < 128 else esc_length

    # (the escape's length is added to the distortion in the reference, :3133; the sum is the same)
    path = walk(last, cands, rate, lam, lambda i: 2 * lam if i else 0, **variant)
    for p, v in path.items():
        out[ZIGZAG[p]] = v
    return out, max(path) if path else 0


def jpeg_uni_ac_lengths(comp=0):
    """the table later FFmpeg gave mjpegenc (ff_init_uni_ac_vlc): length[UNI_AC_ENC_INDEX(run, level + 64)] = the AC code of
    (run, nbits) + nbits for runs of 0 .. 15 (longer runs are not in it: a large length keeps the walk off them), and the
    escape length for what the table does not hold.  What the fixture's maker hands the real function."""
    length = ac_lengths(comp)
    table = [0] * (64 * 128)
    for run in range(64):
        for level in range(-64, 64):
            a = abs(level)
            if a == 0:
                continue
            if run < 16:
                table[uni_ac_enc_index(run, level + 64)] = length[(run << 4) | nbits(a)] + nbits(a)
            else:
                table[uni_ac_enc_index(run, level + 64)] = min(255, (run >> 4) * length[0xF0] + length[((run & 15) << 4) | nbits(a)] + nbits(a))
    return table, 16 + 10


def reference_samples(rng, kind):
    """one seeded 8x8 block of un-shifted samples (64, row-major) for the reference-mode fixture: "noise" full range, "ramp"
    a gradient + noise of +-12, "texture" a 2x2-coarse pattern + noise of +-20, "sparse" a few cosines (long zero runs under
    a high last position)"""
    yy, xx = np.mgrid[:8, :8]
    if kind == "noise":
        s = rng.integers(0, 256, (8, 8))
    elif kind == "ramp":
        s = (xx * int(rng.integers(1, 9)) + yy * int(rng.integers(1, 9)) + int(rng.integers(0, 128))) % 256 + rng.integers(-12, 13, (8, 8))
    elif kind == "texture":
        s = np.kron(rng.integers(0, 256, (4, 4)), np.ones((2, 2), np.int64)) + rng.integers(-20, 21, (8, 8))
    else:
        s = np.full((8, 8), 128.0)
        for _ in range(int(rng.integers(2, 6))):
            u, v = int(rng.integers(0, 8)), int(rng.integers(0, 8))
            s = s + float(rng.integers(8, 60)) * np.cos((2 * xx + 1) * u * np.pi / 16) * np.cos((2 * yy + 1) * v * np.pi / 16)
        s = np.rint(s) + rng.integers(-2, 3, (8, 8))
    return np.clip(s, 0, 255).astype(np.int64).reshape(64)
