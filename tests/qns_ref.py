"""The video encoder's quantizer noise shaping (`-qns`) restated in Python (a helper of the tests, imported as trellis_ref is).

    get_vissual_weight    libavcodec/mpegvideo_enc.c:1434-1455   a visual weight per sample from the local variance
    dct_quantize_refine   libavcodec/mpegvideo_enc.c:3271-3645   per 8x8 block, greedy +-1 changes of the levels, each the one
                                                                 that lowers weighted pixel error + lambda * bits the most

One walk (`walk`: the candidates in order, the three -qns gates, the gradient rule, strict comparison, the remainder's
update) serves two modes, which differ in what they feed it:

    product mode     what the product codes (amv_qns_plan.h): levels in scan order behind any of the encoder's quantisers,
                     the reconstruction every AMV decoder applies (level * Q, for the DC too), samples - 128, the rate of
                     AMV's fixed AC code itself (ZRLs, run/size code, magnitude bits, the EOB unless position 63 is coded).
    reference mode   dct_quantize_refine as it is, fed as tests/golden/make_ref_qns_golden.py feeds the real one: un-shifted
                     samples, dct_quantize_c's levels of the MPEG-1 intra matrix at a qscale, the H.263 reconstruction
                     qmul * level +- qadd with qmul = 2 qscale, qadd = (qscale - 1) | 1, q = 8 << 3 for the DC, a caller's
                     length / last_length tables by UNI_AC_ENC_INDEX.

An iteration's candidates (up to 128, 64 samples each) are scored as one numpy expression.  rem is the int16 the reference
keeps and the score's sum is unsigned 32-bit; the model asserts on every block that neither wraps and that |b| <= 512 (the
range the reference asserts, dsputil.c:3121), which is what amv_qns_plan.h's bounds state.
"""
import numpy as np

import nr_ref as N
import trellis_ref as T

ZIGZAG = [int(x) for x in N.ZIGZAG]      # scan position -> row-major index
QUANT = T.QUANT
RECON_SHIFT = 6
ITERATIONS = 512                         # amv_qns_plan.h: kQnsIterations
CHANGES_SEEN = 90                        # ... and kQnsChangesSeen, what the cap was measured from
BITS_MOST = 3 * 59
LAMBDA_MOST = (0x7FFFFFFF - (1 << 30)) // BITS_MOST
SUM_W2_MOST = 64 * 63 * 63
LAMBDA2_MAX = (((LAMBDA_MOST + 1) << 19) - 1) // SUM_W2_MOST

DEFAULTS = dict(strict=True, minus_first=True, gate_after_last=True, gate_grow=True, gate_gradient=True, gradient=True,
                round_basis=True, shift_b=True, weight_half=True, lambda_shift=19)
# the rules the fixture's maker tells apart, each with a model WITHOUT the rule
VARIANTS = (("strict", {"strict": False}), ("order", {"minus_first": False}), ("gate_after_last", {"gate_after_last": False}),
            ("gate_grow", {"gate_grow": False}), ("gate_gradient", {"gate_gradient": False}), ("gradient", {"gradient": False}),
            ("round_basis", {"round_basis": False}), ("shift_b", {"shift_b": False}), ("weight", {"weight_half": False}),
            ("lambda_shift", {"lambda_shift": 18}))


def lambda2_of_qscale(qscale):
    """lambda = qscale * FF_QP2LAMBDA, lambda2 = (lambda^2 + 64) >> 7 (:144-147): 6962 at 8"""
    lam = qscale * 118
    return (lam * lam + 64) >> 7


def _basis():
    """build_basis (:3252-3269) with the identity permutation: [8 i + j][8 x + y] int16"""
    b = np.zeros((64, 64), np.int64)
    for i in range(8):
        for j in range(8):
            s = 0.25 * (1 << 16)
            if i == 0:
                s *= np.sqrt(0.5)
            if j == 0:
                s *= np.sqrt(0.5)
            for x in range(8):
                for y in range(8):
                    v = s * np.cos((np.pi / 8.0) * i * (x + 0.5)) * np.cos((np.pi / 8.0) * j * (y + 0.5))
                    b[8 * i + j][8 * x + y] = int(np.rint(np.float32(v)))
    return b


BASIS = _basis()
BASIS_SCAN = BASIS[ZIGZAG]               # [scan position][sample]


def basis_hash():
    return "%016x" % N.fnv1a64(BASIS.astype("<i2").tobytes())


def _s16(x):
    return ((x + 32768) & 0xFFFF) - 32768


def visual_weight(samples):
    """get_vissual_weight over 64 samples (row-major) -> w0[x + 8 y]; ff_sqrt (libavutil/internal.h:183-199) is the floor
    square root"""
    s = np.asarray(samples, np.int64).reshape(8, 8)
    out = np.zeros(64, np.int64)
    for y in range(8):
        for x in range(8):
            n = s[max(y - 1, 0):min(8, y + 2), max(x - 1, 0):min(8, x + 2)]
            count, total, sqr = n.size, int(n.sum()), int((n * n).sum())
            v = count * sqr - total * total
            r = int(np.floor(np.sqrt(v)))
            while r * r > v:
                r -= 1
            while (r + 1) * (r + 1) <= v:
                r += 1
            out[x + 8 * y] = (36 * r) // count
    return out


def shaped_weight(w0, weight_half=True):
    """:3345-3359 -> (w[64] in 16 .. 63, the sum of w^2)"""
    w1 = np.abs(w0) + 4 * 36
    w = 15 + (48 * 4 * 36 + (w1 // 2 if weight_half else 0)) // w1
    assert w.min() >= 16 and w.max() <= 63
    return w, int((w * w).sum())


def try_scores(rem, w, rows, scales, round_basis=True, shift_b=True):
    """try_8x8basis for a list of candidates: rows [C, 64] of the basis, scales [C] -> scores [C] (Python ints)"""
    step = (rows * np.asarray(scales, np.int64)[:, None] + (512 if round_basis else 0)) >> 10
    b = rem[None, :] + step
    b = (b >> RECON_SHIFT) if shift_b else ((b + 32) >> RECON_SHIFT)
    assert np.abs(b).max() <= 512, "b = %d leaves the range the reference asserts" % np.abs(b).max()
    wb = w[None, :] * b
    total = ((wb * wb) >> 4).sum(axis=1)
    assert total.max() < (1 << 32), "the unsigned sum wraps"
    return [int(x) >> 2 for x in total]


def add_basis(rem, row, scale, round_basis=True):
    out = rem + ((row * scale + (512 if round_basis else 0)) >> 10)
    assert np.abs(out).max() < 32768, "rem leaves int16"
    return out


def gradient(rem, w):
    """d1 of :3404-3413: ff_jpeg_fdct_islow of (rem w^2 + 2^17) >> 18, row-major"""
    return N.fdct(((rem * w * w + (1 << 17)) >> 18)[None])[0]


# ---- the walk both modes share -----------------------------------------------------------------------------------------------

def walk(mode, levels, rem, w, lam, qns, cap=ITERATIONS, trace=None, **variant):
    """levels: 64 ints in scan order, changed in place; rem, w: int64 [64]; mode: dc_ok(new), dc_scale(change),
    ac_ok(i, new), ac_scale(i, level, new), rate(levels, last, i, level, new, prevs, nexts) -> bits, with prevs[i] / nexts[i]
    the non-zero AC position before / behind i (0: none).  -> the changes made"""
    v = dict(DEFAULTS, **variant)
    order = (-1, 1) if v["minus_first"] else (1, -1)
    changes = 0
    while changes < cap:
        nz = [i for i in range(1, 64) if levels[i]]
        last = nz[-1] if nz else 0
        analyze = v["gradient"] and (last > 2 or qns >= 3 or not v["gate_gradient"])
        d1 = gradient(rem, w) if analyze else None
        prevs, nexts, at = [0] * 64, [0] * 64, 0
        for i in range(1, 64):
            prevs[i] = at
            at = i if levels[i] else at
        at = 0
        for i in range(63, 0, -1):
            nexts[i] = at
            at = i if levels[i] else at
        cands = []
        for change in order:
            if mode.dc_ok(levels[0] + change):
                cands.append((0, change, mode.dc_scale(change), 0))
        for i in range(1, 64):
            if v["gate_after_last"] and qns < 3 and i > last + 1:
                break
            level = levels[i]
            for change in order:
                new = level + change
                if v["gate_grow"] and qns < 2 and abs(new) > abs(level):
                    continue
                if new:
                    if not mode.ac_ok(i, new):
                        continue
                    if not level and analyze:
                        g = int(d1[ZIGZAG[i]])
                        if g and (g < 0) == (new < 0):
                            continue
                cands.append((i, change, mode.ac_scale(i, level, new), mode.rate(levels, last, i, level, new, prevs, nexts)))
        base = try_scores(rem, w, BASIS_SCAN[:1], [0], v["round_basis"], v["shift_b"])[0]
        if not cands:
            break
        tries = try_scores(rem, w, BASIS_SCAN[[c[0] for c in cands]], [c[2] for c in cands], v["round_basis"], v["shift_b"])
        scores = [c[3] * lam + t for c, t in zip(cands, tries)]
        assert -(1 << 31) <= min(scores) and max(scores) < (1 << 31), "a score leaves int32"
        best, pick = base, None
        for c, s in zip(cands, scores):
            if s < best or (not v["strict"] and s == best):
                best, pick = s, c
        if pick is None:
            break
        tied = scores.count(best) - 1
        if trace is not None:                    # (position, change, last_non_zero then, the level before, candidates tied with the
            #                                        winner, best_score before, the winner's score, its bits)
            trace.setdefault("picks", []).append((pick[0], pick[1], last, levels[pick[0]], tied, base, best, pick[3]))
        levels[pick[0]] += pick[1]
        rem = add_basis(rem, BASIS_SCAN[pick[0]], pick[2], v["round_basis"])
        changes += 1
    if trace is not None:
        trace["changes"], trace["rem"] = changes, rem
    return changes


# ---- product mode ------------------------------------------------------------------------------------------------------------

def local_bits(length, i, prev, nxt, a_next, a):
    """amv_qns_plan.h: qns_local_bits"""
    frm = i if a else prev
    bits = T.product_bits(length, i - prev - 1, a) if a else 0
    return bits + (T.product_bits(length, nxt - frm - 1, a_next) if nxt else (length[0x00] if frm < 63 else 0))


class _Product:
    def __init__(self, comp):
        self.q = [int(x) for x in QUANT[comp]]
        self.length = T.ac_lengths(comp)

    def dc_ok(self, new):
        return 0 <= new * self.q[0] + 1024 < 2048

    def dc_scale(self, change):
        return change * self.q[0]

    def ac_ok(self, i, new):
        return abs(new * self.q[i]) < 2048

    def ac_scale(self, i, level, new):
        return (new - level) * self.q[i]

    def rate(self, levels, last, i, level, new, prevs, nexts):
        prev, nxt = prevs[i], nexts[i]
        a_next = abs(levels[nxt]) if nxt else 0
        return local_bits(self.length, i, prev, nxt, a_next, abs(new)) - local_bits(self.length, i, prev, nxt, a_next, abs(level))


def ac_bits(levels, comp):
    """the length of what the packer writes for a block's AC part"""
    length, prev, total = T.ac_lengths(comp), 0, 0
    for i in range(1, 64):
        if levels[i]:
            total += T.product_bits(length, i - prev - 1, abs(int(levels[i])))
            prev = i
    return total + (length[0x00] if prev < 63 else 0)


def qns_block(p, levels, comp, qns, lambda2, cap=ITERATIONS, trace=None, **variant):
    """p: 64 samples 0 .. 255 row-major; levels: 64 in scan order (the DC absolute) -> (refined levels as a list, changes)"""
    v = dict(DEFAULTS, **variant)
    p = np.asarray(p, np.int64).reshape(64)
    levels = [int(x) for x in levels]
    q = QUANT[comp]
    w, sum_w2 = shaped_weight(visual_weight(p), v["weight_half"])
    lam = (sum_w2 * lambda2) >> v["lambda_shift"]
    rem = levels[0] * int(q[0]) * 8 + 32 - ((p - 128) << RECON_SHIFT)
    for i in range(1, 64):
        if levels[i]:
            rem = add_basis(rem, BASIS_SCAN[i], levels[i] * int(q[i]), v["round_basis"])
    changes = walk(_Product(comp), levels, rem, w, lam, qns, cap, trace, **variant)
    return levels, changes


_MOST = {"changes": 0}


def refine_lines(frames, w, h, lines, qns, lambda2, cap=ITERATIONS):
    """frames: [(y, cb, cr)], lines: per frame the zig-zag lines [blocks, 64] a quantiser left -> the refined lines.  qns 0:
    the lines as they are.  The most changes any block took is kept in most_changes()."""
    if not qns:
        return [np.array(zz, np.int16) for zz in lines]
    out = []
    for (y, cb_, cr), zz in zip(frames, lines):
        p = N.frame_blocks(y, cb_, cr, w, h, 0)
        new = np.array(zz, np.int16)
        for b in range(p.shape[0]):
            lv, changes = qns_block(p[b], zz[b], 0 if b % 6 < 4 else 1, qns, lambda2, cap)
            assert cap != ITERATIONS or changes < ITERATIONS, "a block reached the cap"
            _MOST["changes"] = max(_MOST["changes"], changes)
            new[b] = lv
        out.append(new)
    return out


def most_changes():
    return _MOST["changes"]


def seeded_changes(first, count, seed=20261):
    """the measurement behind the cap (amv_qns_plan.h: kQnsChangesSeen): blocks first .. first + count of a series of seeded
    blocks of reference_samples' four kinds in turn, luma and chroma in turn, behind the plain quantiser, refined at qns 3 and
    lambda2 0 -> the most changes one of them took.  `python tests/qns_ref.py` runs 20 000 of them."""
    kinds = ("ramp", "texture", "noise", "sparse")
    most = 0
    for b in range(first, first + count):
        rng = np.random.default_rng([seed, b])
        p = T.reference_samples(rng, kinds[b % 4])
        comp = (b >> 2) & 1
        zz = N.quantize_product(N.fdct((p - 128)[None]), 0)[0] if comp == 0 else None
        if zz is None:                                 # (quantize_product takes the class from the block's place in an MCU)
            zz = N.quantize_product(np.repeat(N.fdct((p - 128)[None]), 5, axis=0), 0)[4]
        most = max(most, qns_block(p, zz, comp, 3, 0)[1])
    return most


# ---- reference mode ----------------------------------------------------------------------------------------------------------

def quantize_reference(block, qscale):
    """dct_quantize_c (:3647-3724) with mb_intra, y_dc_scale 8, bias 0 over 64 fdct outputs of un-shifted samples, row-major
    -> (levels row-major, last_non_zero)"""
    block = [int(x) for x in block]
    qm = T.reference_qmat(qscale)
    out = [0] * 64
    out[0] = (block[0] + 32) // 64
    last = 0
    for i in range(1, 64):
        j = ZIGZAG[i]
        level = block[j] * int(qm[j])
        if abs(level) > (1 << 22) - 1:
            a = abs(level) >> 22
            out[j] = a if level > 0 else -a
            last = i
    return out, last


class _Reference:
    def __init__(self, qscale, length, last_length):
        self.qmul, self.qadd, self.q = 2 * qscale, (qscale - 1) | 1, 8 << 3
        self.length, self.last_length = length, last_length

    def coeff(self, level):
        return 0 if not level else self.qmul * level + (self.qadd if level > 0 else -self.qadd)

    def dc_ok(self, new):
        return 0 <= self.q * new < 2048

    def dc_scale(self, change):
        return self.q * change

    def ac_ok(self, i, new):
        return -2048 < self.coeff(new) < 2048

    def ac_scale(self, i, level, new):
        return self.coeff(new) - self.coeff(level)

    def rate(self, levels, last, i, level, new, prevs, nexts):
        L, LL = self.length, self.last_length
        idx = T.uni_ac_enc_index
        prev = prevs[i]
        run = i - prev - 1
        prev_level = 0
        if prev:
            prev_level = levels[prev] + 64
            if prev_level & ~127:
                prev_level = 0
            prev_run = prev - prevs[prev] - 1
        if i < last:
            next_i = nexts[i]
            run2 = next_i - i - 1
            next_level = levels[next_i] + 64
            if next_level & ~127:
                next_level = 0
            tail = L if next_i < last else LL
        if new and level:
            if -63 < level < 63:
                t = L if i < last else LL
                return t[idx(run, new + 64)] - t[idx(run, level + 64)]
            return 0
        sign = 1 if new else -1                      # a zero becomes +-1, or +-1 becomes zero: the same terms, mirrored
        if i < last:
            return sign * (L[idx(run, 65)] + tail[idx(run2, next_level)] - tail[idx(run + run2 + 1, next_level)])
        s = LL[idx(run, 65)]
        if prev_level:
            s += L[idx(prev_run, prev_level)] - LL[idx(prev_run, prev_level)]
        return sign * s


def refine_block_reference(samples, qscale, lambda2, qns, length, last_length, **variant):
    """samples: 64 un-shifted samples (row-major) -> (64 levels row-major, last_non_zero) as dct_quantize_c followed by
    dct_quantize_refine leave them with mb_intra = 1, y_dc_scale = 8, n = 0"""
    v = dict(DEFAULTS, **variant)
    samples = np.asarray(samples, np.int64).reshape(64)
    block, _ = quantize_reference(N.fdct(samples[None])[0], qscale)
    levels = [block[ZIGZAG[i]] for i in range(64)]
    mode = _Reference(qscale, length, last_length)
    w, sum_w2 = shaped_weight(visual_weight(samples), v["weight_half"])
    lam = (sum_w2 * lambda2) >> v["lambda_shift"]
    rem = levels[0] * mode.q + 32 - (samples << RECON_SHIFT)
    for i in range(1, 64):
        if levels[i]:
            rem = add_basis(rem, BASIS_SCAN[i], mode.coeff(levels[i]), v["round_basis"])
    walk(mode, levels, rem, w, lam, qns, 1 << 30, **variant)
    out = [0] * 64
    for i in range(64):
        out[ZIGZAG[i]] = levels[i]
    return out, max([i for i in range(1, 64) if levels[i]], default=0)


if __name__ == "__main__":
    import concurrent.futures
    import sys

    total, parts = (int(sys.argv[1]) if len(sys.argv) > 1 else 20000), 16
    step = (total + parts - 1) // parts
    with concurrent.futures.ProcessPoolExecutor(parts) as ex:
        seen = list(ex.map(seeded_changes, range(0, total, step), [min(step, total - at) for at in range(0, total, step)]))
    print("the most changes one of %d seeded blocks took at qns 3, lambda2 0: %d" % (total, max(seen)))
