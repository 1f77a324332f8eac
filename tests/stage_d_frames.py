"""Frames for stage D of the reconstruction kernel (amv_reconstruct.hip: chroma_terms, patch_row), and the condition they
must meet.

Stage D takes a 4x2-pixel patch per lane and forms the twelve bytes of each of its two rows -- B G R of four pixels --
as six byte pairs, each one packed add and one saturating pack.  A byte's place in its dword decides which instruction
form writes it, so every one of the 24 places (twelve bytes, two rows) has to be seen clamped to 0 from a negative
sum, clamped to 255 from a sum above 255, and unclamped in between.  The frames are built for that: every MCU has its
chroma DCs at one of five settings (both high, both low, both zero, one of each), its four luma blocks at low, middle
and high levels that differ from block to block, and a horizontal and a vertical AC (natural places 1 and 8) in every
block so that the four pixels and the two rows of a patch differ.
"""
import numpy as np

import coef_builder as cb

SIZES = ((160, 16), (160, 24), (160, 80), (160, 64), (16, 16), (18, 10))
FRAMES_PER_SIZE = 3

_CHROMA = ((89, 89), (-89, -89), (0, 0), (89, -89), (-89, 89))   # DC of Cb, Cr: a step of 9 puts +-89 at +-100
_LUMA = (-118, 0, 117)                                            # DC of Y: a step of 8 puts these at 10, 128, 245
_AC1 = (1, -2, 2, -1, 3)
_AC8 = (2, -1, -3, 1, -2)
_SCAN_OF_AC1, _SCAN_OF_AC8 = int(cb.SCAN_OF_NATURAL[1]), int(cb.SCAN_OF_NATURAL[8])


def mcus(w, h):
    return ((w + 15) // 16) * ((h + 15) // 16)


def frame(w, h, variant):
    """[mcus * 6, 64] int16 scan-order lines; `variant` turns the settings on by one MCU, so three frames of a single
    MCU still see (high, high), (low, low) and (zero, zero) chroma"""
    nm = mcus(w, h)
    coef = np.zeros((nm * 6, 64), np.int64)
    for m in range(nm):
        for k in range(4):
            line = coef[m * 6 + k]
            line[0] = _LUMA[(m + k + variant) % 3] + (5 * m + 3 * k) % 9 - 4
            line[_SCAN_OF_AC1] = _AC1[(m + k) % 5]
            line[_SCAN_OF_AC8] = _AC8[(m + 2 * k) % 5]
        for k, dc in zip((4, 5), _CHROMA[(m + variant) % 5]):
            line = coef[m * 6 + k]
            line[0] = dc
            line[_SCAN_OF_AC1] = 1 if (m + k) % 2 else -1
            line[_SCAN_OF_AC8] = -1 if m % 3 else 1
    return coef.astype(np.int16)


def frames(w, h):
    return np.stack([frame(w, h, v) for v in range(FRAMES_PER_SIZE)])


def sums(orc, coef, w, h, flags):
    """StoreBuffer's sums in front of their clamps for every pixel of the picture, from the oracle's own IDCT output
    -> int32 [h, w, 3] in the order B, G, R, rows in scan order (top first)"""
    mcw, mch = (w + 15) // 16, (h + 15) // 16
    y, u, v = cb._planes(cb.idct_blocks(orc, coef, flags), mcw, mch)
    up = lambda c: np.repeat(np.repeat(c, 2, 0), 2, 1)
    return np.stack(cb.colour_terms(y, up(u), up(v)), -1)[:h, :w]


def coverage(sum_frames, want_frames, oks, w, h):
    """which of (negative -> 0, above 255 -> 255, strictly between) each of the 24 places of a patch has seen over these
    frames, counting decoded pixels inside the picture only -> bool [2, 12, 3].  The expected bytes must agree with
    the sums' classes: that ties the condition to the array the GPU's output is compared with."""
    mcw = (w + 15) // 16
    seen = np.zeros((2, 12, 3), bool)
    for s, want, ok in zip(sum_frames, want_frames, oks):
        px = want[::-1, : w * 3].reshape(h, w, 3)                       # stored bottom-up
        yy, xx = np.mgrid[0:h, 0:w]
        decoded = (yy // 16) * mcw + xx // 16 < ok
        for ch in range(3):
            place = 3 * (xx % 4) + ch
            for cls, hit in enumerate((s[..., ch] < 0, s[..., ch] > 255, (s[..., ch] > 0) & (s[..., ch] < 255))):
                hit = hit & decoded
                assert (px[..., ch][hit] == (0, 255)[cls]).all() if cls < 2 else \
                    ((px[..., ch][hit] > 0) & (px[..., ch][hit] < 255)).all(), "the expected bytes disagree with the sums"
                seen[yy[hit] % 2, place[hit], cls] = True
    return seen


def expected(orc, coefs, oks, w, h, flags):
    return np.stack([cb.picture(orc, c, w, h, ok, flags) for c, ok in zip(coefs, oks)])


def assert_covered(orc, coefs, oks, w, h, flags):
    """the condition, on the expected array; returns that array"""
    want = expected(orc, coefs, oks, w, h, flags)
    seen = coverage([sums(orc, c, w, h, flags) for c in coefs], want, oks, w, h)
    missing = [(int(r), int(p), ("0 from below", "255 from above", "between")[c]) for r, p, c in np.argwhere(~seen)]
    assert not missing, "%dx%d flags %d: (row, byte, class) never seen: %s" % (w, h, flags, missing)
    return want
