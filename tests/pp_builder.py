"""Crafted pictures for the postprocessing tests, seeded and built from 8x8 blocks so that every branch of the reference's
deblock and dering is met in luma and in chroma (tests/test_pp_builder.py asserts that on the restatement's own trace):

  flat blocks whose levels differ from their neighbours' by steps on both sides of QP and of 2 QP   (classes 1 and 0, and the
                                                                                    low-pass's first / last on both sides of QP)
  textured blocks, gentle and rough      (class 2 with middleEnergy on both sides of 8 QP, d clamped by q in both signs)
  ramps with a range of exactly 19 and 20 over the dering's window, and wider ones    (the threshold; updates clamped at + QP2
                                                                                    and - QP2, and unclamped)
  a first and last column that the row-end call changes

picture(width, height, kind, seed, qp) -> [Y, U, V] uint8, pitch = width.  kind: "crafted", "noise", "ramp"."""
import numpy as np

SIZES = ((16, 16), (32, 24), (48, 40), (160, 120), (336, 32))
KINDS = ("crafted", "noise", "ramp")
NARROW = ((16, 22), (16, 48))


def _plane(rng, w, h, kind, qp):
    if kind == "noise":
        return rng.integers(0, 256, (h, w)).astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "ramp":
        return ((xx * 3 + yy * 5 + rng.integers(0, 4, (h, w))) & 255).astype(np.uint8)
    bh, bw = (h + 7) // 8, w // 8
    out = np.zeros((bh * 8, w), np.int64)
    steps = sorted({0, 1, max(qp - 1, 0), qp, qp + 1, 2 * qp - 1 if qp else 0, 2 * qp, 2 * qp + 1, 4 * qp + 3})
    level = int(rng.integers(60, 190))
    r8, c8 = np.mgrid[0:8, 0:8]
    for by in range(bh):
        for bx in range(bw):
            t = int(rng.integers(0, 14))
            level = int(np.clip(level + int(rng.choice(steps)) * int(rng.choice((-1, 1))), 24, 230))
            if t < 3:                                         # flat
                blk = np.full((8, 8), level)
            elif t in (3, 12, 13):                            # flat halves a step of QP .. 2 QP apart: the low-pass's first / last tap is the far one
                step = int(rng.choice((qp, qp + 1, 2 * qp))) * int(rng.choice((-1, 1)))
                blk = np.where((c8 if rng.integers(0, 2) else r8) < 4, level, level + step)
            elif t == 4:                                      # flat but for a speck: still "mostly flat"
                blk = np.full((8, 8), level)
                blk[int(rng.integers(0, 8)), int(rng.integers(0, 8))] += int(rng.integers(2, 12))
            elif t == 5:                                      # gentle texture
                blk = level + rng.integers(-3, 4, (8, 8))
            elif t == 6:                                      # rough texture
                blk = level + rng.integers(-40, 41, (8, 8))
            elif t == 7:                                      # an edge inside the block
                blk = np.where(c8 + r8 // 2 < int(rng.integers(2, 9)), level - 18, level + 18) + rng.integers(-2, 3, (8, 8))
            elif t in (8, 9):                                 # a ramp of range 19 / 20 over any 8 columns beside it
                span = 19 if t == 8 else 20
                blk = level + (c8 * span + 3) // 7 if rng.integers(0, 2) else level + (r8 * span + 3) // 7
            elif t == 10:                                     # a wide smooth ramp with a ripple: dering moves it freely
                blk = level + c8 * 4 + r8 * 3 + (((c8 + r8) & 1) * int(rng.integers(1, 2 * qp + 4)))
            else:                                             # ripple on a step: large corrections, clamped both ways
                blk = level + np.where(c8 < 4, -14, 14) + ((c8 ^ r8) & 1) * int(rng.integers(4, 30)) * int(rng.choice((-1, 1)))
            out[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8] = blk
    if bh >= 2 and bw >= 3:
        # one pair for sure, however small the plane: a flat block over one that steps by QP + 1 at its line 4 -- the vertical
        # low-pass of the edge between them takes its `last` tap from the near side
        out[0:12, 8:16] = level
        out[12:16, 8:16] = level + qp + 1
    out = np.clip(out[:h], 0, 255)
    # the first and last columns: a ripple on a wide range, so the row-end window passes the threshold and moves column 0
    out[:, 0] = np.clip(out[:, 0] + (yy[:, 0] & 1) * 9 - 4, 0, 255)
    out[:, w - 1] = np.clip(out[:, w - 1] - (yy[:, 0] & 1) * 7 + 3, 0, 255)
    if w >= 16:
        out[:, w - 6:w - 1] = np.clip(out[:, w - 6:w - 1] + np.arange(5) * 6, 0, 255)
    return out.astype(np.uint8)


def picture(width, height, kind, seed, qp=12):
    rng = np.random.default_rng([seed, width, height, KINDS.index(kind)])
    return [_plane(rng, width, height, kind, qp), _plane(rng, width // 2, height // 2, kind, qp), _plane(rng, width // 2, height // 2, kind, qp)]


def amv1_frames(orc, golden_dir):
    """the frames of AMV1.amv as the oracle's FFmpeg-mode decode gives them -> (width, height, [[Y, U, V], ...])"""
    import os
    info, vids, _ = orc.parse_amv(open(os.path.join(golden_dir, "AMV1.amv"), "rb").read())
    w, h = info["width"], info["height"]
    return w, h, [[p.copy() for p in orc.yuv_planes(orc.decode_frame_ffmpeg(v, w, h)[0], w, h)] for v in vids]


def cases():
    """the fixture's recipes: (name, width, height, kind or "amv1:k", seed, mode, quality)"""
    out = []
    seed = 100
    for w, h in SIZES + ((320, 240),):
        for mode in ("hb:c,vb:c,dr:c,fq:12", "hb:c,vb:c,fq:12", "vb:c,dr:c,fq:12"):
            for kind in (("crafted",) if (w, h) == (320, 240) else ("crafted", "noise")):
                seed += 1
                out.append(("%dx%d_%s_%s" % (w, h, kind, mode), w, h, kind, seed, mode, 6))
    for mode, quality in (("de", 6), ("de", 4), ("de", 2), ("hb:c:64:20,vb:c,fq:3", 6), ("hb,vb:y,dr:y,fq", 6), ("vb:c,fq:63", 6), ("hb:c,fq:0", 6),
                          ("de,-dr,fq:31", 6), ("vb:c,dr:c,fq:40", 6), ("hb:c,vb:c,dr:c,fq:1", 6), ("hb:c,vb:c,dr:c,fq:0", 6), ("de:c,fq:63", 6)):
        for w, h in ((32, 24), (48, 40), (160, 120)):
            seed += 1
            out.append(("%dx%d_%s_%s_q%d" % (w, h, "crafted", mode, quality), w, h, "crafted", seed, mode, quality))
    # 16 columns: the chroma plane is one block wide, its only dering call is the row-end one and its window folds onto itself
    for w, h in NARROW:
        for mode in ("de:c,fq:12", "de:c,fq:63", "vb:c,dr:c,fq:3"):
            for kind in ("crafted", "noise"):
                seed += 1
                out.append(("%dx%d_%s_%s" % (w, h, kind, mode), w, h, kind, seed, mode, 6))
    for k in range(3):
        out.append(("amv1_%d_de_fq12" % k, 0, 0, "amv1:%d" % k, 0, "de:c,fq:12", 6))
    return out


def case_qp(mode):
    """the QP the crafted picture of a case is built around: the mode's fq, or 1"""
    for tok in mode.replace("/", ",").split(","):
        parts = tok.split(":")
        if parts[0] in ("fq", "forcequant"):
            nums = [p for p in parts[1:] if p.isdigit()]
            return int(nums[0]) if nums else 15
    return 1
