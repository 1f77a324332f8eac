"""The video encoder's byte budget per frame restated in Python (a helper of the tests, imported as nr_ref and trellis_ref are).

A ladder is a list of lambdas in the caller's order of preference; len_r(i) is the length of the chunk the request's trellis
entry writes for frame i at ladder[r]; the budget B(i) is a number of bytes; the chosen rung is the FIRST r with
len_r(i) <= B(i), the last one (flagged with OVER) when none fits.  The model is built on what is there:

    levels    nr_trellis_ref.encode_stream(..., want_coef=True) per rung, each from a copy of the state handed in (the -nr
              sums are taken before the dead zone, so every rung leaves the same state)
    bits      from the levels and the code lengths alone: the DC difference codes and magnitudes, the AC run/size codes,
              magnitudes, ZRLs and EOBs -- what the entropy coder writes before padding and escaping
    lengths   from the bytes: len(nr_ref._chunk(levels))

so the two tables are independent of each other, and len == 4 + ceil(bits / 8) + escapes ties them (tests/test_rate_ref.py).
`device_walk` is the choice as the device makes it (amv_rate_plan.h): floors of the bits, the first floor-fit, a check of the
real length, the next floor-fit.
"""
import hashlib

import numpy as np

import nr_ref as N
import nr_trellis_ref as NT
import trellis_ref as T
from nr_ref import orc

RUNGS_MAX = 16
OVER = 0x80000000
LADDER = [0, 400, 3481, 20000, T.LAMBDA_MAX]
KINDS = ["ramp", "texture", "noise", "flat"]
# the GPU tests' inputs: name -> (w, h, frames, seed)
SHAPES = {"16x16": (16, 16, 8, 37), "50x38": (50, 38, 4, 62), "176x96": (176, 96, 1, 83)}


def frames_of(w, h, n, seed):
    return N.stream(w, h, [KINDS[i % len(KINDS)] for i in range(n)], seed)


def shape(name):
    w, h, n, seed = SHAPES[name]
    return w, h, frames_of(w, h, n, seed)


_DC = {}


def dc_lengths(comp):
    if comp not in _DC:
        _DC[comp] = [int(x) for x in orc.huffman_codes(comp)[0]]
    return _DC[comp]


def block_bits(zz, comp):
    """AC + EOB bits of one block's levels (scan order): T.product_bits per level, the EOB where the last position is 0"""
    length = T.ac_lengths(comp)
    bits, coded = 0, 0
    for k in range(1, 64):
        v = int(zz[k])
        if v:
            bits += T.product_bits(length, k - coded - 1, abs(v))
            coded = k
    return bits + (length[0x00] if coded < 63 else 0)


def dc_bits(diff, comp):
    nb = T.nbits(abs(int(diff)))
    return dc_lengths(comp)[nb] + nb


def frame_dc_bits(zz):
    """the DC term of a frame's lines [blocks, 64] (MCU order: Y0 Y1 Y2 Y3 Cb Cr): each block against its component's predecessor"""
    pred, bits = [0, 0, 0], 0
    for b in range(zz.shape[0]):
        k6 = b % 6
        c = 0 if k6 < 4 else k6 - 3
        bits += dc_bits(int(zz[b, 0]) - pred[c], 0 if k6 < 4 else 1)
        pred[c] = int(zz[b, 0])
    return bits


def frame_bits(zz):
    return frame_dc_bits(zz) + sum(block_bits(zz[b], 0 if b % 6 < 4 else 1) for b in range(zz.shape[0]))


def floor_bytes(bits):
    return 4 + (bits + 7) // 8


def escapes(chunk):
    return chunk[2:-2].count(b"\xff\x00")


_LEVELS = {}


def levels_table(frames, w, h, qbias, nr, state, ladder):
    """-> (levels[rung][frame] zig-zag lines, the state after the frames); made once per input"""
    start = N.new_state() if state is None else np.array(state, np.int64)
    key = (hashlib.sha1(N.raw_bytes(frames)).hexdigest(), w, h, qbias, nr, tuple(int(x) for x in start) if nr else None)
    after = start.copy()
    out = []
    for lam in ladder:
        k = key + (int(lam),)
        if k not in _LEVELS:
            s = start.copy()
            _LEVELS[k] = (NT.encode_stream(frames, w, h, nr, int(lam), state=s, qbias=qbias, want_coef=True), s)
        out.append(_LEVELS[k][0])
        after = _LEVELS[k][1]
    return out, after.copy()


def bits_table(frames, w, h, qbias, nr, state, ladder):
    """[n][rungs] int64: the bits of frame i's scan at ladder[r]"""
    levels, _ = levels_table(frames, w, h, qbias, nr, state, ladder)
    return np.array([[frame_bits(levels[r][i]) for r in range(len(ladder))] for i in range(len(frames))], np.int64)


def chunks_table(frames, w, h, qbias, nr, state, ladder):
    """[n][rungs] the chunks themselves"""
    levels, _ = levels_table(frames, w, h, qbias, nr, state, ladder)
    return [[N._chunk(levels[r][i]) for r in range(len(ladder))] for i in range(len(frames))]


def lens_table(frames, w, h, qbias, nr, state, ladder):
    return np.array([[len(c) for c in row] for row in chunks_table(frames, w, h, qbias, nr, state, ladder)], np.int64)


def choose(lens_row, budget):
    """-> (rung, over): the first rung whose length is inside the budget; none: the last one, over"""
    for r, length in enumerate(lens_row):
        if int(length) <= budget:
            return r, False
    return len(lens_row) - 1, True


def first_fit(bits_row, budget, start):
    for r in range(start, len(bits_row)):
        if floor_bytes(int(bits_row[r])) <= budget:
            return r
    return len(bits_row)


def device_walk(bits_row, lens_row, budget):
    """the choice as the device makes it -> (rung, over, codings): the first floor-fit, then per pass the real length against
    the budget and the next floor-fit; a frame with no floor-fit left is coded at the last rung and not looked at again"""
    rungs = len(bits_row)
    r = first_fit(bits_row, budget, 0)
    if r == rungs:
        return rungs - 1, True, 1
    codings = 1
    while int(lens_row[r]) > budget:
        nxt = first_fit(bits_row, budget, r + 1)
        if nxt == rungs:
            return rungs - 1, True, codings + (0 if r == rungs - 1 else 1)
        r = nxt
        codings += 1
    return r, False, codings


def encode(frames, w, h, qbias, nr, state, ladder, budgets):
    """budgets: one number or one per frame -> (chunks, rungs with OVER or-ed in, the state afterwards)"""
    chunks = chunks_table(frames, w, h, qbias, nr, state, ladder)
    _, after = levels_table(frames, w, h, qbias, nr, state, ladder)
    if np.isscalar(budgets):
        budgets = [budgets] * len(frames)
    out, rungs = [], []
    for i, row in enumerate(chunks):
        r, over = choose([len(c) for c in row], int(budgets[i]))
        out.append(row[r])
        rungs.append(r | (OVER if over else 0))
    return out, rungs, after
