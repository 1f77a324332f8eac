"""AMV chunks requantised in the coefficient domain, restated in Python (a helper of the tests, imported as rate_ref is).

The rule (include/amvhip.h, csrc/amv_requant_plan.h) as a composition of what is there:

    levels    orc.entropy_blocks(chunk, 6 * nmcu): the chunk's lines in scan order, the DC absolute, and the decode's status
    search    trellis_ref.trellis_block(c, comp, 128, lam) on c[i] = level[i] * 8 * Q[i]; the DC level is carried
    chunk     nr_ref._chunk(lines): SOI, the escaped scan, padding, EOI
    choice    rate_ref.choose over the lengths of the rungs' chunks (the first rung that fits)

A frame is coded only if its decode reports nothing, reaches the last block, and every block is in range (`in_range`);
otherwise its status is not zero, its chunk None, its error and its bits 0.
"""
import hashlib

import numpy as np

import nr_ref as N
import rate_ref as R
import trellis_ref as T
from nr_ref import orc

QBIAS = 128                                # the rounding term one half: 128 << 14 = 2^21
COEF_MOST = 8193 + 8 * 61                  # R: |level| * 8 Q
ENERGY_MOST = 1 << 30                      # the sum of (level * 8 Q)^2 over a block's AC positions
DC_MOST = 1023
ST_TRUNCATED, ST_RANGE = 4, 8
OVER = R.OVER
LAMBDA_MAX = T.LAMBDA_MAX
LADDER = [0, 1000, 3481, 20000, T.LAMBDA_MAX]
# a luma block whose AC energy is ENERGY_MOST exactly ({scan position: level}; every |level * 8 Q| is inside COEF_MOST), and
# where one more step of one level still is (position 59: 16 * 8 * 60 = 7680)
AT_ENERGY_MOST = {1: 171, 2: 175, 3: 154, 5: 190, 9: 154, 10: 119, 12: 132, 19: 98, 23: 56, 30: 34, 36: 22, 37: 27, 41: 27, 54: 24,
                  55: 17, 59: 15}


def block_of(levels, dc=0):
    """{scan position: level} -> the 64 levels"""
    out = [0] * 64
    out[0] = dc
    for k, v in levels.items():
        out[k] = v
    return out


def energy(levels, comp):
    return sum(x * x for x in scaled(levels, comp)[1:])


def nblocks(w, h):
    return 6 * orc.nmcu(w, h)


def comp_of(b):
    return 0 if b % 6 < 4 else 1


def scaled(levels, comp):
    """the block's levels (scan order) -> c as the search is handed it (position 0 is not looked at)"""
    return [int(levels[i]) * 8 * int(T.QUANT[comp][i]) for i in range(64)]


def block_in_range(levels, comp):
    c = scaled(levels, comp)
    return (abs(int(levels[0])) <= DC_MOST and all(abs(x) <= COEF_MOST for x in c[1:])
            and sum(x * x for x in c[1:]) <= ENERGY_MOST)


def in_range(zz):
    return all(block_in_range(zz[b], comp_of(b)) for b in range(zz.shape[0]))


_BLOCK = {}


def requant_block(levels, comp, lam):
    """-> the 64 levels after the search (the DC carried)"""
    key = (np.asarray(levels, np.int16).tobytes(), comp, int(lam))
    if key not in _BLOCK:
        out = T.trellis_block(scaled(levels, comp), comp, QBIAS, int(lam))
        out[0] = int(levels[0])
        _BLOCK[key] = out
    return _BLOCK[key]


def decode(chunk, w, h):
    """-> (lines [6 nmcu, 64] int16 or None, status): None where the frame is not coded"""
    nb = nblocks(w, h)
    zz, st = orc.entropy_blocks(chunk, nb)
    if st == 0 and len(zz) < nb:
        st = ST_TRUNCATED
    if st:
        return None, st
    if not in_range(zz):
        return None, ST_RANGE
    return zz, 0


def plane_error(before, after):
    """[3] the sum of ((new - old) * Q)^2 over the AC positions of the blocks of Y, Cb, Cr"""
    err = [0, 0, 0]
    for b in range(before.shape[0]):
        k6 = b % 6
        q = T.QUANT[comp_of(b)]
        err[0 if k6 < 4 else k6 - 3] += sum(((int(after[b][i]) - int(before[b][i])) * int(q[i])) ** 2 for i in range(1, 64))
    return err


_FRAME = {}


def requant_lines(chunk, w, h, lam):
    """-> (lines before or None, lines after or None, status)"""
    key = (hashlib.sha1(bytes(chunk)).hexdigest(), w, h, int(lam))
    if key not in _FRAME:
        zz, st = decode(chunk, w, h)
        after = None
        if zz is not None:
            after = np.array([requant_block(zz[b], comp_of(b), lam) for b in range(zz.shape[0])], np.int16)
        _FRAME[key] = (zz, after, st)
    return _FRAME[key]


def requant(chunks, w, h, lam):
    """the stream entry -> (chunks or None per frame, statuses, errors [n][3])"""
    out, status, err = [], [], []
    for chunk in chunks:
        before, after, st = requant_lines(chunk, w, h, lam)
        out.append(None if after is None else N._chunk(after))
        status.append(st)
        err.append([0, 0, 0] if after is None else plane_error(before, after))
    return out, status, err


def bits_table(chunks, w, h, ladder):
    """[n][rungs]: the bits of the frame's scan at ladder[r]; the row of a frame that is not coded is 0"""
    rows = []
    for chunk in chunks:
        row = []
        for lam in ladder:
            after = requant_lines(chunk, w, h, lam)[1]
            row.append(0 if after is None else R.frame_bits(after))
        rows.append(row)
    return np.array(rows, np.int64).reshape(len(chunks), len(ladder))


def rate(chunks, w, h, ladder, budgets):
    """the rate entry -> (chunks or None, statuses, rungs with OVER or-ed in)"""
    if np.isscalar(budgets):
        budgets = [budgets] * len(chunks)
    table = [requant(chunks, w, h, lam) for lam in ladder]
    out, rungs = [], []
    status = table[0][1]
    for i in range(len(chunks)):
        if status[i]:
            out.append(None)
            rungs.append((len(ladder) - 1) | OVER)
            continue
        r, over = R.choose([len(table[k][0][i]) for k in range(len(ladder))], int(budgets[i]))
        out.append(table[r][0][i])
        rungs.append(r | (OVER if over else 0))
    return out, status, rungs


def pack(chunks):
    """chunks back to back (4-byte aligned blob with slack behind) -> (blob uint8, offs uint64, lens uint32)"""
    lens = np.array([len(c) for c in chunks], np.uint32)
    offs = np.zeros(len(chunks), np.uint64)
    if len(chunks):
        offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    blob = np.zeros(int(lens.sum()) + 16, np.uint8)
    for c, o in zip(chunks, offs):
        blob[int(o): int(o) + len(c)] = np.frombuffer(bytes(c), np.uint8)
    return blob, offs, lens


def synth_chunks(w, h, n, seed=0xC0FFEE, qbias=0):
    """n oracle-encoded synthetic frames of an even size -> list of chunks"""
    blob, offs, lens = orc.synth_stream(seed, 0, n, w, h, qbias)
    return [blob[int(o): int(o) + int(ln)].tobytes() for o, ln in zip(offs, lens)]
