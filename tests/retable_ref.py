"""Re-tabling restated in Python (a helper of the tests, imported as requant_ref is): chunks whose levels were written against
quantiser tables that are not AMV's, re-expressed in AMV's tables in the coefficient domain.

The rule (include/amvhip.h, csrc/amv_retable_plan.h) as a composition of what is there:

    levels    orc.entropy_blocks(chunk, 6 * nmcu): the chunk's lines in scan order, the DC absolute, and the decode's status
    DC        level * Qs[0] / Qd[0] to nearest, halves away from zero
    search    trellis_ref.trellis_block(c, comp, 128, lam) on c[k] = level[k] * 8 * Qs[k], against AMV's tables
    chunk     nr_ref._chunk(lines)
    choice    rate_ref.choose / clip_ref.choose_clip over the lengths of the rungs' chunks

A frame is coded only if its decode reports nothing, reaches the last block, its table index names a table, and every block
is in range; otherwise its status is not zero, its chunk None, its error and its bits 0.

Beside the rule: the reference's amv encoder at any -qscale (`reference_tables`, `quantize_reference`, `reference_chunks`:
nr_ref's reference mode with the matrix of a qscale; tests/golden/ref_retable.json pins it to the reference's own ffmpeg),
and the PSNR of a chunk against its source picture in amvlib's BGR (`psnr`).
"""
import hashlib

import numpy as np

import clip_ref as C
import nr_ref as N
import rate_ref as R
import requant_ref as Q
import trellis_ref as T
from nr_ref import orc

QBIAS = Q.QBIAS
COEF_MOST = 8193                           # |level| * 8 Qs: what amv_trellis_plan.h proves its fits for
ENERGY_MOST = 1 << 30
DC_MOST = 1023                             # the NEW DC
TABLES_MAX = 64
ST_TRUNCATED, ST_RANGE, ST_TABLE = 4, 8, 16
OVER = R.OVER
LAMBDA_MAX = T.LAMBDA_MAX
LADDER = Q.LADDER
AMV_TABLES = [[int(x) for x in T.QUANT[0]], [int(x) for x in T.QUANT[1]]]
# the "Q60" tables the 2007 FFmpeg decoder reads device clips with (sp5x_quant_table[10], [11]), scan order
Q60_TABLES = [[13, 9, 10, 11, 10, 8, 13, 11, 10, 11, 14, 14, 13, 15, 19, 32, 21, 19, 18, 18, 19, 39, 28, 30, 23, 32, 46, 41, 49, 48, 46, 41,
               45, 44, 51, 58, 74, 62, 51, 54, 70, 55, 44, 45, 64, 87, 65, 70, 76, 78, 82, 83, 82, 50, 62, 90, 97, 90, 80, 96, 74, 81, 82, 79],
              [14, 14, 14, 19, 17, 19, 38, 21, 21, 38, 79, 53, 45, 53] + [79] * 50]


# ---- the reference's encoder at a qscale ----------------------------------------------------------------------------------------

def reference_matrix(qscale):
    """mpegvideo_enc.c:2866-2877: clip8(ff_mpeg1_default_intra_matrix[i] * qscale >> 3), entry 0 = 8 -> 64 steps, row-major"""
    assert 1 <= qscale <= 31
    m = np.clip((N.MPEG1_INTRA * int(qscale)) >> 3, 0, 255)
    m[0] = N.MPEG1_INTRA[0]
    return m


def reference_tables(qscale):
    """-> [2][64], luma then chroma (the one matrix twice), scan order"""
    row = [int(x) for x in reference_matrix(qscale)[N.ZIGZAG]]
    return [row, list(row)]


def quantize_reference(coef, qscale):
    """nr_ref.quantize_reference with the matrix of a qscale (identical at 8): dct_quantize_c, bias 0 -> zig-zag lines"""
    coef = np.asarray(coef, np.int64)
    qmat = (1 << 22) // (8 * reference_matrix(qscale))
    level = coef * qmat[None, :]
    q = np.sign(level) * (np.abs(level) >> 22)
    q[:, 0] = (coef[:, 0] + 32) // 64 - 128
    return q[:, N.ZIGZAG]


def reference_lines(frames, w, h, qscale):
    return [quantize_reference(N.fdct(N.frame_blocks(y, cb, cr, w, h, 0)), qscale) for y, cb, cr in frames]


def reference_chunks(frames, w, h, qscale):
    """what `ffmpeg -vcodec amv -qscale Q` writes for the frames [(y, cb, cr)] -> chunks"""
    return [N._chunk(zz) for zz in reference_lines(frames, w, h, qscale)]


# ---- the rule ------------------------------------------------------------------------------------------------------------------

def round_div(v, q):
    """v / q to nearest, halves away from zero"""
    r = (2 * abs(v) + q) // (2 * q)
    return -r if v < 0 else r


def new_dc(level, qs0, comp):
    return round_div(int(level) * int(qs0), int(T.QUANT[comp][0]))


def scaled(levels, qs):
    """the block's levels and its source table (scan order) -> c as the search is handed it (position 0 is not looked at)"""
    return [int(levels[k]) * 8 * int(qs[k]) for k in range(64)]


def block_in_range(levels, comp, qs):
    c = scaled(levels, qs)
    return (abs(new_dc(levels[0], qs[0], comp)) <= DC_MOST and all(abs(x) <= COEF_MOST for x in c[1:])
            and sum(x * x for x in c[1:]) <= ENERGY_MOST)


_BLOCK = {}


def retable_block(levels, comp, qs, lam):
    """-> the 64 levels against AMV's tables"""
    key = (np.asarray(levels, np.int16).tobytes(), comp, bytes(qs), int(lam))
    if key not in _BLOCK:
        out = T.trellis_block(scaled(levels, qs), comp, QBIAS, int(lam))
        out[0] = new_dc(levels[0], qs[0], comp)
        _BLOCK[key] = out
    return _BLOCK[key]


def block_error(before, after, comp, qs):
    """(new * Qd - old * Qs)^2 over all 64 positions"""
    qd = T.QUANT[comp]
    return sum((int(after[k]) * int(qd[k]) - int(before[k]) * int(qs[k])) ** 2 for k in range(64))


def decode(chunk, w, h, table):
    """table: [2][64] or None (a bad index) -> (lines or None, status)"""
    nb = Q.nblocks(w, h)
    zz, st = orc.entropy_blocks(chunk, nb)
    if st == 0 and len(zz) < nb:
        st = ST_TRUNCATED
    if st:
        return None, st
    if table is None:
        return None, ST_TABLE
    if not all(block_in_range(zz[b], Q.comp_of(b), table[Q.comp_of(b)]) for b in range(zz.shape[0])):
        return None, ST_RANGE
    return zz, 0


_FRAME = {}


def retable_lines(chunk, w, h, table, lam):
    """-> (lines before or None, lines after or None, status)"""
    tkey = None if table is None else bytes(table[0]) + bytes(table[1])
    key = (hashlib.sha1(bytes(chunk)).hexdigest(), w, h, tkey, int(lam))
    if key not in _FRAME:
        zz, st = decode(chunk, w, h, table)
        after = None
        if zz is not None:
            after = np.array([retable_block(zz[b], Q.comp_of(b), table[Q.comp_of(b)], lam) for b in range(zz.shape[0])], np.int16)
        _FRAME[key] = (zz, after, st)
    return _FRAME[key]


def plane_error(before, after, table):
    err = [0, 0, 0]
    for b in range(before.shape[0]):
        k6 = b % 6
        comp = Q.comp_of(b)
        err[0 if k6 < 4 else k6 - 3] += block_error(before[b], after[b], comp, table[comp])
    return err


def tables_of(tables, table_of, n):
    """a frame's table, None where its index names none"""
    if table_of is None:
        table_of = [0] * n
    return [tables[t] if t < len(tables) else None for t in table_of]


def retable(chunks, w, h, tables, table_of, lam):
    """the stream entry -> (chunks or None per frame, statuses, errors [n][3])"""
    out, status, err = [], [], []
    for chunk, table in zip(chunks, tables_of(tables, table_of, len(chunks))):
        before, after, st = retable_lines(chunk, w, h, table, lam)
        out.append(None if after is None else N._chunk(after))
        status.append(st)
        err.append([0, 0, 0] if after is None else plane_error(before, after, table))
    return out, status, err


def bits_table(chunks, w, h, tables, table_of, ladder):
    rows = []
    for chunk, table in zip(chunks, tables_of(tables, table_of, len(chunks))):
        row = []
        for lam in ladder:
            after = retable_lines(chunk, w, h, table, lam)[1]
            row.append(0 if after is None else R.frame_bits(after))
        rows.append(row)
    return np.array(rows, np.int64).reshape(len(chunks), len(ladder))


def rate(chunks, w, h, tables, table_of, ladder, budgets):
    """the rate entry -> (chunks or None, statuses, rungs with OVER or-ed in): requant_ref.rate with retable in requant's place"""
    if np.isscalar(budgets):
        budgets = [budgets] * len(chunks)
    table = [retable(chunks, w, h, tables, table_of, lam) for lam in ladder]
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


def clip_lens(chunks, w, h, tables, table_of, ladder):
    """-> (lens [n][rungs] with 0 for a frame that is not coded, coded [n])"""
    table = [retable(chunks, w, h, tables, table_of, lam)[0] for lam in ladder]
    coded = [table[0][i] is not None for i in range(len(chunks))]
    lens = np.array([[len(table[r][i]) if coded[i] else 0 for r in range(len(ladder))] for i in range(len(chunks))], np.int64)
    return lens.reshape(len(chunks), len(ladder)), coded


def clip(chunks, w, h, tables, table_of, ladder, budgets, total):
    """the clip entry -> (chunks or None, statuses, rungs, (clip word 0, S(c*))): clip_ref.requant with retable in requant's place"""
    lens, coded = clip_lens(chunks, w, h, tables, table_of, ladder)
    c, over, S = C.choose_clip(lens, budgets, total, coded)
    out, status, rungs = rate(chunks, w, h, tables, table_of, ladder[c:], budgets)
    return out, status, [(r & ~OVER) + c | (r & OVER) for r in rungs], (c | (OVER if over else 0), S)


# ---- pictures ------------------------------------------------------------------------------------------------------------------

def bgr_of_planes(y, cb, cr, w, h):
    """the source picture as amvlib shows samples (StoreBuffer's pixel maths, AmvJpeg.c:805-831 = the oracle's amvo_yuv_to_bgr;
    a chroma sample serves its 2x2 luma samples) -> [h, w, 3] uint8"""
    Y = np.asarray(y, np.int64)[:h, :w]
    u = np.kron(np.asarray(cb, np.int64), np.ones((2, 2), np.int64))[:h, :w] - 128
    v = np.kron(np.asarray(cr, np.int64), np.ones((2, 2), np.int64))[:h, :w] - 128
    r = (Y * 256 + 18 * u + 367 * v) >> 8
    g = (Y * 256 - 159 * u - 220 * v) >> 8
    b = (Y * 256 + 411 * u - 29 * v) >> 8
    return np.clip(np.stack([b, g, r], axis=-1), 0, 255).astype(np.uint8)


def psnr(a, b):
    mse = np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)
    return 99.0 if mse == 0 else 10.0 * np.log10(255.0 * 255.0 / mse)


def decode_psnr(chunk, frame, w, h):
    """the PSNR of the chunk as every AMV decoder shows it (orc.decode_frame) against the source picture in BGR"""
    got, st, _ = orc.decode_frame(chunk, w, h)
    assert st == 0
    return psnr(got[:, : w * 3].reshape(h, w, 3), bgr_of_planes(*frame, w, h))
