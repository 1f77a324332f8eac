"""The byte budget per clip restated in Python (a helper of the tests, imported as rate_ref is), on top of rate_ref and
requant_ref.

The definition (include/amvhip.h): for a clip rung c, frame i is coded at r_c(i) -- rate_ref.choose over the ladder from c
on -- S(c) is the sum of those lengths, and the clip is coded at the FIRST c with S(c) <= total, the last one (flagged with
OVER) when none fits; the chunks are rate_ref.encode's on the ladder's tail from c* on.  A frame the requant entry does not
code has no lengths: it adds nothing to a sum.

`device_walk` is the choice as the device makes it (amv_clip_plan.h): floor sums that bound S from below, the first clip rung
whose bound fits, the frames moved along their floor-fits pass by pass, the sum of real lengths when a pass lists nobody, and
the move of the clip to the next rung whose bound fits, which takes along the frames below it.
"""
import numpy as np

import rate_ref as R
import requant_ref as Q

OVER = R.OVER
NO_CAP = 0xFFFFFFFF
U64_MAX = (1 << 64) - 1


def passes_most(rungs):
    """amv_clip_plan.h: clip_passes_most"""
    return rungs * (rungs + 1) // 2


def budgets_of(budgets, n):
    return [int(budgets)] * n if np.isscalar(budgets) else [int(b) for b in budgets]


# ---- the definition ---------------------------------------------------------------------------------------------------------

def frame_rung(lens_row, budget, c):
    """r_c(i) -> (rung in the full ladder, over)"""
    r, over = R.choose(lens_row[c:], budget)
    return c + r, over


def clip_sum(lens, budgets, c, coded=None):
    """S(c) over a lens table [n][rungs]; coded: None or a flag per frame"""
    B = budgets_of(budgets, len(lens))
    return sum(int(lens[i][frame_rung(lens[i], B[i], c)[0]]) for i in range(len(lens)) if coded is None or coded[i])


def sums(lens, budgets, coded=None):
    return [clip_sum(lens, budgets, c, coded) for c in range(len(lens[0]))]


def choose_clip(lens, budgets, total, coded=None):
    """-> (c*, over, S(c*))"""
    S = sums(lens, budgets, coded)
    for c, s in enumerate(S):
        if s <= total:
            return c, False, s
    return len(S) - 1, True, S[-1]


def rungs_at(lens, budgets, c, coded=None):
    """d_rung of every frame at clip rung c (OVER or-ed in)"""
    B = budgets_of(budgets, len(lens))
    out = []
    for i in range(len(lens)):
        if coded is not None and not coded[i]:
            out.append((len(lens[i]) - 1) | OVER)
            continue
        r, over = frame_rung(lens[i], B[i], c)
        out.append(r | (OVER if over else 0))
    return out


def encode(frames, w, h, qbias, nr, state, ladder, budgets, total):
    """-> (chunks, rungs in the full ladder with OVER or-ed in, (clip word 0, S(c*)), the state afterwards)"""
    lens = R.lens_table(frames, w, h, qbias, nr, state, ladder)
    c, over, S = choose_clip(lens, budgets, total)
    chunks, rungs, after = R.encode(frames, w, h, qbias, nr, state, ladder[c:], budgets)
    return chunks, [(r & ~OVER) + c | (r & OVER) for r in rungs], (c | (OVER if over else 0), S), after


def requant_lens(chunks, w, h, ladder):
    """-> (lens [n][rungs] with 0 for a frame that is not coded, coded [n])"""
    table = [Q.requant(chunks, w, h, lam)[0] for lam in ladder]
    coded = [table[0][i] is not None for i in range(len(chunks))]
    lens = np.array([[len(table[r][i]) if coded[i] else 0 for r in range(len(ladder))] for i in range(len(chunks))], np.int64)
    return lens.reshape(len(chunks), len(ladder)), coded


def requant(chunks, w, h, ladder, budgets, total):
    """-> (chunks or None, statuses, rungs, (clip word 0, S(c*)))"""
    lens, coded = requant_lens(chunks, w, h, ladder)
    c, over, S = choose_clip(lens, budgets, total, coded)
    out, status, rungs = Q.rate(chunks, w, h, ladder[c:], budgets)
    # (a frame that is not coded has the tail's last rung, flagged: the full ladder's last rung)
    return out, status, [(r & ~OVER) + c | (r & OVER) for r in rungs], (c | (OVER if over else 0), S)


# ---- the walk as the device takes it ------------------------------------------------------------------------------------------

def most_bytes(bits):
    """the longest chunk `bits` of scan can make: every scan byte an FF"""
    return 4 + 2 * ((int(bits) + 7) // 8)


def frame_floor(bits_row, budget, c):
    """a frame's part of F(c): amv_clip_plan.h, clip_floor"""
    rungs = len(bits_row)
    least = None
    r = R.first_fit(bits_row, budget, c)
    while r < rungs:
        f = R.floor_bytes(int(bits_row[r]))
        least = f if least is None else min(least, f)
        if most_bytes(bits_row[r]) <= budget:
            return least
        r = R.first_fit(bits_row, budget, r + 1)
    last = R.floor_bytes(int(bits_row[-1]))
    return last if least is None else min(least, last)


def floor_sums(bits, budgets, coded=None):
    B = budgets_of(budgets, len(bits))
    return [sum(frame_floor(bits[i], B[i], c) for i in range(len(bits)) if coded is None or coded[i]) for c in range(len(bits[0]))]


def record_at(bits_row, budget, c):
    r = R.first_fit(bits_row, budget, c)
    return (r, False) if r < len(bits_row) else (len(bits_row) - 1, True)


def first_rung(F, total, start):
    for c in range(start, len(F)):
        if F[c] <= total:
            return c
    return len(F) - 1


def device_walk(bits, lens, budgets, total, coded=None):
    """-> (c*, over, S, rungs with OVER or-ed in, passes that coded a frame, per-frame codings, the clip rungs coded at)"""
    n, rungs = len(bits), len(bits[0])
    B = budgets_of(budgets, n)
    live = [coded is None or coded[i] for i in range(n)]
    F = floor_sums(bits, budgets, coded)
    c = first_rung(F, total, 0)
    visited = [c]
    record = [record_at(bits[i], B[i], c) if live[i] else (rungs - 1, True) for i in range(n)]
    length = [int(lens[i][record[i][0]]) for i in range(n)]             # the first pass codes every frame
    codings = [1] * n
    passes = 1
    listed = list(range(n))
    while True:
        # the check of the frames just coded (amv_rate_plan.h: rate_check)
        nxt = []
        for i in listed:
            r, over = record[i]
            if over or length[i] <= B[i]:
                continue
            f = R.first_fit(bits[i], B[i], r + 1)
            record[i] = (f, False) if f < rungs else (rungs - 1, True)
            if f < rungs or r != rungs - 1:
                nxt.append(i)
        # the settle
        while not nxt:
            S = sum(length[i] for i in range(n) if live[i])
            if S <= total or c == rungs - 1:
                out = [r | (OVER if over else 0) for r, over in record]
                return c, S > total, S, out, passes, codings, visited
            c = first_rung(F, total, c + 1)
            visited.append(c)
            for i in range(n):
                if live[i] and record[i][0] < c:
                    record[i] = record_at(bits[i], B[i], c)
                    nxt.append(i)
        listed = nxt
        passes += 1
        for i in listed:
            length[i] = int(lens[i][record[i][0]])
            codings[i] += 1


def bound_table(rungs):
    """A bits / lens table that takes every one of passes_most(rungs) passes, with the budget per frame and the total to hand
    over: frame c (c < rungs - 1) fits below rung c, and from c on its floor fits and its length is one byte over until the
    last rung; a last frame that is far too long before the last rung keeps every S(c) over the total."""
    B = 100
    bits = [[8 * (B - 4)] * rungs for _ in range(rungs)]
    lens = [[B if r < c or r == rungs - 1 else B + 1 for r in range(rungs)] for c in range(rungs - 1)]
    bits[rungs - 1] = [8 * 1000] * (rungs - 1) + [8]
    lens.append([2000] * (rungs - 1) + [5])
    budgets = [B] * (rungs - 1) + [NO_CAP]
    return np.array(bits, np.int64), np.array(lens, np.int64), budgets, (rungs - 1) * B + 1004
