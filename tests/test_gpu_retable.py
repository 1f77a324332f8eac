"""Re-tabling (amvhip_retable_stream_dev, _rate_probe_dev, _rate_stream_dev, _clip_stream_dev) on a real MI355X against
tests/retable_ref.py: every frame of every case, d_out, the offsets, the lengths, d_status, d_err, d_bits, d_rung and d_clip, bytes
against bytes and words against words, in both entropy modes.

Shapes are the smallest that reach each path: 16x16 (one MCU) x 1, 3 and 130 (the coder's lane per frame spans two waves and a
tail), 48x32 x 6 chunks of the reference's encoder at -qscale 2, 8 and 31 (what the entries are for), 130x98 and 131x97
oracle-encoded chunks (a partial last MCU row, odd both ways) read against the Q60 tables, against steps of 16 everywhere (which
puts every frame out of range) and of 4,
16x16 x 1030 (two rounds of the coefficient workspace).  The model's tables are made once per input and shared (retable_ref
caches frames and blocks)."""
import ctypes

import numpy as np
import pytest

import clip_ref as C
import nr_ref as N
import rate_ref as R
import requant_ref as Q
import retable_ref as RT
import scan_builder as sb
import test_gpu_requant as TQ
from test_gpu_encode_nr_trellis import FILL, both_modes  # noqa: F401  (both_modes is a fixture)
from test_gpu_parity import _t

pytestmark = pytest.mark.gpu

UNWRITTEN = TQ.UNWRITTEN
CLIP_UNWRITTEN = 0x5A5A5A5A5A5A5A5A
ALL_16 = [[16] * 64] * 2
FOURS = [[4] * 64] * 2
ALL_1, ALL_255 = [[1] * 64] * 2, [[255] * 64] * 2
KINDS = ["ramp", "texture", "ramp", "texture", "noise", "flat"]
# name -> (w, h, frames, tables)
SHAPES = {"16x16 x 1": (16, 16, 1, RT.Q60_TABLES), "16x16 x 3": (16, 16, 3, RT.reference_tables(2)), "16x16 x 130": (16, 16, 130, RT.Q60_TABLES),
          "qscale 2": (48, 32, 6, RT.reference_tables(2)), "qscale 8": (48, 32, 6, RT.reference_tables(8)),
          "qscale 31": (48, 32, 6, RT.reference_tables(31)), "130x98, Q60": (130, 98, 2, RT.Q60_TABLES), "130x98, 16": (130, 98, 2, ALL_16),
          "131x97, Q60": (131, 97, 2, RT.Q60_TABLES), "131x97, 16": (131, 97, 2, ALL_16), "130x98, 4": (130, 98, 2, FOURS),
          "131x97, 4": (131, 97, 2, FOURS)}
_CHUNKS = {}


def chunks_of(name):
    """-> (w, h, chunks, [the table])"""
    w, h, n, table = SHAPES[name]
    key = name.split(",")[0]
    if key not in _CHUNKS:
        if name.startswith("qscale"):
            _CHUNKS[key] = RT.reference_chunks(N.stream(w, h, KINDS, 100), w, h, int(name.split()[1]))
        else:
            _CHUNKS[key] = Q.synth_chunks(w + (w & 1), h + (h & 1), n, seed=0xC0FFEE + w)
    return w, h, _CHUNKS[key], [table]


def _rt(pkg, tables, table_of, keep):
    d_table_of = None
    if table_of is not None:
        d_table_of = _t(np.asarray(table_of, np.uint8))
        keep.append(d_table_of)
    rt = pkg.Retable(tables, d_table_of)
    keep.append(rt)
    return rt


def _stream(ctx, pkg, chunks, w, h, tables, table_of, lam, cap=None, want_err=True):
    """-> (blob, offs, lens, status, err or None)"""
    import torch
    d_blob, blob_bytes, d_offs, d_lens, n = TQ._inputs(chunks)
    cap = 4 * sum(len(c) for c in chunks) + 64 * n + 64 if cap is None else cap
    out, out_offs, out_lens, status = TQ._outs(n, cap)
    err = torch.full((n, 3), -1, dtype=torch.int64, device="cuda:0") if want_err else None
    keep = []
    ctx.retable_stream_dev(d_blob, blob_bytes, d_offs, d_lens, n, w, h, _rt(pkg, tables, table_of, keep), lam, out, cap, out_offs, out_lens, status, err)
    torch.cuda.synchronize()
    return (out.cpu().numpy(), out_offs.cpu().numpy(), out_lens.cpu().numpy(), status.cpu().numpy(),
            err.cpu().numpy().tolist() if want_err else None)


def _probe(ctx, pkg, chunks, w, h, tables, table_of, ladder):
    import torch
    d_blob, blob_bytes, d_offs, d_lens, n = TQ._inputs(chunks)
    bits = torch.full((n, len(ladder)), UNWRITTEN, dtype=torch.int32, device="cuda:0")
    keep = []
    ctx.retable_rate_probe_dev(d_blob, blob_bytes, d_offs, d_lens, n, w, h, _rt(pkg, tables, table_of, keep), ladder, bits)
    torch.cuda.synchronize()
    return bits.cpu().numpy().view(np.uint32).astype(np.int64)


def _rate_of(pkg, ladder, budgets, keep):
    if np.isscalar(budgets):
        return pkg.Rate(ladder, budget=int(budgets))
    keep.append(_t(np.asarray(budgets, np.uint32)))
    return pkg.Rate(ladder, budget=1, d_budget=keep[-1])


def _rate(ctx, pkg, chunks, w, h, tables, table_of, ladder, budgets, cap=None):
    """-> (blob, offs, lens, status, rungs)"""
    import torch
    d_blob, blob_bytes, d_offs, d_lens, n = TQ._inputs(chunks)
    cap = 4 * sum(len(c) for c in chunks) + 64 * n + 64 if cap is None else cap
    out, out_offs, out_lens, status = TQ._outs(n, cap)
    rung = torch.full((n,), UNWRITTEN, dtype=torch.int32, device="cuda:0")
    keep = []
    ctx.retable_rate_stream_dev(d_blob, blob_bytes, d_offs, d_lens, n, w, h, _rt(pkg, tables, table_of, keep), _rate_of(pkg, ladder, budgets, keep),
                                out, cap, out_offs, out_lens, status, rung)
    torch.cuda.synchronize()
    return (out.cpu().numpy(), out_offs.cpu().numpy(), out_lens.cpu().numpy(), status.cpu().numpy(),
            rung.cpu().numpy().view(np.uint32).astype(np.int64))


def _clip(ctx, pkg, chunks, w, h, tables, table_of, ladder, budgets, total, cap=None):
    """-> (blob, offs, lens, status, rungs, clip [2])"""
    import torch
    d_blob, blob_bytes, d_offs, d_lens, n = TQ._inputs(chunks)
    cap = 4 * sum(len(c) for c in chunks) + 64 * n + 64 if cap is None else cap
    out, out_offs, out_lens, status = TQ._outs(n, cap)
    rung = torch.full((n,), UNWRITTEN, dtype=torch.int32, device="cuda:0")
    d_clip = _t(np.full(2, CLIP_UNWRITTEN, np.uint64))
    keep = []
    ctx.retable_clip_stream_dev(d_blob, blob_bytes, d_offs, d_lens, n, w, h, _rt(pkg, tables, table_of, keep), _rate_of(pkg, ladder, budgets, keep),
                                total, out, cap, out_offs, out_lens, status, rung, d_clip)
    torch.cuda.synchronize()
    return (out.cpu().numpy(), out_offs.cpu().numpy(), out_lens.cpu().numpy(), status.cpu().numpy(),
            rung.cpu().numpy().view(np.uint32).astype(np.int64), [int(x) for x in d_clip.cpu().numpy().view(np.uint64)])


_check = TQ._check


# ---- the entries on every shape ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lam", [0, 3481, RT.LAMBDA_MAX])
@pytest.mark.parametrize("name", list(SHAPES))
def test_stream(ctx, pkg, both_modes, name, lam):
    w, h, chunks, tables = chunks_of(name)
    want, status, err = RT.retable(chunks, w, h, tables, None, lam)
    # (the synthetic pictures' strongest levels leave the range against Q60 in one frame of two, against steps of 16 in both:
    # at these sizes the frames that are not coded are part of the case; steps of 4 keep every frame in)
    assert status == [0] * len(chunks) or "x9" in name

    def run(mode):
        got = _stream(ctx, pkg, chunks, w, h, tables, None, lam)
        _check(got, want, status, "%s, lambda %d, %s" % (name, lam, mode))
        assert got[4] == err, "%s, lambda %d, %s: d_err" % (name, lam, mode)
    both_modes(run)


@pytest.mark.parametrize("name", list(SHAPES))
def test_probe_bits(ctx, pkg, both_modes, name):
    w, h, chunks, tables = chunks_of(name)
    want = RT.bits_table(chunks, w, h, tables, None, RT.LADDER)

    def run(mode):
        got = _probe(ctx, pkg, chunks, w, h, tables, None, RT.LADDER)
        assert (got == want).all(), "%s %s: %s" % (name, mode, np.argwhere(got != want)[:6].tolist())
    both_modes(run)


@pytest.mark.parametrize("name", ["16x16 x 130", "130x98, Q60", "clip"])
def test_amvs_own_tables_are_requant_byte_for_byte(ctx, pkg, amv1, both_modes, name):
    """the same context, the same chunks: every output of the stream, probe and rate entries equals the requant sibling's (the
    error too: the DC is carried and adds nothing)"""
    if name == "clip":
        w, h, chunks = amv1["info"]["width"], amv1["info"]["height"], [bytes(c) for c in amv1["video"]][:12]
    else:
        w, h, chunks, _ = chunks_of(name)
    tables = [RT.AMV_TABLES]
    cap = sum(len(c) for c in chunks) + 64
    budget = int(np.median([len(c) for c in chunks])) - 8

    def run(mode):
        for lam in (0, 3481):
            a, b = _stream(ctx, pkg, chunks, w, h, tables, None, lam, cap=cap), TQ._stream(ctx, chunks, w, h, lam, cap=cap)
            assert all((x == y).all() for x, y in zip(a[:4], b[:4])) and a[4] == b[4], "%s, lambda %d, %s" % (name, lam, mode)
            assert (a[3] == 0).all()
        assert (_probe(ctx, pkg, chunks, w, h, tables, None, Q.LADDER) == TQ._probe(ctx, chunks, w, h, Q.LADDER)).all(), mode
        a, b = _rate(ctx, pkg, chunks, w, h, tables, None, Q.LADDER, budget, cap=cap), TQ._rate(ctx, pkg, chunks, w, h, Q.LADDER, budget, cap=cap)
        assert all((x == y).all() for x, y in zip(a, b)), "%s, rate, %s" % (name, mode)
    both_modes(run)


def test_three_tables_over_the_frames_and_a_bad_index(ctx, pkg, both_modes):
    """the reference's rate-controlled runs vary qscale per frame: chunks written at -qscale 2, 8, 31 in turn, named by
    d_table_of; frame 4 names table 3 of three"""
    w, h = 48, 32
    frames = N.stream(w, h, KINDS, 100)
    per_q = {q: RT.reference_chunks(frames, w, h, q) for q in (2, 8, 31)}
    tables = [RT.reference_tables(q) for q in (2, 8, 31)]
    table_of = [0, 1, 2, 0, 3, 2]
    chunks = [per_q[(2, 8, 31)[t % 3]][i] for i, t in enumerate(table_of)]
    model = {lam: RT.retable(chunks, w, h, tables, table_of, lam) for lam in (0, 3481)}
    assert model[0][1] == [0, 0, 0, 0, RT.ST_TABLE, 0]
    alone = [RT.retable([chunks[i]], w, h, [tables[table_of[i]]], None, 3481)[0][0] for i in (0, 1, 2)]
    assert alone == model[3481][0][:3]
    bits = RT.bits_table(chunks, w, h, tables, table_of, RT.LADDER)
    budget = int(np.median([len(c) for c in model[3481][0] if c]))
    want_rate = RT.rate(chunks, w, h, tables, table_of, RT.LADDER, budget)

    def run(mode):
        for lam in (0, 3481):
            got = _stream(ctx, pkg, chunks, w, h, tables, table_of, lam)
            _check(got, model[lam][0], model[lam][1], "three tables, lambda %d, %s" % (lam, mode))
            assert got[4] == model[lam][2], mode
        assert (_probe(ctx, pkg, chunks, w, h, tables, table_of, RT.LADDER) == bits).all() and (bits[4] == 0).all(), mode
        got = _rate(ctx, pkg, chunks, w, h, tables, table_of, RT.LADDER, budget)
        _check(got, want_rate[0], want_rate[1], "three tables, rate, %s" % mode)
        assert list(got[4]) == want_rate[2] and got[4][4] == (4 | RT.OVER), mode
        # every index bad, and the largest one a byte holds
        got = _stream(ctx, pkg, chunks[:2], w, h, tables, [3, 255], 0)
        _check(got, [None, None], [RT.ST_TABLE] * 2, "bad indices, %s" % mode)
    both_modes(run)


# ---- crafted scans ----------------------------------------------------------------------------------------------------------------

CRAFTED_TABLES = [RT.reference_tables(5), FOURS, RT.reference_tables(8), ALL_1, ALL_255, [[9] + [16] * 63, [4] + [16] * 63], [[1] + [16] * 63] * 2]


def crafted():
    """-> [(what, table index, chunk)] of 16x16 frames made with scan_builder: the edges of each range rule and one step over,
    the DC's ties, steps of 1 and of 255, damaged chunks"""
    out = []
    ref5 = CRAFTED_TABLES[0]
    for comp, at in ((0, 2), (1, 4)):
        for k in (1, 6, 33, 63):
            most = RT.COEF_MOST // (8 * ref5[comp][k])
            out.append(("level at the cap, %d %d" % (comp, k), 0, N._chunk(TQ._frame(Q.block_of({k: -most, 2: 1}), at=at))))
            out.append(("level over the cap, %d %d" % (comp, k), 0, N._chunk(TQ._frame(Q.block_of({k: most + 1, 2: 1}), at=at))))
    out.append(("at the energy cap", 1, N._chunk(TQ._frame(Q.block_of({k: 256 if k & 1 else -256 for k in range(1, 17)}, dc=-2000), at=3))))
    out.append(("over the energy cap", 1, N._chunk(TQ._frame(Q.block_of({**{k: 256 for k in range(1, 17)}, 17: 1}), at=3))))
    out.append(("new DC at its edge", 2, N._chunk(TQ._frame(Q.block_of({1: 1}, dc=-1151), at=4))))
    out.append(("new DC over its edge", 2, N._chunk(TQ._frame(Q.block_of({1: 1}, dc=1152), at=5))))
    out.append(("new DC at its edge, luma", 2, N._chunk(TQ._frame(Q.block_of({1: 1}, dc=1023), at=0))))
    out.append(("new DC over its edge, luma", 2, N._chunk(TQ._frame(Q.block_of({1: 1}, dc=-1024), at=1))))
    for sign in (1, -1):
        lines = np.zeros((6, 64), np.int16)
        lines[:, 0] = [4 * sign, -12 * sign, 100 * sign, -28 * sign, 9 * sign, -27 * sign]     # 9 against 8: 36/8, 108/8, 900/8, 252/8; 4 against 9: 36/9 = 4, 108/9
        lines[:, 1] = 3
        out.append(("DC ties, 9 and 4, sign %d" % sign, 5, N._chunk(lines)))
        lines = lines.copy()
        lines[:, 0] = [4 * sign, -12 * sign, 20 * sign, -1 * sign, 9 * sign, -27 * sign]       # 1 against 8: 4/8, 12/8, 20/8 are ties; 1 against 9: 9/9, 27/9
        out.append(("DC ties, 1, sign %d" % sign, 6, N._chunk(lines)))
    out.append(("steps of 1", 3, N._chunk(TQ._frame(Q.block_of({1: 100, 2: -3, 63: 1023}, dc=80), at=2))))
    out.append(("steps of 255", 4, N._chunk(TQ._frame(Q.block_of({1: 4, 5: -1}, dc=-3), at=5))))
    out.append(("steps of 255, over", 4, N._chunk(TQ._frame(Q.block_of({1: 5}), at=1))))
    whole = sb.blocks_from_coefficients(TQ._frame(Q.block_of({k: 1 + k % 5 for k in range(1, 40)}), at=2))
    full = sb.assemble(whole)
    out.append(("truncated", 0, sb.assemble(whole, cut_bit=full.nbits // 2).chunk))
    bad = list(whole)
    bad[3] = (bad[3][0], ["1" * 16], True)
    out.append(("a bad code", 7, sb.assemble(bad).chunk))                       # (its index is bad too: the decode's word stands)
    out.append(("a plain frame", 2, N._chunk(TQ._frame(Q.block_of({k: 1 + k % 5 for k in range(1, 40)}), at=2))))
    return out


def test_crafted_scans(ctx, pkg, both_modes):
    cases = crafted()
    names, table_of, chunks = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    w = h = 16
    at = {name: i for i, name in enumerate(names)}
    model = {lam: RT.retable(chunks, w, h, CRAFTED_TABLES, table_of, lam) for lam in (0, 3481)}
    status = model[0][1]
    not_coded = [n for n in names if status[at[n]]]
    over = [n for n in names if " over " in n or n.startswith("over ") or n.endswith(", over")]
    assert sorted(not_coded) == sorted(over + ["truncated", "a bad code"]) and len(over) == 12
    assert all(status[at[n]] == RT.ST_RANGE for n in over) and status[at["truncated"]] & RT.ST_TRUNCATED
    assert status[at["a bad code"]] not in (0, RT.ST_TABLE, RT.ST_RANGE)
    # the ties went away from zero, the edges were met
    lines = Q.decode(model[0][0][at["DC ties, 9 and 4, sign 1"]], w, h)[0]
    assert lines[:, 0].tolist() == [5, -14, 113, -32, 4, -12]
    lines = Q.decode(model[0][0][at["DC ties, 1, sign -1"]], w, h)[0]
    assert lines[:, 0].tolist() == [-1, 2, -3, 0, -1, 3]
    assert Q.decode(model[0][0][at["new DC at its edge"]], w, h)[0][4][0] == -1023
    assert Q.decode(model[0][0][at["at the energy cap"]], w, h)[0][3][0] == -1000
    bits = RT.bits_table(chunks, w, h, CRAFTED_TABLES, table_of, RT.LADDER)
    assert all((bits[at[n]] == 0).all() for n in not_coded)
    budget = int(np.median([len(c) for c in model[0][0] if c])) - 1
    want_rate = RT.rate(chunks, w, h, CRAFTED_TABLES, table_of, RT.LADDER, budget)
    assert len(set(want_rate[2])) >= 3

    def run(mode):
        for lam in (0, 3481):
            got = _stream(ctx, pkg, chunks, w, h, CRAFTED_TABLES, table_of, lam)
            _check(got, model[lam][0], status, "crafted, lambda %d, %s" % (lam, mode))
            assert got[4] == model[lam][2], "crafted, lambda %d, %s: d_err" % (lam, mode)
        assert (_probe(ctx, pkg, chunks, w, h, CRAFTED_TABLES, table_of, RT.LADDER) == bits).all(), mode
        got = _rate(ctx, pkg, chunks, w, h, CRAFTED_TABLES, table_of, RT.LADDER, budget)
        _check(got, want_rate[0], want_rate[1], "crafted, rate, %s" % mode)
        assert list(got[4]) == want_rate[2], mode
        assert all(got[4][at[n]] == (4 | RT.OVER) and got[3][at[n]] for n in not_coded)
    both_modes(run)


def test_two_rounds_of_the_workspace(ctx, pkg, both_modes):
    """16x16 x 1030: a round of the coefficient workspace holds 1 024 frames, so the last six -- a truncated one, one out of
    range and one with a bad index among them -- go through a second round (the model sees 130 distinct chunks)"""
    w, h, chunks, tables = chunks_of("16x16 x 130")
    cases = {c[0]: c[2] for c in crafted()}
    many = [chunks[i % 130] for i in range(1030)]
    many[1025] = cases["truncated"]
    many[1027] = N._chunk(TQ._frame(Q.block_of({1: 400}), at=2))               # 400 * 8 * 9 = 28 800
    table_of = [0] * 1030
    table_of[1028] = 1
    want, status, err = RT.retable(many, w, h, tables, table_of, 3481)
    assert [i for i, s in enumerate(status) if s] == [1025, 1027, 1028] and status[1027:1029] == [RT.ST_RANGE, RT.ST_TABLE]
    ladder = [0, 20000]
    budget = int(np.median([len(c) for c in want if c]))
    want_rate = RT.rate(many, w, h, tables, table_of, ladder, budget)
    assert {0, 1, 1 | RT.OVER} <= set(want_rate[2])

    def run(mode):
        got = _stream(ctx, pkg, many, w, h, tables, table_of, 3481)
        _check(got, want, status, "two rounds, %s" % mode)
        assert got[4] == err
        got = _rate(ctx, pkg, many, w, h, tables, table_of, ladder, budget)
        _check(got, want_rate[0], want_rate[1], "two rounds, rate, %s" % mode)
        assert list(got[4]) == want_rate[2]
    both_modes(run)


# ---- rate and clip ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["qscale 2", "qscale 31", "131x97, Q60"])
def test_rate(ctx, pkg, both_modes, name):
    """a uniform budget; a d_budget array cycling a middle rung's length, that less one, 7 (nothing fits) and 2^32 - 1 (rung 0)"""
    w, h, chunks, tables = chunks_of(name)
    n = len(chunks)
    table = [RT.retable(chunks, w, h, tables, None, lam)[0] for lam in RT.LADDER]
    lens = np.array([[len(table[r][i] or b"") for r in range(len(RT.LADDER))] for i in range(n)])
    kinds = [lambda i: int(lens[i][2]), lambda i: max(int(lens[i][2]) - 1, 0), lambda i: 7, lambda i: 0xFFFFFFFF]
    per_frame = [kinds[i % 4](i) for i in range(n)]
    cases = [("uniform", RT.LADDER, int(np.median(lens[:, 2]))), ("per frame", RT.LADDER, per_frame), ("descending", RT.LADDER[::-1], int(np.median(lens[:, 2])))]

    def run(mode):
        for kind, ladder, B in cases:
            want, status, rungs = RT.rate(chunks, w, h, tables, None, ladder, B)
            got = _rate(ctx, pkg, chunks, w, h, tables, None, ladder, B)
            what = "%s, %s, %s" % (name, kind, mode)
            _check(got, want, status, what)
            assert list(got[4]) == rungs, "%s: rungs %s, want %s" % (what, [hex(int(x)) for x in got[4]], [hex(x) for x in rungs])
    both_modes(run)


def test_clip(ctx, pkg, both_modes):
    """chunks of the reference's encoder at -qscale 2 with a damaged frame and a bad index among them, at every S(c), that less
    one, and every F(c): d_clip, d_rung and the chunks are the model's, and the rate entry's on the ladder's tail"""
    w, h, chunks, tables = chunks_of("qscale 2")
    chunks = list(chunks)
    chunks[2] = chunks[2][: len(chunks[2]) // 2]
    table_of = [0, 0, 0, 0, 1, 0]
    lens, coded = RT.clip_lens(chunks, w, h, tables, table_of, RT.LADDER)
    bits = RT.bits_table(chunks, w, h, tables, table_of, RT.LADDER)
    assert [i for i in range(6) if not coded[i]] == [2, 4]
    S, F = C.sums(lens, C.NO_CAP, coded), C.floor_sums(bits, C.NO_CAP, coded)
    cases = [(C.NO_CAP, total) for total in sorted({x - d for x in S for d in (0, 1)} | set(F) | {0, C.U64_MAX})]
    cap_per_frame = int(np.median(lens[:, 1]))
    cases += [(cap_per_frame, total) for total in sorted({x - d for x in C.sums(lens, cap_per_frame, coded)[:3] for d in (0, 1)})]
    want = [RT.clip(chunks, w, h, tables, table_of, RT.LADDER, B, total) for B, total in cases]
    assert len({x[3][0] for x in want}) >= 4 and any(x[3][0] & R.OVER for x in want)

    def run(mode):
        for (B, total), (out, status, rungs, clip) in zip(cases, want):
            what = "clip, cap %d, total %d, %s" % (B, total, mode)
            got = _clip(ctx, pkg, chunks, w, h, tables, table_of, RT.LADDER, B, total)
            assert got[5] == list(clip), "%s: d_clip %s, want %s" % (what, got[5], clip)
            _check(got, out, status, what)
            assert list(got[4]) == rungs and got[3][4] == RT.ST_TABLE, what
            assert all(got[4][i] == (4 | R.OVER) and got[3][i] and got[2][i] == 0 for i in (2, 4)), what
            c = clip[0] & ~R.OVER
            tail = _rate(ctx, pkg, chunks, w, h, tables, table_of, RT.LADDER[c:], B)
            assert all((a == b).all() for a, b in zip(tail[:4], got[:4])), what
            assert [((int(r) & ~R.OVER) + c) | (int(r) & R.OVER) for r in tail[4]] == list(got[4]), what
    both_modes(run)


def test_blob_one_byte_short(ctx, pkg, both_modes):
    w, h, chunks, tables = chunks_of("16x16 x 130")
    want, status, _ = RT.retable(chunks, w, h, tables, None, 3481)
    sizes = [len(c) for c in want]
    cap = sum(sizes[:70]) + sizes[70] - 1                      # chunk 70 ends one byte past it

    def run(mode):
        got = _stream(ctx, pkg, chunks, w, h, tables, None, 3481, cap=cap, want_err=False)
        _check(got, want, status, "capacity, %s" % mode, cap=cap)
        assert (got[2][:70] > 0).all() and (got[2][70:] == 0).all()
        got = _rate(ctx, pkg, chunks, w, h, tables, None, [3481, 3481], 0xFFFFFFFF, cap=cap)
        _check(got, want, status, "capacity, rate, %s" % mode, cap=cap)
        assert (got[4] == 0).all()
        total = sum(sizes)
        got = _clip(ctx, pkg, chunks, w, h, tables, None, [3481, 20000], C.NO_CAP, total, cap=total - 1)
        assert got[5] == [0, total] and (got[4] == 0).all() and int(got[2][-1]) == 0 and (got[2][:-1] > 0).all()
        _check(got, want, status, "capacity, clip, %s" % mode, cap=total - 1)
    both_modes(run)


# ---- refusals, and the workspace shared with the other entries ------------------------------------------------------------------------

def test_refusals(ctx, pkg):
    import torch
    w, h, chunks, tables = chunks_of("16x16 x 3")
    d_blob, blob_bytes, d_offs, d_lens, n = TQ._inputs(chunks)
    cap = 4096
    out, out_offs, out_lens, status = TQ._outs(n, cap)
    words = torch.full((n * 16 + 4,), UNWRITTEN, dtype=torch.int32, device="cuda:0")
    err = torch.zeros((n * 3 + 1,), dtype=torch.int64, device="cuda:0")
    d_clip = _t(np.full(3, CLIP_UNWRITTEN, np.uint64))
    L, h_ = ctx.lib, ctx.h
    p = lambda t, off=0: None if t is None else t.data_ptr() + off  # noqa: E731
    a = lambda s: None if s is None else ctypes.addressof(s)  # noqa: E731
    E = pkg.ERR_ARG
    good = pkg.Retable(tables)
    zero = [[list(t) for t in tables[0]]]
    zero[0][1][63] = 0
    bad_tables = [None, pkg.Retable(None, count=1), pkg.Retable(tables, count=0), pkg.Retable(tables * 65), pkg.Retable(zero),
                  pkg.Retable([RT.AMV_TABLES, zero[0]])]
    ladder = (ctypes.c_uint32 * 17)(*([3481] * 17))
    high = (ctypes.c_uint32 * 2)(0, RT.LAMBDA_MAX + 1)

    def stream(rt=good, blob=d_blob, offs=d_offs, lens=d_lens, n_=n, w_=w, h_2=h, lam=0, o=out, oo=out_offs, ol=out_lens, st=status, e=None, off={}):
        return L.amvhip_retable_stream_dev(h_, p(blob, off.get("blob", 0)), blob_bytes, p(offs, off.get("offs", 0)), p(lens, off.get("lens", 0)),
                                           n_, w_, h_2, a(rt), lam, p(o), cap, p(oo, off.get("oo", 0)), p(ol, off.get("ol", 0)),
                                           p(st, off.get("st", 0)), p(e, off.get("e", 0)), None)

    def probe(rt=good, lad=ladder, rungs=2, bits=words, w_=w, h_2=h, n_=n, off=0):
        return L.amvhip_retable_rate_probe_dev(h_, p(d_blob), blob_bytes, p(d_offs), p(d_lens), n_, w_, h_2, a(rt), a(lad), rungs, p(bits, off), None)

    def rate(r, rt=good, rung=words, off=0, w_=w, h_2=h, n_=n):
        return L.amvhip_retable_rate_stream_dev(h_, p(d_blob), blob_bytes, p(d_offs), p(d_lens), n_, w_, h_2, a(rt), a(r), p(out), cap, p(out_offs),
                                                p(out_lens), p(status), p(rung, off), None)

    def clip(r, rt=good, rung=words, clip_=d_clip, off=0, n_=n):
        return L.amvhip_retable_clip_stream_dev(h_, p(d_blob), blob_bytes, p(d_offs), p(d_lens), n_, w, h, a(rt), a(r), 1000, p(out), cap,
                                                p(out_offs), p(out_lens), p(status), p(rung), p(clip_, off), None)

    plain = pkg.Rate([0, 3481], budget=100)
    # what the re-table form adds: every entry, n == 0 included
    for rt in bad_tables:
        assert stream(rt=rt) == E and probe(rt=rt) == E and rate(plain, rt=rt) == E and clip(plain, rt=rt) == E, rt and rt.count
        assert stream(rt=rt, n_=0) == E and probe(rt=rt, n_=0) == E
    assert stream(rt=pkg.Retable(zero)) == E and "step of 0" in L.amvhip_last_error(h_).decode()
    assert stream(rt=pkg.Retable(tables * 64)) == 0
    # what the siblings refuse
    assert stream(blob=None) == E and stream(offs=None) == E and stream(lens=None) == E and stream(st=None) == E
    assert stream(o=None) == E and stream(oo=None) == E and stream(ol=None) == E
    for key in ("blob", "offs", "lens", "oo", "ol", "st"):
        assert stream(off={key: 2}) == E, key
    assert stream(e=err, off={"e": 4}) == E
    assert stream(lam=RT.LAMBDA_MAX + 1) == E and "amvhip_encode_trellis_lambda_max" in L.amvhip_last_error(h_).decode()
    assert stream(w_=0) == E and stream(h_2=16385) == E
    assert stream(n_=0, blob=None, offs=None, lens=None, o=None, oo=None, ol=None, st=None) == 0
    assert probe(lad=None) == E and probe(rungs=0) == E and probe(rungs=17) == E and probe(bits=None) == E and probe(off=2) == E
    assert probe(lad=high) == E and probe(w_=16384, h_2=16384) == E and "blocks" in L.amvhip_last_error(h_).decode()
    assert probe(n_=0, bits=None) == 0
    assert rate(None) == E and rate(pkg.Rate(None, budget=1, rungs=2)) == E and rate(pkg.Rate([1], budget=1, rungs=0)) == E
    assert rate(pkg.Rate([1] * 16, budget=1, rungs=17)) == E and rate(pkg.Rate([0, RT.LAMBDA_MAX + 1], budget=1)) == E
    assert rate(plain, rung=None) == E and rate(plain, off=2) == E and rate(pkg.Rate([0], budget=1, d_budget=words.data_ptr() + 2)) == E
    assert rate(plain, w_=16384, h_2=16384) == E and rate(plain, n_=0) == 0
    assert clip(None) == E and clip(plain, clip_=None) == E and clip(plain, off=4) == E and clip(plain, rung=None) == E and clip(plain, n_=0) == 0
    torch.cuda.synchronize()
    # nothing was queued by a refused call: the one good stream call wrote its outputs, nothing else was touched
    assert (words.cpu().numpy().view(np.uint32) == UNWRITTEN).all() and (d_clip.cpu().numpy() == CLIP_UNWRITTEN).all()
    assert (status.cpu().numpy() == 0).all() and (err.cpu().numpy() == 0).all()
    want = RT.retable(chunks, w, h, tables, None, 0)
    TQ._check((out.cpu().numpy()[:cap + 64], out_offs.cpu().numpy(), out_lens.cpu().numpy(), status.cpu().numpy()), want[0], want[1], "the good call")


def test_the_other_entries_after_a_retable_call(ctx, pkg, orc):
    """the coefficient workspace, the record set, the flags and the rate workspace are shared: the decoder and the requant
    entries give the bytes they gave before a re-table call on the same context"""
    import torch
    w, h = 48, 32
    chunks = Q.synth_chunks(w, h, 3)

    def decode():
        d_blob, blob_bytes, d_offs, d_lens, n = TQ._inputs(chunks)
        out = torch.zeros((n, h, orc.stride(w)), dtype=torch.uint8, device="cuda:0")
        st = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
        ctx.decode_batch_dev(d_blob, blob_bytes, d_offs, d_lens, n, w, h, 0, out, st)
        torch.cuda.synchronize()
        return out.cpu().numpy(), st.cpu().numpy()

    def requant():
        got = TQ._stream(ctx, chunks, w, h, 3481)
        rate = TQ._rate(ctx, pkg, chunks, w, h, Q.LADDER, 300)
        return [x.tolist() if hasattr(x, "tolist") else x for x in got + rate]

    before = (decode(), requant())
    bw, bh, big, tables = chunks_of("130x98, Q60")
    _rate(ctx, pkg, big, bw, bh, tables, None, RT.LADDER, 500)
    _stream(ctx, pkg, big, bw, bh, tables, [0, 1], 3481)                       # (one bad index: its flag must not outlive the call)
    after = (decode(), requant())
    assert (before[0][0] == after[0][0]).all() and (before[0][1] == after[0][1]).all() and before[1] == after[1]
    blob, offs, lens = Q.pack(chunks)
    want, st = orc.decode_batch(blob, offs, lens, w, h)
    assert (after[0][0] == want).all() and (after[0][1] == st).all()
    model = Q.requant(chunks, w, h, 3481)
    TQ._check(TQ._stream(ctx, chunks, w, h, 3481), model[0], model[1], "requant after retable")


def test_every_written_chunk_decodes(ctx, pkg, orc):
    """what the entries write is AMV: the chunks of the reference's encoder at -qscale 2 and 31, re-tabled at three lambdas, decode
    cleanly on the device and in the oracle, to the oracle's picture; and above what the source chunk decodes to, against the
    picture it was made from"""
    import torch
    w, h = 48, 32
    frames = N.stream(w, h, KINDS, 100)
    for q in (2, 31):
        chunks = RT.reference_chunks(frames, w, h, q)
        for lam in (0, 3481, RT.LAMBDA_MAX):
            blob, offs, lens, status, _ = _stream(ctx, pkg, chunks, w, h, [pkg.ffmpeg_amv_tables(q)], None, lam)
            assert (status == 0).all() and (lens > 0).all()
            n = len(chunks)
            out = torch.zeros((n, h, orc.stride(w)), dtype=torch.uint8, device="cuda:0")
            st = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
            ctx.decode_batch_dev(_t(blob), int(lens.sum()), _t(offs.astype(np.uint64)), _t(lens.astype(np.uint32)), n, w, h, 0, out, st)
            torch.cuda.synchronize()
            assert (st.cpu().numpy() == 0).all()
            for i in range(n):
                chunk = blob[int(offs[i]): int(offs[i]) + int(lens[i])].tobytes()
                want, wst, ok = orc.decode_frame(chunk, w, h)
                assert wst == 0 and ok == orc.nmcu(w, h) and (out[i].cpu().numpy() == want).all()
                if KINDS[i] != "flat" and lam != RT.LAMBDA_MAX:
                    assert RT.decode_psnr(chunk, frames[i], w, h) > RT.decode_psnr(chunks[i], frames[i], w, h)
