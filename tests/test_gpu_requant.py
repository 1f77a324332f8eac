"""AMV chunks requantised in the coefficient domain (amvhip_requant_stream_dev, amvhip_requant_rate_probe_dev,
amvhip_requant_rate_stream_dev) on a real MI355X against tests/requant_ref.py: every frame of every case, d_out, the offsets,
the lengths, d_status, d_err, d_bits and d_rung, bytes against bytes and words against words, in both entropy modes.

Shapes are the smallest that reach each path: 16x16 (one MCU) x 1, 3 and 130 (the coder's lane per frame spans two waves and a
tail), 32x16, 176x144 (eleven MCUs a row: segments of 6 and 5), 160x120 and 130x98 (a partial last MCU row, a size that is no
multiple of the MCU), 131x97 (odd both ways: the chunks of 132x98), the first and the last 12 chunks of the reference clip.  The
model's tables are made once per input and shared (requant_ref caches frames and blocks)."""
import numpy as np
import pytest

import nr_ref as N
import rate_ref as R
import requant_ref as Q
import scan_builder as sb
import trellis_ref as T
from test_gpu_encode_nr_trellis import FILL, both_modes  # noqa: F401  (both_modes is a fixture)
from test_gpu_parity import _t

pytestmark = pytest.mark.gpu

UNWRITTEN = 0x5A5A5A5A
SHAPES = {"16x16 x 1": (16, 16, 1), "16x16 x 3": (16, 16, 3), "16x16 x 130": (16, 16, 130), "32x16": (32, 16, 3), "176x144": (176, 144, 2),
          "160x120": (160, 120, 2), "130x98": (130, 98, 2), "131x97": (131, 97, 2), "clip, first 12": (128, 96, 12), "clip, last 12": (128, 96, 12)}
_CHUNKS = {}


def chunks_of(name, amv1):
    if name not in _CHUNKS:
        w, h, n = SHAPES[name]
        if name.startswith("clip"):
            video = [bytes(c) for c in amv1["video"]]
            _CHUNKS[name] = video[:n] if "first" in name else video[-n:]
        else:
            _CHUNKS[name] = Q.synth_chunks(w + (w & 1), h + (h & 1), n, seed=0xC0FFEE + w)
    return SHAPES[name][0], SHAPES[name][1], _CHUNKS[name]


def _inputs(chunks):
    blob, offs, lens = Q.pack(chunks)
    return _t(blob), int(lens.sum()), _t(offs), _t(lens), len(chunks)


def _outs(n, cap):
    import torch
    return (torch.full((cap + 64,), FILL, dtype=torch.uint8, device="cuda:0"), torch.full((n,), -1, dtype=torch.int64, device="cuda:0"),
            torch.full((n,), -1, dtype=torch.int32, device="cuda:0"), torch.full((n,), UNWRITTEN, dtype=torch.int32, device="cuda:0"))


def _stream(ctx, chunks, w, h, lam, cap=None, want_err=True):
    """-> (blob, offs, lens, status, err or None)"""
    import torch
    d_blob, blob_bytes, d_offs, d_lens, n = _inputs(chunks)
    cap = sum(len(c) for c in chunks) + 64 if cap is None else cap
    out, out_offs, out_lens, status = _outs(n, cap)
    err = torch.full((n, 3), -1, dtype=torch.int64, device="cuda:0") if want_err else None
    ctx.requant_stream_dev(d_blob, blob_bytes, d_offs, d_lens, n, w, h, lam, out, cap, out_offs, out_lens, status, err)
    torch.cuda.synchronize()
    return (out.cpu().numpy(), out_offs.cpu().numpy(), out_lens.cpu().numpy(), status.cpu().numpy(),
            err.cpu().numpy().tolist() if want_err else None)


def _probe(ctx, chunks, w, h, ladder):
    import torch
    d_blob, blob_bytes, d_offs, d_lens, n = _inputs(chunks)
    bits = torch.full((n, len(ladder)), UNWRITTEN, dtype=torch.int32, device="cuda:0")
    ctx.requant_rate_probe_dev(d_blob, blob_bytes, d_offs, d_lens, n, w, h, ladder, bits)
    torch.cuda.synchronize()
    return bits.cpu().numpy().view(np.uint32).astype(np.int64)


def _rate(ctx, pkg, chunks, w, h, ladder, budgets, cap=None):
    """budgets: a list (handed over as d_budget) or one number -> (blob, offs, lens, status, rungs)"""
    import torch
    d_blob, blob_bytes, d_offs, d_lens, n = _inputs(chunks)
    cap = sum(len(c) for c in chunks) + 64 if cap is None else cap
    out, out_offs, out_lens, status = _outs(n, cap)
    rung = torch.full((n,), UNWRITTEN, dtype=torch.int32, device="cuda:0")
    if np.isscalar(budgets):
        rate = pkg.Rate(ladder, budget=int(budgets))
    else:
        d_budget = _t(np.asarray(budgets, np.uint32))
        rate = pkg.Rate(ladder, budget=1, d_budget=d_budget)
    ctx.requant_rate_stream_dev(d_blob, blob_bytes, d_offs, d_lens, n, w, h, rate, out, cap, out_offs, out_lens, status, rung)
    torch.cuda.synchronize()
    return (out.cpu().numpy(), out_offs.cpu().numpy(), out_lens.cpu().numpy(), status.cpu().numpy(),
            rung.cpu().numpy().view(np.uint32).astype(np.int64))


def _check(got, want, want_status, what, cap=None):
    """chunks back to back; a frame that is not coded (None) has no bytes and length 0; a chunk that would end past cap is
    not written, its length 0, its offset the scan's all the same"""
    blob, offs, lens, status = got[:4]
    assert [int(s) for s in status] == list(want_status), "%s: status %s, want %s" % (what, list(status), list(want_status))
    pos, end = 0, 0
    for i, c in enumerate(want):
        size = 0 if c is None else len(c)
        fits = cap is None or pos + size <= cap
        assert (int(offs[i]), int(lens[i])) == (pos, size if fits else 0), "%s: frame %d at %d + %d, want %d + %d" % (what, i, offs[i], lens[i], pos, size)
        if size and fits:
            assert blob[pos: pos + size].tobytes() == c, "%s: frame %d differs" % (what, i)
            end = pos + size
        pos += size
    assert (blob[end:] == FILL).all(), "%s: bytes behind the last chunk were written" % what


# ---- the three entries on every shape -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lam", [0, 3481, Q.LAMBDA_MAX])
@pytest.mark.parametrize("name", list(SHAPES))
def test_stream(ctx, amv1, both_modes, name, lam):
    w, h, chunks = chunks_of(name, amv1)
    want, status, err = Q.requant(chunks, w, h, lam)
    assert status == [0] * len(chunks)
    if lam == 0:
        assert want == chunks

    def run(mode):
        got = _stream(ctx, chunks, w, h, lam)
        _check(got, want, status, "%s, lambda %d, %s" % (name, lam, mode))
        assert got[4] == err, "%s, lambda %d, %s: d_err" % (name, lam, mode)
    both_modes(run)


@pytest.mark.parametrize("name", list(SHAPES))
def test_probe_bits(ctx, amv1, both_modes, name):
    w, h, chunks = chunks_of(name, amv1)
    want = Q.bits_table(chunks, w, h, Q.LADDER)

    def run(mode):
        got = _probe(ctx, chunks, w, h, Q.LADDER)
        assert (got == want).all(), "%s %s: %s" % (name, mode, np.argwhere(got != want)[:6].tolist())
    both_modes(run)


def _tables(chunks, w, h, ladder):
    table = [Q.requant(chunks, w, h, lam)[0] for lam in ladder]
    lens = np.array([[len(table[r][i]) for r in range(len(ladder))] for i in range(len(chunks))])
    esc = np.array([[R.escapes(table[r][i]) for r in range(len(ladder))] for i in range(len(chunks))])
    return Q.bits_table(chunks, w, h, ladder), lens, esc


@pytest.mark.parametrize("name", list(SHAPES))
def test_rate(ctx, pkg, amv1, both_modes, name):
    """a uniform budget; a d_budget array cycling a middle rung's length, that less one, the floor of a rung with escapes (it
    floor-fits and need not fit: the redo path), 7 (nothing fits) and 2^32 - 1 (rung 0, whose lambda is 0: the frame as it
    is); a descending ladder; a budget nothing fits"""
    w, h, chunks = chunks_of(name, amv1)
    n = len(chunks)
    bits, lens, esc = _tables(chunks, w, h, Q.LADDER)
    with_escapes = [next((r for r in range(lens.shape[1]) if esc[i][r]), 2) for i in range(n)]
    kinds = [lambda i: int(lens[i][2]), lambda i: int(lens[i][2]) - 1, lambda i: R.floor_bytes(int(bits[i][with_escapes[i]])), lambda i: 7,
             lambda i: 0xFFFFFFFF]
    per_frame = [kinds[i % 5](i) for i in range(n)]
    cases = [("uniform", Q.LADDER, int(np.median(lens[:, 2]))), ("per frame", Q.LADDER, per_frame),
             ("descending", Q.LADDER[::-1], int(np.median(lens[:, 2]))), ("nothing fits", Q.LADDER, 7)]

    def run(mode):
        for kind, ladder, B in cases:
            want, status, rungs = Q.rate(chunks, w, h, ladder, B)
            got = _rate(ctx, pkg, chunks, w, h, ladder, B)
            what = "%s, %s, %s" % (name, kind, mode)
            _check(got, want, status, what)
            assert list(got[4]) == rungs, "%s: rungs %s, want %s" % (what, [hex(int(x)) for x in got[4]], [hex(x) for x in rungs])
            if kind == "nothing fits":
                assert all(r == (len(ladder) - 1) | Q.OVER for r in rungs)
    both_modes(run)
    want, _, rungs = Q.rate(chunks, w, h, Q.LADDER, per_frame)
    assert all(rungs[i] == 0 and want[i] == Q.requant([chunks[i]], w, h, 0)[0][0] for i in range(4, n, 5))


# ---- crafted scans ----------------------------------------------------------------------------------------------------------------

def _frame(block, at=0):
    """a 16x16 frame's six lines: `block` (64 levels) at place `at` of the MCU, small DCs elsewhere"""
    lines = np.zeros((6, 64), np.int16)
    lines[:, 0] = [5, -3, 7, 0, -9, 11]
    lines[at] = block
    return lines


def crafted():
    """-> [(what, chunk)] of 16x16 frames: every AC position alone, runs of 0 .. 61 between two levels (62: position 63 alone), a
    block coded to position 63, no AC at all, the edges of the range rule, damaged chunks, junk padding"""
    out = []
    for k in range(1, 64):
        out.append(("position %d alone" % k, N._chunk(_frame(Q.block_of({k: 3 if k % 2 else -2}, dc=k), at=k % 6))))
    for run in range(62):
        out.append(("a run of %d" % run, N._chunk(_frame(Q.block_of({1: -4, run + 2: 2}, dc=-run), at=run % 6))))
    out.append(("coded to position 63", N._chunk(_frame(Q.block_of({k: (1 + k % 3) * (-1) ** k for k in range(1, 64)}), at=1))))
    out.append(("coded to position 63, chroma", N._chunk(_frame(Q.block_of({k: 2 if k % 7 else -5 for k in range(1, 64)}), at=5))))
    out.append(("no AC", N._chunk(_frame(Q.block_of({}, dc=100)))))
    for comp, at in ((0, 2), (1, 4)):
        for k in (1, 6, 33, 63):
            most = Q.COEF_MOST // (8 * int(T.QUANT[comp][k]))
            out.append(("level at R, %d %d" % (comp, k), N._chunk(_frame(Q.block_of({k: -most, 2: 1}), at=at))))
            out.append(("level over R, %d %d" % (comp, k), N._chunk(_frame(Q.block_of({k: most + 1, 2: 1}), at=at))))
    out.append(("at the energy cap", N._chunk(_frame(Q.block_of(Q.AT_ENERGY_MOST, dc=-1023), at=3))))
    out.append(("over the energy cap", N._chunk(_frame(Q.block_of({**Q.AT_ENERGY_MOST, 59: 16}), at=3))))
    out.append(("DC at its edge", N._chunk(_frame(Q.block_of({1: 1}, dc=1023), at=4))))
    out.append(("DC over its edge", N._chunk(_frame(Q.block_of({1: 1}, dc=1024), at=4))))
    whole = sb.blocks_from_coefficients(_frame(Q.block_of({k: 1 + k % 5 for k in range(1, 40)}), at=2))
    full = sb.assemble(whole)
    out.append(("truncated", sb.assemble(whole, cut_bit=full.nbits // 2).chunk))
    bad = list(whole)
    bad[3] = (bad[3][0], ["1" * 16], True)
    out.append(("a bad code", sb.assemble(bad).chunk))
    out.append(("junk padding", sb.assemble(whole, pad="0").chunk))
    return out


def test_crafted_scans(ctx, pkg, both_modes):
    cases = crafted()
    names, chunks = [c[0] for c in cases], [c[1] for c in cases]
    w = h = 16
    at = {name: i for i, name in enumerate(names)}
    model = {lam: Q.requant(chunks, w, h, lam) for lam in (0, 3481)}
    status = model[0][1]
    not_coded = [n for n in names if status[at[n]]]
    assert sorted(not_coded) == sorted([n for n in names if n.startswith("level over R")] + ["over the energy cap", "DC over its edge", "truncated", "a bad code"])
    assert all(status[at[n]] == Q.ST_RANGE for n in not_coded if n not in ("truncated", "a bad code"))
    assert status[at["truncated"]] & Q.ST_TRUNCATED
    assert model[0][0][at["junk padding"]] != chunks[at["junk padding"]] and sb.assemble(sb.blocks_from_coefficients(
        Q.decode(chunks[at["junk padding"]], w, h)[0])).chunk == model[0][0][at["junk padding"]]
    # every other frame is its own canonical chunk; the neighbours of the frames that are not coded among them
    assert all(model[0][0][i] == chunks[i] for i, n in enumerate(names) if not status[i] and n != "junk padding")
    assert any(a != b for a, b in zip(model[0][0], model[3481][0]))
    bits = Q.bits_table(chunks, w, h, Q.LADDER)
    assert all((bits[at[n]] == 0).all() for n in not_coded)
    budget = int(np.median([len(c) for c in model[0][0] if c])) - 1     # half the frames must move up the ladder
    want_rate = Q.rate(chunks, w, h, Q.LADDER, budget)
    assert len(set(want_rate[2])) >= 4

    def run(mode):
        for lam in (0, 3481):
            got = _stream(ctx, chunks, w, h, lam)
            _check(got, model[lam][0], status, "crafted, lambda %d, %s" % (lam, mode))
            assert got[4] == model[lam][2], "crafted, lambda %d, %s: d_err" % (lam, mode)
        assert (_probe(ctx, chunks, w, h, Q.LADDER) == bits).all(), mode
        got = _rate(ctx, pkg, chunks, w, h, Q.LADDER, budget)
        _check(got, want_rate[0], want_rate[1], "crafted, rate, %s" % mode)
        assert list(got[4]) == want_rate[2], mode
        assert all(got[4][at[n]] == (4 | Q.OVER) and got[3][at[n]] for n in not_coded)
    both_modes(run)


def test_a_capacity_that_cuts_the_batch(ctx, pkg, amv1, both_modes):
    w, h, chunks = chunks_of("16x16 x 130", amv1)
    want, status, _ = Q.requant(chunks, w, h, 3481)
    sizes = [len(c) for c in want]
    cap = sum(sizes[:70]) + sizes[70] - 1                      # chunk 70 ends one byte past it

    def run(mode):
        got = _stream(ctx, chunks, w, h, 3481, cap=cap, want_err=False)
        _check(got, want, status, "capacity, %s" % mode, cap=cap)
        assert (got[2][:70] > 0).all() and (got[2][70:] == 0).all()
        ladder = [3481, 3481]
        got = _rate(ctx, pkg, chunks, w, h, ladder, 0xFFFFFFFF, cap=cap)
        _check(got, want, status, "capacity, rate, %s" % mode, cap=cap)
        assert (got[4] == 0).all()                             # d_rung is written for every frame
    both_modes(run)


def test_two_rounds_of_the_workspace(ctx, pkg, amv1, both_modes):
    """16x16 x 1030: a round of the coefficient workspace holds 1 024 frames, so the last six -- a truncated one and one out of
    range among them -- go through a second round (the model sees 130 distinct chunks: it is made once)"""
    w, h, chunks = chunks_of("16x16 x 130", amv1)
    cases = dict(crafted())
    many = [chunks[i % 130] for i in range(1030)]
    many[1025], many[1027] = cases["truncated"], cases["over the energy cap"]
    want, status, err = Q.requant(many, w, h, 3481)
    assert [i for i, s in enumerate(status) if s] == [1025, 1027]
    ladder = [0, 20000]
    budget = int(np.median([len(c) for c in chunks]))
    want_rate = Q.rate(many, w, h, ladder, budget)
    assert {0, 1, 1 | Q.OVER} <= set(want_rate[2])

    def run(mode):
        got = _stream(ctx, many, w, h, 3481)
        _check(got, want, status, "two rounds, %s" % mode)
        assert got[4] == err
        got = _rate(ctx, pkg, many, w, h, ladder, budget)
        _check(got, want_rate[0], want_rate[1], "two rounds, rate, %s" % mode)
        assert list(got[4]) == want_rate[2]
    both_modes(run)


# ---- refusals, and the workspace shared with the other entries ------------------------------------------------------------------------

def test_refusals(ctx, pkg, amv1):
    import torch
    w, h, chunks = chunks_of("16x16 x 3", amv1)
    d_blob, blob_bytes, d_offs, d_lens, n = _inputs(chunks)
    cap = 4096
    out, out_offs, out_lens, status = _outs(n, cap)
    words = torch.full((n * 16 + 4,), UNWRITTEN, dtype=torch.int32, device="cuda:0")
    err = torch.zeros((n * 3 + 1,), dtype=torch.int64, device="cuda:0")
    L, h_ = ctx.lib, ctx.h
    p = lambda t, off=0: None if t is None else t.data_ptr() + off  # noqa: E731
    import ctypes
    ladder = (ctypes.c_uint32 * 17)(*([3481] * 17))
    high = (ctypes.c_uint32 * 2)(0, Q.LAMBDA_MAX + 1)

    def stream(blob=d_blob, offs=d_offs, lens=d_lens, n_=n, w_=w, h_2=h, lam=0, o=out, oo=out_offs, ol=out_lens, st=status, e=None, off={}):
        return L.amvhip_requant_stream_dev(h_, p(blob, off.get("blob", 0)), blob_bytes, p(offs, off.get("offs", 0)), p(lens, off.get("lens", 0)),
                                           n_, w_, h_2, lam, p(o), cap, p(oo, off.get("oo", 0)), p(ol, off.get("ol", 0)), p(st, off.get("st", 0)),
                                           p(e, off.get("e", 0)), None)

    E = pkg.ERR_ARG
    assert stream(blob=None) == E and stream(offs=None) == E and stream(lens=None) == E and stream(st=None) == E
    assert stream(o=None) == E and stream(oo=None) == E and stream(ol=None) == E
    for key in ("blob", "offs", "lens", "oo", "ol", "st"):
        assert stream(off={key: 2}) == E, key
    assert stream(e=err, off={"e": 4}) == E
    assert stream(lam=Q.LAMBDA_MAX + 1) == E and "amvhip_encode_trellis_lambda_max" in L.amvhip_last_error(h_).decode()
    assert stream(w_=0) == E and stream(h_2=16385) == E
    assert stream(n_=0, blob=None, offs=None, lens=None, o=None, oo=None, ol=None, st=None) == 0

    def probe(lad=ladder, rungs=2, bits=words, w_=w, h_2=h, n_=n, off=0):
        return L.amvhip_requant_rate_probe_dev(h_, p(d_blob), blob_bytes, p(d_offs), p(d_lens), n_, w_, h_2, ctypes.addressof(lad) if lad else None,
                                               rungs, p(bits, off), None)

    assert probe(lad=None) == E and probe(rungs=0) == E and probe(rungs=17) == E and probe(bits=None) == E and probe(off=2) == E
    assert probe(lad=high) == E and probe(w_=16384, h_2=16384) == E and "blocks" in L.amvhip_last_error(h_).decode()
    assert probe(n_=0, bits=None) == 0

    def rate(r, rung=words, off=0, w_=w, h_2=h, n_=n):
        return L.amvhip_requant_rate_stream_dev(h_, p(d_blob), blob_bytes, p(d_offs), p(d_lens), n_, w_, h_2, ctypes.addressof(r) if r else None,
                                                p(out), cap, p(out_offs), p(out_lens), p(status), p(rung, off), None)

    good = pkg.Rate([0, 3481], budget=100)
    assert rate(None) == E and rate(pkg.Rate(None, budget=1, rungs=2)) == E and rate(pkg.Rate([1], budget=1, rungs=0)) == E
    assert rate(pkg.Rate([1] * 16, budget=1, rungs=17)) == E and rate(pkg.Rate([0, Q.LAMBDA_MAX + 1], budget=1)) == E
    assert rate(good, rung=None) == E and rate(good, off=2) == E and rate(pkg.Rate([0], budget=1, d_budget=words.data_ptr() + 2)) == E
    assert rate(good, w_=16384, h_2=16384) == E
    assert rate(good, n_=0) == 0
    torch.cuda.synchronize()
    # nothing was queued: no output was touched
    assert (out.cpu().numpy() == FILL).all() and (words.cpu().numpy().view(np.uint32) == UNWRITTEN).all()
    assert (status.cpu().numpy().view(np.uint32) == UNWRITTEN).all() and (out_lens.cpu().numpy() == -1).all()
    assert rate(good) == 0
    torch.cuda.synchronize()
    assert (status.cpu().numpy() == 0).all()


def test_the_other_entries_after_a_requant_call(ctx, pkg, orc, amv1):
    """the coefficient workspace, the record set and the rate workspace are shared: the trellis encoder and the decoder give
    the bytes they gave before a requant call on the same context"""
    import torch
    from test_gpu_encode_nr_trellis import _encode
    w, h = 48, 32
    frames = N.stream(w, h, ["texture", "ramp", "noise"], 77)
    chunks = Q.synth_chunks(w, h, 3)

    def decode():
        d_blob, blob_bytes, d_offs, d_lens, n = _inputs(chunks)
        out = torch.zeros((n, h, orc.stride(w)), dtype=torch.uint8, device="cuda:0")
        st = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
        ctx.decode_batch_dev(d_blob, blob_bytes, d_offs, d_lens, n, w, h, 0, out, st)
        torch.cuda.synchronize()
        return out.cpu().numpy(), st.cpu().numpy()

    def encode():
        blob, offs, lens = _encode(ctx, frames, w, h, 0, 3481, None, entry="trellis")
        return blob.tobytes(), offs.tolist(), lens.tolist()

    before = (decode(), encode())
    big = chunks_of("176x144", amv1)
    _rate(ctx, pkg, big[2], big[0], big[1], Q.LADDER, 500)
    _stream(ctx, big[2], big[0], big[1], 3481)
    after = (decode(), encode())
    assert (before[0][0] == after[0][0]).all() and (before[0][1] == after[0][1]).all() and before[1] == after[1]
    blob, offs, lens = Q.pack(chunks)
    want, st = orc.decode_batch(blob, offs, lens, w, h)
    assert (after[0][0] == want).all() and (after[0][1] == st).all()
    model = T.encode_frames(frames, w, h, 0, 3481)
    assert [after[1][0][o: o + ln] for o, ln in zip(after[1][1], after[1][2])] == [bytes(c) for c in model]
