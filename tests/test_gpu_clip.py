"""A byte budget per clip (amvhip_encode_*_clip_stream_dev, amvhip_requant_clip_stream_dev) on a real MI355X against
tests/clip_ref.py and against the existing rate entry on the ladder's tail from the clip rung on: every chunk's bytes, d_offs,
d_lens, d_rung, d_clip, no byte behind the last chunk, the -nr state.  Every comparison is of bytes or integers.

Shapes are rate_ref's: 16x16 (one MCU) x 8, 50x38 (padding blocks both ways, escapes at every rung) x 4, 176x96 (segments of 6 +
5) x 1; 16x16 x 1030 is two rounds of the coefficient workspace.  The model's tables are made once per input and shared."""
import numpy as np
import pytest

import clip_ref as C
import img_convert_ref as IR
import nr_ref as N
import pixel_builder as pb
import rate_ref as R
import requant_ref as Q
import test_gpu_requant as TQ
from test_gpu_encode_nr_trellis import FILL, _chunks, _outputs, _state_dev, both_modes  # noqa: F401  (both_modes is a fixture)
from test_gpu_encode_rate import NOT_READ, UNWRITTEN, _check, _planes, _rate, tables_of
from test_gpu_frontend import Pictures, stream
from test_gpu_parity import _t
from test_rate_ref import MULTI_LADDER

pytestmark = pytest.mark.gpu

CLIP_UNWRITTEN = 0x5A5A5A5A5A5A5A5A


def _rate_of(pkg, ladder, budgets, keep):
    if np.isscalar(budgets):
        return pkg.Rate(ladder, budget=int(budgets))
    keep.append(_t(np.asarray(budgets, np.uint32)))
    return pkg.Rate(ladder, budget=1, d_budget=keep[-1])               # (the uniform budget is not read then)


def _clip(ctx, pkg, frames, w, h, ladder, budgets, total, qbias=0, nr=0, d_state=None, cap=None):
    """one call of the YUV420 clip entry -> (blob, offs, lens, rungs, clip [2])"""
    import torch
    n = len(frames)
    cap, d_blob, d_offs, d_lens = _outputs(ctx, n, w, h, cap)
    d_rung = torch.full((n,), UNWRITTEN, dtype=torch.int32, device="cuda:0")
    d_clip = _t(np.full(2, CLIP_UNWRITTEN, np.uint64))
    keep = []
    ctx.encode_yuv420_clip_stream_dev(*_planes(frames, w, h), pkg.Quant(qbias, nr, 1, NOT_READ, d_state), _rate_of(pkg, ladder, budgets, keep),
                                      total, d_blob, cap, d_offs, d_lens, d_rung, d_clip)
    torch.cuda.synchronize()
    return (d_blob.cpu().numpy(), d_offs.cpu().numpy(), d_lens.cpu().numpy(), d_rung.cpu().numpy().view(np.uint32).astype(np.int64),
            [int(x) for x in d_clip.cpu().numpy().view(np.uint64)])


def _check_clip(got, want, what):
    """want: clip_ref.encode's (chunks, rungs, clip, state)"""
    assert got[4] == list(want[2]), "%s: d_clip %s, want %s" % (what, [hex(x) for x in got[4]], [hex(x) for x in want[2]])
    _check(got[:4], want[0], want[1], what)


def _check_tail(ctx, pkg, got, frames, w, h, ladder, budgets, what, **kw):
    """the rate entry on the ladder's tail from the clip rung on writes the same bytes, places and lengths, and its rungs + c*"""
    c = got[4][0] & ~R.OVER
    blob, offs, lens, rungs = _rate(ctx, pkg, frames, w, h, ladder[c:], budgets, **kw)
    assert (blob == got[0]).all() and (offs == got[1]).all() and (lens == got[2]).all(), what
    assert [((int(r) & ~R.OVER) + c) | (int(r) & R.OVER) for r in rungs] == list(got[3]), what


def totals_of(name):
    """-> {what: total} for a shape without a cap per frame"""
    bits, lens, esc = tables_of(name)
    S, F = C.sums(lens, C.NO_CAP), C.floor_sums(bits, C.NO_CAP)
    middle = next(c for c in (2, 1, 3) if esc[:, c].any())
    floor_of = next(c for c in range(len(S) - 1) if S[c] > F[c])
    out = {"S(%d)" % middle: S[middle], "S(%d) - 1" % middle: S[middle] - 1, "F(%d)" % floor_of: F[floor_of], "nothing": 0,
           "everything": C.U64_MAX}
    if name == "16x16":
        out.update({"716": 716, "713": 713, "108": 108, "107": 107})
    return out


# ---- the totals ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["16x16", "50x38"])
def test_totals(ctx, pkg, both_modes, name):
    w, h, frames = R.shape(name)
    bits, lens, esc = tables_of(name)
    totals = totals_of(name)
    want = {what: C.encode(frames, w, h, 0, 0, None, R.LADDER, C.NO_CAP, total) for what, total in totals.items()}
    walks = {what: C.device_walk(bits, lens, C.NO_CAP, total) for what, total in totals.items()}
    # what the totals are there for: a clip that stays, one that moves after coding, one that passes a rung on its floor, the
    # last rung with and without the flag
    assert want["everything"][2][0] == 0 and want["nothing"][2][0] == 4 | R.OVER
    assert any(len(walk[6]) > 1 and walk[6][0] == 0 for walk in walks.values()) and any(walk[6][0] > 0 for walk in walks.values())
    if name == "16x16":
        assert [want[k][2] for k in ("716", "713", "108", "107")] == [(1, 714), (2, 663), (4, 108), (4 | R.OVER, 108)]
        assert walks["716"][6] == [0, 1] and walks["713"][6] == [1, 2]

    def run(mode):
        for what, total in totals.items():
            got = _clip(ctx, pkg, frames, w, h, R.LADDER, C.NO_CAP, total)
            _check_clip(got, want[what], "%s, total %s, %s" % (name, what, mode))
            _check_tail(ctx, pkg, got, frames, w, h, R.LADDER, C.NO_CAP, "%s, total %s, %s: the rate entry on the tail" % (name, what, mode))

    both_modes(run)


@pytest.mark.parametrize("qbias", [0, 128])
def test_qbias(ctx, pkg, qbias):
    w, h, frames = R.shape("50x38")
    lens = R.lens_table(frames, w, h, qbias, 0, None, R.LADDER)
    total = C.sums(lens, C.NO_CAP)[1] - 1
    want = C.encode(frames, w, h, qbias, 0, None, R.LADDER, C.NO_CAP, total)
    assert want[2][0] >= 2
    got = _clip(ctx, pkg, frames, w, h, R.LADDER, C.NO_CAP, total, qbias=qbias)
    _check_clip(got, want, "qbias %d" % qbias)


@pytest.mark.parametrize("bgr", [0, 1])
def test_rgb_and_bgr(ctx, pkg, orc, bgr):
    import torch
    w, h, n = 16, 16, 3
    pix = np.stack([orc.synth_frame(0xA11CE, 20 + t, w, h) for t in range(n)])
    frames = [pb.to_planes(orc, pix[t], w, h, bgr) for t in range(n)]
    stride = w * 3 + 5
    padded = np.full((n, h, stride), 0xEE, np.uint8)
    padded[:, :, : w * 3] = pix.reshape(n, h, w * 3)
    lens = R.lens_table(frames, w, h, 0, 0, None, R.LADDER)
    total = C.sums(lens, C.NO_CAP)[2]
    want = C.encode(frames, w, h, 0, 0, None, R.LADDER, C.NO_CAP, total)
    cap, d_blob, d_offs, d_lens = _outputs(ctx, n, w, h, None)
    d_rung = torch.full((n,), UNWRITTEN, dtype=torch.int32, device="cuda:0")
    d_clip = _t(np.full(2, CLIP_UNWRITTEN, np.uint64))
    ctx.encode_clip_stream_dev(_t(padded), stride, bgr, n, w, h, pkg.Quant(0, 0, 1, NOT_READ), pkg.Rate(R.LADDER, budget=C.NO_CAP), total, d_blob,
                               cap, d_offs, d_lens, d_rung, d_clip)
    torch.cuda.synchronize()
    got = (d_blob.cpu().numpy(), d_offs.cpu().numpy(), d_lens.cpu().numpy(), d_rung.cpu().numpy().view(np.uint32).astype(np.int64),
           [int(x) for x in d_clip.cpu().numpy().view(np.uint64)])
    _check_clip(got, want, "bgr %d" % bgr)


# ---- a cap per frame under the total ---------------------------------------------------------------------------------------------

def test_uniform_cap(ctx, pkg, both_modes):
    """a cap of 150 at 16x16: frames 2 and 6 fit on the last rung alone, while the clip settles at rung 2"""
    w, h, frames = R.shape("16x16")
    lens = R.lens_table(frames, w, h, 0, 0, None, R.LADDER)
    total = C.sums(lens, 150)[2]
    want = C.encode(frames, w, h, 0, 0, None, R.LADDER, 150, total)
    assert want[2] == (2, total) and [i for i in range(8) if want[1][i] == 4] == [2, 6] and set(want[1]) == {2, 4}

    def run(mode):
        got = _clip(ctx, pkg, frames, w, h, R.LADDER, 150, total)
        _check_clip(got, want, "cap 150, %s" % mode)
        _check_tail(ctx, pkg, got, frames, w, h, R.LADDER, 150, "cap 150, %s: the rate entry on the tail" % mode)

    both_modes(run)


@pytest.mark.parametrize("name", ["16x16", "50x38"])
def test_budget_array(ctx, pkg, name):
    """a budget per frame through d_budget: a rung's floor where the frame has an escape (it floor-fits and does not fit: a
    frame moves on inside a clip rung), a middle rung's length elsewhere -- at every S(c), that less one, and every F(c)"""
    w, h, frames = R.shape(name)
    bits, lens, esc = tables_of(name)
    n = len(frames)
    with_escape = [next((r for r in range(5) if esc[i][r]), None) for i in range(n)]
    B = [int(lens[i][2]) - (i & 1) if with_escape[i] is None else R.floor_bytes(int(bits[i][with_escape[i]])) for i in range(n)]
    assert any(R.first_fit(bits[i], B[i], 0) != R.choose(lens[i], B[i])[0] for i in range(n))
    S, F = C.sums(lens, B), C.floor_sums(bits, B)
    for total in sorted({x - d for x in S for d in (0, 1)} | set(F)):
        want = C.encode(frames, w, h, 0, 0, None, R.LADDER, B, total)
        got = _clip(ctx, pkg, frames, w, h, R.LADDER, B, total)
        _check_clip(got, want, "%s, a budget per frame, total %d" % (name, total))
    _check_tail(ctx, pkg, got, frames, w, h, R.LADDER, B, "%s, a budget per frame: the rate entry on the tail" % name)


# ---- ladders ------------------------------------------------------------------------------------------------------------------------

def test_descending_ladder(ctx, pkg, both_modes):
    w, h, frames = R.shape("16x16")
    ladder = [R.LADDER[-1], 0]
    want = C.encode(frames, w, h, 0, 0, None, ladder, C.NO_CAP, 200)
    assert want[2][0] == 0 and want[2][1] <= 200
    over = C.encode(frames, w, h, 0, 0, None, ladder, C.NO_CAP, want[2][1] - 1)
    assert over[2][0] == 1 | R.OVER                                        # one byte less: lambda 0's chunks, flagged

    def run(mode):
        _check_clip(_clip(ctx, pkg, frames, w, h, ladder, C.NO_CAP, 200), want, "descending, %s" % mode)
        _check_clip(_clip(ctx, pkg, frames, w, h, ladder, C.NO_CAP, want[2][1] - 1), over, "descending, a byte short, %s" % mode)

    both_modes(run)


def test_three_equal_rungs(ctx, pkg, both_modes):
    """ladder [400, 400, 400, 3481, max], every frame's budget its floor at 400: frame 6 walks the equal rungs inside the clip
    rung; a total one byte below S(0) = S(1) = S(2) walks the clip over them as well"""
    w, h, frames = R.shape("16x16")
    bits = R.bits_table(frames, w, h, 0, 0, None, MULTI_LADDER)
    lens = R.lens_table(frames, w, h, 0, 0, None, MULTI_LADDER)
    B = [R.floor_bytes(int(bits[i][0])) for i in range(len(frames))]
    S = C.sums(lens, B)
    assert S[0] == S[1] == S[2] > S[3]
    stays = C.encode(frames, w, h, 0, 0, None, MULTI_LADDER, B, S[0])
    moves = C.encode(frames, w, h, 0, 0, None, MULTI_LADDER, B, S[0] - 1)
    assert stays[2][0] == 0 and stays[1][6] == 3 and moves[2][0] == 3 and C.device_walk(bits, lens, B, S[0] - 1)[6] == [0, 1, 2, 3]

    def run(mode):
        _check_clip(_clip(ctx, pkg, frames, w, h, MULTI_LADDER, B, S[0]), stays, "three equal rungs, %s" % mode)
        got = _clip(ctx, pkg, frames, w, h, MULTI_LADDER, B, S[0] - 1)
        _check_clip(got, moves, "three equal rungs, a byte short, %s" % mode)
        _check_tail(ctx, pkg, got, frames, w, h, MULTI_LADDER, B, "three equal rungs, %s: the rate entry on the tail" % mode)

    both_modes(run)


@pytest.mark.parametrize("rungs", [1, 16])
def test_rung_counts(ctx, pkg, rungs):
    w, h, frames = R.shape("16x16")
    ladder = [3481] if rungs == 1 else [R.LADDER[r % 5] for r in range(16)]
    lens = R.lens_table(frames, w, h, 0, 0, None, ladder)
    S = C.sums(lens, C.NO_CAP)
    for total in (S[-1], S[-1] - 1, S[0], min(S), min(S) - 1):
        want = C.encode(frames, w, h, 0, 0, None, ladder, C.NO_CAP, total)
        _check_clip(_clip(ctx, pkg, frames, w, h, ladder, C.NO_CAP, total), want, "%d rungs, total %d" % (rungs, total))
    assert want[2][0] == (rungs - 1) | R.OVER


def test_a_pass_at_every_step_of_the_bound(ctx, pkg):
    """sixteen rungs of which the last alone is small enough, caps under which every floor sum fits: the clip is coded at every
    rung in turn, with frame 6 moving inside some of them -- more passes than a rate call ever queues"""
    w, h, frames = R.shape("16x16")
    ladder = [R.LADDER[r % 4] for r in range(15)] + [R.LADDER[-1]]
    bits = R.bits_table(frames, w, h, 0, 0, None, ladder)
    lens = R.lens_table(frames, w, h, 0, 0, None, ladder)
    B = [R.floor_bytes(int(bits[i][1])) for i in range(len(frames))]      # frame 6 floor-fits at 400 and does not fit
    S = C.sums(lens, B)
    total = S[-1]
    walk = C.device_walk(bits, lens, B, total)
    assert walk[0] == 15 and not walk[1] and walk[6] == list(range(16)) and 16 < walk[4] <= C.passes_most(16)
    want = C.encode(frames, w, h, 0, 0, None, ladder, B, total)
    _check_clip(_clip(ctx, pkg, frames, w, h, ladder, B, total), want, "sixteen rungs, %d passes" % walk[4])


# ---- sizes ----------------------------------------------------------------------------------------------------------------------

def test_176x96(ctx, pkg, both_modes):
    w, h, frames = R.shape("176x96")
    bits, lens, esc = tables_of("176x96")
    S, F = C.sums(lens, C.NO_CAP), C.floor_sums(bits, C.NO_CAP)
    assert esc.any()
    totals = sorted({S[1], S[2] - 1, F[0], S[4] - 1})
    want = {total: C.encode(frames, w, h, 0, 0, None, R.LADDER, C.NO_CAP, total) for total in totals}

    def run(mode):
        for total in totals:
            _check_clip(_clip(ctx, pkg, frames, w, h, R.LADDER, C.NO_CAP, total), want[total], "176x96, total %d, %s" % (total, mode))

    both_modes(run)


def test_two_workspace_rounds_and_one_bump(ctx, pkg):
    """16x16 x 1030, the eight pictures cycling, a total one byte below S(0): every frame is coded at rung 0, the sum is over,
    the clip moves to rung 1 and takes along every frame whose chunk differs there -- frames 1024 .. 1029, the second round of
    the coefficient workspace, among them"""
    w, h, frames = R.shape("16x16")
    bits, lens, esc = tables_of("16x16")
    chunks = R.chunks_table(frames, w, h, 0, 0, None, R.LADDER)
    n = 1030
    many = [frames[i % 8] for i in range(n)]
    lens_many, bits_many = lens[[i % 8 for i in range(n)]], bits[[i % 8 for i in range(n)]]
    S, F = C.sums(lens_many, C.NO_CAP), C.floor_sums(bits_many, C.NO_CAP)
    total = S[0] - 1
    assert F[0] <= total and S[1] <= total
    walk = C.device_walk(bits_many, lens_many, C.NO_CAP, total)
    assert walk[:3] == (1, False, S[1]) and walk[6] == [0, 1] and walk[4] == 2 and all(k == 2 for k in walk[5][1024:])
    got = _clip(ctx, pkg, many, w, h, R.LADDER, C.NO_CAP, total)
    assert got[4] == [1, S[1]]
    _check(got[:4], [chunks[i % 8][1] for i in range(n)], [1] * n, "1030 frames")


# ---- -nr ------------------------------------------------------------------------------------------------------------------------

def test_nr_state_is_the_rate_entrys(ctx, pkg):
    w, h, frames = R.shape("50x38")
    nr = 1500
    start = np.arange(65) * 700 + 3
    start[64] = 2500
    lens = R.lens_table(frames, w, h, 0, nr, start, R.LADDER)
    total = min(C.sums(lens, C.NO_CAP)[:2]) - 1                           # (behind -nr rung 1 is the longer one)
    want = C.encode(frames, w, h, 0, nr, start, R.LADDER, C.NO_CAP, total)
    assert want[2][0] >= 2
    d_state = _state_dev(start)
    got = _clip(ctx, pkg, frames, w, h, R.LADDER, C.NO_CAP, total, nr=nr, d_state=d_state)
    _check_clip(got, want, "nr")
    assert (d_state.cpu().numpy() == want[3]).all()
    rate_state = _state_dev(start)
    _check_tail(ctx, pkg, got, frames, w, h, R.LADDER, C.NO_CAP, "nr: the rate entry on the tail", nr=nr, d_state=rate_state)
    assert (rate_state.cpu().numpy() == d_state.cpu().numpy()).all()
    # two calls with the state carried advance it as one call does
    d_state = _state_dev(start)
    for lo, hi in ((0, 1), (1, 4)):
        _clip(ctx, pkg, frames[lo:hi], w, h, R.LADDER, C.NO_CAP, C.U64_MAX, nr=nr, d_state=d_state)
    assert (d_state.cpu().numpy() == want[3]).all()


# ---- the front-end entry ------------------------------------------------------------------------------------------------------------

def test_front_end_entry(ctx, pkg, both_modes):
    """a 32x24 source, deinterlace + rescale to 16x16: the entry equals amvhip_video_frontend_dev into tight planes followed by
    the YUV420 clip entry, at a total that moves the clip"""
    import torch
    W, H, n, sw, sh = 16, 16, 4, 32, 24
    fe = pkg.Frontend(1)
    frames = [IR.make_picture(IR.YUV420P, sw, sh, k, 11 + 5 * i) for i, k in enumerate(("ramp", "noise", "ramp", "noise"))]
    s = Pictures(IR.YUV420P, sw, sh, n).fill(frames).to_dev()
    d = Pictures(IR.YUVJ420P, W, H, n).to_dev()
    ctx.video_frontend_dev(IR.YUV420P, s.pic(), sw, sh, n, fe, d.pic(), W, H, stream())
    torch.cuda.synchronize()

    def call(front, total):
        cap, d_blob, d_offs, d_lens = _outputs(ctx, n, W, H, None)
        d_rung = torch.full((n,), UNWRITTEN, dtype=torch.int32, device="cuda:0")
        d_clip = _t(np.full(2, CLIP_UNWRITTEN, np.uint64))
        q, rate = pkg.Quant(5, 0, 1, NOT_READ), pkg.Rate(R.LADDER, budget=C.NO_CAP)
        if front:
            ctx.encode_frontend_clip_stream_dev(IR.YUV420P, s.pic(), sw, sh, n, fe, W, H, q, rate, total, d_blob, cap, d_offs, d_lens, d_rung,
                                                d_clip, stream())
        else:
            ctx.encode_yuv420_clip_stream_dev(*d.dev, d.stride[0], d.stride[1], d.frame[0], d.frame[1], n, W, H, q, rate, total, d_blob, cap,
                                              d_offs, d_lens, d_rung, d_clip, stream())
        torch.cuda.synchronize()
        return [x.cpu().numpy() for x in (d_blob, d_offs, d_lens, d_rung, d_clip)]

    def run(mode):
        everything = call(False, C.U64_MAX)
        at_zero = int(everything[4].view(np.uint64)[1])
        assert int(everything[4].view(np.uint64)[0]) == 0 and at_zero == int(everything[2].sum())
        outs = [call(front, at_zero - 1) for front in (False, True)]
        assert all((a == b).all() for a, b in zip(*outs)), mode
        clip = outs[1][4].view(np.uint64)
        assert 1 <= int(clip[0]) <= 4 and int(clip[1]) == int(outs[1][2].sum()) <= at_zero - 1, mode
        assert (outs[1][3] == int(clip[0])).all(), mode

    both_modes(run)


# ---- the requant entry ------------------------------------------------------------------------------------------------------------

def _requant_clip(ctx, pkg, chunks, w, h, ladder, budgets, total, cap=None):
    """-> (blob, offs, lens, status, rungs, clip [2])"""
    import torch
    d_blob, blob_bytes, d_offs, d_lens, n = TQ._inputs(chunks)
    cap = sum(len(c) for c in chunks) + 64 if cap is None else cap
    out, out_offs, out_lens, status = TQ._outs(n, cap)
    rung = torch.full((n,), UNWRITTEN, dtype=torch.int32, device="cuda:0")
    d_clip = _t(np.full(2, CLIP_UNWRITTEN, np.uint64))
    keep = []
    ctx.requant_clip_stream_dev(d_blob, blob_bytes, d_offs, d_lens, n, w, h, _rate_of(pkg, ladder, budgets, keep), total, out, cap, out_offs,
                                out_lens, status, rung, d_clip)
    torch.cuda.synchronize()
    return (out.cpu().numpy(), out_offs.cpu().numpy(), out_lens.cpu().numpy(), status.cpu().numpy(),
            rung.cpu().numpy().view(np.uint32).astype(np.int64), [int(x) for x in d_clip.cpu().numpy().view(np.uint64)])


def test_requant_entry(ctx, pkg, both_modes):
    """synthetic 16x16 chunks with a damaged frame and one out of range among them: neither adds to a sum, both keep the last
    rung flagged and no bytes; the others are the requant rate entry's on the ladder's tail"""
    w, h = 16, 16
    chunks = Q.synth_chunks(w, h, 8)
    chunks[2] = chunks[2][: len(chunks[2]) // 2]
    chunks[5] = N._chunk(TQ._frame(Q.block_of({1: 1}, dc=1024), at=4))
    lens, coded = C.requant_lens(chunks, w, h, Q.LADDER)
    bits = Q.bits_table(chunks, w, h, Q.LADDER)
    assert [i for i in range(8) if not coded[i]] == [2, 5]
    S, F = C.sums(lens, C.NO_CAP, coded), C.floor_sums(bits, C.NO_CAP, coded)
    cap_per_frame = int(np.median(lens[:, 1]))
    cases = [(C.NO_CAP, total) for total in sorted({S[0], S[0] - 1, S[2], S[2] - 1, F[1], S[4], S[4] - 1, 0, C.U64_MAX})]
    cases += [(cap_per_frame, total) for total in sorted({x - d for x in C.sums(lens, cap_per_frame, coded)[:3] for d in (0, 1)})]
    want = [C.requant(chunks, w, h, Q.LADDER, B, total) for B, total in cases]
    assert len({x[3][0] for x in want}) >= 4 and any(x[3][0] & R.OVER for x in want)

    def run(mode):
        for (B, total), (out, status, rungs, clip) in zip(cases, want):
            what = "requant, cap %d, total %d, %s" % (B, total, mode)
            got = _requant_clip(ctx, pkg, chunks, w, h, Q.LADDER, B, total)
            assert got[5] == list(clip), "%s: d_clip %s, want %s" % (what, got[5], clip)
            TQ._check(got, out, status, what)
            assert list(got[4]) == rungs, what
            assert all(got[4][i] == (4 | R.OVER) and got[3][i] and got[2][i] == 0 for i in (2, 5)), what
            c = clip[0] & ~R.OVER
            tail = TQ._rate(ctx, pkg, chunks, w, h, Q.LADDER[c:], B)
            assert all((a == b).all() for a, b in zip(tail[:4], got[:4])), what
            assert [((int(r) & ~R.OVER) + c) | (int(r) & R.OVER) for r in tail[4]] == list(got[4]), what

    both_modes(run)


def test_requant_two_workspace_rounds_and_one_bump(ctx, pkg, both_modes):
    """16x16 x 1030, the eight synthetic chunks cycling, a total one byte below S(0): every frame is coded at rung 0, the sum is
    over, the clip moves to rung 1 and takes along every frame below it -- frames 1024 .. 1029 among them, which a redo pass
    finds in the second round of the coefficient workspace (the serial kernel's round with base 1024).  Rung 1 makes one of the
    eight chunks a byte longer, so S(1) > S(0) and the walk goes on to rung 2 the same way: the model says where it ends."""
    w, h, n = 16, 16, 1030
    eight = Q.synth_chunks(w, h, 8)
    lens8, coded8 = C.requant_lens(eight, w, h, Q.LADDER)
    bits8 = Q.bits_table(eight, w, h, Q.LADDER)
    assert all(coded8)
    cycle = [i % 8 for i in range(n)]
    chunks, lens, bits = [eight[i] for i in cycle], lens8[cycle], bits8[cycle]
    S, F = C.sums(lens, C.NO_CAP), C.floor_sums(bits, C.NO_CAP)
    total = S[0] - 1
    walk = C.device_walk(bits, lens, C.NO_CAP, total)
    c = walk[0]
    assert F[0] <= total and walk[6][:2] == [0, 1] and walk[6][-1] == c                       # the clip moves to rung 1
    assert walk[4] == len(walk[6]) and all(k == walk[4] for k in walk[5][1024:])              # and takes frames 1024 .. 1029 along
    assert walk[1:4] == (False, S[c], [c] * n)
    at_c = Q.requant(eight, w, h, Q.LADDER[c])[0]

    def run(mode):
        got = _requant_clip(ctx, pkg, chunks, w, h, Q.LADDER, C.NO_CAP, total)
        assert got[5] == [c, S[c]], "%s: d_clip %s" % (mode, got[5])
        TQ._check(got, [at_c[i] for i in cycle], [0] * n, "requant, 1030 chunks, %s" % mode)
        assert list(got[4]) == walk[3], mode

    both_modes(run)


# ---- a blob that is too small ---------------------------------------------------------------------------------------------------------

def test_blob_one_byte_short(ctx, pkg):
    w, h, frames = R.shape("50x38")
    lens = R.lens_table(frames, w, h, 0, 0, None, R.LADDER)
    total = C.sums(lens, C.NO_CAP)[2] - 1
    want = C.encode(frames, w, h, 0, 0, None, R.LADDER, C.NO_CAP, total)
    size = sum(len(c) for c in want[0])
    assert size == want[2][1]
    blob, offs, lens_got, rungs, clip = _clip(ctx, pkg, frames, w, h, R.LADDER, C.NO_CAP, total, cap=size - 1)
    assert clip == list(want[2]) and list(rungs) == want[1]                # S is taken before the capacity rule drops a chunk
    assert int(lens_got[-1]) == 0 and int(offs[-1]) == size - len(want[0][-1])
    assert _chunks(blob, offs[:-1], lens_got[:-1]) == want[0][:-1]
    assert (blob[int(offs[-1]):] == FILL).all()
    _check_clip(_clip(ctx, pkg, frames, w, h, R.LADDER, C.NO_CAP, total, cap=size), want, "a blob that just fits")


# ---- refusals ---------------------------------------------------------------------------------------------------------------------

def test_refusals(ctx, pkg):
    import torch
    w, h, frames = R.shape("16x16")
    n = 4
    frames = frames[:n]
    planes = _planes(frames, w, h)
    pix = _t(np.zeros((n, h, w, 3), np.uint8))
    state = np.arange(65) + 5
    d_state = _state_dev(state)
    cap, d_blob, d_offs, d_lens = _outputs(ctx, n, w, h, 4096)
    d_rung = torch.full((n + 1,), UNWRITTEN, dtype=torch.int32, device="cuda:0")
    d_clip = _t(np.full(3, CLIP_UNWRITTEN, np.uint64))
    d_budget = _t(np.full(n + 1, 100, np.uint32))
    lam_most, nr_most = ctx.encode_trellis_lambda_max(), ctx.encode_nr_max(w, h)
    ok_q = pkg.Quant(0, 300, 1, NOT_READ, d_state)
    ok_rate = pkg.Rate(R.LADDER, budget=100, d_budget=d_budget)
    bad_q = [None, pkg.Quant(0, 300, 0, 0, d_state), pkg.Quant(0, 300, 2, 0, d_state), pkg.Quant(256, 300, 1, 0, d_state),
             pkg.Quant(0, nr_most + 1, 1, 0, d_state), pkg.Quant(0, 300, 1, 0, None), pkg.Quant(0, 300, 1, 0, d_state.data_ptr() + 2)]
    bad_ladders = [(None, None), ([], None), (R.LADDER, 0), ([1] * 17, None), (R.LADDER * 4, 17), ([0, lam_most + 1], None),
                   ([0xFFFFFFFF], None)]
    out = (d_blob, cap, d_offs, d_lens)
    front = (IR.YUVJ420P, (planes[:3],) + planes[3:7], w, h, n, None, w, h)
    total = 1000

    def refused(call):
        with pytest.raises(pkg.AmvHipError, match=r"\(-1\)"):
            call()

    def every_encoder(q, rate, outs, rung, clip):
        refused(lambda: ctx.encode_yuv420_clip_stream_dev(*planes, q, rate, total, *outs, rung, clip))
        refused(lambda: ctx.encode_clip_stream_dev(pix, w * 3, 0, n, w, h, q, rate, total, *outs, rung, clip))
        refused(lambda: ctx.encode_frontend_clip_stream_dev(*front, q, rate, total, *outs, rung, clip))

    for q in bad_q:
        every_encoder(q, ok_rate, out, d_rung, d_clip)
    for ladder, rungs in bad_ladders:
        every_encoder(ok_q, pkg.Rate(ladder, budget=100, rungs=rungs), out, d_rung, d_clip)
    for rate, rung, clip in ((None, d_rung, d_clip), (ok_rate, None, d_clip), (ok_rate, d_rung.data_ptr() + 2, d_clip),
                             (pkg.Rate(R.LADDER, budget=100, d_budget=d_budget.data_ptr() + 2), d_rung, d_clip),
                             (ok_rate, d_rung, None), (ok_rate, d_rung, d_clip.data_ptr() + 4)):
        every_encoder(ok_q, rate, out, rung, clip)
    for outs in ((None, cap, d_offs, d_lens), (d_blob, cap, None, d_lens), (d_blob, cap, d_offs, None)):
        every_encoder(ok_q, ok_rate, outs, d_rung, d_clip)
    refused(lambda: ctx.encode_yuv420_clip_stream_dev(*planes[:8], w - 1, h, ok_q, ok_rate, total, *out, d_rung, d_clip))
    # the requant entry: what its rate sibling refuses, and d_clip
    chunks = Q.synth_chunks(w, h, n)
    ins = TQ._inputs(chunks)
    r_out, r_offs, r_lens, r_status = TQ._outs(n, 4096)
    plain = pkg.Rate(Q.LADDER, budget=100)

    def requant(rate=plain, ins=ins, size=(w, h), outs=(r_out, 4096, r_offs, r_lens), status=r_status, rung=d_rung, clip=d_clip):
        refused(lambda: ctx.requant_clip_stream_dev(*ins, *size, rate, total, *outs, status, rung, clip))

    requant(clip=None)
    requant(clip=d_clip.data_ptr() + 4)
    requant(rate=None)
    for ladder, rungs in bad_ladders:
        requant(rate=pkg.Rate(ladder, budget=100, rungs=rungs))
    requant(rate=pkg.Rate(Q.LADDER, budget=100, d_budget=d_budget.data_ptr() + 2))
    requant(rung=None)
    requant(rung=d_rung.data_ptr() + 2)
    requant(status=None)
    requant(ins=(None,) + ins[1:])
    requant(ins=ins[:2] + (None,) + ins[3:])
    requant(ins=ins[:3] + (None,) + ins[4:])
    requant(outs=(None, 4096, r_offs, r_lens))
    requant(outs=(r_out, 4096, None, r_lens))
    requant(outs=(r_out, 4096, r_offs, None))
    requant(size=(0, h))
    torch.cuda.synchronize()
    assert (d_state.cpu().numpy() == state).all() and (d_blob.cpu().numpy() == FILL).all() and (r_out.cpu().numpy() == FILL).all()
    assert (d_offs.cpu().numpy() == -1).all() and (d_lens.cpu().numpy() == -1).all()
    assert (d_rung.cpu().numpy() == UNWRITTEN).all() and (d_clip.cpu().numpy().view(np.uint64) == CLIP_UNWRITTEN).all()
    assert (r_status.cpu().numpy() == UNWRITTEN).all() and (r_lens.cpu().numpy() == -1).all()
    # ... and the bounds themselves are taken: sixteen rungs, the largest lambda and nr, a budget array; n == 0 is nothing
    ladder = [lam_most] + R.LADDER * 3
    B = [100, 60, 7, 300]
    lens = R.lens_table(frames, w, h, 0, nr_most, state, ladder)
    want = C.encode(frames, w, h, 0, nr_most, state, ladder, B, C.sums(lens, B)[1] - 1)
    got = _clip(ctx, pkg, frames, w, h, ladder, B, C.sums(lens, B)[1] - 1, nr=nr_most, d_state=d_state)
    _check_clip(got, want, "the bounds")
    assert (d_state.cpu().numpy() == want[3]).all()
    ctx.encode_yuv420_clip_stream_dev(*planes[:7], 0, w, h, ok_q, ok_rate, total, None, 0, None, None, None, None)
    ctx.requant_clip_stream_dev(None, 0, None, None, 0, w, h, plain, total, None, 0, None, None, None, None, None)


# ---- every written chunk decodes ----------------------------------------------------------------------------------------------------

def test_every_written_chunk_decodes(ctx, pkg):
    import torch
    w, h, frames = R.shape("50x38")
    n = len(frames)
    for what, total in totals_of("50x38").items():
        blob, offs, lens_got, rungs, clip = _clip(ctx, pkg, frames, w, h, R.LADDER, C.NO_CAP, total)
        size = int(offs[-1] + lens_got[-1])
        assert size == clip[1]
        d_out = torch.zeros((n, h, ctx.stride(w)), dtype=torch.uint8, device="cuda:0")
        d_st = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
        ctx.decode_batch_dev(_t(blob), size, _t(offs.astype(np.uint64)), _t(lens_got.astype(np.uint32)), n, w, h, 0, d_out, d_st)
        torch.cuda.synchronize()
        assert (d_st.cpu().numpy() == 0).all(), (what, d_st.cpu().numpy())
