"""A byte budget per frame, met by a device search over the trellis lambda (amvhip_encode_*_rate_probe_dev,
amvhip_encode_*_rate_stream_dev) on a real MI355X against tests/rate_ref.py: d_bits against the bits the model reads off its
levels, and for the rate entries every chunk's bytes, d_offs, d_lens, d_rung, no byte behind the last chunk, and the -nr
state.  Every comparison is of bytes or integers.

Shapes are the smallest that reach each path: 16x16 (one MCU) x 8, 50x38 (padding blocks both ways) x 4, 176x96 (eleven MCUs
a row: segments of 6 + 5, twelve segments) x 1; 16x16 x 1030 is two rounds of the coefficient workspace.  The model's tables
are made once per input and shared (rate_ref caches the levels)."""
import numpy as np
import pytest

import img_convert_ref as IR
import pixel_builder as pb
import rate_ref as R
from test_gpu_encode_nr_trellis import FILL, _chunks, _outputs, _pack, _state_dev, both_modes  # noqa: F401  (both_modes is a fixture)
from test_gpu_frontend import Pictures, stream
from test_gpu_parity import _t
from test_rate_ref import MULTI_LADDER, budgets_of

pytestmark = pytest.mark.gpu

UNWRITTEN = 0x5A5A5A5A
NOT_READ = 0xFFFFFFFF              # the Quant's lambda: a rate call does not read it (the trellis entries would refuse it)


def tables_of(name, qbias=0, ladder=None):
    ladder = R.LADDER if ladder is None else ladder
    w, h, frames = R.shape(name)
    chunks = R.chunks_table(frames, w, h, qbias, 0, None, ladder)
    return (R.bits_table(frames, w, h, qbias, 0, None, ladder), np.array([[len(c) for c in row] for row in chunks]),
            np.array([[R.escapes(c) for c in row] for row in chunks]))


def _planes(frames, w, h):
    Y, Cb, Cr, ys, cs = _pack(frames, w, h)
    return (_t(Y), _t(Cb), _t(Cr), ys, cs, h * ys, (h // 2) * cs, len(frames), w, h)


def _probe(ctx, pkg, frames, w, h, ladder, qbias=0, nr=0, d_state=None):
    import torch
    d_bits = torch.full((len(frames), len(ladder)), UNWRITTEN, dtype=torch.int32, device="cuda:0")
    ctx.encode_yuv420_rate_probe_dev(*_planes(frames, w, h), pkg.Quant(qbias, nr, 1, NOT_READ, d_state), ladder, d_bits)
    torch.cuda.synchronize()
    return d_bits.cpu().numpy().view(np.uint32).astype(np.int64)


def _rate(ctx, pkg, frames, w, h, ladder, budgets, qbias=0, nr=0, d_state=None, cap=None):
    """one call of the YUV420 rate entry; budgets: a list (handed over as d_budget) or one number (the uniform budget)
    -> (blob, offs, lens, rungs)"""
    import torch
    n = len(frames)
    cap, d_blob, d_offs, d_lens = _outputs(ctx, n, w, h, cap)
    d_rung = torch.full((n,), UNWRITTEN, dtype=torch.int32, device="cuda:0")
    if np.isscalar(budgets):
        rate = pkg.Rate(ladder, budget=int(budgets))
    else:
        d_budget = _t(np.asarray(budgets, np.uint32))
        rate = pkg.Rate(ladder, budget=1, d_budget=d_budget)           # (the uniform budget is not read then)
    ctx.encode_yuv420_rate_stream_dev(*_planes(frames, w, h), pkg.Quant(qbias, nr, 1, NOT_READ, d_state), rate, d_blob, cap, d_offs, d_lens,
                                      d_rung)
    torch.cuda.synchronize()
    return d_blob.cpu().numpy(), d_offs.cpu().numpy(), d_lens.cpu().numpy(), d_rung.cpu().numpy().view(np.uint32).astype(np.int64)


def _check(got, want, want_rungs, what):
    blob, offs, lens, rungs = got
    assert list(rungs) == list(want_rungs), "%s: rungs %s, want %s" % (what, [hex(int(x)) for x in rungs], [hex(int(x)) for x in want_rungs])
    pos = 0
    for i, c in enumerate(want):
        assert (int(offs[i]), int(lens[i])) == (pos, len(c)), "%s: frame %d at %d + %d, want %d + %d" % (what, i, offs[i], lens[i], pos, len(c))
        assert blob[pos: pos + len(c)].tobytes() == c, "%s: frame %d differs" % (what, i)
        pos += len(c)
    assert (blob[pos:] == FILL).all(), "%s: bytes behind the last chunk were written" % what


# ---- the probe ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.SHAPES))
@pytest.mark.parametrize("qbias", [0, 128])
def test_probe_bits(ctx, pkg, name, qbias):
    w, h, frames = R.shape(name)
    want = R.bits_table(frames, w, h, qbias, 0, None, R.LADDER)
    got = _probe(ctx, pkg, frames, w, h, R.LADDER, qbias)
    assert (got == want).all(), "%s qbias %d: %s" % (name, qbias, np.argwhere(got != want)[:6].tolist())


@pytest.mark.parametrize("bgr", [0, 1])
def test_probe_rgb_and_bgr(ctx, pkg, orc, bgr):
    import torch
    w, h, n = 16, 16, 3
    pix = np.stack([orc.synth_frame(0xA11CE, 20 + t, w, h) for t in range(n)])
    frames = [pb.to_planes(orc, pix[t], w, h, bgr) for t in range(n)]
    stride = w * 3 + 5
    padded = np.full((n, h, stride), 0xEE, np.uint8)
    padded[:, :, : w * 3] = pix.reshape(n, h, w * 3)
    d_bits = torch.full((n, len(R.LADDER)), UNWRITTEN, dtype=torch.int32, device="cuda:0")
    ctx.encode_rate_probe_dev(_t(padded), stride, bgr, n, w, h, pkg.Quant(0, 0, 1, NOT_READ), R.LADDER, d_bits)
    torch.cuda.synchronize()
    assert (d_bits.cpu().numpy().view(np.uint32) == R.bits_table(frames, w, h, 0, 0, None, R.LADDER)).all()


def test_probe_behind_nr_leaves_the_state(ctx, pkg):
    w, h, frames = R.shape("50x38")
    state = np.arange(65) * 900 + 13
    state[64] = 4000
    d_state = _state_dev(state)
    got = _probe(ctx, pkg, frames, w, h, R.LADDER, 0, 1500, d_state)
    assert (d_state.cpu().numpy() == state).all()
    assert (got == R.bits_table(frames, w, h, 0, 1500, state, R.LADDER)).all()
    assert (got != R.bits_table(frames, w, h, 0, 0, None, R.LADDER)).any()


@pytest.mark.parametrize("rungs", [1, 16])
def test_probe_rung_counts(ctx, pkg, rungs):
    w, h, frames = R.shape("16x16")
    ladder = [3481] if rungs == 1 else [R.LADDER[r % 5] for r in range(16)]
    want = R.bits_table(frames, w, h, 0, 0, None, ladder)
    assert (_probe(ctx, pkg, frames, w, h, ladder) == want).all()


# ---- the rate entries -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(R.SHAPES))
def test_budgets_per_frame(ctx, pkg, both_modes, name):
    """the five budget kinds per frame through d_budget: a middle rung's length, that less one, the floor of a rung with escapes
    (it floor-fits and does not fit: the redo path), 7 (nothing fits: the last rung, flagged) and 2^32 - 1 (rung 0: the blob is
    amvhip_encode_yuv420_trellis_batch_dev's at ladder[0])"""
    import torch
    w, h, frames = R.shape(name)
    bits, lens, esc = tables_of(name)
    kinds = budgets_of(bits, lens, esc)
    n = len(frames)

    def run(mode):
        for kind, B in kinds.items():
            want, want_rungs, _ = R.encode(frames, w, h, 0, 0, None, R.LADDER, B)
            got = _rate(ctx, pkg, frames, w, h, R.LADDER, B)
            _check(got, want, want_rungs, "%s, %s, %s" % (name, kind, mode))
            if kind == "nothing":
                assert all(r == (4 | R.OVER) for r in got[3])
            if kind == "anything":
                cap, d_blob, d_offs, d_lens = _outputs(ctx, n, w, h, None)
                ctx.encode_yuv420_trellis_batch_dev(*_planes(frames, w, h), 0, R.LADDER[0], d_blob, cap, d_offs, d_lens)
                torch.cuda.synchronize()
                assert (d_blob.cpu().numpy() == got[0]).all() and (d_offs.cpu().numpy() == got[1]).all() and (d_lens.cpu().numpy() == got[2]).all()
                assert all(r == 0 for r in got[3])

    both_modes(run)
    # the floor budgets took the redo path: a frame whose first floor-fit is not where it landed
    B = kinds["floor"]
    assert any(R.first_fit(bits[i], B[i], 0) != R.choose(lens[i], B[i])[0] for i in range(n))


def test_several_redo_passes_for_one_frame(ctx, pkg, both_modes):
    """ladder [400, 400, 400, 3481, max], every frame's budget the floor at lambda 400: frame 6 carries an escape there, walks
    the three equal rungs and lands on the fourth"""
    w, h, frames = R.shape("16x16")
    bits = R.bits_table(frames, w, h, 0, 0, None, MULTI_LADDER)
    lens = R.lens_table(frames, w, h, 0, 0, None, MULTI_LADDER)
    B = [R.floor_bytes(int(bits[i][0])) for i in range(len(frames))]
    want, want_rungs, _ = R.encode(frames, w, h, 0, 0, None, MULTI_LADDER, B)
    assert want_rungs[6] == 3 and R.device_walk(bits[6], lens[6], B[6])[2] == 4 and 0 in want_rungs
    both_modes(lambda mode: _check(_rate(ctx, pkg, frames, w, h, MULTI_LADDER, B), want, want_rungs, "three equal rungs, %s" % mode))


def test_descending_ladder_and_uniform_budget(ctx, pkg, both_modes):
    w, h, frames = R.shape("50x38")
    ladder = R.LADDER[::-1]
    lens = R.lens_table(frames, w, h, 0, 0, None, ladder)
    B = int(lens[0][0]) + 20                                  # the ramp frame's length at the largest lambda, and a little
    want, want_rungs, _ = R.encode(frames, w, h, 0, 0, None, ladder, B)
    assert 0 in want_rungs and (4 | R.OVER) in want_rungs      # (the texture frame is over at every rung: it gets lambda 0's chunk)
    both_modes(lambda mode: _check(_rate(ctx, pkg, frames, w, h, ladder, B), want, want_rungs, "descending, uniform %d, %s" % (B, mode)))


def test_redo_lists_across_workspace_rounds(ctx, pkg):
    """16x16 x 1030, the eight pictures and the five budget kinds cycling (periods 8 and 5): frames 1024 .. 1029, the second
    round of the coefficient workspace, hold a frame that is coded twice (1025) and one that nothing fits (1026)"""
    w, h, frames = R.shape("16x16")
    bits, lens, esc = tables_of("16x16")
    kinds = list(budgets_of(bits, lens, esc).values())
    chunks = R.chunks_table(frames, w, h, 0, 0, None, R.LADDER)
    n = 1030
    many = [frames[i % 8] for i in range(n)]
    B = [kinds[(i + 2) % 5][i % 8] for i in range(n)]
    want, want_rungs = [], []
    for i in range(n):
        r, over = R.choose(lens[i % 8], B[i])
        want.append(chunks[i % 8][r])
        want_rungs.append(r | (R.OVER if over else 0))
    tail = range(1024, n)
    assert any(R.first_fit(bits[i % 8], B[i], 0) != want_rungs[i] & 0xF for i in tail) and any(want_rungs[i] & R.OVER for i in tail)
    _check(_rate(ctx, pkg, many, w, h, R.LADDER, B), want, want_rungs, "1030 frames")


def test_nr_one_call_equals_calls_with_the_state_carried(ctx, pkg):
    w, h, frames = R.shape("50x38")
    nr = 1500
    start = np.arange(65) * 700 + 3
    start[64] = 2500
    lens = R.lens_table(frames, w, h, 0, nr, start, R.LADDER)
    bits = R.bits_table(frames, w, h, 0, nr, start, R.LADDER)
    esc = lens - np.array([[R.floor_bytes(int(b)) for b in row] for row in bits])
    B = budgets_of(bits, lens, esc)["floor"][:2] + [int(lens[2][2]), int(lens[3][0])]
    want, want_rungs, want_state = R.encode(frames, w, h, 0, nr, start, R.LADDER, B)
    whole_state = _state_dev(start)
    whole = _rate(ctx, pkg, frames, w, h, R.LADDER, B, nr=nr, d_state=whole_state)
    _check(whole, want, want_rungs, "nr, one call")
    assert (whole_state.cpu().numpy() == want_state).all()
    d_state, parts, rungs = _state_dev(start), [], []
    for lo, hi in ((0, 1), (1, 4)):
        blob, offs, lens_part, rung = _rate(ctx, pkg, frames[lo:hi], w, h, R.LADDER, B[lo:hi], nr=nr, d_state=d_state)
        parts += _chunks(blob, offs, lens_part)
        rungs += list(rung)
    assert parts == want and rungs == want_rungs
    assert (d_state.cpu().numpy() == want_state).all()


def test_front_end_entry(ctx, pkg, both_modes):
    """a 32x24 source, deinterlace + rescale to 16x16: the entry equals amvhip_video_frontend_dev into tight planes followed by
    the YUV420 rate entry"""
    import torch
    W, H, n, sw, sh = 16, 16, 4, 32, 24
    fe = pkg.Frontend(1)
    frames = [IR.make_picture(IR.YUV420P, sw, sh, k, 11 + 5 * i) for i, k in enumerate(("ramp", "noise", "ramp", "noise"))]
    s = Pictures(IR.YUV420P, sw, sh, n).fill(frames).to_dev()
    d = Pictures(IR.YUVJ420P, W, H, n).to_dev()
    ctx.video_frontend_dev(IR.YUV420P, s.pic(), sw, sh, n, fe, d.pic(), W, H, stream())
    torch.cuda.synchronize()
    ladder, budget = R.LADDER, 120

    def run(mode):
        outs = []
        for front in (False, True):
            cap, d_blob, d_offs, d_lens = _outputs(ctx, n, W, H, None)
            d_rung = torch.full((n,), UNWRITTEN, dtype=torch.int32, device="cuda:0")
            q, rate = pkg.Quant(5, 0, 1, NOT_READ), pkg.Rate(ladder, budget=budget)
            if front:
                ctx.encode_frontend_rate_stream_dev(IR.YUV420P, s.pic(), sw, sh, n, fe, W, H, q, rate, d_blob, cap, d_offs, d_lens, d_rung, stream())
            else:
                ctx.encode_yuv420_rate_stream_dev(*d.dev, d.stride[0], d.stride[1], d.frame[0], d.frame[1], n, W, H, q, rate, d_blob, cap,
                                                  d_offs, d_lens, d_rung, stream())
            torch.cuda.synchronize()
            outs.append([x.cpu().numpy() for x in (d_blob, d_offs, d_lens, d_rung)])
        assert all((a == b).all() for a, b in zip(*outs)), mode
        rungs = outs[0][3].view(np.uint32)
        assert (outs[0][2] > 0).all(), mode
        assert all(int(l) <= budget or int(r) & R.OVER for l, r in zip(outs[0][2], rungs))

    both_modes(run)


def test_blob_one_byte_short(ctx, pkg):
    w, h, frames = R.shape("50x38")
    bits, lens, esc = tables_of("50x38")
    B = budgets_of(bits, lens, esc)["floor"]
    want, want_rungs, _ = R.encode(frames, w, h, 0, 0, None, R.LADDER, B)
    total = sum(len(c) for c in want)
    blob, offs, lens_got, rungs = _rate(ctx, pkg, frames, w, h, R.LADDER, B, cap=total - 1)
    assert int(lens_got[-1]) == 0 and int(offs[-1]) == total - len(want[-1])
    assert _chunks(blob, offs[:-1], lens_got[:-1]) == want[:-1]
    assert (blob[int(offs[-1]):] == FILL).all()
    assert list(rungs) == want_rungs                          # d_rung is written for every frame all the same
    # the overflow status is the plain entries': the same frames through the trellis entry with a blob one byte short
    import torch
    lam_total = sum(int(x) for x in lens[:, 2])
    cap, d_blob, d_offs, d_lens = _outputs(ctx, len(frames), w, h, lam_total - 1)
    ctx.encode_yuv420_trellis_batch_dev(*_planes(frames, w, h), 0, R.LADDER[2], d_blob, cap, d_offs, d_lens)
    torch.cuda.synchronize()
    assert int(d_lens.cpu().numpy()[-1]) == 0 and (d_lens.cpu().numpy()[:-1] == lens[:-1, 2]).all()
    _check(_rate(ctx, pkg, frames, w, h, R.LADDER, B, cap=total), want, want_rungs, "a blob that just fits")


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
    d_bits = torch.full((n * 5 + 1,), UNWRITTEN, dtype=torch.int32, device="cuda:0")
    d_budget = _t(np.full(n + 1, 100, np.uint32))
    lam_most, nr_most = ctx.encode_trellis_lambda_max(), ctx.encode_nr_max(w, h)
    ok_q = pkg.Quant(0, 300, 1, NOT_READ, d_state)
    ok_rate = pkg.Rate(R.LADDER, budget=100, d_budget=d_budget)
    bad_q = [None, pkg.Quant(0, 300, 0, 0, d_state), pkg.Quant(0, 300, 2, 0, d_state), pkg.Quant(256, 300, 1, 0, d_state),
             pkg.Quant(0, nr_most + 1, 1, 0, d_state), pkg.Quant(0, 300, 1, 0, None), pkg.Quant(0, 300, 1, 0, d_state.data_ptr() + 2)]
    bad_ladders = [(None, None), ([], None), (R.LADDER, 0), ([1] * 17, None), (R.LADDER * 4, 17), ([0, lam_most + 1], None),
                   ([0xFFFFFFFF], None)]
    out = (d_blob, cap, d_offs, d_lens)

    def refused(call):
        with pytest.raises(pkg.AmvHipError, match=r"\(-1\)"):
            call()

    for q in bad_q:
        refused(lambda: ctx.encode_yuv420_rate_stream_dev(*planes, q, ok_rate, *out, d_rung))
        refused(lambda: ctx.encode_rate_stream_dev(pix, w * 3, 0, n, w, h, q, ok_rate, *out, d_rung))
        refused(lambda: ctx.encode_yuv420_rate_probe_dev(*planes, q, R.LADDER, d_bits))
        refused(lambda: ctx.encode_rate_probe_dev(pix, w * 3, 0, n, w, h, q, R.LADDER, d_bits))
    for ladder, rungs in bad_ladders:
        refused(lambda: ctx.encode_yuv420_rate_stream_dev(*planes, ok_q, pkg.Rate(ladder, budget=100, rungs=rungs), *out, d_rung))
        refused(lambda: ctx.encode_rate_stream_dev(pix, w * 3, 0, n, w, h, ok_q, pkg.Rate(ladder, budget=100, rungs=rungs), *out, d_rung))
        refused(lambda: ctx.encode_yuv420_rate_probe_dev(*planes, ok_q, ladder, d_bits, rungs=rungs))
        refused(lambda: ctx.encode_rate_probe_dev(pix, w * 3, 0, n, w, h, ok_q, ladder, d_bits, rungs=rungs))
    for rate, rung in ((None, d_rung), (ok_rate, None), (ok_rate, d_rung.data_ptr() + 2),
                       (pkg.Rate(R.LADDER, budget=100, d_budget=d_budget.data_ptr() + 2), d_rung)):
        refused(lambda: ctx.encode_yuv420_rate_stream_dev(*planes, ok_q, rate, *out, rung))
        refused(lambda: ctx.encode_rate_stream_dev(pix, w * 3, 0, n, w, h, ok_q, rate, *out, rung))
        refused(lambda: ctx.encode_frontend_rate_stream_dev(IR.YUVJ420P, (planes[:3],) + planes[3:7], w, h, n, None, w, h, ok_q, rate, *out, rung))
    for bits in (None, d_bits.data_ptr() + 2):
        refused(lambda: ctx.encode_yuv420_rate_probe_dev(*planes, ok_q, R.LADDER, bits))
        refused(lambda: ctx.encode_rate_probe_dev(pix, w * 3, 0, n, w, h, ok_q, R.LADDER, bits))
    for outs in ((None, cap, d_offs, d_lens), (d_blob, cap, None, d_lens), (d_blob, cap, d_offs, None)):
        refused(lambda: ctx.encode_yuv420_rate_stream_dev(*planes, ok_q, ok_rate, *outs, d_rung))
    refused(lambda: ctx.encode_yuv420_rate_stream_dev(*planes[:8], w - 1, h, ok_q, ok_rate, *out, d_rung))
    refused(lambda: ctx.encode_yuv420_rate_probe_dev(*planes[:8], w, h - 1, ok_q, R.LADDER, d_bits))
    torch.cuda.synchronize()
    assert (d_state.cpu().numpy() == state).all() and (d_blob.cpu().numpy() == FILL).all()
    assert (d_offs.cpu().numpy() == -1).all() and (d_lens.cpu().numpy() == -1).all()
    assert (d_rung.cpu().numpy() == UNWRITTEN).all() and (d_bits.cpu().numpy() == UNWRITTEN).all()
    # ... and the bounds themselves are taken: sixteen rungs, the largest lambda and nr, a budget array; n == 0 is nothing
    ladder = [lam_most] + R.LADDER * 3
    B = [100, 60, 7, 300]
    want, want_rungs, want_state = R.encode(frames, w, h, 0, nr_most, state, ladder, B)
    got = _rate(ctx, pkg, frames, w, h, ladder, B, nr=nr_most, d_state=d_state)
    _check(got, want, want_rungs, "the bounds")
    assert (d_state.cpu().numpy() == want_state).all()
    ctx.encode_yuv420_rate_stream_dev(*planes[:7], 0, w, h, ok_q, ok_rate, None, 0, None, None, None)
    ctx.encode_yuv420_rate_probe_dev(*planes[:7], 0, w, h, ok_q, R.LADDER, None)


def test_every_written_chunk_decodes(ctx, pkg):
    import torch
    w, h, frames = R.shape("50x38")
    bits, lens, esc = tables_of("50x38")
    n = len(frames)
    for kind, B in budgets_of(bits, lens, esc).items():
        blob, offs, lens_got, rungs = _rate(ctx, pkg, frames, w, h, R.LADDER, B)
        total = int(offs[-1] + lens_got[-1])
        d_out = torch.zeros((n, h, ctx.stride(w)), dtype=torch.uint8, device="cuda:0")
        d_st = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
        ctx.decode_batch_dev(_t(blob), total, _t(offs.astype(np.uint64)), _t(lens_got.astype(np.uint32)), n, w, h, 0, d_out, d_st)
        torch.cuda.synchronize()
        assert (d_st.cpu().numpy() == 0).all(), (kind, d_st.cpu().numpy())
