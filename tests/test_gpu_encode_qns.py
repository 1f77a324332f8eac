"""The -qns entries (amvhip_encode_yuv420_qns_stream_dev, its RGB and front-end forms, amvhip_encode_qns_coefs_dev) on a real
MI355X against the product mode of tests/qns_ref.py: every chunk's bytes, d_offs, d_lens, the levels, the -nr state and
d_sse, in both entropy modes.

Shapes are the smallest that reach each path: 16x16 (one MCU), 50x38 (replicated edges both ways), 176x96 (eleven MCUs a
row: segments of 6 + 5), 16x16 x 1100 (more than one round of the coefficient workspace), 64x32 of crafted blocks.  The
model is Python: the lines a quantiser leaves for (frames, request, qbias) are made once, their refinement once per
(qns, lambda2), and shared by the tests that need them.  The model asserts for every block it walks that the cap is not
reached; the last test checks the most changes any block of this file took against what the cap was measured from."""
import numpy as np
import pytest

import img_convert_ref as R
import nr_ref as N
import nr_trellis_ref as NT
import pixel_builder as pb
import qns_ref as Q
import trellis_ref as T
from test_gpu_encode_psnr import REQUESTS, Source, _fetch, _outputs, _state, both_modes, chunks_of, old_entry, psnr_entry, ref_sse
from test_gpu_frontend import Pictures, stream
from test_gpu_parity import _t

pytestmark = pytest.mark.gpu

FILL = 0xA5
LAMBDA2 = 6962
LAMBDA2_BIG = 104531                # ... of -qscale 31
KINDS = ("ramp", "texture", "noise", "flat")
_BASE, _LINES = {}, {}


# ---- the model ------------------------------------------------------------------------------------------------------------------

def frames_of(w, h, n, seed=33):
    return N.stream(w, h, [KINDS[i % len(KINDS)] for i in range(n)], seed + w)


def base_lines(key, frames, w, h, request, qbias):
    """the zig-zag lines per frame as the request's quantiser leaves them, and the -nr state behind the last frame"""
    k = (key, request, qbias)
    if k not in _BASE:
        nr, trellis, lam = REQUESTS[request]
        state = N.new_state()
        if nr and trellis:
            lines = NT.encode_stream(frames, w, h, nr, lam, state, qbias=qbias, want_coef=True)
        elif nr:
            lines = N.encode_stream(frames, w, h, nr, state, qbias=qbias, want_coef=True)
        elif trellis:
            lines = T.encode_frames(frames, w, h, qbias, lam, want_coef=True)
        else:
            lines = T.encode_frames_plain(frames, w, h, qbias, want_coef=True)
        _BASE[k] = ([np.asarray(zz, np.int16) for zz in lines], np.asarray(state, np.int64))
    return _BASE[k]


def lines_of(key, frames, w, h, request, qbias, qns, lambda2):
    k = (key, request, qbias, qns, lambda2)
    if k not in _LINES:
        _LINES[k] = Q.refine_lines(frames, w, h, base_lines(key, frames, w, h, request, qbias)[0], qns, lambda2)
    return _LINES[k]


def chunks_model(lines):
    return [N._chunk(zz) for zz in lines]


# ---- calls ----------------------------------------------------------------------------------------------------------------------

def yuv_source(orc, frames, w, h):
    return Source(orc, "yuv", w, h, [None] * len(frames), 0, planes=list(frames))


def qns_entry(ctx, pkg, src, request, state, qns, lambda2, qbias=0, want_sse=False, cap=None):
    """-> ((blob, offs, lens), sse [n, 3] uint64 or None)"""
    import torch
    nr, trellis, lam = REQUESTS[request]
    q = pkg.Quant(qbias, nr, trellis, lam, state if nr else None)
    out = _outputs(ctx, src.n, src.w, src.h, cap)
    d_sse = torch.full((src.n, 3), -1, dtype=torch.int64, device="cuda:0") if want_sse else None
    (ctx.encode_yuv420_qns_stream_dev if src.kind == "yuv" else ctx.encode_qns_stream_dev)(*src.head(), q, qns, lambda2, *out, d_sse, stream())
    got = _fetch(out)
    return got, (d_sse.cpu().numpy().view(np.uint64) if want_sse else None)


def check(got, want, what):
    blob, offs, lens = got
    pos = 0
    for i, c in enumerate(want):
        assert (int(offs[i]), int(lens[i])) == (pos, len(c)), "%s: frame %d at %d + %d, want %d + %d" % (what, i, offs[i], lens[i], pos, len(c))
        have = blob[pos: pos + len(c)].tobytes()
        assert have == c, "%s: frame %d differs at byte %d of %d" % (what, i, next(k for k in range(len(c)) if have[k] != c[k]), len(c))
        pos += len(c)
    assert (blob[pos:] == FILL).all(), "%s: bytes behind the last chunk were written" % what


# ---- bytes, offsets and lengths ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lambda2", [0, LAMBDA2, Q.LAMBDA2_MAX])
@pytest.mark.parametrize("qns", [1, 2, 3])
@pytest.mark.parametrize("qbias", [0, 128])
@pytest.mark.parametrize("w,h,n", [(16, 16, 9), (50, 38, 3), (176, 96, 1)])
def test_planes_against_the_model(ctx, pkg, orc, w, h, n, qbias, qns, lambda2):
    assert ctx.encode_qns_lambda2_max() == Q.LAMBDA2_MAX and ctx.encode_qns_lambda2(8) == LAMBDA2
    frames = frames_of(w, h, n)
    want = chunks_model(lines_of((w, h, n), frames, w, h, "plain", qbias, qns, lambda2))
    src = yuv_source(orc, frames, w, h)
    both_modes(ctx, pkg, lambda mode: check(qns_entry(ctx, pkg, src, "plain", None, qns, lambda2, qbias)[0], want,
                                            "%dx%d x %d, qbias %d, qns %d, lambda2 %d, %s" % (w, h, n, qbias, qns, lambda2, mode)))
    if (w, h, qns) == (176, 96, 2):
        assert want != chunks_model(base_lines((w, h, n), frames, w, h, "plain", qbias)[0])      # the refinement did something


@pytest.mark.parametrize("request_name", list(REQUESTS))
def test_behind_each_quantiser(ctx, pkg, orc, request_name):
    """the refinement behind the plain quantiser, -nr, the trellis and both; the -nr state carried over two calls equals one
    call's, and is the model's (the refinement does not touch the sums)"""
    w, h, n, qns = 50, 38, 4, 2
    frames = N.stream(w, h, ["ramp", "texture", "noise", "texture"], 404)
    lines = lines_of("quantisers", frames, w, h, request_name, 0, qns, LAMBDA2)
    want, want_state = chunks_model(lines), base_lines("quantisers", frames, w, h, request_name, 0)[1]
    assert any((a != b).any() for a, b in zip(lines, base_lines("quantisers", frames, w, h, request_name, 0)[0]))
    src = yuv_source(orc, frames, w, h)

    def run(mode):
        state = _state()
        check(qns_entry(ctx, pkg, src, request_name, state, qns, LAMBDA2)[0], want, "%s, one call, %s" % (request_name, mode))
        two = _state()
        parts = []
        for lo, hi in ((0, 1), (1, 4)):
            parts += chunks_of(*qns_entry(ctx, pkg, src.part(lo, hi), request_name, two, qns, LAMBDA2)[0])
        assert parts == want, "%s, two calls, %s" % (request_name, mode)
        assert (two.cpu().numpy() == state.cpu().numpy()).all()
        if REQUESTS[request_name][0]:
            assert (state.cpu().numpy() == want_state).all(), "%s: the -nr state, %s" % (request_name, mode)

    both_modes(ctx, pkg, run)


@pytest.mark.parametrize("bgr", [0, 1])
def test_pixels_errors_and_levels(ctx, pkg, orc, bgr):
    """RGB24 / BGR24 in equal rgb24_to_yuvj420p + the planes entry; d_sse is psnr_ref on the refined levels' chunks;
    amvhip_encode_qns_coefs_dev gives the model's levels"""
    import torch
    w, h, n, qns, qbias = 50, 38, 3, 3 - bgr, 128 * bgr
    pix = [orc.synth_frame(0xA11CE, 20 + t, w, h) for t in range(n)]
    src = Source(orc, "bgr" if bgr else "rgb", w, h, [None] * n, 0, pix=pix)
    lines = lines_of(("rgb", bgr), src.planes, w, h, "trellis", qbias, qns, LAMBDA2)
    want = chunks_model(lines)
    planes = yuv_source(orc, src.planes, w, h)
    want_sse = ref_sse(orc, want, planes)

    def run(mode):
        got, sse = qns_entry(ctx, pkg, src, "trellis", None, qns, LAMBDA2, qbias, want_sse=True)
        check(got, want, "pixels, bgr %d, %s" % (bgr, mode))
        assert (sse == want_sse).all(), "d_sse, bgr %d, %s: %s, want %s" % (bgr, mode, sse.tolist(), want_sse.tolist())
        got, sse = qns_entry(ctx, pkg, planes, "trellis", None, qns, LAMBDA2, qbias, want_sse=True)
        check(got, want, "planes of the pixels, %s" % mode)
        assert (sse == want_sse).all()

    both_modes(ctx, pkg, run)
    assert (want_sse != ref_sse(orc, chunks_model(base_lines(("rgb", bgr), src.planes, w, h, "trellis", qbias)[0]), planes)).any()
    d_coef = torch.full((n, lines[0].shape[0], 64), 0x5A5A, dtype=torch.int16, device="cuda:0")
    ctx.encode_qns_coefs_dev(src.dev[0], src.stride, bgr, n, w, h, pkg.Quant(qbias, 0, 1, REQUESTS["trellis"][2], None), qns, LAMBDA2, d_coef)
    torch.cuda.synchronize()
    have = d_coef.cpu().numpy()
    bad = np.argwhere(have != np.stack(lines))
    assert not len(bad), "first difference at frame, block, position %s: %d, want %d" % (bad[0], have[tuple(bad[0])], np.stack(lines)[tuple(bad[0])])


def test_qns_0_is_the_psnr_entry(ctx, pkg, orc):
    """qns == 0: the bytes, state and errors of the _psnr entry of the request (and, with no d_sse, of the plain entries)"""
    w, h = 50, 38
    src = Source(orc, "rgb", w, h, ["ramp", "noise", "texture"], 12)
    for request in REQUESTS:
        def run(mode):
            want_state, state = _state(), _state()
            want, want_sse = psnr_entry(ctx, pkg, src, request, want_state, qbias=5)
            got, sse = qns_entry(ctx, pkg, src, request, state, 0, LAMBDA2, 5, want_sse=True)
            assert all((a == b).all() for a, b in zip(want, got)) and (sse == want_sse).all(), (request, mode)
            assert (state.cpu().numpy() == want_state.cpu().numpy()).all(), (request, mode)
            none = _state()
            got, sse = qns_entry(ctx, pkg, src, request, none, 0, 0, 5)
            assert all((a == b).all() for a, b in zip(want, got)) and sse is None and (none.cpu().numpy() == want_state.cpu().numpy()).all()
        both_modes(ctx, pkg, run)


def test_the_front_end_entry(ctx, pkg, orc):
    """deinterlace + rescale + pad, 64x48 -> 28x24 inside 32x32: the entry equals amvhip_video_frontend_dev into tight planes
    followed by the planes entry, d_sse included"""
    import torch
    W, H, n, sw, sh = 32, 32, 3, 64, 48
    fe = pkg.Frontend(1, (0, 0, 0, 0), (4, 4, 2, 2), (16, 128, 128))
    frames = [R.make_picture(R.YUV420P, sw, sh, k, 31 + 7 * i) for i, k in enumerate(("ramp", "noise", "ramp"))]
    s = Pictures(R.YUV420P, sw, sh, n).fill(frames).to_dev()
    d = Pictures(R.YUVJ420P, W, H, n).to_dev()
    ctx.video_frontend_dev(R.YUV420P, s.pic(), sw, sh, n, fe, d.pic(), W, H, stream())
    torch.cuda.synchronize()
    d.from_dev()
    two = Source.__new__(Source)
    two.kind, two.w, two.h, two.n, two.planes = "yuv", W, H, n, [tuple(d.planes(i)) for i in range(n)]
    two.dev, two.layout = tuple(d.dev), (d.stride[0], d.stride[1], d.frame[0], d.frame[1])
    want_lines = lines_of("front end", two.planes, W, H, "both", 5, 2, LAMBDA2)

    def run(mode):
        want_state, state = _state(), _state()
        want, want_sse = qns_entry(ctx, pkg, two, "both", want_state, 2, LAMBDA2, 5, want_sse=True)
        check(want, chunks_model(want_lines), "front end + planes entry, %s" % mode)
        out = _outputs(ctx, n, W, H)
        d_sse = torch.full((n, 3), -1, dtype=torch.int64, device="cuda:0")
        nr, trellis, lam = REQUESTS["both"]
        ctx.encode_frontend_qns_stream_dev(R.YUV420P, s.pic(), sw, sh, n, fe, W, H, pkg.Quant(5, nr, trellis, lam, state), 2, LAMBDA2, *out, d_sse, stream())
        got = _fetch(out)
        assert all((a == b).all() for a, b in zip(want, got)), mode
        assert (d_sse.cpu().numpy().view(np.uint64) == want_sse).all() and (state.cpu().numpy() == want_state.cpu().numpy()).all(), mode
        assert (want_sse == ref_sse(orc, chunks_of(*got), two)).all()

    both_modes(ctx, pkg, run)


def test_more_than_one_round_of_the_workspace(ctx, pkg, orc):
    """1100 frames at 16x16 (a round of the coefficient workspace is 1024): the batch equals its frames taken one call at a
    time -- every 37th of them, the first and last of both rounds among them -- and those are the model's"""
    w, h, n = 16, 16, 1100
    rng = np.random.default_rng(78)
    frames = []
    for i in range(n):
        amp = 1 + i % 120
        frames.append(tuple(np.clip(128 + rng.integers(-amp, amp + 1, s), 0, 255).astype(np.uint8) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2))))
    src = yuv_source(orc, frames, w, h)
    picked = sorted(set(range(0, n, 37)) | {1023, 1024, n - 1})

    def run(mode):
        whole, sse = qns_entry(ctx, pkg, src, "plain", None, 3, LAMBDA2, want_sse=True)
        chunks = chunks_of(*whole)
        assert all(c[:2] == b"\xff\xd8" and c[-2:] == b"\xff\xd9" for c in chunks), mode
        for i in picked:
            one, one_sse = qns_entry(ctx, pkg, src.part(i, i + 1), "plain", None, 3, LAMBDA2, want_sse=True)
            assert chunks_of(*one) == [chunks[i]] and (one_sse[0] == sse[i]).all(), "frame %d, %s" % (i, mode)
        return chunks

    both_modes(ctx, pkg, run)
    some = [picked[0], 1023, 1024, n - 1]
    want = chunks_model(lines_of("rounds", [frames[i] for i in some], w, h, "plain", 0, 3, LAMBDA2))
    whole = chunks_of(*qns_entry(ctx, pkg, src, "plain", None, 3, LAMBDA2)[0])
    assert [whole[i] for i in some] == want


# ---- crafted blocks ----------------------------------------------------------------------------------------------------------------

def _line(**at):
    line = np.zeros(64)
    for k, v in at.items():
        line[int(k[1:])] = v
    return line


def crafted_picture():
    """64x32 of blocks made for the walk's edges, as pixel_builder makes blocks (the clipped, rounded inverse DCT of a target
    pattern in quantiser steps) -> (frames, {name: (comp, block index, samples 0 .. 255)})"""
    made, names = {0: [], 1: []}, []

    def add(name, comp, samples):
        names.append((name, comp, len(made[comp])))
        made[comp].append(np.asarray(samples, np.int16).reshape(64))

    for comp in (0, 1):
        add("flat", comp, np.zeros(64))
        add("flat_0", comp, np.full(64, -128))                   # the DC at the lower edge of 0 <= level * Q + 1024
        add("flat_255", comp, np.full(64, 127))                  # ... and at the upper one
        add("past_last", comp, pb.samples_of(_line(p1=3.5, p10=0.93)[None], comp)[0])
        add("eob_moves", comp, pb.samples_of(_line(p1=3.5, p30=1.08)[None], comp)[0])
        add("position_63", comp, pb.samples_of(_line(p62=3.5, p63=3.5)[None], comp)[0])
        add("zrl_goes", comp, pb.samples_of(_line(p1=3.5, p20=0.93, p40=3.5)[None], comp)[0])
        add("size_class", comp, pb.samples_of(_line(p1=3.5, p3=1.93)[None], comp)[0])
    # blocks that are their own transpose: where a scan position and its mirror have equal steps their candidates tie at
    # lambda2 0 (these two seeds: found by walking the model over 400 of them; the test asks the model again)
    for seed in (9, 29):
        tie = np.random.default_rng([0x71E, seed])
        amp = int(tie.integers(5, 60))
        half = tie.integers(-amp, amp + 1, (8, 8))
        add("tie_%d" % seed, 0, np.clip(half + half.T + np.add.outer(np.arange(8), np.arange(8)) * int(tie.integers(0, 8)) - 30, -128, 127))
    # part flat, part busy: the weights pull the DC towards the flat part (rare: these two of 600 seeds, found with the model)
    for seed in (42, 239):
        dc = np.random.default_rng([0xDC, seed])
        amp = int(dc.integers(10, 120))
        busy = dc.integers(-amp, amp + 1, (8, 8))
        cols = int(dc.integers(2, 7))
        busy[:, :cols] = int(dc.integers(-90, 91))
        add("dc_first_%d" % seed, 0, np.clip(busy, -128, 127))
    blocks = pb._fill(64, 32, list(made[0]), list(made[1]))
    assert len(blocks) == 1
    frames = [pb.planes_of_blocks(blocks[0], 64, 32)]
    where = {}
    for name, comp, i in names:                                   # _fill: luma block i is block i % 4 of MCU i // 4, chroma the same by 2
        b = (i // 4) * 6 + i % 4 if comp == 0 else (i // 2) * 6 + 4 + i % 2
        where[(name, comp)] = (b, blocks[0][b].astype(np.int64) + 128)
    return frames, where


def test_crafted_blocks(ctx, pkg, orc):
    """hand-made blocks as a picture.  What each reaches is asked of the model first (its trace: position, change,
    last_non_zero then, the level before, ties), then the picture goes through the entry at the settings that reach it"""
    frames, where = crafted_picture()
    w, h = 64, 32
    base = base_lines("crafted", frames, w, h, "plain", 0)[0][0]

    def walk(name, comp, qns, lambda2, **variant):
        b, p = where[(name, comp)]
        trace = {}
        levels, changes = Q.qns_block(p, base[b], comp, qns, lambda2, trace=trace, **variant)
        return levels, trace.get("picks", []), [int(x) for x in base[b]]

    for comp in (0, 1):
        assert walk("flat", comp, 3, 0)[1] == []                                              # no change
        for name, step in (("flat_0", -1), ("flat_255", 1)):
            start = walk(name, comp, 3, 0)[2]
            assert not Q._Product(comp).dc_ok(start[0] + step) and Q._Product(comp).dc_ok(start[0] - step), (name, comp, start[0])
        levels, picks, start = walk("past_last", comp, 3, 0)
        assert start[10] == 0 and max(i for i in range(1, 64) if start[i]) < 9 and any(p[0] == 10 and p[0] > p[2] + 1 for p in picks), (comp, picks)
        assert walk("past_last", comp, 2, 0)[0][10] == 0 and levels[10] != 0                  # a change only qns 3 makes
        levels, picks, start = walk("eob_moves", comp, 1, LAMBDA2_BIG)
        assert abs(start[30]) == 1 and not any(start[31:]) and levels[30] == 0 and (30, -start[30]) in [(p[0], p[1]) for p in picks], (comp, picks)
        levels, picks, start = walk("position_63", comp, 2, LAMBDA2)
        assert start[63] and levels[63], comp                                                  # position 63 coded: no EOB
        levels, picks, start = walk("zrl_goes", comp, 2, 0)
        assert start[20] == 0 and start[1] and start[40] and not any(start[2:40]) and levels[20] != 0, (comp, picks)   # a run of 38 splits
        levels, picks, start = walk("size_class", comp, 2, 0)
        assert abs(start[3]) == 1 and abs(levels[3]) == 2, (comp, start[3], levels[3])          # one magnitude bit more
    for seed in (9, 29):
        levels, picks, start = walk("tie_%d" % seed, 0, 3, 0)
        assert any(p[4] > 0 for p in picks), picks                                             # a winner that was tied ...
        assert walk("tie_%d" % seed, 0, 3, 0, strict=False)[0] != levels                       # ... and the later candidate would have changed the block
    for seed in (42, 239):
        picks = walk("dc_first_%d" % seed, 0, 3, 0)[1]
        assert picks and picks[0][0] == 0, picks[:2]                                           # a block whose first change is the DC
    src = yuv_source(orc, frames, w, h)
    for qns, lambda2 in ((3, 0), (2, 0), (1, LAMBDA2_BIG), (2, LAMBDA2)):
        want = chunks_model(lines_of("crafted", frames, w, h, "plain", 0, qns, lambda2))
        both_modes(ctx, pkg, lambda mode: check(qns_entry(ctx, pkg, src, "plain", None, qns, lambda2)[0], want,
                                                "crafted, qns %d, lambda2 %d, %s" % (qns, lambda2, mode)))


# ---- round trip, arguments, the entries beside it -------------------------------------------------------------------------------------

def test_every_chunk_decodes(ctx, pkg, orc):
    import torch
    for (w, h, n), qns, lambda2 in (((50, 38, 3), 3, 0), ((176, 96, 1), 2, Q.LAMBDA2_MAX), ((16, 16, 9), 1, LAMBDA2)):
        blob, offs, lens = qns_entry(ctx, pkg, yuv_source(orc, frames_of(w, h, n), w, h), "plain", None, qns, lambda2)[0]
        total = int(offs[-1] + lens[-1])
        d_out = torch.zeros((n, h, ctx.stride(w)), dtype=torch.uint8, device="cuda:0")
        d_st = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
        ctx.decode_batch_dev(_t(blob), total, _t(offs.astype(np.uint64)), _t(lens.astype(np.uint32)), n, w, h, 0, d_out, d_st)
        torch.cuda.synchronize()
        assert (d_st.cpu().numpy() == 0).all(), (w, h, d_st.cpu().numpy())


def test_refused_arguments(ctx, pkg, orc):
    """qns > 3, lambda2 above the bound, a misaligned d_sse, what the entries of q refuse, odd sizes, null outputs:
    AMVHIP_ERR_ARG before anything is written.  (A null d_sse is not refused: errors not wanted.)"""
    import torch
    w, h, n = 48, 32, 2
    state = torch.arange(65, dtype=torch.int32, device="cuda:0")
    out = _outputs(ctx, n, w, h)
    d_sse = torch.full((n, 3), -1, dtype=torch.int64, device="cuda:0")
    d_coef = torch.zeros((n, 36, 64), dtype=torch.int16, device="cuda:0")
    nr, lam = 1200, 3481
    ok_q = pkg.Quant(0, nr, 1, lam, state)
    most = ctx.encode_qns_lambda2_max()
    bad_q = [None, pkg.Quant(0, nr, 0, 0, None), pkg.Quant(0, ctx.encode_nr_max(w, h) + 1, 1, lam, state),
             pkg.Quant(0, nr, 1, ctx.encode_trellis_lambda_max() + 1, state), pkg.Quant(0, nr, 2, lam, state), pkg.Quant(256, nr, 1, lam, state),
             pkg.Quant(0, nr, 1, lam, state.data_ptr() + 2)]
    s = Pictures(R.YUV420P, 64, 48, n).to_dev()
    for kind in ("yuv", "rgb"):
        src = Source(orc, kind, w, h, ["ramp", "noise"], 3)
        entry = ctx.encode_yuv420_qns_stream_dev if kind == "yuv" else ctx.encode_qns_stream_dev
        calls = [(src.head(), q, 2, LAMBDA2, out, d_sse) for q in bad_q]
        calls += [(src.head(), ok_q, 4, LAMBDA2, out, d_sse), (src.head(), ok_q, 0xFFFFFFFF, 0, out, d_sse), (src.head(), ok_q, 2, most + 1, out, d_sse),
                  (src.head(), ok_q, 0, most + 1, out, d_sse), (src.head(), ok_q, 2, 0xFFFFFFFF, out, None), (src.head(), ok_q, 2, LAMBDA2, out, d_sse.data_ptr() + 4)]
        calls += [(src.head()[:-2] + (w - 1, h), ok_q, 2, LAMBDA2, out, d_sse), (src.head()[:-2] + (w, h - 1), ok_q, 2, LAMBDA2, out, d_sse)]
        calls += [(src.head(), ok_q, 2, LAMBDA2, (None,) + out[1:], d_sse), (src.head(), ok_q, 2, LAMBDA2, out[:2] + (None, out[3]), d_sse),
                  (src.head(), ok_q, 2, LAMBDA2, out[:3] + (None,), d_sse)]
        for head, q, qns, lambda2, o, sse in calls:
            with pytest.raises(pkg.AmvHipError, match=r"\(-1\)"):
                entry(*head, q, qns, lambda2, *o, sse, stream())
        if kind == "rgb":
            for q, qns, lambda2 in [(x, 2, LAMBDA2) for x in bad_q] + [(ok_q, 4, LAMBDA2), (ok_q, 2, most + 1)]:
                with pytest.raises(pkg.AmvHipError, match=r"\(-1\)"):
                    ctx.encode_qns_coefs_dev(*src.head(), q, qns, lambda2, d_coef, stream())
            with pytest.raises(pkg.AmvHipError, match=r"\(-1\)"):
                ctx.encode_qns_coefs_dev(*src.head(), ok_q, 2, LAMBDA2, d_coef.data_ptr() + 8, stream())
    for q, qns, lambda2, sse in [(x, 2, LAMBDA2, d_sse) for x in bad_q] + [(ok_q, 4, LAMBDA2, d_sse), (ok_q, 2, most + 1, d_sse), (ok_q, 2, LAMBDA2, d_sse.data_ptr() + 4)]:
        with pytest.raises(pkg.AmvHipError, match=r"\(-1\)"):
            ctx.encode_frontend_qns_stream_dev(R.YUV420P, s.pic(), 64, 48, n, pkg.Frontend(1), w, h, q, qns, lambda2, *out, sse, stream())
    torch.cuda.synchronize()
    assert (out[0].cpu().numpy() == FILL).all() and (out[2].cpu().numpy() == -1).all() and (out[3].cpu().numpy() == -1).all()
    assert (d_sse.cpu().numpy() == -1).all() and (state.cpu().numpy() == np.arange(65)).all() and not d_coef.cpu().numpy().any()
    # no frames: fine, and nothing is written
    src = Source(orc, "yuv", w, h, ["ramp", "noise"], 3)
    ctx.encode_yuv420_qns_stream_dev(*src.head()[:-3], 0, w, h, ok_q, 2, LAMBDA2, *out, d_sse, stream())
    torch.cuda.synchronize()
    assert (d_sse.cpu().numpy() == -1).all() and (state.cpu().numpy() == np.arange(65)).all()


def test_old_entries_before_and_after(ctx, pkg, orc):
    """the plain, -nr and trellis entries called before and after a qns call, in one context: their bytes do not move, and
    the plain entry's are the oracle's"""
    w, h = 50, 38
    src = yuv_source(orc, frames_of(w, h, 3), w, h)

    def run(mode):
        before = {r: old_entry(ctx, src, r, _state(), qbias=5) for r in REQUESTS}
        got = qns_entry(ctx, pkg, src, "both", _state(), 3, LAMBDA2, 5, want_sse=True)[0]
        for r in REQUESTS:
            after = old_entry(ctx, src, r, _state(), qbias=5)
            assert all((a == b).all() for a, b in zip(before[r], after)), (r, mode)
        assert chunks_of(*before["plain"]) == [orc.encode_frame_yuv(y, cb, cr, w, h, qbias=5) for y, cb, cr in src.planes], mode
        assert chunks_of(*got) != chunks_of(*before["both"]), mode

    both_modes(ctx, pkg, run)


def test_no_block_reached_the_cap():
    """(last) every block the model walked for this file stopped by itself (refine_lines asserts it), and none took more
    changes than the count the cap was derived from"""
    lines_of((16, 16, 9), frames_of(16, 16, 9), 16, 16, "plain", 0, 3, 0)      # (walked already unless this test runs alone)
    assert 0 < Q.most_changes() <= Q.CHANGES_SEEN, Q.most_changes()
