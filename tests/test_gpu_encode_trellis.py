"""The trellis entries (amvhip_encode_yuv420_trellis_batch_dev, its RGB and host-buffer forms, amvhip_encode_trellis_coefs_dev)
on a real MI355X against the product mode of tests/trellis_ref.py: every chunk's bytes, d_offs, d_lens, and the levels.

Shapes are the smallest that reach each path: 16x16 (one MCU), 50x38 (padding blocks both ways), 176x96 (eleven MCUs a
row: segments of 6 + 5, twelve segments, three rounds), 160x128 with a frame of saturated noise (the hand-back route
through amv_forward_kernel + amv_pack_kernel), 64x32 of crafted blocks.  The restatement is Python: a (frames, qbias,
lambda) is searched once and shared by the tests that need it."""
import numpy as np
import pytest

import nr_ref as N
import pixel_builder as pb
import trellis_ref as T
from test_gpu_parity import _t

pytestmark = pytest.mark.gpu

FILL = 0xA5
WINDOW_BITS = 1280 * 32        # amv_encode_par.hip's bit-string window: a round (four segments) beyond it is handed back
KINDS = ("ramp", "texture", "noise", "flat")
_LINES = {}


def frames_of(w, h, n, seed=21):
    return N.stream(w, h, [KINDS[i % len(KINDS)] for i in range(n)], seed + w)


def lines_of(key, frames, w, h, qbias, lam):
    """the restatement's zig-zag lines per frame, searched once per (key, qbias, lambda)"""
    k = (key, qbias, lam)
    if k not in _LINES:
        _LINES[k] = T.encode_frames(frames, w, h, qbias, lam, want_coef=True)
    return _LINES[k]


def chunks_of(lines):
    return [N._chunk(zz) for zz in lines]


def _pack(frames, w, h, pad=8):
    n, cw, ch = len(frames), w // 2, h // 2
    ys, cs = w + pad, cw + pad
    Y, Cb, Cr = np.full((n, h, ys), 0xEE, np.uint8), np.full((n, ch, cs), 0xEE, np.uint8), np.full((n, ch, cs), 0xEE, np.uint8)
    for i, (y, cb, cr) in enumerate(frames):
        Y[i, :, :w], Cb[i, :, :cw], Cr[i, :, :cw] = y, cb, cr
    return Y, Cb, Cr, ys, cs


def _outputs(ctx, n, w, h, cap):
    import torch
    cap = ctx.encode_bound(w, h) * n if cap is None else cap
    return (cap, torch.full((cap + 64,), FILL, dtype=torch.uint8, device="cuda:0"), torch.full((n,), -1, dtype=torch.int64, device="cuda:0"),
            torch.full((n,), -1, dtype=torch.int32, device="cuda:0"))


def _encode(ctx, frames, w, h, qbias, lam, cap=None, plain=False):
    """one call of the YUV420 entry (the plain one when asked) -> (blob, offs, lens) as numpy"""
    import torch
    n = len(frames)
    Y, Cb, Cr, ys, cs = _pack(frames, w, h)
    cap, d_blob, d_offs, d_lens = _outputs(ctx, n, w, h, cap)
    args = (_t(Y), _t(Cb), _t(Cr), ys, cs, h * ys, (h // 2) * cs, n, w, h, qbias)
    if plain:
        ctx.encode_yuv420_batch_dev(*args, d_blob, cap, d_offs, d_lens)
    else:
        ctx.encode_yuv420_trellis_batch_dev(*args, lam, d_blob, cap, d_offs, d_lens)
    torch.cuda.synchronize()
    return d_blob.cpu().numpy(), d_offs.cpu().numpy(), d_lens.cpu().numpy()


def _chunks(blob, offs, lens):
    return [blob[int(o): int(o) + int(l)].tobytes() for o, l in zip(offs, lens)]


def _check(blob, offs, lens, want, what):
    pos = 0
    for i, c in enumerate(want):
        assert (int(offs[i]), int(lens[i])) == (pos, len(c)), "%s: frame %d at %d + %d, want %d + %d" % (what, i, offs[i], lens[i], pos, len(c))
        got = blob[pos: pos + len(c)].tobytes()
        assert got == c, "%s: frame %d differs at byte %d of %d" % (what, i, next(k for k in range(len(c)) if got[k] != c[k]), len(c))
        pos += len(c)
    assert (blob[pos:] == FILL).all(), "%s: bytes behind the last chunk were written" % what


@pytest.fixture
def both_modes(ctx, pkg):
    def run(fn):
        try:
            for mode in (pkg.ENTROPY_AUTO, pkg.ENTROPY_SERIAL):
                ctx.set_entropy_mode(mode)
                fn("serial" if mode == pkg.ENTROPY_SERIAL else "auto")
        finally:
            ctx.set_entropy_mode(pkg.ENTROPY_AUTO)
    return run


# ---- bytes, offsets and lengths ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lam", [0, 3481, T.LAMBDA_MAX])
@pytest.mark.parametrize("qbias", [0, 128])
@pytest.mark.parametrize("w,h,n", [(16, 16, 9), (50, 38, 3), (176, 96, 1)])
def test_planes_against_the_restatement(ctx, both_modes, w, h, n, qbias, lam):
    assert ctx.encode_trellis_lambda_max() == T.LAMBDA_MAX
    frames = frames_of(w, h, n)
    want = chunks_of(lines_of((w, h, n), frames, w, h, qbias, lam))
    both_modes(lambda mode: _check(*_encode(ctx, frames, w, h, qbias, lam), want, "%dx%d x %d, qbias %d, lambda %d, %s" % (w, h, n, qbias, lam, mode)))
    if (w, h, lam) == (176, 96, 3481):
        assert want != [N._chunk(zz) for zz in T.encode_frames_plain(frames, w, h, qbias, want_coef=True)]      # the search did something


def _rgb_case(orc, w, h, n, bgr):
    pix = np.stack([orc.synth_frame(0xA11CE, 10 + t, w, h) for t in range(n)])
    return pix, [pb.to_planes(orc, pix[t], w, h, bgr) for t in range(n)]


@pytest.mark.parametrize("bgr,qbias,lam", [(0, 0, 3481), (1, 128, T.LAMBDA_MAX), (1, 0, 0)])
def test_pixels_and_host_forms(ctx, orc, both_modes, bgr, qbias, lam):
    """RGB24 / BGR24 in equal rgb24_to_yuvj420p + the YUV entry; the host-buffer forms equal the device forms"""
    import torch
    w, h, n = 50, 38, 3
    pix, frames = _rgb_case(orc, w, h, n, bgr)
    want = chunks_of(lines_of(("rgb", bgr), frames, w, h, qbias, lam))
    stride = w * 3 + 5
    padded = np.full((n, h, stride), 0xEE, np.uint8)
    padded[:, :, : w * 3] = pix.reshape(n, h, w * 3)

    def run(mode):
        cap, d_blob, d_offs, d_lens = _outputs(ctx, n, w, h, None)
        ctx.encode_trellis_batch_dev(_t(padded), stride, bgr, n, w, h, qbias, lam, d_blob, cap, d_offs, d_lens)
        torch.cuda.synchronize()
        _check(d_blob.cpu().numpy(), d_offs.cpu().numpy(), d_lens.cpu().numpy(), want, "pixels, bgr %d, %s" % (bgr, mode))
        _check(*_encode(ctx, frames, w, h, qbias, lam), want, "planes of the pixels, %s" % mode)
        hb, ho, hl = np.full(cap, FILL, np.uint8), np.zeros(n, np.uint64), np.zeros(n, np.uint32)
        ctx.encode_trellis_batch(padded, stride, bgr, n, w, h, qbias, lam, hb, cap, ho, hl)
        assert _chunks(hb, ho, hl) == want, "host pixels, %s" % mode
        Y, Cb, Cr, ys, cs = _pack(frames, w, h, 4)
        hb, ho, hl = np.full(cap, FILL, np.uint8), np.zeros(n, np.uint64), np.zeros(n, np.uint32)
        ctx.encode_yuv420_trellis_batch(Y, Cb, Cr, ys, cs, h * ys, (h // 2) * cs, n, w, h, qbias, lam, hb, cap, ho, hl)
        assert _chunks(hb, ho, hl) == want, "host planes, %s" % mode

    both_modes(run)


@pytest.mark.parametrize("bgr,qbias,lam", [(0, 0, 3481), (1, 128, T.LAMBDA_MAX), (1, 0, 0)])
def test_coefficients_against_the_restatement(ctx, orc, bgr, qbias, lam):
    """amvhip_encode_trellis_coefs_dev: the levels themselves, zig-zag order, the DC not predicted"""
    import torch
    w, h, n = 50, 38, 3
    pix, frames = _rgb_case(orc, w, h, n, bgr)
    want = np.stack(lines_of(("rgb", bgr), frames, w, h, qbias, lam))
    d_coef = torch.full(want.shape, 0x5A5A, dtype=torch.int16, device="cuda:0")
    ctx.encode_trellis_coefs_dev(_t(pix), w * 3, bgr, n, w, h, qbias, lam, d_coef)
    torch.cuda.synchronize()
    got = d_coef.cpu().numpy()
    bad = np.argwhere(got != want)
    assert not len(bad), "first difference at frame, block, position %s: %d, want %d" % (bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
    # ... and beside the plain stage access, in the same context: that one still gives the oracle's
    d_plain = torch.zeros(want.shape, dtype=torch.int16, device="cuda:0")
    ctx.encode_coefs_dev(_t(pix), w * 3, bgr, n, w, h, qbias, d_plain)
    torch.cuda.synchronize()
    for t in range(n):
        assert (d_plain[t].cpu().numpy() == orc.encode_frame(pix[t], w, h, bgr=bool(bgr), qbias=qbias, want_coef=True)[1]).all()


# ---- crafted blocks ----------------------------------------------------------------------------------------------------------------

def crafted_picture(orc):
    """64x32 of blocks made for the walk's edges, as pixel_builder makes blocks: the clipped, rounded inverse DCT of a target
    pattern (in quantiser steps), or one transform output aimed exactly.  -> (frames, [(name, comp, block index)])"""
    rng = np.random.default_rng(0x7E11)
    made = {0: [], 1: []}
    names = []

    def add(name, comp, samples):
        names.append((name, comp, len(made[comp])))
        made[comp].append(np.asarray(samples, np.int16).reshape(64))

    for comp in (0, 1):
        line = np.zeros(64)
        line[1:] = 0.45 * rng.choice([-1.0, 1.0], 63)
        add("all_below_threshold", comp, pb.samples_of(line[None], comp)[0])
        for last in (27, 28):
            line = np.zeros(64)
            line[1:last] = 0.3 * rng.choice([-1.0, 1.0], last - 1)
            line[2], line[9], line[last] = 2.6, -1.6, 1.7
            add("last_%d" % last, comp, pb.samples_of(line[None], comp)[0])
        for run in (15, 16, 31, 32, 48, 62):
            line = np.zeros(64)
            if run < 62:
                line[1] = 3.5
            line[min(run + 2, 63)] = -3.5
            add("run_%d" % run, comp, pb.samples_of(line[None], comp)[0])
        line = np.zeros(64)
        line[62], line[63] = 3.5, 3.5
        add("position_63_coded", comp, pb.samples_of(line[None], comp)[0])
        line = np.zeros(64)
        line[1] = 90.5
        add("level_of_64_or_more", comp, pb.samples_of(line[None], comp)[0])
    add("exact_tie", 0, pb._aim_output(orc, rng, 0, 6, 96))      # luma position 6: Q = 8, c = 96 = 1.5 * 64 (tests/test_trellis_ref.py)
    blocks = pb._fill(64, 32, list(made[0]), list(made[1]))
    assert len(blocks) == 1
    where = []
    for name, comp, i in names:                                   # _fill: luma block i is block i % 4 of MCU i // 4, chroma the same by 2
        where.append((name, comp, (i // 4) * 6 + i % 4 if comp == 0 else (i // 2) * 6 + 4 + i % 2))
    return [pb.planes_of_blocks(blocks[0], 64, 32)], where


def test_crafted_blocks(ctx, orc, both_modes):
    """the hand-made blocks of tests/test_trellis_ref.py as pictures.  What each reaches is asked of the restatement first:
    every shape is reached from 8-bit samples (outputs of exactly 0 under the last position come by themselves: rounding
    to pixels leaves hundreds in these blocks)"""
    frames, where = crafted_picture(orc)
    coef = T.frame_coefficients(*frames[0], 64, 32)
    at = {(name, comp): b for name, comp, b in where}
    zeros_inside = 0
    for (name, comp), b in at.items():
        qbias, lam = (128, 0) if name == "exact_tie" else (0, 3481)
        c = coef[b][T.ZIGZAG]
        trace = {}
        levels = T.trellis_block(c, comp, qbias, lam, trace=trace)
        coded = [i for i in range(1, 64) if levels[i]]
        zeros_inside += sum(1 for i in range(1, trace["last"]) if c[i] == 0)
        if name == "all_below_threshold":
            assert trace["last"] == 0 and np.abs(c[1:]).max() > 0
        elif name.startswith("last_"):
            assert trace["last"] == int(name[5:]), (name, comp, trace)
        elif name.startswith("run_"):
            run = int(name[4:])
            assert coded == ([1, run + 2] if run < 62 else [63]), (name, comp, coded)
        elif name == "position_63_coded":
            assert 63 in coded
        elif name == "level_of_64_or_more":
            assert abs(levels[1]) >= 64
        else:
            assert c[6] == 96 and levels[6] == 2 and T.trellis_block(c, comp, qbias, lam, strict=False)[6] == 1
    assert zeros_inside >= 4
    for qbias, lam in ((0, 3481), (128, 0)):
        want = chunks_of(lines_of("crafted", frames, 64, 32, qbias, lam))
        both_modes(lambda mode: _check(*_encode(ctx, frames, 64, 32, qbias, lam), want, "crafted, qbias %d, lambda %d, %s" % (qbias, lam, mode)))


# ---- the hand-back route -----------------------------------------------------------------------------------------------------------

def test_hand_back_route_equals_the_one_lane_route(ctx, pkg):
    """160x128 with one frame of saturated noise: neither of its two rounds (240 blocks each) fits the one-kernel coder's
    window, so it is coded by amv_forward_kernel + amv_pack_kernel -- whose bytes are those of the forced one-lane route"""
    w, h, qbias, lam = 160, 128, 0, 3481
    rng = np.random.default_rng(8)
    frames = N.stream(w, h, ["ramp", "flat"], 900)
    frames.insert(1, pb.planes_of_blocks(pb._noise_frame(rng, (128, 128), w, h), w, h))
    auto = _encode(ctx, frames, w, h, qbias, lam)
    try:
        ctx.set_entropy_mode(pkg.ENTROPY_SERIAL)
        serial = _encode(ctx, frames, w, h, qbias, lam)
    finally:
        ctx.set_entropy_mode(pkg.ENTROPY_AUTO)
    chunks = _chunks(*auto)
    assert chunks == _chunks(*serial) and (auto[1] == serial[1]).all() and (auto[2] == serial[2]).all()
    assert all(c[:2] == b"\xff\xd8" and c[-2:] == b"\xff\xd9" for c in chunks)
    noisy = chunks[1]
    scan_bits = 8 * (len(noisy) - 4 - noisy.count(b"\xff\x00"))
    rounds = 2                                                         # 8 MCU rows of one segment, four segments a round
    assert scan_bits > rounds * (WINDOW_BITS + 8), "the noise frame would fit the window: it did not take the hand-back route"
    assert all(8 * len(c) < WINDOW_BITS for i, c in enumerate(chunks) if i != 1)      # ... and the others did not
    # the quiet frames beside it are the restatement's
    want = chunks_of(lines_of("hand_back", [frames[0], frames[2]], w, h, qbias, lam))
    assert [chunks[0], chunks[2]] == want


# ---- capacity, arguments, round trip, the plain entries ---------------------------------------------------------------------------------

def test_blob_one_byte_short(ctx):
    w, h, n, qbias, lam = 50, 38, 3, 0, 3481
    frames = frames_of(w, h, n)
    want = chunks_of(lines_of((w, h, n), frames, w, h, qbias, lam))
    total = sum(len(c) for c in want)
    blob, offs, lens = _encode(ctx, frames, w, h, qbias, lam, cap=total - 1)
    assert int(lens[-1]) == 0 and int(offs[-1]) == total - len(want[-1])
    assert _chunks(blob, offs[:-1], lens[:-1]) == want[:-1]
    assert (blob[int(offs[-1]):] == FILL).all()
    _check(*_encode(ctx, frames, w, h, qbias, lam, cap=total), want, "a blob that just fits")


def test_refused_arguments(ctx, pkg):
    import torch
    w, h, n = 16, 16, 2
    frames = frames_of(w, h, n)
    Y, Cb, Cr, ys, cs = _pack(frames, w, h)
    cap, d_blob, d_offs, d_lens = _outputs(ctx, n, w, h, None)
    planes = (_t(Y), _t(Cb), _t(Cr), ys, cs, h * ys, (h // 2) * cs, n)
    pix = _t(np.zeros((n, h, w, 3), np.uint8))
    d_coef = torch.zeros((n, 6, 64), dtype=torch.int16, device="cuda:0")
    most = ctx.encode_trellis_lambda_max()
    for ww, hh, qbias, lam in ((w, h, 256, 0), (w, h, 0, most + 1), (w, h, 0, 0xFFFFFFFF), (w - 1, h, 0, 0), (w, h - 1, 0, 0)):
        with pytest.raises(pkg.AmvHipError, match=r"\(-1\)"):
            ctx.encode_yuv420_trellis_batch_dev(*planes, ww, hh, qbias, lam, d_blob, cap, d_offs, d_lens)
        with pytest.raises(pkg.AmvHipError, match=r"\(-1\)"):
            ctx.encode_trellis_batch_dev(pix, w * 3, 0, n, ww, hh, qbias, lam, d_blob, cap, d_offs, d_lens)
        with pytest.raises(pkg.AmvHipError, match=r"\(-1\)"):
            ctx.encode_trellis_coefs_dev(pix, w * 3, 0, n, ww, hh, qbias, lam, d_coef)
        hb, ho, hl = np.full(cap, FILL, np.uint8), np.zeros(n, np.uint64), np.zeros(n, np.uint32)
        with pytest.raises(pkg.AmvHipError, match=r"\(-1\)"):
            ctx.encode_yuv420_trellis_batch(Y, Cb, Cr, ys, cs, h * ys, (h // 2) * cs, n, ww, hh, qbias, lam, hb, cap, ho, hl)
        with pytest.raises(pkg.AmvHipError, match=r"\(-1\)"):
            ctx.encode_trellis_batch(np.zeros((n, h, w, 3), np.uint8), w * 3, 0, n, ww, hh, qbias, lam, hb, cap, ho, hl)
        assert (hb == FILL).all()
    torch.cuda.synchronize()
    assert (d_blob.cpu().numpy() == FILL).all() and not d_coef.cpu().numpy().any()
    assert (d_offs.cpu().numpy() == -1).all() and (d_lens.cpu().numpy() == -1).all()


def test_every_chunk_decodes(ctx):
    import torch
    for (w, h, n), qbias, lam in (((50, 38, 3), 0, 3481), ((176, 96, 1), 128, T.LAMBDA_MAX), ((16, 16, 9), 128, 0)):
        frames = frames_of(w, h, n)
        blob, offs, lens = _encode(ctx, frames, w, h, qbias, lam)
        total = int(offs[-1] + lens[-1])
        d_out = torch.zeros((n, h, ctx.stride(w)), dtype=torch.uint8, device="cuda:0")
        d_st = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
        ctx.decode_batch_dev(_t(blob), total, _t(offs.astype(np.uint64)), _t(lens.astype(np.uint32)), n, w, h, 0, d_out, d_st)
        torch.cuda.synchronize()
        assert (d_st.cpu().numpy() == 0).all(), (w, h, d_st.cpu().numpy())


@pytest.mark.parametrize("trellis_first", [True, False])
def test_plain_entries_beside_the_trellis_ones(ctx, orc, both_modes, trellis_first):
    """one plain call beside a trellis call in the same context, in either order: the plain entry gives the oracle's bytes"""
    w, h, n, qbias, lam = 50, 38, 3, 5, 3481
    frames = frames_of(w, h, n)
    want_plain = [orc.encode_frame_yuv(y, cb, cr, w, h, qbias=qbias) for y, cb, cr in frames]

    def run(mode):
        if trellis_first:
            got = _encode(ctx, frames, w, h, qbias, lam)
        plain = _encode(ctx, frames, w, h, qbias, 0, plain=True)
        if not trellis_first:
            got = _encode(ctx, frames, w, h, qbias, lam)
        _check(*plain, want_plain, "the plain entry, %s" % mode)
        assert _chunks(*got) != want_plain

    both_modes(run)
