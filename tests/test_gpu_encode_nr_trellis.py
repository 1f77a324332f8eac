"""-nr and the trellis quantiser in one call (amvhip_encode_yuv420_nr_trellis_stream_dev, its RGB and host-buffer forms) on a
real MI355X against tests/nr_trellis_ref.py: every chunk's bytes, d_offs, d_lens, no byte behind the last chunk, and the
state that comes out.

Shapes are the smallest that reach each path: 48x32 (one segment a row), 176x120 (eleven MCUs a row: two segments, and half
an MCU row of padding blocks), 22x38 (padding blocks both ways), 16x16 with a count next to 65536 (the halving inside the
call), 160x128 with a frame of saturated noise (the hand-back route through amv_forward_kernel + amv_pack_kernel).  The
restatement is Python: a stream is searched once and shared by the tests that need it."""
import numpy as np
import pytest

import nr_ref as N
import nr_trellis_ref as NT
import pixel_builder as pb
import trellis_ref as T
from test_gpu_parity import _t

pytestmark = pytest.mark.gpu

FILL = 0xA5
WINDOW_BITS = 1280 * 32        # amv_encode_par.hip's bit-string window: a round (four segments) beyond it is handed back
_MODEL = {}


def model_of(key, frames, w, h, nr, lam, state=None, qbias=0):
    """the restatement's (chunks, state afterwards) from `state` (all zero when None), made once per key"""
    k = (key, nr, lam, qbias)
    if k not in _MODEL:
        s = N.new_state() if state is None else np.array(state, np.int64)
        _MODEL[k] = (NT.encode_stream(frames, w, h, nr, lam, state=s, qbias=qbias), s)
    return _MODEL[k]


def _pack(frames, w, h, pad=8):
    """planes of n frames as the entries take them, rows padded by `pad` poison bytes"""
    n, cw, ch = len(frames), w // 2, h // 2
    ys, cs = w + pad, cw + pad
    Y, Cb, Cr = np.full((n, h, ys), 0xEE, np.uint8), np.full((n, ch, cs), 0xEE, np.uint8), np.full((n, ch, cs), 0xEE, np.uint8)
    for i, (y, cb, cr) in enumerate(frames):
        Y[i, :, :w], Cb[i, :, :cw], Cr[i, :, :cw] = y, cb, cr
    return Y, Cb, Cr, ys, cs


def _state_dev(state):
    return _t(np.asarray(state, np.int64).astype(np.int32))


def _outputs(ctx, n, w, h, cap):
    import torch
    cap = ctx.encode_bound(w, h) * n if cap is None else cap
    return (cap, torch.full((cap + 64,), FILL, dtype=torch.uint8, device="cuda:0"), torch.full((n,), -1, dtype=torch.int64, device="cuda:0"),
            torch.full((n,), -1, dtype=torch.int32, device="cuda:0"))


def _encode(ctx, frames, w, h, nr, lam, d_state, qbias=0, cap=None, entry="both"):
    """one call of a YUV420 entry -- "both", or "nr", "trellis", "plain" with the arguments each takes -> (blob, offs, lens)"""
    import torch
    n = len(frames)
    Y, Cb, Cr, ys, cs = _pack(frames, w, h)
    cap, d_blob, d_offs, d_lens = _outputs(ctx, n, w, h, cap)
    args = (_t(Y), _t(Cb), _t(Cr), ys, cs, h * ys, (h // 2) * cs, n, w, h, qbias)
    out = (d_blob, cap, d_offs, d_lens)
    if entry == "both":
        ctx.encode_yuv420_nr_trellis_stream_dev(*args, nr, lam, d_state, *out)
    elif entry == "nr":
        ctx.encode_yuv420_nr_stream_dev(*args, nr, d_state, *out)
    elif entry == "trellis":
        ctx.encode_yuv420_trellis_batch_dev(*args, lam, *out)
    else:
        ctx.encode_yuv420_batch_dev(*args, *out)
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


def _run_case(ctx, key, frames, w, h, nr, lam, state=None, qbias=0, mode=""):
    """the combined YUV420 entry from `state` against the restatement: chunks, offsets, lengths, the fill, the state"""
    want, want_state = model_of(key, frames, w, h, nr, lam, state, qbias)
    d_state = _state_dev(N.new_state() if state is None else state)
    what = "%dx%d x %d, nr %d, lambda %d, qbias %d %s" % (w, h, len(frames), nr, lam, qbias, mode)
    _check(*_encode(ctx, frames, w, h, nr, lam, d_state, qbias), want, what)
    got_state = d_state.cpu().numpy()
    assert (got_state == want_state).all(), "%s: state differs at %s" % (what, np.flatnonzero(got_state != want_state)[:8])
    return want


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


# ---- bytes, offsets, lengths and the state --------------------------------------------------------------------------------------

@pytest.mark.parametrize("lam", [3481, 0, T.LAMBDA_MAX])
def test_dead_zone_and_search_together(ctx, both_modes, lam):
    """48x32 x 6 "ramp" at nr 3000.  Frame 0 starts from the all-zero state, so its offsets are 0: its chunk is the trellis
    entry's, the later ones are not; every chunk differs from the -nr entry's.  (At the bound on lambda nearly every AC level
    is dropped with or without the dead zone: there one later chunk that differs is asked for, not all.)"""
    w, h, nr = 48, 32, 3000
    frames = N.stream(w, h, ["ramp"] * 6, 100)
    want = []
    both_modes(lambda mode: want.append(_run_case(ctx, "ramp", frames, w, h, nr, lam, mode=mode)))
    trellis = _chunks(*_encode(ctx, frames, w, h, 0, lam, None, entry="trellis"))
    alone = _chunks(*_encode(ctx, frames, w, h, nr, 0, _state_dev(N.new_state()), entry="nr"))
    assert want[0][0] == trellis[0]
    later = [a != b for a, b in zip(want[0][1:], trellis[1:])]
    assert any(later) if lam == T.LAMBDA_MAX else all(later)
    assert all(a != b for a, b in zip(want[0], alone))


def test_truncation_under_the_search(ctx):
    """two flat frames, then texture at nr 911: 911 * 72 / 1 = 65592 is stored as 56, and the search sees what that leaves"""
    w, h, kinds = 48, 32, ["flat", "flat"] + ["texture"] * 4
    frames = N.stream(w, h, kinds, 300)
    want = _run_case(ctx, "truncation", frames, w, h, 911, 3481)
    assert NT.encode_stream(frames[:3], w, h, 911, 3481, truncate=False)[2] != want[2]


def test_two_segments_and_padding_blocks(ctx, both_modes):
    """176x120: eleven MCUs a row (segments of 6 + 5), the last MCU row half outside the picture; 22x38: padding blocks both
    ways; qbias on the way"""
    big = N.stream(176, 120, ["texture", "ramp", "texture"], 500)
    small = N.stream(22, 38, ["texture", "ramp"], 520)

    def run(mode):
        _run_case(ctx, "176x120", big, 176, 120, 1200, 3481, qbias=40, mode=mode)
        _run_case(ctx, "22x38", small, 22, 38, 600, 870, qbias=128, mode=mode)

    both_modes(run)


def test_halving_inside_the_call(ctx):
    """16x16 x 4 from a count of 65530 (the state and seed of test_gpu_encode_nr.py::test_halving_inside_the_call): 65536
    after frame 0 (stays), 65542 after frame 1: frame 2 starts by halving, and frame 3 differs from a model without it"""
    rng = np.random.default_rng(3)
    state = np.concatenate([rng.integers(0, 16320 * 65530, 64), [65530]])
    state[:3] = (0, 7, 16320 * 65530)
    frames = N.stream(16, 16, ["texture", "ramp", "texture", "ramp"], 40)
    want = _run_case(ctx, "halving", frames, 16, 16, 4000, 870, state=state)
    assert model_of("halving", frames, 16, 16, 4000, 870)[1][64] == 32783
    assert NT.encode_stream(frames, 16, 16, 4000, 870, state=np.array(state, np.int64), halve=False)[3] != want[3]


def test_hand_back_route(ctx, pkg):
    """160x128 with test_gpu_encode_trellis.py's saturated-noise frame between "ramp" and "flat": neither of its two rounds
    fits the one-kernel coder's window, so it is coded by amv_forward_kernel + amv_pack_kernel -- with the offsets and the
    search (its scan is 149 664 bits by the count below against the 81 936 of two windows; the quiet chunks fit one).  Auto,
    serial and the restatement agree on all three chunks"""
    w, h, nr, lam = 160, 128, 3000, 3481
    frames = N.stream(w, h, ["ramp", "flat"], 900)
    frames.insert(1, pb.planes_of_blocks(pb._noise_frame(np.random.default_rng(8), (128, 128), w, h), w, h))
    want = _run_case(ctx, "hand_back", frames, w, h, nr, lam, mode="auto")
    try:
        ctx.set_entropy_mode(pkg.ENTROPY_SERIAL)
        _run_case(ctx, "hand_back", frames, w, h, nr, lam, mode="serial")
    finally:
        ctx.set_entropy_mode(pkg.ENTROPY_AUTO)
    noisy = want[1]
    scan_bits = 8 * (len(noisy) - 4 - noisy.count(b"\xff\x00"))
    rounds = 2                                                         # 8 MCU rows of one segment, four segments a round
    assert scan_bits > rounds * (WINDOW_BITS + 8), "the noise frame would fit the window: it did not take the hand-back route"
    assert all(8 * len(c) < WINDOW_BITS for i, c in enumerate(want) if i != 1)      # ... and the others did not
    assert noisy != _chunks(*_encode(ctx, frames[1:2], w, h, 0, lam, None, entry="trellis"))[0]


def test_one_call_equals_calls_with_the_state_carried(ctx):
    w, h, nr, lam = 48, 32, 1500, 3481
    frames = N.stream(w, h, ["ramp", "texture", "flat", "texture", "ramp", "texture", "texture", "ramp"], 77)
    whole_state = _state_dev(N.new_state())
    whole = _chunks(*_encode(ctx, frames, w, h, nr, lam, whole_state))
    d_state, parts = _state_dev(N.new_state()), []
    for lo, hi in ((0, 3), (3, 4), (4, 8)):
        parts += _chunks(*_encode(ctx, frames[lo:hi], w, h, nr, lam, d_state))
    assert parts == whole
    assert (d_state.cpu().numpy() == whole_state.cpu().numpy()).all()
    want, want_state = model_of("carried", frames, w, h, nr, lam)
    assert whole == want and (whole_state.cpu().numpy() == want_state).all()


def test_nr_0_is_the_trellis_entry(ctx):
    w, h, lam = 48, 32, 3481
    frames = N.stream(w, h, ["ramp", "texture", "noise"], 60)
    state = np.arange(65) * 1000 + 7
    d_state = _state_dev(state)
    got = _encode(ctx, frames, w, h, 0, lam, d_state, qbias=5)
    assert (d_state.cpu().numpy() == state).all()
    trellis = _encode(ctx, frames, w, h, 0, lam, None, qbias=5, entry="trellis")
    assert all((a == b).all() for a, b in zip(got, trellis))
    _check(*got, T.encode_frames(frames, w, h, 5, lam), "nr 0")
    # nr 0 takes no state at all
    assert all((a == b).all() for a, b in zip(_encode(ctx, frames, w, h, 0, lam, None, qbias=5), trellis))
    # ... and lambda 0 is the trellis at lambda 0, not the plain quantiser
    zero = _encode(ctx, frames, w, h, 0, 0, None, qbias=5)
    assert all((a == b).all() for a, b in zip(zero, _encode(ctx, frames, w, h, 0, 0, None, qbias=5, entry="trellis")))
    assert _chunks(*zero) != _chunks(*_encode(ctx, frames, w, h, 0, 0, None, qbias=5, entry="plain"))


@pytest.mark.parametrize("bgr", [0, 1])
def test_rgb_entry_and_host_forms(ctx, orc, bgr):
    """RGB24 / BGR24 in equal rgb24_to_yuvj420p + the YUV entry; the host-buffer forms equal the device forms"""
    import torch
    w, h, n, nr, lam = 48, 32, 3, 800, 3481
    pix = np.stack([orc.synth_frame(0xA11CE, 10 + t, w, h) for t in range(n)])
    frames = [pb.to_planes(orc, pix[t], w, h, bgr) for t in range(n)]
    want, want_state = model_of(("rgb", bgr), frames, w, h, nr, lam)
    _run_case(ctx, ("rgb", bgr), frames, w, h, nr, lam)
    stride = w * 3 + 5
    padded = np.full((n, h, stride), 0xEE, np.uint8)
    padded[:, :, : w * 3] = pix.reshape(n, h, w * 3)
    cap, d_blob, d_offs, d_lens = _outputs(ctx, n, w, h, None)
    d_state = _state_dev(N.new_state())
    ctx.encode_nr_trellis_stream_dev(_t(padded), stride, bgr, n, w, h, 0, nr, lam, d_state, d_blob, cap, d_offs, d_lens)
    torch.cuda.synchronize()
    _check(d_blob.cpu().numpy(), d_offs.cpu().numpy(), d_lens.cpu().numpy(), want, "pixels, bgr %d" % bgr)
    assert (d_state.cpu().numpy() == want_state).all()
    # host-buffer forms, the stream in two calls
    for form in ("pixels", "planes"):
        state = np.zeros(65, np.int32)
        got = []
        for lo, hi in ((0, 1), (1, n)):
            m = hi - lo
            hb, ho, hl = np.full(cap, FILL, np.uint8), np.zeros(m, np.uint64), np.zeros(m, np.uint32)
            if form == "pixels":
                ctx.encode_nr_trellis_stream(np.ascontiguousarray(padded[lo:hi]), stride, bgr, m, w, h, 0, nr, lam, state, hb, cap, ho, hl)
            else:
                Y, Cb, Cr, ys, cs = _pack(frames[lo:hi], w, h, 4)
                ctx.encode_yuv420_nr_trellis_stream(Y, Cb, Cr, ys, cs, h * ys, (h // 2) * cs, m, w, h, 0, nr, lam, state, hb, cap, ho, hl)
            got += _chunks(hb, ho, hl)
            assert (hb[int(ho[-1]) + int(hl[-1]):] == FILL).all(), form
        assert got == want and (state == want_state).all(), form


# ---- capacity, arguments, round trip, the old entries ---------------------------------------------------------------------------

def test_short_blob_and_refused_arguments(ctx, pkg):
    import torch
    w, h, nr, lam = 48, 32, 3000, 3481
    frames = N.stream(w, h, ["ramp"] * 6, 100)[:4]
    want, want_state = model_of("ramp4", frames, w, h, nr, lam)
    total = sum(len(c) for c in want)
    d_state = _state_dev(N.new_state())
    blob, offs, lens = _encode(ctx, frames, w, h, nr, lam, d_state, cap=total - 1)
    assert int(lens[-1]) == 0 and int(offs[-1]) == total - len(want[-1])
    assert _chunks(blob, offs[:-1], lens[:-1]) == want[:-1]
    assert (blob[int(offs[-1]):] == FILL).all()
    assert (d_state.cpu().numpy() == want_state).all()                 # the state has moved on all the same
    _check(*_encode(ctx, frames, w, h, nr, lam, _state_dev(N.new_state()), cap=total), want, "a blob that just fits")
    # the host forms say so with AMVHIP_ERR_SPACE
    Y, Cb, Cr, ys, cs = _pack(frames, w, h)
    hb, ho, hl = np.zeros(total - 1, np.uint8), np.zeros(4, np.uint64), np.zeros(4, np.uint32)
    with pytest.raises(pkg.AmvHipError, match=r"\(-4\)"):
        ctx.encode_yuv420_nr_trellis_stream(Y, Cb, Cr, ys, cs, h * ys, (h // 2) * cs, 4, w, h, 0, nr, lam, np.zeros(65, np.int32), hb, total - 1, ho, hl)
    with pytest.raises(pkg.AmvHipError, match=r"\(-4\)"):
        ctx.encode_nr_trellis_stream(np.zeros((4, h, w, 3), np.uint8), w * 3, 0, 4, w, h, 0, nr, lam, np.zeros(65, np.int32), hb, 8, ho, hl)
    # nr above its bound, lambda above its, a null or misaligned state, odd sizes, null outputs
    nr_most, lam_most = ctx.encode_nr_max(w, h), ctx.encode_trellis_lambda_max()
    assert (nr_most, lam_most) == (24607, T.LAMBDA_MAX)
    d_state = _state_dev(np.arange(65))
    cap, d_blob, d_offs, d_lens = _outputs(ctx, 4, w, h, 4096)
    planes = (_t(Y), _t(Cb), _t(Cr), ys, cs, h * ys, (h // 2) * cs, 4)
    pix = _t(np.zeros((4, h, w, 3), np.uint8))
    out = (d_blob, cap, d_offs, d_lens)
    bad = [(w, h, nr_most + 1, lam, d_state, out), (w, h, 0xFFFFFFFF, lam, d_state, out), (w, h, nr, lam_most + 1, d_state, out),
           (w, h, 0, 0xFFFFFFFF, d_state, out), (w, h, nr, lam, None, out), (w, h, nr, lam, d_state.data_ptr() + 2, out),
           (w - 1, h, nr, lam, d_state, out), (w, h - 1, nr, lam, d_state, out), (w, h, nr, lam, d_state, (None, cap, d_offs, d_lens)),
           (w, h, nr, lam, d_state, (d_blob, cap, None, d_lens)), (w, h, nr, lam, d_state, (d_blob, cap, d_offs, None))]
    for ww, hh, bad_nr, bad_lam, bad_state, outs in bad:
        with pytest.raises(pkg.AmvHipError, match=r"\(-1\)"):
            ctx.encode_yuv420_nr_trellis_stream_dev(*planes, ww, hh, 0, bad_nr, bad_lam, bad_state, *outs)
        with pytest.raises(pkg.AmvHipError, match=r"\(-1\)"):
            ctx.encode_nr_trellis_stream_dev(pix, w * 3, 0, 4, ww, hh, 0, bad_nr, bad_lam, bad_state, *outs)
    hb, ho, hl = np.full(cap, FILL, np.uint8), np.zeros(4, np.uint64), np.zeros(4, np.uint32)
    for bad_nr, bad_lam, bad_state in ((nr_most + 1, lam, np.zeros(65, np.int32)), (nr, lam_most + 1, np.zeros(65, np.int32)), (nr, lam, None)):
        with pytest.raises(pkg.AmvHipError, match=r"\(-1\)"):
            ctx.encode_yuv420_nr_trellis_stream(Y, Cb, Cr, ys, cs, h * ys, (h // 2) * cs, 4, w, h, 0, bad_nr, bad_lam, bad_state, hb, cap, ho, hl)
        with pytest.raises(pkg.AmvHipError, match=r"\(-1\)"):
            ctx.encode_nr_trellis_stream(np.zeros((4, h, w, 3), np.uint8), w * 3, 0, 4, w, h, 0, bad_nr, bad_lam, bad_state, hb, cap, ho, hl)
    torch.cuda.synchronize()
    assert (d_state.cpu().numpy() == np.arange(65)).all() and (d_blob.cpu().numpy() == FILL).all() and (hb == FILL).all()
    assert (d_offs.cpu().numpy() == -1).all() and (d_lens.cpu().numpy() == -1).all()
    # ... and both bounds themselves are taken
    small = N.stream(16, 16, ["texture", "ramp"], 11)
    _run_case(ctx, "bounds", small, 16, 16, ctx.encode_nr_max(16, 16), lam_most)


def test_every_chunk_decodes(ctx):
    import torch
    w, h = 48, 32
    frames = N.stream(w, h, ["ramp", "texture", "flat", "noise", "texture"], 4)
    blob, offs, lens = _encode(ctx, frames, w, h, 3000, 3481, _state_dev(N.new_state()))
    n = len(frames)
    total = int(offs[-1] + lens[-1])
    d_out = torch.zeros((n, h, ctx.stride(w)), dtype=torch.uint8, device="cuda:0")
    d_st = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    ctx.decode_batch_dev(_t(blob), total, _t(offs.astype(np.uint64)), _t(lens.astype(np.uint32)), n, w, h, 0, d_out, d_st)
    torch.cuda.synchronize()
    assert (d_st.cpu().numpy() == 0).all(), d_st.cpu().numpy()


def test_old_entries_beside_the_new_ones(ctx, orc, both_modes):
    """the plain, -nr and trellis entries before and after a combined call on the same context: each gives its own bytes (and
    the -nr entry its own state), so nothing lingers in the workspace"""
    w, h, nr, lam, qbias = 48, 32, 3000, 3481, 5
    frames = N.stream(w, h, ["ramp"] * 6, 100)[:3]
    want_plain = [orc.encode_frame_yuv(y, cb, cr, w, h, qbias=qbias) for y, cb, cr in frames]
    nr_state = N.new_state()
    want_nr = N.encode_stream(frames, w, h, nr, state=nr_state, qbias=qbias)
    want_trellis = T.encode_frames(frames, w, h, qbias, lam)
    want_both, _ = model_of("ramp3", frames, w, h, nr, lam, qbias=qbias)
    assert len({tuple(x) for x in (want_plain, want_nr, want_trellis, want_both)}) == 4

    def old(mode, when):
        _check(*_encode(ctx, frames, w, h, 0, 0, None, qbias, entry="plain"), want_plain, "the plain entry %s, %s" % (when, mode))
        d_state = _state_dev(N.new_state())
        _check(*_encode(ctx, frames, w, h, nr, 0, d_state, qbias, entry="nr"), want_nr, "the -nr entry %s, %s" % (when, mode))
        assert (d_state.cpu().numpy() == nr_state).all()
        _check(*_encode(ctx, frames, w, h, 0, lam, None, qbias, entry="trellis"), want_trellis, "the trellis entry %s, %s" % (when, mode))

    def run(mode):
        old(mode, "before")
        _check(*_encode(ctx, frames, w, h, nr, lam, _state_dev(N.new_state()), qbias), want_both, "the combined entry, %s" % mode)
        old(mode, "after")

    both_modes(run)
