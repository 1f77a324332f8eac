"""The -nr entries (amvhip_encode_yuv420_nr_stream_dev and its RGB and host-buffer forms) on a real MI355X against the
product-mode model of tests/nr_ref.py: every chunk's bytes, d_offs, d_lens and the state that comes out.

Shapes are the smallest that reach each path: 48x32 (one segment a row), 176x120 (eleven MCUs a row: two segments, and
half an MCU row of padding blocks), 160x120 with a frame of full-range noise (the hand-back route through
amv_forward_kernel + amv_pack_kernel), 16x16 with a count next to 65536 (the halving inside the call)."""
import numpy as np
import pytest

import nr_ref as M
from test_gpu_parity import _t

pytestmark = pytest.mark.gpu

FILL = 0xA5
WINDOW_BITS = 1280 * 32        # amv_encode_par.hip's bit-string window: a round (four segments) beyond it is handed back


def _pack(frames, w, h, pad=0):
    """planes of n frames as the entry takes them, rows padded by `pad` poison bytes"""
    n, cw, ch = len(frames), w // 2, h // 2
    ys, cs = w + pad, cw + pad
    Y, Cb, Cr = np.full((n, h, ys), 0xEE, np.uint8), np.full((n, ch, cs), 0xEE, np.uint8), np.full((n, ch, cs), 0xEE, np.uint8)
    for i, (y, cb, cr) in enumerate(frames):
        Y[i, :, :w], Cb[i, :, :cw], Cr[i, :, :cw] = y, cb, cr
    return Y, Cb, Cr, ys, cs


def _state_dev(state):
    return _t(np.asarray(state, np.int64).astype(np.int32))


def _encode(ctx, frames, w, h, nr, d_state, qbias=0, cap=None, pad=8):
    """one call -> (blob, offs, lens) as numpy; d_state (device int32[65]) is read and written"""
    import torch
    n = len(frames)
    Y, Cb, Cr, ys, cs = _pack(frames, w, h, pad)
    cap = ctx.encode_bound(w, h) * n if cap is None else cap
    d_blob = torch.full((cap + 64,), FILL, dtype=torch.uint8, device="cuda:0")
    d_offs = torch.full((n,), -1, dtype=torch.int64, device="cuda:0")
    d_lens = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    ctx.encode_yuv420_nr_stream_dev(_t(Y), _t(Cb), _t(Cr), ys, cs, h * ys, (h // 2) * cs, n, w, h, qbias, nr, d_state, d_blob, cap,
                                    d_offs, d_lens)
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


def _run_case(ctx, w, h, kinds, seed, nr, state=None, qbias=0):
    frames = M.stream(w, h, kinds, seed)
    model_state = M.new_state() if state is None else np.array(state, np.int64)
    d_state = _state_dev(model_state)
    want = M.encode_stream(frames, w, h, nr, state=model_state, qbias=qbias)
    blob, offs, lens = _encode(ctx, frames, w, h, nr, d_state, qbias)
    what = "%dx%d x %d, nr %d" % (w, h, len(frames), nr)
    _check(blob, offs, lens, want, what)
    got_state = d_state.cpu().numpy()
    assert (got_state == model_state).all(), "%s: state differs at %s" % (what, np.flatnonzero(got_state != model_state)[:8])
    return frames, want


@pytest.mark.parametrize("nr", [300, 3000])
def test_ramp_stream(ctx, nr):
    frames, want = _run_case(ctx, 48, 32, ["ramp"] * 6, 100, nr)
    assert want != M.encode_stream(frames, 48, 32, 0)                # the dead zone did something


def test_truncation_case(ctx):
    """two flat frames, then texture at nr 911: 911 * 72 / 1 = 65592 is stored as 56"""
    w, h, kinds = 48, 32, ["flat", "flat"] + ["texture"] * 4
    frames, want = _run_case(ctx, w, h, kinds, 300, 911)
    state = M.new_state()
    untruncated = M.encode_stream(frames, w, h, 911, state=state, truncate=False)
    assert untruncated != want


def test_two_segments_and_padding_blocks(ctx):
    """176x120: eleven MCUs a row (segments of 6 + 5), the last MCU row half outside the picture; qbias on the way"""
    _run_case(ctx, 176, 120, ["texture", "ramp", "texture"], 500, 1200, qbias=40)
    _run_case(ctx, 22, 38, ["texture", "ramp"], 520, 600)              # padding blocks both ways


def test_hand_back_route_applies_the_offsets(ctx):
    """160x120 with one frame of full-range noise: its rounds do not fit the one-kernel coder's window, so it is coded by
    amv_forward_kernel + amv_pack_kernel -- with the same offsets"""
    w, h, kinds = 160, 120, ["ramp", "flat", "noise", "ramp"]
    frames, want = _run_case(ctx, w, h, kinds, 900, 300)
    noisy = want[2]
    scan_bits = 8 * (len(noisy) - 4 - noisy.count(b"\xff\x00"))
    rounds = (8 * 1 + 3) // 4                                          # 8 MCU rows of one segment, four segments a round
    assert scan_bits > rounds * (WINDOW_BITS + 8), "the noise frame would fit the window: it did not take the hand-back route"
    assert all(8 * len(c) < WINDOW_BITS for i, c in enumerate(want) if i != 2)      # ... and the others did not
    assert noisy != M.encode_stream(frames[2:3], w, h, 0)[0]


def test_halving_inside_the_call(ctx):
    """16x16 x 4 from a count of 65530: 65536 after frame 0 (stays), 65542 after frame 1: frame 2 starts by halving"""
    rng = np.random.default_rng(3)
    state = np.concatenate([rng.integers(0, 16320 * 65530, 64), [65530]])
    state[:3] = (0, 7, 16320 * 65530)
    before = state.copy()
    _run_case(ctx, 16, 16, ["texture", "ramp", "texture", "ramp"], 40, 4000, state=state)
    check = np.array(before, np.int64)
    M.encode_stream(M.stream(16, 16, ["texture", "ramp", "texture", "ramp"], 40), 16, 16, 4000, state=check)
    assert check[64] == ((65530 + 12) >> 1) + 12


def test_one_call_equals_calls_with_the_state_carried(ctx):
    w, h, nr = 48, 32, 1500
    frames = M.stream(w, h, ["ramp", "texture", "flat", "texture", "ramp", "texture", "texture", "ramp"], 77)
    whole_state = _state_dev(M.new_state())
    whole = _chunks(*_encode(ctx, frames, w, h, nr, whole_state))
    d_state, parts = _state_dev(M.new_state()), []
    for lo, hi in ((0, 3), (3, 4), (4, 8)):
        parts += _chunks(*_encode(ctx, frames[lo:hi], w, h, nr, d_state))
    assert parts == whole
    assert (d_state.cpu().numpy() == whole_state.cpu().numpy()).all()
    model_state = M.new_state()
    assert whole == M.encode_stream(frames, w, h, nr, state=model_state)
    assert (whole_state.cpu().numpy() == model_state).all()


def test_nr_0_is_the_plain_entry(ctx):
    import torch
    w, h = 48, 32
    frames = M.stream(w, h, ["ramp", "texture", "noise"], 60)
    state = np.arange(65) * 1000 + 7
    d_state = _state_dev(state)
    blob, offs, lens = _encode(ctx, frames, w, h, 0, d_state, qbias=5, pad=0)
    assert (d_state.cpu().numpy() == state).all()
    n = len(frames)
    Y, Cb, Cr, ys, cs = _pack(frames, w, h)
    cap = ctx.encode_bound(w, h) * n
    d_blob = torch.full((cap + 64,), FILL, dtype=torch.uint8, device="cuda:0")
    d_offs = torch.zeros(n, dtype=torch.int64, device="cuda:0")
    d_lens = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    ctx.encode_yuv420_batch_dev(_t(Y), _t(Cb), _t(Cr), ys, cs, h * ys, (h // 2) * cs, n, w, h, 5, d_blob, cap, d_offs, d_lens)
    torch.cuda.synchronize()
    assert (d_offs.cpu().numpy() == offs).all() and (d_lens.cpu().numpy() == lens).all() and (d_blob.cpu().numpy() == blob).all()
    # nr 0 takes no state at all
    ctx.encode_yuv420_nr_stream_dev(_t(Y), _t(Cb), _t(Cr), ys, cs, h * ys, (h // 2) * cs, n, w, h, 5, 0, None, d_blob, cap, d_offs, d_lens)
    torch.cuda.synchronize()
    assert (d_blob.cpu().numpy() == blob).all()


def test_rgb_entry_and_host_forms(ctx, orc):
    """RGB24 / BGR24 in equal rgb24_to_yuvj420p + the YUV entry; the host-buffer forms equal the device forms"""
    import torch
    w, h, n, nr = 48, 32, 3, 800
    L = orc.lib()
    for bgr in (0, 1):
        pix = np.stack([orc.synth_frame(0xA11CE, 10 + t, w, h) for t in range(n)])
        frames = []
        for t in range(n):
            y, cb, cr = np.zeros((h, w), np.uint8), np.zeros((h // 2, w // 2), np.uint8), np.zeros((h // 2, w // 2), np.uint8)
            L.amvo_rgb24_to_yuvj420p(pix[t].ctypes.data, w * 3, w, h, bgr, y.ctypes.data, cb.ctypes.data, cr.ctypes.data)
            frames.append((y, cb, cr))
        model_state = M.new_state()
        want = M.encode_stream(frames, w, h, nr, state=model_state)
        d_state = _state_dev(M.new_state())
        blob, offs, lens = _encode(ctx, frames, w, h, nr, d_state)
        _check(blob, offs, lens, want, "planes")
        cap = ctx.encode_bound(w, h) * n
        d_blob = torch.full((cap + 64,), FILL, dtype=torch.uint8, device="cuda:0")
        d_offs = torch.zeros(n, dtype=torch.int64, device="cuda:0")
        d_lens = torch.zeros(n, dtype=torch.int32, device="cuda:0")
        d_state2 = _state_dev(M.new_state())
        ctx.encode_nr_stream_dev(_t(pix), w * 3, bgr, n, w, h, 0, nr, d_state2, d_blob, cap, d_offs, d_lens)
        torch.cuda.synchronize()
        _check(d_blob.cpu().numpy(), d_offs.cpu().numpy(), d_lens.cpu().numpy(), want, "pixels, bgr %d" % bgr)
        assert (d_state2.cpu().numpy() == model_state).all() and (d_state.cpu().numpy() == model_state).all()
        # host-buffer forms, the stream in two calls
        for form in ("pixels", "planes"):
            state = np.zeros(65, np.int32)
            got = []
            for lo, hi in ((0, 1), (1, n)):
                m = hi - lo
                hb, ho, hl = np.full(cap, FILL, np.uint8), np.zeros(m, np.uint64), np.zeros(m, np.uint32)
                if form == "pixels":
                    ctx.encode_nr_stream(np.ascontiguousarray(pix[lo:hi]), w * 3, bgr, m, w, h, 0, nr, state, hb, cap, ho, hl)
                else:
                    Y, Cb, Cr, ys, cs = _pack(frames[lo:hi], w, h, 4)
                    ctx.encode_yuv420_nr_stream(Y, Cb, Cr, ys, cs, h * ys, (h // 2) * cs, m, w, h, 0, nr, state, hb, cap, ho, hl)
                got += _chunks(hb, ho, hl)
            assert got == want and (state == model_state).all(), form


@pytest.mark.parametrize("bgr", [0, 1])
def test_rgb_entry_on_the_two_stage_route(ctx, pkg, orc, bgr):
    """amvhip_encode_nr_stream_dev in AMVHIP_ENTROPY_SERIAL mode: amv_forward_kernel's RGB instantiation with the offsets.
    176x24: eleven MCUs a row (segments of 6 + 5), the last MCU row half outside the picture."""
    import torch
    w, h, n, nr = 176, 24, 3, 3000
    L = orc.lib()
    pix = np.stack([orc.synth_frame(0xA11CE, 30 + t, w, h) for t in range(n)])
    frames = []
    for t in range(n):
        y, cb, cr = np.zeros((h, w), np.uint8), np.zeros((h // 2, w // 2), np.uint8), np.zeros((h // 2, w // 2), np.uint8)
        L.amvo_rgb24_to_yuvj420p(pix[t].ctypes.data, w * 3, w, h, bgr, y.ctypes.data, cb.ctypes.data, cr.ctypes.data)
        frames.append((y, cb, cr))
    model_state = M.new_state()
    want = M.encode_stream(frames, w, h, nr, state=model_state)
    cap = ctx.encode_bound(w, h) * n
    got = {}
    try:
        for mode in (pkg.ENTROPY_AUTO, pkg.ENTROPY_SERIAL):
            ctx.set_entropy_mode(mode)
            d_blob = torch.full((cap + 64,), FILL, dtype=torch.uint8, device="cuda:0")
            d_offs = torch.full((n,), -1, dtype=torch.int64, device="cuda:0")
            d_lens = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
            d_state = _state_dev(M.new_state())
            ctx.encode_nr_stream_dev(_t(pix), w * 3, bgr, n, w, h, 0, nr, d_state, d_blob, cap, d_offs, d_lens)
            torch.cuda.synchronize()
            got[mode] = (d_blob.cpu().numpy(), d_offs.cpu().numpy(), d_lens.cpu().numpy(), d_state.cpu().numpy())
    finally:
        ctx.set_entropy_mode(pkg.ENTROPY_AUTO)
    auto, serial = got[pkg.ENTROPY_AUTO], got[pkg.ENTROPY_SERIAL]
    for a, s, what in zip(auto, serial, ("bytes", "offsets", "lengths", "state")):
        assert (a == s).all(), "%s differ between the two routes at %s" % (what, np.flatnonzero(a != s)[:8])
    _check(*serial[:3], want, "pixels, bgr %d, serial" % bgr)
    assert (serial[3] == model_state).all()


def test_short_blob_and_refused_arguments(ctx, pkg):
    import torch
    w, h, nr = 48, 32, 300
    frames = M.stream(w, h, ["ramp"] * 4, 100)
    model_state = M.new_state()
    want = M.encode_stream(frames, w, h, nr, state=model_state)
    total = sum(len(c) for c in want)
    d_state = _state_dev(M.new_state())
    blob, offs, lens = _encode(ctx, frames, w, h, nr, d_state, cap=total - 1)
    assert int(lens[-1]) == 0 and int(offs[-1]) == total - len(want[-1])
    assert _chunks(blob, offs[:-1], lens[:-1]) == want[:-1]
    assert (blob[int(offs[-1]):] == FILL).all()
    assert (d_state.cpu().numpy() == model_state).all()                # the state has moved on all the same
    # the host form says so with AMVHIP_ERR_SPACE
    Y, Cb, Cr, ys, cs = _pack(frames, w, h)
    hb, ho, hl, state = np.zeros(total - 1, np.uint8), np.zeros(4, np.uint64), np.zeros(4, np.uint32), np.zeros(65, np.int32)
    with pytest.raises(pkg.AmvHipError, match=r"\(-4\)"):
        ctx.encode_yuv420_nr_stream(Y, Cb, Cr, ys, cs, h * ys, (h // 2) * cs, 4, w, h, 0, nr, state, hb, total - 1, ho, hl)
    # nr above the bound, a null or misaligned state
    most = ctx.encode_nr_max(w, h)
    assert most == 24607
    d_state = _state_dev(np.arange(65))
    d_blob = torch.full((4096,), FILL, dtype=torch.uint8, device="cuda:0")
    d_offs = torch.zeros(4, dtype=torch.int64, device="cuda:0")
    d_lens = torch.zeros(4, dtype=torch.int32, device="cuda:0")
    args = (_t(Y), _t(Cb), _t(Cr), ys, cs, h * ys, (h // 2) * cs, 4, w, h, 0)
    for bad_nr, bad_state in ((most + 1, d_state), (0xFFFFFFFF, d_state), (nr, None), (nr, d_state.data_ptr() + 2)):
        with pytest.raises(pkg.AmvHipError, match=r"\(-1\)"):
            ctx.encode_yuv420_nr_stream_dev(*args, bad_nr, bad_state, d_blob, 4096, d_offs, d_lens)
    with pytest.raises(pkg.AmvHipError, match=r"\(-1\)"):
        ctx.encode_nr_stream_dev(_t(np.zeros((4, h, w, 3), np.uint8)), w * 3, 0, 4, w, h, 0, most + 1, d_state, d_blob, 4096, d_offs, d_lens)
    torch.cuda.synchronize()
    assert (d_state.cpu().numpy() == np.arange(65)).all() and (d_blob.cpu().numpy() == FILL).all()
    # ... and the bound itself is taken
    _run_case(ctx, 16, 16, ["texture", "ramp"], 11, most)


def test_every_chunk_decodes(ctx):
    import torch
    for (w, h), kinds, nr in (((48, 32), ["ramp", "texture", "flat", "noise"], 3000), ((176, 120), ["texture", "noise"], 24607)):
        frames = M.stream(w, h, kinds, 4)
        blob, offs, lens = _encode(ctx, frames, w, h, nr, _state_dev(M.new_state()))
        n = len(frames)
        total = int(offs[-1] + lens[-1])
        d_out = torch.zeros((n, h, ctx.stride(w)), dtype=torch.uint8, device="cuda:0")
        d_st = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
        ctx.decode_batch_dev(_t(blob), total, _t(offs.astype(np.uint64)), _t(lens.astype(np.uint32)), n, w, h, 0, d_out, d_st)
        torch.cuda.synchronize()
        assert (d_st.cpu().numpy() == 0).all(), (w, h, d_st.cpu().numpy())
