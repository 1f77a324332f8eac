"""The encoder's own error in the coding call (amvhip_encode_quant_psnr_stream_dev, its YUV420 and front-end forms) on a real
MI355X.  For each of the four requests -- plain, -nr, trellis at amvhip_encode_trellis_lambda(8), both -- in both entropy
modes and from RGB, BGR and YUV420 sources: chunks, d_offs, d_lens and the -nr state equal the existing entry's, and d_sse
equals tests/psnr_ref.py applied to the chunks the call returned, so the expectation never passes through the code under
test.  Every comparison is on integers and exact.

Sizes: 2x2 and 16x16 (one MCU), 18x34 (edge MCUs cut both ways, chroma 9x17), 160x120 (height % 16 == 8), 336x32 (more
than one segment per MCU row); 1, 3 and -- at 16x16 -- 1030 frames, which is two rounds of the coefficient workspace."""
import numpy as np
import pytest

import frontend_ref as F
import img_convert_ref as R
import nr_ref as N
import pixel_builder as pb
import psnr_ref as P
from test_gpu_frontend import Pictures, stream
from test_gpu_parity import _t

pytestmark = pytest.mark.gpu

FILL = 0xA5
NR, LAM, QBIAS = 1200, 3481, 0
REQUESTS = {"plain": (0, 0, 0), "nr": (NR, 0, 0), "trellis": (0, 1, LAM), "both": (NR, 1, LAM)}
SIZES = [(2, 2), (16, 16), (18, 34), (160, 120), (336, 32)]
KINDS = ["ramp", "checker", "noise", "flat", "texture"]
_REF = {}


# ---- pictures -------------------------------------------------------------------------------------------------------------------

def checker(w, h):
    yy, xx = np.mgrid[:h, :w]
    return (((yy + xx) & 1) * 255).astype(np.uint8)


def yuv_picture(w, h, kind, seed):
    if kind == "checker":
        return checker(w, h), checker(w // 2, h // 2), checker(w // 2, h // 2)[::-1].copy()
    return N.picture(w, h, kind, seed)


def rgb_picture(orc, w, h, kind, seed):
    """[h, w, 3] uint8"""
    if kind == "checker":
        return np.repeat(checker(w, h)[:, :, None], 3, axis=2)
    if kind == "flat":
        return np.full((h, w, 3), 128, np.uint8)
    if kind == "noise":
        return np.random.default_rng(seed).integers(0, 256, (h, w, 3)).astype(np.uint8)
    return orc.synth_frame(pb.SEED, seed, w, h)


class Source:
    """n frames of one kind ("yuv", "rgb", "bgr"): on the device with rows wider than the picture, and as the planes the
    encoder is handed (for RGB / BGR the oracle's rgb24_to_yuvj420p)"""

    def __init__(self, orc, kind, w, h, kinds, seed, planes=None, pix=None):
        self.kind, self.w, self.h, self.n = kind, w, h, len(kinds)
        if kind == "yuv":
            self.planes = planes or [yuv_picture(w, h, k, seed + i) for i, k in enumerate(kinds)]
            n, ys, cs = self.n, w + 8, w // 2 + 8
            Y, Cb, Cr = np.full((n, h, ys), 0xEE, np.uint8), np.full((n, h // 2, cs), 0xEE, np.uint8), np.full((n, h // 2, cs), 0xEE, np.uint8)
            for i, (y, cb, cr) in enumerate(self.planes):
                Y[i, :, :w], Cb[i, :, : w // 2], Cr[i, :, : w // 2] = y, cb, cr
            self.dev = (_t(Y), _t(Cb), _t(Cr))
            self.layout = (ys, cs, h * ys, (h // 2) * cs)
        else:
            pix = pix or [rgb_picture(orc, w, h, k, seed + i) for i, k in enumerate(kinds)]
            self.planes = [pb.to_planes(orc, p, w, h, kind == "bgr") for p in pix]
            self.stride = w * 3 + 5
            padded = np.full((self.n, h, self.stride), 0xEE, np.uint8)
            for i, p in enumerate(pix):
                padded[i, :, : w * 3] = p.reshape(h, w * 3)
            self.dev = (_t(padded),)

    def part(self, lo, hi):
        """frames lo .. hi of the same device buffers"""
        s = Source.__new__(Source)
        s.kind, s.w, s.h, s.n, s.planes = self.kind, self.w, self.h, hi - lo, self.planes[lo:hi]
        s.dev = tuple(d[lo:hi] for d in self.dev)
        if self.kind == "yuv":
            s.layout = self.layout
        else:
            s.stride = self.stride
        return s

    def head(self):
        """the arguments in front of the quantiser's"""
        if self.kind == "yuv":
            return (*self.dev, *self.layout, self.n, self.w, self.h)
        return (self.dev[0], self.stride, 1 if self.kind == "bgr" else 0, self.n, self.w, self.h)


# ---- calls ----------------------------------------------------------------------------------------------------------------------

def _state(values=None):
    import torch
    return torch.zeros(65, dtype=torch.int32, device="cuda:0") if values is None else _t(np.asarray(values, np.int32))


def _outputs(ctx, n, w, h, cap=None):
    import torch
    cap = ctx.encode_bound(w, h) * n if cap is None else cap
    return (torch.full((cap + 64,), FILL, dtype=torch.uint8, device="cuda:0"), cap, torch.full((n,), -1, dtype=torch.int64, device="cuda:0"),
            torch.full((n,), -1, dtype=torch.int32, device="cuda:0"))


def _fetch(out):
    import torch
    torch.cuda.synchronize()
    return out[0].cpu().numpy(), out[2].cpu().numpy(), out[3].cpu().numpy()


def old_entry(ctx, src, request, state, cap=None, qbias=QBIAS):
    """the entry of the request without _psnr -> (blob, offs, lens)"""
    nr, trellis, lam = REQUESTS[request]
    out = _outputs(ctx, src.n, src.w, src.h, cap)
    yuv = src.kind == "yuv"
    if request == "plain":
        (ctx.encode_yuv420_batch_dev if yuv else ctx.encode_batch_dev)(*src.head(), qbias, *out, stream())
    elif request == "nr":
        (ctx.encode_yuv420_nr_stream_dev if yuv else ctx.encode_nr_stream_dev)(*src.head(), qbias, nr, state, *out, stream())
    elif request == "trellis":
        (ctx.encode_yuv420_trellis_batch_dev if yuv else ctx.encode_trellis_batch_dev)(*src.head(), qbias, lam, *out, stream())
    else:
        (ctx.encode_yuv420_nr_trellis_stream_dev if yuv else ctx.encode_nr_trellis_stream_dev)(*src.head(), qbias, nr, lam, state, *out, stream())
    return _fetch(out)


def psnr_entry(ctx, pkg, src, request, state, cap=None, qbias=QBIAS):
    """-> ((blob, offs, lens), sse [n, 3] uint64)"""
    import torch
    nr, trellis, lam = REQUESTS[request]
    q = pkg.Quant(qbias, nr, trellis, lam, state if nr else None)
    out = _outputs(ctx, src.n, src.w, src.h, cap)
    d_sse = torch.full((src.n, 3), -1, dtype=torch.int64, device="cuda:0")
    (ctx.encode_yuv420_quant_psnr_stream_dev if src.kind == "yuv" else ctx.encode_quant_psnr_stream_dev)(*src.head(), q, *out, d_sse, stream())
    return _fetch(out), d_sse.cpu().numpy().view(np.uint64)


def chunks_of(blob, offs, lens):
    return [blob[int(o): int(o) + int(l)].tobytes() for o, l in zip(offs, lens)]


def ref_sse(orc, chunks, src):
    """psnr_ref on the chunks a call returned and the planes it was handed (made once per chunk and picture)"""
    rows = []
    for c, planes in zip(chunks, src.planes):
        key = (c, src.w, src.h, planes[0].tobytes(), planes[1].tobytes(), planes[2].tobytes())
        if key not in _REF:
            _REF[key] = P.sse(orc, c, planes, src.w, src.h)
        rows.append(_REF[key])
    return np.array(rows, np.uint64).reshape(len(chunks), 3)


def both_modes(ctx, pkg, fn):
    try:
        for mode in (pkg.ENTROPY_AUTO, pkg.ENTROPY_SERIAL):
            ctx.set_entropy_mode(mode)
            fn("serial" if mode == pkg.ENTROPY_SERIAL else "auto")
    finally:
        ctx.set_entropy_mode(pkg.ENTROPY_AUTO)


def check_against_old_and_ref(ctx, pkg, orc, src, request, what):
    """the _psnr entry in both modes: bytes, offsets, lengths, fill and state are the old entry's; d_sse is the ref's"""
    old_state = _state()
    want = old_entry(ctx, src, request, old_state)
    chunks = chunks_of(*want)
    assert all(len(c) > 4 for c in chunks), what
    want_sse = ref_sse(orc, chunks, src)

    def run(mode):
        state = _state()
        got, sse = psnr_entry(ctx, pkg, src, request, state)
        for a, b, name in zip(want, got, ("bytes", "offsets", "lengths")):
            assert (a == b).all(), "%s, %s: %s differ at %s" % (what, mode, name, np.flatnonzero(a != b)[:8])
        assert (state.cpu().numpy() == old_state.cpu().numpy()).all(), "%s, %s: the state" % (what, mode)
        assert (sse == want_sse).all(), "%s, %s: d_sse rows %s: %s, want %s" % (
            what, mode, np.flatnonzero((sse != want_sse).any(axis=1))[:4], sse[(sse != want_sse).any(axis=1)][:4].tolist(),
            want_sse[(sse != want_sse).any(axis=1)][:4].tolist())

    both_modes(ctx, pkg, run)
    return chunks, want_sse


# ---- the four requests, three sources, five sizes -------------------------------------------------------------------------------

@pytest.mark.parametrize("request_name", list(REQUESTS))
@pytest.mark.parametrize("kind", ["rgb", "bgr", "yuv"])
def test_requests_sources_and_sizes(ctx, pkg, orc, kind, request_name):
    assert ctx.encode_trellis_lambda(8) == LAM
    for w, h in SIZES:
        for n in (1, 3):
            kinds = [KINDS[(i + w) % len(KINDS)] for i in range(n)] if n == 1 else ["checker", "noise", "ramp"]
            src = Source(orc, kind, w, h, kinds, 50 + w)
            what = "%s %s %dx%d x %d" % (kind, request_name, w, h, n)
            chunks, sse = check_against_old_and_ref(ctx, pkg, orc, src, request_name, what)
            # a coded picture that is not flat has an error on the luma plane, and no sum is more than its plane holds
            assert (sse[:, 0] > 0).all() or kinds == ["flat"], what
            assert (sse[:, 0] <= 65025 * w * h).all() and (sse[:, 1:] <= 65025 * (w // 2) * (h // 2)).all(), what


@pytest.mark.parametrize("request_name", ["plain", "both"])
@pytest.mark.parametrize("kind", ["yuv", "rgb"])
def test_two_rounds_of_the_workspace(ctx, pkg, orc, kind, request_name):
    """1030 frames at 16x16: fallback_round(1030, g, 1024, 2) is 1024, so the frames' levels are made in rounds of 1024 and 6
    -- the second round begins 1024 frames into the source, planes or padded pixel rows, and with -nr reads the offsets of
    frames 1024 .. 1029"""
    w, h, n = 16, 16, 1030
    rng = np.random.default_rng(77)
    shapes = ((h, w), (h // 2, w // 2), (h // 2, w // 2)) if kind == "yuv" else ((h, w, 3),)
    frames = []
    for i in range(n):
        amp = 1 + i % 120
        frames.append(tuple(np.clip(128 + rng.integers(-amp, amp + 1, s), 0, 255).astype(np.uint8) for s in shapes))
    if kind == "yuv":
        src = Source(orc, "yuv", w, h, [None] * n, 0, planes=frames)
    else:
        src = Source(orc, "rgb", w, h, [None] * n, 0, pix=[f[0] for f in frames])
    chunks, sse = check_against_old_and_ref(ctx, pkg, orc, src, request_name, "1030 %s frames, %s" % (kind, request_name))
    assert len({tuple(r) for r in sse[1024:].tolist()}) > 1 and (sse[1024:, 0] > 0).all()


def test_pixel_builder_pictures(ctx, pkg, orc):
    """the crafted pictures of tests/pixel_builder.py (every symbol, run, window edge, FF pattern, quantiser threshold and the
    RGB edge geometries), the first nine frames of each of its batches, with the qbias each was built for where the batch
    has one value, in both entropy modes"""
    cases, _ = pb.corpus(orc)
    for b in pb.batches(orc, cases):
        n = min(b["n"], 9)
        frames = b["frames"][:n]
        qb = {f.qbias for f in frames if f.group}
        qbias = qb.pop() if len(qb) == 1 else 0
        src = Source.__new__(Source)
        src.kind, src.w, src.h, src.n, src.planes = b["kind"], b["w"], b["h"], n, [f.planes for f in frames]
        if b["kind"] == "yuv":
            src.dev = tuple(_t(np.ascontiguousarray(p[:n])) for p in b["planes"])
            src.layout = (b["ys"], b["cs"], b["h"] * b["ys"], (b["h"] // 2) * b["cs"])
        else:
            src.dev, src.stride = (_t(np.ascontiguousarray(b["pix"][:n])),), b["stride"]
        want_chunks = [f.chunk(orc, qbias) for f in frames]
        want = ref_sse(orc, want_chunks, src)

        def run(mode):
            what = "%dx%d %s, %s" % (b["w"], b["h"], b["kind"], mode)
            (got, sse) = psnr_entry(ctx, pkg, src, "plain", None, qbias=qbias)
            assert chunks_of(*got) == want_chunks, what
            assert (sse == want).all(), "%s: rows %s" % (what, np.flatnonzero((sse != want).any(axis=1))[:6])

        both_modes(ctx, pkg, run)


# ---- content --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["rgb", "yuv"])
def test_flat_128_is_exactly_zero(ctx, pkg, orc, kind):
    for w, h in SIZES:
        src = Source(orc, kind, w, h, ["flat", "flat"], 0)
        for request in REQUESTS:
            got, sse = psnr_entry(ctx, pkg, src, request, _state())
            assert (sse == 0).all(), "%s %dx%d %s: %s" % (kind, w, h, request, sse.tolist())
            assert (ref_sse(orc, chunks_of(*got), src) == 0).all()


def test_checkerboard_clips_at_both_ends(ctx, pkg, orc):
    """a 0/255 checkerboard at one-pixel pitch: the ref's IDCT output before the clip leaves 0..255 on both sides, so the
    error depends on the clip being there"""
    for w, h in ((16, 16), (18, 34)):
        src = Source(orc, "yuv", w, h, ["checker"], 0)
        got, sse = psnr_entry(ctx, pkg, src, "plain", None)
        chunk = chunks_of(*got)[0]
        lo, hi = P.canvases(orc, chunk, w, h, unclipped=True)
        assert lo < 0 and hi > 255, (lo, hi)
        assert (sse == ref_sse(orc, [chunk], src)).all() and (sse > 0).all()


# ---- streams, a short blob, the front end ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("request_name", ["nr", "both"])
def test_a_stream_in_three_calls(ctx, pkg, orc, request_name):
    w, h = 48, 32
    src = Source(orc, "yuv", w, h, ["ramp", "texture", "flat", "texture", "ramp", "texture", "noise", "ramp"], 77)
    whole_state = _state()
    whole, whole_sse = psnr_entry(ctx, pkg, src, request_name, whole_state)
    state, parts, rows = _state(), [], []
    for lo, hi in ((0, 3), (3, 4), (4, 8)):
        got, sse = psnr_entry(ctx, pkg, src.part(lo, hi), request_name, state)
        parts += chunks_of(*got)
        rows.append(sse)
    assert parts == chunks_of(*whole)
    assert (np.concatenate(rows) == whole_sse).all() and (state.cpu().numpy() == whole_state.cpu().numpy()).all()
    assert state.cpu().numpy()[64] == 8 * 36
    assert (whole_sse == ref_sse(orc, parts, src)).all()
    # the dead zone did something to the error: the plain request's differs on the later frames
    _, plain_sse = psnr_entry(ctx, pkg, src, "plain" if request_name == "nr" else "trellis", None)
    assert (plain_sse[0] == whole_sse[0]).all() and (plain_sse[1:] != whole_sse[1:]).any()


def test_a_blob_too_small(ctx, pkg, orc):
    """the chunks that do not fit have length 0, and their frames carry their error all the same"""
    w, h = 48, 32
    src = Source(orc, "rgb", w, h, ["ramp", "noise", "texture", "ramp"], 9)

    def run(mode):
        full, full_sse = psnr_entry(ctx, pkg, src, "both", _state())
        chunks = chunks_of(*full)
        total = sum(len(c) for c in chunks)
        state = _state()
        (blob, offs, lens), sse = psnr_entry(ctx, pkg, src, "both", state, cap=total - len(chunks[-1]) - 1)
        assert [int(x) for x in lens[-2:]] == [0, 0] and chunks_of(blob, offs[:-2], lens[:-2]) == chunks[:-2], mode
        assert (blob[int(offs[-2]):] == FILL).all(), mode
        assert (sse == full_sse).all() and (sse[-2:, 0] > 0).all(), mode
        assert state.cpu().numpy()[64] == 4 * 36, mode
        assert (full_sse == ref_sse(orc, chunks, src)).all(), mode

    both_modes(ctx, pkg, run)


@pytest.mark.parametrize("request_name", list(REQUESTS))
def test_the_front_end_entry(ctx, pkg, orc, request_name):
    """deinterlace + rescale + pad, 64x48 -> 28x24 inside 32x32: the entry equals amvhip_video_frontend_dev into tight planes
    followed by the YUV420 entry, d_sse included, and d_sse is the ref's on the workspace pictures"""
    import torch
    W, H, n, sw, sh = 32, 32, 4, 64, 48
    fe_args = (1, (0, 0, 0, 0), (4, 4, 2, 2), (16, 128, 128))
    fe = pkg.Frontend(*fe_args)
    frames = [R.make_picture(R.YUV420P, sw, sh, k, 31 + 7 * i) for i, k in enumerate(("ramp", "noise", "ramp", "noise"))]
    s = Pictures(R.YUV420P, sw, sh, n).fill(frames).to_dev()
    d = Pictures(R.YUVJ420P, W, H, n).to_dev()
    ctx.video_frontend_dev(R.YUV420P, s.pic(), sw, sh, n, fe, d.pic(), W, H, stream())
    torch.cuda.synchronize()
    d.from_dev()
    planes = [tuple(d.planes(i)) for i in range(n)]
    assert all((a == b).all() for got, f in zip(planes, frames)
               for a, b in zip(got, F.frontend(R.YUV420P, f, sw, sh, W, H, orc.img_resample_yuv420, *fe_args)))
    two = Source.__new__(Source)
    two.kind, two.w, two.h, two.n, two.planes = "yuv", W, H, n, planes
    two.dev, two.layout = tuple(d.dev), (d.stride[0], d.stride[1], d.frame[0], d.frame[1])
    nr, trellis, lam = REQUESTS[request_name]

    def run(mode):
        want_state = _state()
        want, want_sse = psnr_entry(ctx, pkg, two, request_name, want_state, qbias=5)
        state = _state()
        out = _outputs(ctx, n, W, H)
        d_sse = torch.full((n, 3), -1, dtype=torch.int64, device="cuda:0")
        q = pkg.Quant(5, nr, trellis, lam, state if nr else None)
        ctx.encode_frontend_quant_psnr_stream_dev(R.YUV420P, s.pic(), sw, sh, n, fe, W, H, q, *out, d_sse, stream())
        got = _fetch(out)
        assert all((a == b).all() for a, b in zip(want, got)), mode
        assert (d_sse.cpu().numpy().view(np.uint64) == want_sse).all() and (state.cpu().numpy() == want_state.cpu().numpy()).all(), mode
        assert (want_sse == ref_sse(orc, chunks_of(*got), two)).all() and (want_sse[:, 0] > 0).all(), mode
        # ... and the chunks are the entry's without _psnr
        plain = _outputs(ctx, n, W, H)
        ctx.encode_frontend_quant_stream_dev(R.YUV420P, s.pic(), sw, sh, n, fe, W, H, pkg.Quant(5, nr, trellis, lam, _state() if nr else None),
                                             *plain, stream())
        assert all((a == b).all() for a, b in zip(_fetch(plain), got)), mode

    both_modes(ctx, pkg, run)


# ---- refusals -------------------------------------------------------------------------------------------------------------------

def test_refusals(ctx, pkg, orc):
    """q == NULL, a trellis other than 0 / 1, what the entries behind refuse of nr, lambda, the state and qbias, a null or
    misaligned d_sse, odd sizes, null outputs: AMVHIP_ERR_ARG before anything is written"""
    import torch
    w, h, n = 48, 32, 2
    state = torch.arange(65, dtype=torch.int32, device="cuda:0")
    out = _outputs(ctx, n, w, h)
    d_sse = torch.full((n, 3), -1, dtype=torch.int64, device="cuda:0")
    ok_q = pkg.Quant(0, NR, 1, LAM, state)
    bad_q = [None, pkg.Quant(0, NR, 0, 0, None), pkg.Quant(0, NR, 1, LAM, None), pkg.Quant(0, ctx.encode_nr_max(w, h) + 1, 1, LAM, state),
             pkg.Quant(0, NR, 1, ctx.encode_trellis_lambda_max() + 1, state), pkg.Quant(0, NR, 2, LAM, state), pkg.Quant(256, NR, 1, LAM, state),
             pkg.Quant(0, NR, 1, LAM, state.data_ptr() + 2)]
    s = Pictures(R.YUV420P, 64, 48, n).to_dev()
    for kind in ("yuv", "rgb"):
        src = Source(orc, kind, w, h, ["ramp", "noise"], 3)
        entry = ctx.encode_yuv420_quant_psnr_stream_dev if kind == "yuv" else ctx.encode_quant_psnr_stream_dev
        calls = [(src.head(), q, out, d_sse) for q in bad_q]
        calls += [(src.head(), ok_q, out, None), (src.head(), ok_q, out, d_sse.data_ptr() + 4)]
        calls += [(src.head()[:-2] + (w - 1, h), ok_q, out, d_sse), (src.head()[:-2] + (w, h - 1), ok_q, out, d_sse)]
        calls += [(src.head(), ok_q, (None,) + out[1:], d_sse), (src.head(), ok_q, out[:2] + (None, out[3]), d_sse), (src.head(), ok_q, out[:3] + (None,), d_sse)]
        for head, q, o, sse in calls:
            with pytest.raises(pkg.AmvHipError, match=r"\(-1\)"):
                entry(*head, q, *o, sse, stream())
    for q, sse in [(x, d_sse) for x in bad_q] + [(ok_q, None), (ok_q, d_sse.data_ptr() + 4)]:
        with pytest.raises(pkg.AmvHipError, match=r"\(-1\)"):
            ctx.encode_frontend_quant_psnr_stream_dev(R.YUV420P, s.pic(), 64, 48, n, pkg.Frontend(1), w, h, q, *out, sse, stream())
    torch.cuda.synchronize()
    assert (out[0].cpu().numpy() == FILL).all() and (out[2].cpu().numpy() == -1).all() and (out[3].cpu().numpy() == -1).all()
    assert (d_sse.cpu().numpy() == -1).all() and (state.cpu().numpy() == np.arange(65)).all()
    # no frames: fine, and nothing is written
    src = Source(orc, "yuv", w, h, ["ramp", "noise"], 3)
    ctx.encode_yuv420_quant_psnr_stream_dev(*src.head()[:-3], 0, w, h, ok_q, *out, d_sse, stream())
    torch.cuda.synchronize()
    assert (d_sse.cpu().numpy() == -1).all() and (state.cpu().numpy() == np.arange(65)).all()
