"""Picture against picture (amvhip_picture_sse_dev, amvhip_picture_sse) on a real MI355X against numpy: every accepted
format, sizes 2x2, 17x9 (odd: the 4:2:0 chroma is 9x5, the 4:2:2 chroma 9x9; a packed row is 51 bytes) and 130x98 (more
than one tile row), 1 and 5 frames, tight rows and rows wider than the picture with the gaps filled differently in the two batches, a sum past 32 bits,
equal pictures, the host form, and every refusal.  All comparisons are on integers and exact."""
import numpy as np
import pytest

import img_convert_ref as R
from test_gpu_frontend import Pictures, stream

pytestmark = pytest.mark.gpu

ACCEPTED = R.PLANAR + (R.GRAY8, R.RGB24, R.BGR24)
REFUSED = tuple(f for f in range(14) if f not in ACCEPTED)
SIZES = [(2, 2), (17, 9), (130, 98)]


def _want(fmt, a, b):
    """[n, 3] by numpy from two lists of frames (lists of planes)"""
    out = np.zeros((len(a), 3), np.uint64)
    for i, (pa, pb_) in enumerate(zip(a, b)):
        if fmt in (R.RGB24, R.BGR24):
            d = pa[0].astype(np.int64).reshape(pa[0].shape[0], -1, 3) - pb_[0].astype(np.int64).reshape(pa[0].shape[0], -1, 3)
            out[i] = (d * d).sum(axis=(0, 1))
        else:
            for p in range(len(pa)):
                d = pa[p].astype(np.int64) - pb_[p].astype(np.int64)
                out[i, p] = (d * d).sum()
    return out


def _batch(fmt, w, h, frames, pad, gap, fill):
    s = Pictures(fmt, w, h, len(frames), pad, gap)
    for buf in s.host:
        buf[:] = fill
    return s.fill(frames).to_dev()


def _sse_dev(ctx, fmt, a, b, w, h, n):
    import torch
    d_sse = torch.full((n, 3), -1, dtype=torch.int64, device="cuda:0")
    ctx.picture_sse_dev(fmt, a.pic(), b.pic(), w, h, n, d_sse, stream())
    torch.cuda.synchronize()
    return d_sse.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("fmt", ACCEPTED, ids=lambda f: R.NAMES[f])
def test_every_format_against_numpy(ctx, fmt):
    for w, h in SIZES:
        for n in (1, 5):
            fa = [R.make_picture(fmt, w, h, "noise", 100 * fmt + 7 * i + w) for i in range(n)]
            fb = [R.make_picture(fmt, w, h, "noise" if i % 2 == 0 else "ramp", 900 + 100 * fmt + i + h) for i in range(n)]
            want = _want(fmt, fa, fb)
            assert (want[:, 0] > 0).all() and ((want[:, 1:] > 0).all() if fmt != R.GRAY8 else (want[:, 1:] == 0).all())
            for pad, gap in ((0, 0), (5, 7)):
                a, b = _batch(fmt, w, h, fa, pad, gap, 0x00), _batch(fmt, w, h, fb, pad, gap, 0xFF)
                got = _sse_dev(ctx, fmt, a, b, w, h, n)
                assert (got == want).all(), "%s %dx%d x %d, pad %d: %s, want %s" % (R.NAMES[fmt], w, h, n, pad, got.tolist(), want.tolist())
                # the host form is the device form
                host = np.full((n, 3), 0xEE, np.uint64)
                ctx.picture_sse(fmt, a.pic("host"), b.pic("host"), w, h, n, host)
                assert (host == want).all(), "%s %dx%d x %d, pad %d, host buffers" % (R.NAMES[fmt], w, h, n, pad)


@pytest.mark.parametrize("h", [4, 8])
def test_sum_past_32_bits(ctx, h):
    """16384x4 GRAY8, all 0 against all 255: 65536 * 65025 = 4 261 478 400, past a signed 32-bit sum and 0.8 % short of an
    unsigned one; 16384x8 is twice that, past both"""
    w = 16384
    a = _batch(R.GRAY8, w, h, [R.make_picture(R.GRAY8, w, h, "zeros")], 0, 0, 0x11)
    b = _batch(R.GRAY8, w, h, [R.make_picture(R.GRAY8, w, h, "ones")], 0, 0, 0x22)
    got = _sse_dev(ctx, R.GRAY8, a, b, w, h, 1)
    assert got.tolist() == [[w * h * 65025, 0, 0]] and w * h * 65025 > (2 ** 31 if h == 4 else 2 ** 32)


@pytest.mark.parametrize("fmt", [R.YUVJ420P, R.YUV444P, R.BGR24], ids=lambda f: R.NAMES[f])
def test_equal_pictures_give_zero(ctx, fmt):
    w, h, n = 130, 98, 3
    frames = [R.make_picture(fmt, w, h, "noise", 40 + i) for i in range(n)]
    a, b = _batch(fmt, w, h, frames, 3, 5, 0x00), _batch(fmt, w, h, frames, 9, 1, 0xFF)     # (other pitches, other gaps)
    assert (_sse_dev(ctx, fmt, a, b, w, h, n) == 0).all()
    # ... and a picture against itself
    assert (_sse_dev(ctx, fmt, a, a, w, h, n) == 0).all()


def test_one_sample_off(ctx):
    """the last sample of the last chroma row of the last frame alone: 3^2 in that frame's entry 2, nothing else"""
    w, h, n = 17, 9, 2
    frames = [R.make_picture(R.YUV420P, w, h, "noise", 5 + i) for i in range(n)]
    other = [[p.copy() for p in f] for f in frames]
    v = int(other[1][2][-1, -1])
    other[1][2][-1, -1] = v + 3 if v <= 252 else v - 3
    a, b = _batch(R.YUV420P, w, h, frames, 2, 0, 0x00), _batch(R.YUV420P, w, h, other, 2, 0, 0x00)
    assert _sse_dev(ctx, R.YUV420P, a, b, w, h, n).tolist() == [[0, 0, 0], [0, 0, 9]]


def test_refusals(ctx, pkg):
    import torch
    w, h, n = 18, 10, 2
    d_sse = torch.full((n, 3), -1, dtype=torch.int64, device="cuda:0")
    for fmt in REFUSED + (-1, 14):
        shape_fmt = fmt if 0 <= fmt < 14 else R.GRAY8
        a = Pictures(shape_fmt, w, h, n).to_dev()
        assert not ctx.picture_sse_supported(fmt, w, h)
        with pytest.raises(pkg.AmvHipError, match=r"\(-1\)"):
            ctx.picture_sse_dev(fmt, a.pic(), a.pic(), w, h, n, d_sse, stream())
        with pytest.raises(pkg.AmvHipError, match=r"\(-1\)"):
            ctx.picture_sse(fmt, a.pic("host"), a.pic("host"), w, h, n, np.zeros((n, 3), np.uint64))
    a = Pictures(R.YUV420P, w, h, n).to_dev()
    planes, stride, c_stride, frame, c_frame = a.pic()
    bad = [((planes, stride, c_stride, frame, c_frame), d_sse.data_ptr() + 4),          # a misaligned d_sse
           ((planes, stride, c_stride, frame, c_frame), None),
           ((planes[:2], stride, c_stride, frame, c_frame), d_sse),                     # a plane missing
           ((planes, w - 1, c_stride, frame, c_frame), d_sse),                          # pitches below the row
           ((planes, stride, w // 2 - 1, frame, c_frame), d_sse)]
    for pic, sse in bad:
        with pytest.raises(pkg.AmvHipError, match=r"\(-1\)"):
            ctx.picture_sse_dev(R.YUV420P, pic, a.pic(), w, h, n, sse, stream())
        with pytest.raises(pkg.AmvHipError, match=r"\(-1\)"):
            ctx.picture_sse_dev(R.YUV420P, a.pic(), pic, w, h, n, sse, stream())
    with pytest.raises(pkg.AmvHipError, match=r"\(-1\)"):
        ctx.picture_sse_dev(R.YUV420P, a.pic(), a.pic(), 0, h, n, d_sse, stream())
    torch.cuda.synchronize()
    assert (d_sse.cpu().numpy() == -1).all()
    # no frames: nothing is written
    ctx.picture_sse_dev(R.YUV420P, a.pic(), a.pic(), w, h, 0, d_sse, stream())
    torch.cuda.synchronize()
    assert (d_sse.cpu().numpy() == -1).all()
