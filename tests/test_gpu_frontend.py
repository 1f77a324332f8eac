"""The video front end on the device (amvhip_deinterlace*, amvhip_video_frontend_dev, amvhip_encode_frontend_batch_dev):
byte-identical to the CPU restatement (frontend_ref.py, itself pinned to the real reference by test_frontend_ref.py), to the
reference-made hashes of tests/golden/ref_frontend.json and -- joined to the encoder -- to the oracle's encoder.  Strided
pictures carry sentinel bytes behind every row and every frame that must come back untouched."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
import frontend_ref as F
import img_convert_ref as R

FIXTURE = json.load(open(os.path.join(GOLDEN, "ref_frontend.json")))["cases"]
FMT = {name: i for i, name in enumerate(R.NAMES)}
SENTINEL = 0x5A


class Pictures:
    """n frames of a format, a buffer per plane, `pad` sentinel bytes behind every row and `gap` behind every frame's plane"""

    def __init__(self, fmt, w, h, n, pad=0, gap=0):
        self.fmt, self.w, self.h, self.n = fmt, w, h, n
        self.shapes = R.plane_shapes(fmt, w, h)
        self.stride = [self.shapes[min(p, 1)][1] + pad for p in range(len(self.shapes))]
        self.frame = [self.shapes[min(p, 1)][0] * self.stride[p] + gap for p in range(len(self.shapes))]
        self.host = [np.full(f * n + 16, SENTINEL, np.uint8) for f in self.frame]
        self.dev = None

    def rows(self, buf, p, i):
        r, c = self.shapes[p]
        return np.lib.stride_tricks.as_strided(buf[i * self.frame[p]:], (r, c), (self.stride[p], 1))

    def fill(self, frames):
        for i, planes in enumerate(frames):
            for p, plane in enumerate(planes):
                self.rows(self.host[p], p, i)[:] = plane
        return self

    def to_dev(self):
        import torch
        self.dev = [torch.from_numpy(b).to("cuda:0") for b in self.host]
        return self

    def from_dev(self):
        self.host = [d.cpu().numpy() for d in self.dev]
        return self

    def pic(self, where="dev"):
        planes = self.dev if where == "dev" else self.host
        many = len(self.stride) > 1
        return (planes, self.stride[0], self.stride[1] if many else 0, self.frame[0], self.frame[1] if many else 0)

    def planes(self, i):
        return [self.rows(self.host[p], p, i).copy() for p in range(len(self.shapes))]

    def check(self, want, what):
        """every frame's rows are `want`, every other byte is still the sentinel"""
        for p in range(len(self.shapes)):
            mask = np.ones(self.host[p].size, bool)
            for i in range(self.n):
                got = self.rows(self.host[p], p, i)
                assert (got == want[i][p]).all(), "%s: plane %d of frame %d differs at %s" % (what, p, i, np.argwhere(got != want[i][p])[:4].tolist())
                self.rows(mask, p, i)[:] = False
            assert (self.host[p][mask] == SENTINEL).all(), "%s: plane %d: a byte outside the picture's rows was written" % (what, p)

    def untouched(self):
        return all((b == SENTINEL).all() for b in self.host)


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def rows_picture(fmt, w, h, rows_of):
    """every plane's row y is the constant rows_of(y, rows of the plane)"""
    return [np.repeat(np.array([[rows_of(y, r)] for y in range(r)], np.uint8), c, axis=1) for r, c in R.plane_shapes(fmt, w, h)]


def deinterlace_contents(fmt, w, h, seed):
    """noise, all 0, all 255, the two clamp pictures (rows 255 0 255 255 255 0 ...: an inner odd row with 255 at the three
    middle taps and 0 at the outer ones sums to 2550, (sum + 4) >> 3 = 319; the inverse picture gives -64), and two pictures
    whose row 3 has sum + 4 = -1 and -8: the shift is arithmetic, both are -1 and clamp to 0 (a logical shift would clamp
    to 255)"""
    hi = rows_picture(fmt, w, h, lambda y, r: 255 if y % 2 == 0 or y % 4 == 3 else 0)
    pics = [R.make_picture(fmt, w, h, "noise", seed), R.make_picture(fmt, w, h, "zeros"), R.make_picture(fmt, w, h, "ones"), hi, [255 - p for p in hi]]
    # row 3 of 0 5 0 0 ...: sum + 4 = -1; of 0 12 0 0: -8.  Row 1 of the same pictures: (2 * 5 + 4) >> 3 = 1, (2 * 12 + 4) >> 3 = 3
    pics.append(rows_picture(fmt, w, h, lambda y, r: 5 if y == 1 else 0))
    pics.append(rows_picture(fmt, w, h, lambda y, r: 12 if y == 1 else 0))
    return pics


DEINT_SIZES = [(4, 4), (8, 8), (36, 8), (48, 32)]


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", F.DEINTERLACED, ids=lambda f: R.NAMES[f])
def test_deinterlace_matches_the_restatement(ctx, fmt):
    """4x4 (both odd rows are the special first and last), 8x8, 36x8 (4:2:0 chroma 18x4: the byte path), 48x32; tight rows and
    rows padded by 5 with a 7-byte frame gap (odd addresses); device and host forms"""
    for (w, h) in DEINT_SIZES:
        frames = deinterlace_contents(fmt, w, h, 10 * fmt + w)
        want = [F.deinterlace(fmt, f, w, h) for f in frames]
        n = len(frames)
        for pad, gap in ((0, 0), (5, 7)):
            s = Pictures(fmt, w, h, n, pad, gap).fill(frames).to_dev()
            d = Pictures(fmt, w, h, n, pad, gap).to_dev()
            ctx.deinterlace_dev(fmt, s.pic(), d.pic(), w, h, n, stream())
            import torch
            torch.cuda.synchronize()
            d.from_dev().check(want, "deinterlace %s %dx%d pad %d (device)" % (R.NAMES[fmt], w, h, pad))
            hd = Pictures(fmt, w, h, n, pad, gap)
            ctx.deinterlace(fmt, s.pic("host"), hd.pic("host"), w, h, n)
            hd.check(want, "deinterlace %s %dx%d pad %d (host)" % (R.NAMES[fmt], w, h, pad))
    # the crafted rows did what they are for
    w, h = 8, 8
    frames = deinterlace_contents(fmt, w, h, 0)
    assert F.deinterlace(fmt, frames[3], w, h)[0][3, 0] == 255 and F.deinterlace(fmt, frames[4], w, h)[0][3, 0] == 0
    assert F.deinterlace(fmt, frames[5], w, h)[0][:4, 0].tolist() == [0, 1, 0, 0] and F.deinterlace(fmt, frames[6], w, h)[0][:4, 0].tolist() == [0, 3, 0, 0]


@pytest.mark.gpu
def test_deinterlace_refusals_leave_the_destination_alone(ctx, pkg):
    import torch
    P = pkg
    for fmt, w, h in ((R.YUVJ420P, 8, 8), (R.RGB24, 8, 8), (R.YUV420P, 6, 4), (R.YUV420P, 4, 6), (R.YUYV422, 8, 8)):
        s = Pictures(fmt, w, h, 2).fill([R.make_picture(fmt, w, h, "noise", k) for k in range(2)]).to_dev()
        d = Pictures(fmt, w, h, 2).to_dev()
        with pytest.raises(P.AmvHipError, match=r"\(-1\)"):
            ctx.deinterlace_dev(fmt, s.pic(), d.pic(), w, h, 2, stream())
        hd = Pictures(fmt, w, h, 2)
        with pytest.raises(P.AmvHipError, match=r"\(-1\)"):
            ctx.deinterlace(fmt, s.pic("host"), hd.pic("host"), w, h, 2)
        torch.cuda.synchronize()
        assert d.from_dev().untouched() and hd.untouched()
    # overlapping buffers: the same planes, and planes shifted by two rows
    w, h = 8, 8
    s = Pictures(R.YUV420P, w, h, 2).fill([R.make_picture(R.YUV420P, w, h, "noise", k) for k in range(2)]).to_dev()
    before = [b.copy() for b in s.host]
    with pytest.raises(P.AmvHipError, match="overlap"):
        ctx.deinterlace_dev(R.YUV420P, s.pic(), s.pic(), w, h, 2, stream())
    shifted = ([s.dev[0].data_ptr() + 16, s.dev[1].data_ptr(), s.dev[2].data_ptr()], s.stride[0], s.stride[1], s.frame[0], s.frame[1])
    other = Pictures(R.YUV420P, w, h, 2).to_dev()
    mixed = ([other.dev[0], s.dev[1], other.dev[2]], other.stride[0], other.stride[1], other.frame[0], other.frame[1])
    for dst in (shifted, mixed):
        with pytest.raises(P.AmvHipError, match="overlap"):
            ctx.deinterlace_dev(R.YUV420P, s.pic(), dst, w, h, 1, stream())
    with pytest.raises(P.AmvHipError, match="overlap"):
        ctx.deinterlace(R.YUV420P, s.pic("host"), s.pic("host"), w, h, 2)
    torch.cuda.synchronize()
    assert all((a == b).all() for a, b in zip(before, s.from_dev().host)) and other.from_dev().untouched()


def run_frontend(ctx, pkg, src, frames, sw, sh, fe, w, h, pad=3, gap=5):
    import torch
    s = Pictures(src, sw, sh, len(frames)).fill(frames).to_dev()
    d = Pictures(R.YUVJ420P, w, h, len(frames), pad, gap).to_dev()
    ctx.video_frontend_dev(src, s.pic(), sw, sh, len(frames), fe, d.pic(), w, h, stream())
    torch.cuda.synchronize()
    return d.from_dev()


@pytest.mark.gpu
@pytest.mark.parametrize("bands", [(2, 2, 2, 2), (4, 0, 0, 2)])
@pytest.mark.parametrize("src", [R.YUV420P, R.YUV422P, R.YUV444P], ids=lambda f: R.NAMES[f])
def test_windowed_deinterlace_through_the_front_end(ctx, pkg, orc, src, bands):
    """16x12, deinterlace + crop, no rescale (the inner size is the cropped one): the restatement's deinterlace of the FULL
    picture, then crop, then convert"""
    w, h = 16, 12
    frames = [R.make_picture(src, w, h, k, 3 + i) for i, k in enumerate(("noise", "ramp", "noise"))]
    cw, ch = w - bands[2] - bands[3], h - bands[0] - bands[1]
    want = []
    for f in frames:
        kept, _, _ = F.crop(src, F.deinterlace(src, f, w, h), w, h, bands)
        want.append(R.convert(src, kept, R.YUVJ420P, cw, ch))
    chain = [F.frontend(src, f, w, h, cw, ch, orc.img_resample_yuv420, True, bands) for f in frames]
    assert all((a == b).all() for x, y in zip(want, chain) for a, b in zip(x, y))
    fe = pkg.Frontend(1, bands)
    run_frontend(ctx, pkg, src, frames, w, h, fe, cw, ch).check(want, "deinterlace + crop %s of %s" % (bands, R.NAMES[src]))
    # without the deinterlace: the crop alone, on the caller's planes (no workspace picture)
    plain = [R.convert(src, F.crop(src, f, w, h, bands)[0], R.YUVJ420P, cw, ch) for f in frames]
    run_frontend(ctx, pkg, src, frames, w, h, pkg.Frontend(0, bands), cw, ch).check(plain, "crop %s of %s" % (bands, R.NAMES[src]))


PADS = [(2, 0, 0, 0), (0, 2, 0, 0), (0, 0, 2, 0), (0, 0, 0, 2), (2, 4, 6, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("color", [(16, 128, 128), (1, 254, 77)])
@pytest.mark.parametrize("pad", PADS)
def test_pad_bands_around_the_window(ctx, pkg, orc, pad, color):
    """a 2x2 window (each side alone at 2: inside 4x2 / 2x4; all four at 2/4/6/2: inside 10x8), by the copy route from a
    YUVJ420P source and by the convert route; and the rescale route 8x8 -> 4x2 into a window of a larger picture"""
    top, bottom, left, right = pad
    fe = pkg.Frontend(0, (0, 0, 0, 0), pad, color)
    for src in (R.YUVJ420P, R.YUV420P):
        frames = [R.make_picture(src, 2, 2, "noise", 50 + i) for i in range(3)]
        w, h = 2 + left + right, 2 + top + bottom
        want = [F.frontend(src, f, 2, 2, w, h, orc.img_resample_yuv420, False, (0, 0, 0, 0), pad, color) for f in frames]
        for f, o in zip(frames, want):                                   # what the restatement says, said once more
            window = f if src == R.YUVJ420P else R.convert(src, f, R.YUVJ420P, 2, 2)
            for i in range(3):
                sh = 1 if i else 0
                inside = np.zeros(o[i].shape, bool)
                inside[top >> sh:(top >> sh) + (2 >> sh), left >> sh:(left >> sh) + (2 >> sh)] = True
                assert (o[i][inside] == window[i].reshape(-1)).all() and (o[i][~inside] == color[i]).all()
        for strides in ((0, 0), (3, 5)):
            run_frontend(ctx, pkg, src, frames, 2, 2, fe, w, h, *strides).check(want, "pad %s around 2x2 from %s" % (pad, R.NAMES[src]))
    frames = [R.make_picture(R.YUV420P, 8, 8, k, 60 + i) for i, k in enumerate(("noise", "ramp", "ones"))]
    w, h = 4 + left + right, 2 + top + bottom
    want = [F.frontend(R.YUV420P, f, 8, 8, w, h, orc.img_resample_yuv420, False, (0, 0, 0, 0), pad, color) for f in frames]
    run_frontend(ctx, pkg, R.YUV420P, frames, 8, 8, fe, w, h).check(want, "pad %s around the rescaled 4x2" % (pad,))


@pytest.mark.gpu
def test_pad_window_2x2_inside_6x6_and_the_rescale_into_8x6(ctx, pkg, orc):
    """the sizes the feature was specified with: window 2x2 inside 6x6 (pads 2 2 2 2), 8x8 -> 4x2 inside 8x6 (pads 2 2 2 2)"""
    for color in ((16, 128, 128), (1, 254, 77)):
        fe = pkg.Frontend(0, (0, 0, 0, 0), (2, 2, 2, 2), color)
        frames = [R.make_picture(R.YUVJ420P, 2, 2, "noise", 70 + i) for i in range(2)]
        want = [F.pad(f, 6, 6, (2, 2, 2, 2), color) for f in frames]
        run_frontend(ctx, pkg, R.YUVJ420P, frames, 2, 2, fe, 6, 6).check(want, "2x2 inside 6x6")
        frames = [R.make_picture(R.YUV420P, 8, 8, "noise", 80 + i) for i in range(2)]
        want = [F.pad(R.sws_scale(R.YUV420P, f, 8, 8, R.YUVJ420P, 4, 2, orc.img_resample_yuv420), 8, 6, (2, 2, 2, 2), color) for f in frames]
        run_frontend(ctx, pkg, R.YUV420P, frames, 8, 8, fe, 8, 6).check(want, "8x8 -> 4x2 inside 8x6")


def encode_dev(ctx, call, n, w, h, cap=None):
    """run an encode entry (a callable taking blob, cap, offs, lens) -> (blob, offs, lens) as numpy"""
    import torch
    cap = cap if cap is not None else ctx.encode_bound(w, h) * n
    blob = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
    offs = torch.zeros(n, dtype=torch.int64, device="cuda:0")
    lens = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    call(blob, cap, offs, lens)
    torch.cuda.synchronize()
    return blob.cpu().numpy(), offs.cpu().numpy(), lens.cpu().numpy()


def chunks_of(blob, offs, lens):
    return [blob[int(o):int(o) + int(l)].tobytes() for o, l in zip(offs, lens)]


def case_frontend(pkg, c):
    color = F.pad_color_from_rgb(int(c["padcolor"], 16)) if c["padcolor"] else F.DEFAULT_COLOR
    return pkg.Frontend(int(c["deinterlace"]), tuple(c["crop"]), tuple(c["pad"]), color), color


@pytest.mark.gpu
@pytest.mark.parametrize("i", [i for i, c in enumerate(FIXTURE) if c["pinned_by"] == "reference"])
def test_the_front_end_matches_the_reference_cases(ctx, pkg, orc, i):
    """every pinned case of ref_frontend.json: the planes of amvhip_video_frontend_dev hash to what the reference's command line
    wrote; the 352x288 -> 160x90 inside 160x120 chains also through the encoder, chunk for chunk the oracle's on the restated planes"""
    c = FIXTURE[i]
    src, (sw, sh), (w, h), n = FMT[c["src"]], c["src_size"], c["dst_size"], c["frames"]
    frames = [R.make_picture(src, sw, sh, c["input"]["kind"], c["input"]["seed"] + k) for k in range(n)]
    fe, color = case_frontend(pkg, c)
    if c["padcolor"]:
        assert color == pkg.pad_color_from_rgb(int(c["padcolor"], 16))
    d = run_frontend(ctx, pkg, src, frames, sw, sh, fe, w, h)
    assert ["%016x" % R.fnv1a64(R.join(d.planes(k))) for k in range(n)] == c["fnv"]
    want = [F.frontend(src, f, sw, sh, w, h, orc.img_resample_yuv420, c["deinterlace"], tuple(c["crop"]), tuple(c["pad"]), color) for f in frames]
    d.check(want, "case %d" % i)
    if c["chain"]:
        s = Pictures(src, sw, sh, n).fill(frames).to_dev()
        got = chunks_of(*encode_dev(ctx, lambda b, cap, o, l: ctx.encode_frontend_batch_dev(src, s.pic(), sw, sh, n, fe, w, h, 0, b, cap, o, l, stream()), n, w, h))
        assert got == [orc.encode_frame_yuv(p[0], p[1], p[2], w, h) for p in want]


@pytest.mark.gpu
def test_no_stage_is_the_entry_without_them(ctx, pkg):
    """fe NULL and fe all zero: blob, offsets and lengths of amvhip_encode_fmt_scaled_batch_dev -- RGB24 and YUVJ420P at the
    target size (the fused and the direct route), YUV420P 352x288 -> 160x120 (the shim)"""
    w, h, n = 160, 120, 4
    for src, sw, sh, pad, gap in ((R.RGB24, w, h, 0, 0), (R.YUVJ420P, w, h, 4, 8), (R.YUV420P, 352, 288, 0, 0)):
        frames = [R.make_picture(src, sw, sh, k, 90 + src + i) for i, k in enumerate(("noise", "ramp", "ones", "noise"))]
        s = Pictures(src, sw, sh, n, pad, gap).fill(frames).to_dev()
        old = encode_dev(ctx, lambda b, c, o, l: ctx.encode_fmt_scaled_batch_dev(src, s.pic(), sw, sh, n, w, h, 0, b, c, o, l, stream()), n, w, h)
        assert all(int(x) > 4 for x in old[2])
        for fe in (None, pkg.Frontend(), pkg.Frontend(0, (0, 0, 0, 0), (0, 0, 0, 0), (9, 9, 9))):
            new = encode_dev(ctx, lambda b, c, o, l: ctx.encode_frontend_batch_dev(src, s.pic(), sw, sh, n, fe, w, h, 0, b, c, o, l, stream()), n, w, h)
            assert all((a == b).all() for a, b in zip(old, new)), R.NAMES[src]


@pytest.mark.gpu
def test_front_end_refusals(ctx, pkg):
    """AMVHIP_ERR_ARG before anything reaches the device (the addresses handed in are never dereferenced); a blob too small
    is reported as amvhip_encode_fmt_scaled_batch_dev reports it: the chunks that do not fit have length 0"""
    lib, hdl, P = ctx.lib, ctx.h, pkg
    import ctypes

    def front(src_fmt, sw, sh, fe, w, hh, n=0):
        return lib.amvhip_video_frontend_dev(hdl, src_fmt, 64, 64, 64, 8192, 8192, 1 << 22, 1 << 22, sw, sh, n, ctypes.addressof(fe) if fe else None,
                                             64, 64, 64, 8192, 8192, 1 << 22, 1 << 22, w, hh, None)

    def enc(src_fmt, sw, sh, fe, w, hh, n=0):
        return lib.amvhip_encode_frontend_batch_dev(hdl, src_fmt, 64, 64, 64, 8192, 8192, 1 << 22, 1 << 22, sw, sh, n, ctypes.addressof(fe) if fe else None,
                                                    w, hh, 0, 64, 4096, 64, 64, None)

    for call in (front, enc):
        assert call(P.PIX_YUV420P, 64, 48, P.Frontend(0, (2, 2, 2, 2), (2, 2, 2, 2)), 32, 24) == P.OK
        for k in range(4):                                                                       # an odd band
            band = tuple(3 if j == k else 0 for j in range(4))
            assert call(P.PIX_YUV420P, 64, 48, P.Frontend(0, band), 32, 24) == P.ERR_ARG
            assert call(P.PIX_YUV420P, 64, 48, P.Frontend(0, (0, 0, 0, 0), band), 32, 24) == P.ERR_ARG
        assert call(P.PIX_YUYV422, 64, 48, P.Frontend(0, (2, 0, 0, 0)), 32, 24) == P.ERR_ARG      # av_picture_crop: planar YUV only
        assert call(P.PIX_RGB24, 64, 48, P.Frontend(0, (0, 0, 2, 0)), 32, 24) == P.ERR_ARG
        assert call(P.PIX_YUYV422, 64, 48, P.Frontend(0, (0, 0, 0, 0), (2, 0, 0, 0)), 32, 24) == P.OK
        assert call(P.PIX_YUV420P, 64, 48, P.Frontend(0, (0, 0, 0, 0), (12, 12, 0, 0)), 32, 24) == P.ERR_ARG   # pads >= the size
        assert call(P.PIX_YUV420P, 64, 48, P.Frontend(0, (0, 0, 0, 0), (0, 0, 32, 0)), 32, 24) == P.ERR_ARG
        assert call(P.PIX_YUV420P, 64, 48, P.Frontend(0, (0, 0, 0, 0), (12, 11 - 1, 0, 0)), 32, 24) == P.OK    # a window of 32x2
        assert call(P.PIX_YUV420P, 64, 48, P.Frontend(0, (0, 0, 0, 0), (12, 12, 0, 0)), 32, 26) == P.OK
        assert call(P.PIX_YUV420P, 64, 48, P.Frontend(0, (24, 24, 0, 0)), 32, 24) == P.ERR_ARG                 # nothing of the source left
        assert call(P.PIX_YUV420P, 64, 48, P.Frontend(0, (24, 22, 0, 0)), 32, 24) == P.OK
        assert call(P.PIX_YUV420P, 64, 48, P.Frontend(1), 33, 24) == P.ERR_ARG and call(P.PIX_YUV420P, 64, 48, P.Frontend(1), 32, 25) == P.ERR_ARG
        assert call(P.PIX_YUYV422, 32, 22, P.Frontend(0, (0, 0, 0, 0), (2, 0, 0, 0)), 32, 24) == P.ERR_ARG     # two steps in the reference
        assert call(P.PIX_RGB565, 64, 48, P.Frontend(1), 32, 24) == P.ERR_ARG
    assert front(P.PIX_YUV420P, 64, 48, None, 32, 24) == P.OK
    # a blob with room for two chunks of four
    w, h, n = 32, 24, 4
    frames = [R.make_picture(R.YUV420P, 64, 48, "noise", 7 + i) for i in range(n)]
    s = Pictures(R.YUV420P, 64, 48, n).fill(frames).to_dev()
    fe = P.Frontend(1, (2, 2, 0, 0), (2, 2, 2, 2))
    full = encode_dev(ctx, lambda b, c, o, l: ctx.encode_frontend_batch_dev(R.YUV420P, s.pic(), 64, 48, n, fe, w, h, 0, b, c, o, l, stream()), n, w, h)
    cap = int(full[2][0] + full[2][1]) + 10
    short = encode_dev(ctx, lambda b, c, o, l: ctx.encode_frontend_batch_dev(R.YUV420P, s.pic(), 64, 48, n, fe, w, h, 0, b, c, o, l, stream()), n, w, h, cap)
    assert [int(x) for x in short[2]] == [int(full[2][0]), int(full[2][1]), 0, 0] and chunks_of(*short)[:2] == chunks_of(*full)[:2]


@pytest.mark.gpu
def test_the_front_end_kernels_are_timed(ctx, pkg):
    """deinterlace and pad bands are counted under AMVHIP_K_PIXFMT, beside the shim's own launch"""
    w, h, n = 16, 16, 2
    frames = [R.make_picture(R.YUV420P, w, h, "noise", i) for i in range(n)]
    s = Pictures(R.YUV420P, w, h, n).fill(frames).to_dev()
    d = Pictures(R.YUVJ420P, w + 4, h + 4, n).to_dev()
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        ctx.video_frontend_dev(R.YUV420P, s.pic(), w, h, n, pkg.Frontend(), d.pic(), w, h, stream())
        shim_alone, _ = ctx.prof_read(pkg.K_PIXFMT)
        ctx.prof_reset()
        ctx.video_frontend_dev(R.YUV420P, s.pic(), w, h, n, pkg.Frontend(1, (0, 0, 0, 0), (2, 2, 2, 2)), d.pic(), w + 4, h + 4, stream())
        launches, ms = ctx.prof_read(pkg.K_PIXFMT)
        ctx.prof_reset()
        d2 = Pictures(R.YUV420P, w, h, n).to_dev()
        ctx.deinterlace_dev(R.YUV420P, s.pic(), d2.pic(), w, h, n, stream())
        alone, ms_alone = ctx.prof_read(pkg.K_PIXFMT)
    finally:
        ctx.prof_enable(False)
    assert shim_alone == 1 and launches == 3 and ms > 0 and alone == 1 and ms_alone > 0
