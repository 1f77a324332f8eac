"""The picture rescaler on the device (amv_resample.hip behind amvhip_resample_yuv420_dev, amvhip_sws_scale_dev and the
scaled encoder entries) on the crafted cases of rescale_ref.py: every phase of both filters, both clamps at both ends,
sources narrower than the taps, ratios of 8192 : 1 both ways, odd sizes, all 256 entries of both range tables through the
store that carries the range step, and batches that make the 65535-frame launch loop go round twice.  Byte-exact
everywhere; the expectation is the oracle (orc.img_resample_yuv420, or img_convert_ref.sws_scale around it) -- the numpy
model of rescale_ref.py only built the cases.  Every byte outside the pictures' rows is a sentinel that must survive.

The narrow source: for a source plane narrower than the four taps the reference's h_resample is undefined
(imgresample.c:339-341); the library repeats the edge sample, as the oracle does, and the edges cases pin that."""
import numpy as np
import pytest

import img_convert_ref as R
import rescale_ref as RR
from test_gpu_img_convert import Strided, encode_dev, run_sws

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
CYCLE = 251                    # a prime: frame k of a long batch is crafted frame k % 251, so a wrong frame base shows


class Frames:
    """n frames of one format, a buffer per plane, whole batches at a time: `pad` sentinel bytes behind every row, `gap`
    behind every frame's plane, and plane p starting offs[p] bytes into its (16-byte aligned) allocation.
    shapes: [(rows, row bytes)] of the planes"""

    def __init__(self, shapes, n, pad=0, gap=0, offs=(0, 0, 0)):
        self.shapes, self.n, self.offs = shapes, n, offs
        self.stride = [shapes[min(p, 1)][1] + pad for p in range(len(shapes))]
        self.frame = [shapes[min(p, 1)][0] * self.stride[p] + gap for p in range(len(shapes))]
        self.host = [np.full(offs[p] + self.frame[p] * n + 16, SENTINEL, np.uint8) for p in range(len(shapes))]
        self.dev = None

    def view(self, buf, p):
        r, c = self.shapes[p]
        return np.lib.stride_tricks.as_strided(buf[self.offs[p]:], (self.n, r, c), (self.frame[p], self.stride[p], 1))

    def fill(self, planes):
        """planes[p]: uint8 [n, rows, row bytes]"""
        for p, a in enumerate(planes):
            self.view(self.host[p], p)[:] = a
        return self

    def to_dev(self):
        import torch
        self.dev = [torch.from_numpy(b).to("cuda:0") for b in self.host]
        return self

    def from_dev(self):
        self.host = [d.cpu().numpy() for d in self.dev]
        return self

    def ptr(self, p):
        return self.dev[p].data_ptr() + self.offs[p] if p < len(self.shapes) else None

    def pic(self):
        many = len(self.shapes) > 1
        return ([self.ptr(p) for p in range(len(self.shapes))], self.stride[0], self.stride[1] if many else 0, self.frame[0],
                self.frame[1] if many else 0)

    def check(self, want, what):
        """every frame's rows are want[p][frame], every other byte is still the sentinel"""
        for p in range(len(self.shapes)):
            got = self.view(self.host[p], p)
            if not (got == want[p]).all():
                raise AssertionError("%s: plane %d differs at (frame, row, column) %s" % (what, p, np.argwhere(got != want[p])[:4].tolist()))
            mask = np.ones(self.host[p].size, bool)
            self.view(mask, p)[:] = False
            assert (self.host[p][mask] == SENTINEL).all(), "%s: plane %d: a byte outside the pictures' rows was written" % (what, p)

    def untouched(self):
        return all((b == SENTINEL).all() for b in self.host)


def planes_of(frames, w, h):
    """tight frames [n, frame bytes] -> [Y [n, h, w], Cb, Cr [n, h >> 1, w >> 1]]"""
    out, pos = [], 0
    for r, c in RR.plane_sizes(w, h):
        out.append(frames[:, pos:pos + r * c].reshape(len(frames), r, c))
        pos += r * c
    return out


def resample(ctx, s, iw, ih, d, ow, oh, n):
    import torch
    rc = ctx.lib.amvhip_resample_yuv420_dev(ctx.h, s.ptr(0), s.ptr(1), s.ptr(2), s.stride[0], s.stride[1], s.frame[0], s.frame[1], iw, ih,
                                            d.ptr(0), d.ptr(1), d.ptr(2), d.stride[0], d.stride[1], d.frame[0], d.frame[1], ow, oh, n, None)
    torch.cuda.synchronize()
    return rc


def batches(orc, group):
    """the cases of a group, those of one size pair joined: [(size, frames, oracle frames)]"""
    by_size = {}
    for c in RR.by_group(orc, group):
        by_size.setdefault(c.size, []).append(c)
    return [(size, np.concatenate([c.frames for c in cs]), np.concatenate([RR.expected(orc, c) for c in cs])) for size, cs in by_size.items()]


@pytest.mark.parametrize("group", ["phases", "clamps", "edges", "ratios", "odd", "flat"])
def test_the_plain_entry_on_every_case(ctx, orc, group):
    """amvhip_resample_yuv420_dev: padded rows and frames on both sides, every plane base at each of the offsets 0..3 (this
    entry has no alignment rule)"""
    for size, frames, want in batches(orc, group):
        iw, ih, ow, oh = size
        n = len(frames)
        src, expect = planes_of(frames, iw, ih), planes_of(want, ow, oh)
        for k in range(4):
            so, do = ((k, k + 1, k + 2), (k + 3, k + 2, k + 1))
            s = Frames(RR.plane_sizes(iw, ih), n, 5, 3, [o % 4 for o in so]).fill(src).to_dev()
            d = Frames(RR.plane_sizes(ow, oh), n, 3, 7, [o % 4 for o in do]).to_dev()
            assert resample(ctx, s, iw, ih, d, ow, oh, n) == 0
            d.from_dev().check(expect, "%s %dx%d -> %dx%d at offsets %d" % (group, iw, ih, ow, oh, k))


def test_flat_pictures_drive_both_range_tables_through_the_shim(ctx, orc):
    """256 flat frames, YUV420P 4x4 -> YUVJ420P 2x2: the rescaler keeps every flat value, so its store's range step sees all
    256 entries of y_ccir_to_jpeg and of c_ccir_to_jpeg"""
    flat = RR.by_name(orc, "flat-4x4-2x2").frames
    frames = [R.split(R.YUV420P, 4, 4, f) for f in flat]
    d = run_sws(ctx, R.YUV420P, frames, 4, 4, R.YUVJ420P, 2, 2, pad=3, gap=5)
    want = [[np.full((2, 2), R.TABLES["y_ccir_to_jpeg"][v], np.uint8)] + [np.full((1, 1), R.TABLES["c_ccir_to_jpeg"][v], np.uint8)] * 2
            for v in range(256)]
    d.check(want, "flat 4x4 -> 2x2 to YUVJ420P")
    # (the restated shim around the oracle says the same)
    assert all((a == b).all() for x, f in zip(want, frames)
               for a, b in zip(x, R.sws_scale(R.YUV420P, f, 4, 4, R.YUVJ420P, 2, 2, orc.img_resample_yuv420)))


@pytest.mark.parametrize("group", ["phases", "clamps"])
def test_the_shim_to_yuvj420p_on_the_phases_and_clamps_cases(ctx, orc, group):
    for size, tight, _ in batches(orc, group):
        iw, ih, ow, oh = size
        frames = [R.split(R.YUV420P, iw, ih, f) for f in tight]
        want = [R.sws_scale(R.YUV420P, f, iw, ih, R.YUVJ420P, ow, oh, orc.img_resample_yuv420) for f in frames]
        run_sws(ctx, R.YUV420P, frames, iw, ih, R.YUVJ420P, ow, oh, pad=3, gap=5).check(want, "shim %s %dx%d -> %dx%d" % (group, iw, ih, ow, oh))


def test_the_scaled_encoder_entries_encode_the_crafted_planes(ctx, pkg, orc):
    """34x34 -> 32x32, the noise of the phases case and the stripes of the clamps cases at that size: the chunks of
    amvhip_encode_fmt_scaled_batch_dev are the oracle's encoder on the restated shim's planes, and the planes of
    amvhip_video_frontend_dev are those planes"""
    import torch
    iw, ih, w, h = 34, 34, 32, 32
    tight = np.concatenate([RR.by_name(orc, "phases-34x34-32x32").frames, RR.stripe_frames(iw, ih)])
    frames = [R.split(R.YUV420P, iw, ih, f) for f in tight]
    n = len(frames)
    want = [R.sws_scale(R.YUV420P, f, iw, ih, R.YUVJ420P, w, h, orc.img_resample_yuv420) for f in frames]
    st = torch.cuda.current_stream().cuda_stream
    s = Strided(R.YUV420P, iw, ih, n, 5, 3).fill(frames).to_dev()
    got = encode_dev(ctx, lambda b, c, o, l: ctx.encode_fmt_scaled_batch_dev(R.YUV420P, s.pic("dev"), iw, ih, n, w, h, 0, b, c, o, l, st), n, w, h)
    for k, p in enumerate(want):
        assert got[k] == orc.encode_frame_yuv(p[0], p[1], p[2], w, h), "picture %d" % k
    d = Strided(R.YUVJ420P, w, h, n, 3, 5).to_dev()
    ctx.video_frontend_dev(R.YUV420P, s.pic("dev"), iw, ih, n, None, d.pic("dev"), w, h, st)
    torch.cuda.synchronize()
    d.from_dev().check(want, "front end 34x34 -> 32x32")


def crafted_cycle(orc):
    """CYCLE frames of 4x4 (noise, all different) and the oracle's 2x2 of each"""
    frames = np.random.default_rng(251).integers(0, 256, (CYCLE, RR.frame_bytes(4, 4)), dtype=np.uint8)
    assert len({f.tobytes() for f in frames}) == CYCLE
    want = np.stack([orc.img_resample_yuv420(f, 4, 4, 2, 2) for f in frames])
    assert len({f.tobytes() for f in want}) > CYCLE // 2
    return frames, want


@pytest.mark.parametrize("dst", [R.YUV420P, R.YUVJ420P], ids=lambda f: R.NAMES[f])
def test_the_shim_goes_round_its_launch_loop_twice(ctx, orc, dst):
    """65537 frames of 4x4 -> 2x2 through amvhip_sws_scale_dev: the second launch takes frames 65535 and 65536"""
    import torch
    n = 65537
    frames, want = crafted_cycle(orc)
    which = np.arange(n) % CYCLE
    expect = planes_of(want, 2, 2)
    if dst == R.YUVJ420P:
        expect = [R.TABLES["y_ccir_to_jpeg"][expect[0]]] + [R.TABLES["c_ccir_to_jpeg"][p] for p in expect[1:]]
        one = R.sws_scale(R.YUV420P, R.split(R.YUV420P, 4, 4, frames[7]), 4, 4, dst, 2, 2, orc.img_resample_yuv420)
        assert all((a == b[7]).all() for a, b in zip(one, expect))
    s = Frames(RR.plane_sizes(4, 4), n).fill([p[which] for p in planes_of(frames, 4, 4)]).to_dev()
    d = Frames(RR.plane_sizes(2, 2), n, 2, 0).to_dev()
    ctx.sws_scale_dev(R.YUV420P, s.pic(), 4, 4, dst, d.pic(), 2, 2, n, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    d.from_dev().check([p[which] for p in expect], "65537 frames to %s" % R.NAMES[dst])


def test_the_plain_entry_takes_65535_frames_and_refuses_65536(ctx, pkg, orc):
    frames, want = crafted_cycle(orc)
    for n in (65535, 65536):
        which = np.arange(n) % CYCLE
        s = Frames(RR.plane_sizes(4, 4), n).fill([p[which] for p in planes_of(frames, 4, 4)]).to_dev()
        d = Frames(RR.plane_sizes(2, 2), n, 1, 0, (1, 2, 3)).to_dev()
        rc = resample(ctx, s, 4, 4, d, 2, 2, n)
        if n == 65535:
            assert rc == pkg.OK
            d.from_dev().check([p[which] for p in planes_of(want, 2, 2)], "65535 frames")
        else:
            assert rc == pkg.ERR_ARG
            assert d.from_dev().untouched(), "a refused call wrote to its destination"
