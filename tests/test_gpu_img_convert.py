"""The pixel-format step on the device (amvhip_img_convert*, amvhip_sws_scale_dev, amvhip_encode_fmt_scaled_batch_dev,
amvhip_decode_fmt_batch_dev): byte-identical to the CPU restatement (img_convert_ref.py, itself pinned to the real
reference by test_img_convert.py), to the reference-made hashes of tests/golden/ref_img_convert.json, and -- joined to the
codec -- to the oracle's encoder and FFmpeg-mode decoder.  Strided pictures carry sentinel bytes behind every row and every
frame that must come back untouched."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, SEED
import img_convert_ref as R

FIXTURE = json.load(open(os.path.join(GOLDEN, "ref_img_convert.json")))["cases"]
FMT = {name: i for i, name in enumerate(R.NAMES)}
PAIRS = R.supported_pairs()
SENTINEL = 0xA5


class Strided:
    """n frames of a format with `pad` sentinel bytes behind every row and `gap` behind every frame's plane; one buffer a plane"""

    def __init__(self, fmt, w, h, n, pad, gap):
        self.fmt, self.w, self.h, self.n = fmt, w, h, n
        self.shapes = R.plane_shapes(fmt, w, h)
        self.stride = [c + pad for _, c in self.shapes]
        if len(self.shapes) == 3:
            self.stride[2] = self.stride[1]
        self.frame = [r * s + gap for (r, _), s in zip(self.shapes, self.stride)]
        if len(self.shapes) == 3:
            self.frame[2] = self.frame[1]
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

    def pic(self, where):
        planes = self.dev if where == "dev" else self.host
        return (planes, self.stride[0], self.stride[1] if len(self.stride) > 1 else 0, self.frame[0], self.frame[1] if len(self.frame) > 1 else 0)

    def check(self, want, what):
        """every frame's rows are `want`, every other byte is still the sentinel"""
        for p in range(len(self.shapes)):
            mask = np.ones(self.host[p].size, bool)
            r, c = self.shapes[p]
            for i in range(self.n):
                got = self.rows(self.host[p], p, i)
                assert (got == want[i][p]).all(), "%s: plane %d of frame %d differs at %s" % (what, p, i, np.argwhere(got != want[i][p])[:4].tolist())
                self.rows(mask, p, i)[:] = False
            assert (self.host[p][mask] == SENTINEL).all(), "%s: plane %d: a byte outside the picture's rows was written" % (what, p)


def pictures(fmt, w, h, kinds, seed):
    return [R.make_picture(fmt, w, h, k, seed + i) for i, k in enumerate(kinds)]


def sizes_of(src, dst):
    return [(48, 32), (70, 26)] + ([(37, 23), (1, 1), (17, 2)] if R.any_size(src, dst) else [(2, 2), (18, 6)])


@pytest.mark.gpu
@pytest.mark.parametrize("src,dst", PAIRS, ids=["%s-%s" % (R.NAMES[s], R.NAMES[d]) for s, d in PAIRS])
def test_every_pair_matches_the_restatement(ctx, src, dst):
    """noise, all 0, all 255 and the 16..235 ramp (the clamps of the range tables and of cm), device and host forms, tight
    and padded rows (the padded ones start at odd addresses: the narrow path)"""
    import torch
    kinds = ["noise", "zeros", "ones", "ramp", "noise"]
    for (w, h) in sizes_of(src, dst):
        frames = pictures(src, w, h, kinds, 100 * src + dst)
        want = [R.convert(src, f, dst, w, h) for f in frames]
        for pad, gap in ((0, 0), (5, 7)):
            s = Strided(src, w, h, len(frames), pad, gap).fill(frames).to_dev()
            d = Strided(dst, w, h, len(frames), pad, gap).to_dev()
            ctx.img_convert_dev(src, s.pic("dev"), dst, d.pic("dev"), w, h, len(frames), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            d.from_dev().check(want, "%s -> %s %dx%d pad %d (device)" % (R.NAMES[src], R.NAMES[dst], w, h, pad))
            hd = Strided(dst, w, h, len(frames), pad, gap)
            ctx.img_convert(src, s.pic("host"), dst, hd.pic("host"), w, h, len(frames))
            hd.check(want, "%s -> %s %dx%d pad %d (host)" % (R.NAMES[src], R.NAMES[dst], w, h, pad))


@pytest.mark.gpu
@pytest.mark.parametrize("src,dst", PAIRS, ids=["%s-%s" % (R.NAMES[s], R.NAMES[d]) for s, d in PAIRS])
def test_a_stream_of_frames(ctx, src, dst):
    import torch
    n, w, h = 304, 48, 32
    frames = pictures(src, w, h, ["noise"] * n, 7000 + 100 * src + dst)
    want = [R.convert(src, f, dst, w, h) for f in frames]
    s = Strided(src, w, h, n, 0, 0).fill(frames).to_dev()
    d = Strided(dst, w, h, n, 3, 1).to_dev()
    ctx.img_convert_dev(src, s.pic("dev"), dst, d.pic("dev"), w, h, n, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    d.from_dev().check(want, "%s -> %s, %d frames" % (R.NAMES[src], R.NAMES[dst], n))


@pytest.mark.gpu
def test_the_converters_are_timed(ctx, pkg):
    import torch
    w, h = 64, 48
    s = Strided(R.RGB24, w, h, 2, 0, 0).fill(pictures(R.RGB24, w, h, ["noise"] * 2, 3)).to_dev()
    d = Strided(R.YUV420P, w, h, 2, 0, 0).to_dev()
    ctx.prof_enable(True)
    ctx.prof_reset()
    ctx.img_convert_dev(R.RGB24, s.pic("dev"), R.YUV420P, d.pic("dev"), w, h, 2, torch.cuda.current_stream().cuda_stream)
    launches, ms = ctx.prof_read(pkg.K_PIXFMT)
    ctx.prof_enable(False)
    assert launches == 1 and ms > 0


def encode_dev(ctx, call, n, w, h):
    """run an encode entry (a callable taking blob, cap, offs, lens) -> [chunk bytes]"""
    import torch
    cap = ctx.encode_bound(w, h) * n
    blob = torch.zeros(cap, dtype=torch.uint8, device="cuda:0")
    offs = torch.zeros(n, dtype=torch.int64, device="cuda:0")
    lens = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    call(blob, cap, offs, lens)
    torch.cuda.synchronize()
    b, o, l = blob.cpu().numpy(), offs.cpu().numpy(), lens.cpu().numpy()
    return [b[int(o[i]):int(o[i]) + int(l[i])].tobytes() for i in range(n)]


@pytest.mark.gpu
def test_standalone_rgb24_to_yuvj420p_is_the_encoders_colour_stage(ctx, orc):
    """RGB24 -> YUVJ420P here, then amvhip_encode_yuv420_batch_dev == amvhip_encode_batch_dev on the RGB frames"""
    import torch
    st = torch.cuda.current_stream().cuda_stream
    w, h, n = 160, 120, 6
    frames = [[orc.synth_frame(SEED, t, w, h).reshape(h, w * 3)] for t in range(n - 2)] + pictures(R.RGB24, w, h, ["noise", "ones"], 5)
    s = Strided(R.RGB24, w, h, n, 0, 0).fill(frames).to_dev()
    d = Strided(R.YUVJ420P, w, h, n, 0, 0).to_dev()
    ctx.img_convert_dev(R.RGB24, s.pic("dev"), R.YUVJ420P, d.pic("dev"), w, h, n, st)
    via = encode_dev(ctx, lambda b, c, o, l: ctx.encode_yuv420_batch_dev(d.dev[0], d.dev[1], d.dev[2], d.stride[0], d.stride[1], d.frame[0],
                                                                         d.frame[1], n, w, h, 0, b, c, o, l, st), n, w, h)
    direct = encode_dev(ctx, lambda b, c, o, l: ctx.encode_batch_dev(s.dev[0], w * 3, 0, n, w, h, 0, b, c, o, l, st), n, w, h)
    assert via == direct and all(len(x) > 4 for x in via)
    assert direct[0] == orc.encode_frame(frames[0][0].reshape(h, w, 3), w, h)


def run_sws(ctx, src, frames, sw, sh, dst, dw, dh, pad=0, gap=0):
    import torch
    s = Strided(src, sw, sh, len(frames), pad, gap).fill(frames).to_dev()
    d = Strided(dst, dw, dh, len(frames), pad, gap).to_dev()
    ctx.sws_scale_dev(src, s.pic("dev"), sw, sh, dst, d.pic("dev"), dw, dh, len(frames), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d.from_dev()


@pytest.mark.gpu
@pytest.mark.parametrize("i", [i for i, c in enumerate(FIXTURE) if c.get("chain")])
def test_the_shim_matches_the_reference_chains(ctx, orc, i):
    """352x288 -> 160x120 into YUVJ420P: the reference-made hashes, and restatement o oracle resampler"""
    c = FIXTURE[i]
    src, (sw, sh), (dw, dh) = FMT[c["src"]], c["src_size"], c["dst_size"]
    frames = [R.make_picture(src, sw, sh, c["input"]["kind"], c["input"]["seed"] + k) for k in range(c["frames"])]
    want = [R.sws_scale(src, f, sw, sh, R.YUVJ420P, dw, dh, orc.img_resample_yuv420) for f in frames]
    d = run_sws(ctx, src, frames, sw, sh, R.YUVJ420P, dw, dh, pad=3, gap=5)
    d.check(want, "shim %s" % c["src"])
    got = [R.join([d.rows(d.host[p], p, k) for p in range(3)]) for k in range(c["frames"])]
    assert ["%016x" % R.fnv1a64(g) for g in got] == c["fnv"]


@pytest.mark.gpu
@pytest.mark.parametrize("src,dst,sw,sh,dw,dh", [
    (R.YUV420P, R.RGB24, 352, 288, 160, 120), (R.UYVY422, R.BGR24, 64, 48, 100, 70), (R.RGB32, R.YUV420P, 64, 48, 32, 24),
    (R.YUVJ444P, R.RGB565, 48, 32, 160, 120), (R.YUV420P, R.YUV420P, 64, 48, 64, 48), (R.RGB24, R.RGB24, 33, 17, 33, 17),
    (R.YUYV422, R.YUV420P, 48, 32, 48, 32), (R.YUV420P, R.GRAY8, 64, 48, 30, 20), (R.YUV420P, R.YUYV422, 64, 48, 32, 24)])
def test_the_shim_in_other_directions(ctx, orc, src, dst, sw, sh, dw, dh):
    frames = pictures(src, sw, sh, ["noise", "ramp", "ones"], 31 * src + dst)
    want = [R.sws_scale(src, f, sw, sh, dst, dw, dh, orc.img_resample_yuv420) for f in frames]
    run_sws(ctx, src, frames, sw, sh, dst, dw, dh, pad=5, gap=3).check(want, "shim %s -> %s" % (R.NAMES[src], R.NAMES[dst]))


@pytest.mark.gpu
@pytest.mark.parametrize("src,sw,sh", [(R.YUV420P, 352, 288), (R.YUV422P, 352, 288), (R.YUYV422, 352, 288), (R.RGB24, 352, 288),
                                       (R.UYVY422, 640, 480), (R.YUVJ444P, 64, 48), (R.YUV422P, 160, 120), (R.YUV420P, 160, 120),
                                       (R.YUVJ422P, 160, 120)])
def test_front_end_and_encoder_in_one_call(ctx, orc, src, sw, sh):
    """(restated shim to YUVJ420P at 160x120) -> the oracle's plane encoder, chunk for chunk"""
    import torch
    w, h, n = 160, 120, 4
    frames = pictures(src, sw, sh, ["noise", "ramp", "ones", "noise"], 900 + src)
    s = Strided(src, sw, sh, n, 0, 0).fill(frames).to_dev()
    got = encode_dev(ctx, lambda b, c, o, l: ctx.encode_fmt_scaled_batch_dev(src, s.pic("dev"), sw, sh, n, w, h, 0, b, c, o, l,
                                                                             torch.cuda.current_stream().cuda_stream), n, w, h)
    for k, f in enumerate(frames):
        y, cb, cr = R.sws_scale(src, f, sw, sh, R.YUVJ420P, w, h, orc.img_resample_yuv420)
        assert got[k] == orc.encode_frame_yuv(y, cb, cr, w, h), "frame %d" % k


@pytest.mark.gpu
def test_front_end_identity_cases_are_the_existing_entries(ctx, orc):
    import torch
    st = torch.cuda.current_stream().cuda_stream
    w, h, n = 160, 120, 5
    for fmt, bgr in ((R.RGB24, 0), (R.BGR24, 1)):
        frames = pictures(fmt, w, h, ["noise", "ramp", "ones", "zeros", "noise"], 40 + fmt)
        s = Strided(fmt, w, h, n, 0, 0).fill(frames).to_dev()
        new = encode_dev(ctx, lambda b, c, o, l: ctx.encode_fmt_scaled_batch_dev(fmt, s.pic("dev"), w, h, n, w, h, 0, b, c, o, l, st), n, w, h)
        old = encode_dev(ctx, lambda b, c, o, l: ctx.encode_batch_dev(s.dev[0], w * 3, bgr, n, w, h, 0, b, c, o, l, st), n, w, h)
        assert new == old and all(len(x) > 4 for x in new)
    frames = pictures(R.YUVJ420P, w, h, ["noise", "ramp", "ones", "zeros", "noise"], 77)
    s = Strided(R.YUVJ420P, w, h, n, 4, 8).fill(frames).to_dev()
    new = encode_dev(ctx, lambda b, c, o, l: ctx.encode_fmt_scaled_batch_dev(R.YUVJ420P, s.pic("dev"), w, h, n, w, h, 0, b, c, o, l, st), n, w, h)
    old = encode_dev(ctx, lambda b, c, o, l: ctx.encode_yuv420_batch_dev(s.dev[0], s.dev[1], s.dev[2], s.stride[0], s.stride[1], s.frame[0],
                                                                         s.frame[1], n, w, h, 0, b, c, o, l, st), n, w, h)
    assert new == old and all(len(x) > 4 for x in new)
    # ... and the scaled YUV420P entry is the shim without its range step: different bytes from the whole shim
    frames = pictures(R.YUV420P, 352, 288, ["ramp"] * n, 5)
    s = Strided(R.YUV420P, 352, 288, n, 0, 0).fill(frames).to_dev()
    shim = encode_dev(ctx, lambda b, c, o, l: ctx.encode_fmt_scaled_batch_dev(R.YUV420P, s.pic("dev"), 352, 288, n, w, h, 0, b, c, o, l, st), n, w, h)
    bare = encode_dev(ctx, lambda b, c, o, l: ctx._check(ctx.lib.amvhip_encode_yuv420_scaled_batch_dev(
        ctx.h, s.dev[0].data_ptr(), s.dev[1].data_ptr(), s.dev[2].data_ptr(), s.stride[0], s.stride[1], s.frame[0], s.frame[1], 352, 288, n, w, h, 0,
        b.data_ptr(), c, o.data_ptr(), l.data_ptr(), st), "encode_yuv420_scaled_batch_dev"), n, w, h)
    y, cb, cr = R.split(R.YUV420P, w, h, orc.img_resample_yuv420(R.join(frames[0]), 352, 288, w, h))
    assert bare[0] == orc.encode_frame_yuv(y, cb, cr, w, h) and shim != bare


def decode_fmt(ctx, pkg, chunks, w, h, dst, pad):
    import torch
    n = len(chunks)
    blob = np.frombuffer(b"".join(chunks), np.uint8)
    lens = np.array([len(c) for c in chunks], np.int32)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    pad_blob = np.concatenate([blob, np.zeros((-blob.size) % 4 + 4, np.uint8)])
    out_stride = w * R.BPP.get(dst, 1) + pad
    fb = ctx.lib.amvhip_pix_frame_bytes(dst, out_stride, h)
    d_out = torch.full((fb * n + 16,), SENTINEL, dtype=torch.uint8, device="cuda:0")
    d_st = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    ctx.decode_fmt_batch_dev(torch.from_numpy(pad_blob).to("cuda:0"), blob.size, torch.from_numpy(offs).to("cuda:0"),
                             torch.from_numpy(lens).to("cuda:0"), n, w, h, pkg.FLAG_FFMPEG, dst, d_out, out_stride, d_st,
                             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), d_st.cpu().numpy(), out_stride, fb


def check_decode_fmt(ctx, pkg, orc, chunks, w, h, dst, pad):
    out, st, stride, fb = decode_fmt(ctx, pkg, chunks, w, h, dst, pad)
    mask = np.ones(out.size, bool)
    for i, ch in enumerate(chunks):
        yuv, want_st, _ = orc.decode_frame_ffmpeg(ch, w, h)
        assert st[i] == want_st
        want = R.convert(R.YUVJ420P, R.split(R.YUVJ420P, w, h, yuv), dst, w, h)
        pos = i * fb
        for p, (rows, cols) in enumerate(R.plane_shapes(dst, w, h)):
            s = stride if p == 0 else (stride + 1) // 2
            got = np.lib.stride_tricks.as_strided(out[pos:], (rows, cols), (s, 1))
            assert (got == want[p]).all(), "frame %d plane %d of %s" % (i, p, R.NAMES[dst])
            np.lib.stride_tricks.as_strided(mask[pos:], (rows, cols), (s, 1))[:] = False
            pos += rows * s
    assert (out[mask] == SENTINEL).all(), "a byte outside the pictures' rows was written"
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("dst", [R.RGB24, R.BGR24, R.RGB32, R.RGB565, R.RGB555, R.GRAY8, R.YUV420P], ids=lambda d: R.NAMES[d])
def test_decoder_and_back_end_in_one_call(ctx, pkg, orc, amv1, dst):
    """AMV1.amv with one damaged chunk among its frames, and a synthetic stream at another size"""
    w, h = amv1["info"]["width"], amv1["info"]["height"]
    chunks = [bytes(c) for c in amv1["video"][:10]]
    chunks[4] = chunks[4][:len(chunks[4]) // 2] + b"\xff\xd9"                    # cut in the middle of its scan
    st = check_decode_fmt(ctx, pkg, orc, chunks, w, h, dst, pad=4)
    assert st[4] != 0 and (np.delete(st, 4) == 0).all()
    blob, offs, lens = orc.synth_stream(SEED, 0, 6, 176, 144)
    chunks = [blob[int(o):int(o) + int(l)].tobytes() for o, l in zip(offs, lens)]
    check_decode_fmt(ctx, pkg, orc, chunks, 176, 144, dst, pad=0)
    # the decoder takes odd sizes, and so do these routes: the same chunks as a 173 x 141 picture
    check_decode_fmt(ctx, pkg, orc, chunks, 173, 141, dst, pad=3)


def _call_convert(lib, h, src, dst, w, hh, planes_src=(64, 64, 64), planes_dst=(64, 64, 64), strides=(4096, 4096)):
    return lib.amvhip_img_convert_dev(h, src, planes_src[0], planes_src[1], planes_src[2], strides[0], strides[0], 1 << 20, 1 << 20,
                                      dst, planes_dst[0], planes_dst[1], planes_dst[2], strides[1], strides[1], 1 << 20, 1 << 20, w, hh, 1,
                                      None)


@pytest.mark.gpu
def test_entry_points_refuse_bad_arguments(ctx, pkg):
    """AMVHIP_ERR_ARG before anything reaches the device: the addresses handed in are never dereferenced on a refusal, and the
    calls that are accepted here have n = 0"""
    lib, h, P = ctx.lib, ctx.h, pkg
    # pairs the reference reaches only through an intermediate picture, or not at all
    for src, dst in ((P.PIX_YUYV422, P.PIX_YUVJ420P), (P.PIX_BGR24, P.PIX_YUVJ420P), (P.PIX_RGB32, P.PIX_YUVJ420P), (P.PIX_RGB24, P.PIX_BGR24),
                     (P.PIX_YUVJ420P, P.PIX_YUYV422), (P.PIX_RGB565, P.PIX_YUV420P), (P.PIX_YUV420P, P.PIX_YUV422P), (P.PIX_GRAY8, P.PIX_YUV420P),
                     (P.PIX_YUV420P, P.PIX_YUV420P), (14, 0), (0, -1)):
        assert _call_convert(lib, h, src, dst, 16, 16) == P.ERR_ARG, (src, dst)
    # odd sizes on the subsampling routes; fine on the routes out of 4:2:0 (n = 0: nothing runs)
    for src, dst in ((P.PIX_RGB24, P.PIX_YUV420P), (P.PIX_YUYV422, P.PIX_YUV420P), (P.PIX_YUV444P, P.PIX_YUVJ420P), (P.PIX_YUV422P, P.PIX_YUV420P),
                     (P.PIX_YUV420P, P.PIX_UYVY422), (P.PIX_RGB24, P.PIX_YUVJ420P)):
        assert _call_convert(lib, h, src, dst, 17, 16) == P.ERR_ARG and _call_convert(lib, h, src, dst, 16, 17) == P.ERR_ARG, (src, dst)
    assert _call_convert(lib, h, P.PIX_RGB24, P.PIX_YUV420P, 0, 16) == P.ERR_ARG
    assert _call_convert(lib, h, P.PIX_RGB24, P.PIX_YUV420P, 16386, 16) == P.ERR_ARG
    # null plane, misaligned plane, pitch below the row
    assert _call_convert(lib, h, P.PIX_RGB24, P.PIX_YUV420P, 16, 16, planes_src=(None, None, None)) == P.ERR_ARG
    assert _call_convert(lib, h, P.PIX_RGB24, P.PIX_YUV420P, 16, 16, planes_dst=(64, None, 64)) == P.ERR_ARG
    assert _call_convert(lib, h, P.PIX_RGB24, P.PIX_YUV420P, 16, 16, planes_dst=(64, 66, 64)) == P.ERR_ARG
    assert _call_convert(lib, h, P.PIX_RGB24, P.PIX_YUV420P, 16, 16, strides=(47, 4096)) == P.ERR_ARG
    assert _call_convert(lib, h, P.PIX_YUVJ420P, P.PIX_RGB32, 16, 16, strides=(4096, 63)) == P.ERR_ARG
    # the shim: each of its conversions must be a supported pair at its size
    sws = lambda sf, sw, sh, df, dw, dh: lib.amvhip_sws_scale_dev(h, sf, 64, 64, 64, 8192, 8192, 1 << 22, 1 << 22, sw, sh, df, 64, 64, 64, 8192,
                                                                  8192, 1 << 22, 1 << 22, dw, dh, 0, None)
    assert sws(P.PIX_YUYV422, 64, 64, P.PIX_YUVJ420P, 64, 64) == P.ERR_ARG          # equal sizes: two steps in the reference
    assert sws(P.PIX_YUYV422, 64, 64, P.PIX_YUVJ420P, 32, 32) == P.OK               # via YUV420P: one step each side
    assert sws(P.PIX_RGB565, 64, 64, P.PIX_YUV420P, 32, 32) == P.ERR_ARG
    assert sws(P.PIX_RGB24, 63, 64, P.PIX_YUV420P, 32, 32) == P.ERR_ARG
    assert sws(P.PIX_YUV420P, 64, 64, P.PIX_YUV422P, 32, 32) == P.ERR_ARG
    assert sws(P.PIX_YUV420P, 64, 64, P.PIX_RGB24, 33, 31) == P.OK
    assert sws(P.PIX_YUV420P, 64, 64, P.PIX_YUV420P, 1, 32) == P.ERR_ARG
    # the encoder behind the shim
    enc = lambda sf, sw, sh, w, hh, q=0, blob=64: lib.amvhip_encode_fmt_scaled_batch_dev(h, sf, 64, 64, 64, 8192, 8192, 1 << 22, 1 << 22, sw, sh, 1,
                                                                                         w, hh, q, blob, 4096, 64, 64, None)
    assert enc(P.PIX_YUV420P, 64, 64, 33, 32) == P.ERR_ARG and enc(P.PIX_YUV420P, 64, 64, 32, 32, q=256) == P.ERR_ARG
    assert enc(P.PIX_YUV420P, 64, 64, 32, 32, blob=None) == P.ERR_ARG
    assert enc(P.PIX_RGB32, 32, 32, 32, 32) == P.ERR_ARG and enc(P.PIX_RGB555, 64, 64, 32, 32) == P.ERR_ARG
    # the decoder in front of the converter
    dec = lambda flags, fmt, stride=64 * 4, out=64: lib.amvhip_decode_fmt_batch_dev(h, 64, 16, 64, 64, 0, 64, 64, flags, fmt, out, stride, 64, None)
    assert dec(0, P.PIX_RGB24) == P.ERR_ARG and dec(P.FLAG_ZIGZAG_FIXED, P.PIX_RGB24) == P.ERR_ARG       # AMVHIP_FLAG_FFMPEG is required
    assert dec(P.FLAG_FFMPEG | P.FLAG_FFMPEG_KEEP, P.PIX_RGB24) == P.ERR_ARG
    assert dec(P.FLAG_FFMPEG, P.PIX_YUVJ420P) == P.ERR_ARG and dec(P.FLAG_FFMPEG, P.PIX_YUYV422) == P.ERR_ARG
    assert dec(P.FLAG_FFMPEG, P.PIX_RGB24, stride=64 * 3 - 1) == P.ERR_ARG
    assert dec(P.FLAG_FFMPEG, P.PIX_RGB24) == P.OK and dec(P.FLAG_FFMPEG, P.PIX_YUV420P, stride=64) == P.OK


@pytest.mark.gpu
@pytest.mark.parametrize("dst", [R.RGB24, R.RGB32, R.RGB565, R.GRAY8], ids=lambda d: R.NAMES[d])
def test_the_shim_towards_an_odd_size_is_deterministic(ctx, orc, dst):
    """img_resample writes (w >> 1) x (h >> 1) chroma, the routines out of YUV420P read (w + 1) / 2 x (h + 1) / 2: the column
    and row in between, undefined in the reference, are 128 here whatever the workspace held before (a first call fills it)"""
    sw, sh, dw, dh = 64, 48, 33, 31
    run_sws(ctx, R.YUV420P, pictures(R.YUV420P, sw, sh, ["ones"] * 3, 1), sw, sh, dst, dw + 1, dh + 1)
    frames = pictures(R.YUV420P, sw, sh, ["noise", "ramp", "zeros"], 55 + dst)
    want = []
    for f in frames:
        out = orc.img_resample_yuv420(R.join(f), sw, sh, dw, dh)
        cw, ch = dw >> 1, dh >> 1
        y = out[:dw * dh].reshape(dh, dw)
        chroma = [np.full(((dh + 1) // 2, (dw + 1) // 2), 128, np.uint8) for _ in range(2)]
        for k, c in enumerate(chroma):
            c[:ch, :cw] = out[dw * dh + k * cw * ch:dw * dh + (k + 1) * cw * ch].reshape(ch, cw)
        want.append(R.convert(R.YUV420P, [y] + chroma, dst, dw, dh))
    run_sws(ctx, R.YUV420P, frames, sw, sh, dst, dw, dh, pad=3, gap=1).check(want, "shim to %s at 33x31" % R.NAMES[dst])
