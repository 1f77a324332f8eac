"""The decode-side postprocessing on the device (amvhip_postprocess_dev, amvhip_postprocess, amvhip_decode_pp_batch_dev): byte for
byte the Python restatement (tests/pp_ref.py, pinned to the reference's own pp_postprocess by tests/test_pp_ref.py), at the
smallest shapes that can still go wrong:

  16x16    chroma is a single block: no edge to deblock        32x24    chroma 16x12: the bottom detour, a height off the grid
  48x40    chroma 24x20                                        160x120  chroma 80x60: several lane rounds in the horizontal pass
  336x32   a wide, low picture: more columns than lanes       16x22, 16x48  chroma one block wide and several strips high: its
                                                                only dering call is the row-end one, whose window folds onto itself
"""
import functools

import numpy as np
import pytest

import pp_builder as B
import pp_ref as P

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5


@functools.lru_cache(maxsize=None)
def _picture(w, h, kind, seed, qp):
    return B.picture(w, h, kind, seed, qp)


@functools.lru_cache(maxsize=None)
def _want(w, h, kind, seed, picture_qp, mode_key, qp):
    """the restatement on one picture; mode_key: (lum, chrom, base_dc_diff, flatness_threshold, forced_quant)"""
    m = dict(zip(("lumMode", "chromMode", "baseDcDiff", "flatnessThreshold", "forcedQuant"), mode_key))
    return P.postprocess(_picture(w, h, kind, seed, picture_qp), w, h, m, qp=qp)


def _key(mode):
    return (mode.lum_mode, mode.chrom_mode, mode.base_dc_diff, mode.flatness_threshold, mode.forced_quant)


def _frame_qp(mode, qps, i):
    return int(qps[i]) if qps is not None else mode.forced_quant if mode.lum_mode & P.FORCE_QUANT else 1


def _flat(frames):
    return np.concatenate([np.concatenate([p.reshape(-1) for p in f]) for f in frames])


def _pic(base, w, h):
    """the picture tuple of n tight YUV420P frames that start at `base` (a tensor, an array or an address)"""
    addr = base if isinstance(base, int) else base.data_ptr() if hasattr(base, "data_ptr") else base.ctypes.data
    fb = w * h * 3 // 2
    return ([addr, addr + w * h, addr + w * h + (w // 2) * (h // 2)], w, w // 2, fb, fb)


def run_dev(ctx, pkg, mode, frames, w, h, qps=None):
    import torch
    n = len(frames)
    src = _flat(frames)
    d_src = torch.from_numpy(src).to("cuda:0")
    d_dst = torch.full((src.size + 16,), SENTINEL, dtype=torch.uint8, device="cuda:0")
    d_qp = torch.from_numpy(np.asarray(qps, np.uint8)).to("cuda:0") if qps is not None else None
    ctx.postprocess_dev(pkg.PIX_YUVJ420P, mode, _pic(d_src, w, h), _pic(d_dst, w, h), w, h, n, d_qp, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (d_src.cpu().numpy() == src).all(), "the source was written"
    out = d_dst.cpu().numpy()
    assert (out[src.size:] == SENTINEL).all(), "bytes behind the last frame were written"
    return out[:src.size]


def check(ctx, pkg, mode_text, w, h, n, kind="crafted", quality=6, qps=None, host=False, seed=40, qps_meant=None):
    mode = pkg.pp_mode_parse(mode_text, quality)
    pqp = B.case_qp(mode_text)
    frames = [_picture(w, h, kind, seed + i, pqp) for i in range(n)]
    want = _flat([_want(w, h, kind, seed + i, pqp, _key(mode), _frame_qp(mode, qps_meant or qps, i)) for i in range(n)])
    if host:
        src = _flat(frames)
        keep = src.copy()
        out = np.full(src.size, SENTINEL, np.uint8)
        ctx.postprocess(pkg.PIX_YUV420P, mode, _pic(src, w, h), _pic(out, w, h), w, h, n, None if qps is None else np.asarray(qps, np.uint8))
        assert (src == keep).all()
    else:
        out = run_dev(ctx, pkg, mode, frames, w, h, qps)
    bad = np.flatnonzero(out != want)
    assert bad.size == 0, "%s %dx%d n=%d: %d bytes differ, the first at %d (frame %d): %d, the restatement has %d" % (
        mode_text, w, h, n, bad.size, bad[0], bad[0] // (w * h * 3 // 2), out[bad[0]], want[bad[0]])


@pytest.mark.parametrize("size", B.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("mode", ["hb:c,fq:12", "vb:c,fq:12", "vb:c,dr:c,fq:12", "de:c,fq:12"])
def test_each_filter_and_the_preset(ctx, pkg, size, mode):
    check(ctx, pkg, mode, size[0], size[1], 3)
    check(ctx, pkg, mode, size[0], size[1], 1, kind="noise")


@pytest.mark.parametrize("size", B.NARROW, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("mode", ["de:c,fq:12", "de:c,fq:63", "vb:c,dr:c,fq:3"])
def test_chroma_one_block_wide(ctx, pkg, size, mode):
    """the dering call of an 8-column plane updates the next line's column 0, which is its own next pixel's left neighbour: raster
    order, not the wavefront"""
    check(ctx, pkg, mode, size[0], size[1], 3)
    check(ctx, pkg, mode, size[0], size[1], 2, kind="noise")


def test_a_device_qp_above_63_counts_as_63(ctx, pkg):
    """d_qp lies on the device and the call does not wait for it: what the header says of such entries, pinned"""
    check(ctx, pkg, "de:c", 48, 40, 3, qps=[64, 200, 255], qps_meant=[63, 63, 63])


def test_more_dering_calls_than_lanes(ctx, pkg):
    """656 columns: 82 dering calls a strip against 64 lanes for their ranges, eleven lane rounds in the deblocking passes"""
    check(ctx, pkg, "de:c,fq:12", 656, 16, 2)
    check(ctx, pkg, "de:c,fq:3", 656, 32, 1, kind="noise")


@pytest.mark.parametrize("size", [(32, 24), (48, 40), (160, 120)], ids=lambda s: "%dx%d" % s)
def test_more_frames_than_a_workgroup_has_planes_and_a_qp_per_frame(ctx, pkg, size):
    """a workgroup takes one plane; five frames, then QPs 0, 1, 31 and 63 in one batch (and the mode's own without d_qp)"""
    check(ctx, pkg, "de:c,fq:12", size[0], size[1], 5)
    check(ctx, pkg, "de:c,fq:31", size[0], size[1], 4, qps=[0, 1, 31, 63])
    check(ctx, pkg, "de:c", size[0], size[1], 4, qps=[63, 0, 31, 1])
    check(ctx, pkg, "de:c", size[0], size[1], 2)                                   # no FORCE_QUANT: QP 1


@pytest.mark.parametrize("size", [(16, 16), (48, 40), (336, 32)], ids=lambda s: "%dx%d" % s)
def test_chroma_copied_qualities_and_thresholds(ctx, pkg, size):
    mode = pkg.pp_mode_parse("hb:y,vb:y,dr:y,fq:y:12")               # (an option on the preset itself is dropped, as in the reference)
    assert mode.chrom_mode == 0 and mode.lum_mode == 7 | P.FORCE_QUANT and mode.forced_quant == 12
    check(ctx, pkg, "hb:y,vb:y,dr:y,fq:y:12", size[0], size[1], 2)
    check(ctx, pkg, "de,fq:12", size[0], size[1], 2, quality=4)                    # no dering; chroma deblocked
    check(ctx, pkg, "de,fq:12", size[0], size[1], 2, quality=2)                    # chrom_mode is the force-quant bit alone
    check(ctx, pkg, "hb:c:64:20,vb:c,fq:3", size[0], size[1], 2)
    check(ctx, pkg, "fq:9", size[0], size[1], 1)                                   # no filter at all: a copy


@pytest.mark.parametrize("size", [(32, 24), (160, 120)], ids=lambda s: "%dx%d" % s)
def test_host_buffers(ctx, pkg, size):
    check(ctx, pkg, "de:c,fq:12", size[0], size[1], 3, host=True)
    check(ctx, pkg, "de:c", size[0], size[1], 3, host=True, qps=[63, 5, 0])


def _decode_pp(ctx, pkg, chunks, w, h, dst, mode, out_stride, fb):
    import torch
    n = len(chunks)
    blob = np.frombuffer(b"".join(chunks), np.uint8)
    lens = np.array([len(c) for c in chunks], np.int32)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    pad_blob = np.concatenate([blob, np.zeros((-blob.size) % 4 + 4, np.uint8)])
    d_out = torch.full((fb * n + 16,), SENTINEL, dtype=torch.uint8, device="cuda:0")
    d_st = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    ctx.decode_pp_batch_dev(torch.from_numpy(pad_blob).to("cuda:0"), blob.size, torch.from_numpy(offs).to("cuda:0"), torch.from_numpy(lens).to("cuda:0"),
                            n, w, h, pkg.FLAG_FFMPEG, dst, d_out, out_stride, d_st, mode, None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert (out[fb * n:] == SENTINEL).all()
    return d_out, out[:fb * n], d_st.cpu().numpy()


def test_decode_and_postprocess_in_one_call(ctx, pkg, orc, amv1):
    """== the oracle's FFmpeg-mode decode, then the restatement: the AMV1.amv frames and one damaged chunk; YUVJ420P straight
    out, and RGB24 == img_convert of those planes"""
    import torch
    w, h = amv1["info"]["width"], amv1["info"]["height"]
    chunks = [bytes(c) for c in amv1["video"][:4]]
    chunks[2] = chunks[2][:len(chunks[2]) // 2] + b"\xff\xd9"
    mode = pkg.pp_mode_parse("de:c,fq:12")
    m = dict(zip(("lumMode", "chromMode", "baseDcDiff", "flatnessThreshold", "forcedQuant"), _key(mode)))
    want, want_st = [], []
    for ch in chunks:
        yuv, st, _ = orc.decode_frame_ffmpeg(ch, w, h)
        want.append(P.postprocess([p.copy() for p in orc.yuv_planes(yuv, w, h)], w, h, m))
        want_st.append(st)
    fb = w * h * 3 // 2
    d_planes, planes, st = _decode_pp(ctx, pkg, chunks, w, h, pkg.PIX_YUVJ420P, mode, w, fb)
    assert (st == np.array(want_st)).all() and st[2] != 0 and (np.delete(st, 2) == 0).all()
    assert (planes == _flat(want)).all()
    n = len(chunks)
    rgb_fb = w * 3 * h
    _, rgb, st = _decode_pp(ctx, pkg, chunks, w, h, pkg.PIX_RGB24, mode, w * 3, rgb_fb)
    assert (st == np.array(want_st)).all()
    d_rgb = torch.zeros(rgb_fb * n, dtype=torch.uint8, device="cuda:0")
    ctx.img_convert_dev(pkg.PIX_YUVJ420P, _pic(d_planes, w, h), pkg.PIX_RGB24, ([d_rgb.data_ptr(), None, None], w * 3, 0, rgb_fb, 0), w, h, n,
                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (rgb == d_rgb.cpu().numpy()).all()


def test_refusals_leave_the_destination_untouched(ctx, pkg):
    import torch
    w, h, n = 32, 32, 2
    fb = w * h * 3 // 2
    d_src = torch.zeros(fb * n + 4096, dtype=torch.uint8, device="cuda:0")
    d_dst = torch.full((fb * n + 4096,), SENTINEL, dtype=torch.uint8, device="cuda:0")
    d_qp = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    good = pkg.pp_mode_parse("de:c,fq:12")

    def call(mode=good, src=None, dst=None, ww=w, hh=h, fmt=pkg.PIX_YUVJ420P):
        return ctx.lib.amvhip_postprocess_dev(ctx.h, fmt, None if mode is None else __import__("ctypes").byref(mode), *ctx._pic(src or _pic(d_src, ww, hh)),
                                              *ctx._pic(dst or _pic(d_dst, ww, hh)), ww, hh, n, d_qp.data_ptr(), None)
    assert call() == pkg.OK
    torch.cuda.synchronize()
    d_dst.fill_(SENTINEL)
    planes, s, cs, f, cf = _pic(d_dst, w, h)
    for bad in ((planes, s + 16, cs, f, cf), (planes, s, cs + 8, f, cf), (planes, s * 2, cs * 2, f, cf)):
        assert call(dst=bad) == pkg.ERR_ARG and call(src=bad, dst=_pic(d_src, w, h)) == pkg.ERR_ARG          # pitches other than width, width / 2
    assert call(dst=(planes, s, cs, f + 2, cf + 2)) == pkg.ERR_ARG                                             # frame pitches off 4 bytes
    assert call(dst=_pic(d_src, w, h)) == pkg.ERR_ARG                                                          # the same planes
    assert call(dst=_pic(d_src.data_ptr() + 64, w, h)) == pkg.ERR_ARG                                          # overlapping planes
    for lum, chrom in ((8, 7), (7, 0x400), (P.DERING, 0), (P.DERING | P.H_DEBLOCK, 7), (7, P.DERING), (7, 7 | 0x100000)):
        assert call(mode=pkg.PpMode(lum, chrom)) == pkg.ERR_ARG, (lum, chrom)                                  # bits beyond the three; dr without vb
    assert call(mode=pkg.PpMode(7 | P.FORCE_QUANT, 7, forced_quant=64)) == pkg.ERR_ARG
    assert call(mode=pkg.PpMode(7 | P.FORCE_QUANT, 7, forced_quant=-1)) == pkg.ERR_ARG
    assert call(mode=None) == pkg.ERR_ARG
    for ww, hh in ((24, 32), (32, 18 + 1), (8, 32), (32, 8), (2048, 32)):
        assert call(ww=ww, hh=hh) == pkg.ERR_ARG, (ww, hh)
    for fmt in (pkg.PIX_YUV422P, pkg.PIX_RGB24, pkg.PIX_GRAY8):
        assert call(fmt=fmt) == pkg.ERR_ARG
    # the host form and the joined entry refuse the same modes and sizes
    src, out = np.zeros(fb * n, np.uint8), np.full(fb * n, SENTINEL, np.uint8)
    for mode, ww in ((pkg.PpMode(P.DERING, 0), w), (good, 24)):
        assert ctx.lib.amvhip_postprocess(ctx.h, pkg.PIX_YUV420P, __import__("ctypes").byref(mode), *ctx._pic(_pic(src, ww, h)), *ctx._pic(_pic(out, ww, h)),
                                          ww, h, n, None) == pkg.ERR_ARG
    assert ctx.lib.amvhip_postprocess(ctx.h, pkg.PIX_YUV420P, __import__("ctypes").byref(good), *ctx._pic(_pic(src, w, h)), *ctx._pic(_pic(out, w, h)),
                                      w, h, n, np.array([3, 64], np.uint8).ctypes.data) == pkg.ERR_ARG          # a QP above 63
    assert (out == SENTINEL).all()
    for flags, fmt, stride, mode in ((0, pkg.PIX_RGB24, w * 3, good), (pkg.FLAG_FFMPEG, pkg.PIX_YUVJ420P, w + 4, good), (pkg.FLAG_FFMPEG, pkg.PIX_YUYV422, w * 2, good),
                                     (pkg.FLAG_FFMPEG, pkg.PIX_RGB24, w * 3, pkg.PpMode(P.DERING, 0)), (pkg.FLAG_FFMPEG | pkg.FLAG_FFMPEG_KEEP, pkg.PIX_RGB24, w * 3, good)):
        assert ctx.lib.amvhip_decode_pp_batch_dev(ctx.h, d_src.data_ptr(), 64, d_src.data_ptr(), d_src.data_ptr(), n, w, h, flags, fmt, d_dst.data_ptr(), stride,
                                                  d_src.data_ptr(), __import__("ctypes").byref(mode), None, None) == pkg.ERR_ARG
    torch.cuda.synchronize()
    assert (d_dst.cpu().numpy() == SENTINEL).all() and (d_src.cpu().numpy() == 0).all()


def test_counted_under_the_pixel_format_kernels(ctx, pkg):
    import torch
    w, h = 32, 24
    mode = pkg.pp_mode_parse("de:c,fq:12")
    d_src = torch.zeros(w * h * 3 // 2, dtype=torch.uint8, device="cuda:0")
    d_dst = torch.zeros(w * h * 3 // 2, dtype=torch.uint8, device="cuda:0")
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        ctx.postprocess_dev(pkg.PIX_YUVJ420P, mode, _pic(d_src, w, h), _pic(d_dst, w, h), w, h, 1, None, torch.cuda.current_stream().cuda_stream)
        launches, ms = ctx.prof_read(pkg.K_PIXFMT)
    finally:
        ctx.prof_enable(False)
    assert launches == 1 and ms > 0
