"""The pixel-format kernels on the device (amv_pixfmt.hip behind amvhip_img_convert_dev, and the launch loops of
amv_frontend.hip) on crafted pictures: every ragged tail of a 16-column tile, every allowed plane base, every value through
each of the three load / store paths (16-byte vectors, unaligned dwords, single bytes), the inputs pixfmt_builder.py finds
on the rounding steps, clamps and dropped bits of the RGB routes, and batches that make every 65535-frame launch loop (the
five converters', the two of amv_frontend.hip, the one of amv_picture_sse.hip) go round twice.  Byte-exact; the expectation is img_convert_ref.convert (frontend_ref for the front end's own stages), and
every byte outside the pictures' rows is a sentinel that must survive."""
import numpy as np
import pytest

import frontend_ref as F
import img_convert_ref as R
import pixfmt_builder as B
from test_gpu_crafted_rescale import CYCLE, Frames
from test_gpu_img_convert import PAIRS, Strided

pytestmark = pytest.mark.gpu
PAIR_IDS = ["%s-%s" % (R.NAMES[s], R.NAMES[d]) for s, d in PAIRS]
PLANES_PAIRS = [(s, d) for s, d in PAIRS if R.route(s, d) in ("planes", "gray")]


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def convert_strided(ctx, src, frames, dst, w, h, pad, gap=0):
    """frames through amvhip_img_convert_dev in Strided holders -> the destination holder, read back"""
    import torch
    s = Strided(src, w, h, len(frames), pad, gap).fill(frames).to_dev()
    d = Strided(dst, w, h, len(frames), pad, gap).to_dev()
    ctx.img_convert_dev(src, s.pic("dev"), dst, d.pic("dev"), w, h, len(frames), stream())
    torch.cuda.synchronize()
    return d.from_dev()


def check_pictures(ctx, src, dst, frames, w, h, what, pads=(0, 5)):
    want = [R.convert(src, f, dst, w, h) for f in frames]
    for pad in pads:
        convert_strided(ctx, src, frames, dst, w, h, pad, 7 if pad else 0).check(want, "%s -> %s %dx%d pad %d: %s" % (R.NAMES[src], R.NAMES[dst], w, h, pad, what))


def tail_sizes(src, dst):
    """every residue of the width mod 16 the pair's size rule allows, alone and behind a whole tile"""
    if R.any_size(src, dst):
        return [(w, h) for r in range(1, 17) for w in (r, 16 + r) for h in (1, 2, 3)]
    return [(w, 2) for r in range(2, 17, 2) for w in (r, 16 + r)]


def test_the_tail_sizes_cover_every_residue():
    for src, dst in PAIRS:
        sizes = tail_sizes(src, dst)
        want = set(range(16)) if R.any_size(src, dst) else set(range(0, 16, 2))
        assert {w % 16 for w, _ in sizes if w <= 16} == want == {w % 16 for w, _ in sizes if w > 16}


@pytest.mark.parametrize("src,dst", PAIRS, ids=PAIR_IDS)
def test_every_tail_of_every_pair(ctx, src, dst):
    """tight rows and rows padded by 5 (odd row addresses: the unaligned and the byte paths)"""
    for k, (w, h) in enumerate(tail_sizes(src, dst)):
        frames = [R.make_picture(src, w, h, "noise", 31 * src + dst + 1000 * k + i) for i in range(2)]
        check_pictures(ctx, src, dst, frames, w, h, "tails")


def based(ctx, src, frames, dst, w, h, soffs, doffs):
    """tight rows, plane p of the source soffs[p] and of the destination doffs[p] bytes into a 16-byte aligned allocation"""
    import torch
    n = len(frames)
    s = Frames(R.plane_shapes(src, w, h), n, 0, 0, soffs).fill([np.stack([f[p] for f in frames]) for p in range(len(frames[0]))]).to_dev()
    d = Frames(R.plane_shapes(dst, w, h), n, 0, 0, doffs).to_dev()
    assert all(t.data_ptr() % 16 == 0 for t in s.dev + d.dev)
    ctx.img_convert_dev(src, s.pic(), dst, d.pic(), w, h, n, stream())
    torch.cuda.synchronize()
    return d.from_dev()


@pytest.mark.parametrize("src,dst", PAIRS, ids=PAIR_IDS)
def test_every_plane_base_of_every_pair(ctx, pkg, src, dst):
    """32x4, tight rows: every plane of source and destination at +4, +8 and +12 with the others at +0, all planes at
    different bases, and a base at +2 refused"""
    w, h = 32, 4
    frames = [R.make_picture(src, w, h, "noise", 77 * src + dst + i) for i in range(2)]
    want = [R.convert(src, f, dst, w, h) for f in frames]
    expect = [np.stack([x[p] for x in want]) for p in range(len(want[0]))]
    ns, nd = len(frames[0]), len(want[0])
    layouts = [([0] * ns, [0] * nd)]
    for p in range(ns + nd):
        for off in (4, 8, 12):
            offs = [off if k == p else 0 for k in range(ns + nd)]
            layouts.append((offs[:ns], offs[ns:]))
    layouts += [([4, 8, 12][:ns], [12, 4, 8][:nd]), ([8, 12, 4][:ns], [4, 8, 12][:nd]), ([12] * ns, [12] * nd)]
    for soffs, doffs in layouts:
        based(ctx, src, frames, dst, w, h, soffs, doffs).check(expect, "%s -> %s bases %s %s" % (R.NAMES[src], R.NAMES[dst], soffs, doffs))
    for soffs, doffs in (([2] + [0] * (ns - 1), [0] * nd), ([0] * ns, [0] * (nd - 1) + [2])):
        with pytest.raises(pkg.AmvHipError, match=r"\(-1\)"):
            based(ctx, src, frames, dst, w, h, soffs, doffs)


@pytest.mark.parametrize("src,dst", PLANES_PAIRS, ids=["%s-%s" % (R.NAMES[s], R.NAMES[d]) for s, d in PLANES_PAIRS])
def test_every_value_on_every_path_of_the_planes_routes(ctx, src, dst):
    """all 256 values in every plane (so every entry of the route's range tables): 32x32 tight at +0 (16-byte vectors), 32x32
    tight at +4 (unaligned dwords), 14x74 (a ragged tail: single bytes); and the shrinking routes' rounding"""
    for turn, (w, h, off) in enumerate(((32, 32, 0), (32, 32, 4), (14, 74, 0))):
        frames = [B.value_picture(src, w, h, turn), B.value_picture(src, w, h, 101 + turn)]
        want = [R.convert(src, f, dst, w, h) for f in frames]
        ns, nd = len(frames[0]), len(want[0])
        based(ctx, src, frames, dst, w, h, [off] * ns, [off] * nd).check([np.stack([x[p] for x in want]) for p in range(nd)],
                                                                           "values %dx%d at +%d" % (w, h, off))
    if src in R.P422 + R.P444:
        for w in (32, 14):
            check_pictures(ctx, src, dst, [B.shrink_picture(src, w, t) for t in range(4)], w, 2, "shrink rounding")


@pytest.mark.parametrize("src,dst", B.RGB_IN_PAIRS, ids=["%s-%s" % (R.NAMES[s], R.NAMES[d]) for s, d in B.RGB_IN_PAIRS])
def test_rgb_in_on_the_rounding_steps(ctx, src, dst):
    """the patches pixfmt_builder finds on the luma and chroma steps (negative chroma numerators: the shift is arithmetic),
    the corner colours and patches of four different pixels; in whole tiles (32 wide) and with a ragged tail (22 wide)"""
    patches, met = B.rgb_in_patches(dst)
    assert len(met) == (10 if dst == R.YUVJ420P else 8)
    for w in (32, 22):
        planes, h = B.rgb_picture(src, patches, w)
        rolled, _ = B.rgb_picture(src, np.roll(patches, 5, axis=0)[:, ::-1], w)
        check_pictures(ctx, src, dst, [planes, rolled], w, h, "rgb_in steps")


RGB_OUT_PAIRS = [(s, d) for s, d in PAIRS if R.route(s, d) == "rgb_out"]


@pytest.mark.parametrize("src,dst", RGB_OUT_PAIRS, ids=["%s-%s" % (R.NAMES[s], R.NAMES[d]) for s, d in RGB_OUT_PAIRS])
def test_rgb_out_on_the_clamps_and_dropped_bits(ctx, src, dst):
    """(Y, Cb, Cr) whose channels sit at -1, 0, 255, 256 and far outside before the clamp, on negative rounding steps, on
    every channel value (both sides of every bit RGB565 / RGB555 drop) and on the saturated colours"""
    triples, met = B.rgb_out_triples(src)
    assert met["values"] == 768
    for w in (32, 22):
        planes, h = B.yuv_picture(triples, w)
        rolled, _ = B.yuv_picture(np.roll(triples, 7, axis=0), w)
        check_pictures(ctx, src, dst, [planes, rolled], w, h, "rgb_out steps")
    # an odd size: the last column and row serve one pixel
    planes, h = B.yuv_picture(triples, 22)
    odd = [planes[0][:h - 1, :21], planes[1], planes[2]]
    check_pictures(ctx, src, dst, [odd], 21, h - 1, "rgb_out steps, odd size")


# ---- 65537 frames: every launch loop goes round twice ----------------------------------------------------------------------

N_LONG = 65537
LONG_PAIRS = [(R.YUV420P, R.YUVJ420P, 1, 1), (R.YUYV422, R.YUV420P, 2, 2), (R.YUV420P, R.UYVY422, 2, 2), (R.RGB24, R.YUV420P, 2, 2),
              (R.YUVJ420P, R.RGB24, 1, 1)]


def cycle_of(fmt, w, h, seed):
    """CYCLE different noise pictures of a format"""
    frames = [R.make_picture(fmt, w, h, "noise", seed + i) for i in range(CYCLE)]
    assert len({R.join(f).tobytes() for f in frames}) > CYCLE // 2
    return frames


def stacked(pictures, which):
    """[picture][plane] -> [plane] uint8 [len(which), rows, cols], frame k being picture which[k]"""
    return [np.stack([f[p] for f in pictures])[which] for p in range(len(pictures[0]))]


def test_the_long_pairs_are_one_of_each_kernel():
    assert [R.route(s, d) for s, d, _, _ in LONG_PAIRS] == ["planes", "packed_in", "packed_out", "rgb_in", "rgb_out"]
    for s, d, w, h in LONG_PAIRS:
        assert (w, h) == ((1, 1) if R.any_size(s, d) else (2, 2))


@pytest.mark.parametrize("src,dst,w,h", LONG_PAIRS, ids=["%s-%s" % (R.NAMES[s], R.NAMES[d]) for s, d, _, _ in LONG_PAIRS])
def test_a_converter_goes_round_its_launch_loop_twice(ctx, src, dst, w, h):
    """the second launch takes frames 65535 and 65536 from a frame base; frame k is crafted picture k % 251"""
    import torch
    pictures = cycle_of(src, w, h, 4000 + src)
    want = [R.convert(src, f, dst, w, h) for f in pictures]
    which = np.arange(N_LONG) % CYCLE
    s = Frames(R.plane_shapes(src, w, h), N_LONG).fill(stacked(pictures, which)).to_dev()
    d = Frames(R.plane_shapes(dst, w, h), N_LONG, 1, 0).to_dev()
    ctx.img_convert_dev(src, s.pic(), dst, d.pic(), w, h, N_LONG, stream())
    torch.cuda.synchronize()
    d.from_dev().check(stacked(want, which), "65537 frames %s -> %s" % (R.NAMES[src], R.NAMES[dst]))


def test_deinterlace_goes_round_its_launch_loop_twice(ctx):
    import torch
    w, h = 4, 4
    pictures = cycle_of(R.YUV420P, w, h, 5000)
    want = [F.deinterlace(R.YUV420P, f, w, h) for f in pictures]
    which = np.arange(N_LONG) % CYCLE
    s = Frames(R.plane_shapes(R.YUV420P, w, h), N_LONG).fill(stacked(pictures, which)).to_dev()
    d = Frames(R.plane_shapes(R.YUV420P, w, h), N_LONG, 1, 0).to_dev()
    ctx.deinterlace_dev(R.YUV420P, s.pic(), d.pic(), w, h, N_LONG, stream())
    torch.cuda.synchronize()
    d.from_dev().check(stacked(want, which), "65537 frames deinterlaced")


def test_the_pad_bands_go_round_their_launch_loop_twice(ctx, pkg, orc):
    """a 2x2 window inside 4x4 (bands of 2 above and to the right) through amvhip_video_frontend_dev"""
    import torch
    bands, color = (2, 0, 0, 2), (1, 254, 77)
    pictures = cycle_of(R.YUV420P, 2, 2, 6000)
    want = [F.frontend(R.YUV420P, f, 2, 2, 4, 4, orc.img_resample_yuv420, False, (0, 0, 0, 0), bands, color) for f in pictures]
    assert (want[0][0][:2] == color[0]).all() and (want[0][0][2:, :2] != color[0]).any()
    which = np.arange(N_LONG) % CYCLE
    s = Frames(R.plane_shapes(R.YUV420P, 2, 2), N_LONG).fill(stacked(pictures, which)).to_dev()
    d = Frames(R.plane_shapes(R.YUVJ420P, 4, 4), N_LONG, 0, 4).to_dev()
    ctx.video_frontend_dev(R.YUV420P, s.pic(), 2, 2, N_LONG, pkg.Frontend(0, (0, 0, 0, 0), bands, color), d.pic(), 4, 4, stream())
    torch.cuda.synchronize()
    d.from_dev().check(stacked(want, which), "65537 frames padded")


def test_picture_sse_goes_round_its_launch_loop_twice(ctx):
    """the eighth loop over 65535 frames (amv_picture_sse.hip): YUV420P 2x2, the sums of all 65537 frames and the row behind"""
    import torch
    w, h = 2, 2
    a, b = cycle_of(R.YUV420P, w, h, 7000), cycle_of(R.YUV420P, w, h, 8000)
    want = np.array([[((x[p].astype(np.int64) - y[p].astype(np.int64)) ** 2).sum() for p in range(3)] for x, y in zip(a, b)], np.int64)
    assert len({tuple(r) for r in want.tolist()}) > CYCLE // 2
    which = np.arange(N_LONG) % CYCLE
    fa = Frames(R.plane_shapes(R.YUV420P, w, h), N_LONG).fill(stacked(a, which)).to_dev()
    fb = Frames(R.plane_shapes(R.YUV420P, w, h), N_LONG, 1, 3).fill(stacked(b, which)).to_dev()
    d_sse = torch.full((N_LONG + 1, 3), -7, dtype=torch.int64, device="cuda:0")
    ctx.picture_sse_dev(R.YUV420P, fa.pic(), fb.pic(), w, h, N_LONG, d_sse, stream())
    torch.cuda.synchronize()
    got = d_sse.cpu().numpy()
    assert (got[:N_LONG] == want[which]).all(), np.argwhere(got[:N_LONG] != want[which])[:4].tolist()
    assert (got[N_LONG] == -7).all()
