"""No-GPU checks of the pixel-format step (img_convert and the sws_scale shim of the reference): the CPU restatement in
img_convert_ref.py against outputs of the real reference (tests/golden/ref_img_convert.json, made by
tests/golden/make_ref_img_convert_golden.py), the four range tables against closed forms, the restatement against what
oracle/_ref holds of the reference, and the new entry points' presence and refusals through the built library."""
import ctypes
import json
import os
from fractions import Fraction

import numpy as np
import pytest

from conftest import GOLDEN
import img_convert_ref as R

FIXTURE = json.load(open(os.path.join(GOLDEN, "ref_img_convert.json")))["cases"]
FMT = {name: i for i, name in enumerate(R.NAMES)}
NEW_SYMBOLS = ("amvhip_img_convert_supported", "amvhip_pix_frame_bytes", "amvhip_img_convert_dev", "amvhip_img_convert",
               "amvhip_sws_scale_dev", "amvhip_encode_fmt_scaled_batch_dev", "amvhip_decode_fmt_batch_dev")


def case_inputs(c):
    (sw, sh), src = c["src_size"], FMT[c["src"]]
    return [R.make_picture(src, sw, sh, c["input"]["kind"], c["input"]["seed"] + i) for i in range(c["frames"])]


def restated(c, orc):
    (sw, sh), (dw, dh) = c["src_size"], c["dst_size"]
    return [R.join(R.sws_scale(FMT[c["src"]], p, sw, sh, FMT[c["dst"]], dw, dh, orc.img_resample_yuv420)) for p in case_inputs(c)]


def check_against_fixture(c, frames):
    """frames: tight output frames (uint8 arrays) of a case the reference pinned"""
    (dw, dh), dst = c["dst_size"], FMT[c["dst"]]
    assert len(frames) == c["frames"]
    got_rows = [[row.tolist() for row in p[:2]] for p in R.split(dst, dw, dh, frames[0])]
    assert got_rows == c["rows"][0], (c["src"], c["dst"], c["src_size"])
    assert ["%016x" % R.fnv1a64(f) for f in frames] == c["fnv"], (c["src"], c["dst"], c["src_size"])


def test_fixture_covers_what_it_should():
    conv = [c for c in FIXTURE if "src" in c and not c["chain"]]
    assert {(FMT[c["src"]], FMT[c["dst"]]) for c in conv} == set(R.supported_pairs())
    for pair in R.supported_pairs():
        sizes = {tuple(c["src_size"]) for c in conv if (FMT[c["src"]], FMT[c["dst"]]) == pair}
        assert len(sizes) >= 2
        if R.route(*pair) in ("gray", "rgb_out"):
            assert any(w & 1 and h & 1 for w, h in sizes)
    chains = {c["src"] for c in FIXTURE if c.get("chain")}
    assert chains == {"yuv420p", "yuv422p", "yuyv422", "rgb24"}
    assert all(c["src_size"] == [352, 288] and c["dst_size"] == [160, 120] and c["dst"] == "yuvj420p" for c in FIXTURE if c.get("chain"))
    assert {c["dst"] for c in FIXTURE if "clip" in c} == {"yuv420p", "rgb24"}
    # what the real reference did not pin: only the odd sizes, which its raw-video command line refuses
    for c in FIXTURE:
        if c["pinned_by"] != "reference":
            assert c["src_size"][0] & 1 and "multiple of 2" in c["refusal"]
    assert os.path.getsize(os.path.join(GOLDEN, "ref_img_convert.json")) < os.path.getsize(os.path.join(GOLDEN, "AMV1.amv")) // 4


@pytest.mark.parametrize("i", [i for i, c in enumerate(FIXTURE) if "src" in c])
def test_restatement_reproduces_the_reference(i, orc):
    c = FIXTURE[i]
    frames = restated(c, orc)
    if c["pinned_by"] == "reference":
        check_against_fixture(c, frames)
    else:                                     # odd sizes: the shapes at least
        assert all(f.size == R.frame_bytes(FMT[c["dst"]], *c["dst_size"]) for f in frames)


@pytest.mark.parametrize("dst", ["yuv420p", "rgb24"])
def test_restatement_on_a_decoded_clip(dst, orc, amv1):
    """ffmpeg -i AMV1.amv -pix_fmt yuv420p|rgb24: the reference's amv decoder, then img_convert from YUVJ420P"""
    c = [c for c in FIXTURE if c.get("clip") == "AMV1.amv" and c["dst"] == dst][0]
    assert c["pinned_by"] == "reference"
    w, h = amv1["info"]["width"], amv1["info"]["height"]
    assert c["bytes"] == c["frames"] * R.frame_bytes(FMT[dst], w, h)
    for i in range(c["frames"]):
        yuv, st, _ = orc.decode_frame_ffmpeg(amv1["video"][i], w, h)
        assert st == 0
        out = R.join(R.convert(R.YUVJ420P, R.split(R.YUVJ420P, w, h, yuv), FMT[dst], w, h))
        assert "%016x" % R.fnv1a64(out) == c["fnv"][i]


def test_range_tables_have_their_closed_forms():
    """all 4 x 256 entries against the exact rationals of colorspace.h:69-84: round(x * 2^10) constants, floor of the
    fixed-point product, the clamps"""
    def fix(fr):
        return int(fr * 1024 + Fraction(1, 2))               # FIX(): (int)(x * 1024 + 0.5), x > 0
    ky, kyi, kc, kci = fix(Fraction(255, 219)), fix(Fraction(219, 255)), fix(Fraction(127, 112)), fix(Fraction(112, 127))
    assert (ky, kyi, kc, kci) == (R.FIX(255.0 / 219.0), R.FIX(219.0 / 255.0), R.FIX(127.0 / 112.0), R.FIX(112.0 / 127.0)) == (1192, 879, 1161, 903)
    t = R.range_tables()
    for i in range(256):
        assert t["y_ccir_to_jpeg"][i] == min(max(((i - 16) * ky + 512) // 1024, 0), 255)
        assert t["y_jpeg_to_ccir"][i] == (i * kyi + 512) // 1024 + 16
        assert t["c_ccir_to_jpeg"][i] == min(max(((i - 128) * kc + 512) // 1024 + 128, 0), 255)
        assert t["c_jpeg_to_ccir"][i] == max(((i - 128) * kci + 512) // 1024 + 128, 16)
    # the nominal ranges map onto each other, and the clamps are reached
    assert t["y_ccir_to_jpeg"][16] == 0 and t["y_ccir_to_jpeg"][235] == 255 and t["y_ccir_to_jpeg"][0] == 0 and t["y_ccir_to_jpeg"][255] == 255
    assert t["y_jpeg_to_ccir"][0] == 16 and t["y_jpeg_to_ccir"][255] == 235
    assert t["c_ccir_to_jpeg"][16] == 1 and t["c_ccir_to_jpeg"][240] == 255 and t["c_ccir_to_jpeg"][128] == 128
    assert t["c_jpeg_to_ccir"][0] == 16 and t["c_jpeg_to_ccir"][255] == 240 and t["c_jpeg_to_ccir"][128] == 128


def test_rgb24_to_yuvj420p_is_the_reference_routine(orc):
    ref = orc.avcref()
    if ref is None:
        pytest.skip("oracle/_ref is not built here")
    for w, h, seed in ((48, 32, 1), (70, 26, 2), (160, 120, 3)):
        pic = R.make_picture(R.RGB24, w, h, "noise", seed)
        y, cb, cr = (np.zeros(s, np.uint8) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2)))
        rgb = np.ascontiguousarray(pic[0])
        ref.amvref_rgb24_to_yuvj420p(rgb.ctypes.data, w * 3, w, h, y.ctypes.data, cb.ctypes.data, cr.ctypes.data)
        got = R.convert(R.RGB24, pic, R.YUVJ420P, w, h)
        assert (got[0] == y).all() and (got[1] == cb).all() and (got[2] == cr).all()


def test_shim_with_yuv420p_on_both_sides_is_the_resampler(orc):
    pic = R.make_picture(R.YUV420P, 352, 288, "noise", 11)
    out = R.join(R.sws_scale(R.YUV420P, pic, 352, 288, R.YUV420P, 160, 120, orc.img_resample_yuv420))
    assert out.tobytes() == orc.img_resample_yuv420(R.join(pic), 352, 288, 160, 120).tobytes()
    same = R.sws_scale(R.YUV420P, pic, 352, 288, R.YUV420P, 352, 288, orc.img_resample_yuv420)
    assert R.join(same).tobytes() == R.join(pic).tobytes()


def test_new_entry_points_are_exported(pkg):
    lib = pkg.load_library()
    for name in NEW_SYMBOLS:
        assert name in pkg.SYMBOLS and getattr(lib, name) is not None
    assert pkg.PIX_COUNT == 14 and [getattr(pkg, "PIX_" + n.upper().replace("GRAY", "GRAY8")) for n in R.NAMES] == list(range(14))
    assert pkg.K_PIXFMT == 12 and lib.amvhip_kernel_name(pkg.K_PIXFMT).decode().startswith("amv_pix_")
    # the supported pairs are the restatement's, no more and no less
    for s in range(-1, 15):
        for d in range(-1, 15):
            known = 0 <= s < 14 and 0 <= d < 14 and R.route(s, d) is not None
            assert bool(lib.amvhip_img_convert_supported(s, d, 16, 16)) == known, (s, d)
            # odd sizes: only the routes out of 4:2:0 planes; never an empty or oversized picture
            for w, h in ((17, 16), (16, 17), (37, 23)):
                assert bool(lib.amvhip_img_convert_supported(s, d, w, h)) == (known and R.any_size(s, d)), (s, d, w, h)
            assert not lib.amvhip_img_convert_supported(s, d, 0, 16) and not lib.amvhip_img_convert_supported(s, d, 16, 16386)
    assert lib.amvhip_pix_frame_bytes(pkg.PIX_RGB24, 480, 120) == 480 * 120
    assert lib.amvhip_pix_frame_bytes(pkg.PIX_YUV420P, 161, 121) == 161 * 121 + 2 * 81 * 61
    assert lib.amvhip_pix_frame_bytes(pkg.PIX_YUVJ444P, 10, 4) == 120 and lib.amvhip_pix_frame_bytes(14, 10, 4) == 0


def _call_convert(lib, h, src, dst, w, hh, planes_src=(64, 64, 64), planes_dst=(64, 64, 64), strides=(4096, 4096)):
    return lib.amvhip_img_convert_dev(h, src, planes_src[0], planes_src[1], planes_src[2], strides[0], strides[0], 1 << 20, 1 << 20,
                                      dst, planes_dst[0], planes_dst[1], planes_dst[2], strides[1], strides[1], 1 << 20, 1 << 20, w, hh, 1,
                                      None)


def test_entry_points_refuse_a_null_context(pkg):
    """AMVHIP_ERR_ARG with no device at hand (the addresses handed in are never dereferenced on a refusal); the refusals that
    need a context are in test_gpu_img_convert.py, and those of pairs and sizes are amvhip_img_convert_supported's above"""
    lib = pkg.load_library()
    P = pkg
    assert _call_convert(lib, None, P.PIX_RGB24, P.PIX_YUV420P, 16, 16) == P.ERR_ARG
    assert lib.amvhip_sws_scale_dev(None, 0, 64, 64, 64, 64, 32, 4096, 1024, 64, 64, 1, 64, 64, 64, 32, 16, 4096, 1024, 32, 32, 1, None) == P.ERR_ARG
    assert lib.amvhip_encode_fmt_scaled_batch_dev(None, 0, 64, 64, 64, 64, 32, 4096, 1024, 64, 64, 1, 32, 32, 0, 64, 4096, 64, 64, None) == P.ERR_ARG
    assert lib.amvhip_decode_fmt_batch_dev(None, 64, 16, 64, 64, 1, 16, 16, P.FLAG_FFMPEG, P.PIX_RGB24, 64, 48, 64, None) == P.ERR_ARG
