"""No-GPU checks of the video front end (deinterlace, crop, pad around the sws_scale shim): the CPU restatement in
frontend_ref.py against outputs of the real reference's command line (tests/golden/ref_frontend.json, made by
tests/golden/make_ref_frontend_golden.py), the restatement against itself in its other forms, the plan's arithmetic walked by
tests/c/frontend_plan_test.cc, and what the new entry points answer before they touch a device."""
import ctypes
import importlib.util
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import frontend_ref as F
import img_convert_ref as R

FIXTURE = json.load(open(os.path.join(GOLDEN, "ref_frontend.json")))["cases"]
FMT = {name: i for i, name in enumerate(R.NAMES)}
NEW_SYMBOLS = ("amvhip_pad_color_from_rgb", "amvhip_deinterlace_supported", "amvhip_deinterlace_dev", "amvhip_deinterlace",
               "amvhip_video_frontend_dev", "amvhip_encode_frontend_batch_dev")


def case_inputs(c):
    (sw, sh), src = c["src_size"], FMT[c["src"]]
    return [R.make_picture(src, sw, sh, c["input"]["kind"], c["input"]["seed"] + i) for i in range(c["frames"])]


def case_color(c):
    return F.pad_color_from_rgb(int(c["padcolor"], 16)) if c["padcolor"] else F.DEFAULT_COLOR


def restated(c, orc):
    (sw, sh), (dw, dh) = c["src_size"], c["dst_size"]
    return [F.frontend(FMT[c["src"]], p, sw, sh, dw, dh, orc.img_resample_yuv420, c["deinterlace"], tuple(c["crop"]), tuple(c["pad"]), case_color(c))
            for p in case_inputs(c)]


def test_fixture_covers_what_it_should():
    pinned = [c for c in FIXTURE if c["pinned_by"] == "reference"]
    alone = {(c["src"], tuple(c["src_size"])) for c in pinned if c["deinterlace"] and not any(c["crop"]) and not any(c["pad"])}
    assert alone >= {(f, s) for f in ("yuv420p", "yuv422p", "yuv444p") for s in ((48, 32), (36, 8))} | {("yuvj420p", (48, 32)), ("rgb24", (48, 32))}
    for color in (None, "336699"):
        pads = {tuple(c["pad"]) for c in pinned if c["padcolor"] == color and any(c["pad"]) and not any(c["crop"])}
        assert sum(1 for p in pads if sum(1 for v in p if v) == 1) == 4 and any(all(p) for p in pads)
    assert any(any(c["crop"]) and not any(c["pad"]) and not c["deinterlace"] for c in pinned)
    chains = [c for c in pinned if c["chain"]]
    assert {c["deinterlace"] for c in chains} == {True, False}
    assert all(c["src_size"] == [352, 288] and c["dst_size"] == [160, 120] and any(c["crop"]) and any(c["pad"]) for c in chains)
    assert any(c["src"] == "yuvj420p" and any(c["pad"]) and not any(c["crop"]) and c["inner_size"] is None for c in pinned)     # the copy route
    # crop + pad without a rescale is the corner where the reference is not a function of its input: not pinned at all
    assert not any(any(c["crop"]) and any(c["pad"]) and c["inner_size"] is None for c in FIXTURE)
    # what the real reference did not pin: the crop it refuses
    for c in FIXTURE:
        if c["pinned_by"] != "reference":
            assert c["src"] == "yuyv422" and any(c["crop"])
    assert os.path.getsize(os.path.join(GOLDEN, "ref_frontend.json")) < 256 * 1024


@pytest.mark.parametrize("i", range(len(FIXTURE)))
def test_restatement_reproduces_the_reference(i, orc):
    c = FIXTURE[i]
    if c["pinned_by"] != "reference":
        with pytest.raises(ValueError, match="av_picture_crop refuses"):
            restated(c, orc)
        return
    frames = restated(c, orc)
    dw, dh = c["dst_size"]
    assert [[row.tolist() for row in p[:2]] for p in frames[0]] == c["rows"][0], (c["src"], c["src_size"], c["crop"], c["pad"])
    assert ["%016x" % R.fnv1a64(R.join(f)) for f in frames] == c["fnv"], (c["src"], c["src_size"], c["crop"], c["pad"])
    assert all(R.join(f).size == R.frame_bytes(R.YUVJ420P, dw, dh) for f in frames)


def test_a_refused_deinterlace_is_no_deinterlace():
    """ffmpeg.c:602-608: the pinned outputs with -deinterlace on yuvj420p and rgb24 are those without it"""
    for src in ("yuvj420p", "rgb24"):
        on, off = ([c for c in FIXTURE if c["src"] == src and c["deinterlace"] == d and not any(c["crop"]) and not any(c["pad"])] for d in (True, False))
        assert len(on) == 1 and len(off) == 1 and on[0]["pinned_by"] == off[0]["pinned_by"] == "reference"
        assert on[0]["input"] == off[0]["input"] and on[0]["fnv"] == off[0]["fnv"] and on[0]["rows"] == off[0]["rows"]
        assert not F.deinterlace_supported(FMT[src], 48, 32)
    # ... and where the routine does run, the picture changes
    on, off = ([c for c in FIXTURE if c["chain"] and c["src"] == "yuv420p" and c["input"]["kind"] == "noise" and c["deinterlace"] == d] for d in (True, False))
    assert on[0]["input"] == off[0]["input"] and on[0]["fnv"] != off[0]["fnv"]


def test_fixture_is_what_the_reference_makes(tmp_path):
    """tests/golden/ref_frontend.json is made again from the reference tree and must equal the committed file; skipped where
    the reference tree is not at hand (AMV_REFERENCE; AMV_REF_FFMPEG names a reference ffmpeg built earlier)"""
    spec = importlib.util.spec_from_file_location("make_ref_frontend_golden", os.path.join(GOLDEN, "make_ref_frontend_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    reference = os.environ.get("AMV_REFERENCE", "/root/reference")
    ffmpeg = os.environ.get("AMV_REF_FFMPEG")
    if not ffmpeg and not os.path.isdir(os.path.join(reference, "AMVmuxer", "ffmpeg")):
        pytest.skip("the reference tree is not here")
    out = str(tmp_path / "ref_frontend.json")
    cmd = ["python3", os.path.join(GOLDEN, "make_ref_frontend_golden.py"), "--reference", reference, "--out", out, "--jobs", "8"]
    subprocess.run(cmd + (["--ffmpeg", ffmpeg] if ffmpeg else []), check=True, capture_output=True)
    assert json.load(open(out)) == json.load(open(os.path.join(GOLDEN, "ref_frontend.json")))


def _pictures():
    for fmt in F.DEINTERLACED:
        for (w, h) in ((4, 4), (8, 8), (36, 8), (48, 32), (16, 12)):
            for kind in ("noise", "zeros", "ones", "ramp"):
                yield fmt, w, h, R.make_picture(fmt, w, h, kind, 17 * fmt + w)


def test_in_place_and_out_of_place_deinterlace_agree():
    for fmt, w, h, pic in _pictures():
        a, b = F.deinterlace(fmt, pic, w, h), F.deinterlace(fmt, pic, w, h, inplace=True)
        assert all((x == y).all() for x, y in zip(a, b)), (R.NAMES[fmt], w, h)
        assert all((x[0::2] == p[0::2]).all() for x, p in zip(a, pic))               # the top field is copied
    # the taps, by hand: rows 10 20 30 40 -> row 1 = (-10 + 40 + 40 + 120 - 40 + 4) >> 3 = 19, row 3 = (-20 + 120 + 80 + 160 - 40 + 4) >> 3 = 38
    p = np.repeat(np.array([[10], [20], [30], [40]], np.uint8), 4, axis=1)
    assert F.deinterlace_plane(p)[:, 0].tolist() == [10, 19, 30, 38] == F.deinterlace_plane_inplace(p)[:, 0].tolist()
    # the clamps: row 3 of 255 0 255 255 255 0 .. sums to 2550 (+ 4 >> 3 = 319), of the inverse to -510 (+ 4 >> 3 = -64, floor)
    hi = np.repeat(np.array([[255], [0], [255], [255], [255], [0], [255], [255]], np.uint8), 4, axis=1)
    assert F.deinterlace_plane(hi)[3, 0] == 255 and (4 * 255 + 2 * 255 + 4 * 255 + 4) >> 3 == 319
    assert F.deinterlace_plane(255 - hi)[3, 0] == 0 and (-255 - 255 + 4) >> 3 == -64
    # the arithmetic shift: sum + 4 of -1 and of -8 is -1 after >> 3 (a truncating division would give 0 and -1)
    for outer, want in ((5, -1), (12, -8)):
        p = np.repeat(np.array([[0], [outer], [0], [0], [0], [0], [0], [0]], np.uint8), 4, axis=1)
        assert -outer + 4 == want and want >> 3 == -1 and F.deinterlace_plane(p)[3, 0] == 0


def test_deinterlace_then_crop_is_the_windowed_form():
    """every even crop 0 .. 6 on 16 x 12: the rows and columns kept of the deinterlaced full picture == the window computed
    alone with the rules taken from the full picture's row index"""
    bands = [(t, b, l, r) for t in (0, 2, 4, 6) for b in (0, 2, 4, 6) for l in (0, 2, 4, 6) for r in (0, 2, 4, 6)]
    for fmt in (R.YUV420P, R.YUV422P, R.YUV444P):
        pic = R.make_picture(fmt, 16, 12, "noise", 3 + fmt)
        full = F.deinterlace(fmt, pic, 16, 12)
        for band in bands:
            if band[0] + band[1] > 10:
                continue
            want, cw, ch = F.crop(fmt, full, 16, 12, band)
            got = F.deinterlace_window(fmt, pic, 16, 12, band)
            assert (cw, ch) == (16 - band[2] - band[3], 12 - band[0] - band[1])
            assert all(g.shape == w.shape and (g == w).all() for g, w in zip(got, want)), (R.NAMES[fmt], band)


def test_pad_and_crop_restatements():
    win = [np.full((2, 2), 9, np.uint8), np.full((1, 1), 8, np.uint8), np.full((1, 1), 7, np.uint8)]
    out = F.pad(win, 6, 6, (2, 2, 2, 2), (1, 254, 77))
    assert out[0].shape == (6, 6) and out[1].shape == (3, 3)
    assert (out[0][2:4, 2:4] == 9).all() and out[0].sum() == 4 * 9 + 32 * 1 and out[1][1, 1] == 8 and out[1].sum() == 8 + 8 * 254
    assert out[2].tolist() == [[77, 77, 77], [77, 7, 77], [77, 77, 77]]
    with pytest.raises(ValueError):
        F.crop(R.YUYV422, R.make_picture(R.YUYV422, 8, 8, "noise"), 8, 8, (2, 0, 0, 0))
    pic = R.make_picture(R.YUV420P, 8, 8, "noise", 1)
    got, w, h = F.crop(R.YUV420P, pic, 8, 8, (2, 0, 4, 0))
    assert (w, h) == (4, 6) and (got[0] == pic[0][2:, 4:]).all() and (got[1] == pic[1][1:, 2:]).all()


def test_pad_color_from_rgb_everywhere_on_a_grid(pkg):
    """a 17^3 grid of RGB values: the library and the restatement against the macros' arithmetic once more as plain integers
    (FIX(x) = round(1024 x): 306 601 117 / 173 339 512 / 512 429 83)"""
    grid = [min(16 * k, 255) for k in range(17)]
    for r in grid:
        for g in grid:
            for b in grid:
                want = ((306 * r + 601 * g + 117 * b + 512) >> 10, ((-173 * r - 339 * g + 512 * b + 511) >> 10) + 128,
                        ((512 * r - 429 * g - 83 * b + 511) >> 10) + 128)
                assert all(0 <= v <= 255 for v in want)
                rgb = (r << 16) | (g << 8) | b
                assert F.pad_color_from_rgb(rgb) == want == pkg.pad_color_from_rgb(rgb), (r, g, b)
    assert pkg.pad_color_from_rgb(0) == (0, 128, 128) and pkg.pad_color_from_rgb(0xFFFFFF) == (255, 128, 128)
    assert pkg.pad_color_from_rgb(0x336699) == F.pad_color_from_rgb(0x336699)


def test_frontend_plan_arithmetic(tmp_path):
    """tests/c/frontend_plan_test.cc: the plan's rectangles against painted byte maps, a stand-alone program under the address
    and undefined-behaviour sanitizers"""
    exe = str(tmp_path / "frontend_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "amv-codec-tools_amd", "csrc"), os.path.join(ROOT, "tests", "c", "frontend_plan_test.cc"), "-o", exe],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().splitlines()[-1] == "ok 163593", out.stdout + out.stderr


def test_new_entry_points_are_exported(pkg):
    lib = pkg.load_library()
    for name in NEW_SYMBOLS:
        assert name in pkg.SYMBOLS and getattr(lib, name) is not None
    exported = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in exported.splitlines() if line.strip()}
    assert set(NEW_SYMBOLS) <= names
    assert pkg.K_PIXFMT == 12 and lib.amvhip_kernel_name(13) in (None, b"")          # no kernel id was added
    # the struct as the header declares it: nine 32-bit words, three bytes, padded to a multiple of four
    S = pkg.Frontend
    assert ctypes.sizeof(S) == 40 and S.pad_color.offset == 36 and S.pad_color.size == 3
    assert [getattr(S, n).offset for n, _ in S._fields_[:9]] == list(range(0, 36, 4))
    fe = S(1, (2, 4, 6, 8), (10, 12, 14, 16), (1, 2, 3))
    assert (fe.deinterlace, fe.crop_top, fe.crop_bottom, fe.crop_left, fe.crop_right) == (1, 2, 4, 6, 8)
    assert (fe.pad_top, fe.pad_bottom, fe.pad_left, fe.pad_right, tuple(fe.pad_color)) == (10, 12, 14, 16, (1, 2, 3))
    assert tuple(S().pad_color) == (16, 128, 128)
    # the deinterlacer's list, without a device
    for fmt in range(-1, 15):
        for w, h in ((48, 32), (4, 4), (36, 8), (6, 4), (4, 6), (0, 4), (16388, 4)):
            want = fmt in F.DEINTERLACED and F.deinterlace_supported(fmt, w, h) and w <= 16384
            assert bool(lib.amvhip_deinterlace_supported(fmt, w, h)) == bool(want), (fmt, w, h)


def test_entry_points_refuse_a_null_context(pkg):
    lib, P = pkg.load_library(), pkg
    pic = (64, 64, 64, 64, 32, 4096, 1024)
    assert lib.amvhip_deinterlace_dev(None, P.PIX_YUV420P, *pic, *pic, 16, 16, 1, None) == P.ERR_ARG
    assert lib.amvhip_deinterlace(None, P.PIX_YUV420P, *pic, *pic, 16, 16, 1) == P.ERR_ARG
    assert lib.amvhip_video_frontend_dev(None, P.PIX_YUV420P, *pic, 64, 64, 1, None, *pic, 32, 32, None) == P.ERR_ARG
    assert lib.amvhip_encode_frontend_batch_dev(None, P.PIX_YUV420P, *pic, 64, 64, 1, None, 32, 32, 0, 64, 4096, 64, 64, None) == P.ERR_ARG
