"""No-GPU checks of `-psnr`: the restatement (tests/psnr_ref.py) pinned to the oracle's FFmpeg-compat decoder, its zero, the
host arithmetic of amv_host_plan.h through the library (ctypes) and on the CPU (tests/c/psnr_plan_test.cc), and the entry
points' declarations, exports and bindings."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, SEED
import psnr_ref as P

NAMES = ["amvhip_psnr_db", "amvhip_psnr_report", "amvhip_picture_sse_supported", "amvhip_picture_sse_dev", "amvhip_picture_sse",
         "amvhip_encode_quant_psnr_stream_dev", "amvhip_encode_yuv420_quant_psnr_stream_dev", "amvhip_encode_frontend_quant_psnr_stream_dev"]


@pytest.mark.parametrize("w,h", [(16, 16), (48, 32), (336, 32)])
def test_placement_is_the_ffmpeg_decoders(orc, w, h):
    """height % 16 == 0: the FFmpeg mode's flip is the exact one, so the routine with the Q60 tables must be
    amvo_decode_frame_ffmpeg's planes byte for byte -- scan, dequantisation, IDCT, block placement and the flip at once"""
    for t in range(2):
        chunk = orc.encode_frame(orc.synth_frame(SEED, 3 + t, w, h), w, h)
        want, status, ok = orc.decode_frame_ffmpeg(chunk, w, h)
        assert status == 0 and ok == orc.nmcu(w, h)
        for got, plane in zip(P.reconstruct(orc, chunk, w, h, q60=True), orc.yuv_planes(want, w, h)):
            assert got.shape == plane.shape and (got == plane).all(), np.argwhere(got != plane)[:4].tolist()
        # ... and the encoder's own tables give another picture
        assert any((a != b).any() for a, b in zip(P.reconstruct(orc, chunk, w, h), orc.yuv_planes(want, w, h)))


def test_tables_are_the_headers(orc):
    """the restatement's tables are the tests' own copy (coef_builder.py); the product's header states the same five, entry
    for entry, the oracle's Q60 tables agree, and the oracle's own quantiser -- a third statement of amvlib's steps -- divides
    by the same two: a coefficient of 8 * Q[k] * m at scan position k comes out as level m when it rounds to nearest (qbias
    128); at m = 60 a step that were off by one would give 59 or 61"""
    t, hdr = P.tables(), P.header_tables()
    assert sorted(t) == sorted(hdr)
    for name in t:
        assert t[name].shape == (64,) and (t[name] == hdr[name]).all(), name
    for chroma, name in ((0, "kQ60Luma"), (1, "kQ60Chroma")):
        q = np.zeros(64, np.uint8)
        orc.lib().amvo_q60_table(chroma, q.ctypes.data)
        assert (t[name] == q).all()
    assert sorted(t["kScanOfNatural"]) == list(range(64))
    natural_of_scan = np.argsort(t["kScanOfNatural"])
    for comp, name in ((0, "kQuantLuma"), (1, "kQuantChroma")):
        for m in (1, 60):
            dct = np.zeros(64, np.int16)
            dct[natural_of_scan] = 8 * t[name] * m                     # natural order in, as the fdct leaves it
            out = np.zeros(64, np.int16)
            orc.lib().amvo_quantize_block(dct.ctypes.data, comp, 128, out.ctypes.data)
            assert (out == m).all(), (name, m, out.tolist())


@pytest.mark.parametrize("w,h", [(2, 2), (16, 16), (18, 34), (160, 120)])
def test_flat_128_is_exact(orc, w, h):
    planes = (np.full((h, w), 128, np.uint8), np.full((h // 2, w // 2), 128, np.uint8), np.full((h // 2, w // 2), 128, np.uint8))
    chunk = orc.encode_frame_yuv(*planes, w, h)
    assert P.sse(orc, chunk, planes, w, h) == [0, 0, 0]
    # a picture that is not flat has an error, and only the visible samples count: the sum is bounded by them
    noisy = tuple(np.random.default_rng(w).integers(0, 256, p.shape).astype(np.uint8) for p in planes)
    got = P.sse(orc, orc.encode_frame_yuv(*noisy, w, h), noisy, w, h)
    assert 0 < got[0] <= 65025 * w * h and all(0 < e <= 65025 * (w // 2) * (h // 2) for e in got[1:])


def test_rgb_sources_use_the_fused_conversion(orc):
    """the handed picture of an RGB chunk is rgb24_to_yuvj420p's: the oracle's RGB encoder and its YUV encoder on those planes
    write the same chunk, so the error is one number"""
    import pixel_builder as pb
    w, h = 18, 34
    pix = np.random.default_rng(5).integers(0, 256, (h, w, 3)).astype(np.uint8)
    for bgr in (0, 1):
        planes = pb.to_planes(orc, pix, w, h, bgr)
        chunk = orc.encode_frame(pix, w, h, bgr=bool(bgr))
        assert chunk == orc.encode_frame_yuv(*planes, w, h)
        assert all(e > 0 for e in P.sse(orc, chunk, planes, w, h))


def test_psnr_arithmetic_through_the_library(pkg):
    for sse, samples in ((1, 1), (7, 4), (65025, 19200), (123456789, 76800), (4261478400, 65536), (2 ** 40, 2 ** 32)):
        assert abs(pkg.psnr_db(sse, samples) - -10 * math.log10(sse / (samples * 255.0 * 255.0))) <= 1e-9
    assert pkg.psnr_db(0, 100) == math.inf and math.isnan(pkg.psnr_db(3, 0))
    w, h, n = 160, 120, 5
    rng = np.random.default_rng(2)
    sse = rng.integers(1, 2 ** 33, (n, 3)).astype(np.uint64)
    got = pkg.psnr_report(sse, w, h)
    scale = w * h * 255.0 * 255.0 * n
    sums = [int(sse[:, p].astype(object).sum()) for p in range(3)]
    want = [-10 * math.log10(sums[0] / scale), -10 * math.log10(sums[1] / (scale / 4)), -10 * math.log10(sums[2] / (scale / 4)),
            -10 * math.log10(sum(sums) / (scale * 1.5))]
    assert all(abs(a - b) <= 1e-9 for a, b in zip(got, want)), (got, want)
    assert pkg.psnr_report(np.zeros((3, 3), np.uint64), w, h) == (math.inf,) * 4
    # the -vstats figure is the report's luma entry of one frame
    assert pkg.psnr_report(sse[1:2], w, h)[0] == pkg.psnr_db(int(sse[1, 0]), w * h)


def test_picture_sse_supported_over_every_format(pkg):
    taken = {pkg.PIX_YUV420P, pkg.PIX_YUVJ420P, pkg.PIX_YUV422P, pkg.PIX_YUVJ422P, pkg.PIX_YUV444P, pkg.PIX_YUVJ444P, pkg.PIX_GRAY8,
             pkg.PIX_RGB24, pkg.PIX_BGR24}
    assert pkg.PIX_COUNT == 14
    for fmt in range(-1, pkg.PIX_COUNT + 1):
        assert bool(pkg.picture_sse_supported(fmt, 17, 9)) == (fmt in taken), fmt
        assert bool(pkg.picture_sse_supported(fmt, 16384, 4)) == (fmt in taken), fmt
        assert not pkg.picture_sse_supported(fmt, 0, 9) and not pkg.picture_sse_supported(fmt, 17, 16385)


def test_host_arithmetic(tmp_path):
    """psnr_db, psnr_report and picture_sse_ok of amv_host_plan.h, walked by tests/c/psnr_plan_test.cc under the address and
    undefined-behaviour sanitizers"""
    exe = str(tmp_path / "psnr_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "amv-codec-tools_amd", "csrc"), os.path.join(ROOT, "tests", "c", "psnr_plan_test.cc"), "-o", exe],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok ") and not out.stderr, out.stdout + out.stderr
    assert int(out.stdout.split()[1]) >= 48 + 11 + 16


def test_declared_exported_and_bound(pkg):
    text = open(os.path.join(ROOT, "include", "amvhip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in exported and name in pkg.SYMBOLS, name
    # no kernel id was added for them: the SSE kernel is timed as pixel-format work, the error kernel as forward-DCT work
    assert "#define AMVHIP_K_COUNT 13" in text

