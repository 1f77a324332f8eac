"""The reduced-size decode without a device: the numpy restatement (tests/lowres_ref.py) against what the reference's own
`ffmpeg -lowres L` made of JPEG stills (tests/golden/ref_lowres.json, written by tests/golden/make_ref_lowres_golden.py), the
geometry of amv_host_plan.h walked by tests/c/lowres_plan_test.cc, and what the new entry points answer before they touch
a device."""
import json
import os
import subprocess
import sys

import numpy as np

import lowres_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)


def test_restatement_reproduces_the_reference(pkg, orc):
    """every case of the fixture: the still is made again, its coefficients come from the oracle's entropy stage, the
    tables are the ones its header carries, the placement is the ordinary top-down one -- hash and rows as recorded"""
    import make_ref_lowres_golden as G
    doc = json.load(open(os.path.join(GOLDEN, "ref_lowres.json")))
    stills = {json.dumps(d, sort_keys=True): (w, h, chunk) for d, w, h, chunk in G.stills(pkg, orc)}
    assert len(doc["cases"]) == 3 * len(stills) >= 36
    seen = set()
    for case in doc["cases"]:
        assert case["pinned_by"] == "reference"
        key = json.dumps({k: case[k] for k in ("clip", "frame", "synth") if k in case}, sort_keys=True)
        w, h, chunk = stills[key]
        L = case["lowres"]
        assert [w, h] == case["size"]
        seen.add((key, L))
        nb = ((w + 15) // 16) * ((h + 15) // 16) * 6
        coef, st = orc.entropy_blocks(chunk, nb)
        assert st == 0 and len(coef) == nb, (case, st)
        tables = R.header_tables(G.still_bytes(pkg, w, h, chunk))
        planes = R.split(R.picture(coef, w, h, L, nb // 6, tables, flip=False), R.plane_sizes(w, h, L))
        # (the command line hands out the picture less an odd last column or row, and of an odd-sized output the last
        # chroma column or row is not the decoder's: make_ref_lowres_golden.py)
        ow, oh = case["out_size"]
        assert 0 <= R.dim(w, L) - ow <= 1 and 0 <= R.dim(h, L) - oh <= 1
        got = G.kept_planes(planes, ow, oh)
        for c, (g, rows) in enumerate(zip(got, case["rows"])):
            assert g[:2].tolist() == rows, "%s lowres %d plane %d: first rows differ" % (key, L, c)
        assert "%016x" % R.fnv1a64(np.concatenate([g.reshape(-1) for g in got])) == case["fnv"], "%s lowres %d" % (key, L)
    assert len(seen) == len(doc["cases"])


def test_the_four_branches_are_not_one_formula():
    """FIX_1_306562965 = 10703 against FIX_0_541196100 - FIX_1_847759065 = -10704: with d2 == 0, d6 != 0 the reference's
    branch and the general one differ by d6 before the descale; the restatement selects as the reference does"""
    assert R.FIX_1_306562965 == 10703 and R.FIX_0_541196100 - R.FIX_1_847759065 == -10704
    assert R.FIX_0_541196100 + R.FIX_0_765366865 == R.FIX_1_306562965        # (so the d6 == 0 branch IS the general one)
    d0, d6 = np.array([1028]), np.array([1022])
    zero = np.zeros(1, np.int64)
    assert int(R._even4(d0, zero, zero, d6)[1][0]) == (1028 << 13) - 1022 * 10703
    assert int(R._even4(d0, zero, zero, d6, folded=True)[1][0]) == (1028 << 13) - 1022 * 10704
    for d2 in (0, 7):       # the other three shapes agree with the general formula
        for v6 in (0, 5):
            if d2 or not v6:
                a = R._even4(d0, np.array([d2]), zero, np.array([v6]))
                b = R._even4(d0, np.array([d2]), zero, np.array([v6]), folded=True)
                assert all(int(x[0]) == int(y[0]) for x, y in zip(a, b))
    # blocks on which the difference reaches a pixel, in a row and in a column
    rng = np.random.default_rng(0x10703)
    for place in ((0, 3), (3, 0)):
        blk = np.zeros((4000, 8, 8), np.int64)
        blk[:, 0, 0] = rng.integers(0, 2040, 4000)
        blk[:, place[0], place[1]] = rng.integers(-2000, 2000, 4000)
        exact, other = np.clip(R.rev_dct4(blk), 0, 255), np.clip(R.rev_dct4(blk, folded=True), 0, 255)
        assert (exact != other).any(axis=(1, 2)).sum() > 10


def test_lowres_plan_arithmetic(tmp_path):
    """tests/c/lowres_plan_test.cc: the plan's geometry against brute force for every (w, h, lowres) with w, h <= 80, a
    stand-alone program under the address and undefined-behaviour sanitizers"""
    exe = str(tmp_path / "lowres_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "amv-codec-tools_amd", "csrc"), os.path.join(ROOT, "tests", "c", "lowres_plan_test.cc"), "-o", exe],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip().splitlines()[-1] == "ok %d" % (3 * 80 * 80), out.stdout + out.stderr


def test_geometry_helpers(pkg):
    lib = pkg.load_library()
    assert lib.amvhip_lowres_dim(129, 3) == 17 and lib.amvhip_lowres_dim(128, 3) == 16 and lib.amvhip_lowres_dim(1, 3) == 1
    assert lib.amvhip_lowres_dim(129, 4) == 0 and lib.amvhip_lowres_frame_bytes(160, 120, 4) == 0
    for w, h in ((160, 120), (130, 98), (336, 32), (37, 23), (16, 16), (1, 1)):
        for L in (1, 2, 3):
            assert lib.amvhip_lowres_dim(w, L) == R.dim(w, L) == -(-w // (1 << L))
            assert lib.amvhip_lowres_frame_bytes(w, h, L) == R.frame_bytes(w, h, L)
    assert lib.amvhip_lowres_frame_bytes(130, 98, 2) == 33 * 25 + 2 * 17 * 13
    assert lib.amvhip_lowres_dim(160, 0) == 160 and lib.amvhip_lowres_frame_bytes(160, 120, 0) == lib.amvhip_yuv420_frame_bytes(160, 120)


def test_entry_points_refuse_without_a_device(pkg):
    """no context: AMVHIP_ERR_ARG from every new entry point, whatever else is wrong with the call (tests/test_gpu_lowres.py
    asks the same of a live context, argument by argument)"""
    lib = pkg.load_library()
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data
    F, K, Y, RGB = pkg.FLAG_FFMPEG, pkg.FLAG_FFMPEG_KEEP, pkg.PIX_YUVJ420P, pkg.PIX_RGB24
    for flags, L, fmt, stride in ((F, 1, Y, 8), (F, 0, Y, 16), (F, 4, Y, 1), (0, 1, Y, 8), (pkg.FLAG_ZIGZAG_FIXED, 1, Y, 8), (F | K, 1, Y, 8),
                                  (F, 1, Y, 9), (F, 1, Y, 16), (F, 2, RGB, 3)):
        assert lib.amvhip_decode_lowres_batch_dev(None, p, 64, p, p, 1, 16, 16, flags, L, fmt, p, stride, p, None) == pkg.ERR_ARG
        assert lib.amvhip_decode_lowres_batch(None, p, 64, p, p, 1, 16, 16, flags, L, fmt, p, stride, p) == pkg.ERR_ARG
    for L in (0, 1, 4):
        assert lib.amvhip_reconstruct_lowres_dev(None, p, p, 1, 16, 16, L, p, None) == pkg.ERR_ARG
    assert not buf.any()
