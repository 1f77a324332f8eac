"""No-GPU checks of the postprocessing: the Python restatement (tests/pp_ref.py) against plane hashes and parsed modes of the
reference's own pp_postprocess / pp_get_mode_by_name_and_quality (tests/golden/ref_postprocess.json, made by
tests/golden/make_ref_postprocess_golden.py), the HIP-free arithmetic of amv_pp_plan.h in the kernel's order against the
reference's loop order and against the fixture (tests/c/pp_plan_test.cc, plain and under the sanitizers as a stand-alone
program), named faults the fixture must tell from the real thing, and the library's own mode parser."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import pp_builder as B
import pp_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = json.load(open(os.path.join(GOLDEN, "ref_postprocess.json")))


@pytest.fixture(scope="module")
def pictures(orc):
    aw, ah, amv = B.amv1_frames(orc, GOLDEN)
    out = {}
    for case in FIXTURE["cases"]:
        if case["kind"].startswith("amv1:"):
            assert (case["width"], case["height"]) == (aw, ah)
            out[case["name"]] = amv[int(case["kind"][5:])]
        else:
            out[case["name"]] = B.picture(case["width"], case["height"], case["kind"], case["seed"], B.case_qp(case["mode"]))
    return out


def test_fixture_matches_the_builder():
    recipes = B.cases()
    assert [c["name"] for c in FIXTURE["cases"]] == [r[0] for r in recipes]
    for c, r in zip(FIXTURE["cases"], recipes):
        assert (c["kind"], c["seed"], c["mode"], c["quality"]) == (r[3], r[4], r[5], r[6])
    sizes = {(c["width"], c["height"]) for c in FIXTURE["cases"]}
    assert set(B.SIZES) | set(B.NARROW) | {(320, 240)} <= sizes


def test_restatement_reproduces_every_hash_and_mode(pictures):
    for case in FIXTURE["cases"]:
        m = P.parse_mode(case["mode"], case["quality"])
        assert m == case["parsed"], case["name"]
        assert case["qp"] == (m["forcedQuant"] if m["lumMode"] & P.FORCE_QUANT else 1)
        got = P.postprocess(pictures[case["name"]], case["width"], case["height"], m)
        assert ["%016x" % P.fnv1a64(p.tobytes()) for p in got] == case["fnv"], case["name"]
    for r in FIXTURE["refused"]:
        assert P.parse_mode(r["mode"], 6) is None, r["mode"]


def test_restatement_is_a_function_of_the_picture(pictures):
    """what the maker checks on the real function, on the restatement: the destination's bytes and a used context do not
    matter -- and dering without a vertical deblock is the mode where they do (the entries refuse it)"""
    case = next(c for c in FIXTURE["cases"] if c["name"].startswith("48x40_crafted_hb:c,vb:c,dr:c"))
    pic, w, h = pictures[case["name"]], case["width"], case["height"]
    m = P.parse_mode(case["mode"], 6)
    used = P.Context(w)
    P.postprocess(B.picture(w, h, "noise", 5), w, h, m, ctx=used)
    a, b, c = P.postprocess(pic, w, h, m, prefill=0), P.postprocess(pic, w, h, m, prefill=255), P.postprocess(pic, w, h, m, ctx=used, prefill=0x55)
    assert all((x == y).all() and (x == z).all() for x, y, z in zip(a, b, c))
    m = P.parse_mode("dr:c,fq:12", 6)
    differ = False
    for seed in range(12):
        pic = B.picture(w, h, "crafted", seed, 12)
        differ |= any((x != y).any() for x, y in zip(P.postprocess(pic, w, h, m, prefill=0), P.postprocess(pic, w, h, m, prefill=255)))
    assert differ


@pytest.mark.parametrize("fault", P.FAULTS)
def test_named_fault_changes_an_expected_plane(pictures, fault):
    for case in FIXTURE["cases"]:
        if case["width"] > 160:
            continue
        got = P.postprocess(pictures[case["name"]], case["width"], case["height"], case["parsed"], faults=(fault,))
        if ["%016x" % P.fnv1a64(p.tobytes()) for p in got] != case["fnv"]:
            return
    raise AssertionError("no case tells %s from the reference" % fault)


def _build(tmp_path, name, extra):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall"] + extra + ["-I", os.path.join(ROOT, "amv-codec-tools_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", "pp_plan_test.cc"), "-o", exe], check=True)
    return exe


def test_plan_header_both_orders_equal_the_fixture(tmp_path, pictures):
    """amv_pp_plan.h: the kernel's order == the reference's loop order == the fixture, plain and under the address and
    undefined-behaviour sanitizers (a stand-alone program)"""
    listing = str(tmp_path / "cases.txt")
    with open(listing, "w") as f:
        for i, case in enumerate(FIXTURE["cases"]):
            path = str(tmp_path / ("pic%d.raw" % i))
            np.concatenate([p.reshape(-1) for p in pictures[case["name"]]]).tofile(path)
            m = case["parsed"]
            f.write("%d %d %d %d %d %d %d %d %s\n" % (i, case["width"], case["height"], m["lumMode"] & P.FILTER_BITS, m["chromMode"] & P.FILTER_BITS,
                                                     case["qp"], m["baseDcDiff"], m["flatnessThreshold"], path))
    for name, extra in (("pp_plan_test", []), ("pp_plan_test_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        out = subprocess.run([_build(tmp_path, name, extra), listing], capture_output=True, text=True)
        assert out.returncode == 0 and not out.stderr, out.stdout[-2000:] + out.stderr[-2000:]
        lines = out.stdout.splitlines()
        assert lines[-1] == "ok %d" % len(FIXTURE["cases"])
        assert lines[-2].startswith("further shapes ") and int(lines[-2].split()[-1]) >= 280       # the two orders on shapes beyond the fixture's
        for case, line in zip(FIXTURE["cases"], lines):
            assert line.split()[1:] == case["fnv"], case["name"]


PARSER_CASES = [("de", 6), ("de", 5), ("de", 4), ("de", 3), ("de", 2), ("de", 1), ("de", 0), ("default", 6), ("hb", 6), ("hdeblock:a", 0), ("vb:c", 6),
                ("vdeblock:y", 6), ("dr", 6), ("dering:a:c", 5), ("hb:c:64:20,vb:c,fq:3", 6), ("hb:0x40:010", 6), ("vb:-5:+7", 6), ("hb:n,vb", 6),
                ("fq", 6), ("forcequant:31", 6), ("fq:63,de", 6), ("de,-dr", 6), ("de/-hb/-vb", 6), ("hb,-hb", 6), ("de:c,fq:12", 6), ("hb:a:c", 2),
                ("hb:1:2:3", 6), ("hb:zz", 6), ("fq:1:2", 6), ("dr:3", 6), ("", 6), (",", 6), ("nosuch", 6), ("hb,nosuch", 6), ("de,,fq", 6)]
NOT_BUILT = ("h1", "x1hdeblock", "v1", "x1vdeblock", "ha", "ahdeblock", "va", "avdeblock", "al", "autolevels", "lb", "li", "ci", "md", "fd", "l5",
             "tn", "tmpnoise:1:2:3", "fa", "fast", "ac", "de,lb", "hb,tn")


def test_library_parser_is_the_restatement(pkg):
    """amvhip_pp_mode_parse == tests/pp_ref.parse_mode (which the fixture pins to the reference's parser) on every case of the
    fixture and on the option grammar; every filter and preset that is not built is AMVHIP_ERR_ARG, never dropped"""
    def parse(name, quality):
        mode = pkg.PpMode()
        rc = pkg.load_library().amvhip_pp_mode_parse(name.encode(), quality, ctypes.byref(mode))
        assert rc in (0, pkg.ERR_ARG)
        return None if rc else {"lumMode": mode.lum_mode, "chromMode": mode.chrom_mode, "baseDcDiff": mode.base_dc_diff,
                                "flatnessThreshold": mode.flatness_threshold, "forcedQuant": mode.forced_quant}
    for case in FIXTURE["cases"]:
        assert parse(case["mode"], case["quality"]) == case["parsed"], case["mode"]
    for name, quality in PARSER_CASES:
        assert parse(name, quality) == P.parse_mode(name, quality), (name, quality)
    assert parse("de", 6) == {"lumMode": 7, "chromMode": 7, "baseDcDiff": 32, "flatnessThreshold": 39, "forcedQuant": 0}
    assert parse("de", 4)["lumMode"] == 3 and parse("de", 4)["chromMode"] == 3 and parse("de", 2)["chromMode"] == 0
    for name in NOT_BUILT:
        assert parse(name, 6) is None and P.parse_mode(name, 6) is None, name
    assert pkg.load_library().amvhip_pp_mode_parse(None, 6, ctypes.byref(pkg.PpMode())) == pkg.ERR_ARG
    assert pkg.load_library().amvhip_pp_mode_parse(b"de", 6, None) == pkg.ERR_ARG
    assert parse("hb," * 200, 6) is None                          # longer than the reference's 500-byte buffer


def test_supported_sizes(pkg):
    lib = pkg.load_library()
    for w, h in B.SIZES + ((320, 240), (640, 480)):
        assert lib.amvhip_postprocess_supported(w, h) == 1, (w, h)
    for w, h in ((8, 16), (24, 16), (16, 8), (16, 17), (0, 0), (100, 100), (1 << 20, 16)):
        assert lib.amvhip_postprocess_supported(w, h) == 0, (w, h)


def test_library_and_binding_have_the_entries(pkg):
    names = ("amvhip_pp_mode_parse", "amvhip_postprocess_supported", "amvhip_postprocess_dev", "amvhip_postprocess", "amvhip_decode_pp_batch_dev")
    header = open(os.path.join(ROOT, "include", "amvhip.h")).read()
    lib = pkg.load_library()
    for name in names:
        assert name + "(" in header and name in pkg.SYMBOLS and getattr(lib, name), name
    assert len(pkg.SYMBOLS["amvhip_postprocess_dev"][1]) == len(pkg.SYMBOLS["amvhip_deinterlace_dev"][1]) + 2       # mode in front, d_qp before the stream
    assert len(pkg.SYMBOLS["amvhip_decode_pp_batch_dev"][1]) == len(pkg.SYMBOLS["amvhip_decode_fmt_batch_dev"][1]) + 2
    assert b"amv_postprocess_kernel" in open(pkg.LIB_PATH, "rb").read()
    for method in ("postprocess_supported", "postprocess_dev", "postprocess", "decode_pp_batch_dev"):
        assert callable(getattr(pkg.Context, method)), method
    assert ctypes.sizeof(pkg.PpMode) == 20 and (pkg.PP_V_DEBLOCK, pkg.PP_H_DEBLOCK, pkg.PP_DERING, pkg.PP_FORCE_QUANT) == (P.V_DEBLOCK, P.H_DEBLOCK, P.DERING, P.FORCE_QUANT)
    assert "AMVHIP_K_PIXFMT" in header[header.index("amvhip_decode_pp_batch_dev: arguments"):header.index("#define AMVHIP_PP_V_DEBLOCK")]
