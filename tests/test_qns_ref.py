"""No-GPU checks of the video encoder's quantizer noise shaping: the Python restatement (tests/qns_ref.py) in reference mode
against levels the reference's own dct_quantize_refine gave (tests/golden/ref_qns.json, made by
tests/golden/make_ref_qns_golden.py), the basis against the reference's own table, product mode's conditions, the HIP-free
arithmetic of amv_qns_plan.h against the model (tests/c/qns_plan_test.cc), and the entry points' declarations and bindings."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import nr_ref as N
import qns_ref as Q
import trellis_ref as T
from conftest import GOLDEN, ROOT

NAMES = ("amvhip_encode_qns_lambda2", "amvhip_encode_qns_lambda2_max", "amvhip_encode_qns_stream_dev", "amvhip_encode_yuv420_qns_stream_dev",
         "amvhip_encode_frontend_qns_stream_dev", "amvhip_encode_qns_coefs_dev")
HEADER = os.path.join(ROOT, "amv-codec-tools_amd", "csrc", "amv_qns_plan.h")


# ---- reference mode against the fixture ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(GOLDEN, "ref_qns.json")))


def reference_case(case, length, **variant):
    """the fixture's seeded sample blocks through refine_block_reference -> [blocks, 65]: levels, last_non_zero"""
    rng = np.random.default_rng(case["seed"])
    out = []
    for b in range(case["blocks"]):
        levels, last = Q.refine_block_reference(T.reference_samples(rng, case["kind"]), case["qscale"], case["lambda2"], case["qns"], length, length,
                                                **variant)
        out.append(levels + [last])
    return np.array(out, np.int16)


def case_hash(case, length, **variant):
    try:
        return "%016x" % N.fnv1a64(reference_case(case, length, **variant).astype("<i2").tobytes())
    except AssertionError:                       # a model without a rule may leave the ranges the model asserts
        return "out of range"


def test_reference_mode_reproduces_the_fixture(golden):
    length, _ = T.jpeg_uni_ac_lengths(0)
    assert "%016x" % N.fnv1a64(bytes(length)) == golden["length_table"]
    assert len(golden["cases"]) >= 12 and {c["qns"] for c in golden["cases"]} == {1, 2, 3}
    assert any(c["lambda2"] == 0 for c in golden["cases"]) and any(c["lambda2"] == 6962 for c in golden["cases"])
    for case in golden["cases"]:
        assert case_hash(case, length) == case["levels"], case["name"]
    assert all(any(c["changed"] for c in golden["cases"] if c["qns"] == qns) for qns in (1, 2, 3))


def test_basis_is_the_references(golden):
    assert Q.basis_hash() == golden["basis"]
    assert Q.BASIS[0][0] == 8192 and Q.BASIS.min() >= -16384 and Q.BASIS.max() <= 16384


def test_fixture_tells_the_walks_rules_apart(golden):
    """what the maker recorded holds again: for every rule it marks as pinned by the reference, a walk without the rule gives
    other levels on the first case the maker lists for it -- so the hashes above pin the rule.  (The maker walked every case
    with every variant; that takes minutes, so here one case per rule is walked again.)"""
    length, _ = T.jpeg_uni_ac_lengths(0)
    assert set(golden["pinned_by"]) == {rule for rule, _ in Q.VARIANTS}
    for rule, variant in Q.VARIANTS:
        pinned = golden["pinned_by"][rule]
        assert pinned in ("reference", "restatement"), rule
        telling = [c for c in golden["cases"] if rule in c["tells_apart"]]
        assert bool(telling) == (pinned == "reference"), rule
        if telling:
            case = min(telling, key=lambda c: c["changed"])
            assert case_hash(case, length, **variant) != case["levels"], (rule, case["name"])


# ---- product mode ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def picture():
    """nr_ref.picture(48, 32, "texture", 7): its sample blocks (0 .. 255) and the plain quantiser's lines"""
    frame = N.picture(48, 32, "texture", 7)
    return N.frame_blocks(*frame, 48, 32, 0), N.quantize_product(T.frame_coefficients(*frame, 48, 32), 0)


def _weighted_error(p, levels, comp):
    """the score's distortion half, from scratch: the remainder of the levels, then try_8x8basis at no change"""
    w, _ = Q.shaped_weight(Q.visual_weight(p))
    q = Q.QUANT[comp]
    rem = int(levels[0]) * int(q[0]) * 8 + 32 - ((np.asarray(p, np.int64) - 128) << 6)
    for i in range(1, 64):
        if levels[i]:
            rem = Q.add_basis(rem, Q.BASIS_SCAN[i], int(levels[i]) * int(q[i]))
    return Q.try_scores(rem, w, Q.BASIS_SCAN[:1], [0])[0], w


@pytest.mark.parametrize("qns,lambda2", [(1, 6962), (2, 6962), (3, 0), (3, Q.LAMBDA2_MAX)])
def test_every_change_lowers_the_score(picture, qns, lambda2):
    """product mode on a picture's blocks: weighted error + lambda * ac_bits falls strictly with every change (so the walk
    ends), qns 1 never raises a magnitude, and the levels stay inside the gates"""
    p, zz = picture
    changed = 0
    for b in range(0, p.shape[0], 3):
        comp = 0 if b % 6 < 4 else 1
        start = [int(x) for x in zz[b]]
        trace = {}
        levels, changes = Q.qns_block(p[b], start, comp, qns, lambda2, trace=trace)
        assert changes < Q.ITERATIONS
        changed += changes
        before, w = _weighted_error(p[b], start, comp)
        lam = (int((w * w).sum()) * lambda2) >> 19
        walked, error = list(start), before
        for i, change, _, level_before, _, base, best, bits in trace.get("picks", []):
            # the walk's own error (its remainder carries add_8x8basis's rounding of every step, so it is not the error of
            # the levels taken from scratch): what it started the iteration from is what the change before left, the change
            # wins strictly, and its bits are the difference of the whole block's AC lengths
            assert walked[i] == level_before and base == error and best < base, (b, i, change)
            bits_before = Q.ac_bits(walked, comp)
            walked[i] += change
            assert bits == (Q.ac_bits(walked, comp) - bits_before if i else 0), (b, i, change)
            error = best - bits * lam
        assert walked == levels
        if qns == 1:
            assert all(abs(a) <= abs(s) for a, s in zip(levels[1:], start[1:]))
        assert all(abs(levels[i] * int(Q.QUANT[comp][i])) < 2048 for i in range(1, 64))
    assert changed > 0


def test_qns_0_and_the_cap(picture):
    p, zz = picture
    frames_lines = Q.refine_lines([N.picture(48, 32, "texture", 7)], 48, 32, [zz], 0, 6962)
    assert (frames_lines[0] == zz).all()
    b = next(b for b in range(p.shape[0]) if Q.qns_block(p[b], zz[b], 0 if b % 6 < 4 else 1, 3, 0)[1] > 4)
    trace = {}
    capped, changes = Q.qns_block(p[b], zz[b], 0 if b % 6 < 4 else 1, 3, 0, cap=3, trace=trace)
    assert changes == 3 and len(trace["picks"]) == 3
    assert capped != Q.qns_block(p[b], zz[b], 0 if b % 6 < 4 else 1, 3, 0)[0]


def test_lambda2_constants():
    assert Q.lambda2_of_qscale(8) == 6962
    text = open(HEADER).read()
    assert re.search(r"kQnsIterations = %d;" % Q.ITERATIONS, text) and re.search(r"kQnsChangesSeen = %d;" % Q.CHANGES_SEEN, text)
    assert Q.ITERATIONS > 4 * Q.CHANGES_SEEN >= Q.ITERATIONS // 2 and Q.ITERATIONS & (Q.ITERATIONS - 1) == 0


def test_the_cap_is_four_times_the_measured_most():
    """a sample of the measurement behind kQnsChangesSeen (python tests/qns_ref.py walks all 20 000 seeded blocks): no block
    of the sample takes more changes than the header says were seen"""
    assert Q.seeded_changes(0, 64) <= Q.CHANGES_SEEN


# ---- amv_qns_plan.h ------------------------------------------------------------------------------------------------------------

def _ints(a):
    return " ".join(str(int(x)) for x in np.asarray(a).reshape(-1))


def _vectors(picture):
    p, zz = picture
    lines = ["B %s" % _ints(Q.BASIS)]
    for b in range(0, p.shape[0], 2):
        comp = 0 if b % 6 < 4 else 1
        for qns, lambda2, cap in ((1, 6962, Q.ITERATIONS), (2, 6962, Q.ITERATIONS), (3, 0, Q.ITERATIONS), (3, Q.LAMBDA2_MAX, Q.ITERATIONS), (3, 0, 3)):
            levels, changes = Q.qns_block(p[b], zz[b], comp, qns, lambda2, cap)
            lines.append("R %d %d %d %d %s %s %s %d" % (comp, qns, lambda2, cap, _ints(p[b]), _ints(zz[b]), _ints(levels), changes))
    return "\n".join(lines) + "\n"


def test_host_arithmetic(tmp_path, picture):
    """qns_block, the basis and the bounds of amv_qns_plan.h, walked by tests/c/qns_plan_test.cc under the address and
    undefined-behaviour sanitizers, on vectors the model writes -- the same blocks once more with a cap of 3"""
    exe, vec = str(tmp_path / "qns_plan_test"), str(tmp_path / "vectors.txt")
    text = _vectors(picture)
    assert " 3 0 3 " in text
    open(vec, "w").write(text)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "amv-codec-tools_amd", "csrc"), os.path.join(ROOT, "tests", "c", "qns_plan_test.cc"), "-o", exe],
                   check=True)
    out = subprocess.run([exe, vec], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.splitlines()[-1].startswith("ok ") and not out.stderr, out.stdout + out.stderr
    assert int(out.stdout.split()[-1]) >= text.count("\n") + 200
    assert "lambda2 max %d\n" % Q.LAMBDA2_MAX in out.stdout


# ---- the entry points ----------------------------------------------------------------------------------------------------------

def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "amvhip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"^uint32_t\s+amvhip_encode_qns_lambda2_max\s*\(\s*void\s*\)\s*;", text, flags=re.M)
    assert re.search(r"^uint32_t\s+amvhip_encode_qns_lambda2\s*\(\s*uint32_t\s+qscale\s*\)\s*;", text, flags=re.M)
    for name in NAMES[2:]:
        assert re.search(r"^int\s+%s\s*\(\s*amvhip_ctx\s*\*\s*ctx\b[^;{]*\)\s*;" % name, text, flags=re.M), name
    for new, old in (("amvhip_encode_qns_stream_dev", "amvhip_encode_quant_psnr_stream_dev"),
                     ("amvhip_encode_yuv420_qns_stream_dev", "amvhip_encode_yuv420_quant_psnr_stream_dev"),
                     ("amvhip_encode_frontend_qns_stream_dev", "amvhip_encode_frontend_quant_psnr_stream_dev")):
        a = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % new, text).group(1)
        b = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % old, text).group(1)
        names = [x.split()[-1].lstrip("*") for x in a.split(",")]
        old_names = [x.split()[-1].lstrip("*") for x in b.split(",")]
        at = old_names.index("q") + 1
        assert names == old_names[:at] + ["qns", "lambda2"] + old_names[at:], new


def test_library_exports_them(pkg):
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in NAMES:
        assert name in exported, name
    data = open(pkg.LIB_PATH, "rb").read()
    for kernel in (b"amv_qns_refine_kernelILb0E", b"amv_qns_refine_kernelILb1E"):
        assert kernel in data, kernel


def test_binding_has_them(pkg):
    for name in NAMES:
        assert name in pkg.SYMBOLS, name
    for new, old in (("amvhip_encode_qns_stream_dev", "amvhip_encode_quant_psnr_stream_dev"),
                     ("amvhip_encode_yuv420_qns_stream_dev", "amvhip_encode_yuv420_quant_psnr_stream_dev"),
                     ("amvhip_encode_frontend_qns_stream_dev", "amvhip_encode_frontend_quant_psnr_stream_dev")):
        assert len(pkg.SYMBOLS[new][1]) == len(pkg.SYMBOLS[old][1]) + 2, new
    for method in ("encode_qns_lambda2_max", "encode_qns_lambda2", "encode_qns_stream_dev", "encode_yuv420_qns_stream_dev",
                   "encode_frontend_qns_stream_dev", "encode_qns_coefs_dev"):
        assert callable(getattr(pkg.Context, method)), method


def test_lambda2_functions_and_null_context(pkg):
    lib = pkg.load_library()
    assert lib.amvhip_encode_qns_lambda2_max() == Q.LAMBDA2_MAX
    for q in (1, 2, 8, 31, 99):
        assert lib.amvhip_encode_qns_lambda2(q) == Q.lambda2_of_qscale(q)
    assert lib.amvhip_encode_qns_lambda2(8) == 6962
    too_big = next(q for q in range(1, 1 << 16) if Q.lambda2_of_qscale(q) > Q.LAMBDA2_MAX)
    assert lib.amvhip_encode_qns_lambda2(too_big) == 0 and lib.amvhip_encode_qns_lambda2(too_big - 1) == Q.lambda2_of_qscale(too_big - 1)
    assert lib.amvhip_encode_qns_lambda2(0) == 0 and lib.amvhip_encode_qns_lambda2(0xFFFFFFFF) == 0
    buf = (ctypes.c_uint8 * 512)(*([0xEE] * 512))
    p = ctypes.addressof(buf)
    assert lib.amvhip_encode_yuv420_qns_stream_dev(None, p, p, p, 16, 8, 384, 384, 1, 16, 16, p, 1, 6962, p, 64, p, p, None, None) == pkg.ERR_ARG
    assert lib.amvhip_encode_qns_stream_dev(None, p, 48, 0, 1, 16, 16, p, 1, 6962, p, 64, p, p, None, None) == pkg.ERR_ARG
    assert lib.amvhip_encode_qns_coefs_dev(None, p, 48, 0, 1, 16, 16, p, 1, 6962, p, None) == pkg.ERR_ARG
    assert bytes(buf) == b"\xee" * 512
