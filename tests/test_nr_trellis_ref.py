"""tests/nr_trellis_ref.py, the restatement the -nr + trellis GPU tests compare against, held to what pins it: reference mode
against what the reference's own dct_quantize_trellis_c gave with noise reduction on (tests/golden/ref_nr_trellis.json, made
by tests/golden/make_ref_nr_trellis_golden.py), product mode against its two parents (nr_ref, trellis_ref), the HIP-free
arithmetic of amv_nr_plan.h + amv_trellis_plan.h against the model (tests/c/nr_trellis_plan_test.cc), and the entry points'
declarations and exports."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import nr_ref as N
import nr_trellis_ref as NT
import trellis_ref as T
from conftest import GOLDEN, ROOT

NAMES = ["amvhip_encode_yuv420_nr_trellis_stream_dev", "amvhip_encode_yuv420_nr_trellis_stream", "amvhip_encode_nr_trellis_stream_dev",
         "amvhip_encode_nr_trellis_stream", "amvhip_encode_frontend_quant_stream_dev"]
NR_NAMES = ["amvhip_encode_yuv420_nr_stream_dev", "amvhip_encode_yuv420_nr_stream", "amvhip_encode_nr_stream_dev", "amvhip_encode_nr_stream"]


# ---- reference mode against the fixture ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(GOLDEN, "ref_nr_trellis.json")))


def _model(case, length, esc_length, **variant):
    rng = np.random.default_rng(case["seed"])
    samples = [T.reference_samples(rng, case["kind"]) for _ in range(case["blocks"])]
    state, offsets = NT.reference_state(case["offsets_seed"])
    levels = NT.reference_blocks(samples, case["qscale"], case["lambda"], length, esc_length, state, offsets, **variant)
    return "%016x" % N.fnv1a64(levels.astype("<i2").tobytes()), "%016x" % N.fnv1a64(state.astype("<i4").tobytes())


def test_reference_mode_reproduces_the_fixture(golden):
    length, esc_length = T.jpeg_uni_ac_lengths(0)
    assert golden["esc_length"] == esc_length and "%016x" % N.fnv1a64(bytes(length)) == golden["length_table"]
    assert len(golden["cases"]) >= 8
    for case in golden["cases"]:
        assert _model(case, length, esc_length) == (case["levels"], case["error_sum"]), case["name"]


def test_fixture_tells_the_order_and_the_sums_apart(golden):
    """what the maker recorded holds again: a model that searches on the un-denoised outputs gives other levels, one that
    sums the denoised magnitudes other sums, on some case each -- so the hashes above pin both to the reference"""
    length, esc_length = T.jpeg_uni_ac_lengths(0)
    assert golden["pinned_by"] == {"search_on_denoised": "reference", "sums_before_offset": "reference"}
    case = next(c for c in golden["cases"] if len(c["tells_apart"]) == 2)
    levels, sums = _model(case, length, esc_length, search_undenoised=True)
    assert levels != case["levels"] and sums == case["error_sum"]
    levels, sums = _model(case, length, esc_length, sum_denoised=True)
    assert levels == case["levels"] and sums != case["error_sum"]


# ---- product mode against its parents -----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ramp():
    """48x32 x 6 "ramp", seed 100, at nr 3000 and lambda 3481: the chunks of both levers, and the state"""
    frames = N.stream(48, 32, ["ramp"] * 6, 100)
    state = N.new_state()
    return frames, NT.encode_stream(frames, 48, 32, 3000, 3481, state=state), state


def test_nr_0_is_the_trellis_entry(ramp):
    frames = ramp[0][:2]
    state = np.arange(65, dtype=np.int64) * 1000 + 7
    assert NT.encode_stream(frames, 48, 32, 0, 3481, state=state, qbias=40) == T.encode_frames(frames, 48, 32, 40, 3481)
    assert (state == np.arange(65) * 1000 + 7).all()


def test_state_is_that_of_nr_alone(ramp):
    """the sums are taken before the offset is applied: the state does not depend on the quantiser behind it"""
    frames, both, state = ramp
    alone_state = N.new_state()
    alone = N.encode_stream(frames, 48, 32, 3000, state=alone_state)
    assert (state == alone_state).all() and state[64] == 6 * 36
    assert all(a != b for a, b in zip(both, alone))


def test_the_two_levers_add_up(ramp):
    """both < either alone < plain, with the byte counts of the CPU run the combination was specified from; frame 0 starts
    from the all-zero state, so its offsets are 0 and its chunk is the trellis entry's -- every later chunk differs"""
    frames, both, _ = ramp
    trellis = T.encode_frames(frames, 48, 32, 0, 3481)
    sizes = [sum(len(c) for c in s) for s in (both, N.encode_stream(frames, 48, 32, 3000), trellis, N.encode_stream(frames, 48, 32, 0))]
    assert sizes == [1238, 1478, 1279, 1695]
    assert both[0] == trellis[0] and all(a != b for a, b in zip(both[1:], trellis[1:]))


def test_truncation_and_halving_reach_the_search():
    """the two corners of update_noise_reduction show in the chunks behind the search too: the uint16 store (nr 911 behind two
    flat frames: frame 2 differs from a model without it) and the halving (16x16 from a count of 65530: frame 3 differs)"""
    w, h = 48, 32
    frames = N.stream(w, h, ["flat", "flat"] + ["texture"] * 4, 300)
    want = NT.encode_stream(frames, w, h, 911, 3481)
    assert NT.encode_stream(frames, w, h, 911, 3481, truncate=False)[2] != want[2]
    rng = np.random.default_rng(3)
    state = np.concatenate([rng.integers(0, 16320 * 65530, 64), [65530]])
    state[:3] = (0, 7, 16320 * 65530)
    frames = N.stream(16, 16, ["texture", "ramp", "texture", "ramp"], 40)
    a, b = state.copy(), state.copy()
    want = NT.encode_stream(frames, 16, 16, 4000, 870, state=a)
    assert NT.encode_stream(frames, 16, 16, 4000, 870, state=b, halve=False)[3] != want[3]
    assert a[64] == 32783


# ---- the host arithmetic --------------------------------------------------------------------------------------------------------

def _ints(v):
    return " ".join(str(int(x)) for x in v)


def test_host_arithmetic(tmp_path):
    """nr_block then trellis_block on the blocks of a stream as the model walks them (state, offsets, outputs, levels), and
    denoised blocks at the edges of the bound on lambda in 64 bits, by tests/c/nr_trellis_plan_test.cc under the address and
    undefined-behaviour sanitizers"""
    w, h, nr = 48, 32, 3000
    lines = []
    state = N.new_state()
    for f, (y, cb, cr) in enumerate(N.stream(w, h, ["texture", "ramp", "noise"], 9)):
        coef = N.fdct(N.frame_blocks(y, cb, cr, w, h, 128))
        offsets = N.frame_start(state, nr)
        for b in range(0, coef.shape[0], 7):
            comp, qbias, lam = (0 if b % 6 < 4 else 1), (0, 128, 77)[b % 3], (3481, 0, T.LAMBDA_MAX)[(b + f) % 3]
            before = state.copy()
            den = N.denoise_blocks(state, offsets, coef[b:b + 1], N.DC_SHIFT)[0]
            c = den[T.ZIGZAG]
            lines.append("N %d %d %d %s %s %s %s %s" % (comp, qbias, lam, _ints(before), _ints(offsets), _ints(coef[b]), _ints(state),
                                                       _ints([c[0]] + T.trellis_block(c, comp, qbias, lam)[1:])))
    exe, vec = str(tmp_path / "nr_trellis_plan_test"), str(tmp_path / "vectors.txt")
    open(vec, "w").write("\n".join(lines) + "\n")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "amv-codec-tools_amd", "csrc"), "-I", os.path.join(ROOT, "tests", "c"),
                    os.path.join(ROOT, "tests", "c", "nr_trellis_plan_test.cc"), "-o", exe], check=True)
    out = subprocess.run([exe, vec], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.splitlines()[-1].startswith("ok ") and not out.stderr, out.stdout + out.stderr
    assert int(out.stdout.split()[-1]) == len(lines) + 2 * 3 * 3 * 7 * 3 and len(lines) >= 15


# ---- the entry points ----------------------------------------------------------------------------------------------------------

def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "amvhip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"^int\s+%s\s*\(\s*amvhip_ctx\s*\*\s*ctx\b[^;{]*\)\s*;" % name, text, flags=re.M), name
    for new, nr in zip(NAMES[:4], NR_NAMES):               # the -nr entries' arguments with lambda directly behind nr
        a = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % new, text).group(1)
        b = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % nr, text).group(1)
        names = [x.split()[-1].lstrip("*") for x in a.split(",")]
        nr_names = [x.split()[-1].lstrip("*") for x in b.split(",")]
        at = nr_names.index("nr") + 1
        assert names == nr_names[:at] + ["lambda"] + nr_names[at:], new
    a = re.search(r"\bamvhip_encode_frontend_quant_stream_dev\s*\(([^;]*)\)\s*;", text).group(1)
    b = re.search(r"\bamvhip_encode_frontend_batch_dev\s*\(([^;]*)\)\s*;", text).group(1)
    names = [" ".join(x.split()) for x in a.split(",")]
    batch = [" ".join(x.split()) for x in b.split(",")]
    assert names == [x if x != "uint32_t qbias" else "const amvhip_quant *q" for x in batch]
    assert re.search(r"typedef\s+struct\s+amvhip_quant\s*\{\s*uint32_t\s+qbias;\s*uint32_t\s+nr;\s*uint32_t\s+trellis;\s*uint32_t\s+lambda;\s*"
                     r"int32_t\s*\*\s*d_state;\s*\}\s*amvhip_quant\s*;", text)


def test_library_exports_them(pkg):
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in NAMES:
        assert name in exported, name
    data = open(pkg.LIB_PATH, "rb").read()
    for kernel in (b"amv_forward_kernelILb0EJNS_12NrTrellisArgE", b"amv_forward_kernelILb1EJNS_12NrTrellisArgE",
                   b"amv_encode_frame_kernelILb0EJNS_12NrTrellisArgE", b"amv_encode_frame_kernelILb1EJNS_12NrTrellisArgE"):
        assert kernel in data, kernel


def test_binding_has_them(pkg):
    for new, nr in zip(NAMES[:4], NR_NAMES):
        assert len(pkg.SYMBOLS[new][1]) == len(pkg.SYMBOLS[nr][1]) + 1, new
    assert len(pkg.SYMBOLS[NAMES[4]][1]) == len(pkg.SYMBOLS["amvhip_encode_frontend_batch_dev"][1])
    for method in ("encode_yuv420_nr_trellis_stream_dev", "encode_yuv420_nr_trellis_stream", "encode_nr_trellis_stream_dev",
                   "encode_nr_trellis_stream", "encode_frontend_quant_stream_dev"):
        assert callable(getattr(pkg.Context, method)), method
    # amvhip_quant as a C compiler lays it out: four uint32_t, then the pointer
    assert ctypes.sizeof(pkg.Quant) == 16 + ctypes.sizeof(ctypes.c_void_p) and pkg.Quant.d_state.offset == 16
    q = pkg.Quant(qbias=5, nr=300, trellis=1, lam=3481, state=0x1000)
    assert (q.qbias, q.nr, q.trellis, q.lambda_, q.d_state) == (5, 300, 1, 3481, 0x1000)


def test_null_context_and_untouched_memory(pkg):
    lib = pkg.load_library()
    buf = (ctypes.c_uint8 * 512)(*([0xEE] * 512))
    p = ctypes.addressof(buf)
    assert lib.amvhip_encode_yuv420_nr_trellis_stream_dev(None, p, p, p, 16, 8, 384, 384, 1, 16, 16, 0, 300, 3481, p, p, 64, p, p, None) == pkg.ERR_ARG
    assert lib.amvhip_encode_yuv420_nr_trellis_stream(None, p, p, p, 16, 8, 384, 384, 1, 16, 16, 0, 300, 3481, p, p, 64, p, p) == pkg.ERR_ARG
    assert lib.amvhip_encode_nr_trellis_stream_dev(None, p, 48, 0, 1, 16, 16, 0, 300, 3481, p, p, 64, p, p, None) == pkg.ERR_ARG
    assert lib.amvhip_encode_nr_trellis_stream(None, p, 48, 0, 1, 16, 16, 0, 300, 3481, p, p, 64, p, p) == pkg.ERR_ARG
    q = pkg.Quant(0, 300, 1, 3481, p)
    assert lib.amvhip_encode_frontend_quant_stream_dev(None, pkg.PIX_YUV420P, p, p, p, 16, 8, 384, 384, 16, 16, 1, None, 16, 16,
                                                       ctypes.addressof(q), p, 64, p, p, None) == pkg.ERR_ARG
    assert bytes(buf) == b"\xee" * 512
