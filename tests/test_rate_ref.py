"""No-GPU checks of the encoder's byte budget per frame: the model (tests/rate_ref.py) against itself -- bits from the levels,
lengths from the bytes, tied by len == 4 + ceil(bits / 8) + escapes -- on the inputs the GPU tests use, what those inputs must
contain, the choice as the device makes it against the definition, the HIP-free arithmetic of amv_rate_plan.h against the
model (tests/c/rate_plan_test.cc), and the entry points' declarations and bindings."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import rate_ref as R
import trellis_ref as T
from conftest import ROOT

NAMES = ("amvhip_encode_rate_probe_dev", "amvhip_encode_yuv420_rate_probe_dev", "amvhip_encode_rate_stream_dev",
         "amvhip_encode_yuv420_rate_stream_dev", "amvhip_encode_frontend_rate_stream_dev")
MULTI_LADDER = [400, 400, 400, 3481, T.LAMBDA_MAX]


@pytest.fixture(scope="module")
def tables():
    """name -> (bits [n][5], lens [n][5], escapes [n][5]) at qbias 0 over R.LADDER, for the three shapes"""
    out = {}
    for name in R.SHAPES:
        w, h, frames = R.shape(name)
        chunks = R.chunks_table(frames, w, h, 0, 0, None, R.LADDER)
        out[name] = (R.bits_table(frames, w, h, 0, 0, None, R.LADDER), np.array([[len(c) for c in row] for row in chunks]),
                     np.array([[R.escapes(c) for c in row] for row in chunks]))
    return out


def budgets_of(bits, lens, esc):
    """the GPU tests' budget kinds per frame -> {kind: [B(i)]}"""
    n = lens.shape[0]
    with_escapes = [next((r for r in range(lens.shape[1]) if esc[i][r]), None) for i in range(n)]
    return {"middle": [int(lens[i][2]) for i in range(n)], "middle - 1": [int(lens[i][2]) - 1 for i in range(n)],
            "floor": [R.floor_bytes(int(bits[i][2 if with_escapes[i] is None else with_escapes[i]])) for i in range(n)],
            "nothing": [7] * n, "anything": [0xFFFFFFFF] * n}


def test_length_is_floor_plus_escapes(tables):
    for name, (bits, lens, esc) in tables.items():
        for i in range(lens.shape[0]):
            for r in range(lens.shape[1]):
                assert lens[i][r] == 4 + -(-int(bits[i][r]) // 8) + esc[i][r], (name, i, r)
                assert R.floor_bytes(int(bits[i][r])) <= lens[i][r]
    w, h, frames = R.shape("16x16")                          # qbias and -nr on the way: the tie holds behind both
    state = np.arange(65) * 300 + 11
    bits = R.bits_table(frames[:4], w, h, 128, 2000, state, R.LADDER[1:4])
    chunks = R.chunks_table(frames[:4], w, h, 128, 2000, state, R.LADDER[1:4])
    assert all(len(chunks[i][r]) == R.floor_bytes(int(bits[i][r])) + R.escapes(chunks[i][r]) for i in range(4) for r in range(3))


def test_inputs_hold_what_the_gpu_tests_rely_on(tables):
    bits, lens, esc = tables["50x38"]
    assert (esc > 0).any()
    assert esc[1][2] == 9                                    # the texture frame at lambda 3481
    assert (tables["176x96"][2] > 0).any()
    # sizes are not monotone in lambda: frame 6 of the 16x16 stream costs a byte more at 400 than at 0
    bits, lens, esc = tables["16x16"]
    assert (int(lens[6][0]), int(lens[6][1])) == (195, 196)
    assert any((np.diff(t[1], axis=1) > 0).any() for t in tables.values())
    # a first floor-fit that is not the first true fit, at the "floor" budgets the GPU tests hand over
    for name, (bits, lens, esc) in tables.items():
        B = budgets_of(bits, lens, esc)["floor"]
        redo = [i for i in range(lens.shape[0]) if R.first_fit(bits[i], B[i], 0) != R.choose(lens[i], B[i])[0]]
        assert redo, name
    # several redo passes for one frame: three equal rungs that floor-fit and do not fit
    w, h, frames = R.shape("16x16")
    bits = R.bits_table(frames, w, h, 0, 0, None, MULTI_LADDER)
    lens = R.lens_table(frames, w, h, 0, 0, None, MULTI_LADDER)
    B = R.floor_bytes(int(bits[6][0]))
    assert R.device_walk(bits[6], lens[6], B) == (3, False, 4) and R.choose(lens[6], B) == (3, False)


def test_device_walk_is_the_definition(tables):
    """rate_first_fit + the check, run as the device loop runs them, give `choose` on every row at every budget kind -- and at
    every budget around a row's own floors and lengths"""
    rows = 0
    for name, (bits, lens, esc) in tables.items():
        kinds = budgets_of(bits, lens, esc)
        for i in range(lens.shape[0]):
            around = {int(x) + d for x in list(lens[i]) + [R.floor_bytes(int(b)) for b in bits[i]] for d in (-1, 0, 1)}
            for B in [k[i] for k in kinds.values()] + sorted(around):
                for order in (slice(None), slice(None, None, -1)):          # ascending and descending ladders
                    rung, over, codings = R.device_walk(bits[i][order], lens[i][order], B)
                    assert (rung, over) == R.choose(lens[i][order], B), (name, i, B)
                    assert 1 <= codings <= lens.shape[1]
                    rows += 1
    assert rows > 500


def _ints(xs):
    return " ".join(str(int(x)) for x in xs)


def _vectors(tables):
    lines = []
    w, h, frames = R.shape("50x38")
    levels, _ = R.levels_table(frames, w, h, 0, 0, None, R.LADDER)
    for r in (0, 2, 4):
        for i in (0, 1, 2):
            zz = levels[r][i]
            for b in range(0, zz.shape[0], 5):
                comp = 0 if b % 6 < 4 else 1
                lines.append("B %d %s %d" % (comp, _ints(zz[b]), R.block_bits(zz[b], comp)))
    for comp in (0, 1):
        for diff in list(range(-40, 41)) + [-2047, -1024, -1023, -256, -255, 255, 256, 1023, 1024, 2047]:
            lines.append("D %d %d %d" % (comp, diff, R.dc_bits(diff, comp)))
    before = {}
    for b in range(40):                                       # the predecessor by walking the blocks as the coder does
        c = 0 if b % 6 < 4 else b % 6 - 3
        lines.append("P %d %d" % (b, before.get(c, -1)))
        before[c] = b
    for bits in list(range(0, 40)) + [4095, 4096, 4097, (1 << 32) - 9, (1 << 32) - 8, (1 << 32) - 7, (1 << 32) - 1]:
        lines.append("F %d %d" % (bits, R.floor_bytes(bits)))
    for name, (bits, lens, esc) in tables.items():
        kinds = budgets_of(bits, lens, esc)
        for i in range(lens.shape[0]):
            for B in sorted({k[i] for k in kinds.values()} | {int(x) - 1 for x in lens[i]}):
                for row_b, row_l in ((bits[i], lens[i]), (bits[i][::-1], lens[i][::-1]), (bits[i][:1], lens[i][:1])):
                    fits = [R.first_fit(row_b, B, start) for start in range(len(row_b) + 1)]
                    rung, over, codings = R.device_walk(row_b, row_l, B)
                    lines.append("W %d %d %s %s %s %d %d %d" % (len(row_b), B, _ints(row_b), _ints(row_l), _ints(fits), rung, over, codings))
    return "\n".join(lines) + "\n"


def test_host_arithmetic(tmp_path, tables):
    """block bits, the DC term, floors and rate_first_fit from every `from` of amv_rate_plan.h, walked by
    tests/c/rate_plan_test.cc under the address and undefined-behaviour sanitizers, on vectors the model writes"""
    exe, vec = str(tmp_path / "rate_plan_test"), str(tmp_path / "vectors.txt")
    text = _vectors(tables)
    assert all(text.count("\n%s " % tag) >= 40 for tag in "BDPFW")
    open(vec, "w").write(text)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "amv-codec-tools_amd", "csrc"), os.path.join(ROOT, "tests", "c", "rate_plan_test.cc"), "-o", exe],
                   check=True)
    out = subprocess.run([exe, vec], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.splitlines()[-1].startswith("ok ") and not out.stderr, out.stdout + out.stderr
    assert int(out.stdout.split()[-1]) >= text.count("\n") + 10
    assert "bits per block at most 2048, blocks at most 2097151\n" in out.stdout


# ---- the entry points ----------------------------------------------------------------------------------------------------------

def _arguments(text, name):
    return [x.split()[-1].lstrip("*") for x in re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, text).group(1).split(",")]


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "amvhip.h")).read()
    assert re.search(r"^#define\s+AMVHIP_RATE_RUNGS_MAX\s+16\s*$", text, flags=re.M)
    assert re.search(r"^#define\s+AMVHIP_RATE_OVER\s+0x80000000u\b", text, flags=re.M)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"typedef\s+struct\s+amvhip_rate\s*\{\s*const\s+uint32_t\s*\*\s*ladder\s*;\s*uint32_t\s+rungs\s*;\s*uint32_t\s+budget\s*;"
                     r"\s*const\s+uint32_t\s*\*\s*d_budget\s*;\s*\}\s*amvhip_rate\s*;", text)
    for name in NAMES:
        assert re.search(r"^int\s+%s\s*\(\s*amvhip_ctx\s*\*\s*ctx\b[^;{]*\)\s*;" % name, text, flags=re.M), name
    for new, old in (("amvhip_encode_rate_stream_dev", "amvhip_encode_quant_psnr_stream_dev"),
                     ("amvhip_encode_yuv420_rate_stream_dev", "amvhip_encode_yuv420_quant_psnr_stream_dev"),
                     ("amvhip_encode_frontend_rate_stream_dev", "amvhip_encode_frontend_quant_psnr_stream_dev")):
        names, old_names = _arguments(text, new), _arguments(text, old)
        at = old_names.index("q") + 1
        assert names == old_names[:at] + ["rate"] + [("d_rung" if x == "d_sse" else x) for x in old_names[at:]], new
    for new, old in (("amvhip_encode_rate_probe_dev", "amvhip_encode_quant_psnr_stream_dev"),
                     ("amvhip_encode_yuv420_rate_probe_dev", "amvhip_encode_yuv420_quant_psnr_stream_dev")):
        names, old_names = _arguments(text, new), _arguments(text, old)
        assert names == old_names[:old_names.index("q") + 1] + ["ladder", "rungs", "d_bits", "stream"], new


def test_library_exports_them(pkg):
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in NAMES:
        assert name in exported, name
    data = open(pkg.LIB_PATH, "rb").read()
    for kernel in (b"amv_rate_probe_kernelILb0ELb0E", b"amv_rate_probe_kernelILb0ELb1E", b"amv_rate_probe_kernelILb1ELb0E",
                   b"amv_rate_probe_kernelILb1ELb1E", b"amv_rate_dc_kernel", b"amv_rate_choose_kernel", b"amv_rate_check_kernel",
                   b"amv_forward_kernelILb0EJNS_13TrellisFramesE", b"amv_forward_kernelILb1EJNS_15NrTrellisFramesE"):
        assert kernel in data, kernel
    # the one-kernel encoder has no instantiation with a lambda per frame
    assert b"amv_encode_frame_kernelILb0EJNS_10TrellisArgE" in data
    assert b"amv_encode_frame_kernelILb0EJNS_13TrellisFramesE" not in data and b"amv_encode_frame_kernelILb1EJNS_15NrTrellisFramesE" not in data


def test_binding_has_them(pkg):
    for name in NAMES:
        assert name in pkg.SYMBOLS, name
    for new, old in (("amvhip_encode_rate_stream_dev", "amvhip_encode_quant_psnr_stream_dev"),
                     ("amvhip_encode_yuv420_rate_stream_dev", "amvhip_encode_yuv420_quant_psnr_stream_dev"),
                     ("amvhip_encode_frontend_rate_stream_dev", "amvhip_encode_frontend_quant_psnr_stream_dev")):
        assert len(pkg.SYMBOLS[new][1]) == len(pkg.SYMBOLS[old][1]) + 1, new
    for new, old in (("amvhip_encode_rate_probe_dev", "amvhip_encode_quant_psnr_stream_dev"),
                     ("amvhip_encode_yuv420_rate_probe_dev", "amvhip_encode_yuv420_quant_psnr_stream_dev")):
        assert len(pkg.SYMBOLS[new][1]) == len(pkg.SYMBOLS[old][1]) - 2, new
    for name in NAMES:
        assert callable(getattr(pkg.Context, name[len("amvhip_"):])), name
    assert (pkg.RATE_RUNGS_MAX, pkg.RATE_OVER) == (R.RUNGS_MAX, R.OVER)
    # the struct's layout is the header's: two pointers round two words
    assert ctypes.sizeof(pkg.Rate) == 2 * ctypes.sizeof(ctypes.c_void_p) + 8
    assert (pkg.Rate.ladder.offset, pkg.Rate.rungs.offset, pkg.Rate.budget.offset, pkg.Rate.d_budget.offset) == (0, 8, 12, 16)
    rate = pkg.Rate([5, 6, 7], budget=99)
    assert (rate.rungs, rate.budget, rate.d_budget) == (3, 99, None)
    assert list((ctypes.c_uint32 * 3).from_address(rate.ladder)) == [5, 6, 7]


def test_null_context_is_refused(pkg):
    lib = pkg.load_library()
    buf = (ctypes.c_uint8 * 512)(*([0xEE] * 512))
    p = ctypes.addressof(buf)
    assert lib.amvhip_encode_rate_probe_dev(None, p, 48, 0, 1, 16, 16, p, p, 1, p, None) == pkg.ERR_ARG
    assert lib.amvhip_encode_yuv420_rate_probe_dev(None, p, p, p, 16, 8, 384, 384, 1, 16, 16, p, p, 1, p, None) == pkg.ERR_ARG
    assert lib.amvhip_encode_rate_stream_dev(None, p, 48, 0, 1, 16, 16, p, p, p, 64, p, p, p, None) == pkg.ERR_ARG
    assert lib.amvhip_encode_yuv420_rate_stream_dev(None, p, p, p, 16, 8, 384, 384, 1, 16, 16, p, p, p, 64, p, p, p, None) == pkg.ERR_ARG
    assert lib.amvhip_encode_frontend_rate_stream_dev(None, pkg.PIX_YUV420P, p, p, p, 16, 8, 384, 384, 16, 16, 1, None, 16, 16, p, p, p, 64, p,
                                                      p, p, None) == pkg.ERR_ARG
    assert all(b == 0xEE for b in buf)
