"""No-GPU checks of the trellis stream (`-trellis N` with the step index chained on the device): the three entry points are
declared, exported and bound, refuse a NULL context, and the host arithmetic around them holds."""
import ctypes
import os
import re
import subprocess

from conftest import ROOT

NAMES = ("amvhip_adpcm_encode_trellis_stream_dev", "amvhip_adpcm_encode_trellis_stream", "amvhip_adpcm_trellis_chain_stats")


def test_header_declares_the_stream_entry_points():
    text = open(os.path.join(ROOT, "include", "amvhip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"^int\s+%s\s*\(\s*amvhip_ctx\s*\*\s*ctx\b[^;{]*\)\s*;" % name, text, flags=re.M), name
    dev = re.search(r"amvhip_adpcm_encode_trellis_stream_dev\s*\(([^;]*)\)\s*;", text).group(1)
    assert [a.split()[-1].lstrip("*") for a in dev.split(",")] == ["ctx", "d_pcm", "d_pcm_offs", "d_nsamp", "n", "first_step_index", "trellis",
                                                                 "d_blob", "d_offs", "d_step_out", "stream"]


def test_library_exports_them(pkg):
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in NAMES:
        assert name in exported, name
    data = open(pkg.LIB_PATH, "rb").read()
    for kernel in (b"amv_adpcm_trellis_guess_kernel", b"amv_adpcm_trellis_sweep_kernel", b"amv_adpcm_trellis_map_kernel"):
        assert kernel in data, kernel


def test_binding_has_them(pkg):
    for name in NAMES:
        assert name in pkg.SYMBOLS, name
    assert len(pkg.SYMBOLS["amvhip_adpcm_encode_trellis_stream_dev"][1]) == 11
    assert len(pkg.SYMBOLS["amvhip_adpcm_encode_trellis_stream"][1]) == 12
    for method in ("adpcm_encode_trellis_stream_dev", "adpcm_encode_trellis_stream", "adpcm_trellis_chain_stats"):
        assert callable(getattr(pkg.Context, method)), method


def test_null_context_is_refused(pkg):
    lib = pkg.load_library()
    buf = (ctypes.c_uint8 * 64)(*([0xEE] * 64))
    p = ctypes.addressof(buf)
    assert lib.amvhip_adpcm_encode_trellis_stream_dev(None, p, p, p, 1, 0, 3, p, p, p, None) == pkg.ERR_ARG
    assert lib.amvhip_adpcm_encode_trellis_stream(None, p, 2, p, p, 1, 0, 3, p, 9, p, p) == pkg.ERR_ARG
    out = (ctypes.c_uint32 * 64)(*([0xEE] * 64))
    assert lib.amvhip_adpcm_trellis_chain_stats(None, out) == pkg.ERR_ARG
    assert bytes(buf) == b"\xee" * 64 and list(out) == [0xEE] * 64


def test_host_arithmetic(tmp_path):
    """adpcm_trellis_tail and the chain plan of both ADPCM encoders (amv_host_plan.h), walked by
    tests/c/adpcm_chain_plan_test.cc under the address and undefined-behaviour sanitizers"""
    exe = str(tmp_path / "adpcm_chain_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "amv-codec-tools_amd", "csrc"), os.path.join(ROOT, "tests", "c", "adpcm_chain_plan_test.cc"), "-o", exe],
                   check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok ") and not out.stderr, out.stdout + out.stderr
