"""No-GPU checks of the -nr noise reduction: the Python restatement (tests/nr_ref.py) against chunks of the reference's own
encoder (tests/golden/ref_nr.json, made by tests/golden/make_ref_nr_golden.py), the model's own invariants, the HIP-free
arithmetic of amv_nr_plan.h against the model (tests/c/nr_plan_test.cc), and the entry points' declarations and bindings."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import nr_ref as M
from conftest import GOLDEN, ROOT

NAMES = ("amvhip_encode_nr_max", "amvhip_encode_yuv420_nr_stream_dev", "amvhip_encode_yuv420_nr_stream", "amvhip_encode_nr_stream_dev",
         "amvhip_encode_nr_stream")


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(GOLDEN, "ref_nr.json")))


def _frames(case):
    w, h = case["size"]
    return w, h, M.stream(w, h, [k for k, n in case["runs"] for _ in range(n)], case["seed"])


def test_fdct_restatement_is_the_oracles(orc):
    rng = np.random.default_rng(5)
    blocks = np.concatenate([rng.integers(-128, 128, (40, 64)), rng.integers(0, 256, (40, 64)), np.full((1, 64), 255), np.full((1, 64), -128)])
    mine = M.fdct(blocks)
    for b, want in zip(blocks.astype(np.int16), mine):
        got = b.copy()
        orc.lib().amvo_fdct_islow(got.ctypes.data)
        assert (got == want).all()
    # the DC rule's premise: shifting the samples by 128 moves position 0 by 8192 and nothing else
    shifted = M.fdct(blocks[:40] + 128) - M.fdct(blocks[:40])
    assert (shifted[:, 0] == M.DC_SHIFT).all() and not shifted[:, 1:].any()


def test_reference_mode_reproduces_every_fixture_chunk(golden):
    assert [c["name"] for c in golden["cases"]] == ["ramp_nr0", "ramp_nr300", "ramp_nr3000", "ramp_nr30000", "truncation", "halving"]
    for case in golden["cases"]:
        w, h, frames = _frames(case)
        assert (w % 16, h % 16) == (0, 0) and len(frames) == case["frames"]
        chunks = M.encode_stream(frames, w, h, case["nr"], mode="reference")
        assert sum(len(c) for c in chunks) == case["bytes"], case["name"]
        if "chunks" in case:
            assert [[len(c), "%016x" % M.fnv1a64(c)] for c in chunks] == case["chunks"], case["name"]
        else:
            hsh, points = M.FNV_BASIS, dict((i, v) for i, v in case["chain"])
            for i, c in enumerate(chunks):
                hsh = M.fnv1a64(c, hsh)
                if i + 1 in points:
                    assert "%016x" % hsh == points.pop(i + 1), (case["name"], i + 1)
            assert not points
    sizes = {c["nr"]: c["bytes"] for c in golden["cases"][:4]}
    assert sizes[0] > sizes[300] > sizes[3000] > sizes[30000]        # the lever: size against detail


def test_fixture_tells_truncation_and_halving_apart(golden):
    """what the maker recorded holds again: without the 16-bit truncation, and (where the maker found such an input) without
    the halving, the model gives other coefficients on these cases -- so the chunks above pin both"""
    case = golden["cases"][4]
    w, h, frames = _frames(case)
    a = M.encode_stream(frames, w, h, case["nr"], mode="reference", want_coef=True)
    b = M.encode_stream(frames, w, h, case["nr"], mode="reference", want_coef=True, truncate=False)
    assert [sum(int((x != y).sum()) for x, y in zip(a, b)), sum(x.size for x in a)] == case["without_truncation_differ"]
    assert case["without_truncation_differ"][0] > 0
    case = golden["cases"][5]
    assert golden["halving_pinned_by"] in ("reference", "restatement")
    assert (case["without_halving_differ"][0] > 0) == (golden["halving_pinned_by"] == "reference")
    assert case["frames"] * 6 > 65536 + 6 * 100                       # the count passes 65536 well inside the stream


def test_product_mode_with_nr_0_is_the_plain_encoder(orc):
    for (w, h), kinds in (((48, 32), ["ramp", "texture"]), ((22, 38), ["texture", "noise"])):       # the second: padding blocks both ways
        frames = M.stream(w, h, kinds, 40)
        state = M.new_state()
        for (y, cb, cr), chunk in zip(frames, M.encode_stream(frames, w, h, 0, state=state, qbias=3)):
            assert chunk == orc.encode_frame_yuv(y, cb, cr, w, h, qbias=3)
        assert not state.any()


def test_model_is_split_invariant():
    w, h = 48, 32
    frames = M.stream(w, h, ["ramp", "texture", "flat", "texture", "ramp", "noise", "texture", "ramp"], 77)
    for mode in ("product", "reference"):
        whole_state = M.new_state()
        whole = M.encode_stream(frames, w, h, 700, state=whole_state, mode=mode)
        state, parts = M.new_state(), []
        for lo, hi in ((0, 3), (3, 4), (4, 8)):
            parts += M.encode_stream(frames[lo:hi], w, h, 700, state=state, mode=mode)
        assert parts == whole and (state == whole_state).all()
    assert whole != M.encode_stream(frames, w, h, 0, mode="reference")


def _ints(a):
    return " ".join(str(int(x)) for x in np.asarray(a).reshape(-1))


def _vectors():
    """what nr_plan_test.cc replays: the halving (a count of 65536 stays, 65537 halves), the truncation, the DC at
    D - offset < 0, and random blocks"""
    rng = np.random.default_rng(9)
    lines = []
    for count in (0, 1, 65536, 65537, 65536 + 1800, 131000):
        for nr in (1, 300, 911, 24000):
            state = np.concatenate([rng.integers(0, 16320 * (count + 1) + 1, 64), [count]]).astype(np.int64)
            state[:4] = (0, 1, 2, 16320 * count)                     # small sums: nr * count / (sum + 1) is far above 65535
            before = state.copy()
            off = M.frame_start(state, nr)
            assert count <= 65536 or state[64] == count >> 1
            lines.append("F %d %s %s %s" % (nr, _ints(before), _ints(state), _ints(off)))
    assert any(int(v) > 0xFFFF for v in M.frame_start(np.concatenate([np.zeros(64, np.int64), [72]]), 911, truncate=False))
    for k in range(24):
        state = np.concatenate([rng.integers(0, 1 << 30, 64), [rng.integers(0, 131000)]]).astype(np.int64)
        off = rng.integers(0, (40, 3000, 65536)[k % 3], 64)
        block = rng.integers(-2000, 2001, 64) * (rng.integers(0, 3, 64) > 0)
        block[0] = (-8192, 8128, -8000, 0, 300)[k % 5]               # reference DC 0, 16320, 192, 8192, 8492
        if k % 5 == 2:
            off[0] = 193                                              # D - offset < 0: the DC stops at 0, i.e. -8192 here
        before = state.copy()
        out = M.denoise_blocks(state, off, block[None, :], M.DC_SHIFT)[0]
        if k % 5 == 2:
            assert out[0] == -8192
        lines.append("B %s %s %s %s %s" % (_ints(before), _ints(off), _ints(block), _ints(state), _ints(out)))
    return "\n".join(lines) + "\n"


def test_host_arithmetic(tmp_path):
    """nr_frame_start, nr_block, the bound and the workspace of amv_nr_plan.h, walked by tests/c/nr_plan_test.cc under the
    address and undefined-behaviour sanitizers, on vectors the model writes"""
    exe, vec = str(tmp_path / "nr_plan_test"), str(tmp_path / "vectors.txt")
    open(vec, "w").write(_vectors())
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "amv-codec-tools_amd", "csrc"), os.path.join(ROOT, "tests", "c", "nr_plan_test.cc"), "-o", exe],
                   check=True)
    out = subprocess.run([exe, vec], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("ok ") and not out.stderr, out.stdout + out.stderr
    assert int(out.stdout.split()[1]) >= 48 + 8


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "amvhip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"^uint32_t\s+amvhip_encode_nr_max\s*\(\s*uint32_t\s+width\s*,\s*uint32_t\s+height\s*\)\s*;", text, flags=re.M)
    for name in NAMES[1:]:
        assert re.search(r"^int\s+%s\s*\(\s*amvhip_ctx\s*\*\s*ctx\b[^;{]*\)\s*;" % name, text, flags=re.M), name
    dev = re.search(r"amvhip_encode_yuv420_nr_stream_dev\s*\(([^;]*)\)\s*;", text).group(1)
    plain = re.search(r"amvhip_encode_yuv420_batch_dev\s*\(([^;]*)\)\s*;", text).group(1)
    names = [a.split()[-1].lstrip("*") for a in dev.split(",")]
    plain_names = [a.split()[-1].lstrip("*") for a in plain.split(",")]
    at = plain_names.index("qbias") + 1
    assert names == plain_names[:at] + ["nr", "d_state"] + plain_names[at:]


def test_library_exports_them(pkg):
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in NAMES:
        assert name in exported, name
    data = open(pkg.LIB_PATH, "rb").read()
    for kernel in (b"amv_nr_sums_kernel", b"amv_nr_chain_kernel"):
        assert kernel in data, kernel


def test_binding_has_them(pkg):
    for name in NAMES:
        assert name in pkg.SYMBOLS, name
    assert len(pkg.SYMBOLS["amvhip_encode_yuv420_nr_stream_dev"][1]) == len(pkg.SYMBOLS["amvhip_encode_yuv420_batch_dev"][1]) + 2
    assert len(pkg.SYMBOLS["amvhip_encode_nr_stream_dev"][1]) == len(pkg.SYMBOLS["amvhip_encode_batch_dev"][1]) + 2
    for method in ("encode_nr_max", "encode_yuv420_nr_stream_dev", "encode_yuv420_nr_stream", "encode_nr_stream_dev", "encode_nr_stream"):
        assert callable(getattr(pkg.Context, method)), method


def test_bound_and_null_context(pkg):
    lib = pkg.load_library()
    # 65536 is where the count settles for every frame of up to 65536 blocks: one bound for all of them
    assert lib.amvhip_encode_nr_max(16, 16) == lib.amvhip_encode_nr_max(320, 240) == lib.amvhip_encode_nr_max(1920, 1080) == 24607
    assert lib.amvhip_encode_nr_max(15, 16) == 0 and lib.amvhip_encode_nr_max(0, 16) == 0       # no size the encoder takes
    assert lib.amvhip_encode_nr_max(1680, 1664) == 24607 and lib.amvhip_encode_nr_max(1696, 1664) == 0   # 65520 blocks; 66144 blocks
    buf = (ctypes.c_uint8 * 512)(*([0xEE] * 512))
    p = ctypes.addressof(buf)
    assert lib.amvhip_encode_yuv420_nr_stream_dev(None, p, p, p, 16, 8, 384, 384, 1, 16, 16, 0, 300, p, p, 64, p, p, None) == pkg.ERR_ARG
    assert lib.amvhip_encode_yuv420_nr_stream(None, p, p, p, 16, 8, 384, 384, 1, 16, 16, 0, 300, p, p, 64, p, p) == pkg.ERR_ARG
    assert lib.amvhip_encode_nr_stream_dev(None, p, 48, 0, 1, 16, 16, 0, 300, p, p, 64, p, p, None) == pkg.ERR_ARG
    assert lib.amvhip_encode_nr_stream(None, p, 48, 0, 1, 16, 16, 0, 300, p, p, 64, p, p) == pkg.ERR_ARG
    assert bytes(buf) == b"\xee" * 512
