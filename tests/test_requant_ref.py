"""No-GPU checks of requantising chunks in the coefficient domain: the model (tests/requant_ref.py) on the reference clip and on
oracle-encoded frames -- lambda 0 is the identity, every chunk is in range, a searched block never costs more than the one it
came from -- the HIP-free arithmetic of amv_requant_plan.h against the model and against 64-bit arithmetic
(tests/c/requant_plan_test.cc), and the entry points' declarations, exports and bindings."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import rate_ref as R
import requant_ref as Q
import trellis_ref as T
from conftest import ROOT

NAMES = ("amvhip_requant_stream_dev", "amvhip_requant_rate_probe_dev", "amvhip_requant_rate_stream_dev")


@pytest.fixture(scope="module")
def clip(amv1):
    return amv1["info"]["width"], amv1["info"]["height"], [bytes(c) for c in amv1["video"]]


def test_clip_is_the_one_the_numbers_were_taken_on(clip):
    w, h, chunks = clip
    assert (w, h, len(chunks)) == (128, 96, 252)


def test_lambda_0_returns_every_chunk_of_the_clip(clip):
    """all 252 chunks: in range, byte for byte at lambda 0, no error, and the largest AC value the issue names"""
    w, h, chunks = clip
    out, status, err = Q.requant(chunks, w, h, 0)
    assert status == [0] * len(chunks)
    assert all(o == c for o, c in zip(out, chunks)), [i for i, (o, c) in enumerate(zip(out, chunks)) if o != c][:8]
    assert err == [[0, 0, 0]] * len(chunks)
    most = 0
    for c in chunks:
        zz = Q.decode(c, w, h)[0]
        for b in range(zz.shape[0]):
            most = max(most, max(abs(x) for x in Q.scaled(zz[b], Q.comp_of(b))[1:]))
    assert most == 5904


def test_a_searched_block_never_costs_more(clip):
    """every twelfth chunk at lambda 200 (byte for byte still) and all 252 at 3481: every block's distortion + lambda * bits is at most the
    input levels' own -- the chunk's levels are a path of the walk -- and never has more bits; signs stay"""
    w, h, chunks = clip
    assert Q.requant(chunks[::12], w, h, 200)[0] == chunks[::12]
    lam, shorter = 3481, 0
    for chunk in chunks:
        before, after, st = Q.requant_lines(chunk, w, h, lam)
        assert st == 0
        for b in range(before.shape[0]):
            comp = Q.comp_of(b)
            if (before[b] == after[b]).all():
                continue
            c = Q.scaled(before[b], comp)
            assert T.block_cost(c, after[b], comp, lam) <= T.block_cost(c, before[b], comp, lam)
            # the input has the least distortion there is (every error 0), so what the search saves it saves in bits
            assert R.block_bits(after[b], comp) <= R.block_bits(before[b], comp)
            assert R.block_bits(after[b], comp) * lam <= T.block_cost(c, before[b], comp, lam) + sum(x * x for x in c[1:])
            old, new = before[b].astype(int), after[b].astype(int)
            coded = old != 0                                   # a coded level shrinks by at most one or goes; a zero may become +1 (it can shorten a run)
            assert ((np.abs(new[coded]) == np.abs(old[coded])) | (np.abs(new[coded]) == np.abs(old[coded]) - 1) | (new[coded] == 0)).all()
            assert (new[coded] * old[coded] >= 0).all() and np.isin(new[~coded], (0, 1)).all()
            assert after[b][0] == before[b][0]
        assert R.frame_bits(after) <= R.frame_bits(before)
        shorter += R.frame_bits(after) < R.frame_bits(before)
    assert shorter > 0


def test_the_issues_three_frames(clip):
    w, h, chunks = clip
    for k, want in ((0, [2655, 2582, 2116, 1110]),):
        assert [len(Q.requant([chunks[k]], w, h, lam)[0][0]) for lam in (0, 1000, 3481, 20000)] == want
    for k in (0, 100, 251):
        lens = [len(Q.requant([chunks[k]], w, h, lam)[0][0]) for lam in (0, 1000, 3481, 20000)]
        assert lens[0] == len(chunks[k]) and lens == sorted(lens, reverse=True) and len(set(lens)) == 4
        # qbias 0 would not even offer the chunk's own level: an exact multiple rounds one down
        zz = Q.decode(chunks[k], w, h)[0]
        moved = sum(T.trellis_block(Q.scaled(zz[b], Q.comp_of(b)), Q.comp_of(b), 0, 0)[1:] != [int(x) for x in zz[b][1:]] for b in range(zz.shape[0]))
        assert moved > 0


@pytest.mark.parametrize("w,h,qbias", [(16, 16, 0), (48, 32, 0), (48, 32, 128), (176, 144, 0)])
def test_lambda_0_is_the_identity_on_oracle_frames(w, h, qbias):
    chunks = Q.synth_chunks(w, h, 3, qbias=qbias)
    out, status, err = Q.requant(chunks, w, h, 0)
    assert status == [0, 0, 0] and out == chunks and err == [[0, 0, 0]] * 3
    # and the error is what the levels say
    smaller, _, err = Q.requant(chunks, w, h, 20000)
    assert all(len(a) < len(b) for a, b in zip(smaller, chunks)) and all(sum(e) > 0 for e in err)


def test_rate_is_first_fit_over_the_stream_entrys_chunks():
    w, h = 48, 32
    chunks = Q.synth_chunks(w, h, 4)
    table = [Q.requant(chunks, w, h, lam)[0] for lam in Q.LADDER]
    budgets = [len(table[2][0]), len(table[2][1]) - 1, 7, 1 << 31]
    out, status, rungs = Q.rate(chunks, w, h, Q.LADDER, budgets)
    assert status == [0] * 4
    assert rungs[2] == (4 | Q.OVER) and rungs[3] == 0 and out[3] == chunks[3] and rungs[0] <= 2 < rungs[1]
    assert all(out[i] == table[rungs[i] & ~Q.OVER][i] for i in range(4))
    bits = Q.bits_table(chunks, w, h, Q.LADDER)
    assert all(len(table[r][i]) == R.floor_bytes(int(bits[i][r])) + R.escapes(table[r][i]) for i in range(4) for r in range(len(Q.LADDER)))
    # a frame that is not coded: status, no chunk, the last rung flagged, a zero row
    bad = chunks[1][: len(chunks[1]) // 2]
    out, status, rungs = Q.rate([chunks[0], bad], w, h, Q.LADDER, 1 << 31)
    assert status[0] == 0 and status[1] != 0 and out[1] is None and rungs == [0, 4 | Q.OVER]
    assert (Q.bits_table([bad], w, h, Q.LADDER) == 0).all()


def test_the_range_rule():
    at = Q.block_of(Q.AT_ENERGY_MOST)
    assert Q.energy(at, 0) == Q.ENERGY_MOST and Q.block_in_range(at, 0)
    over = Q.block_of({**Q.AT_ENERGY_MOST, 59: 16})
    assert all(abs(x) <= Q.COEF_MOST for x in Q.scaled(over, 0)) and not Q.block_in_range(over, 0)
    for comp in (0, 1):
        for k in range(1, 64):
            q8 = 8 * int(T.QUANT[comp][k])
            assert Q.block_in_range(Q.block_of({k: Q.COEF_MOST // q8}), comp) and not Q.block_in_range(Q.block_of({k: -(Q.COEF_MOST // q8) - 1}), comp)
    assert Q.block_in_range(Q.block_of({}, dc=-1023), 0) and not Q.block_in_range(Q.block_of({}, dc=1024), 1)
    assert Q.COEF_MOST == 8681 and Q.LAMBDA_MAX == 537567


def _vectors(clip):
    """R comp lambda in[64] ok out[64] err: blocks of the clip, of the edges, and out of range"""
    w, h, chunks = clip
    rng = np.random.default_rng(5)
    blocks = []
    for k in (0, 100, 251):
        zz = Q.decode(chunks[k], w, h)[0]
        blocks += [(zz[b], Q.comp_of(b)) for b in rng.choice(zz.shape[0], 12, replace=False)]
    at = Q.block_of(Q.AT_ENERGY_MOST, dc=-1023)
    blocks += [(at, 0), ([-x for x in at], 0), (Q.block_of({**Q.AT_ENERGY_MOST, 59: 16}), 0), (Q.block_of({}, dc=1024), 1), (Q.block_of({}), 1)]
    for comp in (0, 1):
        for k in (1, 27, 28, 62, 63):
            q8 = 8 * int(T.QUANT[comp][k])
            blocks += [(Q.block_of({k: Q.COEF_MOST // q8, 1: 1}), comp), (Q.block_of({k: Q.COEF_MOST // q8 + 1}), comp)]
    lines = []
    for levels, comp in blocks:
        for lam in (0, 1000, 3481, Q.LAMBDA_MAX):
            ok = Q.block_in_range(levels, comp)
            out = Q.requant_block(levels, comp, lam) if ok else [0] * 64
            err = sum(((int(out[i]) - int(levels[i])) * int(T.QUANT[comp][i])) ** 2 for i in range(1, 64)) if ok else 0
            lines.append("R %d %d %s %d %s %d" % (comp, lam, " ".join(str(int(x)) for x in levels), ok, " ".join(str(int(x)) for x in out), err))
    return "\n" + "\n".join(lines) + "\n"


def test_host_arithmetic(tmp_path, clip):
    """amv_requant_plan.h walked by tests/c/requant_plan_test.cc under the address and undefined-behaviour sanitizers: the
    model's blocks, every level as its own first candidate, the 64-bit walk at the edges of the range and of lambda"""
    exe, vec = str(tmp_path / "requant_plan_test"), str(tmp_path / "vectors.txt")
    text = _vectors(clip)
    assert text.count("\nR ") >= 200 and " 0 " + " ".join(["0"] * 64) + " 0\n" in text
    open(vec, "w").write(text)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "amv-codec-tools_amd", "csrc"), os.path.join(ROOT, "tests", "c", "requant_plan_test.cc"), "-o", exe],
                   check=True)
    out = subprocess.run([exe, vec], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.splitlines()[-1].startswith("ok ") and not out.stderr, out.stdout + out.stderr
    assert int(out.stdout.split()[-1]) >= text.count("\nR ") + 80 + 252
    assert "first candidates: " in out.stdout and "edges: sums inside " in out.stdout
    least = int(re.search(r"edges: sums inside (-?\d+) \.\. ", out.stdout).group(1))
    assert -Q.ENERGY_MOST <= least < -(Q.ENERGY_MOST * 15 // 16)


# ---- the entry points ----------------------------------------------------------------------------------------------------------

def _arguments(text, name):
    return [x.split()[-1].lstrip("*") for x in re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, text).group(1).split(",")]


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "amvhip.h")).read()
    assert re.search(r"^#define\s+AMVHIP_ST_RANGE\s+8u\b", text, flags=re.M)
    bits = [int(x) for x in re.findall(r"^#define\s+AMVHIP_ST_\w+\s+(\d+)u\b", text, flags=re.M)]
    assert len(bits) == len(set(bits)) == 4 and all(b & (b - 1) == 0 for b in bits)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"^int\s+%s\s*\(\s*amvhip_ctx\s*\*\s*ctx\b[^;{]*\)\s*;" % name, text, flags=re.M), name
    front = _arguments(text, "amvhip_decode_batch_dev")
    front = front[: front.index("height") + 1]
    outs = ["d_out", "out_cap", "d_out_offs", "d_out_lens", "d_status"]
    assert _arguments(text, NAMES[0]) == front + ["lambda"] + outs + ["d_err", "stream"]
    assert _arguments(text, NAMES[1]) == front + ["ladder", "rungs", "d_bits", "stream"]
    assert _arguments(text, NAMES[2]) == front + ["rate"] + outs + ["d_rung", "stream"]


def test_library_exports_them(pkg):
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    for name in NAMES:
        assert name in exported, name
    data = open(pkg.LIB_PATH, "rb").read()
    for kernel in (b"amv_requant_kernel", b"amv_requant_probe_kernel", b"amv_requant_finish_kernel"):
        assert kernel in data, kernel


def test_binding_has_them(pkg):
    for name in NAMES:
        assert name in pkg.SYMBOLS, name
        assert callable(getattr(pkg.Context, name[len("amvhip_"):])), name
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "amvhip.h")).read(), flags=re.S)
    for name in NAMES:
        assert len(pkg.SYMBOLS[name][1]) == len(_arguments(text, name)), name
    assert pkg.ST_RANGE == Q.ST_RANGE == 8 and pkg.ST_TRUNCATED == Q.ST_TRUNCATED


def test_null_context_is_refused(pkg):
    lib = pkg.load_library()
    buf = (ctypes.c_uint8 * 512)(*([0xEE] * 512))
    p = ctypes.addressof(buf)
    assert lib.amvhip_requant_stream_dev(None, p, 64, p, p, 1, 16, 16, 0, p, 64, p, p, p, None, None) == pkg.ERR_ARG
    assert lib.amvhip_requant_rate_probe_dev(None, p, 64, p, p, 1, 16, 16, p, 1, p, None) == pkg.ERR_ARG
    assert lib.amvhip_requant_rate_stream_dev(None, p, 64, p, p, 1, 16, 16, p, p, 64, p, p, p, p, None) == pkg.ERR_ARG
    assert all(b == 0xEE for b in buf)
