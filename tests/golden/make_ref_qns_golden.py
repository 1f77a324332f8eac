"""Writes tests/golden/ref_qns.json: levels the REAL reference's dct_quantize_refine gave on seeded blocks.

    python tests/golden/make_ref_qns_golden.py [--reference DIR] [--build DIR] [--jobs N] [--out FILE]

The reference's command line cannot run this path for its amv encoder (intra_ac_vlc_length is NULL for MJPEG), and two of the
functions are static, so the maker builds the reference's ffmpeg in a temporary directory
(make_ref_img_convert_golden.build_ffmpeg; --build names one built earlier), compiles tests/golden/ref_qns_harness.c inside
its libavcodec -- the harness #includes mpegvideo_enc.c where it lies there -- links it with its libavcodec.a / libavutil.a,
and calls get_vissual_weight, dct_quantize_c and dct_quantize_refine themselves on a hand-filled context (the harness says
how).  Nothing of the reference enters this repository: the fixture holds, per case, the seed of its sample blocks
(tests/trellis_ref.reference_samples makes them again), qns, qscale and lambda2, and the FNV-1a-64 hash of the int16 levels
(64 per block, row-major, then the return value); and once the hash of the function's own basis table.

The length tables handed to the function are tests/trellis_ref.jpeg_uni_ac_lengths, as for the trellis fixture.

What the cases pin, and how the maker makes sure they do: the model must reproduce every hash, and for each rule of the walk
(tests/qns_ref.VARIANTS: strictness and the candidate order, the three -qns gates, the gradient rule, the + 512 >> 10 and
>> 6 roundings, the weight formula, the >> 19) a model WITHOUT the rule must give other levels on at least one case;
"pinned_by" says "reference" for a rule where it does and "restatement" where no such case was found."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import nr_ref as N  # noqa: E402
import qns_ref as Q  # noqa: E402
import trellis_ref as T  # noqa: E402
from make_ref_img_convert_golden import CONFIGURE, build_ffmpeg  # noqa: E402

BLOCKS = 12


def samples_of(case):
    rng = np.random.default_rng(case["seed"])
    return [T.reference_samples(rng, case["kind"]) for _ in range(case["blocks"])]


def model(case, length, **variant):
    out = []
    for s in samples_of(case):
        levels, last = Q.refine_block_reference(s, case["qscale"], case["lambda2"], case["qns"], length, length, **variant)
        out.append(levels + [last])
    return np.array(out, np.int16)


def differs(case, length, variant, got):
    try:
        return bool((model(case, length, **variant) != got).any())
    except AssertionError:                       # a model without the rule may leave the ranges the model asserts
        return True


def link_harness(build, work):
    exe = os.path.join(work, "ref_qns_harness")
    cmd = ["gcc", "-O1", "-w", "-fgnu89-inline", "-DHAVE_AV_CONFIG_H", "-I", build, "-I", os.path.join(build, "libavutil"),
           "-I", os.path.join(build, "libavcodec"), os.path.join(HERE, "ref_qns_harness.c"), os.path.join(build, "libavcodec", "libavcodec.a"),
           os.path.join(build, "libavutil", "libavutil.a"), "-lm", "-lpthread", "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:
        raise SystemExit("the harness does not link:\n" + p.stderr[-4000:])
    return exe


def reference(exe, work, case, length):
    """-> (the function's basis [64, 64], the levels and return values [blocks, 65])"""
    inp, out = os.path.join(work, "in.txt"), os.path.join(work, "out.txt")
    with open(inp, "w") as f:
        f.write("%d %d %d %d\n" % (case["qscale"], case["lambda2"], case["qns"], case["blocks"]))
        f.write(" ".join(str(x) for x in length) + "\n")
        for s in samples_of(case):
            f.write(" ".join(str(int(x)) for x in s) + "\n")
    subprocess.run([exe, inp, out], check=True)
    flat = np.array(open(out).read().split(), np.int64)
    return flat[:4096].reshape(64, 64), flat[4096:].reshape(case["blocks"], 65).astype(np.int16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("AMV_REFERENCE", "/root/reference"))
    ap.add_argument("--build", help="the directory of a reference ffmpeg built earlier with make_ref_img_convert_golden's configure line")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(HERE, "ref_qns.json"))
    a = ap.parse_args()

    length, _ = T.jpeg_uni_ac_lengths(0)
    cases = []
    for i, (kind, qscale) in enumerate((k, q) for q in (8, 2) for k in ("ramp", "texture", "noise", "sparse")):
        for qns in (1, 2, 3):
            # lambda2 of the qscale, and 0 on the noise blocks: the walk without a rate term
            lambda2 = 0 if (kind, qns) == ("noise", 3) else Q.lambda2_of_qscale(qscale)
            cases.append({"name": "%s_q%d_qns%d" % (kind, qscale, qns), "kind": kind, "seed": 5200 + 13 * i + qns, "blocks": BLOCKS,
                          "qscale": qscale, "qns": qns, "lambda2": lambda2})
    basis_hash = None
    with tempfile.TemporaryDirectory() as work:
        build = a.build or os.path.dirname(build_ffmpeg(a.reference, work, a.jobs))
        exe = link_harness(build, work)
        for case in cases:
            basis, got = reference(exe, work, case, length)
            assert (basis == Q.BASIS).all(), "the basis departs from the reference's at %s" % np.argwhere(basis != Q.BASIS)[0]
            basis_hash = "%016x" % N.fnv1a64(basis.astype("<i2").tobytes())
            mine = model(case, length)
            assert (got == mine).all(), "%s: the restatement departs from the reference at block, position %s" % (case["name"], np.argwhere(got != mine)[0])
            plain = np.array([Q.quantize_reference(N.fdct(s[None])[0], case["qscale"])[0] for s in samples_of(case)], np.int16)
            case["levels"] = "%016x" % N.fnv1a64(got.astype("<i2").tobytes())
            case["changed"] = int((got[:, :64] != plain).sum())
            case["tells_apart"] = [rule for rule, v in Q.VARIANTS if differs(case, length, v, got)]
            print(case["name"], case["changed"], case["tells_apart"], flush=True)
    pinned = {rule: "reference" if any(rule in c["tells_apart"] for c in cases) else "restatement" for rule, _ in Q.VARIANTS}
    assert all(any(c["changed"] for c in cases if c["qns"] == qns and c["kind"] == kind) for qns in (1, 2, 3) for kind in ("ramp", "texture", "noise", "sparse"))
    doc = {"about": "levels of the reference's dct_quantize_c + dct_quantize_refine on seeded blocks; made by make_ref_qns_golden.py",
           "configure": " ".join(CONFIGURE[1:]), "length_table": "%016x" % N.fnv1a64(bytes(length)), "basis": basis_hash,
           "pinned_by": pinned, "cases": cases}
    with open(a.out, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
    print("%d cases; pinned by: %s" % (len(cases), pinned))


if __name__ == "__main__":
    main()
