"""Writes tests/golden/ref_trellis.json: levels the REAL reference's dct_quantize_trellis_c gave on seeded blocks.

    python tests/golden/make_ref_trellis_golden.py [--reference DIR] [--build DIR] [--jobs N] [--out FILE]

The reference's command line cannot run this path for its amv encoder (no intra_ac_vlc_length is set for MJPEG: the first
AC coefficient reads through a null pointer), so the maker builds the reference's ffmpeg in a temporary directory
(make_ref_img_convert_golden.build_ffmpeg; --build names one built earlier), compiles tests/golden/ref_trellis_harness.c
against its headers and links it with its libavcodec.a / libavutil.a, and calls the function itself on a hand-filled
context (the harness says how).  Nothing of the reference enters this repository: the fixture holds, per case, the seed of
its sample blocks (tests/trellis_ref.reference_samples makes them again), the qscale and lambda, and the FNV-1a-64 hash of
the int16 levels (64 per block, row-major, then the return value).

The length table handed to the function is tests/trellis_ref.jpeg_uni_ac_lengths: the JPEG AC code's lengths laid out by
UNI_AC_ENC_INDEX, with esc_length for levels beyond +-64.

What the cases pin, and how the maker makes sure they do: the model must reproduce every hash, and for each of three rules
of the walk -- the `last_non_zero <= 27` pruning rule, survivors taken newest first, strictly smaller wins -- a model
WITHOUT the rule must give other levels on at least one case; "pinned_by" says "reference" for a rule where it does and
"restatement" where no such case was found."""
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
import trellis_ref as T  # noqa: E402
from make_ref_img_convert_golden import CONFIGURE, build_ffmpeg  # noqa: E402

BLOCKS = 96
VARIANTS = (("narrow_rule", {"narrow_rule": False}), ("newest_first", {"newest_first": False}), ("strict", {"strict": False}))


def samples_of(case):
    rng = np.random.default_rng(case["seed"])
    return [T.reference_samples(rng, case["kind"]) for _ in range(case["blocks"])]


def model(case, length, esc_length, **variant):
    out = []
    for s in samples_of(case):
        levels, last = T.trellis_block_reference(N.fdct(s[None])[0], case["qscale"], case["lambda"], length, esc_length, **variant)
        out.append(levels + [last])
    return np.array(out, np.int16)


def link_harness(build, work):
    exe = os.path.join(work, "ref_trellis_harness")
    cmd = ["gcc", "-O1", "-w", "-fgnu89-inline", "-I", build, "-I", os.path.join(build, "libavutil"), "-I", os.path.join(build, "libavcodec"),
           os.path.join(HERE, "ref_trellis_harness.c"), os.path.join(build, "libavcodec", "libavcodec.a"),
           os.path.join(build, "libavutil", "libavutil.a"), "-lm", "-lpthread", "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:
        raise SystemExit("the harness does not link:\n" + p.stderr[-4000:])
    return exe


def reference(exe, work, case, length, esc_length):
    inp, out = os.path.join(work, "in.txt"), os.path.join(work, "out.txt")
    with open(inp, "w") as f:
        f.write("%d %d %d %d\n" % (case["qscale"], 2 * case["lambda"], esc_length, case["blocks"]))
        f.write(" ".join(str(x) for x in length) + "\n")
        for s in samples_of(case):
            f.write(" ".join(str(int(x)) for x in s) + "\n")
    subprocess.run([exe, inp, out], check=True)
    return np.loadtxt(out, dtype=np.int64).reshape(case["blocks"], 65).astype(np.int16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("AMV_REFERENCE", "/root/reference"))
    ap.add_argument("--build", help="the directory of a reference ffmpeg built earlier with make_ref_img_convert_golden's configure line")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(HERE, "ref_trellis.json"))
    a = ap.parse_args()

    length, esc_length = T.jpeg_uni_ac_lengths(0)
    cases = []
    for i, (kind, qscale) in enumerate((k, q) for q in (8, 2, 5) for k in ("ramp", "texture", "noise", "sparse")):
        for lam in sorted({T.lambda_of_qscale(qscale), T.lambda_of_qscale(8)}):
            cases.append({"name": "%s_q%d_l%d" % (kind, qscale, lam), "kind": kind, "seed": 4100 + 17 * i, "blocks": BLOCKS, "qscale": qscale, "lambda": lam})
    with tempfile.TemporaryDirectory() as work:
        build = a.build or os.path.dirname(build_ffmpeg(a.reference, work, a.jobs))
        exe = link_harness(build, work)
        kept = []
        for case in cases:
            got = reference(exe, work, case, length, esc_length)
            mine = model(case, length, esc_length)
            assert (got == mine).all(), "%s: the restatement departs from the reference at block, position %s" % (case["name"], np.argwhere(got != mine)[0])
            case["levels"] = "%016x" % N.fnv1a64(got.astype("<i2").tobytes())
            case["nonzero"] = int((got[:, :64] != 0).sum())
            case["escapes"] = int((np.abs(got[:, 1:64]) > 63).sum())
            case["last_over_27"] = int((got[:, 64] > 27).sum())
            case["tells_apart"] = [rule for rule, v in VARIANTS if (model(case, length, esc_length, **v) != got).any()]
            print(case["name"], case["nonzero"], case["escapes"], case["last_over_27"], case["tells_apart"], flush=True)
            kept.append(case)
    pinned = {rule: "reference" if any(rule in c["tells_apart"] for c in kept) else "restatement" for rule, _ in VARIANTS}
    assert any(c["escapes"] for c in kept) and any(c["last_over_27"] for c in kept) and any(c["last_over_27"] < c["blocks"] for c in kept)
    doc = {"about": "levels of the reference's dct_quantize_trellis_c on seeded blocks; made by make_ref_trellis_golden.py",
           "configure": " ".join(CONFIGURE[1:]), "esc_length": esc_length, "length_table": "%016x" % N.fnv1a64(bytes(length)),
           "pinned_by": pinned, "cases": kept}
    with open(a.out, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
    print("%d cases; pinned by: %s" % (len(kept), pinned))


if __name__ == "__main__":
    main()
