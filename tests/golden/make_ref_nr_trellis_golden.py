"""Writes tests/golden/ref_nr_trellis.json: what the REAL reference's dct_quantize_trellis_c gave on seeded blocks with noise
reduction on -- the order of the two steps (denoise_dct right behind the fdct, the search on what it leaves,
mpegvideo_enc.c:2987-2990) and where the sums are taken (before the offset is applied, :2948-2953).

    python tests/golden/make_ref_nr_trellis_golden.py [--reference DIR] [--build DIR] [--jobs N] [--out FILE]

Made as tests/golden/ref_trellis.json is (make_ref_trellis_golden.py says why the reference's command line cannot run this
path for its amv encoder, and how its ffmpeg is built in a temporary directory): tests/golden/ref_nr_trellis_harness.c is
compiled against that build's headers, linked with its libavcodec.a / libavutil.a, and calls the function itself on a
hand-filled context whose dct_error_sum, dct_count and dct_offset are filled too.  Nothing of the reference enters this
repository: the fixture holds, per case, the seed of its sample blocks (tests/trellis_ref.reference_samples), the qscale,
the lambda, the seed of the state and offsets (tests/nr_trellis_ref.reference_state), the FNV-1a-64 hash of the int16
levels (64 per block, row-major, then the return value) and that of dct_error_sum[64], dct_count afterwards (int32).

What the cases pin, and how the maker makes sure they do: the model (tests/nr_trellis_ref.reference_blocks) must reproduce
every hash, and each of two wrong models must differ on at least one case -- one that searches on the UN-denoised outputs
(other levels), one that sums the DENOISED magnitudes (other sums); "pinned_by" says "reference" for a rule where it does
and "restatement" where no such case was found."""
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
import nr_trellis_ref as NT  # noqa: E402
import trellis_ref as T  # noqa: E402
from make_ref_img_convert_golden import CONFIGURE, build_ffmpeg  # noqa: E402

BLOCKS = 48
VARIANTS = (("search_on_denoised", {"search_undenoised": True}), ("sums_before_offset", {"sum_denoised": True}))


def samples_of(case):
    rng = np.random.default_rng(case["seed"])
    return [T.reference_samples(rng, case["kind"]) for _ in range(case["blocks"])]


def model(case, length, esc_length, **variant):
    """-> (levels + return values int16 [blocks, 65], the state afterwards int64 [65])"""
    state, offsets = NT.reference_state(case["offsets_seed"])
    levels = NT.reference_blocks(samples_of(case), case["qscale"], case["lambda"], length, esc_length, state, offsets, **variant)
    return levels, state


def hashes(levels, state):
    return "%016x" % N.fnv1a64(levels.astype("<i2").tobytes()), "%016x" % N.fnv1a64(np.asarray(state).astype("<i4").tobytes())


def link_harness(build, work):
    exe = os.path.join(work, "ref_nr_trellis_harness")
    cmd = ["gcc", "-O1", "-w", "-fgnu89-inline", "-I", build, "-I", os.path.join(build, "libavutil"), "-I", os.path.join(build, "libavcodec"),
           os.path.join(HERE, "ref_nr_trellis_harness.c"), os.path.join(build, "libavcodec", "libavcodec.a"),
           os.path.join(build, "libavutil", "libavutil.a"), "-lm", "-lpthread", "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:
        raise SystemExit("the harness does not link:\n" + p.stderr[-4000:])
    return exe


def reference(exe, work, case, length, esc_length):
    inp, out = os.path.join(work, "in.txt"), os.path.join(work, "out.txt")
    state, offsets = NT.reference_state(case["offsets_seed"])
    with open(inp, "w") as f:
        f.write("%d %d %d %d\n" % (case["qscale"], 2 * case["lambda"], esc_length, case["blocks"]))
        f.write(" ".join(str(x) for x in length) + "\n")
        f.write(" ".join(str(int(x)) for x in state) + "\n")
        f.write(" ".join(str(int(x)) for x in offsets) + "\n")
        for s in samples_of(case):
            f.write(" ".join(str(int(x)) for x in s) + "\n")
    subprocess.run([exe, inp, out], check=True)
    rows = np.loadtxt(out, dtype=np.int64).reshape(case["blocks"] + 1, 65)
    return rows[:-1].astype(np.int16), rows[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("AMV_REFERENCE", "/root/reference"))
    ap.add_argument("--build", help="the directory of a reference ffmpeg built earlier with make_ref_img_convert_golden's configure line")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(HERE, "ref_nr_trellis.json"))
    a = ap.parse_args()

    length, esc_length = T.jpeg_uni_ac_lengths(0)
    cases = []
    for i, (kind, qscale) in enumerate((k, q) for q in (8, 2) for k in ("ramp", "texture", "noise", "sparse")):
        lam = T.lambda_of_qscale(qscale)
        cases.append({"name": "%s_q%d_l%d" % (kind, qscale, lam), "kind": kind, "seed": 5200 + 13 * i, "blocks": BLOCKS, "qscale": qscale,
                      "lambda": lam, "offsets_seed": 7300 + 29 * i})
    with tempfile.TemporaryDirectory() as work:
        build = a.build or os.path.dirname(build_ffmpeg(a.reference, work, a.jobs))
        exe = link_harness(build, work)
        for case in cases:
            got, got_state = reference(exe, work, case, length, esc_length)
            mine, my_state = model(case, length, esc_length)
            assert (got == mine).all(), "%s: the restatement departs from the reference at block, position %s" % (case["name"], np.argwhere(got != mine)[0])
            assert (got_state == my_state).all(), "%s: the sums depart from the reference at %s" % (case["name"], np.flatnonzero(got_state != my_state)[:8])
            case["levels"], case["error_sum"] = hashes(got, got_state)
            case["nonzero"] = int((got[:, :64] != 0).sum())
            case["offset_most"] = int(NT.reference_state(case["offsets_seed"])[1].max())
            case["tells_apart"] = [rule for rule, v in VARIANTS if hashes(*model(case, length, esc_length, **v)) != (case["levels"], case["error_sum"])]
            print(case["name"], case["nonzero"], case["offset_most"], case["tells_apart"], flush=True)
    pinned = {rule: "reference" if any(rule in c["tells_apart"] for c in cases) else "restatement" for rule, _ in VARIANTS}
    # the two wrong models differ on at least one case each: the fixture pins the order of the steps and the place of the sums
    assert all(v == "reference" for v in pinned.values()), pinned
    doc = {"about": "levels and sums of the reference's dct_quantize_trellis_c with noise reduction on, on seeded blocks; made by "
                    "make_ref_nr_trellis_golden.py",
           "configure": " ".join(CONFIGURE[1:]), "esc_length": esc_length, "length_table": "%016x" % N.fnv1a64(bytes(length)),
           "pinned_by": pinned, "cases": cases}
    with open(a.out, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
    print("%d cases; pinned by: %s" % (len(cases), pinned))


if __name__ == "__main__":
    main()
