"""Writes tests/golden/ref_nr.json: chunks of the REAL reference's amv encoder with -nr N, through its own command line.

    python tests/golden/make_ref_nr_golden.py [--reference DIR] [--ffmpeg BINARY] [--jobs N] [--out FILE] [--budget N]

The reference's ffmpeg is built in a temporary directory by make_ref_img_convert_golden.build_ffmpeg; nothing of it enters
this repository.  Every case is

    ffmpeg -f rawvideo -pix_fmt yuvj420p -s WxH -r 16 -i in.raw -an -vcodec amv -qscale 8 -nr N -f rawvideo out

on seeded pictures made by tests/nr_ref.stream (the test makes the same input again); the output is split into chunks at
FF D8 ... FF D9.  Sizes are multiples of 16: below that the reference reads edge rows outside the picture.  The fixture
keeps the length and FNV-1a-64 hash of every chunk; for the long case a chained hash (every chunk hashed from the hash of
the one before) with a checkpoint every CHECK frames.

What the cases pin, and how the maker makes sure they do:
  * 48x32, 6 frames of ramp + noise at -nr 0, 300, 3000, 30000: the dead zone and the running sums.
  * 48x32, two flat frames of 128 and four textured ones at -nr 911: the offset's truncation to 16 bits.  The maker asserts
    that the model WITHOUT the truncation gives other coefficients here.
  * 16x16 over enough frames to pass 65536 blocks: the halving.  Halving sums and count together nearly preserves the
    offsets, so the maker searches seeded inputs, on the CPU and within --budget candidates, for one on which the model
    WITHOUT the halving gives other coefficients; "halving_pinned_by" says "reference" when it found one (that input is the
    case) and "restatement" when it did not (the first candidate is the case: the chunks still cross the halving, but would
    not tell a model without it apart)."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import nr_ref as M  # noqa: E402
from make_ref_img_convert_golden import CONFIGURE, build_ffmpeg, run  # noqa: E402

CHECK = 512
LONG_FRAMES = 11100          # 6 blocks a frame: the count passes 65536 at the start of frame 10923


def expand(runs):
    return [k for k, n in runs for _ in range(n)]


def long_candidates(budget):
    """(runs, nr, seed): inputs on which the halving might show -- large offsets (a high nr), and positions whose sums stay
    small (flat frames between rare textured ones), where sum / 2 + 1 and (sum + 1) / 2 differ most"""
    out = []
    for i in range(budget):
        seed = 7000 + 13 * i
        if i % 2 == 0:
            out.append(([["ramp", LONG_FRAMES]], (20000, 4000, 24000, 500)[(i // 2) % 4], seed))
        else:
            out.append(([["texture", 1], ["flat", 10919], ["texture", LONG_FRAMES - 10920]], (911, 20000, 4000, 24000)[(i // 2) % 4], seed))
    return out


def coefficients_differ(w, h, frames, nr, **without):
    a = M.encode_stream(frames, w, h, nr, mode="reference", want_coef=True)
    b = M.encode_stream(frames, w, h, nr, mode="reference", want_coef=True, **without)
    return sum(int((x != y).sum()) for x, y in zip(a, b)), sum(x.size for x in a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("AMV_REFERENCE", "/root/reference"))
    ap.add_argument("--ffmpeg", help="a reference ffmpeg built earlier with make_ref_img_convert_golden's configure line")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(HERE, "ref_nr.json"))
    ap.add_argument("--budget", type=int, default=8, help="seeded inputs tried for one that shows the halving")
    a = ap.parse_args()

    cases = []
    for nr in (0, 300, 3000, 30000):
        cases.append({"name": "ramp_nr%d" % nr, "size": [48, 32], "runs": [["ramp", 6]], "seed": 100, "nr": nr})
    trunc = {"name": "truncation", "size": [48, 32], "runs": [["flat", 2], ["texture", 4]], "seed": 300, "nr": 911}
    frames = M.stream(48, 32, expand(trunc["runs"]), trunc["seed"])
    differ, of = coefficients_differ(48, 32, frames, trunc["nr"], truncate=False)
    assert differ, "the truncation case does not tell a model without the 16-bit truncation apart"
    trunc["without_truncation_differ"] = [differ, of]
    cases.append(trunc)

    pinned, tried, chosen = "restatement", [], None
    for runs, nr, seed in long_candidates(a.budget):
        frames = M.stream(16, 16, expand(runs), seed)
        differ, of = coefficients_differ(16, 16, frames, nr, halve=False)
        tried.append({"runs": runs, "nr": nr, "seed": seed, "without_halving_differ": [differ, of]})
        print("halving candidate", runs, nr, seed, "->", differ, "of", of, flush=True)
        if chosen is None or differ:
            chosen = {"name": "halving", "size": [16, 16], "runs": runs, "seed": seed, "nr": nr, "without_halving_differ": [differ, of]}
        if differ:
            pinned = "reference"
            break
    cases.append(chosen)

    with tempfile.TemporaryDirectory() as work:
        ffmpeg = a.ffmpeg or build_ffmpeg(a.reference, work, a.jobs)
        inp = os.path.join(work, "in.raw")
        for case in cases:
            (w, h), kinds = case["size"], expand(case["runs"])
            with open(inp, "wb") as f:
                f.write(M.raw_bytes(M.stream(w, h, kinds, case["seed"])))
            data, err = run(ffmpeg, work, ["-f", "rawvideo", "-pix_fmt", "yuvj420p", "-s", "%dx%d" % (w, h), "-r", "16", "-i", inp, "-an",
                                           "-vcodec", "amv", "-qscale", "8", "-nr", str(case["nr"]), "-f", "rawvideo"])
            assert data is not None, err
            chunks = M.split_chunks(data)
            assert len(chunks) == len(kinds), "%d chunks for %d frames" % (len(chunks), len(kinds))
            case["frames"] = len(kinds)
            case["bytes"] = len(data)
            if len(chunks) <= 64:
                case["chunks"] = [[len(c), "%016x" % M.fnv1a64(c)] for c in chunks]
            else:
                hsh, points = M.FNV_BASIS, []
                for i, c in enumerate(chunks):
                    hsh = M.fnv1a64(c, hsh)
                    if (i + 1) % CHECK == 0 or i + 1 == len(chunks):
                        points.append([i + 1, "%016x" % hsh])
                case["chain"] = points
    doc = {"about": "chunks of the reference's amv encoder with -nr (its ffmpeg command line); made by make_ref_nr_golden.py",
           "configure": " ".join(CONFIGURE[1:]), "halving_pinned_by": pinned, "halving_candidates": tried, "cases": cases}
    with open(a.out, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
    print("%d cases; the halving is pinned by the %s (%d candidates tried)" % (len(cases), pinned, len(tried)))


if __name__ == "__main__":
    main()
