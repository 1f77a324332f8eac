"""Writes tests/golden/ref_retable.json: chunks of the REAL reference's amv encoder at several -qscale, through its own command line.

    python tests/golden/make_ref_retable_golden.py [--reference DIR] [--ffmpeg BINARY] [--jobs N] [--out FILE]

The reference's ffmpeg is built in a temporary directory by make_ref_img_convert_golden.build_ffmpeg; nothing of it enters
this repository.  Every case is

    ffmpeg -f rawvideo -pix_fmt yuvj420p -s 48x32 -r 16 -i in.raw -an -vcodec amv -qscale Q -f rawvideo out

for Q = 2, 5, 13, 31 on the three pictures tests/nr_ref.stream(48, 32, ["ramp", "texture", "noise"], 100) makes (the test makes
the same input again); the output is split into chunks at FF D8 ... FF D9.  The fixture keeps the length and the FNV-1a-64 hash
of every chunk.  Q = 8 is pinned already by ref_nr.json's ramp_nr0.

What it pins: tests/retable_ref.reference_chunks -- the matrix clip8(ff_mpeg1_default_intra_matrix * qscale >> 3) with entry 0
= 8 (mpegvideo_enc.c:2866-2877), and with it amvhip_ffmpeg_amv_tables and the inputs of the re-table tests.  With -qscale given,
CODEC_FLAG_QSCALE is set and the `qscale < 3` rule of :2863 does not apply; Q = 2 is here to show it."""
import argparse
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import nr_ref as M  # noqa: E402
from make_ref_img_convert_golden import CONFIGURE, build_ffmpeg, run  # noqa: E402

SIZE, KINDS, SEED, QSCALES = (48, 32), ["ramp", "texture", "noise"], 100, (2, 5, 13, 31)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("AMV_REFERENCE", "/root/reference"))
    ap.add_argument("--ffmpeg", help="a reference ffmpeg built earlier with make_ref_img_convert_golden's configure line")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(HERE, "ref_retable.json"))
    a = ap.parse_args()

    w, h = SIZE
    cases = []
    with tempfile.TemporaryDirectory() as work:
        ffmpeg = a.ffmpeg or build_ffmpeg(a.reference, work, a.jobs)
        inp = os.path.join(work, "in.raw")
        with open(inp, "wb") as f:
            f.write(M.raw_bytes(M.stream(w, h, KINDS, SEED)))
        for q in QSCALES:
            data, err = run(ffmpeg, work, ["-f", "rawvideo", "-pix_fmt", "yuvj420p", "-s", "%dx%d" % (w, h), "-r", "16", "-i", inp, "-an",
                                           "-vcodec", "amv", "-qscale", str(q), "-f", "rawvideo"])
            assert data is not None, err
            chunks = M.split_chunks(data)
            assert len(chunks) == len(KINDS), "%d chunks for %d frames" % (len(chunks), len(KINDS))
            cases.append({"name": "qscale%d" % q, "qscale": q, "size": [w, h], "kinds": KINDS, "seed": SEED, "bytes": len(data),
                          "chunks": [[len(c), "%016x" % M.fnv1a64(c)] for c in chunks]})
            print("qscale", q, [len(c) for c in chunks], flush=True)
    doc = {"about": "chunks of the reference's amv encoder at -qscale Q (its ffmpeg command line); made by make_ref_retable_golden.py",
           "configure": " ".join(CONFIGURE[1:]), "cases": cases}
    with open(a.out, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
    print("%d cases" % len(cases))


if __name__ == "__main__":
    main()
