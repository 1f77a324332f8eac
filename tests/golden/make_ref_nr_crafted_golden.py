"""Writes tests/golden/ref_nr_crafted.json: chunks of the REAL reference's amv encoder with -nr N on the crafted corpus of
tests/nr_builder.py, through its own command line.

    python tests/golden/make_ref_nr_crafted_golden.py [--reference DIR] [--ffmpeg BINARY] [--jobs N] [--out FILE]

It works as make_ref_nr_golden.py does: the reference's ffmpeg is built in a temporary directory by
make_ref_img_convert_golden.build_ffmpeg (nothing of it enters this repository), every case is

    ffmpeg -f rawvideo -pix_fmt yuvj420p -s WxH -r 16 -i in.raw -an -vcodec amv -qscale 8 -nr N -f rawvideo out

and the fixture keeps the length and FNV-1a-64 hash of every chunk.  The command line cannot be handed a state, so the
cases are the corpus's that start from the zero state at sizes that are multiples of 16 (cases(), below): group B's frame
of all-zero samples followed by offsets of 65534, 32766 and the wrapped 2, and the zero-state cases of groups C and D.  The
test makes the same corpus again and replays it through the model's reference mode.

The maker asserts that the model with each of the faults signed_offsets, dc_unclamped and no_truncation gives other
coefficients (reference mode) somewhere on these streams, so the reference's own chunks pin all three; the counts are
recorded per case as "differ": {fault: [coefficients that differ, of]}."""
import argparse
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import nr_builder as B  # noqa: E402
import nr_ref as M  # noqa: E402
from make_ref_img_convert_golden import CONFIGURE, build_ffmpeg, run  # noqa: E402

PINNED = ("signed_offsets", "dc_unclamped", "no_truncation")


def cases():
    """the corpus's cases the command line can run: from the zero state, whole MCUs"""
    return [c for c in B.corpus(M.orc)[0] if c.from_zero() and c.w % 16 == 0 and c.h % 16 == 0]


def differ(case):
    """{fault: [coefficients that differ from the model's, of]} in reference mode"""
    a = M.encode_stream(case.frames, case.w, case.h, case.nr, mode="reference", want_coef=True)
    out = {}
    for fault in PINNED:
        b = M.encode_stream(case.frames, case.w, case.h, case.nr, mode="reference", want_coef=True, faults=(fault,))
        out[fault] = [sum(int((x != y).sum()) for x, y in zip(a, b)), sum(x.size for x in a)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("AMV_REFERENCE", "/root/reference"))
    ap.add_argument("--ffmpeg", help="a reference ffmpeg built earlier with make_ref_img_convert_golden's configure line")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(HERE, "ref_nr_crafted.json"))
    a = ap.parse_args()

    chosen = cases()
    assert {c.group for c in chosen} == {"B", "C", "D"}, sorted({c.group for c in chosen})
    docs = [{"name": c.name, "size": [c.w, c.h], "nr": c.nr, "frames": len(c.frames), "differ": differ(c)} for c in chosen]
    for fault in PINNED:
        assert sum(d["differ"][fault][0] for d in docs), "no case tells a model with %s apart" % fault

    with tempfile.TemporaryDirectory() as work:
        ffmpeg = a.ffmpeg or build_ffmpeg(a.reference, work, a.jobs)
        inp = os.path.join(work, "in.raw")
        for case, doc in zip(chosen, docs):
            with open(inp, "wb") as f:
                f.write(M.raw_bytes(case.frames))
            data, err = run(ffmpeg, work, ["-f", "rawvideo", "-pix_fmt", "yuvj420p", "-s", "%dx%d" % (case.w, case.h), "-r", "16", "-i", inp, "-an",
                                           "-vcodec", "amv", "-qscale", "8", "-nr", str(case.nr), "-f", "rawvideo"])
            assert data is not None, err
            chunks = M.split_chunks(data)
            assert len(chunks) == len(case.frames), "%s: %d chunks for %d frames" % (case.name, len(chunks), len(case.frames))
            doc["bytes"] = len(data)
            doc["chunks"] = [[len(c), "%016x" % M.fnv1a64(c)] for c in chunks]
    doc = {"about": "chunks of the reference's amv encoder with -nr (its ffmpeg command line) on the zero-state cases of tests/nr_builder.py; "
                    "made by make_ref_nr_crafted_golden.py",
           "configure": " ".join(CONFIGURE[1:]), "seed": B.SEED, "pinned": list(PINNED), "cases": docs}
    with open(a.out, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
    print("%d cases, %d chunks" % (len(docs), sum(len(d["chunks"]) for d in docs)))


if __name__ == "__main__":
    main()
