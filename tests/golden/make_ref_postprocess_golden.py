"""Writes tests/golden/ref_postprocess.json: plane hashes of the REAL reference's pp_postprocess and the modes its
pp_get_mode_by_name_and_quality parsed.

    python tests/golden/make_ref_postprocess_golden.py [--reference DIR] [--build DIR] [--jobs N] [--out FILE]

The maker builds the reference's ffmpeg in a temporary directory (make_ref_img_convert_golden.build_ffmpeg: --disable-mmx, so
the C path is the only one; --build names a tree built earlier), compiles tests/golden/ref_postprocess_harness.c inside it --
the harness #includes libpostproc/postprocess.c where it lies there -- and links it with its libavutil.a.  Nothing of the
reference enters this repository: the fixture holds, per case, the picture's recipe (size, builder kind and seed of
tests/pp_builder.picture, or "frame k of AMV1.amv as the oracle's FFmpeg-mode decode gives it"), the mode string and quality, the
forced QP, the fields the parser gave, and the FNV-1a-64 of each output plane.

Every case runs three times: destination pre-filled with 0x00, with 0xFF, and on a context that has processed another
picture.  A case whose three outputs differ is REFUSED: that refusal is the proof that the fixture pins a function of the
picture.  The maker also asserts that tests/pp_ref.py reproduces every case, and prints the reference's single-core time."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import pp_builder as B  # noqa: E402
import pp_ref as P  # noqa: E402
from make_ref_img_convert_golden import CONFIGURE, build_ffmpeg  # noqa: E402

REFUSED_MODES = ("h1", "v1", "ha", "va", "al", "lb", "li", "ci", "md", "fd", "l5", "tn", "fa", "ac", "nosuch", "hb:zz")


def link_harness(build, work):
    exe = os.path.join(work, "ref_postprocess_harness")
    cmd = ["gcc", "-O2", "-w", "-fgnu89-inline", "-DHAVE_AV_CONFIG_H", "-I", build, "-I", os.path.join(build, "libavutil"),
           "-I", os.path.join(build, "libpostproc"), os.path.join(HERE, "ref_postprocess_harness.c"), os.path.join(build, "libavutil", "libavutil.a"),
           "-lm", "-o", exe]
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:
        raise SystemExit("the harness does not link:\n" + p.stderr[-4000:])
    return exe


def pictures():
    import __graft_entry__ as G
    orc = G.load_oracle()
    orc.build()
    aw, ah, amv = B.amv1_frames(orc, HERE)
    out = []
    for name, w, h, kind, seed, mode, quality in B.cases():
        if kind.startswith("amv1:"):
            w, h, planes = aw, ah, amv[int(kind[5:])]
        else:
            planes = B.picture(w, h, kind, seed, B.case_qp(mode))
        out.append(({"name": name, "width": w, "height": h, "kind": kind, "seed": seed, "mode": mode, "quality": quality}, planes))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("AMV_REFERENCE", "/root/reference"))
    ap.add_argument("--build", help="the directory of a reference ffmpeg built earlier with make_ref_img_convert_golden's configure line")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(HERE, "ref_postprocess.json"))
    a = ap.parse_args()
    pics = pictures()
    cases, refused = [], []
    with tempfile.TemporaryDirectory() as work:
        build = a.build or os.path.dirname(build_ffmpeg(a.reference, work, a.jobs))
        exe = link_harness(build, work)
        inp, outp = os.path.join(work, "in.txt"), os.path.join(work, "out.txt")
        with open(inp, "w") as f:
            for i, (case, planes) in enumerate(pics):
                path = os.path.join(work, "pic%d.raw" % i)
                np.concatenate([p.reshape(-1) for p in planes]).tofile(path)
                f.write("%d %d %d %s %s\n" % (case["width"], case["height"], case["quality"], case["mode"], path))
            for mode in REFUSED_MODES:
                f.write("16 16 6 %s %s\n" % (mode, os.path.join(work, "pic0.raw")))
        subprocess.run([exe, inp, outp], check=True)
        lines = open(outp).read().splitlines()
    assert len(lines) == len(pics) + len(REFUSED_MODES)
    for (case, planes), line in zip(pics, lines):
        f = line.split()
        assert f[0] != "refused", case["name"]
        if f[5] != "1":
            raise SystemExit("REFUSED: %s is not a function of the picture (the three runs differ)" % case["name"])
        case["parsed"] = {"lumMode": int(f[0]), "chromMode": int(f[1]), "baseDcDiff": int(f[2]), "flatnessThreshold": int(f[3]), "forcedQuant": int(f[4])}
        case["qp"] = int(f[4]) if int(f[0]) & P.FORCE_QUANT else 1
        case["fnv"] = f[6:9]
        m = P.parse_mode(case["mode"], case["quality"])
        assert m == case["parsed"], (case["name"], m, case["parsed"])
        mine = ["%016x" % P.fnv1a64(p.tobytes()) for p in P.postprocess(planes, case["width"], case["height"], m)]
        assert mine == case["fnv"], "%s: the restatement departs from the reference: %s / %s" % (case["name"], mine, case["fnv"])
        print("%-48s %s  %.0f us a frame on one core" % (case["name"], " ".join(case["fnv"]), float(f[9])), flush=True)
        cases.append(case)
    for mode, line in zip(REFUSED_MODES, lines[len(pics):]):
        # the reference parses the filters this library does not build; it refuses only the last two
        refused.append({"mode": mode, "reference": "refused" if line == "refused" else "parsed"})
        assert P.parse_mode(mode, 6) is None, mode
    doc = {"about": "plane hashes of the reference's pp_postprocess (C path) and the modes its parser gave; made by make_ref_postprocess_golden.py",
           "configure": " ".join(CONFIGURE[1:]), "cases": cases, "refused": refused}
    with open(a.out, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
    print("%d cases, every one the same on a 0x00 and a 0xFF destination and on a used context" % len(cases))


if __name__ == "__main__":
    main()
