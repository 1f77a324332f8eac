"""Writes tests/golden/ref_frontend.json: outputs of the REAL reference's -deinterlace, -crop*, -pad* and -padcolor, through
its own command line.

    python tests/golden/make_ref_frontend_golden.py [--reference DIR] [--ffmpeg BINARY] [--jobs N] [--out FILE]

The reference's ffmpeg is built in a temporary directory by make_ref_img_convert_golden.build_ffmpeg; nothing of it enters
this repository.  Every case is

    ffmpeg -f rawvideo -pix_fmt SRC -s WxH -i in.raw [-deinterlace] [-crop* N] [-s IWxIH] [-pad* N] [-padcolor RRGGBB]
           -f rawvideo -pix_fmt yuvj420p out.raw

on a seeded input made by tests/img_convert_ref.make_picture (the test makes the same input again); cases that differ in
-deinterlace alone share their input.  -s behind the input is
the INNER size: the pads are added to it (ffmpeg.c:2859-2860); the -crop* options subtract from the size parsed so far
(:2172), so they stand in front of -s.  The fixture keeps the FNV-1a-64 hash of every output frame and the first two rows of
each of its planes.  A case the reference's command line refuses is recorded with "pinned_by": "restatement" and the refusal.

Crop + pad without a rescale is left out: there av_picture_pad copies rows of the uncropped pitch past the window
(imgconvert.c:2282-2291), and what the picture holds afterwards is not a function of the input alone."""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import img_convert_ref as R  # noqa: E402
from make_ref_img_convert_golden import CONFIGURE, build_ffmpeg, describe, run  # noqa: E402

FRAMES = 2
SIDES = ("top", "bottom", "left", "right")


def case_list():
    """(src, (w, h), deinterlace, crop, inner size or None, pad, padcolor or None, kind, chain)"""
    none = (0, 0, 0, 0)
    cases = []
    for src in (R.YUV420P, R.YUV422P, R.YUV444P):
        for size in ((48, 32), (36, 8)):
            cases.append((src, size, True, none, None, none, None, "noise", False))
    for src in (R.YUVJ420P, R.RGB24):                                   # not in avpicture_deinterlace's list: goes on without
        cases.append((src, (48, 32), True, none, None, none, None, "noise", False))
        cases.append((src, (48, 32), False, none, None, none, None, "noise", False))
    for color in (None, "336699"):
        for pad in ((4, 0, 0, 0), (0, 6, 0, 0), (0, 0, 2, 0), (0, 0, 0, 8), (2, 4, 6, 2)):
            cases.append((R.YUV420P, (48, 32), False, none, None, pad, color, "noise", False))       # convert into the window
            cases.append((R.YUV422P, (64, 48), False, none, (32, 24), pad, color, "ramp", False))    # rescale into the window
    for src in (R.YUV420P, R.YUV422P, R.YUV444P, R.YUVJ420P):
        cases.append((src, (48, 32), False, (2, 4, 6, 2), None, none, None, "noise", False))
    cases.append((R.YUV420P, (48, 32), True, (2, 4, 6, 2), None, none, None, "noise", False))
    cases.append((R.YUYV422, (48, 32), False, (2, 0, 0, 0), None, none, None, "noise", False))       # av_picture_crop refuses
    for deint in (True, False):
        for kind in ("noise", "ramp"):
            cases.append((R.YUV420P, (352, 288), deint, (16, 16, 0, 0), (160, 90), (14, 16, 0, 0), None, kind, True))
    cases.append((R.YUV422P, (352, 288), True, (16, 16, 8, 8), (156, 90), (14, 16, 2, 2), "102030", "noise", True))
    for color in (None, "ff8000"):
        cases.append((R.YUVJ420P, (48, 32), False, none, None, (2, 4, 6, 2), color, "noise", False))  # no rescale: the copy route
    return cases


def command(inp, src, size, deint, crop, inner, pad, color):
    args = ["-f", "rawvideo", "-pix_fmt", R.NAMES[src], "-s", "%dx%d" % size, "-i", inp]
    if deint:
        args += ["-deinterlace"]
    for side, v in zip(SIDES, crop):
        if v:
            args += ["-crop" + side, str(v)]
    if inner:
        args += ["-s", "%dx%d" % inner]
    for side, v in zip(SIDES, pad):
        if v:
            args += ["-pad" + side, str(v)]
    if color:
        args += ["-padcolor", color]
    return args + ["-f", "rawvideo", "-pix_fmt", "yuvj420p"]


def out_size(size, crop, inner, pad):
    iw, ih = inner or (size[0] - crop[2] - crop[3], size[1] - crop[0] - crop[1])
    return iw + pad[2] + pad[3], ih + pad[0] + pad[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("AMV_REFERENCE", "/root/reference"))
    ap.add_argument("--ffmpeg", help="a reference ffmpeg built earlier with make_ref_img_convert_golden's configure line")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(HERE, "ref_frontend.json"))
    a = ap.parse_args()
    cases = []
    with tempfile.TemporaryDirectory() as work:
        ffmpeg = a.ffmpeg or build_ffmpeg(a.reference, work, a.jobs)
        inp = os.path.join(work, "in.raw")
        seeds = {}                                                      # a case with and without -deinterlace: one input
        for src, size, deint, crop, inner, pad, color, kind, chain in case_list():
            seed = seeds.setdefault((src, size, crop, inner, pad, color, kind), 5000 + 11 * len(seeds))
            np.concatenate([R.join(R.make_picture(src, size[0], size[1], kind, seed + i)) for i in range(FRAMES)]).tofile(inp)
            ow, oh = out_size(size, crop, inner, pad)
            case = {"src": R.NAMES[src], "src_size": list(size), "deinterlace": deint, "crop": list(crop), "inner_size": list(inner) if inner else None,
                    "pad": list(pad), "padcolor": color, "dst_size": [ow, oh], "frames": FRAMES, "input": {"kind": kind, "seed": seed},
                    "chain": chain}
            data, err = run(ffmpeg, work, command(inp, src, size, deint, crop, inner, pad, color))
            desc = None
            if data is not None:
                desc, err = describe(R.YUVJ420P, ow, oh, data, FRAMES)
            if desc is None:
                case.update({"pinned_by": "restatement", "refusal": err})
            else:
                case.update({"pinned_by": "reference"}, **desc)
            cases.append(case)
    doc = {"about": "outputs of the reference's ffmpeg command line (-deinterlace, -crop*, -pad*, -padcolor); made by make_ref_frontend_golden.py",
           "configure": " ".join(CONFIGURE[1:]), "cases": cases}
    with open(a.out, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
    pinned = sum(c["pinned_by"] == "reference" for c in cases)
    print("%d cases, %d pinned by the reference, %d by the restatement alone" % (len(cases), pinned, len(cases) - pinned))
    for c in cases:
        if c["pinned_by"] != "reference":
            print("  not pinned:", c["src"], c["src_size"], "crop", c["crop"], c["refusal"])


if __name__ == "__main__":
    main()
