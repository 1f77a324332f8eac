"""Writes tests/golden/ref_img_convert.json: outputs of the REAL reference's img_convert and sws_scale shim, through its own
command line.

    python tests/golden/make_ref_img_convert_golden.py [--reference DIR] [--ffmpeg BINARY] [--jobs N]

The reference's ffmpeg (AMVmuxer/ffmpeg of the reference tree) is copied to a temporary directory, configured with the
line of SURVEY.md section 8c and built there, as tools/ffmpeg_integration.sh does; nothing of it enters this repository.
Every case is

    ffmpeg -f rawvideo -pix_fmt SRC -s WxH -i in.raw -f rawvideo -pix_fmt DST [-s W'xH'] out.raw

on a seeded input made by tests/img_convert_ref.make_picture (the test makes the same input again), or the decode of
tests/golden/AMV1.amv.  The fixture keeps the FNV-1a-64 hash of every output frame and the first two rows of each of its
planes.  A case the reference's command line refuses is recorded with "pinned_by": "restatement" and the refusal."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import img_convert_ref as R  # noqa: E402

CONFIGURE = ["./configure", "--disable-mmx", "--disable-network", "--disable-zlib", "--disable-vhook", "--disable-ffserver",
             "--disable-ffplay", "--disable-debug", "--extra-cflags=-fgnu89-inline -w"]
FRAMES = 2
EVEN, EVEN2, ODD = (48, 32), (70, 26), (37, 23)


def build_ffmpeg(reference, work, jobs):
    src = os.path.join(reference, "AMVmuxer", "ffmpeg")
    dst = os.path.join(work, "ffmpeg")
    shutil.copytree(src, dst)
    subprocess.run(["chmod", "-R", "u+w", dst], check=True)
    subprocess.run(CONFIGURE, cwd=dst, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    subprocess.run(["make", "-j%d" % jobs], cwd=dst, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return os.path.join(dst, "ffmpeg")


def run(ffmpeg, work, args):
    out = os.path.join(work, "out.raw")
    if os.path.exists(out):
        os.remove(out)
    p = subprocess.run([ffmpeg] + args + ["-y", out], cwd=work, capture_output=True, text=True)
    if p.returncode != 0 or not os.path.exists(out):
        return None, (p.stderr.strip().splitlines() or ["failed"])[-1]
    return open(out, "rb").read(), None


def describe(fmt, w, h, data, frames):
    fb = R.frame_bytes(fmt, w, h)
    if len(data) != fb * frames:
        return None, "the output holds %d bytes, %d frames of %d were expected" % (len(data), frames, fb)
    hashes, rows = [], []
    for i in range(frames):
        frame = np.frombuffer(data[i * fb:(i + 1) * fb], np.uint8)
        hashes.append("%016x" % R.fnv1a64(frame))
        rows.append([[row.tolist() for row in p[:2]] for p in R.split(fmt, w, h, frame)])
    return {"fnv": hashes, "rows": rows[:1]}, None         # the rows of the first frame only: the hashes pin the rest


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("AMV_REFERENCE", "/root/reference"))
    ap.add_argument("--ffmpeg", help="a reference ffmpeg built earlier with the configure line above")
    ap.add_argument("--jobs", type=int, default=8)
    a = ap.parse_args()
    cases = []
    with tempfile.TemporaryDirectory() as work:
        ffmpeg = a.ffmpeg or build_ffmpeg(a.reference, work, a.jobs)
        inp = os.path.join(work, "in.raw")

        def convert_case(src, dst, sw, sh, dw, dh, kind, seed, chain):
            frames = [R.join(R.make_picture(src, sw, sh, kind, seed + i)) for i in range(FRAMES)]
            np.concatenate(frames).tofile(inp)
            args = ["-f", "rawvideo", "-pix_fmt", R.NAMES[src], "-s", "%dx%d" % (sw, sh), "-i", inp, "-f", "rawvideo", "-pix_fmt", R.NAMES[dst]]
            if (sw, sh) != (dw, dh):
                args += ["-s", "%dx%d" % (dw, dh)]
            case = {"src": R.NAMES[src], "dst": R.NAMES[dst], "src_size": [sw, sh], "dst_size": [dw, dh], "frames": FRAMES,
                    "input": {"kind": kind, "seed": seed}, "chain": chain}
            data, err = run(ffmpeg, work, args)
            desc = None
            if data is not None:
                desc, err = describe(dst, dw, dh, data, FRAMES)
            if desc is None:
                case.update({"pinned_by": "restatement", "refusal": err})
            else:
                case.update({"pinned_by": "reference"}, **desc)
            cases.append(case)

        seed = 1000
        for src, dst in R.supported_pairs():
            # the reference defines every output byte at odd sizes only on the routes whose routines have tail code
            odd = R.route(src, dst) in ("gray", "rgb_out")
            for (w, h), kind in ((EVEN, "noise"), (ODD if odd else EVEN2, "noise"), (EVEN, "ramp")):
                seed += 7
                convert_case(src, dst, w, h, w, h, kind, seed, False)
        for src in (R.YUV420P, R.YUV422P, R.YUYV422, R.RGB24):
            seed += 7
            convert_case(src, R.YUVJ420P, 352, 288, 160, 120, "noise", seed, True)
            seed += 7
            convert_case(src, R.YUVJ420P, 352, 288, 160, 120, "ramp", seed, True)
        clip = os.path.join(HERE, "AMV1.amv")
        for dst in (R.YUV420P, R.RGB24):
            data, err = run(ffmpeg, work, ["-i", clip, "-an", "-vframes", "4", "-f", "rawvideo", "-pix_fmt", R.NAMES[dst]])
            case = {"clip": "AMV1.amv", "dst": R.NAMES[dst], "frames": 4}
            if data is None:
                case.update({"pinned_by": "restatement", "refusal": err})
            else:
                case.update({"pinned_by": "reference", "bytes": len(data),
                             "fnv": ["%016x" % R.fnv1a64(data[i * (len(data) // 4):(i + 1) * (len(data) // 4)]) for i in range(4)]})
            cases.append(case)
    doc = {"about": "outputs of the reference's ffmpeg command line (img_convert / sws_scale shim); made by make_ref_img_convert_golden.py",
           "configure": " ".join(CONFIGURE[1:]), "cases": cases}
    with open(os.path.join(HERE, "ref_img_convert.json"), "w") as f:
        json.dump(doc, f, separators=(",", ":"))
    pinned = sum(c["pinned_by"] == "reference" for c in cases)
    print("%d cases, %d pinned by the reference, %d by the restatement alone" % (len(cases), pinned, len(cases) - pinned))
    for c in cases:
        if c["pinned_by"] != "reference":
            print("  not pinned:", c.get("src", c.get("clip")), "->", c["dst"], c.get("src_size"), c["refusal"])


if __name__ == "__main__":
    main()
