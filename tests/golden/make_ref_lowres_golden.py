"""Writes tests/golden/ref_lowres.json: what the REAL reference's `-lowres 1|2|3` makes of JPEG stills, through its own
command line.

    python tests/golden/make_ref_lowres_golden.py [--reference DIR] [--ffmpeg BINARY] [--jobs N]

The reference's ffmpeg is copied to a temporary directory and built there as make_ref_img_convert_golden.py does; nothing of
it enters this repository.  A still is the bytes of amvhip_jpeg_header(h, w) followed by a chunk's scan (the chunk without
its FF D8): chunks of tests/golden/AMV1.amv and seeded chunks from the oracle's encoder at 48x32 and 37x23.  Every case is

    ffmpeg -lowres L -i still.jpg -cropright CR -cropbottom CB -f rawvideo -pix_fmt yuvj420p out.raw

-- the reference's ordinary MJPEG path, top-down, whose lowres works (the AMV decoder's does not: include/amvhip.h).  The
crop is what makes the command line hand the reduced picture out as it is: ffmpeg.c sets lowres after it has read the
stream's size (:2643, :2687-2699), so without it the output keeps the full size and reads the small picture as a large
one, and with -s it rescales a picture that is small already.  Cropped by the difference (:1651-1658: no rescaler, the
picture's top-left corner) the output is the decoder's picture; the crops must be even, so where full - reduced is odd the
output is one column or row short of it ("out_size" of the case).  An odd-sized output holds its chroma as ffmpeg's picture
copy makes it, (width >> 1) x (height >> 1) samples tight behind the luma (the rawvideo writer then counts (width + 1) >> 1
and pads with what the buffer held), so the chroma planes are kept at out_size / 2, rounded down, and read from there.
The fixture keeps the FNV-1a-64 hash of the kept planes and the first two rows of each.  tests/test_lowres_ref.py
makes the same stills again and compares tests/lowres_ref.py with them."""
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
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402
import lowres_ref as R  # noqa: E402
from make_ref_img_convert_golden import build_ffmpeg  # noqa: E402

AMV1_FRAMES = (0, 1, 7, 23, 50, 77, 101, 128, 160, 199, 230, 251)
SYNTH = ((48, 32, 0x10E5, 0), (48, 32, 0x10E5, 5), (37, 23, 0x10E6, 0), (37, 23, 0x10E6, 3))    # (w, h, seed, frame)


def stills(pkg, orc):
    """[(description, w, h, chunk)]: the same list the test makes"""
    amv = orc.parse_amv(open(os.path.join(HERE, "AMV1.amv"), "rb").read())
    w, h = int(amv[0]["width"]), int(amv[0]["height"])
    out = [({"clip": "AMV1.amv", "frame": k}, w, h, bytes(amv[1][k])) for k in AMV1_FRAMES]
    for w, h, seed, t in SYNTH:   # (the encoder wants even sizes: the frame is made with whole MCUs, the still claims w x h)
        ew, eh = (w + 15) // 16 * 16, (h + 15) // 16 * 16
        out.append(({"synth": {"seed": seed, "frame": t}}, w, h, bytes(orc.encode_frame(orc.synth_frame(seed, t, ew, eh), ew, eh))))
    return out


def still_bytes(pkg, w, h, chunk):
    lib = pkg.load_library()
    hdr = np.zeros(lib.amvhip_jpeg_header(h, w, None, 0), np.uint8)
    lib.amvhip_jpeg_header(h, w, hdr.ctypes.data, hdr.size)
    assert chunk[:2] == b"\xff\xd8"
    return hdr.tobytes() + chunk[2:]


def output_planes(data, ow, oh):
    """the planes of an ow x oh output of the command line as it lays them out: Y, then Cb and Cr of (ow >> 1) x (oh >> 1)"""
    cw, ch = ow // 2, oh // 2
    y, c = data[: ow * oh].reshape(oh, ow), data[ow * oh: ow * oh + 2 * cw * ch].reshape(2, ch, cw)
    return [y, c[0], c[1]]


def kept_planes(planes, ow, oh):
    """... and the same cut of the restatement's planes"""
    return [planes[0][:oh, :ow], planes[1][:oh // 2, :ow // 2], planes[2][:oh // 2, :ow // 2]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("AMV_REFERENCE", "/root/reference"))
    ap.add_argument("--ffmpeg", help="a reference ffmpeg built earlier with the configure line of make_ref_img_convert_golden.py")
    ap.add_argument("--jobs", type=int, default=8)
    a = ap.parse_args()
    pkg, orc = entry.load_package(), entry.load_oracle()
    cases = []
    with tempfile.TemporaryDirectory() as work:
        ffmpeg = a.ffmpeg or build_ffmpeg(a.reference, work, a.jobs)
        jpg, out = os.path.join(work, "still.jpg"), os.path.join(work, "out.raw")
        for desc, w, h, chunk in stills(pkg, orc):
            open(jpg, "wb").write(still_bytes(pkg, w, h, chunk))
            for L in (1, 2, 3):
                if os.path.exists(out):
                    os.remove(out)
                cr, cb = (w - R.dim(w, L) + 1) & ~1, (h - R.dim(h, L) + 1) & ~1
                sizes = R.sizes_420(w - cr, h - cb)
                p = subprocess.run([ffmpeg, "-lowres", str(L), "-i", jpg, "-cropright", str(cr), "-cropbottom", str(cb), "-f", "rawvideo",
                                    "-pix_fmt", "yuvj420p", "-y", out], cwd=work, capture_output=True, text=True)
                if p.returncode != 0 or not os.path.exists(out):
                    raise SystemExit("the reference refused %r at lowres %d: %s" % (desc, L, (p.stderr.strip().splitlines() or ["failed"])[-1]))
                data = np.fromfile(out, np.uint8)
                if data.size != sum(a * b for a, b in sizes):
                    raise SystemExit("%r at lowres %d: %d bytes, %d expected" % (desc, L, data.size, sum(a * b for a, b in sizes)))
                kept = output_planes(data, w - cr, h - cb)
                case = dict(desc, size=[w, h], lowres=L, out_size=[w - cr, h - cb], pinned_by="reference",
                            fnv="%016x" % R.fnv1a64(np.concatenate([p.reshape(-1) for p in kept])), rows=[[row.tolist() for row in p[:2]] for p in kept])
                cases.append(case)
    doc = {"about": "the reference's ffmpeg -lowres L on JPEG stills (header of amvhip_jpeg_header + a chunk's scan); made by "
                    "make_ref_lowres_golden.py", "cases": cases}
    with open(os.path.join(HERE, "ref_lowres.json"), "w") as f:
        json.dump(doc, f, separators=(",", ":"))
    print("%d cases pinned by the reference" % len(cases))


if __name__ == "__main__":
    main()
