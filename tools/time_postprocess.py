#!/usr/bin/env python3
"""Timing of the decode-side postprocessing beside the decode it follows (not the bench): builds the synthetic stream on the
device as time_kernels.py does, decodes it once into tight YUVJ420P planes, then times amvhip_postprocess_dev for `hb,vb` and
for `de` (forced QP 12, chroma filtered) and amvhip_decode_fmt_batch_dev (to YUV420P) alone on the same frames, at 160x120
and 320x240 -- each `--runs` times, `--steps` calls a run, after two warm-up calls, with HIP events around the calls.  Prints
one JSON line per (size, what, run) and a table last: milliseconds per 1 000 frames, the bytes moved (planes read once, written
once) and the fraction of the HBM roof (--roof GB/s) that is.  --out appends the table to a file.  AMVHIP_LIB selects a build."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=1000)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--roof", type=float, default=8000.0, help="HBM roof, GB/s")
ap.add_argument("--out", default="")
a = ap.parse_args()
pkg = entry.load_package()
ctx = pkg.Context(0)
dev = "cuda:0"
n = a.frames
s = torch.cuda.current_stream().cuda_stream
MODES = (("hb,vb", "hb:c,vb:c,fq:12"), ("de", "de:c,fq:12"))
rows = []


def timed(call):
    for _ in range(2):
        call()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(a.steps):
        call()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / a.steps * 1000.0 / n          # ms per 1 000 frames


for w, h in ((160, 120), (320, 240)):
    cap = max(1 << 20, n * w * h)
    blob = torch.zeros(cap, dtype=torch.uint8, device=dev)
    offs = torch.zeros(n, dtype=torch.int64, device=dev)
    lens = torch.zeros(n, dtype=torch.int32, device=dev)
    rgb = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
    ctx.synth_frames_dev(0xA11CE, 0, n, w, h, rgb, s)
    ctx.encode_batch_dev(rgb, w * 3, 0, n, w, h, 0, blob, cap, offs, lens, s)
    torch.cuda.synchronize()
    del rgb
    fb = ctx.yuv420_frame_bytes(w, h)
    st = torch.empty(n, dtype=torch.int32, device=dev)
    planes = torch.empty(n * fb, dtype=torch.uint8, device=dev)
    cleaned = torch.empty(n * fb, dtype=torch.uint8, device=dev)
    ctx.decode_batch_dev(blob, cap, offs, lens, n, w, h, pkg.FLAG_FFMPEG, planes, st, s)
    torch.cuda.synchronize()
    assert int((st != 0).sum()) == 0

    def pic(t):
        p = t.data_ptr()
        return ([p, p + w * h, p + w * h + (w // 2) * (h // 2)], w, w // 2, fb, fb)

    for run in range(a.runs):
        ms = timed(lambda: ctx.decode_fmt_batch_dev(blob, cap, offs, lens, n, w, h, pkg.FLAG_FFMPEG, pkg.PIX_YUV420P, cleaned, w, st, s))
        rows.append({"size": [w, h], "what": "decode_fmt", "run": run, "ms_per_1000": round(ms, 4)})
        print(json.dumps(rows[-1]), flush=True)
        for name, text in MODES:
            mode = pkg.pp_mode_parse(text)
            ms = timed(lambda: ctx.postprocess_dev(pkg.PIX_YUVJ420P, mode, pic(planes), pic(cleaned), w, h, n, None, s))
            gb = 2.0 * fb * 1000 / 1e9
            rows.append({"size": [w, h], "what": name, "run": run, "ms_per_1000": round(ms, 4), "gb_per_1000": round(gb, 5),
                         "roof_fraction": round(gb / (ms / 1000.0) / a.roof, 5)})
            print(json.dumps(rows[-1]), flush=True)
    del blob, planes, cleaned
lines = ["%d frames, %d calls a run, %d runs; ms per 1 000 frames (median of the runs); roof %.0f GB/s" % (n, a.steps, a.runs, a.roof),
         "size      what         ms / 1000 frames (runs)        median   GB / 1000   of the roof   + on the decode"]
for w, h in ((160, 120), (320, 240)):
    dec = sorted(r["ms_per_1000"] for r in rows if r["size"] == [w, h] and r["what"] == "decode_fmt")[a.runs // 2]
    for what in ("decode_fmt", "hb,vb", "de"):
        mine = [r for r in rows if r["size"] == [w, h] and r["what"] == what]
        med = sorted(r["ms_per_1000"] for r in mine)[a.runs // 2]
        lines.append("%-9s %-12s %-30s %8.4f  %9s  %11s  %14s" % (
            "%dx%d" % (w, h), what, " ".join("%.4f" % r["ms_per_1000"] for r in mine), med,
            "%.4f" % mine[0]["gb_per_1000"] if what != "decode_fmt" else "", "%.2f %%" % (100 * sorted(r["roof_fraction"] for r in mine)[a.runs // 2]) if what != "decode_fmt" else "",
            "+ %.0f %%" % (100 * med / dec) if what != "decode_fmt" else ""))
print("\n".join(lines))
if a.out:
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n\n")
