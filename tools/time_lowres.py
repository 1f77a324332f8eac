#!/usr/bin/env python3
"""Kernel-level timing of the reduced-size decode against the full-size FFmpeg-compat decode (not the bench): builds the
synthetic stream on the device as time_kernels.py does, then times the entropy stage and AMVHIP_K_RECON with HIP events
through the library's own profiling hooks (amvhip_prof_read) for the full-size mode and lowres 1, 2, 3 -- each `--runs`
times, `--steps` calls a run, after two warm-up calls.  Prints one JSON line per (mode, run) and a table last; --out
writes the table to a file.  AMVHIP_LIB selects a library build."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=160000)
ap.add_argument("--width", type=int, default=160)
ap.add_argument("--height", type=int, default=120)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--out", default="")
a = ap.parse_args()
pkg = entry.load_package()
ctx = pkg.Context(0)
dev = "cuda:0"
w, h, n = a.width, a.height, a.frames
s = torch.cuda.current_stream().cuda_stream
cap = max(1 << 20, n * w * h)
blob = torch.zeros(cap, dtype=torch.uint8, device=dev)
offs = torch.zeros(n, dtype=torch.int64, device=dev)
lens = torch.zeros(n, dtype=torch.int32, device=dev)
pos = 0
toffs = torch.zeros(2000, dtype=torch.int64, device=dev)
rgb = torch.empty((2000, h, w, 3), dtype=torch.uint8, device=dev)
for lo in range(0, n, 2000):
    cnt = min(2000, n - lo)
    ctx.synth_frames_dev(0xA11CE, lo, cnt, w, h, rgb, s)
    ctx.encode_batch_dev(rgb, w * 3, 0, cnt, w, h, 0, blob[pos:], cap - pos, toffs, lens[lo:], s)
    torch.cuda.synchronize()
    offs[lo:lo + cnt] = toffs[:cnt] + pos
    pos = (int(offs[lo + cnt - 1]) + int(lens[lo + cnt - 1]) + 3) & ~3
del rgb
st = torch.empty(n, dtype=torch.int32, device=dev)
out = torch.empty(n * ctx.yuv420_frame_bytes(w, h), dtype=torch.uint8, device=dev)
ENTROPY = (pkg.K_UNSTUFF, pkg.K_HUFFMAN, pkg.K_HUFFMAN_SERIAL)


def call(L):
    if L == 0:
        ctx.decode_batch_dev(blob, cap, offs, lens, n, w, h, pkg.FLAG_FFMPEG, out, st, s)
    else:
        ctx.decode_lowres_batch_dev(blob, cap, offs, lens, n, w, h, pkg.FLAG_FFMPEG, L, pkg.PIX_YUVJ420P, out, ctx.lowres_dim(w, L), st, s)


rows = []
for L in (0, 1, 2, 3):
    for run in range(a.runs):
        ctx.prof_enable(False)
        for _ in range(2):
            call(L)
        torch.cuda.synchronize()
        ctx.prof_enable(True)
        ctx.prof_reset()
        for _ in range(a.steps):
            call(L)
        torch.cuda.synchronize()
        ent = sum(ctx.prof_read(k)[1] for k in ENTROPY) / a.steps
        rec = ctx.prof_read(pkg.K_RECON)[1] / a.steps
        bytes_out = ctx.yuv420_frame_bytes(w, h) if L == 0 else ctx.lowres_frame_bytes(w, h, L)
        row = {"size": [w, h], "frames": n, "lowres": L, "run": run, "entropy_ms": round(ent, 4), "recon_ms": round(rec, 4),
               "out_bytes_per_frame": int(bytes_out), "bad": int((st != 0).sum())}
        rows.append(row)
        print(json.dumps(row), flush=True)
lines = ["%dx%d x %d frames, %d calls a run; ms per call (entropy = unstuff + huffman + serial huffman; recon = AMVHIP_K_RECON)" % (w, h, n, a.steps),
         "mode        out B/frame  entropy ms (runs)            recon ms (runs)              recon, median  vs full size"]
full = sorted(r["recon_ms"] for r in rows if r["lowres"] == 0)[a.runs // 2]
for L in (0, 1, 2, 3):
    mine = [r for r in rows if r["lowres"] == L]
    med = sorted(r["recon_ms"] for r in mine)[a.runs // 2]
    lines.append("%-11s %11d  %-28s %-28s %13.4f  %11.2fx" % ("full size" if L == 0 else "lowres %d" % L, mine[0]["out_bytes_per_frame"],
                                                               " ".join("%.4f" % r["entropy_ms"] for r in mine),
                                                               " ".join("%.4f" % r["recon_ms"] for r in mine), med, med / full))
print("\n".join(lines))
if a.out:
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n\n")
