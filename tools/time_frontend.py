#!/usr/bin/env python3
"""Timing of the video front end joined to the encoder, one JSON line per case: --frames (default 1 000) frames of 352x288
YUV420P -> 160x120 chunks, in one process, the calls alternating, wall time of the whole call between two events on the
stream (median, min and max of --steps calls after two warm-up rounds):

    base       amvhip_encode_fmt_scaled_batch_dev (the entry without the stages)
    identity   amvhip_encode_frontend_batch_dev with every field of amvhip_frontend zero: the same path
    letterbox  the same with -deinterlace, -croptop 16 -cropbottom 16, a 160x90 window and -padtop 14 -padbottom 16

and, for base and letterbox, the kernel ms the library's own events record under AMVHIP_K_PIXFMT (deinterlace, rescale, pad
bands) and under the encoder's ids.  Frame 0 of the letterbox picture is checked against the CPU restatement."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402
import frontend_ref as F  # noqa: E402
import img_convert_ref as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=15)
ap.add_argument("--frames", type=int, default=1000)
a = ap.parse_args()
pkg = entry.load_package()
orc = entry.load_oracle()
ctx = pkg.Context(0)
dev = "cuda:0"
st = torch.cuda.current_stream().cuda_stream
n, sw, sh, w, h = a.frames, 352, 288, 160, 120
planes = [torch.empty(n * r * c, dtype=torch.uint8, device=dev).random_(0, 256) for r, c in R.plane_shapes(R.YUV420P, sw, sh)]
pic = (planes, sw, sw // 2, sw * sh, (sw // 2) * (sh // 2))
cap = ctx.encode_bound(w, h) * n
blob = torch.zeros(cap, dtype=torch.uint8, device=dev)
offs = torch.zeros(n, dtype=torch.int64, device=dev)
lens = torch.zeros(n, dtype=torch.int32, device=dev)
bands = ((16, 16, 0, 0), (14, 16, 0, 0))
letterbox = pkg.Frontend(1, *bands)
calls = {"base": lambda: ctx.encode_fmt_scaled_batch_dev(R.YUV420P, pic, sw, sh, n, w, h, 0, blob, cap, offs, lens, st),
         "identity": lambda: ctx.encode_frontend_batch_dev(R.YUV420P, pic, sw, sh, n, pkg.Frontend(), w, h, 0, blob, cap, offs, lens, st),
         "letterbox": lambda: ctx.encode_frontend_batch_dev(R.YUV420P, pic, sw, sh, n, letterbox, w, h, 0, blob, cap, offs, lens, st)}
times = {k: [] for k in calls}
for it in range(a.steps + 2):
    for key, call in calls.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        if it >= 2:
            times[key].append(e0.elapsed_time(e1))
kernels = {}
for key in ("base", "letterbox"):
    per = []
    for it in range(5):
        ctx.prof_enable(True)
        ctx.prof_reset()
        calls[key]()
        torch.cuda.synchronize()
        per.append([ctx.prof_read(k)[1] for k in range(13)])
    ctx.prof_enable(False)
    med = np.median(np.array(per), axis=0)
    kernels[key] = {ctx.lib.amvhip_kernel_name(k).decode(): round(float(med[k]), 4) for k in range(13) if med[k] > 0}
# frame 0 of the letterbox picture
d = [torch.zeros(r * c, dtype=torch.uint8, device=dev) for r, c in R.plane_shapes(R.YUVJ420P, w, h)]
ctx.video_frontend_dev(R.YUV420P, pic, sw, sh, 1, letterbox, (d, w, w // 2, w * h, (w // 2) * (h // 2)), w, h, st)
torch.cuda.synchronize()
f0 = [p[: r * c].cpu().numpy().reshape(r, c) for p, (r, c) in zip(planes, R.plane_shapes(R.YUV420P, sw, sh))]
want = R.join(F.frontend(R.YUV420P, f0, sw, sh, w, h, orc.img_resample_yuv420, True, *bands))
exact = bool((np.concatenate([p.cpu().numpy() for p in d]) == want).all())
med = {k: float(np.median(v)) for k, v in times.items()}
print(json.dumps({"case": "%d frames 352x288 yuv420p -> 160x120 chunks" % n, "device": torch.cuda.get_device_name(0), "steps": a.steps,
                  "ms_median": {k: round(v, 3) for k, v in med.items()},
                  "ms_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in times.items()},
                  "identity_over_base": round(med["identity"] / med["base"], 4),
                  "letterbox_minus_base_ms": round(med["letterbox"] - med["base"], 3),
                  "kernel_ms_median": kernels, "letterbox_frame0_exact": exact}), flush=True)
ctx.close()
