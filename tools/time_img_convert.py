#!/usr/bin/env python3
"""Timing of the pixel-format step (amvhip_img_convert_dev and the entries built on it), one JSON line per case.

Routes: kernel ms from the HIP events the library records around its launch (AMVHIP_K_PIXFMT; median of --steps calls after
two warm-up calls), bytes in + out per frame, achieved GB/s and the fraction of the 8 TB/s HBM roof; frame 0 of every route is
checked against the CPU restatement (tests/img_convert_ref.py).

The yardstick (--frames, default 8 000 frames of 640x480 YUV420P -> 160x120): amvhip_encode_fmt_scaled_batch_dev (the whole
shim: rescale with the range step in its store, then the encoder) beside amvhip_encode_yuv420_scaled_batch_dev (the rescaler's
untouched instantiation, then the same encoder: the code path of the commit before the pixel-format step, standing in for a
build of that commit) on the same frames, in the same process, calls alternating; wall time of the
whole call between two events on the stream."""
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
import img_convert_ref as R  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--route-frames", type=int, default=512)
ap.add_argument("--frames", type=int, default=8000)
ap.add_argument("--size", default="640x480")
a = ap.parse_args()
w, h = (int(v) for v in a.size.split("x"))
pkg = entry.load_package()
ctx = pkg.Context(0)
dev = "cuda:0"
st = torch.cuda.current_stream().cuda_stream
name = torch.cuda.get_device_name(0)


def tight(fmt, n, fill):
    """n tight frames on the device, one buffer a plane -> (planes, picture tuple)"""
    shapes = R.plane_shapes(fmt, w, h)
    planes = []
    for r, c in shapes:
        t = torch.empty(n * r * c, dtype=torch.uint8, device=dev)
        if fill:
            t.random_(0, 256)
        planes.append(t)
    stride = [c for _, c in shapes]
    frame = [r * c for r, c in shapes]
    return planes, (planes, stride[0], stride[1] if len(stride) > 1 else 0, frame[0], frame[1] if len(frame) > 1 else 0)


for src, dst in R.supported_pairs():
    n = a.route_frames
    sp, spic = tight(src, n, True)
    dp, dpic = tight(dst, n, False)
    per = []
    for it in range(a.steps + 2):
        ctx.prof_enable(it >= 2)
        ctx.prof_reset()
        ctx.img_convert_dev(src, spic, dst, dpic, w, h, n, st)
        torch.cuda.synchronize()
        if it >= 2:
            per.append(ctx.prof_read(pkg.K_PIXFMT)[1])
    ctx.prof_enable(False)
    ms = float(np.median(per))
    f0 = [p[: r * c].cpu().numpy().reshape(r, c) for p, (r, c) in zip(sp, R.plane_shapes(src, w, h))]
    want = R.join(R.convert(src, f0, dst, w, h))
    got = np.concatenate([p[: r * c].cpu().numpy() for p, (r, c) in zip(dp, R.plane_shapes(dst, w, h))])
    # towards GRAY8 only the luma plane is read
    per_frame = (w * h if dst == R.GRAY8 else R.frame_bytes(src, w, h)) + R.frame_bytes(dst, w, h)
    gbs = per_frame * n / (ms * 1e-3) / 1e9
    print(json.dumps({"case": "%s -> %s" % (R.NAMES[src], R.NAMES[dst]), "device": name, "size": a.size, "frames": n,
                      "bytes_in_plus_out_per_frame": per_frame, "kernel_ms_median": round(ms, 4), "kernel_ms_min": round(min(per), 4),
                      "kernel_ms_max": round(max(per), 4), "GB_per_s": round(gbs, 1), "fraction_of_8TBps": round(gbs / 8000, 3),
                      "frame0_exact": bool((got == want).all())}), flush=True)
    del sp, dp

# ---- the yardstick ---------------------------------------------------------------------------------------------------------
n, ow, oh = a.frames, 160, 120
sp, spic = tight(R.YUV420P, n, True)
cap = ctx.encode_bound(ow, oh) * n
blob = torch.zeros(cap, dtype=torch.uint8, device=dev)
offs = torch.zeros(n, dtype=torch.int64, device=dev)
lens = torch.zeros(n, dtype=torch.int32, device=dev)


def old_call():
    ctx._check(ctx.lib.amvhip_encode_yuv420_scaled_batch_dev(ctx.h, sp[0].data_ptr(), sp[1].data_ptr(), sp[2].data_ptr(), w, w // 2, w * h,
                                                             (w // 2) * (h // 2), w, h, n, ow, oh, 0, blob.data_ptr(), cap, offs.data_ptr(),
                                                             lens.data_ptr(), st), "encode_yuv420_scaled_batch_dev")


def new_call():
    ctx.encode_fmt_scaled_batch_dev(R.YUV420P, spic, w, h, n, ow, oh, 0, blob, cap, offs, lens, st)


times = {"old": [], "new": []}
for it in range(a.steps + 2):
    for key, call in (("old", old_call), ("new", new_call)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        if it >= 2:
            times[key].append(e0.elapsed_time(e1))
old, new = float(np.median(times["old"])), float(np.median(times["new"]))
print(json.dumps({"case": "yardstick: %d frames %s yuv420p -> 160x120 chunks" % (n, a.size), "device": name,
                  "encode_yuv420_scaled_batch_dev_ms_median": round(old, 3), "encode_yuv420_scaled_ms_min_max": [round(min(times["old"]), 3), round(max(times["old"]), 3)],
                  "encode_fmt_scaled_batch_dev_ms_median": round(new, 3), "encode_fmt_scaled_ms_min_max": [round(min(times["new"]), 3), round(max(times["new"]), 3)],
                  "new_over_old": round(new / old, 4)}), flush=True)
ctx.close()
