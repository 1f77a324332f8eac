#!/usr/bin/env python3
"""Timing of the requant entries beside what a caller does without them (an experiment's tool, not the bench): the bench's
synthetic stream made on the device and encoded once by amvhip_encode_batch_dev -- the chunks a user already has -- then

    requant          amvhip_requant_stream_dev at --lambda: chunks in, chunks out
    decode + encode  what a user must do today: amvhip_decode_fmt_batch_dev to YUV420P planes, then
                     amvhip_encode_yuv420_trellis_batch_dev at the same lambda (an IDCT, a clamp, a colour round trip, a second
                     fdct with a second rounding)
    probe, rate      amvhip_requant_rate_probe_dev and amvhip_requant_rate_stream_dev with a ladder of --rungs at a uniform
                     budget = the median length of the requant call's chunks at the middle rung, with the share of frames per
                     rung and the share flagged

each timed with device events around the call(s); the median, the fastest and the slowest of --steps are printed as one JSON
line.  --only picks one measurement, so that the two routes can alternate a process per measurement on one machine.

    python tools/time_requant.py [--only requant|decode_encode|rate] [--frames 1000] [--width 320] [--height 240] [--lambda 3481]
                                 [--rungs 8] [--steps 20]

The split by kernel is the kernel trace's: run this tool under `rocprofv3 --kernel-trace --stats -- python tools/time_requant.py`."""
import argparse
import ctypes
import json
import os
import statistics

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=os.path.join(ROOT, "amv-codec-tools_amd", "libamvhip.so"))
ap.add_argument("--only", default="all", choices=["all", "requant", "decode_encode", "rate"])
ap.add_argument("--frames", type=int, default=1000)
ap.add_argument("--width", type=int, default=320)
ap.add_argument("--height", type=int, default=240)
ap.add_argument("--lambda", dest="lam", type=int, default=3481)
ap.add_argument("--rungs", type=int, default=8)
ap.add_argument("--steps", type=int, default=20)
a = ap.parse_args()

vp, u32, u64, cint = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int


class Rate(ctypes.Structure):
    _fields_ = [("ladder", vp), ("rungs", u32), ("budget", u32), ("d_budget", vp)]


lib = ctypes.CDLL(a.lib)                       # (torch is imported first: one HIP runtime per process)
lib.amvhip_create.argtypes = [ctypes.POINTER(vp), cint]
lib.amvhip_destroy.argtypes = [vp]
lib.amvhip_synth_frames_dev.argtypes = [vp, u32, u32, u32, u32, u32, vp, vp]
lib.amvhip_encode_batch_dev.argtypes = [vp, vp, u32, cint, u32, u32, u32, u32, vp, u64, vp, vp, vp]
lib.amvhip_decode_fmt_batch_dev.argtypes = [vp, vp, u64, vp, vp, u32, u32, u32, u32, cint, vp, u32, vp, vp]
lib.amvhip_encode_yuv420_trellis_batch_dev.argtypes = [vp, vp, vp, vp, u32, u32, u64, u64, u32, u32, u32, u32, u32, vp, u64, vp, vp, vp]
lib.amvhip_requant_stream_dev.argtypes = [vp, vp, u64, vp, vp, u32, u32, u32, u32, vp, u64, vp, vp, vp, vp, vp]
lib.amvhip_requant_rate_probe_dev.argtypes = [vp, vp, u64, vp, vp, u32, u32, u32, vp, u32, vp, vp]
lib.amvhip_requant_rate_stream_dev.argtypes = [vp, vp, u64, vp, vp, u32, u32, u32, ctypes.POINTER(Rate), vp, u64, vp, vp, vp, vp, vp]
lib.amvhip_encode_trellis_lambda_max.restype = u32
PIX_YUV420P = 0
FLAG_FFMPEG = 2
OVER = 0x80000000

h_ctx = vp()
assert lib.amvhip_create(ctypes.byref(h_ctx), 0) == 0, "no usable HIP device"
dev = "cuda:0"
w, h, n, rungs = a.width, a.height, a.frames, a.rungs
cw, ch = w // 2, h // 2
s = torch.cuda.current_stream().cuda_stream
cap = max(1 << 20, n * w * h)


def outputs():
    return (torch.zeros(cap, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.int64, device=dev),
            torch.zeros(n, dtype=torch.int32, device=dev))


# the chunks a user already has
rgb = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
assert lib.amvhip_synth_frames_dev(h_ctx, 0xA11CE, 0, n, w, h, rgb.data_ptr(), s) == 0
src, src_offs, src_lens = outputs()
assert lib.amvhip_encode_batch_dev(h_ctx, rgb.data_ptr(), w * 3, 0, n, w, h, 0, src.data_ptr(), cap, src_offs.data_ptr(), src_lens.data_ptr(), s) == 0
torch.cuda.synchronize()
del rgb
src_bytes = int(src_lens.to(torch.int64).sum().item())
chunks = (h_ctx, src.data_ptr(), src_bytes, src_offs.data_ptr(), src_lens.data_ptr(), n, w, h)

blob, offs, lens = outputs()
tail = (blob.data_ptr(), cap, offs.data_ptr(), lens.data_ptr())
status = torch.zeros(n, dtype=torch.int32, device=dev)
rung = torch.zeros(n, dtype=torch.int32, device=dev)
bits = torch.zeros((n, rungs), dtype=torch.int32, device=dev)
planes = torch.empty((n, w * h + 2 * cw * ch), dtype=torch.uint8, device=dev)
top = min(52259, lib.amvhip_encode_trellis_lambda_max())
ladder = [top * r * r // max(1, (rungs - 1) ** 2) for r in range(rungs)]
c_ladder = (u32 * rungs)(*ladder)


def requant(lam=None):
    assert lib.amvhip_requant_stream_dev(*chunks, a.lam if lam is None else lam, *tail, status.data_ptr(), None, s) == 0


def decode_encode():
    assert lib.amvhip_decode_fmt_batch_dev(*chunks, FLAG_FFMPEG, PIX_YUV420P, planes.data_ptr(), w, status.data_ptr(), s) == 0
    y = planes.data_ptr()
    assert lib.amvhip_encode_yuv420_trellis_batch_dev(h_ctx, y, y + w * h, y + w * h + cw * ch, w, cw, planes.shape[1], planes.shape[1], n, w, h,
                                                      0, a.lam, *tail, s) == 0


def probe():
    assert lib.amvhip_requant_rate_probe_dev(*chunks, ctypes.addressof(c_ladder), rungs, bits.data_ptr(), s) == 0


def rate(budget):
    r = Rate(ctypes.addressof(c_ladder), rungs, budget, None)
    assert lib.amvhip_requant_rate_stream_dev(*chunks, ctypes.byref(r), *tail, status.data_ptr(), rung.data_ptr(), s) == 0


def timed(call):
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


out = {"frames": n, "size": [w, h], "steps": a.steps, "lambda": a.lam, "source_mean_chunk": src_bytes / n}
if a.only in ("all", "requant"):
    out["requant"] = timed(requant)
    torch.cuda.synchronize()
    out["requant"].update({"mean_chunk": float(lens.sum().item()) / n, "not_coded": int((status != 0).sum().item())})
if a.only in ("all", "decode_encode"):
    out["decode_encode"] = timed(decode_encode)
    torch.cuda.synchronize()
    out["decode_encode"]["mean_chunk"] = float(lens.sum().item()) / n
if a.only in ("all", "rate"):
    requant(ladder[rungs // 2])
    torch.cuda.synchronize()
    budget = int(lens.to(torch.int64).median().item())
    out.update({"ladder": ladder, "budget": budget, "probe": timed(probe), "rate": timed(lambda: rate(budget))})
    torch.cuda.synchronize()
    got = rung.cpu().numpy().view("uint32")
    landed = got & (OVER - 1)
    out["rate"].update({"mean_chunk": float(lens.sum().item()) / n, "over_share": float(((got & OVER) != 0).mean()),
                        "rung_share": [round(float((landed == r).mean()), 4) for r in range(rungs)]})
if a.only in ("all", "requant"):
    out["requant_again"] = timed(requant)
torch.cuda.synchronize()
lib.amvhip_destroy(h_ctx)
print(json.dumps(out))
