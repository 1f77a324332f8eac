#!/usr/bin/env python3
"""Timing of the clip entry beside the rate entry it stands on (an experiment's tool, not the bench): tools/time_encode_rate.py's
set-up -- the bench's synthetic stream made on the device, converted to YUVJ420P planes once, the ascending ladder -- then

    rate, no redo     amvhip_encode_yuv420_rate_stream_dev at a budget nothing exceeds: every frame on rung 0
    clip, no bump     amvhip_encode_yuv420_clip_stream_dev with no cap per frame at a total nothing exceeds: the same chunks; on
                      top of the rate call the floor, start and settle kernels and the pass groups that find nothing to do
    clip, one bump    at total = S(0) - 1: every frame coded at rung 0, the sum a byte over, the clip moves to the next rung that
                      fits and codes the frames again -- beside `rate, tail`: the rate call on the ladder from that rung on,
                      which writes the same chunks in one pass
    rate, median      the rate call at a uniform budget = the median of d_lens at the middle rung (time_encode_rate.py's `rate`)
    clip, that sum    the clip call, no cap per frame, at the sum of the lengths `rate, median` wrote -- with its clip rung, its
                      sum, and beside it the rate call on the ladder's tail from that rung
    one rung          the rate call and the clip call with the ladder [ladder[0]]: no redo pass in either, so
                      clip_kernels_ms = their difference (floor + start + settle), and
                      empty_groups_ms = (clip, no bump - rate, no redo) - clip_kernels_ms: what the clip call's extra empty pass
                      groups cost -- rungs (rungs + 1) / 2 - 1 of them against the rate call's rungs - 1

each timed with device events around the call; the median and the fastest of --steps are printed as one JSON line.

    python tools/time_encode_clip.py [--lib PATH] [--frames 1000] [--width 320] [--height 240] [--rungs 8] [--steps 20]

The split by kernel is the kernel trace's: run this tool under `rocprofv3 --kernel-trace --stats -- python tools/time_encode_clip.py`."""
import argparse
import ctypes
import json
import os
import statistics

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=os.path.join(ROOT, "amv-codec-tools_amd", "libamvhip.so"))
ap.add_argument("--frames", type=int, default=1000)
ap.add_argument("--width", type=int, default=320)
ap.add_argument("--height", type=int, default=240)
ap.add_argument("--rungs", type=int, default=8)
ap.add_argument("--steps", type=int, default=20)
a = ap.parse_args()

vp, u32, u64, cint = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int


class Quant(ctypes.Structure):
    _fields_ = [("qbias", u32), ("nr", u32), ("trellis", u32), ("lambda_", u32), ("d_state", vp)]


class Rate(ctypes.Structure):
    _fields_ = [("ladder", vp), ("rungs", u32), ("budget", u32), ("d_budget", vp)]


lib = ctypes.CDLL(a.lib)                       # (torch is imported first: one HIP runtime per process)
lib.amvhip_create.argtypes = [ctypes.POINTER(vp), cint]
lib.amvhip_destroy.argtypes = [vp]
lib.amvhip_synth_frames_dev.argtypes = [vp, u32, u32, u32, u32, u32, vp, vp]
lib.amvhip_img_convert_dev.argtypes = [vp, cint, vp, vp, vp, u32, u32, u64, u64, cint, vp, vp, vp, u32, u32, u64, u64, u32, u32, u32, vp]
planes_args = [vp, vp, vp, vp, u32, u32, u64, u64, u32, u32, u32]
lib.amvhip_encode_yuv420_trellis_batch_dev.argtypes = planes_args + [u32, u32, vp, u64, vp, vp, vp]
lib.amvhip_encode_trellis_lambda_max.restype = u32
lib.amvhip_encode_yuv420_rate_stream_dev.argtypes = planes_args + [ctypes.POINTER(Quant), ctypes.POINTER(Rate), vp, u64, vp, vp, vp, vp]
lib.amvhip_encode_yuv420_clip_stream_dev.argtypes = planes_args + [ctypes.POINTER(Quant), ctypes.POINTER(Rate), u64, vp, u64, vp, vp, vp, vp, vp]
PIX_YUVJ420P, PIX_RGB24 = 1, 8
OVER = 0x80000000
NO_CAP, EVERYTHING = 0xFFFFFFFF, (1 << 64) - 1

h_ctx = vp()
assert lib.amvhip_create(ctypes.byref(h_ctx), 0) == 0, "no usable HIP device"
dev = "cuda:0"
w, h, n, rungs = a.width, a.height, a.frames, a.rungs
cw, ch = w // 2, h // 2
s = torch.cuda.current_stream().cuda_stream
rgb = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
Y = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
Cb = torch.empty((n, ch, cw), dtype=torch.uint8, device=dev)
Cr = torch.empty((n, ch, cw), dtype=torch.uint8, device=dev)
assert lib.amvhip_synth_frames_dev(h_ctx, 0xA11CE, 0, n, w, h, rgb.data_ptr(), s) == 0
assert lib.amvhip_img_convert_dev(h_ctx, PIX_RGB24, rgb.data_ptr(), None, None, w * 3, 0, w * 3 * h, 0, PIX_YUVJ420P, Y.data_ptr(),
                                  Cb.data_ptr(), Cr.data_ptr(), w, cw, w * h, cw * ch, w, h, n, s) == 0
cap = max(1 << 20, n * w * h)
blob = torch.zeros(cap, dtype=torch.uint8, device=dev)
offs = torch.zeros(n, dtype=torch.int64, device=dev)
lens = torch.zeros(n, dtype=torch.int32, device=dev)
rung = torch.zeros(n, dtype=torch.int32, device=dev)
clip = torch.zeros(2, dtype=torch.int64, device=dev)
planes = (h_ctx, Y.data_ptr(), Cb.data_ptr(), Cr.data_ptr(), w, cw, w * h, cw * ch, n, w, h)
tail = (blob.data_ptr(), cap, offs.data_ptr(), lens.data_ptr())
# time_encode_rate.py's ladder: ascending from 0 to the reference's lambda for qscale 31 (52 259), quadratic
top = min(52259, lib.amvhip_encode_trellis_lambda_max())
ladder = [top * r * r // max(1, (rungs - 1) ** 2) for r in range(rungs)]
c_ladder = (u32 * rungs)(*ladder)
quant = Quant(0, 0, 1, 0, None)


def rate_of(budget, first=0, count=None):
    return Rate(ctypes.addressof(c_ladder) + 4 * first, (count or rungs - first), budget, None)


def rate_call(budget, first=0, count=None):
    r = rate_of(budget, first, count)
    assert lib.amvhip_encode_yuv420_rate_stream_dev(*planes, ctypes.byref(quant), ctypes.byref(r), *tail, rung.data_ptr(), s) == 0


def clip_call(total, count=None):
    r = rate_of(NO_CAP, 0, count)
    assert lib.amvhip_encode_yuv420_clip_stream_dev(*planes, ctypes.byref(quant), ctypes.byref(r), total, *tail, rung.data_ptr(),
                                                    clip.data_ptr(), s) == 0


def clip_record():
    torch.cuda.synchronize()
    c, S = (int(x) & (1 << 64) - 1 for x in clip.cpu().numpy())
    return {"rung": c & (OVER - 1), "over": bool(c & OVER), "sum": S}


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
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4)}


out = {"lib": a.lib, "frames": n, "size": [w, h], "steps": a.steps, "ladder": ladder, "groups": rungs * (rungs + 1) // 2 - 1}
out["rate_no_redo"] = timed(lambda: rate_call(NO_CAP))
out["clip_no_bump"] = timed(lambda: clip_call(EVERYTHING))
out["clip_no_bump"].update(clip_record())
at_zero = out["clip_no_bump"]["sum"]
out["clip_one_bump"] = timed(lambda: clip_call(at_zero - 1))
out["clip_one_bump"].update(clip_record())
bumped = out["clip_one_bump"]["rung"]
out["rate_tail_of_one_bump"] = timed(lambda: rate_call(NO_CAP, bumped))

assert lib.amvhip_encode_yuv420_trellis_batch_dev(*planes, 0, ladder[rungs // 2], *tail, s) == 0
torch.cuda.synchronize()
budget = int(lens.to(torch.int64).median().item())
out["budget"] = budget
out["rate_median"] = timed(lambda: rate_call(budget))
torch.cuda.synchronize()
that_sum = int(lens.to(torch.int64).sum().item())
got = rung.cpu().numpy().view("uint32") & (OVER - 1)
out["rate_median"].update({"sum": that_sum, "rung_share": [round(float((got == r).mean()), 4) for r in range(rungs)]})
out["clip_that_sum"] = timed(lambda: clip_call(that_sum))
out["clip_that_sum"].update(clip_record())
landed = out["clip_that_sum"]["rung"]
out["rate_tail_of_that_sum"] = timed(lambda: rate_call(NO_CAP, landed))

out["rate_one_rung"] = timed(lambda: rate_call(NO_CAP, 0, 1))
out["clip_one_rung"] = timed(lambda: clip_call(EVERYTHING, 1))
out["clip_kernels_ms"] = round(out["clip_one_rung"]["median_ms"] - out["rate_one_rung"]["median_ms"], 4)
out["empty_groups_ms"] = round(out["clip_no_bump"]["median_ms"] - out["rate_no_redo"]["median_ms"] - out["clip_kernels_ms"], 4)
out["rate_no_redo_again"] = timed(lambda: rate_call(NO_CAP))
torch.cuda.synchronize()
lib.amvhip_destroy(h_ctx)
print(json.dumps(out))
