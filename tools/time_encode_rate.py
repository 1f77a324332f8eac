#!/usr/bin/env python3
"""Timing of the rate entry beside what a caller does without it (an experiment's tool, not the bench): the bench's synthetic
stream made on the device, converted to YUVJ420P planes once, then

    trellis x rungs   amvhip_encode_yuv420_trellis_batch_dev once per lambda of the ladder: what a caller on a library without
                      the rate entries pays to learn every frame's size at every rung (the second pass, one more call per
                      distinct lambda chosen, is left out: in that caller's favour)
    probe             amvhip_encode_yuv420_rate_probe_dev: the bits table alone
    rate              amvhip_encode_yuv420_rate_stream_dev at a uniform budget = the median of d_lens at the middle rung, with
                      the share of frames per rung, the share that was flagged, and -- from the probe's bits and the lengths
                      the call returned, nothing else -- the share of frames that took a redo pass (their first floor-fit is
                      not where they landed)
    rate, no redo     the same call at a budget nothing exceeds: every frame lands on rung 0 in the first pass, so the redo
                      launches run empty.  `empty_redo_ms` = (this call - the probe) - (the same call with the one-rung ladder
                      [ladder[0]], which has no redo pass - its probe): the rungs - 1 empty forward + pack + check launches
    trellis x rungs   again: the drift of the machine between the first and the last measurement

each timed with device events around the call(s); the median and the fastest of --steps are printed as one JSON line.  --lib
selects a library build, so that the eight trellis calls can be timed on the parent commit's library and on this one's in
alternating runs on the same machine (the library is loaded with a table of its own here: an older build lacks the rate
entries).

    python tools/time_encode_rate.py [--lib PATH] [--frames 1000] [--width 320] [--height 240] [--rungs 8] [--steps 20]

The split by kernel is the kernel trace's: run this tool under `rocprofv3 --kernel-trace --stats -- python tools/time_encode_rate.py`."""
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
has_rate = hasattr(lib, "amvhip_encode_yuv420_rate_stream_dev")
if has_rate:
    lib.amvhip_encode_yuv420_rate_stream_dev.argtypes = planes_args + [ctypes.POINTER(Quant), ctypes.POINTER(Rate), vp, u64, vp, vp, vp, vp]
    lib.amvhip_encode_yuv420_rate_probe_dev.argtypes = planes_args + [ctypes.POINTER(Quant), vp, u32, vp, vp]
PIX_YUVJ420P, PIX_RGB24 = 1, 8
OVER = 0x80000000

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
bits = torch.zeros((n, rungs), dtype=torch.int32, device=dev)
planes = (h_ctx, Y.data_ptr(), Cb.data_ptr(), Cr.data_ptr(), w, cw, w * h, cw * ch, n, w, h)
tail = (blob.data_ptr(), cap, offs.data_ptr(), lens.data_ptr())
# an ascending ladder from 0 to the reference's lambda for qscale 31 (52 259), quadratic like the reference's own lambda(qscale)
top = min(52259, lib.amvhip_encode_trellis_lambda_max())
ladder = [top * r * r // max(1, (rungs - 1) ** 2) for r in range(rungs)]
c_ladder = (u32 * rungs)(*ladder)
quant = Quant(0, 0, 1, 0, None)


def trellis(lam):
    assert lib.amvhip_encode_yuv420_trellis_batch_dev(*planes, 0, lam, *tail, s) == 0


def every_rung():
    for lam in ladder:
        trellis(lam)


def probe(count=None):
    assert lib.amvhip_encode_yuv420_rate_probe_dev(*planes, ctypes.byref(quant), ctypes.addressof(c_ladder), count or rungs, bits.data_ptr(), s) == 0


def rate(budget, count=None):
    r = Rate(ctypes.addressof(c_ladder), count or rungs, budget, None)
    assert lib.amvhip_encode_yuv420_rate_stream_dev(*planes, ctypes.byref(quant), ctypes.byref(r), *tail, rung.data_ptr(), s) == 0


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


out = {"lib": a.lib, "frames": n, "size": [w, h], "steps": a.steps, "ladder": ladder, "trellis_x_rungs": timed(every_rung)}
if has_rate:
    trellis(ladder[rungs // 2])
    torch.cuda.synchronize()
    budget = int(lens.to(torch.int64).median().item())
    out["budget"] = budget
    out["probe"] = timed(probe)
    out["rate"] = timed(lambda: rate(budget))
    torch.cuda.synchronize()
    got = rung.cpu().numpy().view("uint32")
    floors = 4 + (bits.cpu().numpy().view("uint32").astype("int64") + 7) // 8
    first = [next((r for r in range(rungs) if floors[i][r] <= budget), rungs - 1) for i in range(n)]
    landed = got & (OVER - 1)
    out["rate"].update({"mean_chunk": float(lens.sum().item()) / n, "over_share": float(((got & OVER) != 0).mean()),
                        "redo_share": float((landed != first).mean()),
                        "rung_share": [round(float((landed == r).mean()), 4) for r in range(rungs)]})
    out["rate_no_redo"] = timed(lambda: rate(0xFFFFFFFF))
    out["probe_one_rung"] = timed(lambda: probe(1))
    out["rate_one_rung"] = timed(lambda: rate(0xFFFFFFFF, 1))
    out["empty_redo_ms"] = round((out["rate_no_redo"]["median_ms"] - out["probe"]["median_ms"])
                                 - (out["rate_one_rung"]["median_ms"] - out["probe_one_rung"]["median_ms"]), 4)
    out["trellis_x_rungs_again"] = timed(every_rung)
torch.cuda.synchronize()
lib.amvhip_destroy(h_ctx)
print(json.dumps(out))
