#!/usr/bin/env python3
"""Timing of the -nr encode entry beside the plain YUV420 entry (an experiment's tool, not the bench): the bench's
synthetic stream made on the device, converted to YUVJ420P planes once, then

    plain   amvhip_encode_yuv420_batch_dev
    nr      amvhip_encode_yuv420_nr_stream_dev with --nr (state zeroed before every call), where the library has it

each timed with device events around the call; the median and the fastest of --steps calls are printed as one JSON line.
--lib selects a library build, so that the plain entry can be timed on the parent commit's library and on this one's in
two runs on the same machine (the library is loaded with a table of its own here: an older build lacks the nr entries).

    python tools/time_encode_nr.py [--lib PATH] [--frames 1000] [--width 320] [--height 240] [--nr 300] [--steps 30]

The per-pass split of the nr entry (amv_nr_sums_kernel, amv_nr_chain_kernel, amv_encode_frame_kernel with offsets) is the
kernel trace's: run this tool under `rocprofv3 --kernel-trace --stats -- python tools/time_encode_nr.py`."""
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
ap.add_argument("--nr", type=int, default=300)
ap.add_argument("--steps", type=int, default=30)
a = ap.parse_args()

vp, u32, u64, cint = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
lib = ctypes.CDLL(a.lib)                       # (torch is imported first: one HIP runtime per process)
lib.amvhip_create.argtypes = [ctypes.POINTER(vp), cint]
lib.amvhip_destroy.argtypes = [vp]
lib.amvhip_synth_frames_dev.argtypes = [vp, u32, u32, u32, u32, u32, vp, vp]
lib.amvhip_img_convert_dev.argtypes = [vp, cint, vp, vp, vp, u32, u32, u64, u64, cint, vp, vp, vp, u32, u32, u64, u64, u32, u32, u32, vp]
plain_args = [vp, vp, vp, vp, u32, u32, u64, u64, u32, u32, u32, u32, vp, u64, vp, vp, vp]
lib.amvhip_encode_yuv420_batch_dev.argtypes = plain_args
has_nr = hasattr(lib, "amvhip_encode_yuv420_nr_stream_dev")
if has_nr:
    lib.amvhip_encode_yuv420_nr_stream_dev.argtypes = plain_args[:12] + [u32, vp] + plain_args[12:]
PIX_YUVJ420P, PIX_RGB24 = 1, 8

h_ctx = vp()
assert lib.amvhip_create(ctypes.byref(h_ctx), 0) == 0, "no usable HIP device"
dev = "cuda:0"
w, h, n = a.width, a.height, a.frames
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
state = torch.zeros(65, dtype=torch.int32, device=dev)
head = (h_ctx, Y.data_ptr(), Cb.data_ptr(), Cr.data_ptr(), w, cw, w * h, cw * ch, n, w, h, 0)
tail = (blob.data_ptr(), cap, offs.data_ptr(), lens.data_ptr(), s)


def plain():
    assert lib.amvhip_encode_yuv420_batch_dev(*head, *tail) == 0


def with_nr():
    state.zero_()
    assert lib.amvhip_encode_yuv420_nr_stream_dev(*head, a.nr, state.data_ptr(), *tail) == 0


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
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "mean_chunk": float(lens.sum().item()) / n}


out = {"lib": a.lib, "frames": n, "size": [w, h], "steps": a.steps, "plain": timed(plain)}
if has_nr:
    out["nr"] = dict(timed(with_nr), nr=a.nr)
    out["plain_again"] = timed(plain)          # the drift of the box between the first and the last measurement
torch.cuda.synchronize()
lib.amvhip_destroy(h_ctx)
print(json.dumps(out))
