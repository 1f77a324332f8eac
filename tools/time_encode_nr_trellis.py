#!/usr/bin/env python3
"""Timing, size and error of the -nr + trellis encode entry beside its neighbours (an experiment's tool, not the bench): the
bench's synthetic stream made on the device, converted to YUVJ420P planes once, then

    plain     amvhip_encode_yuv420_batch_dev
    nr        amvhip_encode_yuv420_nr_stream_dev at --nr, the state zeroed before every call
    trellis   amvhip_encode_yuv420_trellis_batch_dev at --lambda
    both      amvhip_encode_yuv420_nr_trellis_stream_dev at --nr and --lambda, where the library has it

each timed with device events around the call; the median, the fastest and the slowest of --steps calls are printed as one
JSON line.  --lib selects a library build, so that the existing entries can be timed on the parent commit's library and on
this one's in alternating runs on the same machine (the library is loaded with a table of its own here: an older build lacks
the combined entry).

--table adds, per --nr-rows value at --lambda and --qbias, the mean chunk bytes and the PSNR of amvhip_decode_batch_dev's
pictures against the source pixels, the plain and the trellis entry's first.

    python tools/time_encode_nr_trellis.py [--lib PATH] [--frames 1000] [--width 320] [--height 240] [--nr 300] [--lambda 3481]
                                           [--steps 30] [--table --nr-rows 300,3000 --qbias 0]

The split of the combined entry by kernel is the kernel trace's: run this tool under
`rocprofv3 --kernel-trace --stats -- python tools/time_encode_nr_trellis.py`."""
import argparse
import ctypes
import json
import math
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
ap.add_argument("--lambda", dest="lam", type=int, default=3481)
ap.add_argument("--qbias", type=int, default=0)
ap.add_argument("--nr-rows", default="300,3000")
ap.add_argument("--steps", type=int, default=30)
ap.add_argument("--table", action="store_true")
a = ap.parse_args()

vp, u32, u64, cint = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
lib = ctypes.CDLL(a.lib)                       # (torch is imported first: one HIP runtime per process)
lib.amvhip_create.argtypes = [ctypes.POINTER(vp), cint]
lib.amvhip_destroy.argtypes = [vp]
lib.amvhip_synth_frames_dev.argtypes = [vp, u32, u32, u32, u32, u32, vp, vp]
lib.amvhip_img_convert_dev.argtypes = [vp, cint, vp, vp, vp, u32, u32, u64, u64, cint, vp, vp, vp, u32, u32, u64, u64, u32, u32, u32, vp]
lib.amvhip_decode_batch_dev.argtypes = [vp, vp, u64, vp, vp, u32, u32, u32, u32, vp, vp, vp]
lib.amvhip_stride.restype = u32
lib.amvhip_stride.argtypes = [u32]
plain_args = [vp, vp, vp, vp, u32, u32, u64, u64, u32, u32, u32, u32, vp, u64, vp, vp, vp]
lib.amvhip_encode_yuv420_batch_dev.argtypes = plain_args
lib.amvhip_encode_yuv420_nr_stream_dev.argtypes = plain_args[:12] + [u32, vp] + plain_args[12:]
lib.amvhip_encode_yuv420_trellis_batch_dev.argtypes = plain_args[:12] + [u32] + plain_args[12:]
has_both = hasattr(lib, "amvhip_encode_yuv420_nr_trellis_stream_dev")
if has_both:
    lib.amvhip_encode_yuv420_nr_trellis_stream_dev.argtypes = plain_args[:12] + [u32, u32, vp] + plain_args[12:]
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
tail = (blob.data_ptr(), cap, offs.data_ptr(), lens.data_ptr(), s)
head = (h_ctx, Y.data_ptr(), Cb.data_ptr(), Cr.data_ptr(), w, cw, w * h, cw * ch, n, w, h, a.qbias)


def plain():
    assert lib.amvhip_encode_yuv420_batch_dev(*head, *tail) == 0


def nr(value=None):
    state.zero_()                              # (inside the timed span, for both libraries alike: a 260-byte fill)
    assert lib.amvhip_encode_yuv420_nr_stream_dev(*head, a.nr if value is None else value, state.data_ptr(), *tail) == 0


def trellis():
    assert lib.amvhip_encode_yuv420_trellis_batch_dev(*head, a.lam, *tail) == 0


def both(value=None):
    state.zero_()
    assert lib.amvhip_encode_yuv420_nr_trellis_stream_dev(*head, a.nr if value is None else value, a.lam, state.data_ptr(), *tail) == 0


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
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "mean_chunk": float(lens.sum().item()) / n}


def size_and_psnr():
    """of what the last encode call left in blob / offs / lens"""
    stride = lib.amvhip_stride(w)
    out = torch.zeros((n, h, stride), dtype=torch.uint8, device=dev)
    st = torch.full((n,), -1, dtype=torch.int32, device=dev)
    total = int((offs[-1] + lens[-1]).item())
    assert lib.amvhip_decode_batch_dev(h_ctx, blob.data_ptr(), total, offs.data_ptr(), lens.data_ptr(), n, w, h, 0, out.data_ptr(), st.data_ptr(), s) == 0
    torch.cuda.synchronize()
    assert int(st.abs().sum().item()) == 0, "a chunk did not decode"
    sq = 0.0
    for lo in range(0, n, 100):                # (float64 sums of a hundred frames at a time)
        d = out[lo: lo + 100, :, : w * 3].reshape(-1, h, w, 3).flip(-1).to(torch.float64) - rgb[lo: lo + 100].to(torch.float64)
        sq += float((d * d).sum().item())
    return {"mean_chunk": round(total / n, 1), "psnr_db": round(10.0 * math.log10(255.0 ** 2 / (sq / (n * h * w * 3))), 3)}


out = {"lib": a.lib, "frames": n, "size": [w, h], "steps": a.steps, "nr": a.nr, "lambda": a.lam, "qbias": a.qbias,
       "plain": timed(plain), "nr_entry": timed(nr), "trellis": timed(trellis)}
if has_both:
    out["both"] = timed(both)
out["plain_again"] = timed(plain)              # the drift of the box between the first and the last measurement
if a.table:
    rows = []
    for name, call in (("plain", plain), ("trellis", trellis)):
        call()
        rows.append(dict({"entry": name}, **size_and_psnr()))
    for value in [int(x) for x in a.nr_rows.split(",")]:
        nr(value)
        rows.append(dict({"entry": "nr", "nr": value}, **size_and_psnr()))
        if has_both:
            both(value)
            rows.append(dict({"entry": "both", "nr": value, "lambda": a.lam}, **size_and_psnr()))
    out["table"] = rows
torch.cuda.synchronize()
lib.amvhip_destroy(h_ctx)
print(json.dumps(out))
