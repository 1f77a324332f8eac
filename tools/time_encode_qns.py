#!/usr/bin/env python3
"""Timing, size and the encoder's own error of the -qns entry beside the plain YUV420 entry (an experiment's tool, not the
bench): the bench's synthetic stream made on the device, converted to YUVJ420P planes once, then

    plain     amvhip_encode_yuv420_batch_dev
    qns 1 2 3 amvhip_encode_yuv420_qns_stream_dev behind the plain quantiser at --lambda2, where the library has it
    plain     again: the drift of the machine between the first and the last measurement

each timed with device events around the call; the median and the fastest of --steps calls are printed as one JSON line,
for the qns lines with the mean chunk size and the PSNR of the encoder's own error (d_sse through amvhip_psnr_report).
--lib selects a library build, so that the plain entry can be timed on the parent commit's library and on this one's in
alternating runs on the same machine (the library is loaded with a table of its own here: an older build lacks the qns
entries).

    python tools/time_encode_qns.py [--lib PATH] [--frames 1000] [--width 320] [--height 240] [--lambda2 6962] [--steps 30]

The split by kernel is the kernel trace's: run this tool under `rocprofv3 --kernel-trace --stats -- python tools/time_encode_qns.py`."""
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
ap.add_argument("--lambda2", type=int, default=6962)
ap.add_argument("--steps", type=int, default=30)
a = ap.parse_args()

vp, u32, u64, cint = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int


class Quant(ctypes.Structure):
    _fields_ = [("qbias", u32), ("nr", u32), ("trellis", u32), ("lambda_", u32), ("d_state", vp)]


lib = ctypes.CDLL(a.lib)                       # (torch is imported first: one HIP runtime per process)
lib.amvhip_create.argtypes = [ctypes.POINTER(vp), cint]
lib.amvhip_destroy.argtypes = [vp]
lib.amvhip_synth_frames_dev.argtypes = [vp, u32, u32, u32, u32, u32, vp, vp]
lib.amvhip_img_convert_dev.argtypes = [vp, cint, vp, vp, vp, u32, u32, u64, u64, cint, vp, vp, vp, u32, u32, u64, u64, u32, u32, u32, vp]
plain_args = [vp, vp, vp, vp, u32, u32, u64, u64, u32, u32, u32, u32, vp, u64, vp, vp, vp]
lib.amvhip_encode_yuv420_batch_dev.argtypes = plain_args
has_qns = hasattr(lib, "amvhip_encode_yuv420_qns_stream_dev")
if has_qns:
    lib.amvhip_encode_yuv420_qns_stream_dev.argtypes = plain_args[:11] + [ctypes.POINTER(Quant), u32, u32] + plain_args[12:16] + [vp, vp]
    lib.amvhip_psnr_report.argtypes = [vp, u32, u32, u32, vp]
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
sse = torch.zeros((n, 3), dtype=torch.int64, device=dev)
planes = (h_ctx, Y.data_ptr(), Cb.data_ptr(), Cr.data_ptr(), w, cw, w * h, cw * ch, n, w, h)
tail = (blob.data_ptr(), cap, offs.data_ptr(), lens.data_ptr())
quant = Quant(0, 0, 0, 0, None)


def plain():
    assert lib.amvhip_encode_yuv420_batch_dev(*planes, 0, *tail, s) == 0


def qns(level, want_sse=False):
    assert lib.amvhip_encode_yuv420_qns_stream_dev(*planes, ctypes.byref(quant), level, a.lambda2, *tail, sse.data_ptr() if want_sse else None, s) == 0


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


def own_psnr(level):
    qns(level, True)
    torch.cuda.synchronize()
    host = sse.cpu().numpy().view("uint64").copy()
    out = (ctypes.c_double * 4)()
    lib.amvhip_psnr_report(host.ctypes.data, n, w, h, ctypes.cast(out, vp))
    return {"psnr_y": round(out[0], 3), "psnr_all": round(out[3], 3)}


out = {"lib": a.lib, "frames": n, "size": [w, h], "steps": a.steps, "plain": timed(plain)}
if has_qns:
    out["lambda2"] = a.lambda2
    out["qns_0"] = own_psnr(0)
    for level in (1, 2, 3):
        out["qns_%d" % level] = dict(timed(lambda: qns(level)), **own_psnr(level))
    out["plain_again"] = timed(plain)
torch.cuda.synchronize()
lib.amvhip_destroy(h_ctx)
print(json.dumps(out))
