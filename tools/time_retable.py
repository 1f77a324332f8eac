#!/usr/bin/env python3
"""Timing of the re-table stream entry beside its requant sibling (an experiment's tool, not the bench): the bench's synthetic
stream made on the device and encoded once by amvhip_encode_batch_dev, then ONE of

    requant        amvhip_requant_stream_dev at --lambda (with --lib: any build's, the parent commit's as the yardstick)
    retable        amvhip_retable_stream_dev at --lambda with --tables amv (AMV's own: the same search, the same chunks out) or
                   --tables qN (the reference encoder's at -qscale N: the chunks read as if that encoder had written them.  The
                   source chunks are this library's, so their levels are large where AMV's steps are small: against q8 nearly
                   every frame of the synthetic stream leaves the range rule -- not_coded says how many -- against q3 none does)

timed with device events around the call; the median, the fastest and the slowest of --steps are printed as one JSON line.  One
measurement a process, so that builds and entries can alternate on one machine.

    python tools/time_retable.py --only requant|retable [--tables amv|q1..q31] [--lib FILE] [--frames 1000] [--width 320] [--height 240]
                                 [--lambda 3481] [--steps 20]

The split by kernel is the kernel trace's: run this tool under `rocprofv3 --kernel-trace --stats -- python tools/time_retable.py`."""
import argparse
import ctypes
import json
import os
import statistics

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=os.path.join(ROOT, "amv-codec-tools_amd", "libamvhip.so"))
ap.add_argument("--only", required=True, choices=["requant", "retable"])
ap.add_argument("--tables", default="amv", choices=["amv"] + ["q%d" % q for q in range(1, 32)])
ap.add_argument("--frames", type=int, default=1000)
ap.add_argument("--width", type=int, default=320)
ap.add_argument("--height", type=int, default=240)
ap.add_argument("--lambda", dest="lam", type=int, default=3481)
ap.add_argument("--steps", type=int, default=20)
a = ap.parse_args()

vp, u32, u64, cint = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
# AMV's tables, scan order (AmvJpeg.c:30-39, 52-61)
AMV = [[8, 6, 6, 7, 6, 5, 8, 7, 7, 7, 9, 9, 8, 10, 12, 20, 13, 12, 11, 11, 12, 25, 18, 19, 15, 20, 29, 26, 31, 30, 29, 26, 28, 28, 32, 36, 46, 39,
        32, 34, 44, 39, 28, 28, 40, 55, 41, 44, 48, 49, 52, 52, 52, 31, 39, 57, 61, 56, 50, 60, 46, 51, 52, 50],
       [9, 9, 9, 12, 11, 12, 24, 13, 13, 24, 50, 33, 28, 33] + [50] * 50]


class Retable(ctypes.Structure):
    _fields_ = [("tables", vp), ("count", u32), ("d_table_of", vp)]


lib = ctypes.CDLL(a.lib)                       # (torch is imported first: one HIP runtime per process)
lib.amvhip_create.argtypes = [ctypes.POINTER(vp), cint]
lib.amvhip_destroy.argtypes = [vp]
lib.amvhip_synth_frames_dev.argtypes = [vp, u32, u32, u32, u32, u32, vp, vp]
lib.amvhip_encode_batch_dev.argtypes = [vp, vp, u32, cint, u32, u32, u32, u32, vp, u64, vp, vp, vp]
lib.amvhip_requant_stream_dev.argtypes = [vp, vp, u64, vp, vp, u32, u32, u32, u32, vp, u64, vp, vp, vp, vp, vp]

h_ctx = vp()
assert lib.amvhip_create(ctypes.byref(h_ctx), 0) == 0, "no usable HIP device"
dev = "cuda:0"
w, h, n = a.width, a.height, a.frames
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

if a.only == "retable":
    lib.amvhip_retable_stream_dev.argtypes = [vp, vp, u64, vp, vp, u32, u32, u32, ctypes.POINTER(Retable), u32, vp, u64, vp, vp, vp, vp, vp]
    lib.amvhip_ffmpeg_amv_tables.argtypes = [u32, vp]
    c_tables = (ctypes.c_uint8 * 128)(*(AMV[0] + AMV[1]))
    if a.tables != "amv":
        assert lib.amvhip_ffmpeg_amv_tables(int(a.tables[1:]), ctypes.addressof(c_tables)) == 0
    rt = Retable(ctypes.addressof(c_tables), 1, None)


def requant():
    assert lib.amvhip_requant_stream_dev(*chunks, a.lam, *tail, status.data_ptr(), None, s) == 0


def retable():
    assert lib.amvhip_retable_stream_dev(*chunks, ctypes.byref(rt), a.lam, *tail, status.data_ptr(), None, s) == 0


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


out = {"what": a.only + (" " + a.tables if a.only == "retable" else ""), "lib": os.path.relpath(a.lib, ROOT), "frames": n, "size": [w, h],
       "steps": a.steps, "lambda": a.lam, "source_mean_chunk": src_bytes / n}
out.update(timed(requant if a.only == "requant" else retable))
torch.cuda.synchronize()
out.update({"mean_chunk": float(lens.sum().item()) / n, "not_coded": int((status != 0).sum().item())})
lib.amvhip_destroy(h_ctx)
print(json.dumps(out))
