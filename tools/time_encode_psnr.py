#!/usr/bin/env python3
"""Timing of the _psnr encode entries beside the entries without, and the "size and error" tables of DESIGN.md made from
d_lens and d_sse in one call per row (an experiment's tool, not the bench).  The bench's synthetic stream is made on the
device as RGB24; per request -- plain, nr, trellis, both --

    old     amvhip_encode_batch_dev / _nr_stream_dev / _trellis_batch_dev / _nr_trellis_stream_dev
    psnr    amvhip_encode_quant_psnr_stream_dev with the same request

each timed with device events around the call (the -nr state zeroed inside the span, for both alike); the median, the
fastest and the slowest of --steps calls are printed as one JSON line.

--table adds the rows of the two tables: qbias 0 and 128, plain and trellis at the lambdas of qscale 1, 2, 4, 8, 16; and at
qbias 0 -nr alone and with lambda 3481 at --nr-rows.  A row is one _psnr call: mean chunk bytes from d_lens, and the
Y / U / V / * figures of amvhip_psnr_report over d_sse.

    python tools/time_encode_psnr.py [--frames 8000] [--width 320] [--height 240] [--nr 300] [--lambda 3481] [--steps 20]
                                     [--table --table-frames 1000 --nr-rows 300,3000]

The split of a _psnr call by kernel is the kernel trace's: run this tool under
`rocprofv3 --kernel-trace --stats -- python tools/time_encode_psnr.py --steps 5`."""
import argparse
import ctypes
import json
import os
import statistics

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=os.path.join(ROOT, "amv-codec-tools_amd", "libamvhip.so"))
ap.add_argument("--frames", type=int, default=8000)
ap.add_argument("--width", type=int, default=320)
ap.add_argument("--height", type=int, default=240)
ap.add_argument("--nr", type=int, default=300)
ap.add_argument("--lambda", dest="lam", type=int, default=3481)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--table", action="store_true")
ap.add_argument("--table-frames", type=int, default=1000)
ap.add_argument("--nr-rows", default="300,3000")
a = ap.parse_args()

vp, u32, u64, cint = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int


class Quant(ctypes.Structure):
    _fields_ = [("qbias", u32), ("nr", u32), ("trellis", u32), ("lam", u32), ("d_state", vp)]


lib = ctypes.CDLL(a.lib)                       # (torch is imported first: one HIP runtime per process)
lib.amvhip_create.argtypes = [ctypes.POINTER(vp), cint]
lib.amvhip_destroy.argtypes = [vp]
lib.amvhip_synth_frames_dev.argtypes = [vp, u32, u32, u32, u32, u32, vp, vp]
plain_args = [vp, vp, u32, cint, u32, u32, u32, u32, vp, u64, vp, vp, vp]
lib.amvhip_encode_batch_dev.argtypes = plain_args
lib.amvhip_encode_nr_stream_dev.argtypes = plain_args[:8] + [u32, vp] + plain_args[8:]
lib.amvhip_encode_trellis_batch_dev.argtypes = plain_args[:8] + [u32] + plain_args[8:]
lib.amvhip_encode_nr_trellis_stream_dev.argtypes = plain_args[:8] + [u32, u32, vp] + plain_args[8:]
lib.amvhip_encode_quant_psnr_stream_dev.argtypes = plain_args[:7] + [vp] + plain_args[8:12] + [vp, vp]
lib.amvhip_psnr_report.argtypes = [vp, u32, u32, u32, vp]
lib.amvhip_psnr_report.restype = None

h_ctx = vp()
assert lib.amvhip_create(ctypes.byref(h_ctx), 0) == 0, "no usable HIP device"
dev = "cuda:0"
w, h = a.width, a.height
n_all = max(a.frames, a.table_frames if a.table else 0)
s = torch.cuda.current_stream().cuda_stream
rgb = torch.empty((n_all, h, w, 3), dtype=torch.uint8, device=dev)
assert lib.amvhip_synth_frames_dev(h_ctx, 0xA11CE, 0, n_all, w, h, rgb.data_ptr(), s) == 0
cap = max(1 << 20, n_all * w * h)
blob = torch.zeros(cap, dtype=torch.uint8, device=dev)
offs = torch.zeros(n_all, dtype=torch.int64, device=dev)
lens = torch.zeros(n_all, dtype=torch.int32, device=dev)
sse = torch.zeros((n_all, 3), dtype=torch.int64, device=dev)
state = torch.zeros(65, dtype=torch.int32, device=dev)


def old(n, qbias, nr, trellis, lam):
    head = (h_ctx, rgb.data_ptr(), w * 3, 0, n, w, h, qbias)
    tail = (blob.data_ptr(), cap, offs.data_ptr(), lens.data_ptr(), s)
    state.zero_()
    if nr and trellis:
        rc = lib.amvhip_encode_nr_trellis_stream_dev(*head, nr, lam, state.data_ptr(), *tail)
    elif nr:
        rc = lib.amvhip_encode_nr_stream_dev(*head, nr, state.data_ptr(), *tail)
    elif trellis:
        rc = lib.amvhip_encode_trellis_batch_dev(*head, lam, *tail)
    else:
        rc = lib.amvhip_encode_batch_dev(*head, *tail)
    assert rc == 0


def psnr(n, qbias, nr, trellis, lam):
    q = Quant(qbias, nr, trellis, lam, state.data_ptr() if nr else None)
    state.zero_()
    assert lib.amvhip_encode_quant_psnr_stream_dev(h_ctx, rgb.data_ptr(), w * 3, 0, n, w, h, ctypes.addressof(q), blob.data_ptr(), cap,
                                                   offs.data_ptr(), lens.data_ptr(), sse.data_ptr(), s) == 0


def timed(call, *args):
    for _ in range(2):
        call(*args)
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call(*args)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def row(n, qbias, nr, trellis, lam):
    """one _psnr call -> mean chunk bytes from d_lens, Y / U / V / * from d_sse"""
    psnr(n, qbias, nr, trellis, lam)
    torch.cuda.synchronize()
    host = sse[:n].cpu().numpy().view("uint64").copy()
    out = (ctypes.c_double * 4)()
    lib.amvhip_psnr_report(host.ctypes.data, n, w, h, ctypes.cast(out, vp))
    return {"qbias": qbias, "nr": nr, "lambda": lam if trellis else None, "mean_chunk": round(float(lens[:n].sum().item()) / n, 1),
            "psnr_y": round(out[0], 3), "psnr_u": round(out[1], 3), "psnr_v": round(out[2], 3), "psnr_all": round(out[3], 3)}


requests = {"plain": (0, 0, 0), "nr": (a.nr, 0, 0), "trellis": (0, 1, a.lam), "both": (a.nr, 1, a.lam)}
lib_name = os.path.relpath(os.path.abspath(a.lib), ROOT)       # (relative to the repository: the record names no machine)
out = {"lib": lib_name if not lib_name.startswith("..") else os.path.basename(a.lib), "frames": a.frames, "size": [w, h], "steps": a.steps, "nr": a.nr, "lambda": a.lam}
for name, req in requests.items():
    out[name] = {"old": timed(old, a.frames, 0, *req), "psnr": timed(psnr, a.frames, 0, *req)}
out["plain_again"] = {"old": timed(old, a.frames, 0, 0, 0, 0)}      # the drift of the box between the first and the last measurement
if a.table:
    n = a.table_frames
    rows = []
    for qbias in (0, 128):
        rows.append(row(n, qbias, 0, 0, 0))
        for lam in (54, 217, 870, 3481, 13924):
            rows.append(row(n, qbias, 0, 1, lam))
    for value in [int(x) for x in a.nr_rows.split(",")]:
        rows.append(row(n, 0, value, 0, 0))
        rows.append(row(n, 0, value, 1, a.lam))
    out["table_frames"] = n
    out["table"] = rows
torch.cuda.synchronize()
lib.amvhip_destroy(h_ctx)
print(json.dumps(out))
