#!/usr/bin/env python3
"""Times `-trellis N` over one stream of chunks three ways (device events around device-resident calls, a host clock around
the host loop, which synchronises per chunk):
  (a) amvhip_adpcm_encode_trellis_stream_dev: the step index chained on the device;
  (b) amvhip_adpcm_encode_trellis_batch_dev with the true start indices handed in: one pass, no chain -- the floor;
  (c) the loop over amvhip_adpcm_encode_frame_trellis, one chunk per call, the index carried on the host.
All three must write the same bytes, or nothing is reported.  (a) and (b) alternate inside one loop; every shape is warmed
up first.  Prints one JSON line per N and writes them to --out."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--chunks", type=int, default=1000)
ap.add_argument("--samples", type=int, default=1378)
ap.add_argument("--trellis", type=int, nargs="+", default=[3, 5])
ap.add_argument("--reps", type=int, default=7, help="timed repetitions of (a) and (b)")
ap.add_argument("--loop-reps", type=int, default=2, help="timed repetitions of (c)")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_time_adpcm_trellis_stream.jsonl"))
a = ap.parse_args()

pkg = entry.load_package()
lib = pkg.load_library()
assert torch.cuda.is_available(), "a timing needs the GPU"
ctx = pkg.Context(0)
dev = "cuda:0"
n, spf = a.chunks, a.samples & ~1
s = torch.cuda.current_stream().cuda_stream
pcm = torch.empty(n * spf, dtype=torch.int16, device=dev)
ctx.synth_audio_dev(0xA11CE, 0, n * spf, pcm, s)
pcm_offs = torch.arange(n, dtype=torch.int64, device=dev) * spf
nsamp = torch.full((n,), spf, dtype=torch.int32, device=dev)
clen = 8 + spf // 2
offs = torch.arange(n, dtype=torch.int64, device=dev) * clen
torch.cuda.synchronize()
h_pcm = pcm.cpu().numpy()


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


lines = []
for N in a.trellis:
    blob_a = torch.zeros(n * clen, dtype=torch.uint8, device=dev)
    blob_b = torch.zeros(n * clen, dtype=torch.uint8, device=dev)
    ends = torch.zeros(n, dtype=torch.int32, device=dev)
    ends_b = torch.zeros(n, dtype=torch.int32, device=dev)
    run_a = lambda: ctx.adpcm_encode_trellis_stream_dev(pcm, pcm_offs, nsamp, n, 0, N, blob_a, offs, ends, s)
    run_a()
    torch.cuda.synchronize()
    stats = ctx.adpcm_trellis_chain_stats()
    starts = torch.cat([torch.zeros(1, dtype=torch.int32, device=dev), ends[:-1]]).contiguous()

    def run_b():
        rc = lib.amvhip_adpcm_encode_trellis_batch_dev(ctx.h, pcm.data_ptr(), pcm_offs.data_ptr(), nsamp.data_ptr(), n, starts.data_ptr(), N,
                                                       blob_b.data_ptr(), offs.data_ptr(), ends_b.data_ptr(), s)
        assert rc == 0, rc
    run_b()
    torch.cuda.synchronize()
    assert torch.equal(blob_a, blob_b) and torch.equal(ends, ends_b), "the stream call and the one-pass floor differ"
    ta, tb = [], []
    for it in range(a.reps + 1):          # (the first round is the second warm-up)
        x, y = timed(run_a), timed(run_b)
        if it:
            ta.append(x)
            tb.append(y)

    def run_c(count):
        idx = ctypes.c_int32(0)
        out = np.zeros((count, clen), np.uint8)
        for i in range(count):
            seg = h_pcm[i * spf:(i + 1) * spf]
            m = lib.amvhip_adpcm_encode_frame_trellis(ctx.h, seg.ctypes.data, spf, ctypes.byref(idx), N, out[i].ctypes.data, clen)
            assert m == clen, m
            if i % 100 == 99:
                print("  frame loop, N = %d: %d chunks" % (N, i + 1), file=sys.stderr, flush=True)
        return out, idx.value
    run_c(min(n, 8))
    tc = []
    for _ in range(a.loop_reps):
        t0 = time.perf_counter()
        out_c, end_c = run_c(n)
        tc.append((time.perf_counter() - t0) * 1e3)
    assert out_c.reshape(-1).tobytes() == blob_a.cpu().numpy().tobytes() and end_c == int(ends[-1]), "the host loop and the stream call differ"
    A, B, C = spread(ta), spread(tb), spread(tc)
    line = {"device": torch.cuda.get_device_name(0), "chunks": n, "samples": spf, "trellis": N,
            "stream_call": A, "one_pass_floor": B, "frame_loop": C,
            "a_over_b": A["median_ms"] / B["median_ms"], "c_over_a": C["median_ms"] / A["median_ms"],
            "fallback": stats["exhaustive"], "recoded_per_sweep": stats["recoded"],
            "guess_tail_samples": spf - ((spf + 127) // 128 - 2) * 128 if spf > 256 else spf}
    print(json.dumps(line), flush=True)
    lines.append(line)
    assert A["median_ms"] < C["median_ms"], "the stream call is not shorter than the loop it replaces: the chain is not working as designed"
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    for line in lines:
        f.write(json.dumps(line) + "\n")
ctx.close()
