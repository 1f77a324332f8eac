#!/usr/bin/env python3
"""Kernel timing of the audio resampler (amvhip_audio_resample_batch_dev) on the cases of DESIGN §4 / §7.1: kernel ms from
the HIP events the library records around its two launches (median of --steps calls), GB/s over the algorithmic bytes
2 * ch_in * N_in + 2 * ch_out * N_out and the fraction of the 8 TB/s HBM roof, beside the CPU restatement
(tests/audio_resample_ref.py, numpy) timed on one stream and scaled to the case.  Stream 0 of every case is checked against
the restatement.  One JSON line per case."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402
import audio_resample_ref as R  # noqa: E402

CASES = (("44.1k stereo -> 22.05k mono, 1000 x 10 s", 1000, 2, 44100, 1),
         ("48k mono -> 22.05k mono, 1000 x 10 s", 1000, 1, 48000, 1),
         ("44.1k stereo -> 22.05k mono, 8 x 10 s", 8, 2, 44100, 1),
         ("48k mono -> 22.05k mono, 8 x 10 s", 8, 1, 48000, 1))

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--seconds", type=float, default=10.0)
a = ap.parse_args()
pkg = entry.load_package()
ctx = pkg.Context(0)
dev = "cuda:0"
s = torch.cuda.current_stream().cuda_stream
for name, n, in_ch, in_rate, out_ch in CASES:
    frames = int(a.seconds * in_rate)
    n_out = pkg.audio_resample_out_samples(in_rate, 22050, frames)
    pcm = torch.empty(n * frames * in_ch, dtype=torch.int16, device=dev)
    ctx.synth_audio_dev(0xA11CE, 0, pcm.numel(), pcm, s)
    pcm_offs = torch.arange(n, dtype=torch.int64, device=dev) * (frames * in_ch)
    nsamp = torch.full((n,), frames, dtype=torch.int64, device=dev)
    out_offs = torch.arange(n, dtype=torch.int64, device=dev) * (n_out * out_ch)
    out = torch.zeros(n * n_out * out_ch, dtype=torch.int16, device=dev)
    per = []
    for it in range(a.steps + 2):
        ctx.prof_enable(it >= 2)
        ctx.prof_reset()
        ctx.audio_resample_batch_dev(pcm, pcm_offs, nsamp, n, in_ch, in_rate, out, out_offs, out_ch, 22050, s)
        torch.cuda.synchronize()
        if it >= 2:
            per.append(ctx.prof_read(pkg.K_AUDIO_RESAMPLE)[1])
    ctx.prof_enable(False)
    ms = float(np.median(per))
    x0 = pcm[: frames * in_ch].cpu().numpy()
    t0 = time.perf_counter()
    want = R.resample_whole(x0, in_ch, in_rate, out_ch, 22050)
    cpu_ms = (time.perf_counter() - t0) * 1e3
    exact = out[: n_out * out_ch].cpu().numpy().tobytes() == want.tobytes()
    nbytes = n * (2 * in_ch * frames + 2 * out_ch * n_out)
    gbs = nbytes / (ms * 1e-3) / 1e9
    print(json.dumps({"case": name, "device": torch.cuda.get_device_name(0), "streams": n, "in_frames": frames, "out_frames": n_out,
                      "filter_length": R.filter_length(in_rate, 22050), "kernel_ms_median": round(ms, 4),
                      "kernel_ms_min": round(min(per), 4), "kernel_ms_max": round(max(per), 4), "algorithmic_GB": round(nbytes / 1e9, 4),
                      "GB_per_s": round(gbs, 1), "fraction_of_8TBps": round(gbs / 8000, 3),
                      "cpu_restatement_ms_one_stream": round(cpu_ms, 1), "cpu_restatement_ms_scaled": round(cpu_ms * n, 1),
                      "stream0_exact": exact}), flush=True)
    del pcm, out
ctx.close()
