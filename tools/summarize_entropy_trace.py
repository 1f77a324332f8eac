#!/usr/bin/env python3
"""tools/time_kernels.py --trace x.npy -> profiles/<tag>.json: what a launch of the several-lanes-per-frame entropy kernel
that is one generation of waves deep lasts as long as.  Per wave (amvhip_entropy_trace): begin / end on the constant-rate
clock, shader clocks of the first walk / the synchronisation rounds / the strict pass, rounds of its worst frame, share
length, workgroup and wave number.  Summarised by wave number inside the workgroup (wave k of a workgroup sits on SIMD
k mod 4: with ten waves per workgroup SIMDs 0 and 1 hold three, and the issue arbiter serves the oldest first) and by rounds.
A trace of the one-lane kernel (a task is 64 frames on one wave; its line carries HW_ID) is summarised by wave number, by the
SIMD the wave ran on and by how many of the workgroup's waves shared that SIMD, with the part of the launch during which a
workgroup's lighter SIMDs (those with fewer of its waves than the fullest) run no task.

    python tools/summarize_entropy_trace.py gpurun_out/r06_trace_10k.npy gpurun_out/r06_trace_10k.json profiles/r06_entropy_trace_10k.json
"""
import json
import sys

import numpy as np

npy, tk_json, out_path = sys.argv[1:4]
tr = np.load(npy)
tr = tr[tr[:, 1] != 0]
t0 = int(tr[:, 0].min())
beg = (tr[:, 0].astype(np.int64) - t0) / 100.0
dur = (tr[:, 1] - tr[:, 0]).astype(np.int64) / 100.0
end = beg + dur
wave = ((tr[:, 7] >> np.uint64(16)) & np.uint64(0xffff)).astype(int)
wg = (tr[:, 7] >> np.uint64(32)).astype(int)
res = json.load(open(tk_json))
res.pop("trace", None)


def idle_share(sel, launch):
    """mean over the workgroups of the part of the launch during which none of the selected tasks of the workgroup runs"""
    shares = []
    for g in np.unique(wg):
        m = sel & (wg == g)
        if not m.any():
            continue
        busy, upto = 0.0, 0.0
        for i in np.argsort(np.where(m, beg, np.inf))[:int(m.sum())]:
            lo, hi = max(beg[i], upto), end[i]
            if hi > lo:
                busy += hi - lo
                upto = hi
        shares.append(1.0 - busy / launch)
    return float(np.mean(shares))


if int(tr[0, 7] & np.uint64(0xffff)) == 1:
    # The one-lane-per-frame kernel: a task is 64 frames on one wave, no phases and no rounds; the question is where the
    # waves run.  The SIMD comes from HW_ID (word 5, bits 4-5); a trace without it falls back on wave number mod 4.
    hw = (tr[:, 5] & np.uint64(0xffffffff)).astype(np.int64)
    simd = np.where(hw != 0, (hw >> 4) & 3, wave % 4).astype(int)
    launch = float(end.max())
    out = {"source": "tools/time_kernels.py --trace (amvhip_entropy_trace), one launch of the one-lane kernel", "time_kernels": res,
           "tasks": int(len(tr)), "workgroups": int(len(np.unique(wg))), "waves_per_workgroup": int(wave.max() + 1),
           "launch_us": launch, "begin_us": {"p50": float(np.median(beg)), "max": float(beg.max())},
           "duration_us": {"p50": float(np.median(dur)), "p99": float(np.percentile(dur, 99)), "max": float(dur.max())},
           "strides": {"min": int(tr[:, 3].min()), "p50": int(np.median(tr[:, 3])), "max": int(tr[:, 3].max())},
           "simd_is_wave_mod_4": round(float((simd == wave % 4).mean()), 4), "by_wave_number": [], "by_simd": []}
    for w in range(wave.max() + 1):
        m = wave == w
        if m.any():
            out["by_wave_number"].append({"wave": w, "simd_mode": int(np.bincount(simd[m]).argmax()), "tasks": int(m.sum()),
                                          "duration_us": round(float(dur[m].mean()), 1), "end_us_mean": round(float(end[m].mean()), 1),
                                          "end_us_max": round(float(end[m].max()), 1), "kclk": round(float(tr[m, 2].astype(np.int64).mean() / 1e3))})
    # waves of a workgroup that share a SIMD: how many, and what that does to a task
    key = wg * 4 + simd
    load = np.bincount(key, minlength=int(key.max()) + 1)[key]
    for s in range(4):
        m = simd == s
        if m.any():
            out["by_simd"].append({"simd": s, "tasks": int(m.sum()), "duration_us": round(float(dur[m].mean()), 1),
                                   "end_us_mean": round(float(end[m].mean()), 1), "end_us_max": round(float(end[m].max()), 1),
                                   "no_task_running_share": round(idle_share(m, launch), 4)})
    out["by_tasks_on_the_simd"] = [{"tasks_on_simd": int(k), "tasks": int((load == k).sum()), "duration_us": round(float(dur[load == k].mean()), 1),
                                    "end_us_mean": round(float(end[load == k].mean()), 1), "end_us_max": round(float(end[load == k].max()), 1)}
                                   for k in np.unique(load)]
    # The SIMDs that carry fewer tasks than their workgroup's fullest (two of the four with ten waves; WHICH two differs from
    # workgroup to workgroup: the hardware places waves 8 and 9, HW_ID says where): when do their tasks end, and for what
    # part of the launch do they run none?
    fullest = np.zeros(int(wg.max()) + 1, int)
    np.maximum.at(fullest, wg, load)
    light = load < fullest[wg]
    if light.any():
        last = [end[light & (wg == g)].max() for g in np.unique(wg) if (light & (wg == g)).any()]
        out["lighter_simds"] = {"tasks": int(light.sum()), "workgroups": len(last), "no_task_running_share": round(idle_share(light, launch), 4),
                                "end_us_mean": round(float(end[light].mean()), 1), "last_end_us": round(float(end[light].max()), 1),
                                "last_end_over_launch": round(float(end[light].max()) / launch, 4),
                                "mean_last_end_per_workgroup_over_launch": round(float(np.mean(last)) / launch, 4)}
    json.dump(out, open(out_path, "w"), indent=1)
    print(json.dumps(out, indent=1)[:6000])
    sys.exit(0)

rounds = (tr[:, 6] & np.uint64(0xffffffff)).astype(int)
share = (tr[:, 6] >> np.uint64(32)).astype(int)
ph = tr[:, 2:6].astype(np.int64) / 1000.0
out ={"source": "tools/time_kernels.py --trace (amvhip_entropy_trace), one launch", "time_kernels": res,
       "waves": int(len(tr)), "workgroups": int(len(np.unique(wg))), "waves_per_workgroup": int(np.bincount(wg).max()),
       "launch_us": float(end.max()), "begin_us": {"p50": float(np.median(beg)), "max": float(beg.max())},
       "duration_us": {"p50": float(np.median(dur)), "p99": float(np.percentile(dur, 99)), "max": float(dur.max())},
       "share_bits": {"min": int(share.min()), "p50": int(np.median(share)), "max": int(share.max())},
       "by_wave_number": [], "by_rounds": [], "last_to_end": []}
for w in range(wave.max() + 1):
    m = wave == w
    out["by_wave_number"].append({"wave": w, "simd": w % 4, "n": int(m.sum()), "duration_us": round(float(dur[m].mean()), 1),
                                  "end_us_max": round(float(end[m].max()), 1),
                                  "kclk": {"first_walk": round(float(ph[m, 0].mean())), "rounds": round(float(ph[m, 1].mean())),
                                           "strict": round(float(ph[m, 2].mean())), "per_round": round(float((ph[m, 1] / np.maximum(rounds[m], 1)).mean()))}})
for r in np.unique(rounds):
    m = rounds == r
    out["by_rounds"].append({"rounds": int(r), "waves": int(m.sum()), "duration_us": round(float(dur[m].mean()), 1),
                             "end_us_max": round(float(end[m].max()), 1)})
for i in np.argsort(-end)[:16]:
    out["last_to_end"].append({"end_us": round(float(end[i]), 1), "begin_us": round(float(beg[i]), 1), "wave": int(wave[i]), "rounds": int(rounds[i]),
                               "share_bits": int(share[i]), "kclk": [int(x) for x in ph[i, :3]]})
# what the launch would last if every wave with more rounds than r had needed only r (its rounds phase scaled down)
out["if_rounds_were_capped"] = {}
for cap in (3, 4, 5):
    d2 = dur - np.where(rounds > cap, ph[:, 1] * (1.0 - cap / np.maximum(rounds, 1)) / 2.4, 0.0)    # kclk at 2.4 GHz -> us
    out["if_rounds_were_capped"][str(cap)] = round(float((beg + d2).max()), 1)
json.dump(out, open(out_path, "w"), indent=1)
print(json.dumps({k: v for k, v in out.items() if k not in ("last_to_end",)}, indent=1)[:3000])
