"""Writes tests/golden/ref_audio_resample.json and ref_audio_resample_crafted.json: outputs of the REAL reference's audio_resample.

    python tests/golden/make_ref_audio_resample_golden.py [--out FILE] [--crafted-out FILE]

The reference's libavcodec/resample.c and resample2.c are compiled where they lie into oracle/_ref/libarref.so (`make -C oracle
ref`; the recipe and oracle/ref_harness_audio.c, the entry point around audio_resample_init / audio_resample /
audio_resample_close, are committed, nothing of the reference is).  This script calls it on the inputs the tests make again:

  ref_audio_resample.json          169 cases on the seeded inputs of tests/audio_resample_ref.py (make_input, packet_sizes): per
                                   rate into 22 050 Hz a grid of the four channel modes, full-scale squares, streams shorter
                                   than the filter; silence; first packets short enough for the mirrored head's `% N` to wrap;
                                   the counts DESIGN.md section 2 quotes
  ref_audio_resample_crafted.json  the crafted streams of tests/audio_resample_builder.py (reference_cases)

Per case: the lengths, the per-call counts (in full where there are at most 8 calls, 16 for the crafted cases), the FNV-1a-64 of
the output bytes and of the counts as int32, and the samples in full where there are at most 64.
tests/test_audio_resample_builder.py::test_fixtures_are_what_the_reference_build_makes makes both again and compares."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))
import audio_resample_ref as R  # noqa: E402
import audio_resample_builder as B  # noqa: E402

LIBRARY = os.path.join(ROOT, "oracle", "_ref", "libarref.so")
RATES = (8000, 11025, 16000, 22050, 32000, 44100, 48000, 96000)
WHAT = ("reference libavcodec/resample.c audio_resample (resample2.c av_resample, int16 branch) over seeded inputs; fnv = FNV-1a-64 "
        "of the int16 output bytes of all calls, counts_fnv = of the per-call counts as int32")
WHAT_CRAFTED = ("reference libavcodec/resample.c audio_resample over the crafted streams of tests/audio_resample_builder.py "
                "(reference_cases, by name); fnv and counts_fnv as in ref_audio_resample.json")


def load():
    """oracle/_ref/libarref.so, or None where it is not built"""
    if not os.path.exists(LIBRARY):
        return None
    lib = ctypes.CDLL(LIBRARY)
    lib.ref_audio_resample_run.restype = ctypes.c_long
    lib.ref_audio_resample_run.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                                                ctypes.c_long, ctypes.c_void_p]
    return lib


def run_reference(lib, x, in_ch, in_rate, out_ch, out_rate, sizes):
    """(concatenated output, per-call counts) of the reference's audio_resample over packets of `sizes` frames"""
    x = np.ascontiguousarray(x, np.int16)
    sizes = np.array(sizes, np.int32)
    ratio = np.float32(out_rate) / np.float32(in_rate)
    cap = sum(int(np.float32(4 * int(nb)) * ratio) + 16 for nb in sizes) * out_ch
    out, counts = np.zeros(cap, np.int16), np.zeros(len(sizes), np.int32)
    n = lib.ref_audio_resample_run(out_ch, in_ch, out_rate, in_rate, x.ctypes.data, sizes.ctypes.data, len(sizes), out.ctypes.data,
                                   cap, counts.ctypes.data)
    assert n >= 0, "the reference refused (%d)" % n
    return out[:n * out_ch].copy(), counts.tolist()


def grid_specs():
    """the 169 cases of ref_audio_resample.json, in the file's order"""
    specs, seed = [], 100

    def add(tag, in_rate, in_ch, out_ch, kind, s, frames, packets):
        specs.append({"tag": tag, "in_rate": in_rate, "out_rate": 22050, "in_ch": in_ch, "out_ch": out_ch,
                      "input": {"kind": kind, "seed": s, "frames": frames}, "packets": packets})

    for rate in RATES:
        fl = R.filter_length(rate, 22050)
        for ic, oc in ((1, 1), (2, 1), (1, 2), (2, 2)):
            seed += 1
            add("grid", rate, ic, oc, "noise", seed, rate // 4 + 123, None)
            add("grid", rate, ic, oc, "noise", seed, rate // 4 + 123, {"seed": seed, "max": 2000})
        for ic, oc in ((1, 1), (2, 2), (2, 1)):
            seed += 1
            add("square", rate, ic, oc, "square", seed, rate // 8 + 77, None)
            add("square", rate, ic, oc, "square", seed, rate // 8 + 77, {"seed": seed, "max": 700})
        for frames in (1, 2, fl // 2, fl - 1):
            seed += 1
            add("short", rate, 1, 1, "noise", seed, frames, None)
        seed += 1
        add("short", rate, 2, 2, "square", seed, fl - 1, None)
    add("silence", 44100, 2, 1, "silence", 0, 5000, None)
    add("silence", 48000, 2, 2, "silence", 0, 5000, {"seed": 9, "max": 500})
    for rate, ic, oc, first in ((44100, 2, 1, 5), (44100, 2, 1, 10), (8000, 1, 1, 3), (96000, 2, 2, 17), (48000, 1, 2, 1), (16000, 1, 1, 16)):
        seed += 1
        add("wrap", rate, ic, oc, "noise", seed, 6000, {"first": first, "seed": seed, "max": 300})
    for every in (None, 1000, 37, 10, 20):
        add("anchor", 44100, 2, 1, "noise", 1, 100000, {"every": every} if every else None)
    add("anchor", 48000, 1, 1, "noise", 2, 48000, None)
    add("anchor", 8000, 1, 1, "noise", 3, 1000, None)
    add("anchor", 8000, 1, 1, "noise", 3, 1000, {"every": 7})
    add("anchor", 44100, 1, 1, "noise", 4, 30, None)
    return specs


def results(out, counts, out_ch, most_calls):
    """what a fixture keeps of a case's output"""
    r = {"calls": len(counts), "out_frames": len(out) // out_ch, "counts_fnv": R.fnv1a64(np.array(counts, np.int32).tobytes()),
         "fnv": R.fnv1a64(out.tobytes())}
    if len(out) <= 64:
        r["samples"] = out.tolist()
    if len(counts) <= most_calls:
        r["counts"] = counts
    return r


def compute(lib):
    """ref_audio_resample.json as the reference build makes it"""
    cases = []
    for s in grid_specs():
        i = s["input"]
        x = R.make_input(i["kind"], i["seed"], i["frames"], s["in_ch"])
        out, counts = run_reference(lib, x, s["in_ch"], s["in_rate"], s["out_ch"], s["out_rate"], R.packet_sizes(s["packets"], i["frames"]))
        cases.append({**s, **results(out, counts, s["out_ch"], 8)})
    return {"what": WHAT, "cases": cases}


def compute_crafted(lib):
    """ref_audio_resample_crafted.json as the reference build makes it"""
    cases = []
    for c in B.reference_cases():
        frames = c["x"].size // c["in_ch"]
        out, counts = run_reference(lib, c["x"], c["in_ch"], c["in_rate"], c["out_ch"], c["out_rate"], c["packets"] or [frames])
        cases.append({"name": c["name"], "in_rate": c["in_rate"], "out_rate": c["out_rate"], "in_ch": c["in_ch"], "out_ch": c["out_ch"],
                      "frames": frames, "packets": c["packets"], **results(out, counts, c["out_ch"], 16)})
    return {"what": WHAT_CRAFTED, "cases": cases}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "ref_audio_resample.json"))
    ap.add_argument("--crafted-out", default=os.path.join(HERE, "ref_audio_resample_crafted.json"))
    a = ap.parse_args()
    lib = load()
    assert lib is not None, "no %s: run `make -C oracle ref` where the reference tree is" % LIBRARY
    for path, doc in ((a.out, compute(lib)), (a.crafted_out, compute_crafted(lib))):
        with open(path, "w") as f:
            json.dump(doc, f, separators=(",", ":"))
        print("%s: %d cases, %d bytes" % (path, len(doc["cases"]), os.path.getsize(path)))


if __name__ == "__main__":
    main()
