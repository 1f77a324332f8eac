"""The entropy kernels on crafted scans (tests/scan_builder.py), against the oracle, on a real MI355X.

Every frame of the builder's corpus -- every symbol of the four tables, the longest symbols back to back, predictors
that wrap, ZRL / run-15 edges, FF at every byte offset, frames over, just under and just over their record space,
errors in every block of an MCU and in the last 17 bits, cuts inside codes -- sits between ordinary synthetic frames in
a blob that starts at an odd offset, so that records a frame writes past its own space show up in its neighbours.
Status and every byte equal the oracle's in the amvlib modes (both zig-zag tables), FFmpeg-compat and its keep mode;
the stage accessor gives the oracle's status, MCU count and coefficients, and a valid frame's coefficients are the
builder's own.  Through every entropy kernel: the lane counts a batch gets by itself, 1 (with and without the
heavy-frame split), 2, 8 and 64, the serial kernel, and the layout of large batches.  The parallel kernels hand exactly
the frames with more records than their record space to the serial kernel."""
import os

import numpy as np
import pytest

import scan_builder as sb
from conftest import SEED
from test_gpu_parity import _blob_of, _t

pytestmark = pytest.mark.gpu

CONFIGS = {
    "auto": {},
    "lanes1": {"AMVHIP_SYNC_LANES": "1"},
    "lanes1_split0": {"AMVHIP_SYNC_LANES": "1", "AMVHIP_SPLIT": "0"},
    "lanes1_split64": {"AMVHIP_SYNC_LANES": "1", "AMVHIP_SPLIT": "64"},
    "lanes2": {"AMVHIP_SYNC_LANES": "2"},
    "lanes8": {"AMVHIP_SYNC_LANES": "8"},
    "lanes64": {"AMVHIP_SYNC_LANES": "64"},
    "layout_large": {"AMVHIP_LAYOUT": "large"},
    "serial": {},
}
KNOBS = ("AMVHIP_SYNC_LANES", "AMVHIP_SPLIT", "AMVHIP_LAYOUT")


@pytest.fixture(scope="module")
def batches(orc):
    """per geometry: the crafted frames, each between two synthetic ones, and what the oracle makes of every chunk"""
    by_geom = {}
    for c in sb.corpus():
        by_geom.setdefault((c.w, c.h), []).append(c)
    out = []
    rng = np.random.default_rng(77)
    for (w, h), cases in by_geom.items():
        synth = [orc.encode_frame(orc.synth_frame(SEED, 11 * t, w, h), w, h) for t in range(3)]
        chunks, where = [synth[0]], []
        for i, c in enumerate(cases):
            where.append(len(chunks))
            chunks += [c.chunk, synth[(i + 1) % 3]]
        fb = orc.lib().amvo_yuv420_frame_bytes(w, h)
        before = rng.integers(0, 256, (len(chunks), fb), dtype=np.uint8)
        want = {
            0: [orc.decode_frame(c, w, h, 0, want_coef=True) for c in chunks],
            1: [orc.decode_frame(c, w, h, 1) for c in chunks],
            "ffmpeg": [orc.decode_frame_ffmpeg(c, w, h) for c in chunks],
            "keep": [orc.decode_frame_ffmpeg_keep(c, w, h, before[i]) for i, c in enumerate(chunks)],
        }
        for k, i in enumerate(where):      # the oracle is the builder's model on these (test_scan_builder pins it)
            assert (want[0][i][1], want[0][i][2]) == (cases[k].status, cases[k].ok), cases[k].name
        out.append({"w": w, "h": h, "cases": cases, "chunks": chunks, "where": where, "before": before, "want": want,
                    "over": sum(c.over for c in cases), "near": sum(not (c.over or c.under) for c in cases)})
    assert [(b["over"], b["near"]) for b in out if (b["w"], b["h"]) == (160, 120)] == [(4, 0)]
    return out


@pytest.fixture(scope="module")
def ctxs(pkg):
    keep = {k: os.environ.get(k) for k in KNOBS}
    made = {}
    try:
        for name, env in CONFIGS.items():
            for k in KNOBS:
                if k in env:
                    os.environ[k] = env[k]
                else:
                    os.environ.pop(k, None)
            made[name] = pkg.Context(0)
        made["serial"].set_entropy_mode(pkg.ENTROPY_SERIAL)
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    yield made
    for c in made.values():
        c.close()


def _decode(c, b, flags, out0):
    import torch
    blob, offs, lens, nbytes = _blob_of(b["chunks"], pad_front=1)
    n = len(b["chunks"])
    d_out = torch.from_numpy(out0).to("cuda:0")
    d_st = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    c.decode_batch_dev(_t(blob), nbytes, _t(offs), _t(lens), n, b["w"], b["h"], flags, d_out, d_st,
                       torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), d_st.cpu().numpy()


def _names(b, bad):
    """which frames of the batch differ: the crafted frames' names, the synthetic neighbours' places"""
    at = dict(zip(b["where"], (c.name for c in b["cases"])))
    return [at.get(int(i), "synthetic #%d" % int(i)) for i in bad[:6]]


def _check_handed(c, b, key):
    if key == "serial":
        return
    handed = c.entropy_stats(False)["handed_to_serial"]
    assert b["over"] <= handed <= b["over"] + b["near"], (key, b["w"], b["h"], handed, b["over"])


@pytest.mark.parametrize("key", list(CONFIGS))
def test_crafted_scans_decode_as_the_oracle(ctxs, pkg, batches, key):
    c = ctxs[key]
    for b in batches:
        w, h, n = b["w"], b["h"], len(b["chunks"])
        for flags in (0, 1):
            got, st = _decode(c, b, flags, np.full((n, h, c.stride(w)), 0x5A, np.uint8))
            _check_handed(c, b, key)
            want = np.stack([x[0] for x in b["want"][flags]])
            wst = np.array([x[1] for x in b["want"][flags]], np.int32)
            assert (st == wst).all(), (key, w, h, flags, _names(b, np.nonzero(st != wst)[0]))
            bad = np.nonzero((got != want).reshape(n, -1).any(1))[0]
            assert bad.size == 0, (key, w, h, flags, _names(b, bad))
        fb = b["before"].shape[1]
        got, st = _decode(c, b, pkg.FLAG_FFMPEG, np.full((n, fb), 0x5A, np.uint8))
        _check_handed(c, b, key)
        want = np.stack([x[0] for x in b["want"]["ffmpeg"]])
        wst = np.array([x[1] for x in b["want"]["ffmpeg"]], np.int32)
        assert (st == wst).all(), (key, w, h, "ffmpeg", _names(b, np.nonzero(st != wst)[0]))
        bad = np.nonzero((got != want).any(1))[0]
        assert bad.size == 0, (key, w, h, "ffmpeg", _names(b, bad))
        got, st = _decode(c, b, pkg.FLAG_FFMPEG | pkg.FLAG_FFMPEG_KEEP, b["before"].copy())
        want = np.stack([x[0] for x in b["want"]["keep"]])
        wst = np.array([x[1] for x in b["want"]["keep"]], np.int32)
        assert (st == wst).all(), (key, w, h, "keep", _names(b, np.nonzero(st != wst)[0]))
        bad = np.nonzero((got != want).any(1))[0]
        assert bad.size == 0, (key, w, h, "keep", _names(b, bad))


@pytest.mark.parametrize("key", list(CONFIGS))
def test_crafted_scans_through_the_stage_accessor(ctxs, batches, key):
    import torch
    c = ctxs[key]
    for b in batches:
        w, h, n = b["w"], b["h"], len(b["chunks"])
        nblk = sb.mcus(w, h) * 6
        blob, offs, lens, nbytes = _blob_of(b["chunks"], pad_front=1)
        d_coef = torch.full((n, nblk, 64), 77, dtype=torch.int16, device="cuda:0")
        d_st = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
        d_ok = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
        c.huffman_decode_dev(_t(blob), nbytes, _t(offs), _t(lens), n, w, h, d_coef, d_st, d_ok)
        torch.cuda.synchronize()
        _check_handed(c, b, key)
        coef, st, ok = d_coef.cpu().numpy(), d_st.cpu().numpy(), d_ok.cpu().numpy()
        want = b["want"][0]
        assert (st == np.array([x[1] for x in want])).all(), (key, w, h, _names(b, np.nonzero(st != [x[1] for x in want])[0]))
        assert (ok == np.array([x[2] for x in want])).all(), (key, w, h, _names(b, np.nonzero(ok != [x[2] for x in want])[0]))
        for i in range(n):
            upto = int(want[i][2]) * 6
            assert (coef[i, :upto] == want[i][3][:upto]).all(), (key, w, h, _names(b, [i]))
        for k, i in enumerate(b["where"]):
            case = b["cases"][k]
            if case.coef is not None:
                assert (coef[i] == case.coef).all(), (key, case.name)
