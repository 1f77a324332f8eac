"""No-GPU checks of the audio resampler (audio_resample of the reference, the -ac / -ar half of AMVmuxer/Makefile:16): the CPU
restatement in audio_resample_ref.py against outputs of the real reference (tests/golden/ref_audio_resample.json), the
closed-form position against av_resample's index / frac loop, the library's published output length, and the new entry
points' refusals."""
import ctypes
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
import audio_resample_ref as R

FIXTURE = json.load(open(os.path.join(GOLDEN, "ref_audio_resample.json")))["cases"]
RATES = (8000, 11025, 16000, 22050, 32000, 44100, 48000, 96000)


def run_case(c):
    x = R.make_input(c["input"]["kind"], c["input"]["seed"], c["input"]["frames"], c["in_ch"])
    sizes = R.packet_sizes(c["packets"], c["input"]["frames"])
    return R.resample_packets(x, c["in_ch"], c["in_rate"], c["out_ch"], c["out_rate"], sizes)


def check_case(c, out, counts):
    assert len(counts) == c["calls"] and sum(counts) == c["out_frames"] and len(out) == c["out_frames"] * c["out_ch"]
    assert R.fnv1a64(np.array(counts, np.int32).tobytes()) == c["counts_fnv"]
    if "counts" in c:
        assert counts == c["counts"]
    if "samples" in c:
        assert out.tolist() == c["samples"]
    assert R.fnv1a64(out.tobytes()) == c["fnv"]


def test_fixture_covers_what_it_should():
    pairs = {(c["in_rate"], c["in_ch"], c["out_ch"]) for c in FIXTURE if c["out_rate"] == 22050}
    assert {(r, i, o) for r in RATES for i, o in ((1, 1), (2, 1), (1, 2), (2, 2))} <= pairs
    kinds = {c["input"]["kind"] for c in FIXTURE}
    assert kinds == {"noise", "square", "silence"}
    assert any(c["input"]["frames"] < R.filter_length(c["in_rate"], c["out_rate"]) for c in FIXTURE)
    assert any(c["packets"] and c["packets"].get("first") for c in FIXTURE)


@pytest.mark.parametrize("i", range(len(FIXTURE)))
def test_restatement_reproduces_the_reference(i):
    c = FIXTURE[i]
    out, counts = run_case(c)
    check_case(c, out, counts)
    if c["packets"] is None:       # the whole-stream form is the same call
        x = R.make_input(c["input"]["kind"], c["input"]["seed"], c["input"]["frames"], c["in_ch"])
        assert R.resample_whole(x, c["in_ch"], c["in_rate"], c["out_ch"], c["out_rate"]).tobytes() == out.tobytes()


def test_filter_lengths():
    assert [R.filter_length(r, 22050) for r in (44100, 48000, 96000)] == [40, 44, 88]
    assert all(R.filter_length(r, 22050) == 16 for r in (8000, 11025, 16000))
    bank = R.filter_bank(44100, 22050)
    assert bank.shape == (1024, 40) and abs(int(bank[0].astype(np.int64).sum()) - 32768) < 40


@pytest.mark.parametrize("in_rate", RATES + (22050 * 2 + 1,))
def test_closed_form_position_is_the_recurrence(in_rate):
    n = 10 ** 6
    fl = R.filter_length(in_rate, 22050)
    assert (R.positions(in_rate, 22050, n, R.index0(fl)) == R.recurrence(in_rate, 22050, n)).all()


def test_published_output_length(pkg):
    lib = pkg.load_library()
    f = lib.amvhip_audio_resample_out_samples
    # the counts of the real reference the issue lists
    assert f(44100, 22050, 100000) == 49990 and f(48000, 22050, 48000) == 22040
    assert f(8000, 22050, 1000) == 2735 and f(44100, 22050, 30) == 10
    for c in FIXTURE:
        if c["packets"] is None:
            assert f(c["in_rate"], c["out_rate"], c["input"]["frames"]) == c["out_frames"]
    rng = np.random.default_rng(5)
    for _ in range(3000):
        a, b = (int(v) for v in rng.integers(R.RATE_MIN, R.RATE_MAX + 1, 2))
        n = int(rng.integers(0, 1 << int(rng.integers(1, 31))))
        assert f(a, b, n) == R.out_samples(a, b, n), (a, b, n)
    assert f(999, 22050, 1000) == 0 and f(44100, 192001, 1000) == 0 and f(44100, 22050, 0) == 0


@pytest.mark.parametrize("in_rate,in_ch,out_ch", [(44100, 2, 1), (48000, 1, 1), (8000, 1, 2), (96000, 2, 2), (22050, 1, 1)])
def test_whole_equals_packets_when_the_first_packet_holds_fl(in_rate, in_ch, out_ch):
    fl = R.filter_length(in_rate, 22050)
    x = R.make_input("noise", in_rate + in_ch, 7000, in_ch)
    whole = R.resample_whole(x, in_ch, in_rate, out_ch, 22050)
    for spec in ({"first": fl, "seed": 3, "max": 50}, {"seed": 4, "max": 3000}, {"first": fl + 1, "seed": 5, "max": 9}):
        out, _ = R.resample_packets(x, in_ch, in_rate, out_ch, 22050, R.packet_sizes(spec, 7000))
        assert out.tobytes() == whole.tobytes()


def test_entry_points_refuse_without_a_context_or_device(pkg):
    import torch
    lib = pkg.load_library()
    names = ("amvhip_audio_resample_out_samples", "amvhip_audio_resample_batch_dev", "amvhip_audio_resample_batch",
             "amvhip_audio_resample_init", "amvhip_audio_resample", "amvhip_audio_resample_close")
    for name in names:
        assert name in pkg.SYMBOLS and getattr(lib, name) is not None
    one = np.ones(4, np.uint64)
    pcm = np.zeros(64, np.int16)
    assert lib.amvhip_audio_resample_batch_dev(None, pcm.ctypes.data, one.ctypes.data, one.ctypes.data, 1, 1, 44100,
                                               pcm.ctypes.data, one.ctypes.data, 1, 22050, None) == pkg.ERR_ARG
    assert lib.amvhip_audio_resample_batch(None, pcm.ctypes.data, 64, one.ctypes.data, one.ctypes.data, 1, 1, 44100,
                                           pcm.ctypes.data, 64, one.ctypes.data, 1, 22050) == pkg.ERR_ARG
    assert not lib.amvhip_audio_resample_init(None, 1, 2, 22050, 44100)
    assert lib.amvhip_audio_resample(None, pcm.ctypes.data, pcm.ctypes.data, 4) == pkg.ERR_ARG
    lib.amvhip_audio_resample_close(None)
    if not torch.cuda.is_available():         # no device: no context, so nothing can run (there is no CPU fallback)
        with pytest.raises(pkg.AmvHipError):
            pkg.Context(0)
    else:                                     # a device: the reference's refusals (resample.c:134-138) and the rate range
        ctx = pkg.Context(0)
        for args in ((1, 3, 22050, 44100), (6, 2, 22050, 44100), (1, 2, 22050, 999), (1, 2, 192001, 44100), (0, 1, 22050, 44100)):
            assert not lib.amvhip_audio_resample_init(ctx.h, *args)
        with pytest.raises(pkg.AmvHipError):
            ctx.audio_resample_batch_dev(pcm, one, one, 1, 3, 44100, pcm, one, 1, 22050)
        ctx.close()
