"""No-GPU proof of what tests/audio_resample_builder.py claims for its crafted streams, from the CPU restatement alone
(audio_resample_ref.py: positions, filter_bank, out_samples, Packetised) -- never from the code under test -- and the pin of
that restatement to the real reference on every crafted stream (tests/golden/ref_audio_resample_crafted.json, remade from
oracle/_ref where the reference build is at hand)."""
import functools
import importlib.util
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import audio_resample_ref as R
import audio_resample_builder as B

CRAFTED = json.load(open(os.path.join(GOLDEN, "ref_audio_resample_crafted.json")))["cases"]


@functools.lru_cache(maxsize=None)
def reference_cases():
    return {c["name"]: c for c in B.reference_cases()}


def rows_read(in_rate, out_rate, frames):
    I = B.whole_positions(in_rate, out_rate, frames)
    return len(np.unique(I & (R.PHASES - 1)))


def test_what_the_older_tests_reach():
    """the coverage table of DESIGN.md section 7.1, `before`: the rate pairs of test_gpu_audio_resample.py and of the fixture
    read at most 640 of a bank's 1024 rows however long the stream (441 at most when downsampling), and run tiles of 256
    outputs and of 1 only"""
    rows = {(a, b): rows_read(a, b, 10 * a) for a, b in ((44100, 22050), (11025, 22050), (22050, 44100), (192000, 1000), (1000, 192000),
                                                        (11025, 48000), (48000, 22050), (96000, 22050), (8000, 22050), (16000, 22050),
                                                        (32000, 22050), (8000, 44100), (22050, 22050))}
    assert rows == {(44100, 22050): 1, (11025, 22050): 2, (22050, 44100): 2, (192000, 1000): 1, (1000, 192000): 192, (11025, 48000): 640,
                    (48000, 22050): 147, (96000, 22050): 147, (8000, 22050): 441, (16000, 22050): 441, (32000, 22050): 441,
                    (8000, 44100): 441, (22050, 22050): 1}
    assert {B.tile(a, b) for a, b in rows} == {1, 256} and B.tile(192000, 1000) == 1


# ---- a. coefficient streams ----------------------------------------------------------------------------------------------

def test_coefficient_pairs_are_the_ones_asked_for():
    facts = {(a, b): (R.filter_length(a, b), B.fl_pad(a, b) - R.filter_length(a, b), B.tile(a, b)) for a, b in B.COEFFICIENT_STREAMS}
    assert facts == {(22050, 22051): (20, 4, 256), (44100, 22049): (41, 7, 256), (8000, 22051): (16, 0, 256),
                     (96000, 4001): (480, 0, 150), (192000, 7001): (549, 3, 129)}


@pytest.mark.parametrize("pair", list(B.COEFFICIENT_STREAMS), ids=lambda p: "%d-%d" % p)
def test_coefficient_stream_singles_out_the_bank(pair):
    """every output with I_k >= 0 of the impulse train is minus one bank entry, exactly, and the entries cover the bank: every
    (phase, tap) pair of the three short filters, every phase row and every tap index of the two long ones.  Tiles
    hold first frames of both parities, so both v_alignbit shifts run side by side (at 2.0001 : 1 in a few tiles only)"""
    a, b = pair
    frames = B.COEFFICIENT_STREAMS[pair]
    fl = R.filter_length(a, b)
    bank = R.filter_bank(a, b)
    k, ph, tap = B.singled_out(a, b, frames)
    if pair in B.COEFFICIENT_ALL_PAIRS:
        assert len(np.unique(ph * fl + tap)) == R.PHASES * fl
    assert len(np.unique(ph)) == R.PHASES and len(np.unique(tap)) == fl
    x = B.impulse_train(a, b, frames)
    out = R.resample_whole(x, 1, a, 1, b)
    assert len(out) == R.out_samples(a, b, frames) and k[-1] == len(out) - 1
    assert (out[k] == -bank[ph, tap]).all()                      # (32768 c + 16384) >> 15 = c
    assert np.count_nonzero(bank[ph, tap]) > 0.6 * len(k)         # ... and c is mostly not a zero (the long filters' tails are)
    # rel, the first frame of an output relative to its tile's span: its parity picks the v_alignbit shift
    I = B.whole_positions(a, b, frames)
    t = B.tile(a, b)
    s = I[k] >> R.PHASE_SHIFT
    s0 = np.maximum(I[(k // t) * t] >> R.PHASE_SHIFT, 0)
    odd = ((s - s0) & 1).astype(bool)
    both = np.intersect1d(np.unique(k[odd] // t), np.unique(k[~odd] // t))
    # steps of 2.0001 and 23.994 frames turn the parity rarely: a few tiles only; the other pairs: all but the head's tile
    assert len(both) >= (1 if pair in ((44100, 22049), (96000, 4001)) else len(np.unique(k // t)) - 1)
    # the restatement's whole output, against the real reference
    f = next(c for c in CRAFTED if c["name"] == "coeff_%d_%d" % pair)
    assert f["frames"] == frames and f["out_frames"] == len(out) and R.fnv1a64(out.tobytes()) == f["fnv"]


def test_a_wrong_row_pitch_would_show():
    """rows of fl_pad != fl: reading row p at p * fl instead of p * fl_pad (or the reverse) changes the coefficient stream"""
    for a, b in ((22050, 22051), (44100, 22049), (192000, 7001)):
        fl, pad = R.filter_length(a, b), B.fl_pad(a, b)
        assert pad != fl
        bank = R.filter_bank(a, b)
        padded = np.zeros((R.PHASES, pad), np.int16)
        padded[:, :fl] = bank
        wrong = padded.reshape(-1)[:R.PHASES * fl].reshape(R.PHASES, fl)     # the padded bank read at the pitch fl
        _, ph, tap = B.singled_out(a, b, B.COEFFICIENT_STREAMS[(a, b)])
        assert (wrong[ph, tap] != bank[ph, tap]).mean() > 0.5


# ---- b. rounding and range -----------------------------------------------------------------------------------------------

def test_rounding_stream_hits_negative_ties():
    a, b, frames = B.ROUNDING
    k, ph, tap = B.singled_out(a, b, frames)
    c = R.filter_bank(a, b)[ph, tap].astype(np.int64)
    ties = (c < 0) & (c & 1 == 1)                                 # 16384 c + 16384 = (c + 1) * 2^14: a tie, at a negative sum
    assert int(ties.sum()) == 13095
    out = R.resample_whole(B.rounding_cases()[0]["x"], 1, a, 1, b)
    assert (out[k] == (c + 1) >> 1).all()
    assert ((c[ties] + 1) >> 1 != -((-c[ties] + 1) >> 1)).all()   # rounding half away from zero would differ on each of them


def test_saturation_windows_reach_both_ends_and_never_wrap():
    """the largest |sum| any int16 input reaches on any row of the two banks: 2 050 442 697 (95.5 % of 2^31) at fl 16 and
    1 739 151 446 at fl 41; with the rounding constant 2^14 added neither wraps the 32-bit sum.  The crafted windows reach
    exactly those sums, and saturate the output in both directions"""
    bounds = {pair: B.heaviest_row(*pair) for pair in B.SATURATION_PAIRS}
    assert bounds == {(8000, 22051): (511, 2050442697), (44100, 22049): (151, 1739151446)}
    assert all(reach + (1 << 14) < (1 << 31) for _, reach in bounds.values())
    assert bounds[(8000, 22051)][1] > 0.95 * (1 << 31)
    cases = {c["name"]: c for c in B.saturation_cases()}
    for a, b in B.SATURATION_PAIRS:
        fl = R.filter_length(a, b)
        row = R.filter_bank(a, b)[bounds[(a, b)][0]].astype(np.int64)
        sums = {}
        for sign in ("pos", "neg"):
            c = cases["sat_%s_%d_%d" % (sign, a, b)]
            k, ph, s = c["window"]
            assert B.where(a, b, k)["phase"] == ph == bounds[(a, b)][0] and B.where(a, b, k)["first_frame"] == s >= 0
            sums[sign] = int((c["x"][s:s + fl].astype(np.int64) * row).sum())
            out, _ = B.expected(c)
            assert out[k] == (32767 if sign == "pos" else -32768)
            assert (sums[sign] + (1 << 14)) >> 15 not in range(-32768, 32768)          # the clip did it
        assert max(sums["pos"], -sums["neg"]) == bounds[(a, b)][1] and sums["pos"] > 0 > sums["neg"]


def test_stereo_constants_floor_the_mix():
    mixes = {(l, r): int(R._planes(np.array([l, r], np.int16), 2, 1)[0][0]) for l, r in B.STEREO_CONSTANTS}
    assert mixes == {(-1, 0): -1, (-32768, -32768): -32768, (32767, 32767): 32767, (-32768, 32767): -1}
    assert int((-1 + 0) / 2) == 0 and int((-32768 + 32767) / 2) == 0       # a truncating mix would give 0 for both
    cases = B.stereo_cases()
    assert {(c["in_ch"], c["out_ch"]) for c in cases} == {(2, 1), (2, 2)} and len(cases) == 8
    a, b = B.STEREO_PAIR
    for c in cases:
        out, _ = B.expected(c)
        l, r = (int(v) for v in c["x"][:2])
        if c["out_ch"] == 1:
            assert out.tobytes() == R.resample_whole(np.full(B.STEREO_FRAMES, mixes[(l, r)], np.int16), 1, a, 1, b).tobytes()
        else:
            assert out[0::2].tobytes() == R.resample_whole(np.full(B.STEREO_FRAMES, l, np.int16), 1, a, 1, b).tobytes()
            assert out[1::2].tobytes() == R.resample_whole(np.full(B.STEREO_FRAMES, r, np.int16), 1, a, 1, b).tobytes()


# ---- c. tile seams -------------------------------------------------------------------------------------------------------

def test_seam_streams_end_on_and_around_tile_boundaries():
    batches = B.seam_batches()
    assert {(a, b): B.tile(a, b) for a, b, *_ in batches} == B.SEAM_TILES
    assert sorted(B.SEAM_TILES.values()) == [22, 65, 129, 150, 256]
    assert {(ic, oc) for _, _, ic, oc, _ in batches} == {(1, 1), (2, 1), (1, 2), (2, 2)}
    for a, b, ic, oc, cases in batches:
        t = B.tile(a, b)
        frames = [c["x"].size // ic for c in cases]
        assert [R.out_samples(a, b, f) for f in frames] == [t - 1, t, t + 1, 2 * t, 2 * t + 1]
        assert all(R.out_samples(a, b, f - 1) < n for f, n in zip(frames, B.seam_counts(t)))      # the fewest frames that do
        if (a, b) == (192000, 8000):
            assert frames == [3793, 3817, 3841, 7417, 7441]
        # the last tile of the five streams holds T-1, T, 1, T and 1 outputs: lanes j > last idle in three of them
        assert [(n - 1) % t + 1 for n in B.seam_counts(t)] == [t - 1, t, 1, t, 1]


# ---- d. batch shapes -----------------------------------------------------------------------------------------------------

def test_batch_shapes():
    a, b = B.SHAPE_PAIR
    assert B.SHAPE_COUNTS == (1023, 1024, 1025, 2049)           # one short of, exactly, one past one pass of the scan; two passes + 1
    for n in B.SHAPE_COUNTS:
        streams = B.shape_batch(n, n)
        assert len(streams) == n
        outs = [R.out_samples(a, b, len(s)) for s in streams]
        assert min(outs) >= 1 and max(outs) <= B.tile(a, b)       # every stream is one tile: tiles[i] == i, the scan's carry shows
        assert min(len(s) for s in streams) < R.filter_length(a, b) < max(len(s) for s in streams)
    streams = B.empty_stream_batch()
    empty = [i for i, s in enumerate(streams) if len(s) == 0]
    assert empty == [0, 5, 6, 7, 12] and len(streams) == 13
    assert all(R.out_samples(a, b, len(s)) > 0 for s in streams if len(s)) and R.out_samples(a, b, 0) == 0


# ---- e. streaming sequences ----------------------------------------------------------------------------------------------

def test_streaming_sequences_make_the_events_they_are_for():
    traces = {c["name"]: (c, B.trace(c)) for c in B.streaming_cases()}
    assert {(c["in_ch"], c["out_ch"]) for c, _ in traces.values()} >= {(1, 1), (2, 2), (2, 1)}

    c, t = traces["cut_1000_192000"]
    assert c["packets"] == [1, 1, 1, 1, 0, 3, 40]
    assert (t[0]["uncut"], t[0]["lenout"], t[0]["made"]) == (1344, 784, 784)             # cut by lenout ...
    assert t[1]["index"] == -2987 and t[1]["frac"] != 0 and t[1]["src"] != t[0]["src"]      # ... inside the mirrored head
    c, t = traces["cut_8000_48000"]
    assert c["packets"] == [1, 1, 2, 0, 30]
    assert t[0]["made"] == t[0]["lenout"] < t[0]["uncut"] and t[1]["index"] < 0 and t[1]["frac"] != 0 and t[1]["src"] != t[0]["src"]
    c, t = traces["starve_192000_8000"]
    assert c["packets"] == [100] * 8 + [0, 1]
    assert [r["made"] for r in t[:4]] == [10, 0, 0, 0]
    for name, (c, t) in traces.items():
        fl = R.filter_length(c["in_rate"], c["out_rate"])
        assert 0 in c["packets"], name                                                      # a call with nb_samples == 0
        assert all(r["src"] > 0 for r in t), name                                           # (never on an empty resampler)
        if name.startswith("cut"):
            assert t[0]["made"] == t[0]["lenout"] < t[0]["uncut"] and t[1]["index"] < 0 and t[1]["frac"] != 0, name
        # calls in a row that make nothing because the kept tail and the packet are shorter than the filter
        starved = [r["made"] == 0 and r["index"] >= 0 and r["src"] < fl for r in t]
        run = 3 if name.startswith("starve") else 2
        assert any(all(starved[i:i + run]) for i in range(len(t) - run + 1)), name
        assert t[-1]["made"] > 0 or name.startswith("starve"), name


# ---- the restatement against the real reference --------------------------------------------------------------------------

def test_crafted_fixture_names_the_builder_cases():
    assert [c["name"] for c in CRAFTED] == list(reference_cases()) and len(CRAFTED) == 48
    assert os.path.getsize(os.path.join(GOLDEN, "ref_audio_resample_crafted.json")) < 45000


@pytest.mark.parametrize("i", range(len(CRAFTED)), ids=[c["name"] for c in CRAFTED])
def test_restatement_reproduces_the_reference_on_crafted_streams(i):
    f = CRAFTED[i]
    c = reference_cases()[f["name"]]
    assert (c["in_ch"], c["in_rate"], c["out_ch"], c["out_rate"], c["x"].size // c["in_ch"], c["packets"]) == \
        (f["in_ch"], f["in_rate"], f["out_ch"], f["out_rate"], f["frames"], f["packets"])
    out, counts = B.expected(c)
    assert len(counts) == f["calls"] and sum(counts) == f["out_frames"] and len(out) == f["out_frames"] * f["out_ch"]
    if "counts" in f:
        assert counts == f["counts"]
    assert R.fnv1a64(np.array(counts, np.int32).tobytes()) == f["counts_fnv"]
    if "samples" in f:
        assert out.tolist() == f["samples"]
    assert R.fnv1a64(out.tobytes()) == f["fnv"], B.where(c["in_rate"], c["out_rate"], 0)


def test_fixtures_are_what_the_reference_build_makes():
    """both fixtures, every case, made again by tests/golden/make_ref_audio_resample_golden.py from the reference's own
    resample.c / resample2.c in oracle/_ref/libarref.so; skipped where that library is not built (no reference tree)"""
    spec = importlib.util.spec_from_file_location("make_ref_audio_resample_golden",
                                                  os.path.join(ROOT, "tests", "golden", "make_ref_audio_resample_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lib = mod.load()
    if lib is None:
        pytest.skip("oracle/_ref/libarref.so is not built here")
    old = mod.compute(lib)
    assert len(old["cases"]) == 169
    assert old == json.load(open(os.path.join(GOLDEN, "ref_audio_resample.json")))
    assert mod.compute_crafted(lib) == json.load(open(os.path.join(GOLDEN, "ref_audio_resample_crafted.json")))


def test_a_failure_names_its_output():
    c = B.coefficient_cases()[3]                                  # 96000 -> 4001, tiles of 150
    want, _ = B.expected(c)
    assert B.first_difference(c, want, want) is None
    got = want.copy()
    got[1000] ^= 1
    msg = B.first_difference(c, got, want)
    I = int(B.whole_positions(96000, 4001, c["x"].size)[1000])
    assert c["name"] in msg and repr({"output": 1000, "phase": I & 1023, "first_frame": I >> 10, "tile": 6}) in msg
