"""The audio resampler on crafted streams (tests/audio_resample_builder.py; what each stream reaches is proved without a GPU in
tests/test_audio_resample_builder.py): every row and tap of five filter banks, rounding ties and both saturations, tiles of
150, 129, 65, 22 and 256 outputs ending on and around a boundary, the carry of the tile scan, empty and oversize streams, and
packet sequences cut inside the mirrored head.  Every comparison is byte for byte against the CPU restatement
(audio_resample_ref.py, pinned to the real reference on these streams by tests/golden/ref_audio_resample_crafted.json), in the
device form and the host form, with sentinels around every output; a failure names the case, the first differing output, its
phase row, first frame and tile."""
import ctypes

import numpy as np
import pytest

import audio_resample_ref as R
import audio_resample_builder as B

SENTINEL = 0x5A5A
HUGE = 1 << 32                                  # frames of the stream that "makes nothing"


def layout(sizes, seed):
    """offsets of blocks of `sizes` samples with 1, 3, 5 or 7 samples between them (and in front): nothing 16-byte aligned"""
    rng = np.random.default_rng(seed)
    offs, pos = [], 0
    for n in sizes:
        pos += 1 + 2 * int(rng.integers(0, 4))
        offs.append(pos)
        pos += n
    return offs, pos + 8


def split(out, offs, lens, what):
    gaps = np.ones(out.size, bool)
    for o, n in zip(offs, lens):
        gaps[o:o + n] = False
    assert (out[gaps].view(np.uint16) == SENTINEL).all(), "%s: written outside the streams' outputs" % what
    return [out[o:o + n] for o, n in zip(offs, lens)]


def run_forms(ctx, streams, in_ch, in_rate, out_ch, out_rate, lens, seed, huge_at=None):
    """streams (interleaved int16) -> {"device": outputs, "host": outputs} of one batch call per form; `lens`: the samples
    each output slot gets (the restatement's lengths, not the library's).  huge_at: the stream index at which the device
    form gets one more stream, of 2^32 frames, with an output slot of no samples"""
    import torch
    pcm_offs, pcm_size = layout([len(s) for s in streams], seed)
    out_offs, out_size = layout(lens, seed + 1)
    pcm = np.zeros(pcm_size, np.int16)
    for o, s in zip(pcm_offs, streams):
        pcm[o:o + len(s)] = s
    nsamp = [len(s) // in_ch for s in streams]
    got = {}
    # the host form
    out = np.full(out_size, SENTINEL, np.uint16).view(np.int16)
    ctx.audio_resample_batch(pcm, pcm.size, np.array(pcm_offs, np.uint64), np.array(nsamp, np.uint64), len(streams), in_ch, in_rate,
                             out, out.size, np.array(out_offs, np.uint64), out_ch, out_rate)
    got["host"] = split(out, out_offs, lens, "host form")
    # the device form
    d_offs, d_nsamp, d_out_offs = list(pcm_offs), list(nsamp), list(out_offs)
    if huge_at is not None:
        d_offs.insert(huge_at, 0)
        d_nsamp.insert(huge_at, HUGE)
        d_out_offs.insert(huge_at, out_offs[huge_at])             # no samples of its own: the next stream's slot starts here
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.array(a, np.uint64).view(np.int64)).to(dev)
    d_out = torch.from_numpy(np.full(out_size, SENTINEL, np.uint16).view(np.int16)).to(dev)
    ctx.audio_resample_batch_dev(torch.from_numpy(pcm).to(dev), t(d_offs), t(d_nsamp), len(d_nsamp), in_ch, in_rate, d_out, t(d_out_offs),
                                 out_ch, out_rate, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got["device"] = split(d_out.cpu().numpy(), out_offs, lens, "device form")
    return got


def check_cases(ctx, cases, seed, huge_at=None):
    """one batch of whole-stream cases of one format, both forms, against the restatement; returns the expected outputs"""
    c0 = cases[0]
    fmt = (c0["in_ch"], c0["in_rate"], c0["out_ch"], c0["out_rate"])
    assert all((c["in_ch"], c["in_rate"], c["out_ch"], c["out_rate"]) == fmt and c["packets"] is None for c in cases)
    want = [B.expected(c)[0] for c in cases]
    got = run_forms(ctx, [c["x"] for c in cases], *fmt, [len(w) for w in want], seed, huge_at)
    for form, outs in got.items():
        for i, (c, o, w) in enumerate(zip(cases, outs, want)):
            diff = B.first_difference(c, o, w)
            assert diff is None, "%s form, stream %d of %d: %s" % (form, i, len(cases), diff)
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("pair", list(B.COEFFICIENT_STREAMS), ids=lambda p: "%d-%d" % p)
def test_every_bank_entry(ctx, pkg, pair):
    """impulse trains: every output past the head is minus one coefficient of the bank the host built -- all 1024 x fl of
    22050 -> 22051, 44100 -> 22049 (rows padded by 4 and 7 taps) and 8000 -> 22051, every row and every tap of 96000 -> 4001
    and 192000 -> 7001 (tiles of 150 and 129) -- compared with the restatement's output and with its bank, entry by entry"""
    a, b = pair
    c = next(c for c in B.coefficient_cases() if (c["in_rate"], c["out_rate"]) == pair)
    k, ph, tap = B.singled_out(a, b, c["x"].size)
    want_entries = -R.filter_bank(a, b)[ph, tap]
    got = run_forms(ctx, [c["x"]], 1, a, 1, b, [R.out_samples(a, b, c["x"].size)], a)
    want = B.expected(c)[0]
    for form, (o,) in got.items():
        bad = np.flatnonzero(o[k] != want_entries)
        assert bad.size == 0, "%s form, %s: bank[%d][%d] read as %d, is %d: %r" % (
            form, c["name"], ph[bad[0]], tap[bad[0]], -int(o[k[bad[0]]]), -int(want_entries[bad[0]]), B.where(a, b, int(k[bad[0]])))
        diff = B.first_difference(c, o, want)
        assert diff is None, "%s form: %s" % (form, diff)


@pytest.mark.gpu
def test_rounding_saturation_and_the_stereo_mix(ctx, pkg):
    """(acc + 2^14) >> 15 on 13 095 negative ties; windows that reach +-2 050 442 697 and +-1 739 151 446 and must clip, not
    wrap; stereo constants whose sum is odd and negative through 2 -> 1, and full scale through 2 -> 1 and 2 -> 2"""
    check_cases(ctx, B.rounding_cases(), 1)
    sat = B.saturation_cases()
    for a, b in B.SATURATION_PAIRS:
        cases = [c for c in sat if (c["in_rate"], c["out_rate"]) == (a, b)]
        want = check_cases(ctx, cases, 2)
        assert [int(w[c["window"][0]]) for c, w in zip(cases, want)] == [32767, -32768]
    stereo = B.stereo_cases()
    for oc in (1, 2):
        check_cases(ctx, [c for c in stereo if c["out_ch"] == oc], 3 + oc)


@pytest.mark.gpu
@pytest.mark.parametrize("batch", B.seam_batches(), ids=lambda b: "%d-%d_%dto%d" % b[:4])
def test_tile_seams(ctx, pkg, batch):
    """streams of T-1, T, T+1, 2T and 2T+1 outputs in one ragged batch, for tiles of T = 150, 129, 65, 22 and 256 outputs"""
    a, b, ic, oc, cases = batch
    want = check_cases(ctx, cases, a + b)
    assert [len(w) // oc for w in want] == list(B.seam_counts(B.SEAM_TILES[(a, b)]))


@pytest.mark.gpu
@pytest.mark.parametrize("n", B.SHAPE_COUNTS)
def test_stream_counts_around_the_scan_width(ctx, pkg, n):
    """1023, 1024, 1025 and 2049 one-tile streams: the 1024-wide scan of the tile counts, its carry and its last word"""
    a, b = B.SHAPE_PAIR
    check_cases(ctx, [B.case("shape%d_stream%d" % (n, i), 1, a, 1, b, s) for i, s in enumerate(B.shape_batch(n, n))], n)


@pytest.mark.gpu
def test_empty_and_oversize_streams_make_nothing(ctx, pkg):
    """streams of no frames first, last and three in a row; in the device form also a stream of 2^32 frames (between two
    real ones, and in front of all): nothing is written for them, and their neighbours are exact"""
    a, b = B.SHAPE_PAIR
    cases = [B.case("empty_batch_stream%d" % i, 1, a, 1, b, s) for i, s in enumerate(B.empty_stream_batch())]
    want = check_cases(ctx, cases, 11, huge_at=3)
    assert [len(w) for i, w in enumerate(want) if i in B.EMPTY_AT] == [0] * 5
    check_cases(ctx, cases[1:5], 12, huge_at=0)


@pytest.mark.gpu
def test_streaming_sequences(ctx, pkg):
    """audio_resample per packet: the first call cut by lenout inside the mirrored head (the next starts at a negative index
    with frac != 0 over a longer buffer), packets of no frames, runs of calls that make nothing; every call's count and
    samples against the restatement, nothing written past a call's count"""
    lib = pkg.load_library()
    for c in B.streaming_cases():
        want, counts = B.expected(c)
        tr = B.trace(c)
        r = ctx.audio_resampler(c["out_ch"], c["in_ch"], c["out_rate"], c["in_rate"])
        pos = opos = 0
        for call, (nb, n, t) in enumerate(zip(c["packets"], counts, tr)):
            packet = np.ascontiguousarray(c["x"][pos * c["in_ch"]:(pos + nb) * c["in_ch"]])
            pos += nb
            room = t["lenout"] * c["out_ch"]
            buf = np.full(room + 16, SENTINEL, np.uint16).view(np.int16)
            got = lib.amvhip_audio_resample(r.h, buf[8:].ctypes.data, packet.ctypes.data, nb)
            assert got == n, "%s, call %d: returned %d, expected %d" % (c["name"], call, got, n)
            o = buf[8:8 + n * c["out_ch"]]
            diff = B.first_difference(c, o, want[opos:opos + n * c["out_ch"]], t["index"], t["frac"])
            assert diff is None, "call %d (%d frames): %s" % (call, nb, diff)
            assert (buf[:8].view(np.uint16) == SENTINEL).all() and (buf[8 + n * c["out_ch"]:].view(np.uint16) == SENTINEL).all(), \
                "%s, call %d: written outside its %d outputs" % (c["name"], call, n)
            opos += n * c["out_ch"]
        r.close()
        assert opos == len(want)
