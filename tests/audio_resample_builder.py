"""Crafted streams for the audio resampler (test side only): inputs built so that a named path of amv_audio_resample.hip,
amvhip_audio.hip or the bank builder of amv_host_plan.h must run, and the arithmetic that says which path an output takes.
Everything here is derived from the CPU restatement (audio_resample_ref.py: positions, filter_bank, out_samples), never from
the code under test; tests/test_audio_resample_builder.py proves each claim, tests/test_gpu_crafted_audio_resample.py runs
the streams on the device, tests/golden/make_ref_audio_resample_golden.py runs them through the real reference.

A case is a dict: name, in_ch, in_rate, out_ch, out_rate, x (interleaved int16), packets (None: one call on the whole
stream; a list: one audio_resample call per entry, frames each).

  coefficient_cases()   impulse trains that single out one bank entry per output (every row and tap of five banks)
  rounding_cases()      the same train at +16384: every odd negative coefficient is a negative rounding tie
  saturation_cases()    windows sign-matched to the heaviest bank row, and their negations: both saturations, |sum| near 2^31
  stereo_cases()        constant stereo frames through 2 -> 1 (the floor of (l + r) >> 1) and 2 -> 2
  seam_batches()        per tile size 150, 129, 65, 22, 256: streams of T-1, T, T+1, 2T, 2T+1 outputs
  shape_batches()       1023 / 1024 / 1025 / 2049 tiny streams; streams of no frames first, last and three in a row
  streaming_cases()     packet sequences cut by lenout inside the mirrored head, packets of no frames, calls that make nothing
"""
import numpy as np

import audio_resample_ref as R

SPAN, BLOCK = 4096, 256                        # kAudioSpan of amv_kernels.h, kBlock of amv_audio_resample.hip


def fl_pad(in_rate, out_rate):
    """taps of a bank row as the device keeps it: a multiple of 8 (audio_plan of amvhip_audio.hip)"""
    return (R.filter_length(in_rate, out_rate) + 7) & ~7


def tile(in_rate, out_rate):
    """outputs per workgroup pass: audio_resample_tile of amv_audio_resample.hip, restated"""
    t = min((SPAN - fl_pad(in_rate, out_rate) - 4) * out_rate // in_rate, BLOCK)
    return t if t else 1


def case(name, in_ch, in_rate, out_ch, out_rate, x, packets=None):
    x = np.ascontiguousarray(x, np.int16)
    assert x.size % in_ch == 0 and (packets is None or sum(packets) == x.size // in_ch)
    return {"name": name, "in_ch": in_ch, "in_rate": in_rate, "out_ch": out_ch, "out_rate": out_rate, "x": x, "packets": packets}


def expected(c):
    """(interleaved output, per-call counts) of the restatement"""
    if c["packets"] is None:
        out = R.resample_whole(c["x"], c["in_ch"], c["in_rate"], c["out_ch"], c["out_rate"])
        return out, [len(out) // c["out_ch"]]
    return R.resample_packets(c["x"], c["in_ch"], c["in_rate"], c["out_ch"], c["out_rate"], c["packets"])


def whole_positions(in_rate, out_rate, frames):
    """I_k of every output of one call on a whole stream"""
    return R.positions(in_rate, out_rate, R.out_samples(in_rate, out_rate, frames), R.index0(R.filter_length(in_rate, out_rate)))


def where(in_rate, out_rate, k, base=None, frac0=0):
    """what a failure names: phase row, first frame and tile number of output k of a call from (base, frac0)"""
    if base is None:
        base = R.index0(R.filter_length(in_rate, out_rate))
    i = int(R.positions(in_rate, out_rate, k + 1, base, frac0)[k])
    return {"output": k, "phase": i & (R.PHASES - 1), "first_frame": i >> R.PHASE_SHIFT, "tile": k // tile(in_rate, out_rate)}


def first_difference(c, got, want, base=None, frac0=0):
    """None where got == want, else a message naming the first differing output of case c (interleaved samples)"""
    got, want = np.asarray(got), np.asarray(want)
    if got.size != want.size:
        return "%s: %d samples, expected %d" % (c["name"], got.size, want.size)
    bad = np.flatnonzero(got != want)
    if bad.size == 0:
        return None
    k = int(bad[0]) // c["out_ch"]
    return "%s: sample %d is %d, expected %d: %r" % (c["name"], int(bad[0]), int(got[bad[0]]), int(want[bad[0]]),
                                                       where(c["in_rate"], c["out_rate"], k, base, frac0))


# ---- a. coefficient streams ----------------------------------------------------------------------------------------------

# (in_rate, out_rate): frames.  The first three single out every (phase, tap) pair of their bank; the last two (long
# filters, tiles of 150 and 129 outputs) every phase row and every tap index.
COEFFICIENT_ALL_PAIRS = {(22050, 22051): 463050, (44100, 22049): 1984500, (8000, 22051): 136000}
COEFFICIENT_ROWS_AND_TAPS = {(96000, 4001): 288000, (192000, 7001): 288000}
COEFFICIENT_STREAMS = {**COEFFICIENT_ALL_PAIRS, **COEFFICIENT_ROWS_AND_TAPS}


def impulse_train(in_rate, out_rate, frames, amp=-32768):
    """mono: amp at every frame m * fl, zero elsewhere: a window of fl frames holds exactly one impulse"""
    x = np.zeros(frames, np.int16)
    x[::R.filter_length(in_rate, out_rate)] = amp
    return x


def singled_out(in_rate, out_rate, frames):
    """(k, phase, tap) of the outputs with I_k >= 0 of an impulse train: output k is amp * bank[phase][tap], rounded"""
    fl = R.filter_length(in_rate, out_rate)
    I = whole_positions(in_rate, out_rate, frames)
    k = np.flatnonzero(I >= 0)
    return k, I[k] & (R.PHASES - 1), (-(I[k] >> R.PHASE_SHIFT)) % fl


def coefficient_cases():
    return [case("coeff_%d_%d" % (a, b), 1, a, 1, b, impulse_train(a, b, n)) for (a, b), n in COEFFICIENT_STREAMS.items()]


# ---- b. rounding and range -----------------------------------------------------------------------------------------------

ROUNDING = (22050, 22051, 50000)               # in_rate, out_rate, frames
SATURATION_PAIRS = ((8000, 22051), (44100, 22049))   # upsampling (fl 16), downsampling (fl 41)
STEREO_CONSTANTS = ((-1, 0), (-32768, -32768), (32767, 32767), (-32768, 32767))
STEREO_PAIR, STEREO_FRAMES = (44100, 22050), 300


def rounding_cases():
    a, b, n = ROUNDING
    return [case("tie_%d_%d" % (a, b), 1, a, 1, b, impulse_train(a, b, n, 16384))]


def heaviest_row(in_rate, out_rate):
    """(phase, largest |sum| an int16 window can reach on that row), the row where it is largest"""
    bank = R.filter_bank(in_rate, out_rate).astype(np.int64)
    pos, neg = np.where(bank > 0, bank, 0).sum(axis=1), np.where(bank < 0, -bank, 0).sum(axis=1)
    reach = np.maximum(32767 * pos + 32768 * neg, 32768 * pos + 32767 * neg)
    return int(np.argmax(reach)), int(reach.max())


def saturation_cases():
    """per pair: zeros, but for one window matched in sign to the heaviest row at full scale (positive sum), and the same
    with every sign turned (negative sum); the window sits at the first output with I_k >= 0 that reads that row"""
    out = []
    for a, b in SATURATION_PAIRS:
        fl = R.filter_length(a, b)
        ph, _ = heaviest_row(a, b)
        I = R.positions(a, b, 2 * b, R.index0(fl))
        k = int(np.flatnonzero((I >= 0) & ((I & (R.PHASES - 1)) == ph))[0])
        s = int(I[k] >> R.PHASE_SHIFT)
        row = R.filter_bank(a, b)[ph]
        for name, hi, lo in (("pos", 32767, -32768), ("neg", -32768, 32767)):
            x = np.zeros(s + 4 * fl, np.int16)
            x[s:s + fl] = np.where(row >= 0, hi, lo)
            c = case("sat_%s_%d_%d" % (name, a, b), 1, a, 1, b, x)
            c["window"] = (k, ph, s)
            out.append(c)
    return out


def stereo_cases():
    a, b = STEREO_PAIR
    return [case("stereo_%d_%d_to%d" % (l & 0xFFFF, r & 0xFFFF, oc), 2, a, oc, b, np.tile(np.array([l, r], np.int16), STEREO_FRAMES))
            for l, r in STEREO_CONSTANTS for oc in (1, 2)]


# ---- c. tile seams -------------------------------------------------------------------------------------------------------

# (in_rate, out_rate, in_ch, out_ch): tiles of 150, 129, 65, 22 and 256 outputs; every channel mode at least once
SEAM_PAIRS = ((192000, 8000, 1, 1), (192000, 7001, 2, 1), (192000, 4000, 1, 2), (192000, 2000, 2, 2), (44100, 22050, 2, 1))
SEAM_TILES = {(192000, 8000): 150, (192000, 7001): 129, (192000, 4000): 65, (192000, 2000): 22, (44100, 22050): 256}


def frames_for(in_rate, out_rate, outputs):
    """the fewest frames of a whole stream that make `outputs` outputs (out_samples is monotonic in the frames)"""
    lo, hi = 0, 1
    while R.out_samples(in_rate, out_rate, hi) < outputs:
        hi *= 2
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if R.out_samples(in_rate, out_rate, mid) < outputs:
            lo = mid
        else:
            hi = mid
    assert R.out_samples(in_rate, out_rate, hi) == outputs, (in_rate, out_rate, outputs)
    return hi


def seam_counts(t):
    return (t - 1, t, t + 1, 2 * t, 2 * t + 1)


def seam_batches():
    """[(in_rate, out_rate, in_ch, out_ch, [case, ...])]: one ragged batch per pair, noise input"""
    out = []
    for a, b, ic, oc in SEAM_PAIRS:
        t = tile(a, b)
        cases = [case("seam_%d_%d_%d" % (a, b, n), ic, a, oc, b, R.make_input("noise", 7000 + n, frames_for(a, b, n), ic))
                 for n in seam_counts(t)]
        out.append((a, b, ic, oc, cases))
    return out


# ---- d. batch shapes -----------------------------------------------------------------------------------------------------

SHAPE_PAIR = (44100, 22050)                    # fl 40, one phase row: cheap
SHAPE_COUNTS = (1023, 1024, 1025, 2049)        # around the carry of the 1024-wide scan of amv_audio_tiles_kernel
EMPTY_AT = (0, 5, 6, 7, 12)                    # of 13 streams: first, three in a row, last


def shape_batch(n, seed):
    """n tiny mono noise streams, 1 .. 120 frames (streams shorter than the filter, and of one to a few dozen outputs)"""
    frames = 1 + R.hash32(seed, np.arange(n)).astype(np.int64) % 120
    return [R.make_input("noise", seed + i, int(f), 1) for i, f in enumerate(frames)]


def empty_stream_batch():
    streams = shape_batch(13, 900)
    for i in EMPTY_AT:
        streams[i] = np.zeros(0, np.int16)
    return streams


# ---- e. streaming sequences ----------------------------------------------------------------------------------------------

STREAMING = (
    ("cut_1000_192000", 1, 1000, 1, 192000, (1, 1, 1, 1, 0, 3, 40)),
    ("cut_8000_48000", 1, 8000, 1, 48000, (1, 1, 2, 0, 30)),
    ("starve_192000_8000", 1, 192000, 1, 8000, (100,) * 8 + (0, 1)),
    ("cut_2to2_1000_192000", 2, 1000, 2, 192000, (1, 1, 0, 1, 2, 37)),
    ("starve_2to1_192000_8000", 2, 192000, 1, 8000, (100,) * 6 + (0, 300, 1)),
)


def streaming_cases():
    return [case(name, ic, a, oc, b, R.make_input("noise", 8000 + i, sum(p), ic), list(p))
            for i, (name, ic, a, oc, b, p) in enumerate(STREAMING)]


def trace(c):
    """per call of a streaming case, from the restatement's state: index and frac before the call, frames the call sees
    (kept tail + packet), lenout, the outputs av_resample would make without lenout, and the outputs it makes"""
    r = R.Packetised(c["out_ch"], c["in_ch"], c["out_rate"], c["in_rate"])
    rows, pos = [], 0
    for nb in c["packets"]:
        index, frac, src = r.index, r.frac, len(r.temp[0]) + nb
        uncut = R.out_count(c["in_rate"], c["out_rate"], src, index, frac)
        made = len(r.feed(c["x"][pos * c["in_ch"]:(pos + nb) * c["in_ch"]])) // c["out_ch"]
        pos += nb
        rows.append({"index": index, "frac": frac, "src": src, "lenout": int(np.float32(4 * nb) * r.ratio) + 16, "uncut": uncut,
                     "made": made})
    return rows


def reference_cases():
    """the cases that one stream of the reference can state (everything but the batch shapes of d), for the fixture
    tests/golden/ref_audio_resample_crafted.json"""
    seams = [c for *_, cases in seam_batches() for c in cases]
    return coefficient_cases() + rounding_cases() + saturation_cases() + stereo_cases() + seams + streaming_cases()
