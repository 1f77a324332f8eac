"""CPU restatement of the reference's audio resampler (test side only): audio_resample of libavcodec/resample.c:129-242 in
front of av_resample (libavcodec/resample2.c:182-324) as the reference ships it -- the int16 branch (FILTER_SHIFT 15,
FELEM2 int32_t, WINDOW_TYPE 9), 16 taps at cutoff 0.8, 1024 phases (resample.c:165).

Two entry points:
  resample_whole(x, in_ch, in_rate, out_ch, out_rate)            one audio_resample call on a whole stream
  Packetised(...).feed(packet)                                  audio_resample per packet, line by line (temp, consumed,
                                                                lenout), what ffmpeg.c:502 does per decoded packet
plus the arithmetic the device path publishes (filter_length, out_count, positions) and the seeded integer generators the
fixture tests/golden/ref_audio_resample.json was made from.

The filter bank is built with Python's math (the C library's sin / sqrt), in the double / float operation order of
av_build_filter (resample2.c:93-139); the sums are taken in int64 and reduced modulo 2**32, like FELEM2 int32_t.
"""
import functools
import math

import numpy as np

PHASE_SHIFT, PHASES = 10, 1024
TAPS, CUTOFF, FILTER_SHIFT, WINDOW_TYPE = 16, 0.8, 15, 9
RATE_MIN, RATE_MAX = 1000, 192000
FNV_BASIS, FNV_PRIME = 0xCBF29CE484222325, 0x100000001B3


def fnv1a64(data):
    h = FNV_BASIS
    for b in bytes(data):
        h = ((h ^ b) * FNV_PRIME) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


# ---- seeded integer generators (restated by the fixture's producer) ---------------------------------------------------

def hash32(seed, i):
    """integer hash of (seed, i): uint32 numpy array for an index array i"""
    i = np.asarray(i, dtype=np.uint64)
    h = (i * np.uint64(0x9E3779B1) + np.uint64((seed * 0x85EBCA77) & 0xFFFFFFFF)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x2C1B3C6D)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(12)
    h = (h * np.uint64(0x297A2D39)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(15)
    return h.astype(np.uint32)


def make_input(kind, seed, frames, channels):
    """interleaved int16, frames x channels.  noise: the hash's top 16 bits; square: full scale (32767 / -32768) with a
    half period of 3 + seed % 61 frames (channel c: + 7 c); silence: zeros"""
    n = frames * channels
    if kind == "noise":
        return (hash32(seed, np.arange(n)) >> np.uint32(16)).astype(np.uint16).view(np.int16)
    if kind == "square":
        f = np.arange(frames)[:, None]
        half = 3 + seed % 61 + 7 * np.arange(channels)[None, :]
        return np.where((f // half) % 2 == 0, 32767, -32768).astype(np.int16).reshape(n)
    if kind == "silence":
        return np.zeros(n, np.int16)
    raise ValueError(kind)


def packet_sizes(spec, frames):
    """spec None: one packet; {"first": a, "seed": s, "max": m}: a first packet of a frames (optional), then sizes
    1 + hash32(s, j) % m until the stream is used up; {"every": m}: packets of m"""
    if spec is None:
        return [frames]
    out, left = [], frames
    if spec.get("first"):
        out.append(min(spec["first"], left))
        left -= out[-1]
    j = 0
    while left > 0:
        if "every" in spec:
            p = spec["every"]
        else:
            p = 1 + int(hash32(spec["seed"], j)) % spec["max"]
        j += 1
        out.append(min(p, left))
        left -= out[-1]
    return out


# ---- the filter bank (av_resample_init + av_build_filter) ---------------------------------------------------------------

def filter_length(in_rate, out_rate):
    factor = min(out_rate * CUTOFF / in_rate, 1.0)
    return max(int(math.ceil(TAPS / factor)), 1)


def _bessel(x):
    v, t = 1.0, 1.0
    x = x * x / 4
    for i in range(1, 50):
        t *= x / (i * i)
        v += t
    return v


class _Bank:
    """the 1024 rows of one rate pair, each built when it is first asked for (a pair whose positions are periodic uses one
    row, or a few: 192000 -> 1000 reads row 0 of 1024 rows of 3840 taps) and kept"""

    def __init__(self, in_rate, out_rate):
        self.factor = min(out_rate * CUTOFF / in_rate, 1.0)
        self.fl = filter_length(in_rate, out_rate)
        self.table = np.zeros((PHASES, self.fl), np.int16)
        self.built = np.zeros(PHASES, bool)

    def _row(self, ph):
        factor, fl = self.factor, self.fl
        center = (fl - 1) // 2
        scale = 1 << FILTER_SHIFT
        tab, norm = [], 0.0
        for i in range(fl):
            x = math.pi * (float(i - center) - ph / PHASES) * factor
            y = 1.0 if x == 0 else math.sin(x) / x
            w = 2.0 * x / (factor * fl * math.pi)
            a = 1 - w * w
            y *= _bessel(WINDOW_TYPE * math.sqrt(a if a > 0 else 0))
            tab.append(y)
            norm += y
        row = []
        for y in tab:
            v = round(float(np.float32(y * scale / norm)))      # lrintf: to float, then to nearest, ties to even
            row.append(min(max(v, -32768), 32767))
        return row

    def rows(self, phases):
        """the table, with (at least) the rows `phases` names built"""
        for ph in np.unique(phases)[~self.built[np.unique(phases)]]:
            self.table[ph] = self._row(int(ph))
            self.built[ph] = True
        return self.table


@functools.lru_cache(maxsize=None)
def _bank(in_rate, out_rate):
    return _Bank(in_rate, out_rate)


def filter_bank(in_rate, out_rate):
    """1024 x fl int16, every row built (the wrap row of resample2.c:194-195 serves the linear mode only)"""
    return _bank(in_rate, out_rate).rows(np.arange(PHASES))


# ---- positions and counts ------------------------------------------------------------------------------------------------

def index0(fl):
    return -PHASES * ((fl - 1) // 2)


def positions(in_rate, out_rate, count, base, frac0=0):
    """I_k = base + floor((frac0 + k * in_rate * 1024) / out_rate): the index / frac recurrence of resample2.c:288-293"""
    k = np.arange(count, dtype=np.int64)
    return base + (frac0 + k * (in_rate * PHASES)) // out_rate


def out_count(in_rate, out_rate, src_size, base, frac0=0):
    """outputs one av_resample call makes before its break (:266-267), no dst_size limit"""
    if src_size <= 0:
        return 0
    fl = filter_length(in_rate, out_rate)
    lim = max(0, src_size - fl + 1) * PHASES
    m = lim - base
    if m <= 0:
        return 0
    d = in_rate * PHASES
    return (m * out_rate - frac0 + d - 1) // d


def out_samples(in_rate, out_rate, frames):
    """what amvhip_audio_resample_out_samples returns: output frames of one audio_resample call on a whole stream"""
    return out_count(in_rate, out_rate, frames, index0(filter_length(in_rate, out_rate)))


def recurrence(in_rate, out_rate, count):
    """the literal index / frac loop of av_resample (no compensation), for checking `positions`"""
    fl = filter_length(in_rate, out_rate)
    src_incr, dst = out_rate, in_rate * PHASES
    dst_incr_frac, dst_incr = dst % src_incr, dst // src_incr
    index, frac = index0(fl), 0
    out = np.empty(count, np.int64)
    for k in range(count):
        out[k] = index
        frac += dst_incr_frac
        index += dst_incr
        if frac >= src_incr:
            frac -= src_incr
            index += 1
    return out


# ---- av_resample on one channel ------------------------------------------------------------------------------------------

def _wrap32(v):
    return ((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def filter_channel(x, in_rate, out_rate, I):
    """av_resample's sums for positions I over the channel x (the call's whole buffer: src_size = len(x))"""
    if len(I) == 0:
        return np.zeros(0, np.int16)
    bank = _bank(in_rate, out_rate).rows(I & (PHASES - 1))       # the rows these positions read
    fl = bank.shape[1]
    out, x64 = [], x.astype(np.int64)
    step = max(1, (1 << 21) // fl)                                 # rows per pass: bounded memory at any filter length
    for a in range(0, len(I), step):
        Ic = I[a:a + step]
        s = Ic >> PHASE_SHIFT
        idx = s[:, None] + np.arange(fl)[None, :]
        head = s < 0
        idx[head] = np.abs(idx[head]) % len(x)                      # the mirrored head (:263-265)
        acc = (x64[idx] * bank[Ic & (PHASES - 1)].astype(np.int64)).sum(axis=1)
        val = _wrap32(_wrap32(acc) + (1 << (FILTER_SHIFT - 1))) >> FILTER_SHIFT
        out.append(np.clip(val, -32768, 32767).astype(np.int16))   # (unsigned)(val + 32768) > 65535 ? (val >> 31) ^ 32767 : val
    return np.concatenate(out)


def _planes(x, in_ch, out_ch):
    """the channels that are filtered (resample.c:198-216): 2 -> 1 downmixes (l + r) >> 1 first"""
    x = np.asarray(x, np.int16)
    if in_ch == 1:
        return [x]
    st = x.reshape(-1, 2).astype(np.int32)
    if out_ch == 1:
        return [((st[:, 0] + st[:, 1]) >> 1).astype(np.int16)]
    return [st[:, 0].astype(np.int16), st[:, 1].astype(np.int16)]


def _mux(outs, out_ch):
    if out_ch == 1:
        return outs[0]
    if len(outs) == 1:
        return np.repeat(outs[0], 2)
    return np.stack(outs, axis=1).reshape(-1)


def check_args(in_ch, in_rate, out_ch, out_rate):
    if in_ch not in (1, 2) or out_ch not in (1, 2):
        raise ValueError("channels: 1 or 2 in, 1 or 2 out")
    if not (RATE_MIN <= in_rate <= RATE_MAX and RATE_MIN <= out_rate <= RATE_MAX):
        raise ValueError("rates: %d .. %d" % (RATE_MIN, RATE_MAX))


def resample_whole(x, in_ch, in_rate, out_ch, out_rate):
    """one audio_resample call on the whole interleaved stream x: out_samples(...) frames, interleaved out_ch"""
    check_args(in_ch, in_rate, out_ch, out_rate)
    planes = _planes(x, in_ch, out_ch)
    frames = len(planes[0])
    if frames == 0:
        return np.zeros(0, np.int16)
    fl = filter_length(in_rate, out_rate)
    I = positions(in_rate, out_rate, out_count(in_rate, out_rate, frames, index0(fl)), index0(fl))
    return _mux([filter_channel(p, in_rate, out_rate, I) for p in planes], out_ch)


class Packetised:
    """audio_resample_init + audio_resample per packet (resample.c:129-242), state kept as the reference keeps it"""

    def __init__(self, out_ch, in_ch, out_rate, in_rate):
        check_args(in_ch, in_rate, out_ch, out_rate)
        self.in_ch, self.out_ch, self.in_rate, self.out_rate = in_ch, out_ch, in_rate, out_rate
        self.ratio = np.float32(out_rate) / np.float32(in_rate)
        self.index, self.frac = index0(filter_length(in_rate, out_rate)), 0
        self.temp = [np.zeros(0, np.int16) for _ in range(2 if in_ch == 2 and out_ch == 2 else 1)]

    def feed(self, packet):
        """one call: returns the interleaved output (its length / out_ch is the call's return value)"""
        nb = len(packet) // self.in_ch
        lenout = int(np.float32(4 * nb) * self.ratio) + 16
        bufin = [np.concatenate([t, p]) for t, p in zip(self.temp, _planes(packet, self.in_ch, self.out_ch))]
        src = len(bufin[0])
        if src == 0:
            return np.zeros(0, np.int16)
        n = min(out_count(self.in_rate, self.out_rate, src, self.index, self.frac), lenout)
        I = positions(self.in_rate, self.out_rate, n, self.index, self.frac)
        outs = [filter_channel(b, self.in_rate, self.out_rate, I) for b in bufin]
        total = self.frac + n * self.in_rate * PHASES
        index = self.index + total // self.out_rate
        self.frac = total % self.out_rate
        consumed = max(index, 0) >> PHASE_SHIFT
        self.index = index & (PHASES - 1) if index >= 0 else index
        self.temp = [b[consumed:] for b in bufin]
        return _mux(outs, self.out_ch)


def resample_packets(x, in_ch, in_rate, out_ch, out_rate, sizes):
    """(concatenated output, per-call counts) of audio_resample over packets of `sizes` frames"""
    r = Packetised(out_ch, in_ch, out_rate, in_rate)
    outs, counts, pos = [], [], 0
    for nb in sizes:
        o = r.feed(x[pos * in_ch:(pos + nb) * in_ch])
        pos += nb
        outs.append(o)
        counts.append(len(o) // out_ch)
    return (np.concatenate(outs) if outs else np.zeros(0, np.int16)), counts
