"""Crafted audio for the ADPCM kernels (a helper of the tests, imported as scan_builder, coef_builder and pixel_builder are).

Ordinary content -- synthetic audio, noise, silence -- reaches 576 of the plain quantiser's 1424 (step index, nibble)
cells, only even chunk sizes laid back to back, and none of the decoder's states an encoder never writes.  Here every
chunk is written sample by sample (or byte by byte) so that a named state is met on purpose:

  A  cells    a closed-loop stream: the model below tracks (predictor, step index) and the generator emits the sample
              that makes the wanted delta.  For every index 0..88, every magnitude q 0..7, both signs and two edges -- the
              smallest |d| with that quotient, ceil(q step / 4) (q = 0: d = 0 and d = -1), and the largest,
              ceil((q + 1) step / 4) - 1 (q = 7: the sample at the rail the delta points to, from at least 32768 away) --
              2848 cases over the 1424 cells, each followed by a sample whose quotient shows a wrong factor in the table cell
              the case read (an exact multiple of the step, or the largest delta of a quotient); then both rails:
              d = +65535, d = -65535, and runs along each rail that clamp the predictor from the indices they pass.  Where a
              delta does not fit from where the predictor stands, samples at the far rail and down-steps of magnitude 3 take
              it across first.  The stream is coded as chunks of CHUNK samples (the predictor
              restarts from a chunk's first sample, adpcm.c:464, and the generator knows it), the index carried.
  B  lengths  every even count 0..130 (0..4 tiles of 32 samples with every remainder), 254..288 (a second flush group),
              1376..1380, in waves of 64 chunks whose tile counts ascend, descend, have the longest row at lane 0, at
              lane 63, alone among empty rows, and have no full tile at all; content: slices of A and full-scale noise
  C  layout   Layout: 0 or 1 spare samples between PCM chunks (addresses 0 and 2 modulo 4), 0..3 spare bytes between
              blob chunks, everything outside the chunks poisoned
  D  trellis  short chunks (2..300 samples, the freeze at 128 +-2, odd counts) of silence, constants, full-scale squares,
              slices of A and quiet noise: ties, duplicates, full frontiers, renormalisation, squares past int32
  decoder     nibble bodies no encoder writes: every byte value from every start index, header indices past 88, runs of
              0x77 / 0xFF / 0x00 / 0x88 around the 12-byte lane run and the 768-byte tile of amv_adpcm_decode_kernel

The expected bytes are never made here: they are the oracle's (amvo_adpcm_encode_chunk, amvo_adpcm_encode_chunk_trellis,
amvo_adpcm_decode_chunk).  The models below restate adpcm_ima_compress_sample (adpcm.c:219-227), AdpcmImaExpandNibble
(AdpcmIma.c:170-204) and adpcm_compress_trellis (adpcm.c:287-443, IMA branch) for steering the generator, for counting
what the corpus reaches and for the states the oracle does not hand out (the decoder's end index); tests/test_pcm_builder.py
holds them to the oracle byte for byte on the whole corpus, which is what licenses their counts.

Cases of part A that are left out (NOT_REACHED): none -- the generator steers the predictor to the far rail before a
delta that would not fit, which also reaches the large edges at indices 87 and 88.
"""
import bisect

import numpy as np

STEP = (7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 19, 21, 23, 25, 28, 31, 34, 37, 41, 45,
        50, 55, 60, 66, 73, 80, 88, 97, 107, 118, 130, 143, 157, 173, 190, 209, 230, 253, 279, 307,
        337, 371, 408, 449, 494, 544, 598, 658, 724, 796, 876, 963, 1060, 1166, 1282, 1411, 1552, 1707, 1878, 2066,
        2272, 2499, 2749, 3024, 3327, 3660, 4026, 4428, 4871, 5358, 5894, 6484, 7132, 7845, 8630, 9493, 10442, 11487, 12635, 13899,
        15289, 16818, 18500, 20350, 22385, 24623, 27086, 29794, 32767)
ADJUST = (-1, -1, -1, -1, 2, 4, 6, 8) * 2
LOOK = (1, 3, 5, 7, 9, 11, 13, 15, -1, -3, -5, -7, -9, -11, -13, -15)
LO, HI = -32768, 32767
CHUNK = 1378                    # samples per chunk of part A (22050 Hz at 16 frames a second)
POISON = 0xEE
CELLS, CASES = 89 * 16, 89 * 8 * 2 * 2
NOT_REACHED = ()                # (index, q, minus, edge) cases of part A the generator leaves out, each with its reason
TILE = 32                       # amv_adpcm.hip kTile: samples per row and staging tile
FREEZE = 128


def _clip16(v):
    return HI if v > HI else (LO if v < LO else v)


def _clip_idx(v):
    return 0 if v < 0 else (88 if v > 88 else v)


def _trunc_div(a, b):
    """C's division (b > 0)"""
    return a // b if a >= 0 else -((-a) // b)


def _ceil_div(a, b):
    return -((-a) // b)


# ------------------------------------------------------------------------------------------------ the plain quantiser

class Events:
    """what a walk of the plain quantiser or of the decoder met"""

    def __init__(self):
        self.cells = set()                       # (index, nibble)
        self.cases = set()                       # (index, q, minus, edge): part A's 2848
        self.clamp_hi, self.clamp_lo = set(), set()     # indices from which the predictor was clamped at 32767 / -32768
        self.index_hi = set()                    # adjustments (2, 4, 6, 8) that were clamped at 88
        self.index_lo = 0                        # moves below 0
        self.exact = set()                       # (index, k): |d| * 4 == k * step, k 0..7
        self.big = 0                             # |d| >= 32768
        self.plus_65535 = self.minus_65535 = 0
        # the 89 x 8 cells of amv_adpcm.hip's table hold the quotient factor of the index they lead to: it shows in the NEXT
        # sample's quotient alone.  (index, q) of the cells whose next sample, in the same chunk, was an exact multiple
        # k * step with 1 <= k <= 7 (a factor too small gives k - 1) / the largest |d| of a quotient below 7 (too large: + 1)
        self.last = None
        self.exact_after, self.large_after = set(), set()

    def move(self, index, nibble, pred, moved):
        self.cells.add((index, nibble))
        if moved > HI:
            self.clamp_hi.add(index)
        if moved < LO:
            self.clamp_lo.add(index)
        to = index + ADJUST[nibble]
        if to > 88:
            self.index_hi.add(ADJUST[nibble])
        if to < 0:
            self.index_lo += 1

    def summary(self):
        return ("cells %d/%d, cases %d/%d, predictor clamped at +rail from %d indices, at -rail from %d, index clamped at 88 by %s, "
                "at 0 %d times, exact multiples (index, k) %d/712, |d| >= 32768 %d times, d = +65535 %d, d = -65535 %d, table cells "
                "followed by an exact multiple %d/712, by a largest delta %d/712"
                % (len(self.cells), CELLS, len(self.cases), CASES, len(self.clamp_hi), len(self.clamp_lo), sorted(self.index_hi),
                   self.index_lo, len(self.exact), self.big, self.plus_65535, self.minus_65535, len(self.exact_after),
                   len(self.large_after)))


def edge_delta(step, q, minus, edge):
    """|d| of a case of part A (None: the rail case, whose delta depends on where the predictor stands)"""
    if edge == 0:
        return _ceil_div(q * step, 4) if q else (1 if minus else 0)
    return _ceil_div((q + 1) * step, 4) - 1 if q < 7 else None


def compress_sample(pred, index, sample, ev=None):
    """adpcm_ima_compress_sample, adpcm.c:219-227 -> (nibble, predictor, index)"""
    d = sample - pred
    step = STEP[index]
    ad = -d if d < 0 else d
    quot = ad * 4 // step
    q = 7 if quot > 7 else quot
    minus = 1 if d < 0 else 0
    nibble = q + 8 * minus
    moved = pred + _trunc_div(step * LOOK[nibble], 8)
    if ev is not None:
        ev.move(index, nibble, pred, moved)
        if ad * 4 % step == 0 and quot < 8:
            ev.exact.add((index, quot))
            if quot and ev.last:
                ev.exact_after.add(ev.last)
        if quot < 7 and ad == _ceil_div((quot + 1) * step, 4) - 1 and ev.last:
            ev.large_after.add(ev.last)
        ev.last = (index, q)
        if ad >= 32768:
            ev.big += 1
        if d == 65535:
            ev.plus_65535 += 1
        if d == -65535:
            ev.minus_65535 += 1
        for edge in (0, 1):
            want = edge_delta(step, q, minus, edge)
            if want is None:
                hit = quot >= 7 and ad >= 32768 and sample == (LO if minus else HI)
            else:
                hit = ad == want
            if hit:
                ev.cases.add((index, q, minus, edge))
    return nibble, _clip16(moved), _clip_idx(index + ADJUST[nibble])


def header(first, index, count):
    """adpcm.c:465-466,479: le16 first sample, le16 step index, le32 sample count"""
    return bytes([first & 0xff, (first >> 8) & 0xff, index & 0xff, (index >> 8) & 0xff,
                  count & 0xff, (count >> 8) & 0xff, (count >> 16) & 0xff, (count >> 24) & 0xff])


def encode_chunk(samples, index, ev=None, trace=None):
    """the AMV case of adpcm_encode_frame (adpcm.c:461-498) -> (chunk bytes, index after); trace: the (index, nibble) cell
    of every sample"""
    x = [int(v) for v in samples]
    pairs = len(x) // 2
    if pairs == 0:
        return header(0, index, 0), index
    pred = x[0]
    out = bytearray(header(pred, index, 2 * pairs))
    if ev is not None:
        ev.last = None
    for k in range(pairs):
        i0 = index
        hi, pred, index = compress_sample(pred, index, x[2 * k], ev)
        i1 = index
        lo, pred, index = compress_sample(pred, index, x[2 * k + 1], ev)
        if trace is not None:
            trace += [(i0, hi), (i1, lo)]
        out.append((hi << 4) | lo)
    return bytes(out), index


def expand_nibble(pred, index, nibble, ev=None):
    """AdpcmImaExpandNibble, AdpcmIma.c:170-204 with shift 3 -> (predictor, index)"""
    diff = ((2 * (nibble & 7) + 1) * STEP[index]) >> 3
    moved = pred - diff if nibble & 8 else pred + diff
    if ev is not None:
        ev.move(index, nibble, pred, moved)
    return _clip16(moved), _clip_idx(index + ADJUST[nibble])


def decode_chunk(chunk, ev=None):
    """AMVDec.c:312-320 + AdpcmImaDecodeFrame (mono, high nibble first) -> (samples, (predictor, index) at the end)"""
    chunk = bytes(chunk)
    pred = int.from_bytes(chunk[0:2], "little", signed=True)
    index = _clip_idx(chunk[2])
    out = np.zeros(2 * (len(chunk) - 8), np.int16)
    for k, byte in enumerate(chunk[8:]):
        pred, index = expand_nibble(pred, index, byte >> 4, ev)
        out[2 * k] = pred
        pred, index = expand_nibble(pred, index, byte & 15, ev)
        out[2 * k + 1] = pred
    return out, (pred, index)


# ------------------------------------------------------------------------------------------------ the trellis search

class TrellisEvents:
    def __init__(self):
        self.duplicates = 0       # candidates dropped because a node of the new frontier decodes to the same value (:347-352)
        self.full = 0             # candidates dropped against a full frontier (:342)
        self.replaced = 0         # candidates that took the worst node's place
        self.ties = 0             # insertions that met an equal ssd
        self.renormalised = 0     # :398-402
        self.freezes = 0          # :405-417
        self.wide = 0             # steps with a candidate |sample - dec| >= 46341: the square leaves int32

    def names(self):
        return ("duplicates", "full", "replaced", "ties", "renormalised", "freezes", "wide")

    def summary(self):
        return ", ".join("%s %d" % (k, getattr(self, k)) for k in self.names())


def encode_chunk_trellis(samples, index, trellis, ev=None):
    """adpcm_compress_trellis, adpcm.c:287-443 (IMA branch), in the AMV case's framing (:461-487) -> (chunk bytes, index after).
    A node is [ssd, sample1, step index, path]; a path is (nibble, the path before)."""
    x = [int(v) for v in samples]
    n = len(x) // 2 * 2
    if n == 0:
        return header(0, index, 0), index
    frontier = 1 << trellis
    nodes = [[0, x[0], index, None]]
    nib = [0] * n
    froze = -1

    def back(path, hi, lo):
        for k in range(hi, lo, -1):
            nib[k] = path[0]
            path = path[1]

    for i in range(n):
        sample = x[i]
        nxt, ssds, seen = [], [], set()           # the new frontier sorted by ssd, its ssds, its decoded values
        wide = False
        for j, (base, predictor, step, path) in enumerate(nodes):
            rng = 1 if j < frontier // 2 else 0                               # :333
            st = STEP[step]
            div = _trunc_div((sample - predictor) * 4, st)                    # :376
            nmin = min(max(div - rng, -7), 6)
            nmax = min(max(div + rng, -6), 7)
            if nmin <= 0:
                nmin -= 1                                                     # distinguish -0 from +0
            if nmax < 0:
                nmax -= 1
            for nidx in range(nmin, nmax + 1):
                nibble = 7 - nidx if nidx < 0 else nidx
                dec = _clip16(predictor + _trunc_div(st * LOOK[nibble], 8))
                d = sample - dec
                if d >= 46341 or d <= -46341:
                    wide = True
                ssd = (base + ((d * d) & 0xffffffff)) & 0xffffffff
                full = len(nxt) == frontier
                if full and ssd >= ssds[-1]:                                  # :342
                    if ev is not None:
                        ev.full += 1
                    continue
                if dec in seen:                                               # :347-352
                    if ev is not None:
                        ev.duplicates += 1
                    continue
                k = bisect.bisect_right(ssds, ssd)                            # the first node it beats (:353-354)
                if ev is not None and k > 0 and ssds[k - 1] == ssd:
                    ev.ties += 1
                if full:
                    seen.discard(nxt.pop()[1])
                    ssds.pop()
                    if ev is not None:
                        ev.replaced += 1
                nxt.insert(k, [ssd, dec, _clip_idx(step + ADJUST[nibble]), (nibble, path)])
                ssds.insert(k, ssd)
                seen.add(dec)
        if ev is not None and wide:
            ev.wide += 1
        nodes = nxt
        if nodes[0][0] > (1 << 28):                                           # :398-402
            off = nodes[0][0]
            for node in nodes[1:]:
                node[0] = (node[0] - off) & 0xffffffff
            nodes[0][0] = 0
            if ev is not None:
                ev.renormalised += 1
        if i == froze + FREEZE:                                               # :405-417
            back(nodes[0][3], i, froze)
            froze = i
            nodes = nodes[:1]
            if ev is not None:
                ev.freezes += 1
    back(nodes[0][3], n - 1, froze)
    out = bytearray(header(x[0], index, n))
    for k in range(n // 2):
        out.append((nib[2 * k] << 4) | nib[2 * k + 1])
    return bytes(out), nodes[0][2]


# ------------------------------------------------------------------------------------------------ part C: the layout

class Layout:
    """n chunks of `sizes` samples: where each lies in the PCM array (spare samples behind each chunk: pcm_gaps, cycled) and
    in the blob (8 + size // 2 bytes each, spare bytes behind each: blob_gaps, cycled).  One more byte behind the blob is
    the sentinel."""

    def __init__(self, sizes, pcm_gaps=(0,), blob_gaps=(0,), name=""):
        self.name = name
        self.sizes = np.array(sizes, np.uint32)
        self.n = len(sizes)
        pg = [pcm_gaps[i % len(pcm_gaps)] for i in range(self.n)]
        bg = [blob_gaps[i % len(blob_gaps)] for i in range(self.n)]
        self.lens = np.array([8 + int(s) // 2 for s in sizes], np.uint32)
        self.pcm_offs = np.cumsum([0] + [int(s) + g for s, g in zip(sizes, pg)])[:-1].astype(np.uint64)
        self.offs = np.cumsum([0] + [int(l) + g for l, g in zip(self.lens, bg)])[:-1].astype(np.uint64)
        self.pcm_samples = int(sum(int(s) for s in sizes) + sum(pg))
        self.blob_bytes = int(self.lens.sum() + sum(bg)) + 1

    def pcm(self, chunks):
        """the chunks' samples in place; the spare samples are loud and alternate in sign"""
        out = np.where(np.arange(self.pcm_samples) % 2 == 0, 30000, -30000).astype(np.int16)
        for o, c in zip(self.pcm_offs, chunks):
            out[int(o):int(o) + len(c)] = c
        return out

    def blob(self, chunks, fill=POISON):
        out = np.full(self.blob_bytes, fill, np.uint8)
        for o, c in zip(self.offs, chunks):
            out[int(o):int(o) + len(c)] = np.frombuffer(bytes(c), np.uint8)
        return out

    def chunk_of_byte(self, at):
        """(chunk, offset inside it) of blob byte `at`; (chunk, None) for a spare byte behind that chunk"""
        i = int(np.searchsorted(self.offs, at, "right")) - 1
        k = at - int(self.offs[i])
        return i, (k if k < int(self.lens[i]) else None)


# the layouts every batch goes through: (name, spare samples, spare bytes)
LAYOUTS = (("packed", (0,), (0,)), ("odd-1", (1,), (1,)), ("mixed-2", (1, 0, 0, 1, 1), (2,)), ("odd-3", (1,), (3,)),
           ("mixed-0123", (0, 1, 1), (0, 1, 2, 3)))


def layouts(sizes):
    return [Layout(sizes, pg, bg, name) for name, pg, bg in LAYOUTS]


# ------------------------------------------------------------------------------------------------ part A: every cell

class _Loop:
    """the generator's view of the encoder: the stream so far, and (predictor, index) behind it"""

    def __init__(self, chunk):
        self.out, self.pred, self.index, self.chunk, self.ev = [], 0, 0, chunk, Events()

    def at_start(self):
        return len(self.out) % self.chunk == 0

    def emit(self, sample):
        assert LO <= sample <= HI, sample
        if self.at_start():
            self.pred = sample                     # adpcm.c:464
            self.ev.last = None
        _, self.pred, self.index = compress_sample(self.pred, self.index, sample, self.ev)
        self.out.append(sample)

    def step_toward(self, index, low, swing=False):
        """one sample that moves the step index toward `index`: up with the smallest delta of a magnitude 4..7, down with
        d = 0 and d = -1; low: the one that takes the predictor down where there is a choice.  swing: down with the largest
        delta of magnitude 3 instead (step - 1, or as far as the rail lets it), for a predictor that has to cross the range"""
        step = STEP[self.index]
        if self.index > index:
            d = -1 if low and self.pred > LO else 0
            if swing:
                d = _clip16(self.pred - (step - 1) if low else self.pred + (step - 1)) - self.pred
        else:
            need = index - self.index
            q = 7 if need >= 8 else (need + 1) // 2 + 3
            d = _ceil_div(q * step, 4) * (-1 if low else 1)
            if not LO <= self.pred + d <= HI:
                d = -d
        self.emit(self.pred + d)

    def probe(self, low, large):
        """the sample behind a case: one whose quotient depends on the factor the case's cell handed on -- an exact multiple
        k * step (k 1..3 where step * k is a multiple of 4: the index goes down as a steering sample would take it; else
        k = 4, d = step), or (large) the largest |d| of a quotient 1..3"""
        step = STEP[self.index]
        pick = len(self.out) % 3
        if large:
            mag = _ceil_div((pick + 2) * step, 4) - 1
        else:
            ks = [k for k in (1, 2, 3) if k * step % 4 == 0] or [4]
            mag = ks[pick % len(ks)] * step // 4
        d = -mag if low else mag
        if not LO <= self.pred + d <= HI:
            d = -d
        self.emit(self.pred + d)

    def to_rail(self, rail):
        """samples at a rail until the predictor stands on it"""
        for _ in range(64):
            if self.pred == rail and not self.at_start():
                return
            self.emit(rail)
        raise AssertionError("the predictor does not settle on the rail")


def _case_delta(case, pred, step):
    """the delta that makes `case` from predictor `pred`, None if no sample gives it from there"""
    _, q, minus, edge = case
    mag = edge_delta(step, q, minus, edge)
    if mag is None:
        d = (LO if minus else HI) - pred
        return d if abs(d) >= max(32768, _ceil_div(7 * step, 4)) else None
    d = -mag if minus else mag
    return d if LO <= pred + d <= HI else None


def part_a(chunk=CHUNK):
    """-> (samples int16, even count; Events of the generator's own walk; cases it gave up on)"""
    g = _Loop(chunk)
    missed = []
    for index in range(89):
        for minus in (0, 1):
            for q in range(8):
                for edge in (0, 1):
                    case = (index, q, minus, edge)
                    if case in g.ev.cases and (index, q) in (g.ev.large_after if edge else g.ev.exact_after):
                        continue                             # (met on the way to another case, probe and all)
                    pushes = 0
                    for _ in range(400):
                        if g.at_start() or len(g.out) % chunk >= chunk - 2:
                            g.emit(g.pred)                   # (a case and the probe behind it stay inside one chunk)
                        elif g.index != index:
                            g.step_toward(index, not minus, pushes > 0)
                        else:
                            d = _case_delta(case, g.pred, STEP[index])
                            if d is not None:
                                g.emit(g.pred + d)
                                g.probe(not minus, edge == 1)
                                break
                            if pushes == 8:
                                break
                            pushes += 1
                            g.emit(HI if minus else LO)      # to the far rail: the delta does not fit from here
                    if case not in g.ev.cases:
                        missed.append(case)
    # both rails: the two largest deltas, then a run along each rail from index 88 down
    for rail in (LO, HI):
        g.to_rail(rail)
        g.emit(-1 - rail)                                    # d = +65535 from the low rail, -65535 from the high one
    for rail in (HI, LO):
        for k in range(64):
            if g.index == 88:
                break
            g.emit(HI if k % 2 else LO)
        g.to_rail(rail)
        for _ in range(120):
            if g.index == 0:
                break
            # along the high rail d = 0 overshoots every time; along the low one d = -1 does whenever the predictor has
            # come off the rail by less than step / 8
            g.emit(HI if rail == HI else (g.pred - 1 if g.pred > LO else LO))
    if len(g.out) % 2:
        g.emit(g.pred)
    return np.array(g.out, np.int16), g.ev, missed


# ------------------------------------------------------------------------------------------------ part B: lengths

EVENS = tuple(range(0, 132, 2))
LENGTHS = EVENS + (254, 256, 258, 286, 288, 1376, 1378, 1380)


def waves():
    """name -> 64 chunk sizes: the orders of tile counts within one wave that encode_rows depends on"""
    w = {}
    w["ascending"] = list(EVENS[:60]) + [130, 256, 288, 1378]
    w["descending"] = [1380, 286, 258, 128] + list(EVENS[63:3:-1])
    w["longest at lane 0"] = [1376] + [EVENS[(7 * k) % 66] for k in range(63)]
    w["longest at lane 63"] = [EVENS[(11 * k + 5) % 66] for k in range(63)] + [1380]
    w["one long row"] = [0] * 17 + [1378] + [0] * 46
    w["no full tile"] = [EVENS[(5 * k + 3) % 16] for k in range(64)]
    used = set(s for v in w.values() for s in v)
    rest = [s for s in LENGTHS if s not in used]
    w["the rest"] = (rest + [254, 122, 34, 62, 64, 66, 94, 96, 98, 126] * 7)[:64]
    return w


def wave_properties(sizes):
    tiles = [s // TILE for s in sizes]
    return {"ascending": tiles == sorted(tiles) and tiles[0] < tiles[-1],
            "descending": tiles == sorted(tiles, reverse=True) and tiles[0] > tiles[-1],
            "longest at lane 0": tiles[0] == max(tiles) and tiles.count(max(tiles)) == 1,
            "longest at lane 63": tiles[-1] == max(tiles) and tiles.count(max(tiles)) == 1,
            "one long row": sum(1 for t in tiles if t) == 1 and max(sizes) > 4 * TILE and sum(sizes) == max(sizes),
            "no full tile": max(tiles) == 0 and max(sizes) > 0}


# ------------------------------------------------------------------------------------------------ the corpus

class Batch:
    """chunks that go through a kernel in one call: their samples, the index each starts from when the chunks are
    independent (starts), and what the oracle makes of them (computed once)"""

    def __init__(self, name, chunks, starts=None):
        self.name = name
        self.chunks = [np.ascontiguousarray(c, np.int16) for c in chunks]
        self.sizes = [len(c) for c in self.chunks]
        self.n = len(chunks)
        self.starts = None if starts is None else [int(s) for s in starts]
        self._want = {}

    def want(self, orc, trellis=0, starts=None, first=0):
        """(chunks' bytes, start indices, end indices) from the oracle.  starts None: one stream from `first`"""
        key = (trellis, None if starts is None else tuple(starts), first)
        if key not in self._want:
            out, begins, ends, idx = [], [], [], first
            for i, c in enumerate(self.chunks):
                if starts is not None:
                    idx = starts[i]
                begins.append(idx)
                if len(c) < 2:
                    chunk = header(0, idx, 0)
                elif trellis:
                    chunk, idx = orc.adpcm_encode_chunk_trellis(c, idx, trellis)
                else:
                    chunk, idx = orc.adpcm_encode_chunk(c, idx)
                out.append(chunk)
                ends.append(idx)
            self._want[key] = (out, begins, ends)
        return self._want[key]

    def cell_of(self, chunk, offset, start):
        """where the plain model stands at byte `offset` of chunk `chunk` coded from `start`: for a failure's message"""
        if offset is None:
            return "spare byte behind the chunk"
        if offset < 8:
            return "header byte %d" % offset
        trace = []
        encode_chunk(self.chunks[chunk], start, None, trace)
        a, b = trace[2 * (offset - 8)], trace[2 * (offset - 8) + 1]
        return "samples %d, %d: cells (index %d, nibble %d), (index %d, nibble %d)" % (2 * (offset - 8), 2 * (offset - 8) + 1, a[0], a[1], b[0], b[1])


def explain(batch, lay, got, want, start_of=None):
    """the first differing byte of two blobs, named: case, layout, chunk, byte and -- start_of(chunk) given: the index the
    plain quantiser starts that chunk from -- the cells of that byte's samples"""
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    if bad.size == 0:
        return None
    at = int(bad[0])
    i, k = lay.chunk_of_byte(at)
    names = getattr(batch, "names", None)
    where = batch.cell_of(i, k, start_of(i)) if start_of else ("header" if k is not None and k < 8 else "spare byte" if k is None else "nibbles")
    return ("%s, layout %s: %d bytes differ, the first at blob byte %d = chunk %d (%s%d samples) byte %s: got %#04x, want %#04x; %s"
            % (batch.name, lay.name, bad.size, at, i, names[i] + ", " if names else "", batch.sizes[i], k, int(got[at]), int(want[at]), where))


def _cut(stream, size):
    return [stream[o:o + size] for o in range(0, len(stream), size)]


def _sequential_starts(chunks, first=0):
    starts, idx = [], first
    for c in chunks:
        starts.append(idx)
        _, idx = encode_chunk(c, idx)
    return starts


def _content(a, noise, sizes, salt):
    """chunk k: a slice of part A (k even) or of full-scale noise (k odd), each from a place of its own"""
    chunks = []
    for k, s in enumerate(sizes):
        src = noise if k % 2 else a
        o = (salt + 977 * k) % (len(src) - 1400)
        chunks.append(src[o:o + s].copy())
    return chunks


def squares(size, period):
    x = np.empty(size, np.int16)
    x[:] = np.where((np.arange(size) // period) % 2 == 0, HI, LO)
    return x


D_SIZES = (2, 4, 6, 16, 34, 126, 128, 130, 256, 258, 300, 1, 3, 129)


def part_d(a, rng):
    """-> [(name, samples)]: short chunks for the trellis search"""
    quiet = rng.integers(-40, 41, 4096).astype(np.int16)
    out = []
    for k, s in enumerate(D_SIZES):
        out.append(("silence %d" % s, np.zeros(s, np.int16)))
        out.append(("constant %d" % s, np.full(s, (-32768, 32767, 1000, -3, 12345)[k % 5], np.int16)))
        out.append(("squares %d period %d" % (s, 1 + k % 4), squares(s, 1 + k % 4)))
        out.append(("part A %d" % s, a[(1009 * k) % (len(a) - 400):][:s].copy()))
        out.append(("quiet noise %d" % s, quiet[300 * k % 3000:][:s].copy()))
    return out


RUN_LENGTHS = (11, 12, 13, 767, 768, 769, 1536, 1537)
# byte of the run -> the header it starts from: the index walks to its other end, the predictor to a rail and stays there
RUN_STARTS = {0x77: (LO, 0), 0xFF: (HI, 0), 0x00: (5000, 88), 0x88: (-5000, 88)}


def decoder_only():
    """-> [(name, chunk bytes)]: bodies the encoders never write"""
    out = []
    preds = (0, HI, LO, 1234, -20000, 32000, -32700, 7)
    for index in range(89):
        for byte in range(256):
            out.append(("byte %#04x from index %d" % (byte, index), header(preds[(byte + index) % 8], index, 2) + bytes([byte])))
    body = bytes((37 * k + 11) % 256 for k in range(700))
    for index in (89, 255, 128):
        out.append(("header index %d" % index, header(-5, index, 2 * len(body)) + body))
    for byte, (pred, index) in RUN_STARTS.items():
        for n in RUN_LENGTHS:
            out.append(("%d bytes of %#04x" % (n, byte), header(pred, index, 2 * n) + bytes([byte]) * n))
    return out


class Corpus:
    pass


_CACHE = {}


def corpus(seed=0x9C3A):
    """the whole corpus (built once per process; nothing in it depends on the oracle)"""
    if seed in _CACHE:
        return _CACHE[seed]
    rng = np.random.default_rng(seed)
    c = Corpus()
    c.a, c.a_events, c.a_missed = part_a()
    c.noise = rng.integers(-32768, 32768, 16384).astype(np.int16)
    a_chunks = _cut(c.a, CHUNK)
    c.batch_a = Batch("part A", a_chunks, _sequential_starts(a_chunks))
    w = waves()
    c.waves = w
    b1 = w["ascending"] + w["descending"] + w["longest at lane 0"] + [130, 0, 1380, 62, 2]
    b2 = w["longest at lane 63"] + w["one long row"] + w["no full tile"] + w["the rest"]
    c.batches_b = []
    for name, sizes, salt in (("part B, batch 1", b1, 3), ("part B, batch 2", b2, 5003)):
        chunks = _content(c.a, c.noise, sizes, salt)
        c.batches_b.append(Batch(name, chunks, [(31 * k + 7) % 89 for k in range(len(sizes))]))
    c.d_cases = part_d(c.a, rng)
    c.batch_d = Batch("part D", [x for _, x in c.d_cases], [(37 * k + 88) % 89 for k in range(len(c.d_cases))])
    c.batch_d.names = [n for n, _ in c.d_cases]
    c.decoder_only = decoder_only()
    _CACHE[seed] = c
    return c
