"""Crafted blocks and states for the -nr noise reduction (a helper of the tests, imported as pixel_builder is).

The offsets of -nr have no accessor: they show only through the coded levels and through the state that comes out.  So
every case here is a short stream -- a size, an nr, a start state, frames written block by block -- built so that one wrong
offset, sign or index changes a level or a sum.  Blocks come from pixel_builder (exact transform outputs from _aim_output,
the quantiser's thresholds from ac_threshold, DC rounding ties from dc_ties, extreme outputs from range_patterns), start
states from solving  offset = (nr * count + s / 2) / (s + 1)  for the sum s of each position.

  A  thresholds   from a handed state (count 65536) with 63 pairwise different AC offsets: for every AC position, both
                  components and both signs two blocks whose output there is +-(offset + T) and +-(offset + T - 1), T the
                  first output that quantises to +-1 -- the dead zone leaves +-T (a level of +-1) and +-(T - 1) (0), so a
                  dead zone one too wide or too narrow changes a level.  At nr_max with qbias 0 and 128, and with offsets
                  of 2 .. 64 at a low nr.  48x32, a frame a case.  The same blocks once at 176x24 (both segments of an MCU
                  row, the last row half outside the picture) and once at 22x38 (padding blocks both ways)
  B  offsets from 32768 up: from the zero state a frame of all-zero samples (every sum 0), so the next frame's 64 offsets are
                  all (nr * 6) & 0xFFFF: 65534, 32766 and the wrapped 2; noise under them, then threshold blocks against the
                  offsets that follow.  A handed state with 32767 and 32768 on neighbouring positions
  C  the DC       D - offset of 0, of 1, below 0, and on both sides of every rounding tie of dc_ties(); blocks of all 0
                  (D = 0) and all 255 (D = 16320), whole frames of them
  D  range        every max_n / min_n pattern, checkerboard and stripes: from the zero state (frame 0 under offsets of 0) and
                  from a handed state with large offsets
  E  the chain    counts of 65536 (stays) and 65537 (halves at once), odd sums and an odd count at a halving, sums of 0, 1
                  and 2, every sum at 16320 * (count + 1) under nr_max (the largest dividend the bound allows), quotients of
                  65536 (stored as 0), 65535 and above 65536
  F  identity     per group of eight positions a frame in which only they carry large outputs, under offsets far apart

Every start state lies inside the bound of amv_nr_plan.h (in_bound): inside it nothing wraps and tests/nr_ref.py is exact.
The expectation is never made here: it is nr_ref.encode_stream / nr_trellis_ref.encode_stream of the case.
"""
import numpy as np

import nr_ref as N
import pixel_builder as pb

LARGEST = 16320                      # amv_nr_plan.h: kNrLargest
FULL = 1 << 16                       # the count at which a stream settles
SEED = 0x2E01
GROUPS = "ABCDEF"
DROP_CAP = 0.05                      # of group A's (position, sign, component) triples


def count_start_most(blocks):
    return max(FULL, blocks)


def count_most(blocks):
    return count_start_most(blocks) + blocks


def nr_max(blocks):
    """amv_nr_plan.h's nr_max, restated (test_nr_builder pins it to amvhip_encode_nr_max)"""
    c0 = count_start_most(blocks)
    return (0x7FFFFFFF - LARGEST * (c0 + 1) // 2) // c0


NR_MAX = nr_max(6)


def blocks_of(w, h):
    return ((w + 15) // 16) * ((h + 15) // 16) * 6


def in_bound(state, blocks):
    s = np.asarray(state, np.int64)
    return bool(0 <= s[64] <= count_most(blocks) and (s[:64] >= 0).all() and (s[:64] <= LARGEST * (s[64] + 1)).all())


def quotient(nr, count, s):
    """the offset before its 16-bit store"""
    return (nr * count + s // 2) // (s + 1)


def dividend_most(blocks):
    """the largest dividend the bound allows: nr_max on the largest count a frame can start with, every sum full"""
    c0 = count_start_most(blocks)
    return nr_max(blocks) * c0 + LARGEST * (c0 + 1) // 2


def solve_sum(nr, count, target):
    """a sum inside the bound whose quotient is `target`, or None (the quotient falls as the sum grows)"""
    lo, hi = 0, LARGEST * (count + 1)
    while lo < hi:
        mid = (lo + hi) // 2
        if quotient(nr, count, mid) <= target:
            hi = mid
        else:
            lo = mid + 1
    return lo if quotient(nr, count, lo) == target else None


def state_for(nr, count, targets):
    """the state of `count` whose 64 quotients are `targets`, or None where one has no solution"""
    sums = [solve_sum(nr, count, int(t)) for t in targets]
    if any(s is None for s in sums):
        return None
    return np.array(sums + [count], np.int64)


class Case:
    """one stream: name, group, size, nr, qbias, the start state (65 int64), frames [(Y, Cb, Cr) uint8 planes], aims
    {what reach() counts: the least the case must reach}, meta (what the builder placed, for the tests)"""

    def __init__(self, name, group, w, h, nr, state, frames, aims, qbias=0, meta=None):
        self.name, self.group, self.w, self.h, self.nr, self.qbias = name, group, w, h, int(nr), qbias
        self.state = N.new_state() if state is None else np.array(state, np.int64)
        self.frames, self.aims, self.meta = frames, aims, meta or {}
        assert in_bound(self.state, blocks_of(w, h)), name
        assert 0 < self.nr <= nr_max(blocks_of(w, h)), name

    def from_zero(self):
        return not self.state.any()


# ------------------------------------------------------------------------------------------------ frames

def planes_of(blocks, w, h):
    """[mcus * 6, 64] sample blocks (the encoder's order and orientation) -> (Y, Cb, Cr) of a w x h picture: the picture of
    whole MCUs, cut to the size (the encoder starts at the bottom row and the left column)"""
    W, H = (w + 15) // 16 * 16, (h + 15) // 16 * 16
    y, cb, cr = pb.planes_of_blocks(blocks, W, H)
    return (np.ascontiguousarray(y[H - h:, :w]), np.ascontiguousarray(cb[(H - h) // 2:, : w // 2]),
            np.ascontiguousarray(cr[(H - h) // 2:, : w // 2]))


def frame_of(w, h, luma, chroma, rest=0):
    """a frame whose luma blocks are `luma` and chroma blocks `chroma`, in order, the rest flat -> (planes, {id of a given
    block: its place})"""
    n = blocks_of(w, h)
    blocks = np.full((n, 64), rest, np.int16)
    at, li, ci = {}, 0, 0
    for b in range(n):
        if b % 6 < 4 and li < len(luma):
            blocks[b], at[("y", li)] = luma[li], b
            li += 1
        elif b % 6 >= 4 and ci < len(chroma):
            blocks[b], at[("c", ci)] = chroma[ci], b
            ci += 1
    return planes_of(blocks, w, h), at


def flat_frame(w, h, byte):
    return (np.full((h, w), byte, np.uint8), np.full((h // 2, w // 2), byte, np.uint8), np.full((h // 2, w // 2), byte, np.uint8))


def noise_frame(rng, w, h, saturated=False):
    def plane(pw, ph):
        if saturated:
            return rng.choice(np.array([0, 255], np.uint8), (ph, pw))
        return rng.integers(0, 256, (ph, pw)).astype(np.uint8)
    return plane(w, h), plane(w // 2, h // 2), plane(w // 2, h // 2)


def offsets_at(state, nr):
    """the offsets a frame starting from `state` gets (state untouched)"""
    return N.frame_start(np.array(state, np.int64), nr)


def craft_stream(w, h, nr, state, makers):
    """frames made one after another, each maker handed the offsets its frame will get: maker(offsets) -> planes"""
    st, frames = np.array(state, np.int64), []
    for make in makers:
        planes = make(offsets_at(st, nr))
        N.encode_stream([planes], w, h, nr, state=st, want_coef=True)
        frames.append(planes)
    return frames


# ------------------------------------------------------------------------------------------------ what a case reaches

def reach(case):
    """counted with the model over the case's frames: {clamped_dc: blocks with D - offset <= 0, dc_at_0 / dc_at_1:
    D - offset == 0 / 1, live_under_32768: non-zero outputs at a position whose offset is 32768 or more, offsets_32768:
    such offsets over the frames, halvings, quotient_65536 / quotient_above / quotient_65535: offsets whose quotient before
    the store is 65536 / above it / 65535, survivors_above: non-zero outputs left under a quotient above 65536,
    survivors_at_65536: the same under a quotient of exactly 65536,
    d_min, d_max: the DC magnitudes' extremes, ac_max: the largest AC magnitude, divisor_min, dividend_max,
    sum_max: the largest sum in the state afterwards, padding_blocks, frames}"""
    st = case.state.copy()
    out = dict.fromkeys(("clamped_dc", "dc_at_0", "dc_at_1", "live_under_32768", "offsets_32768", "halvings", "quotient_65536",
                         "quotient_above", "quotient_65535", "survivors_above", "survivors_at_65536", "ac_max", "dividend_max"), 0)
    out.update(d_min=LARGEST, d_max=0, divisor_min=1 << 40, frames=len(case.frames))
    out["padding_blocks"] = int(N.outside_blocks(case.w, case.h).sum())
    for y, cb, cr in case.frames:
        coef = N.fdct(N.frame_blocks(y, cb, cr, case.w, case.h, 128))
        out["halvings"] += int(st[64] > FULL)
        off = N.frame_start(st, case.nr)
        raw = quotient(case.nr, int(st[64]), st[:64])
        out["dividend_max"] = max(out["dividend_max"], int((case.nr * st[64] + st[:64] // 2).max()))
        out["divisor_min"] = min(out["divisor_min"], int(st[:64].min()) + 1)
        out["quotient_65536"] += int((raw == 65536).sum())
        out["quotient_65535"] += int((raw == 65535).sum())
        out["quotient_above"] += int((raw > 65536).sum())
        out["offsets_32768"] += int((off >= 32768).sum())
        D = coef[:, 0] + N.DC_SHIFT
        out["clamped_dc"] += int((D - off[0] <= 0).sum())
        out["dc_at_0"] += int((D - off[0] == 0).sum())
        out["dc_at_1"] += int((D - off[0] == 1).sum())
        out["d_min"], out["d_max"] = min(out["d_min"], int(D.min())), max(out["d_max"], int(D.max()))
        out["ac_max"] = max(out["ac_max"], int(np.abs(coef[:, 1:]).max()))
        live = coef != 0
        live[:, 0] = D != 0
        out["live_under_32768"] += int(live[:, off >= 32768].sum())
        den = N.denoise_blocks(st, off, coef, N.DC_SHIFT)
        out["survivors_above"] += int((den[:, 1:][:, raw[1:] > 65536] != 0).sum())
        out["survivors_at_65536"] += int((den[:, 1:][:, raw[1:] == 65536] != 0).sum())
    out["sum_max"] = int(st[:64].max())
    return out


# ------------------------------------------------------------------------------------------------ threshold blocks

_THETA = {}


def theta_of(orc, comp, scan, qbias):
    """pixel_builder.ac_threshold, asked once"""
    k = (comp, scan, qbias)
    if k not in _THETA:
        _THETA[k] = pb.ac_threshold(orc, comp, scan, qbias)
    return _THETA[k]


class Thresholds:
    """the pairs of group A for one set of offsets and one qbias: (position, sign, component) -> (on, under) sample blocks
    whose output at the position is sign * (offset + T) and sign * (offset + T - 1); `dropped`: what _aim_output did not make"""

    def __init__(self, orc, rng, offsets, qbias, only=None):
        self.offsets, self.qbias, self.pairs, self.dropped, self.theta = np.asarray(offsets, np.int64), qbias, {}, [], {}
        for comp in (0, 1):
            for pos in range(1, 64):
                scan = int(pb.SCAN_OF_NATURAL[pos])
                t = self.theta[(pos, comp)] = theta_of(orc, comp, scan, qbias)
                for sign in (1, -1):
                    if only is not None and (pos, sign, comp) not in only:
                        continue
                    want = int(self.offsets[pos]) + t
                    on, under = pb._aim_output(orc, rng, comp, scan, sign * want), pb._aim_output(orc, rng, comp, scan, sign * (want - 1))
                    if on is None or under is None:
                        self.dropped.append((pos, sign, comp))
                    else:
                        self.pairs[(pos, sign, comp)] = (on, under)

    def lists(self, keys):
        """-> (blocks, [(key, index of on, index of under)]) of the pairs of `keys` that exist"""
        blocks, where = [], []
        for k in keys:
            if k in self.pairs:
                where.append((k, len(blocks), len(blocks) + 1))
                blocks += list(self.pairs[k])
        return blocks, where


def _threshold_frame(w, h, th, luma_keys, chroma_keys):
    """-> (planes, triples [(position, sign, component, block of `on`, block of `under`)])"""
    luma, lw = th.lists(luma_keys)
    chroma, cw = th.lists(chroma_keys)
    planes, at = frame_of(w, h, luma, chroma)
    triples = [(k[0], k[1], k[2], at[("y", a)], at[("y", b)]) for k, a, b in lw if ("y", b) in at]
    triples += [(k[0], k[1], k[2], at[("c", a)], at[("c", b)]) for k, a, b in cw if ("c", b) in at]
    return planes, triples


def _spread(lo, step):
    """64 offsets, pairwise different: lo + step * (a permutation of 0 .. 63)"""
    return lo + step * ((np.arange(64) * 29) % 64)


def _group_a(orc, rng, cases, dropped):
    w, h = 48, 32
    small = np.concatenate([[2], 2 + ((np.arange(63) * 29) % 63)])          # AC positions: 2 .. 64, each once
    variants = (("nr_max_q0", NR_MAX, 0, _spread(37, 7)), ("nr_max_q128", NR_MAX, 128, _spread(37, 7)), ("small_offsets", 64, 0, small))
    kept = {}
    for name, nr, qbias, offsets in variants:
        state = state_for(nr, FULL, offsets)
        if state is None:
            dropped.append("A_%s (no state)" % name)
            continue
        assert (offsets_at(state, nr) == offsets).all() and len(set(offsets[1:].tolist())) == 63
        th = Thresholds(orc, rng, offsets, qbias)
        dropped += ["A_%s position %d sign %d component %d" % ((name,) + k) for k in th.dropped]
        kept[name] = (th, state, nr)
        luma = [(p, s, 0) for p in range(1, 64) for s in (1, -1)]
        chroma = [(p, s, 1) for p in range(1, 64) for s in (1, -1)]
        for i in range(21):                                                  # 12 luma pairs and 6 chroma pairs a frame
            lk = [luma[(12 * i + j) % len(luma)] for j in range(12)]
            planes, triples = _threshold_frame(w, h, th, lk, chroma[6 * i: 6 * i + 6])
            cases.append(Case("A_%s_%02d" % (name, i), "A", w, h, nr, state, [planes], {"thresholds": len(triples)}, qbias,
                              {"triples": triples, "offsets": offsets, "theta": th.theta, "variant": name}))
    # the same blocks where the geometry differs: two segments a row and a half-outside last row; padding blocks both ways
    if "nr_max_q0" in kept:
        th, state, nr = kept["nr_max_q0"]
        keys = [(p, s, c) for p in range(1, 64) for s in (1, -1) for c in (0, 1)]
        for name, (w, h), first in (("A_both_segments_176x24", (176, 24), 0), ("A_padding_22x38", (22, 38), 40)):
            n = blocks_of(w, h)
            lk = [k for k in keys[first:] if k[2] == 0][: n // 6 * 2]
            ck = [k for k in keys[first:] if k[2] == 1][: n // 6]
            planes, triples = _threshold_frame(w, h, th, lk, ck)
            more = noise_frame(rng, w, h)
            cases.append(Case(name, "A", w, h, nr, state, [planes, more], {"padding_blocks": 1, "frames": 2}, 0,
                              {"offsets": th.offsets, "theta": th.theta}))
    return {name: len(v[0].pairs) for name, v in kept.items()}


def _few_thresholds(orc, rng, w, h, keys_luma, keys_chroma, qbias=0):
    """a maker for craft_stream: threshold pairs of a few positions against whatever offsets the frame gets (flat where the
    output cannot be reached)"""
    def make(offsets):
        th = Thresholds(orc, rng, offsets, qbias, only=set(keys_luma) | set(keys_chroma))
        return _threshold_frame(w, h, th, keys_luma, keys_chroma)[0]
    return make


def _group_b(orc, rng, cases, dropped):
    w, h = 16, 16
    for nr, first in ((21845, 65534), (5461, 32766), (10923, 2)):
        assert (nr * 6) & 0xFFFF == first
        lk, ck = [(9 + nr % 7, 1, 0), (18 + nr % 5, -1, 0)], [(3 + nr % 4, -1, 1)]
        makers = [lambda off: flat_frame(w, h, 0), lambda off: noise_frame(rng, w, h), _few_thresholds(orc, rng, w, h, lk, ck),
                  lambda off: noise_frame(rng, w, h)]
        frames = craft_stream(w, h, nr, N.new_state(), makers)
        aims = {"d_min": 0, "frames": 4}
        if first >= 32768:
            aims.update(offsets_32768=64, live_under_32768=300, clamped_dc=6)
        cases.append(Case("B_zero_frame_then_%d" % first, "B", w, h, nr, None, frames, aims))
    r, c = np.indices((8, 8))
    targets = np.where(((r + c) & 1).reshape(64) == 1, 32768, 32767)
    state = state_for(NR_MAX, FULL, targets)
    if state is None:
        dropped.append("B_handed_32767_32768")
        return
    pats = dict(pb.range_patterns())
    loud, _ = frame_of(w, h, [pats["max_9"], pats["min_18"], pats["checkerboard"], pats["max_63"]], [pats["min_1"], pats["max_8"]])
    cases.append(Case("B_handed_32767_32768", "B", w, h, NR_MAX, state, [noise_frame(rng, w, h), loud, noise_frame(rng, w, h, True)],
                      {"offsets_32768": 32, "live_under_32768": 150, "clamped_dc": 6}))


def _dc_wants(off0):
    """[(name, the DC output x)] a frame under a DC offset of off0 should hold: D - offset of 0, 1 and -5, and x' on both
    sides of every rounding tie -- the ones a block of 8-bit samples reaches"""
    out = {0: [], 1: []}
    for comp in (0, 1):
        for name, d in (("at_0", 0), ("at_1", 1), ("below_0", -5)):
            out[comp].append((name, d + off0 - N.DC_SHIFT))
        for c, total, level in pb.dc_ties():
            if c == comp:
                out[comp].append(("tie_%d" % level, total + off0))
        out[comp] = [(n, x) for n, x in out[comp] if -8192 <= x <= 8128]
    return out


def _dc_frame(w, h, turn):
    """a maker: the DC blocks against the frame's DC offset, the lists turned by `turn` frames' worth, then all 0 and all 255"""
    def make(offsets):
        wants = _dc_wants(int(offsets[0]))
        n = blocks_of(w, h) // 6
        lists = []
        for comp, per in ((0, 4 * n), (1, 2 * n)):
            blocks = [pb._block_of_sum(x) for _, x in wants[comp]] + [np.full(64, -128, np.int16), np.full(64, 127, np.int16)]
            k = (turn * per) % len(blocks)
            lists.append((blocks[k:] + blocks[:k])[:per])
        return frame_of(w, h, lists[0], lists[1])[0]
    return make


def _group_c(orc, rng, cases, dropped):
    # handed: a DC offset of 20 lets every tie be reached (x + 20 <= 8128), one of 3000 is a large one
    for name, dc_off in (("C_ties_handed_small_offset", 20), ("C_ties_handed_large_offset", 3000)):
        targets = _spread(50, 3)
        targets[0] = dc_off
        state = state_for(NR_MAX, FULL, targets)
        if state is None:
            dropped.append(name)
            continue
        frames = craft_stream(48, 32, NR_MAX, state, [_dc_frame(48, 32, 0), _dc_frame(48, 32, 1)])
        cases.append(Case(name, "C", 48, 32, NR_MAX, state, frames, {"dc_at_0": 2, "dc_at_1": 2, "clamped_dc": 4, "d_min": 0, "d_max": LARGEST, "halvings": 1}))
    # from zero: a frame of all-zero samples, then DC blocks against an offset of nr * 12 at 32x16
    for i, nr in enumerate((2, 1)):
        makers = [lambda off: flat_frame(32, 16, 0)] + [_dc_frame(32, 16, 2 * i + k) for k in range(3)]
        frames = craft_stream(32, 16, nr, N.new_state(), makers)
        cases.append(Case("C_ties_zero_state_nr%d" % nr, "C", 32, 16, nr, None, frames, {"dc_at_0": 1, "dc_at_1": 1, "clamped_dc": 13, "d_min": 0}))
    # whole frames of the extremes: the sums kernel's largest and smallest DC magnitude in every block
    for name, nr in (("C_extremes_zero_state", 300), ("C_extremes_zero_state_clamping", 2000)):
        frames = [flat_frame(16, 16, 0), flat_frame(16, 16, 255), flat_frame(16, 16, 255), flat_frame(16, 16, 0), noise_frame(rng, 16, 16)]
        cases.append(Case(name, "C", 16, 16, nr, None, frames, {"d_min": 0, "d_max": LARGEST, "clamped_dc": 12}))


def _group_d(orc, rng, cases, dropped):
    w, h = 64, 16
    pats = [s for _, s in pb.range_patterns()]
    targets = np.array([2, 5, 17, 60, 250, 900, 2500, 6000])[(np.arange(64) * 5) % 8] + np.arange(64)
    state = state_for(NR_MAX, FULL, targets)
    for k in range(5):
        frames = []
        for f in range(4):
            luma = [pats[(64 * k + 16 * f + j) % len(pats)] for j in range(16)]
            chroma = [pats[(32 * k + 8 * f + j) % len(pats)] for j in range(8)]
            frames.append(frame_of(w, h, luma, chroma)[0])
        cases.append(Case("D_range_zero_state_%d" % k, "D", w, h, 20000, None, frames, {"ac_max": 4000, "frames": 4}, meta={"chroma": [(32 * k + j) % len(pats) for j in range(32)]}))
        if state is None:
            dropped.append("D_range_handed_%d" % k)
        else:
            cases.append(Case("D_range_handed_%d" % k, "D", w, h, NR_MAX, state, frames, {"ac_max": 4000, "frames": 4}))


def _group_e(orc, rng, cases, dropped):
    w, h = 16, 16

    def noisy(n, seed):
        r = np.random.default_rng(seed)
        return [N.picture(w, h, ("texture", "ramp", "noise")[i % 3], seed + i) if i % 2 == 0 else noise_frame(r, w, h, True) for i in range(n)]

    sums = rng.integers(0, LARGEST * (FULL - 8), 64)
    cases.append(Case("E_count_65536_stays", "E", w, h, 4000, np.concatenate([sums, [FULL]]), noisy(3, 11), {"halvings": 1}))
    cases.append(Case("E_count_65537_halves_odd_sums", "E", w, h, 4000, np.concatenate([sums | 1, [FULL + 1]]), noisy(3, 12), {"halvings": 1},
                      meta={"halves_first": True}))
    cases.append(Case("E_odd_count_halves_later", "E", w, h, 4000, np.concatenate([sums | 1, [FULL - 5]]), noisy(4, 13), {"halvings": 1}))
    small = np.array([0, 1, 2] * 22)[:64]
    cases.append(Case("E_sums_0_1_2", "E", w, h, 300, np.concatenate([small, [3]]), noisy(3, 14), {"frames": 3}, meta={"divisor_min": 1}))
    # a count of 0 with sums up to 16320: every offset 0 whatever nr, the sums alone decide what comes out
    cases.append(Case("E_count_0_offsets_0", "E", w, h, NR_MAX, np.concatenate([rng.integers(0, LARGEST + 1, 64), [0]]), noisy(3, 16),
                      {"frames": 3}, meta={"first_offsets": 0}))
    full = np.full(64, LARGEST * (FULL + 1))
    case = Case("E_every_sum_full_nr_max", "E", w, h, NR_MAX, np.concatenate([full, [FULL]]),
                [flat_frame(w, h, 255)] + noisy(2, 15), {"dividend_max": dividend_most(6), "d_max": LARGEST})
    assert NR_MAX * FULL + int(full[0]) // 2 == dividend_most(6) == 2147426272 < 1 << 31
    cases.append(case)
    # quotients around 65536.  Near it neighbouring sums move the quotient by 65536 / nr > 2, so no one state holds both 65535
    # and 65536: 65536 and the first one above it at a count of 65536, 65535 at a count of 65535
    above = next((t for t in range(65537, 65537 + 64) if solve_sum(NR_MAX, FULL, t) is not None), None)
    for name, count, targets, aims in (
            ("E_quotients_65536_and_above", FULL, (65536, above, 300, 65536), {"quotient_65536": 32, "quotient_above": 16, "survivors_above": 20, "survivors_at_65536": 20}),
            ("E_quotient_65535", FULL - 1, (65535, 300), {"quotient_65535": 32})):
        state = None if None in targets else state_for(NR_MAX, count, np.array(targets)[np.arange(64) % len(targets)])
        if state is None:
            dropped.append(name)
            continue
        frames = [noise_frame(rng, w, h, True), noise_frame(rng, w, h, True), noise_frame(rng, w, h)]
        cases.append(Case(name, "E", w, h, NR_MAX, state, frames, aims))


def _group_f(orc, rng, cases, dropped):
    w, h = 48, 32
    offsets = _spread(45, 45)                                                # 45 .. 2880, neighbours far apart
    state = state_for(NR_MAX, FULL, offsets)
    if state is None:
        dropped.append("F (no state)")
        return
    keys = [(p, 1 if p & 1 else -1, c) for p in range(1, 64) for c in (0, 1)]
    th = Thresholds(orc, rng, offsets, 0, only=set(keys))
    for g in range(8):
        ps = [p for p in range(8 * g, 8 * g + 8) if p]
        lk = [(p, 1 if p & 1 else -1, 0) for p in ps]
        ck = [(p, 1 if p & 1 else -1, 1) for p in ps[:6]]
        missing = [k for k in lk + ck if k not in th.pairs]
        if len(missing) > 4:
            dropped.append("F_positions_%d_%d" % (ps[0], ps[-1]))
            continue
        planes, triples = _threshold_frame(w, h, th, lk, ck)
        cases.append(Case("F_positions_%d_%d" % (ps[0], ps[-1]), "F", w, h, NR_MAX, state, [planes], {"thresholds": len(triples)},
                          meta={"triples": triples, "offsets": offsets, "theta": th.theta, "positions": ps}))


_CORPUS = {}


def corpus(orc, seed=SEED):
    """-> (cases, info): info = {dropped: names of what could not be made, pairs: group A's pairs made per variant}.  Built
    once per process."""
    if seed not in _CORPUS:
        cases, dropped, pairs = [], [], None
        for i, group in enumerate((_group_a, _group_b, _group_c, _group_d, _group_e, _group_f)):
            # a generator per group: what a group draws does not depend on the groups in front of it (nor does the fixture)
            made = group(orc, np.random.default_rng([seed, i]), cases, dropped)
            pairs = made if i == 0 else pairs
        assert len({c.name for c in cases}) == len(cases)
        for name in dropped:
            print("nr_builder: dropped", name)
        _CORPUS[seed] = (cases, {"dropped": dropped, "pairs": pairs})
    return _CORPUS[seed]
