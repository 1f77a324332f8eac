"""numpy restatement of the picture rescaler (component_resample, AMVmuxer/ffmpeg/libavcodec/imgresample.c:341-405) for
one plane, and the crafted rescale cases built with it.  TEST INFRASTRUCTURE, and for BUILDING cases and COUNTING what
they reach only: the expectation of every GPU test stays the oracle (orc.img_resample_yuv420, or
img_convert_ref.sws_scale around it); test_rescale_ref.py pins this model to the oracle on every case.

The rule restated: an output sample at (x, y) sits at the 16.16 positions -65536 + x * h_incr and 2 * 65536 + y * v_incr;
the phase is (pos >> 12) & 15; four taps from pos >> 16 on (horizontally) and the four lines up to pos >> 16 (vertically),
each clamped to the plane (the edge sample repeats, also where the plane is narrower than the taps); the horizontal sum
>> 8 is clipped to 0..255 before the vertical sum, whose >> 8 is clipped again.  Increments and filters are those of the
luma sizes for all three planes (img_resample, :474-495).

A case is (name, group, (iw, ih, ow, oh), frames): frames is uint8 [n, iw * ih + 2 * (iw >> 1) * (ih >> 1)], tight
YUV420P pictures with (w >> 1) x (h >> 1) chroma, as the oracle takes them."""
import ctypes
from collections import namedtuple

import numpy as np

POS_BITS, PHASE_BITS, FILTER_BITS, TAPS = 16, 4, 8, 4

Case = namedtuple("Case", "name group size frames")
Result = namedtuple("Result", "out hmid vsum hphase vphase")


def filters(orc, iw, ih, ow, oh):
    """(h_incr, v_incr, hf [16, 4], vf [16, 4]) of img_resample_full_init (:425-472), the filters from the oracle's builder"""
    out = []
    for o, i in ((ow, iw), (oh, ih)):
        f = np.zeros(64, np.int16)
        orc.lib().amvo_build_resample_filter(ctypes.c_void_p(f.ctypes.data), o, i)
        out.append(f.reshape(16, 4).astype(np.int64))
    return (iw << POS_BITS) // ow, (ih << POS_BITS) // oh, out[0], out[1]


def phases(n_out, incr, start):
    pos = start + np.arange(n_out, dtype=np.int64) * incr
    return pos >> POS_BITS, (pos >> (POS_BITS - PHASE_BITS)) & 15


def resample_plane(plane, ow, oh, h_incr, v_incr, hf, vf, mid_clamp=True):
    """one plane [ih, iw] -> Result: out uint8 [oh, ow]; hmid [ih, ow], the horizontal sums >> 8 before their clamp; vsum
    [oh, ow], the vertical sums >> 8 before theirs; the phases of the output columns and rows.  mid_clamp=False leaves
    the clamp between the two stages out (what a kernel that forgot it would compute)."""
    ih, iw = plane.shape
    s0, hph = phases(ow, h_incr, -(1 << POS_BITS))
    sx = np.clip(s0[:, None] + np.arange(TAPS), 0, iw - 1)                      # [ow, 4]
    hmid = (plane.astype(np.int64)[:, sx] * hf[hph][None, :, :]).sum(axis=2) >> FILTER_BITS
    mid = np.clip(hmid, 0, 255) if mid_clamp else hmid
    y1, vph = phases(oh, v_incr, 2 << POS_BITS)
    lines = np.clip(y1[:, None] - 3 + np.arange(TAPS), 0, ih - 1)               # [oh, 4]
    vsum = (mid[lines] * vf[vph][:, :, None]).sum(axis=1) >> FILTER_BITS
    return Result(np.clip(vsum, 0, 255).astype(np.uint8), hmid, vsum, hph, vph)


def plane_sizes(w, h):
    return [(h, w), (h >> 1, w >> 1), (h >> 1, w >> 1)]


def frame_bytes(w, h):
    return w * h + 2 * (w >> 1) * (h >> 1)


def split(frame, w, h):
    out, pos = [], 0
    for r, c in plane_sizes(w, h):
        out.append(frame[pos:pos + r * c].reshape(r, c))
        pos += r * c
    return out


def join(planes):
    return np.concatenate([np.ascontiguousarray(p, np.uint8).reshape(-1) for p in planes])


def resample_frame(orc, frame, iw, ih, ow, oh, mid_clamp=True):
    """a tight frame -> [Result of Y, Cb, Cr]"""
    h_incr, v_incr, hf, vf = filters(orc, iw, ih, ow, oh)
    return [resample_plane(p, c, r, h_incr, v_incr, hf, vf, mid_clamp)
            for p, (r, c) in zip(split(frame, iw, ih), plane_sizes(ow, oh))]


def model_frame(orc, frame, iw, ih, ow, oh, mid_clamp=True):
    return join([r.out for r in resample_frame(orc, frame, iw, ih, ow, oh, mid_clamp)])


# ---- the pictures --------------------------------------------------------------------------------------------------------

def _noise(w, h, n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, frame_bytes(w, h)), dtype=np.uint8)


def _from_planes(w, h, fn):
    """a frame whose three planes are fn(rows, cols) -> uint8 [rows, cols]"""
    return join([fn(r, c) for r, c in plane_sizes(w, h)])


def _stripes(w, h, width, vertical, inverse):
    def fn(r, c):
        k = (np.arange(c)[None, :] if vertical else np.arange(r)[:, None]) // width
        return np.broadcast_to(((k + inverse) & 1) * 255, (r, c)).astype(np.uint8)
    return _from_planes(w, h, fn)


def _checker(w, h, inverse):
    return _from_planes(w, h, lambda r, c: (((np.arange(r)[:, None] + np.arange(c)[None, :] + inverse) & 1) * 255).astype(np.uint8))


def stripe_frames(w, h):
    """stripes of width 1, 2 and 3, vertical and horizontal, and a checkerboard; each with its inverse"""
    out = [_stripes(w, h, k, v, inv) for k in (1, 2, 3) for v in (True, False) for inv in (0, 1)]
    return np.stack(out + [_checker(w, h, 0), _checker(w, h, 1)])


def tap_frames(orc, iw, ih, ow, oh):
    """for every phase p and both directions: the 4-sample pattern that is 255 where the tap of p is positive and 0
    elsewhere, and its inverse, repeated with period 4 and aligned so that the first luma output column (or row) of phase
    p has its four taps on one whole pattern -- the largest and the smallest sum that phase can give"""
    h_incr, v_incr, hf, vf = filters(orc, iw, ih, ow, oh)
    frames = []
    for vertical in (False, True):
        n_out, incr, f, start = (oh, v_incr, vf, 2 << POS_BITS) if vertical else (ow, h_incr, hf, -(1 << POS_BITS))
        first, ph = phases(n_out, incr, start)
        if vertical:
            first = first - 3
        for p in range(16):
            at = np.flatnonzero(ph == p)
            inside = [k for k in at if first[k] >= 0 and first[k] + 3 < (ih if vertical else iw)]
            if not inside:
                continue
            origin = int(first[inside[0]])
            for inverse in (0, 1):
                pat = ((f[p] > 0) ^ bool(inverse)).astype(np.uint8) * 255

                def fn(r, c, pat=pat, origin=origin, vertical=vertical):
                    k = (np.arange(r)[:, None] if vertical else np.arange(c)[None, :]) - origin
                    return np.broadcast_to(pat[k % 4], (r, c)).astype(np.uint8)
                frames.append(_from_planes(iw, ih, fn))
    return np.stack(frames)


EDGE_SOURCES = [(2, 2), (2, 4), (3, 6), (4, 4), (6, 4)]
EDGE_DESTINATIONS = [(2, 2), (2, 4), (4, 6), (64, 64)]
RATIOS = [(2, 2, 16384, 2), (16384, 2, 2, 2), (2, 16384, 2, 2), (2, 2, 2, 16384)]
CLAMP_SIZES = [(16, 16, 32, 32), (32, 32, 34, 34)]
PHASE_SIZES = [(34, 34, 32, 32), (32, 32, 34, 34), (16, 16, 66, 50)]
FLAT_SIZE = (4, 4, 2, 2)


def flat_frames(w=4, h=4):
    """frame v is all v, v = 0..255"""
    return np.repeat(np.arange(256, dtype=np.uint8)[:, None], frame_bytes(w, h), axis=1)


def _edge_frames(w, h, seed):
    """noise, and the extremes that make every clamped tap count: all 0, all 255, left/top half 0 and right/bottom 255"""
    n = frame_bytes(w, h)
    ramp = _from_planes(w, h, lambda r, c: ((np.arange(c)[None, :] * 2 >= c) * 255 | np.zeros((r, 1), np.int64)).astype(np.uint8))
    bars = _from_planes(w, h, lambda r, c: ((np.arange(r)[:, None] * 2 >= r) * 255 | np.zeros((1, c), np.int64)).astype(np.uint8))
    return np.concatenate([_noise(w, h, 4, seed), np.zeros((1, n), np.uint8), np.full((1, n), 255, np.uint8), ramp[None], bars[None]])


_CASES = {}


def cases(orc):
    """the case list (built once a process; the arrays are shared: leave them unchanged)"""
    if "all" in _CASES:
        return _CASES["all"]
    out = []
    for k, (iw, ih, ow, oh) in enumerate(PHASE_SIZES):
        out.append(Case("phases-%dx%d-%dx%d" % (iw, ih, ow, oh), "phases", (iw, ih, ow, oh), _noise(iw, ih, 3, 500 + k)))
    for iw, ih, ow, oh in CLAMP_SIZES:
        out.append(Case("stripes-%dx%d-%dx%d" % (iw, ih, ow, oh), "clamps", (iw, ih, ow, oh), stripe_frames(iw, ih)))
    for iw, ih, ow, oh in (CLAMP_SIZES[1],):                    # every phase both ways; an interpolating filter overshoots most
        out.append(Case("taps-%dx%d-%dx%d" % (iw, ih, ow, oh), "clamps", (iw, ih, ow, oh), tap_frames(orc, iw, ih, ow, oh)))
    for k, (iw, ih) in enumerate(EDGE_SOURCES):
        for ow, oh in EDGE_DESTINATIONS:
            out.append(Case("edges-%dx%d-%dx%d" % (iw, ih, ow, oh), "edges", (iw, ih, ow, oh), _edge_frames(iw, ih, 600 + k)))
    for k, (iw, ih, ow, oh) in enumerate(RATIOS):
        fr = np.concatenate([_noise(iw, ih, 2, 700 + k), stripe_frames(iw, ih)[[2, 3]]])
        out.append(Case("ratios-%dx%d-%dx%d" % (iw, ih, ow, oh), "ratios", (iw, ih, ow, oh), fr))
    out.append(Case("odd-35x33-33x31", "odd", (35, 33, 33, 31), np.concatenate([_noise(35, 33, 2, 800), stripe_frames(35, 33)[[2, 6]]])))
    out.append(Case("flat-4x4-2x2", "flat", FLAT_SIZE, flat_frames()))
    _CASES["all"] = out
    return out


def by_group(orc, group):
    return [c for c in cases(orc) if c.group == group]


def by_name(orc, name):
    return next(c for c in cases(orc) if c.name == name)


def expected(orc, case):
    """the oracle's frames of a case, uint8 [n, frame bytes of the destination]; computed once a process"""
    key = ("want", case.name)
    if key not in _CASES:
        iw, ih, ow, oh = case.size
        _CASES[key] = np.stack([orc.img_resample_yuv420(f, iw, ih, ow, oh) for f in case.frames])
    return _CASES[key]


def phases_reached(orc, case_list, plane):
    """(set of horizontal phases, set of vertical phases) the output samples of plane 0 / 1 of the cases use"""
    hs, vs = set(), set()
    for c in case_list:
        iw, ih, ow, oh = c.size
        h_incr, v_incr, _, _ = filters(orc, iw, ih, ow, oh)
        r, cc = plane_sizes(ow, oh)[plane]
        hs |= set(phases(cc, h_incr, -(1 << POS_BITS))[1].tolist())
        vs |= set(phases(r, v_incr, 2 << POS_BITS)[1].tolist())
    return hs, vs
