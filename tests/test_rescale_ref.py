"""The crafted rescale cases of rescale_ref.py, without a GPU: the numpy model is the oracle byte for byte on every case,
the cases reach what they were built for, and -- where oracle/_ref is built -- the oracle is the reference's own
img_resample wherever the reference defines the result.

Figures of this module's own run (asserted below as PHASES_REACHED, CLAMP_CASES and CLAMP_PICTURES_BITTEN):
  * phases: each of 34x34 -> 32x32, 32x32 -> 34x34 and 16x16 -> 66x50 alone reaches all 16 horizontal and all 16 vertical
    phases in its luma plane, and all 16 and 16 in its chroma planes too (17 / 16 / 33 x 25 samples step through every
    phase as well), so 16 x 16 is required of every plane of every phases case.  The flagship 352x288 -> 160x120 reaches
    6 and 6.
  * clamps: 3 cases (stripes at 16x16 -> 32x32 and 32x32 -> 34x34, the per-phase tap patterns at 32x32 -> 34x34).  In all
    3 the sum between the stages leaves 0..255 at both ends, so does the final sum, and a model without the intermediate
    clamp differs from the oracle: in 2 of 14, 4 of 14 and 31 of 64 pictures (12, 416 and 2920 bytes).  Pictures that
    vary only vertically cannot bite there (a flat row keeps its value through the horizontal stage); they are what
    drives the final sum out of range.
  * flat: 4x4 -> 2x2 keeps every flat value 0..255 (the phase is always 0, the filter's one tap 256)."""
import numpy as np
import pytest

import rescale_ref as RR
from test_oracle_pin import _need_avcref

PHASES_REACHED = {"luma": (16, 16), "chroma": (16, 16)}
CLAMP_CASES = 3
CLAMP_PICTURES_BITTEN = {"stripes-16x16-32x32": (2, 14), "stripes-32x32-34x34": (4, 14), "taps-32x32-34x34": (31, 64)}


def test_the_case_list_is_what_was_asked_for(orc):
    cs = RR.cases(orc)
    assert len({c.name for c in cs}) == len(cs)
    for c in cs:
        iw, ih, ow, oh = c.size
        assert c.frames.dtype == np.uint8 and c.frames.shape[1] == RR.frame_bytes(iw, ih) and len(c.frames) >= 1
    sizes = lambda g: [c.size for c in RR.by_group(orc, g)]
    assert sizes("phases") == [(34, 34, 32, 32), (32, 32, 34, 34), (16, 16, 66, 50)]
    assert set(sizes("clamps")) == {(16, 16, 32, 32), (32, 32, 34, 34)}
    assert set(sizes("edges")) == {s + d for s in [(2, 2), (2, 4), (3, 6), (4, 4), (6, 4)] for d in [(2, 2), (2, 4), (4, 6), (64, 64)]}
    assert sizes("ratios") == [(2, 2, 16384, 2), (16384, 2, 2, 2), (2, 16384, 2, 2), (2, 2, 2, 16384)]
    assert sizes("odd") == [(35, 33, 33, 31)] and sizes("flat") == [(4, 4, 2, 2)]
    flat = RR.by_name(orc, "flat-4x4-2x2").frames
    assert flat.shape == (256, 24) and all((flat[v] == v).all() for v in range(256))
    assert sum(len(c.frames) for c in cs) < 600                                        # a few hundred small frames


def test_the_model_is_the_oracle_on_every_case(orc):
    for c in RR.cases(orc):
        want = RR.expected(orc, c)
        ny = c.size[2] * c.size[3]
        for k, f in enumerate(c.frames):
            got = RR.model_frame(orc, f, *c.size)
            assert (got[:ny] == want[k][:ny]).all(), "%s: luma of picture %d" % (c.name, k)
            assert (got[ny:] == want[k][ny:]).all(), "%s: chroma of picture %d" % (c.name, k)


def test_every_phase_is_reached_in_every_plane(orc):
    full = set(range(16))
    ph = RR.by_group(orc, "phases")
    for plane, key in ((0, "luma"), (1, "chroma")):
        for c in ph:
            hs, vs = RR.phases_reached(orc, [c], plane)
            assert hs == full and vs == full, (c.name, key)
            assert (len(hs), len(vs)) == PHASES_REACHED[key]
        hs, vs = RR.phases_reached(orc, ph, plane)
        assert hs == full and vs == full
    # every output sample is a (column phase, row phase) pair of a full grid: 16 x 16 pairs, and the model used them
    for c in ph:
        for r in RR.resample_frame(orc, c.frames[0], *c.size):
            assert len({(a, b) for a in r.hphase.tolist() for b in r.vphase.tolist()}) == 256
    # what the reference-pinned chains reach at their one size
    hs, vs = RR.phases_reached(orc, [RR.Case("flagship", "", (352, 288, 160, 120), None)], 0)
    assert (len(hs), len(vs)) == (6, 6)


def test_the_clamp_cases_hit_both_clamps_at_both_ends(orc):
    cs = RR.by_group(orc, "clamps")
    assert len(cs) == CLAMP_CASES
    bitten = {}
    for c in cs:
        want = RR.expected(orc, c)
        mid_lo = mid_hi = out_lo = out_hi = False
        pictures = 0
        for k, f in enumerate(c.frames):
            for r in RR.resample_frame(orc, f, *c.size):
                mid_lo |= bool((r.hmid < 0).any())
                mid_hi |= bool((r.hmid > 255).any())
                out_lo |= bool((r.vsum < 0).any())
                out_hi |= bool((r.vsum > 255).any())
            pictures += bool((RR.model_frame(orc, f, *c.size, mid_clamp=False) != want[k]).any())
        assert mid_lo and mid_hi, "%s: the sum between the stages stays inside 0..255" % c.name
        assert out_lo and out_hi, "%s: the final sum stays inside 0..255" % c.name
        assert pictures >= 1, "%s: a rescaler without the intermediate clamp gives the same bytes" % c.name
        bitten[c.name] = (pictures, len(c.frames))
    assert bitten == CLAMP_PICTURES_BITTEN
    # stripes of width 2 or 3 put a large share of the output on 0 or on 255
    c = RR.by_name(orc, "stripes-16x16-32x32")
    for k in (4, 5, 8, 9):                                                             # vertical stripes of width 2 and 3
        luma = RR.expected(orc, c)[k][:32 * 32]
        assert ((luma == 0) | (luma == 255)).mean() > 0.25


def test_the_tap_patterns_meet_their_phase(orc):
    """in the picture built for phase p, some output column (or row) of phase p has its taps on exactly the pattern: its sum
    is the largest (smallest) that phase can give"""
    c = RR.by_name(orc, "taps-32x32-34x34")
    h_incr, v_incr, hf, vf = RR.filters(orc, *c.size)
    assert len(c.frames) == 64
    k = 0
    for vertical, f in ((False, hf), (True, vf)):
        for p in range(16):
            for inverse in (0, 1):
                r = RR.resample_frame(orc, c.frames[k], *c.size, mid_clamp=False)[0]
                sums, ph = (r.vsum[:, 0], r.vphase) if vertical else (r.hmid[0], r.hphase)
                taps = f[p][f[p] > 0] if not inverse else f[p][f[p] <= 0]
                assert (int(taps.sum()) * 255) >> 8 in sums[ph == p].tolist(), (vertical, p, inverse)
                k += 1


def test_flat_pictures_at_phase_zero_stay_flat(orc):
    c = RR.by_name(orc, "flat-4x4-2x2")
    want = RR.expected(orc, c)
    assert want.shape == (256, 6)
    for v in range(256):
        assert (want[v] == v).all(), v
    # ... and at a fractional ratio they do not: flat pictures are no way through the range step in general
    f = np.full(RR.frame_bytes(352, 288), 3, np.uint8)
    assert (orc.img_resample_yuv420(f, 352, 288, 160, 120) != 3).any()


def _ref(R, frame, iw, ih, ow, oh):
    out = np.zeros(RR.frame_bytes(ow, oh), np.uint8)
    frame = np.ascontiguousarray(frame)
    assert R.amvref_img_resample(frame.ctypes.data, iw, ih, out.ctypes.data, ow, oh) == 0
    return out


def test_the_oracle_is_the_reference_where_the_source_is_four_wide(orc):
    """every case whose source is at least 4 wide, and noise at source widths 4..16, heights 2..64 towards 2x2, 6x6, 16x4,
    4x16 and 34x34.  Sources 2 and 3 wide (a chroma plane of one column) are left out: the reference's h_resample
    (imgresample.c:339-341) steps its destination back by a negative count there, which is undefined; the oracle and the
    library repeat the edge sample, and test_gpu_crafted_rescale.py pins that on the edges cases."""
    R = _need_avcref(orc)
    checked = 0
    for c in RR.cases(orc):
        if c.size[0] < 4:
            continue
        want = RR.expected(orc, c)
        for k, f in enumerate(c.frames):
            assert (_ref(R, f, *c.size) == want[k]).all(), "%s: picture %d" % (c.name, k)
        checked += 1
    assert checked == len([c for c in RR.cases(orc) if c.size[0] >= 4]) >= 16
    rng = np.random.default_rng(44)
    for iw in range(4, 17):
        for ih in range(2, 65):
            f = rng.integers(0, 256, RR.frame_bytes(iw, ih), dtype=np.uint8)
            for ow, oh in ((2, 2), (6, 6), (16, 4), (4, 16), (34, 34)):
                assert (_ref(R, f, iw, ih, ow, oh) == orc.img_resample_yuv420(f, iw, ih, ow, oh)).all(), (iw, ih, ow, oh)
