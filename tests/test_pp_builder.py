"""The crafted pictures of tests/pp_builder.py meet every branch of the reference's deblock and dering: asserted on the
restatement's own trace (tests/pp_ref.py), per plane kind (luma "y", chroma "c") and per size class.  A condition on the
builder, not a measurement: a branch that is never taken is a branch the GPU tests never compare."""
import numpy as np
import pytest

import pp_builder as B
import pp_ref as P

CLASSES = {"small": B.SIZES[:3], "large": B.SIZES[3:]}
QPS = (1, 12, 40)
SEEDS = range(40, 48)

# per direction (v: vertical deblock, h: horizontal)
DEBLOCK = ("class0", "class1", "class2",                    # flat with a step over 2 QP / flat / textured
           "def_low_energy", "def_high_energy",             # middleEnergy on both sides of 8 QP
           "def_clamped_pos", "def_clamped_neg", "def_moved",   # d clamped by q in both signs, and d that moves pixels
           "first_near", "first_far", "last_near", "last_far")  # first / last on both sides of QP
DERING = ("dering_flat19", "dering_range20",                # the threshold: a range of 19 skips, of 20 filters
          "dering_flat", "dering_ranged", "dering_plus", "dering_minus", "dering_plain",   # clamped at + QP2, at - QP2, unclamped
          "row_end_changed")                                # the call behind the x loop changes a pixel of the next line's column 0


@pytest.fixture(scope="module")
def traces():
    out = {}
    for name, sizes in CLASSES.items():
        tr = {}
        for w, h in sizes:
            for qp in QPS:
                m = P.parse_mode("de:c,fq:%d" % qp, 6)
                for seed in SEEDS:
                    P.postprocess(B.picture(w, h, "crafted", seed, qp), w, h, m, trace=tr)
        out[name] = tr
    return out


@pytest.mark.parametrize("size_class", sorted(CLASSES))
@pytest.mark.parametrize("plane", ["y", "c"])
def test_every_branch_is_taken(traces, size_class, plane):
    tr = traces[size_class]
    missing = [k for k in ["%s_%s_%s" % (plane, d, b) for d in "vh" for b in DEBLOCK] + ["%s_%s" % (plane, b) for b in DERING] if not tr.get(k)]
    assert not missing, missing


def test_pictures_are_seeded_and_tight():
    for w, h in B.SIZES:
        a, b = B.picture(w, h, "crafted", 7, 12), B.picture(w, h, "crafted", 7, 12)
        assert [p.shape for p in a] == [(h, w), (h // 2, w // 2), (h // 2, w // 2)] and all(p.dtype == np.uint8 for p in a)
        assert all((x == y).all() for x, y in zip(a, b))
        assert any((x != y).any() for x, y in zip(a, B.picture(w, h, "crafted", 8, 12)))
    assert B.case_qp("de:c,fq:31") == 31 and B.case_qp("hb,fq") == 15 and B.case_qp("de") == 1


def test_amv1_frames_are_the_oracles(orc, amv1):
    from conftest import GOLDEN
    w, h, frames = B.amv1_frames(orc, GOLDEN)
    assert (w, h) == (amv1["info"]["width"], amv1["info"]["height"]) and len(frames) >= 3
    yuv, st, _ = orc.decode_frame_ffmpeg(amv1["video"][0], w, h)
    assert st == 0 and (np.concatenate([p.reshape(-1) for p in frames[0]]) == yuv).all()
