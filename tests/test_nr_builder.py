"""Pins of the -nr corpus (tests/nr_builder.py), against the model alone (tests/nr_ref.py; no GPU):

  (a) every case reaches the arithmetic its name states -- counted with the model -- and no group is empty;
  (b) every start state is inside the bound of amv_nr_plan.h;
  (c) every named fault of nr_ref.faults_of changes the model's coefficients or the state that comes out for at least one
      case; dead_zone_plus_1 and dead_zone_minus_1 for each (AC position, sign, component) separately, the fault confined
      to that one.  The table of fault -> detecting cases is printed (pytest -s shows it; DESIGN.md holds a copy);
  (d) tests/golden/ref_nr_crafted.json -- the REAL reference's chunks of the zero-state cases -- is what the model's reference
      mode gives, and the counts its maker recorded (a model with signed_offsets, dc_unclamped, no_truncation gives other
      coefficients there) hold again.
"""
import json
import os
import sys

import numpy as np
import pytest

import nr_builder as B
import nr_ref as N
import pixel_builder as pb
from conftest import GOLDEN

sys.path.insert(0, GOLDEN)


@pytest.fixture(scope="module")
def built(orc):
    cases, info = B.corpus(orc)
    return cases, info, {c.name: B.reach(c) for c in cases}


def _run(case, faults=(), mode="product"):
    """-> (zig-zag lines per frame, the state afterwards)"""
    st = case.state.copy()
    return N.encode_stream(case.frames, case.w, case.h, case.nr, state=st, mode=mode, qbias=case.qbias, want_coef=True, faults=faults), st


def _differs(a, b):
    return any((x != y).any() for x, y in zip(a[0], b[0])) or (a[1] != b[1]).any()


def test_every_case_reaches_what_it_is_for(built):
    """(a)"""
    cases, info, reach = built
    assert {c.group for c in cases} == set(B.GROUPS)
    print()
    for g in B.GROUPS:
        print("group %s: %d cases" % (g, sum(c.group == g for c in cases)))
    for c in cases:
        r = reach[c.name]
        for what, least in c.aims.items():
            if what == "thresholds":
                continue
            assert (r[what] <= least) if what in ("d_min", "divisor_min") else (r[what] >= least), (c.name, what, r[what], least)
        if c.meta.get("first_offsets") == 0:
            assert not B.offsets_at(c.state, c.nr).any() and c.state[:64].any(), c.name
        if c.meta.get("halves_first"):
            assert c.state[64] == B.FULL + 1 and (c.state[:64] & 1).all(), c.name
    # the thresholds: the block's output is sign * (offset + T) and one less, the model's levels +-1 and 0
    met = 0
    for c in cases:
        if "triples" not in c.meta:
            continue
        assert len(c.meta["triples"]) >= c.aims["thresholds"] > 0 and len(c.frames) == 1
        coef = N.fdct(N.frame_blocks(*c.frames[0], c.w, c.h, 128))
        lines = _run(c)[0][0]
        assert (B.offsets_at(c.state, c.nr) == c.meta["offsets"]).all(), c.name
        for pos, sign, comp, on, under in c.meta["triples"]:
            want = int(c.meta["offsets"][pos]) + c.meta["theta"][(pos, comp)]
            assert (coef[on, pos], coef[under, pos]) == (sign * want, sign * (want - 1)), (c.name, pos, sign, comp)
            scan = pb.SCAN_OF_NATURAL[pos]
            assert (lines[on][scan], lines[under][scan]) == (sign, 0), (c.name, pos, sign, comp)
            assert (on % 6 >= 4) == bool(comp) and (under % 6 >= 4) == bool(comp)
            met += 1
    print("threshold pairs met: %d" % met)
    # group A: at most 5 % of a variant's (position, sign, component) triples dropped
    assert set(info["pairs"]) == {"nr_max_q0", "nr_max_q128", "small_offsets"}
    for name, made in info["pairs"].items():
        print("group A %s: %d of 252 pairs made" % (name, made))
        assert made >= 252 * (1 - B.DROP_CAP), name
    print("dropped: %s" % (info["dropped"] or "none"))
    # what the issue's table says today's streams never reach
    total = {k: sum(r[k] for r in reach.values()) for k in ("clamped_dc", "live_under_32768", "quotient_65536", "quotient_above", "halvings")}
    print("over the corpus:", total, "D from %d to %d, largest AC %d, largest dividend %d" % (
        min(r["d_min"] for r in reach.values()), max(r["d_max"] for r in reach.values()), max(r["ac_max"] for r in reach.values()),
        max(r["dividend_max"] for r in reach.values())))
    assert min(r["d_min"] for r in reach.values()) == 0 and max(r["d_max"] for r in reach.values()) == B.LARGEST
    assert max(r["ac_max"] for r in reach.values()) >= 8000
    assert max(r["dividend_max"] for r in reach.values()) == B.dividend_most(6) < 1 << 31
    assert min(r["divisor_min"] for r in reach.values()) == 1
    assert all(v > 0 for v in total.values())


def test_every_start_state_is_inside_the_bound(built, pkg):
    """(b); and the builder's restatement of the bound is the library's"""
    lib = pkg.load_library()
    for c in built[0]:
        blocks = B.blocks_of(c.w, c.h)
        assert B.in_bound(c.state, blocks), c.name
        assert 0 < c.nr <= lib.amvhip_encode_nr_max(c.w, c.h) == B.nr_max(blocks), c.name
        assert c.w <= 176 and c.h <= 38 and blocks <= 132 and len(c.frames) <= 5, c.name
        st = c.state.copy()                       # ... and the stream stays inside it
        for f in c.frames:
            N.encode_stream([f], c.w, c.h, c.nr, state=st, want_coef=True)
            assert B.in_bound(st, blocks), c.name
    assert B.NR_MAX == 24607


def test_every_fault_is_detected(built):
    """(c)"""
    cases = built[0]
    base = {c.name: _run(c) for c in cases}
    print()
    print("fault -> detecting cases")
    for fault in N.FAULTS:
        hit = [c.name for c in cases if _differs(base[c.name], _run(c, (fault,)))]
        groups = "".join(g for g in B.GROUPS if any(n.startswith(g + "_") for n in hit))
        print("  %-24s %3d cases, groups %-6s e.g. %s" % (fault, len(hit), groups, ", ".join(hit[:2])))
        assert hit, fault
    # the dead zone one too wide or too narrow, confined to one (position, sign, component)
    for fault in ("dead_zone_plus_1", "dead_zone_minus_1"):
        found, by_coef, by_variant = set(), 0, {}
        for c in cases:
            if c.group != "A" or "triples" not in c.meta:
                continue
            for pos, sign, comp, on, under in c.meta["triples"]:
                got = _run(c, {fault: (pos, sign, comp)})
                if _differs(base[c.name], got):
                    found.add((pos, sign, comp))
                    by_coef += any((x != y).any() for x, y in zip(base[c.name][0], got[0]))
                    by_variant.setdefault(c.meta["variant"], set()).add((pos, sign, comp))
        print("  %-24s confined: %d of %d (position, sign, component) detected; per variant %s" % (
            fault, len(found), 63 * 2 * 2, {k: len(v) for k, v in sorted(by_variant.items())}))
        missing = [(p, s, k) for p in range(1, 64) for s in (1, -1) for k in (0, 1) if (p, s, k) not in found]
        assert not missing, (fault, missing[:8])


def test_fixture_of_the_real_reference(built):
    """(d)"""
    import make_ref_nr_crafted_golden as maker
    golden = json.load(open(os.path.join(GOLDEN, "ref_nr_crafted.json")))
    chosen = maker.cases()
    assert [c.name for c in chosen] == [d["name"] for d in golden["cases"]] and golden["seed"] == B.SEED
    assert {c.group for c in chosen} == {"B", "C", "D"} and golden["pinned"] == list(maker.PINNED)
    assert {"B_zero_frame_then_65534", "B_zero_frame_then_32766", "B_zero_frame_then_2"} <= {c.name for c in chosen}
    for c, d in zip(chosen, golden["cases"]):
        assert (d["size"], d["nr"], d["frames"]) == ([c.w, c.h], c.nr, len(c.frames)), c.name
        chunks = N.encode_stream(c.frames, c.w, c.h, c.nr, mode="reference")
        assert [[len(x), "%016x" % N.fnv1a64(x)] for x in chunks] == d["chunks"] and sum(len(x) for x in chunks) == d["bytes"], c.name
        assert maker.differ(c) == d["differ"], c.name
    for fault in maker.PINNED:
        assert sum(d["differ"][fault][0] for d in golden["cases"]) > 0, fault
