"""Pins of the picture builder (tests/pixel_builder.py) and of what its corpus reaches (no GPU).

The GPU tests compare the encoder kernels with the oracle's chunks of the builder's frames; what a frame is there for is
checked here, from the oracle's own coefficients and chunk of every case:
  (a) the builder's placement of blocks and its bit model are the oracle's (its lines are what amvo_encode_frame_yuv420's
      chunk decodes to; scan_builder's chunk of those lines is the oracle's chunk);
  (b) every group reaches what its name says -- each count printed.
"""
import numpy as np
import pytest

import pixel_builder as pb
import scan_builder as sb


@pytest.fixture(scope="module")
def built(orc):
    cases, reach = pb.corpus(orc)
    info = {}
    for c in cases:
        lines = c.lines(orc)
        info[c.name] = {"lines": lines, "chunk": c.chunk(orc), "model": pb.frame_model(lines, c.w, c.h)}
    return cases, reach, info


def _group(built, g):
    return [(c, built[2][c.name]) for c in built[0] if c.group == g]


def test_placement_and_bit_model_are_the_oracles(orc, built):
    """(a)"""
    cases, _, info = built
    for c in cases:
        i = info[c.name]
        got, st = orc.entropy_blocks(i["chunk"], len(i["lines"]))
        assert st == 0 and (got == i["lines"]).all(), c.name
        frame = sb.assemble(sb.blocks_from_coefficients(i["lines"]))
        assert frame.chunk == i["chunk"] and frame.raw == pb.scan_of(i["chunk"]) and frame.nbits == i["model"]["nbits"], c.name
        if c.kind != "yuv":                      # ... and an RGB case's planes are its pixels' conversion: the same chunk
            assert orc.encode_frame_yuv(*c.planes, c.w, c.h, qbias=c.qbias) == i["chunk"], c.name
    # the placement model at sizes that end inside an MCU, against the oracle's own coefficients of the pixels
    for c in cases:
        if c.kind != "yuv":
            blocks = pb.blocks_of_planes(*c.planes, c.w, c.h)
            assert (pb.lines_of(orc, blocks, [0, 0, 0, 0, 1, 1] * (len(blocks) // 6), c.qbias) == info[c.name]["lines"]).all(), c.name


def _symbols_of(lines):
    """-> {(table, run, size, sign)}, {(table, run)} of every zero run, {(table, position)} of single-coefficient blocks,
    the masks of group 2's interest, DC differences per predictor"""
    syms, runs, alone, masks, dcs, zrls, top = set(), set(), set(), set(), {0: set(), 1: set(), 2: set()}, set(), 0
    pred = [0, 0, 0]
    for b, line in enumerate(lines.astype(np.int64)):
        t, comp = (0 if b % 6 < 4 else 1), pb.COMP_OF[b % 6]
        d = int(line[0]) - pred[comp]
        pred[comp] = int(line[0])
        dcs[comp].add((abs(d).bit_length(), int(np.sign(d))))
        nz = np.nonzero(line[1:])[0] + 1
        last = 0
        for k in nz.tolist():
            run, v = k - last - 1, int(line[k])
            runs.add((t, run))
            zrls.add(run // 16)
            syms.add((t, run % 16, abs(v).bit_length(), int(np.sign(v))))
            top = max(top, abs(v))
            last = k
        if nz.size == 1:
            alone.add((t, int(nz[0])))
        masks.add((t, tuple(nz.tolist())) if nz.size <= 2 or nz.size >= 62 else None)
    return syms, runs, alone, masks, dcs, zrls, top


def test_symbols_and_runs(orc, built):
    """groups 1 and 2"""
    syms, runs, alone, masks, zrls, top = set(), set(), set(), set(), set(), 0
    dcs = {0: set(), 1: set(), 2: set()}
    values = set()
    for c, i in _group(built, 1) + _group(built, 2):
        s, r, a, m, d, z, t = _symbols_of(i["lines"])
        syms |= s; runs |= r; alone |= a; masks |= m; zrls |= z
        top = max(top, t)
        for k in dcs:
            dcs[k] |= d[k]
        for b, line in enumerate(i["lines"].astype(np.int64)):
            last = 0
            for k in (np.nonzero(line[1:])[0] + 1).tolist():
                values.add((0 if b % 6 < 4 else 1, k - last - 1, int(line[k])))
                last = k
    both = lambda t: {(run, size) for tt, run, size, sg in syms if tt == t and (tt, run, size, -sg) in syms}
    luma, chroma = both(0), both(1)
    print("AC symbols in both signs: luma %d, chroma %d; the largest |AC| %d" % (len(luma), len(chroma), top))
    assert {(r, s) for r in range(16) for s in range(1, 8)} <= luma and len({x for x in luma if x[1] == 8}) >= 5 and len(luma) >= 117
    assert {(r, s) for r in range(16) for s in range(1, 6)} <= chroma and len({x for x in chroma if x[1] in (6, 7)}) >= 13 and len(chroma) >= 93
    assert top < 256 and not any(s[2] >= 9 for s in syms)              # AC sizes 9 and 10: not from 8-bit samples
    # the smallest and the largest magnitude of each size that the builder found are in the frames
    exact = [0, 0]
    for (t, run, size, sg), (lo, hi) in built[1]["symbols"].items():
        assert (t, run, sg * lo) in values and (t, run, sg * hi) in values, (t, run, size, sg)
        exact[t] += (lo, hi) == (1 << (size - 1), (1 << size) - 1)
    print("symbols (table, run, size, sign) whose smallest and largest magnitude are both reached: luma %d of %d, chroma %d of %d"
          % (exact[0], sum(k[0] == 0 for k in built[1]["symbols"]), exact[1], sum(k[0] == 1 for k in built[1]["symbols"])))
    assert exact[0] >= 204 and exact[1] >= 158
    for t in (0, 1):
        assert {run for tt, run in runs if tt == t} >= set(range(63)), t       # every zero run 0 .. 62
        assert {p for tt, p in alone if tt == t} >= set(range(1, 64)), t        # one coefficient at every position
        for want in ((31,), (32,), (31, 32), (63,), (31, 63), (2, 63)):
            assert (t, want) in masks, (t, want)
        assert (t, tuple(range(1, 64))) in masks and (t, tuple(range(1, 63))) in masks     # 63 ACs (no EOB), 62 and an EOB
    assert zrls >= {0, 1, 2, 3}
    want = {(0, 0)} | {(s, sg) for s in range(1, 9) for sg in (1, -1)}
    for comp in (0, 1, 2):
        assert dcs[comp] >= want and max(s for s, _ in dcs[comp]) == 8, (comp, sorted(dcs[comp]))


def test_symbol_split(built):
    """group 3"""
    kinds = set()
    for c, i in _group(built, 3):
        seg = i["model"]["segments"][0]
        kinds |= set().union(*seg["starts"])
        if "symbols" in c.meta:
            assert seg["symbols"] == c.meta["symbols"] and seg["per"] == (2 if c.meta["symbols"] > 64 else 1), c.name
            assert sum(r > 0 for r in seg["runs"]) == (min(64, c.meta["symbols"]) if seg["per"] == 1 else 33), c.name
        if "under" in c.meta:
            under, over = max(r for r in seg["runs"] if r <= pb.OWN_BITS), min(r for r in seg["runs"] if r > pb.OWN_BITS)
            assert (under, over) == (c.meta["under"], c.meta["over"]) and under >= pb.OWN_BITS - 8 and over <= pb.OWN_BITS + 8, c.name
            print("%s: the runs closest to %d bits: %d and %d" % (c.name, pb.OWN_BITS, under, over))
    assert {c.meta["symbols"] for c, _ in _group(built, 3) if "symbols" in c.meta} >= {60, 64, 65}
    assert sum("under" in c.meta for c, _ in _group(built, 3)) >= 1
    assert kinds >= {"second", "last_coefficient", "eob", "behind_31"}, kinds


def test_predictor_paths(built):
    """group 4"""
    assert len(pb.segments(*pb.BIG)) == 10 and [nb // 6 for _, nb in pb.segments(*pb.BIG)][:2] == [6, 5]
    assert [nb // 6 for _, nb in pb.segments(*pb.TALL)] == [7, 7, 7]
    seen = set()
    for c, i in _group(built, 4):
        dc = i["lines"][:, 0].astype(np.int64)
        for s, (first, nb) in enumerate(pb.segments(c.w, c.h)):
            for k in c.meta["blocks"]:
                b = first + k
                if k in (1, 2, 3):
                    continue
                before = b - 3 if k == 0 else b - 6
                step = int(dc[b] - (dc[before] if before >= 0 else 0))
                assert abs(step) >= (128 if first else 100), (c.name, s, k, step)
                seen.add((c.w, k, first > 0, s % pb.WAVES == 0 and s > 0))
    for w in (pb.BIG[0], pb.TALL[0]):
        for k in (0, 4, 5):
            assert (w, k, False, False) in seen and (w, k, True, False) in seen                # the frame's start, a later segment
    assert all((pb.BIG[0], k, True, True) in seen for k in (0, 4, 5))                      # wave 0 from wave 3 of the round before


def test_window_and_hand_back(built):
    """group 5"""
    carried, subs = set(), {}
    for c, i in _group(built, 5):
        m = i["model"]
        if "carried" in c.meta:
            early = [f for f in m["flushes"] if not f[3]]
            assert m["handed_back"] is None and early and early[0][2] == c.meta["carried"], c.name
            carried.add(early[0][2])
        else:
            subs.setdefault(c.meta["sub"], []).append((c.name, m))
    assert carried == set(range(8))
    for name, m in subs["last"]:
        assert m["handed_back"] == len(m["round_bits"]) - 1 > 0 and m["wrote_before"], name
    for name, m in subs["first"]:
        assert m["handed_back"] == 0, name
    for name, m in subs["after"]:
        assert m["handed_back"] is None and m["fits_after_flush"], name
    print("round bits of the hand-back cases:", {name: m["round_bits"] for name, m in subs["last"] + subs["first"]})


def test_ff_bytes_and_tails(built):
    """group 6"""
    have, longest = set(), 0
    for c, i in _group(built, 6):
        raw = pb.scan_of(i["chunk"])
        got = pb.ff_properties(i["model"], raw)
        assert set(c.meta["reaches"]) <= got, c.name
        have |= got
        longest = max(longest, pb.longest_ff_run(raw))
    print("group 6 reaches %s; the longest FF run: %d bytes" % (sorted(have), longest))
    assert have >= set(pb.FF_PROPERTIES), set(pb.FF_PROPERTIES) - have
    assert longest >= 2


def test_transform_range(orc, built):
    """group 7: each pattern gives the largest (smallest) output the oracle makes of any candidate at its position"""
    pats = pb.range_patterns()
    out = pb.fdct(orc, np.stack([s for _, s in pats])).astype(np.int64)
    for n in range(64):
        assert out[2 * n, n] == out[:, n].max() and out[2 * n + 1, n] == out[:, n].min(), n
    print("the largest |output|: DC %d, AC %d" % (np.abs(out[:, 0]).max(), np.abs(out[:, 1:]).max()))
    assert np.abs(out).max() <= 8192
    luma, chroma, whole = set(), set(), 0
    for c, _ in _group(built, 7):
        blocks = pb.blocks_of_planes(*c.planes, c.w, c.h).reshape(-1, 6, 64)
        for m in blocks:
            luma |= {m[k].tobytes() for k in range(4)}
            chroma |= {m[4].tobytes(), m[5].tobytes()}
            whole += len({m[k].tobytes() for k in range(4)}) == 1
    want = {s.tobytes() for _, s in pats}
    assert want <= luma and want <= chroma and whole >= len(pats)


def test_quantiser_edges(orc, built):
    """group 8"""
    cases, reach, info = built
    ties = pb.dc_ties()
    lines = info["quantiser_dc_ties"]["lines"]
    blocks = pb.blocks_of_planes(*[c for c in cases if c.name == "quantiser_dc_ties"][0].planes, 64, 32)
    dct = pb.fdct(orc, blocks)
    at = {0: [b for b in range(len(lines)) if b % 6 < 4], 1: [b for b in range(len(lines)) if b % 6 >= 4]}
    for comp in (0, 1):
        mine = [t for t in ties if t[0] == comp]
        assert len(mine) == 12
        for b, (_, total, want) in zip(at[comp], mine):
            assert int(dct[b, 0]) == total and int(lines[b, 0]) == want, (comp, total, want, int(lines[b, 0]))
    # the AC thresholds: per (qbias, table, position, sign) a block on the last output that gives 0 and one on the first that gives +-1
    met = 0
    for qbias in (0, 128):
        found = set()
        for c in cases:
            if c.name.startswith("quantiser_ac_thresholds_q%d_" % qbias):
                blocks = pb.blocks_of_planes(*c.planes, c.w, c.h)
                comp = np.array([0, 0, 0, 0, 1, 1] * (len(blocks) // 6))
                dct = pb.fdct(orc, blocks)
                q = pb.quantise(orc, dct, comp, qbias)
                assert (q == info[c.name]["lines"]).all()
                for t in (0, 1):
                    for scan in range(1, 64):
                        x, v = dct[comp == t, pb.NATURAL_OF_SCAN[scan]].astype(int), q[comp == t, scan].astype(int)
                        found |= {(t, scan, int(a), int(b)) for a, b in zip(x, v)}
        for t in (0, 1):
            for scan in range(1, 64):
                thr = pb.ac_threshold(orc, t, scan, qbias)
                for sg in (1, -1):
                    met += (t, scan, sg * (thr - 1), 0) in found and (t, scan, sg * thr, sg) in found
    print("AC thresholds met exactly on both sides: %d of %d" % (met, pb.AC_THRESHOLDS))
    assert met == reach["ac_thresholds_met"] == pb.AC_THRESHOLDS_MET


def test_rgb_cases(orc, built):
    """group 9"""
    cases = [c for c, _ in _group(built, 9)]
    assert {(c.w - 1) % 16 + 1 for c in cases} >= {2, 6, 10, 14} and {c.h % 16 for c in cases} >= {2, 14}
    assert {c.kind for c in cases} == {"rgb", "bgr"}
    hits = {}
    for c in cases:
        bgr = c.kind == "bgr"
        p = c.pix.reshape(c.h // 2, 2, c.w // 2, 2, 3).transpose(0, 2, 1, 3, 4)
        y, u, v = pb.rgb_terms(p, bgr)
        for key, n in (("y_under", (y % 1024 == 1023).sum()), ("y_on", (y % 1024 == 0).sum()), ("u_under", (u % 4096 == 4095).sum()),
                       ("u_on", (u % 4096 == 0).sum()), ("v_under", (v % 4096 == 4095).sum()), ("v_on", (v % 4096 == 0).sum())):
            hits[(key, bgr)] = hits.get((key, bgr), 0) + int(n)
        if "patches" in c.name:
            flat = p.reshape(-1, 4, 3)
            assert sum(len({tuple(q) for q in m.tolist()}) == 4 for m in flat) >= 8, c.name
            assert {tuple(q) for q in c.pix.reshape(-1, 3).tolist()} >= {tuple(255 * np.array(e)) for e in np.ndindex(2, 2, 2)}, c.name
        else:
            d = np.abs(np.diff(c.pix.astype(int), axis=0)).max(2), np.abs(np.diff(c.pix.astype(int), axis=1)).max(2)
            assert d[0].min() >= 16 and d[1].min() >= 16, c.name
    print("sums on the edge of a rounding step:", hits)
    assert len(hits) == 12 and all(n >= 4 for n in hits.values()), hits


def test_batches(orc, built):
    cases = built[0]
    bs = pb.batches(orc, cases)
    frames = sum(b["n"] for b in bs)
    print("cases per group: %s; %d frames in %d batches" % ({g: sum(c.group == g for c in cases) for g in range(1, 10)}, frames, len(bs)))
    assert frames < 400 and sum(len(b["cases"]) for b in bs) == len(cases)
    for b in bs:
        assert b["where"] == list(range(1, b["n"], 2)) and all(b["frames"][i] is c for i, c in zip(b["where"], b["cases"]))
        assert all(b["frames"][i].group == 0 for i in range(0, b["n"], 2))
        Y, Cb, Cr = b["planes"]
        assert (Y[:, :, b["w"]:] == pb.POISON).all() and (Cb[:, :, b["w"] // 2:] == pb.POISON).all() and b["ys"] > b["w"]
        if b["kind"] != "yuv":
            assert b["stride"] > b["w"] * 3 and (b["pix"][:, :, b["w"] * 3:] == pb.POISON).all()
