"""Pins of the coefficient builder (tests/coef_builder.py) and of what its corpus reaches (no GPU).

The GPU tests compare the reconstruction kernels with the builder's pictures; those are trusted because of these:
  (a) the builder's tables and its de-zig-zag are the oracle's (amvo_idct_block of the builder's products is
      amvo_dequant_idct_block; the Q60 products, wrapped, are amvo_ffmpeg_dequant_block);
  (b) its colour conversion is amvo_yuv_to_bgr over y -128 .. 383 and a (u, v) grid that holds every triple of class 4;
  (c) its picture of every case a scan can carry is amvo_decode_frame's (both zig-zag tables) and
      amvo_decode_frame_ffmpeg's of the scan scan_builder writes for it, whose coefficients are the case's;
  (d) the corpus reaches what it was built for -- counted from the oracle's own values, each count printed.
"""
import numpy as np
import pytest

import coef_builder as cb
import scan_builder as sb


@pytest.fixture(scope="module")
def built(orc):
    return cb.corpus(orc)


def test_tables_and_zigzag_are_the_oracles(orc):
    """(a)"""
    L = orc.lib()
    rng = np.random.default_rng(1)
    coef = rng.integers(-300, 301, (600, 64)) * (rng.random((600, 64)) < 0.5)
    coef[:64, :] = np.eye(64, dtype=np.int64) * 1000          # one coefficient at each scan position
    for flags in (0, 1):
        want = cb.idct_blocks(orc, coef, flags)
        nat = np.ascontiguousarray(cb.dequantised(coef, flags).reshape(-1, 64).astype(np.int32))
        for b in range(nat.shape[0]):
            L.amvo_idct_block(nat.ctypes.data + 256 * b)
        nat[np.arange(nat.shape[0]) % 6 < 4] += 128
        assert (nat == want).all(), flags
    for comp in (0, 1):
        q = np.zeros(64, np.uint8)
        L.amvo_q60_table(comp, q.ctypes.data)
        assert (q == cb.Q60[comp]).all()
    coef = rng.integers(-32768, 32768, (600, 64))
    nat = cb.dequantised(coef, table=cb.Q60).reshape(-1, 64)
    nat[:, 0] += 1024
    got = np.empty((600, 64), np.int16)
    c16 = np.ascontiguousarray(coef.astype(np.int16))
    for b in range(600):
        L.amvo_ffmpeg_dequant_block(c16.ctypes.data + 128 * b, cb.COMP_OF[b % 6], got.ctypes.data + 128 * b)
    assert (got == cb.wrap16(nat)).all()


def test_colour_conversion_is_the_oracles(orc, built):
    """(b)"""
    triples = built[1]
    ys = sorted(set(range(-128, 384)))
    uv = sorted(set(range(-256, 256, 41)) | {255} | {t[1] for t in triples} | {t[2] for t in triples})
    assert all(y in ys and u in uv and v in uv for y, u, v in triples)
    y, u, v = (a.reshape(-1) for a in np.meshgrid(ys, uv, uv, indexing="ij"))
    got = cb.yuv_to_bgr(y, u, v)
    want = np.zeros((y.size, 3), np.uint8)
    fn, p = orc.lib().amvo_yuv_to_bgr, want.ctypes.data
    for i, (a, b, c) in enumerate(zip(y.tolist(), u.tolist(), v.tolist())):
        fn(a, b, c, p + 3 * i)
    assert (got == want).all()


def test_builder_pictures_are_the_oracles_frames(orc, built):
    """(c)"""
    valid = [c for c in built[0] if not c.dense_only]
    assert len(valid) >= 25
    for c in valid:
        chunk = c.chunk()
        for flags in (0, 1):
            pic, st, ok, coef = orc.decode_frame(chunk, c.w, c.h, flags, want_coef=True)
            assert st == 0 and ok == c.nmcu and (coef == c.coef).all(), c.name
            assert (pic == cb.picture(orc, c.coef, c.w, c.h, c.nmcu_ok, flags)).all(), (c.name, flags)
        pic, st, ok = orc.decode_frame_ffmpeg(chunk, c.w, c.h)
        assert st == 0 and (pic == cb.picture_ffmpeg(orc, c.coef, c.w, c.h, c.nmcu_ok)).all(), c.name
    # a frame that stops early: the oracle's own frame of a scan cut behind nmcu_ok MCUs leaves the same picture
    for c in [c for c in built[0] if c.name in ("nmcu_ok_13", "nmcu_ok_9", "nmcu_ok_10_176x144")]:
        blocks = sb.blocks_from_coefficients(c.coef[: c.nmcu_ok * 6]) + [(None, ["1" * 16], False)]
        chunk = sb.assemble(blocks).chunk
        pic, st, ok = orc.decode_frame(chunk, c.w, c.h, 0)
        assert st & sb.ST_FORMAT and ok == c.nmcu_ok, c.name
        assert (pic == cb.picture(orc, c.coef, c.w, c.h, c.nmcu_ok, 0)).all(), c.name
        pic, st, ok = orc.decode_frame_ffmpeg(chunk, c.w, c.h)
        assert (pic == cb.picture_ffmpeg(orc, c.coef, c.w, c.h, c.nmcu_ok)).all(), c.name


def _shape(nat):
    rows, cols = (nat[1:, :] != 0).any(), (nat[:, 1:] != 0).any()
    return {(False, False): "dc_only", (False, True): "columns_shortcut", (True, False): "rows_shortcut"}.get(
        (bool(rows), bool(cols)) if (nat[1:, 1:] == 0).all() else None, "general")


def test_corpus_coverage(orc, built):
    """(d)"""
    cases, triples = built
    by_name = {c.name: c for c in cases}
    count = {}
    # domains: D is inside what the header promises; E holds cases on both sides of it... or none inside: say which
    count["cases D / E / E inside the bound"] = (sum(c.domain == cb.D for c in cases), sum(c.domain == cb.E for c in cases),
                                                 sum(c.domain == cb.E and c.in_bound for c in cases))
    assert all(c.in_bound for c in cases if c.domain == cb.D) and count["cases D / E / E inside the bound"][2] >= 2
    count["frames a scan can carry"] = sum(not c.dense_only for c in cases)
    # class 1: every scan position alone with +-1, +-1023 (D) and the ends of int16 (E); the quirk
    alone = {}
    for c in cases:
        if c.name.startswith("placement"):
            for line in c.coef:
                nz = np.nonzero(line)[0]
                if nz.size == 1:
                    alone.setdefault(int(nz[0]), set()).add(int(line[nz[0]]))
    assert all({1, -1, 1023, -1023, 32767, -32767, -32768} <= alone[s] for s in range(64)), alone
    zero = cb.idct_blocks(orc, np.zeros((1, 64)), 0)
    for v in (1023, -32768):
        a31, a37 = (cb.one(31, v)[None], cb.one(37, v)[None])
        assert (cb.idct_blocks(orc, a31, 0) == zero).all() and (cb.idct_blocks(orc, a31, 1) != zero).any()
        assert (cb.idct_blocks(orc, a37, 0) != cb.idct_blocks(orc, a37, 1)).any()
    for name in ("placement_D0", "placement_D1", "placement_D2", "placement_Eo0"):
        c = by_name[name]
        assert (cb.picture(orc, c.coef, c.w, c.h, c.nmcu_ok, 0) != cb.picture(orc, c.coef, c.w, c.h, c.nmcu_ok, 1)).any(), name
    # class 2: rows and columns that take the reference's shortcuts (the inputs of its IDCT: AmvJpeg.c:1087, 1134)
    subsets = {(d, f): set() for d in (cb.D, cb.E) for f in (0, 1)}
    n = {"rows of a first element alone": 0, "blocks of row 0 alone": 0, "blocks of column 0 alone": 0, "all-zero blocks": 0,
         "DC-only blocks": 0, "E first elements at 2^20 and beyond": 0, "E first elements just under 2^20": 0}
    for c in cases:
        if not c.name.startswith(("shortcuts", "placement")):
            continue
        for flags in (0, 1):
            nat = cb.dequantised(c.coef, flags)
            first = (nat[:, :, 1:] == 0).all(2)
            for b in np.nonzero(((nat[:, :, 1:] != 0).sum(2) >= 6).any(1) | first.all(1))[0]:
                subsets[(c.domain, flags)].add(int(sum(1 << r for r in range(8) if first[b, r])))
        n["rows of a first element alone"] += int((first & (nat[:, :, 0] != 0)).sum())
        n["all-zero blocks"] += int((nat == 0).all((1, 2)).sum())
        shapes = [_shape(b) for b in nat]
        n["blocks of row 0 alone"] += shapes.count("columns_shortcut")
        n["blocks of column 0 alone"] += shapes.count("rows_shortcut")
        n["DC-only blocks"] += shapes.count("dc_only")
        if c.domain == cb.E:
            v0 = np.abs(nat[:, 1:, 0][first[:, 1:]])
            n["E first elements at 2^20 and beyond"] += int((v0 >= 1 << 20).sum())
            n["E first elements just under 2^20"] += int(((v0 < 1 << 20) & (v0 >= (1 << 20) - 64)).sum())
    count.update(n)
    assert all(v >= 1 for v in n.values()), n
    count["row subsets (domain, flags)"] = {k: len(v) for k, v in subsets.items()}
    assert len(subsets[(cb.D, 0)]) == 256 and len(subsets[(cb.D, 1)]) == 256, count
    assert len(subsets[(cb.E, 0)] | subsets[(cb.E, 1)]) >= 250, count
    # class 3: outputs on each iclp edge in front of the clamp, by the path that made them
    edges = {}
    c = by_name["iclp_D0"]
    nat = cb.dequantised(c.coef, 0)
    for b in range(6 * 48):
        pre = cb.preclamp(orc, c.coef[b], 0 if b % 6 < 4 else 1)
        for e in cb.ICLP_EDGES:
            edges[(_shape(nat[b]), e)] = edges.get((_shape(nat[b]), e), 0) + int((pre == e).sum())
    count["iclp edges"] = edges
    assert all(edges.get((s, e), 0) >= 1 for s in cb.ICLP_SHAPES for e in cb.ICLP_EDGES), edges
    # class 4: every channel on each side of both clamps, the chroma terms at their ends, MCUs of all-different samples
    chan = {}
    ends = {k: 0 for k in ("r max", "r min", "g max", "g min", "b max", "b min")}
    different = 0
    for name in ("colour_0", "colour_1"):
        c = by_name[name]
        px = cb.idct_blocks(orc, c.coef, 0).reshape(-1, 6, 64)
        y, u, v = px[:, 0, 0], px[:, 4, 0], px[:, 5, 0]
        for ch, t in zip("bgr", cb.colour_terms(y, u, v)):
            for e in (-1, 0, 255, 256):
                chan[(ch, e)] = chan.get((ch, e), 0) + int((t == e).sum())
        for key, t, want in (("r max", 18 * u + 367 * v, 385 * 255), ("r min", 18 * u + 367 * v, 385 * -256),
                             ("g max", -159 * u - 220 * v, 379 * 256), ("g min", -159 * u - 220 * v, -379 * 255),
                             ("b max", 411 * u - 29 * v, 411 * 255 + 29 * 256), ("b min", 411 * u - 29 * v, -411 * 256 - 29 * 255)):
            ends[key] += int((t == want).sum())
        different += sum(len(set(m[4].tolist())) == 64 and len(set(m[5].tolist())) == 64 and
                         len({tuple(m[k].tolist()) for k in range(4)}) == 4 for m in px)
    count["channels on clamp edges"], count["chroma terms at their ends"], count["MCUs of all-different samples"] = chan, ends, different
    assert all(chan.get((ch, e), 0) >= 1 for ch in "bgr" for e in (-1, 0, 255, 256)), chan
    assert all(v >= 1 for v in ends.values()) and different >= 8, (ends, different)
    assert max(abs(385 * 256), abs(379 * 256), 411 * 256 + 29 * 255) >> 8 <= 440        # the bound the packed path relies on
    grid = {(y, u, v) for y in (-128, -1, 0, 255, 256, 383) for u in (-256, -1, 0, 255) for v in (-256, -1, 0, 255)}
    assert grid <= set(triples)
    # class 5: full blocks of +-1023 under the ends of int16, in frames a scan can carry too
    full = {}
    for c in cases:
        if c.name.startswith("large_sums"):
            for line in c.coef[(np.abs(c.coef[:, 1:]) == 1023).all(1)]:
                if int(line[0]) in (32767, -32767, -32768):
                    full[(int(line[0]), not c.dense_only)] = full.get((int(line[0]), not c.dense_only), 0) + 1
    count["full blocks under DC ends (dc, scan-carriable)"] = full
    assert all(full.get((dc, True), 0) >= 1 for dc in (32767, -32768)) and all(full.get((dc, False), 0) >= 5 for dc in (32767, -32767, -32768)), full
    # class 6: what the int16 stores of the FFmpeg mode do
    ff = {"products wrapped to 0": 0, "products wrapped to 32767": 0, "products wrapped to -32768": 0,
          "rows of a first element alone only after the wrap": 0, "flat rows wrapped": 0, "flat rows just inside": 0}
    crop = {k: 0 for k in ("-1", "0", "255", "256", "under -1024", "over 1279")}
    for c in cases:
        nat = cb.dequantised(c.coef, table=cb.Q60)
        nat[:, 0, 0] += 1024
        w = cb.wrap16(nat)
        if c.name.startswith("ffmpeg_wraps"):
            ff["products wrapped to 0"] += int(((w == 0) & (nat != 0)).sum())
            ff["products wrapped to 32767"] += int(((w == 32767) & (nat != 32767)).sum())
            ff["products wrapped to -32768"] += int(((w == -32768) & (nat != -32768)).sum())
            alone = (w[:, :, 1:] == 0).all(2)
            ff["rows of a first element alone only after the wrap"] += int((alone & (nat[:, :, 1:] != 0).any(2)).sum())
            ff["flat rows wrapped"] += int((alone & (np.abs(w[:, :, 0] * 8 + 4) > 32771)).sum())
            ff["flat rows just inside"] += int((alone & (np.abs(w[:, :, 0]) <= 4095) & (np.abs(w[:, :, 0]) >= 4080)).sum())
            out = cb.ffmpeg_blocks(orc, c.coef, put=False).astype(np.int64)
            for k, hit in (("-1", out == -1), ("0", out == 0), ("255", out == 255), ("256", out == 256),
                           ("under -1024", out < -1024), ("over 1279", out > 1279)):
                crop[k] += int(hit.sum())
    count.update(ff)
    count["outputs in front of the crop"] = crop
    assert all(v >= 1 for v in ff.values()) and all(v >= 1 for v in crop.values()), (ff, crop)
    # class 7: where decoding stops, where the picture ends
    assert {c.nmcu_ok for c in cases if (c.w, c.h) == (160, 120)} >= set(range(10, 21)) | {0, 1, 9, 79, 80}
    assert {(c.w, c.h) for c in cases} == set(cb.GEOMETRIES) | {(160, 120)}
    tails = {(c.w - 1) % 16 + 1 for c in cases}
    count["pixels the last MCU of a row keeps"] = sorted(tails)
    assert tails >= {1, 2, 3, 4, 6, 8, 10, 12, 14, 15, 16}
    assert {(c.h + 15) // 16 for c in cases} >= {8, 9} and any(c.h % 16 for c in cases) and any(c.h % 2 for c in cases)
    for w, h in cb.GEOMETRIES:
        oks = {c.nmcu_ok for c in cases if (c.w, c.h) == (w, h)}
        assert sb.mcus(w, h) in oks and 0 in oks and sb.mcus(w, h) - 1 in oks, (w, h, oks)
    print("coverage:", count)
