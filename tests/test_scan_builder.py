"""Pins of the scan builder (tests/scan_builder.py) and of the oracle's entropy decoder on crafted scans (no GPU).

The builder writes scans symbol by symbol; what the GPU tests compare the entropy kernels with on those scans is the
oracle, and the oracle is trusted there because of these:
  (a) on the coefficients the oracle's encoder quantised from the suite's usual content, the builder writes the
      encoder's bytes;
  (b) the builder writes what the reference's own entropy coder writes (oracle/_ref/libavcref.so, where it is built) on
      coefficient arrays that reach every symbol, both magnitude extremes of every size and DC differences of +-2047;
  (c) the oracle decodes every corpus frame to the builder's coefficients (valid frames) and to the model decoder's
      coefficients, status and MCU count (every frame);
  (d) the corpus holds what the suite's other streams never do: every symbol of the four tables, DC differences of
      every size, magnitudes up to +-1023, predictors that wrap, ZRL and run-15 edges at indexes 48 / 49, FF at every
      byte offset, a frame with more records than its record space, one just under it and one just over, errors in
      every block of an MCU and in the last 17 bits of a chunk, cuts inside a code, its magnitude and the last EOB.
"""
import numpy as np
import pytest

import scan_builder as sb
from conftest import SEED


@pytest.fixture(scope="module")
def corpus():
    return sb.corpus()


def test_builder_tables_are_the_oracles(orc):
    for t in range(4):
        size, code = orc.huffman_codes(t)
        assert {s: (int(size[s]), int(code[s])) for s in range(256) if size[s]} == sb.CODES[t], t


def _usual_content(orc):
    """(picture, w, h, qbias): what the suite's decode tests encode"""
    rng = np.random.default_rng(31)
    out = [(orc.synth_frame(SEED, t, 160, 120), 160, 120, 0) for t in (0, 17, 69)]
    out += [(orc.synth_frame(SEED, 5, 160, 120), 160, 120, 128), (orc.synth_frame(SEED, 3, 130, 98), 130, 98, 0),
            (orc.synth_frame(SEED, 2, 16, 16), 16, 16, 0), (orc.synth_frame(SEED, 1, 320, 240), 320, 240, 128)]
    h, w = 120, 160
    out.append((rng.integers(0, 256, (h, w, 3), dtype=np.uint8), w, h, 0))                              # noise
    out.append((np.clip(orc.synth_frame(SEED, 9, w, h).astype(np.int32) + rng.integers(-30, 31, (h, w, 3)), 0, 255)
                .astype(np.uint8), w, h, 0))                                                             # synth + noise
    out.append((np.full((h, w, 3), 200, np.uint8), w, h, 0))                                              # flat
    chk = ((np.add.outer(np.arange(h), np.arange(w)) & 1) * 255).astype(np.uint8)
    out.append((np.repeat(chk[:, :, None], 3, 2), w, h, 0))                                               # checker
    return out


def test_builder_writes_the_encoders_bytes(orc):
    """(a)"""
    for pic, w, h, qbias in _usual_content(orc):
        chunk, coef = orc.encode_frame(pic, w, h, qbias=qbias, want_coef=True)
        blocks = sb.blocks_from_coefficients(coef)
        assert sb.assemble(blocks).chunk == chunk, (w, h, qbias)
        # ... and its coefficients back, the DC as the running sum the encoder started from
        assert (sb.expected_coefficients(blocks) == coef).all(), (w, h, qbias)


def _reference_arrays(rng):
    """coefficient arrays (zig-zag, DC not predicted) the reference coder can take: every AC symbol with both extremes
    of its size, long zero runs (ZRL), full blocks, and DC values that move by +-2047 without leaving int16"""
    arrays = []
    for t in range(3):
        nb = 6 * 40
        coef = np.zeros((nb, 64), np.int64)
        dc = [0, 0, 0]
        for b in range(nb):
            c = sb.COMP_OF[b % 6]
            step = int(rng.choice([2047, -2047, 1024, -1024, 1, 0, -1, 300]))
            if not -32767 <= dc[c] + step <= 32767:
                step = -step
            dc[c] += step
            coef[b, 0] = dc[c]
            i = 1
            while i < 64:
                i += int(rng.choice([0, 0, 1, 3, 7, 15, 16, 20, 33]))
                if i >= 64:
                    break
                s = int(rng.integers(1, 11))
                coef[b, i] = int(rng.choice(sb._extremes(s)))
                i += 1
            if t == 2 and b % 7 == 0:
                coef[b, 1:] = rng.choice([1023, -1023, 512, -512], 63)
        arrays.append(coef.astype(np.int16))
    # every symbol of the four tables with both extremes of its size, the DC differences turned round where the sum
    # would leave int16
    for _ in range(2):
        blocks, dc = [], [0, 0, 0]
        for b, (d, items, eob) in enumerate(sb._every_symbol(rng, 80)):
            c = sb.COMP_OF[b % 6]
            d = d if -32767 <= dc[c] + d <= 32767 else -d
            dc[c] += d
            blocks.append((d, items, eob))
        arrays.append(sb.expected_coefficients(blocks))
    return arrays


def test_builder_matches_reference_coder(orc, corpus):
    """(b)"""
    if orc.avcref() is None:
        pytest.skip("oracle/_ref/libavcref.so is built only where the reference tree exists")
    arrays = _reference_arrays(np.random.default_rng(4))
    for case in corpus:       # valid corpus frames whose predictors never wrap: the reference codes them alike
        if case.coef is not None and case.blocks == sb.blocks_from_coefficients(case.coef):
            arrays.append(case.coef)
    assert len(arrays) >= 8
    for coef in arrays:
        blocks = sb.blocks_from_coefficients(coef)
        assert sb.assemble(blocks).chunk[2:] == orc.ref_mjpeg_encode_scan(coef)
    seen = {(t, s) for coef in arrays for _, t, s, *_ in sb.assemble(sb.blocks_from_coefficients(coef)).syms}
    assert all((t, s) in seen for t in range(4) for s in sb.CODES[t])      # every symbol of every table went through it


def test_oracle_decodes_the_crafted_scans(orc, corpus):
    """(c)"""
    for case in corpus:
        nblk = sb.mcus(case.w, case.h) * 6
        _, st, ok, coef = orc.decode_frame(case.chunk, case.w, case.h, want_coef=True)
        assert (st, ok) == (case.status, case.ok), case.name
        assert (coef == case.want_coef).all(), case.name
        if case.coef is not None:
            assert st == 0 and (coef == case.coef).all(), case.name
        blocks, est = orc.entropy_blocks(case.chunk, nblk)
        assert est == case.status and len(blocks) == case.blocks_ok and (blocks == case.want_blocks).all(), case.name
        before = np.full(orc.lib().amvo_yuv420_frame_bytes(case.w, case.h), 0x33, np.uint8)
        _, kst, kblocks = orc.decode_frame_ffmpeg_keep(case.chunk, case.w, case.h, before)
        assert (kst, kblocks) == (case.status, case.blocks_ok), case.name


def _valid(corpus):
    return [c for c in corpus if c.coef is not None]


def test_corpus_coverage(corpus):
    """(d)"""
    by_name = {c.name: c for c in corpus}
    assert len(by_name) == len(corpus)
    valid = _valid(corpus)
    # every symbol of the four tables, in valid frames
    syms = [s for c in valid for s in c.frame.syms]
    for t in range(4):
        assert {s[2] for s in syms if s[1] == t} == set(sb.CODES[t]), t
    # both magnitude extremes of every size, both signs: AC sizes 1..10 under every run, DC sizes 0..11
    values = set()
    for c in valid:
        for b, (d, items, _) in enumerate(c.blocks):
            dct, act = sb.tables_of(b % 6)
            values.add((dct, sb.size_of(d), d))
            values.update((act, (it[0] << 4) | sb.size_of(it[1]), it[1]) for it in items if it != "ZRL")
    for t in range(4):
        for sym in sb.CODES[t]:
            if t < 2 or sym & 15:
                size = sym if t < 2 else sym & 15
                assert all((t, sym, v) in values for v in sb._extremes(size)), (t, hex(sym))
    # codes longer than 9 bits start at every bit offset mod 32; every 16-bit code at two offsets at least
    for t in (2, 3):
        long_at = {s[3] % 32 for s in syms if s[1] == t and sb.CODES[t][s[2]][0] > 9}
        assert long_at == set(range(32)), t
        for sym, (n, _) in sb.CODES[t].items():
            if n == 16:
                assert len({s[3] % 32 for s in syms if s[1] == t and s[2] == sym}) >= 2, (t, hex(sym))
    # the longest symbols back to back: 26-bit AC symbols and 22-bit chroma DC symbols, many in a row
    lengths = [len(s[4]) for s in by_name["longest"].frame.syms]
    assert max(lengths) == 26 and sum(1 for a, b in zip(lengths, lengths[1:]) if a == b == 26) > 1000
    assert any(s[1] == 1 and len(s[4]) == 22 for s in by_name["longest"].frame.syms)
    # every predictor wraps several times in a frame
    for name in ("dc_wrap_up", "dc_wrap_down"):
        c = by_name[name]
        for comp in range(3):
            sums = np.cumsum([d for b, (d, _, _) in enumerate(c.blocks) if sb.COMP_OF[b % 6] == comp])
            assert (np.abs(sums).max() + 32768) // 65536 >= 2, (name, comp)
        assert c.coef[:, 0].min() < -30000 and c.coef[:, 0].max() > 30000
    # record space: a frame over it, one just under it (every kernel's layout), one just over it; no 160x120 frame in
    # between (the GPU tests count the frames handed to the serial kernel)
    assert by_name["dense_all_ac"].over and by_name["dense_all_ac"].records == 30720
    under, over = by_name["dense_just_under"], by_name["dense_just_over"]
    assert under.under and under.records > 0.85 * under.space and (under.symbols + 31) // 32 * 32 == under.space
    assert over.over and over.records - over.space <= 32
    assert all(c.over or c.under for c in corpus if (c.w, c.h) == (160, 120))
    for c in valid:          # what the model decoder walks is what was written
        assert c.walked == sb.records_of(c.blocks), c.name
    # past an early cut the zeros decode as luma blocks full of -1: those frames are over their space too
    assert {c.name for c in corpus if c.over} == {"dense_all_ac", "dense_just_over", "cut_in_16bit_code", "cut_in_magnitude"}
    # ZRL and end-of-block edges: ZRL filling a block at 48, ZRL before EOB, ZRL x3 then a value, run 15 at 48, a value
    # at 63 without EOB; ZRL / run 15 at 49 overrun
    edges = by_name["zrl_eob_edges"]
    seen = set()
    for d, items, eob in edges.blocks:
        i = 1
        for j, it in enumerate(items):
            run = 15 if it == "ZRL" else it[0]
            if it == "ZRL" and i == 48:
                seen.add("zrl fills at 48")
            if it == "ZRL" and j + 1 == len(items) and eob:
                seen.add("zrl then eob")
            if it != "ZRL" and run == 15 and i == 48:
                seen.add("run 15 at 48")
            if j >= 3 and items[j - 3: j] == ["ZRL"] * 3 and it != "ZRL":
                seen.add("zrl x3 then a value")
            i += run + 1
        if i == 64 and items[-1] != "ZRL":
            seen.add("value at 63")
    assert len(seen) == 5, seen
    for name in ("zrl_at_49_block68", "zrl_at_49_block346", "run15_at_49_block68", "run15_at_49_block347"):
        c = by_name[name]
        blk = int(name.rsplit("block", 1)[1])
        assert c.status == sb.ST_OVERRUN and c.blocks_ok == blk and c.ok == blk // 6, name
    # FF at every byte offset mod 16 of the scan, and as its last byte
    raw = by_name["ff_bytes"].frame.raw
    assert {i % 16 for i, b in enumerate(raw) if b == 0xFF} == set(range(16)) and raw[-1] == 0xFF
    # errors at exact places: no code in every block of the first, a middle and the last MCU
    for m in (0, 40, 79):
        for k in range(6):
            c = by_name["noncode_mcu%d_block%d" % (m, k)]
            assert (c.status, c.ok, c.blocks_ok) == (sb.ST_FORMAT, m, 6 * m + k), c.name
    tails = [c for c in corpus if c.name.startswith("noncode_tail")]
    assert {c.status for c in tails} >= {sb.ST_FORMAT, sb.ST_FORMAT | sb.ST_TRUNCATED, sb.ST_TRUNCATED}
    for name in ("cut_in_16bit_code", "cut_in_magnitude", "cut_in_last_eob", "cut_one_byte_early"):
        assert by_name[name].status & sb.ST_TRUNCATED, name
    assert by_name["cut_in_last_eob"].status == sb.ST_TRUNCATED and by_name["cut_in_last_eob"].ok == 80
    assert by_name["cut_after_last_symbol"].status == 0 and by_name["no_eoi_byte_aligned"].status == 0
    # the other geometries
    assert {(c.w, c.h) for c in corpus} == {(160, 120), (16, 16), (130, 98), (336, 32), (320, 240)}
