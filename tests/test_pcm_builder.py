"""The crafted audio corpus (tests/pcm_builder.py) without a GPU: its models are the oracle's encoders and decoder byte
for byte on every chunk of it, and it reaches what it claims -- counted by those models, printed, asserted."""
import numpy as np
import pytest

import pcm_builder as pb


@pytest.fixture(scope="module")
def corp():
    return pb.corpus()


def _encode_batches(c):
    return [c.batch_a] + c.batches_b + [c.batch_d]


def test_plain_model_is_the_oracle(orc, corp):
    """every chunk of parts A, B and D from its start index: bytes and end index; part A also as one stream from index 0"""
    chunks = 0
    for b in _encode_batches(corp):
        want, _, ends = b.want(orc, 0, b.starts)
        for i, c in enumerate(b.chunks):
            assert pb.encode_chunk(c, b.starts[i]) == (want[i], ends[i]), (b.name, i)
            chunks += 1
    idx = 0
    for i, chunk in enumerate(corp.batch_a.want(orc)[0]):
        got, idx = pb.encode_chunk(corp.batch_a.chunks[i], idx)
        assert got == chunk, i
    assert corp.batch_a.want(orc)[1] == corp.batch_a.starts        # (the stream's own starts: what part A was generated for)
    print("plain model == oracle on %d chunks" % chunks)


@pytest.mark.parametrize("trellis", [1, 2, 3, 4, 5])
def test_trellis_model_is_the_oracle_and_part_d_meets_every_event(orc, corp, trellis):
    ev = pb.TrellisEvents()
    for b in (corp.batch_a, corp.batch_d):
        want, _, ends = b.want(orc, trellis, b.starts)
        for i, c in enumerate(b.chunks):
            assert pb.encode_chunk_trellis(c, b.starts[i], trellis, ev) == (want[i], ends[i]), (trellis, b.name, i, len(c))
    print("trellis %d: %s" % (trellis, ev.summary()))
    for name in ev.names():
        assert getattr(ev, name) >= 1, (trellis, name)


def test_decoder_model_is_the_oracle(orc, corp):
    """the oracle-encoded chunks of every part and the decoder-only chunks: every sample (the end index is the model's alone:
    every sample behind a move depends on it)"""
    ev, chunks = pb.Events(), 0
    for b in _encode_batches(corp):
        for chunk in b.want(orc, 0, b.starts)[0]:
            if len(chunk) > 8:
                got, (pred, _) = pb.decode_chunk(chunk, ev)
                want, _ = orc.adpcm_decode_chunk(chunk)
                assert (got == want).all() and pred == want[-1], b.name
                chunks += 1
    assert len(ev.cells) == pb.CELLS                 # the encoded corpus walks the decoder through every cell as well
    for name, chunk in corp.decoder_only:
        got, (pred, _) = pb.decode_chunk(chunk, ev)
        want, _ = orc.adpcm_decode_chunk(chunk)
        assert (got == want).all() and pred == want[-1], name
        chunks += 1
    print("decoder model == oracle on %d chunks; %s" % (chunks, ev.summary()))


def test_part_a_reaches_every_cell(orc, corp):
    """counted by the model on the chunks as they are coded (the stream from index 0 in chunks of CHUNK samples), not by the
    generator"""
    ev, idx = pb.Events(), 0
    for c in corp.batch_a.chunks:
        _, idx = pb.encode_chunk(c, idx, ev)
    print("part A: %d samples in %d chunks; %s" % (corp.a.size, corp.batch_a.n, ev.summary()))
    all_cases = {(i, q, m, e) for i in range(89) for q in range(8) for m in (0, 1) for e in (0, 1)}
    assert corp.a.size % 2 == 0 and corp.a.size < 20000
    assert len(ev.cells) == pb.CELLS == 1424
    assert all_cases - ev.cases == set(pb.NOT_REACHED) and len(pb.NOT_REACHED) <= 8 and not corp.a_missed
    assert ev.plus_65535 >= 1 and ev.minus_65535 >= 1 and ev.big >= 2
    assert len(ev.clamp_hi) >= 20 and len(ev.clamp_lo) >= 20
    assert ev.index_hi == {2, 4, 6, 8} and ev.index_lo >= 1
    # the exact multiples, where the nudge of the float quotient decides: every index with k = 4 (d = +-step) at the least
    assert {(i, 4) for i in range(89)} <= ev.exact
    # every cell of the kernel's 89 x 8 table hands its quotient factor to a sample that shows it wrong in either direction
    table = {(i, q) for i in range(89) for q in range(8)}
    assert ev.exact_after == table and ev.large_after == table


def test_part_b_lengths_and_orders(corp):
    sizes = [s for b in corp.batches_b for s in b.sizes]
    assert set(pb.LENGTHS) <= set(sizes) and all(s % 2 == 0 for s in sizes)
    assert set(range(0, 132, 2)) | {254, 256, 258, 286, 288, 1376, 1378, 1380} == set(pb.LENGTHS)
    # 0..4 tiles with every remainder: the 16-sample loop 0..1 times, the 2-sample loop 0..7 times; a second flush group
    rem = {(s // pb.TILE, (s % pb.TILE) // 16, (s % 16) // 2) for s in sizes}
    assert {(t, a, b) for t in range(4) for a in (0, 1) for b in range(8)} <= rem and (4, 0, 0) in rem and (4, 0, 1) in rem
    assert {s // pb.TILE for s in sizes} >= {7, 8, 9, 43} and (8, 1, 7) in rem
    assert all(b.n >= 128 for b in corp.batches_b) and corp.batches_b[0].n % 64 != 0
    # a wave is 64 consecutive chunks: each order is there, in a wave of a batch
    found = set()
    for b in corp.batches_b:
        for w in range(0, b.n - 63, 64):
            found |= {k for k, v in pb.wave_properties(b.sizes[w:w + 64]).items() if v}
    print("orders of tile counts met in a wave:", sorted(found))
    assert found == {"ascending", "descending", "longest at lane 0", "longest at lane 63", "one long row", "no full tile"}
    # neighbouring chunks differ: no two chunks of a batch share their first 8 samples, silence aside
    for b in corp.batches_b:
        heads = [c[:8].tobytes() for c in b.chunks if len(c) >= 8]
        assert len(set(heads)) == len(heads), b.name


def test_layouts(corp):
    for b in _encode_batches(corp):
        seen_parity, seen_gap = set(), set()
        for lay in pb.layouts(b.sizes):
            assert lay.n == b.n and (lay.lens == [8 + s // 2 for s in b.sizes]).all()
            ends = lay.offs + lay.lens
            gaps = np.append(lay.offs[1:], lay.blob_bytes - 1) - ends
            assert (gaps.astype(np.int64) >= 0).all() and gaps.max() <= 3 and lay.blob_bytes == int(ends[-1] + gaps[-1]) + 1
            pgaps = np.append(lay.pcm_offs[1:], lay.pcm_samples) - (lay.pcm_offs + lay.sizes)
            assert set(pgaps.astype(np.int64).tolist()) <= {0, 1}
            seen_gap |= set(gaps.astype(np.int64).tolist())
            seen_parity |= {(int(o) % 2, int(s) > 0) for o, s in zip(lay.pcm_offs, lay.sizes)}
            pcm = lay.pcm(b.chunks)
            assert pcm.size == lay.pcm_samples and all((pcm[int(o):int(o) + len(c)] == c).all() for o, c in zip(lay.pcm_offs, b.chunks))
            blob = lay.blob([bytes([i & 255]) * int(l) for i, l in enumerate(lay.lens)])
            assert blob[-1] == pb.POISON and int((blob == pb.POISON).sum()) >= int(gaps.sum()) + 1
            for i in (0, b.n // 2, b.n - 1):
                assert lay.chunk_of_byte(int(lay.offs[i])) == (i, 0)
                assert lay.chunk_of_byte(int(ends[i]) - 1) == (i, int(lay.lens[i]) - 1)
                if gaps[i]:
                    assert lay.chunk_of_byte(int(ends[i])) == (i, None)
        assert seen_gap == {0, 1, 2, 3} and {(0, True), (1, True)} <= seen_parity, b.name


def test_decoder_only_chunks(corp):
    names = dict(corp.decoder_only)
    assert all(("byte %#04x from index %d" % (b, i)) in names for i in range(89) for b in range(256))
    assert {c[2] for _, c in corp.decoder_only} >= {89, 255} | set(range(89))
    for byte, (pred, index) in pb.RUN_STARTS.items():
        for n in pb.RUN_LENGTHS:
            chunk = names["%d bytes of %#04x" % (n, byte)]
            assert len(chunk) == 8 + n and set(chunk[8:]) == {byte}
            pcm, (p, i) = pb.decode_chunk(chunk)
            # the run takes the index to its end (up: within 11 nibbles; down: a move per nibble) and the predictor to a rail
            assert i == (88 if byte & 7 else max(88 - 2 * n, 0)), (byte, n)
            assert p == (pb.LO if byte & 8 else pb.HI), (byte, n, p)
            assert int(np.abs(pcm.astype(np.int32)).max()) >= 32767
    assert set(pb.RUN_LENGTHS) == {11, 12, 13, 767, 768, 769, 1536, 1537}
