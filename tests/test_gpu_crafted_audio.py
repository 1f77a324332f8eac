"""The ADPCM kernels on the crafted audio of tests/pcm_builder.py: every cell of the plain quantiser's table, every tail of
its staging, every layout, the trellis search's events, the decoder's states no encoder writes.  Expected bytes and
samples are the oracle's, expected states the model's (tests/test_pcm_builder.py holds the model to the oracle); every
check is byte for byte, and a failure names the case, the layout, the chunk, the first differing byte and the
(index, nibble) cells the model was in at that byte's samples."""
import ctypes

import numpy as np
import pytest

import pcm_builder as pb
from test_gpu_parity import _t, _with_env

pytestmark = pytest.mark.gpu

FILL = pb.POISON
NLAYOUTS = len(pb.LAYOUTS)


@pytest.fixture(scope="module")
def corp():
    return pb.corpus()


def _plain_batches(c):
    return [c.batch_a] + c.batches_b


def _check_blob(batch, lay, got, chunks, starts, what, plain=True):
    """every byte of the blob, the spare bytes and the sentinel included"""
    want = lay.blob(chunks)
    assert got.shape == want.shape
    why = pb.explain(batch, lay, got, want, (lambda i: starts[i]) if plain else None)
    assert why is None, "%s: %s" % (what, why)


def _plain_dev(ctx, batch, lay, starts):
    """amvhip_adpcm_encode_batch_dev on the batch in this layout -> the blob with its sentinel"""
    import torch
    d_blob = torch.full((lay.blob_bytes,), FILL, dtype=torch.uint8, device="cuda:0")
    d_si = None if starts is None else _t(np.array(starts, np.int32))
    ctx.adpcm_encode_batch_dev(_t(lay.pcm(batch.chunks)), _t(lay.pcm_offs), _t(lay.sizes), lay.n, d_si, d_blob, _t(lay.offs), None)
    torch.cuda.synchronize()
    return d_blob.cpu().numpy()


@pytest.mark.parametrize("layout", range(NLAYOUTS), ids=[l[0] for l in pb.LAYOUTS])
@pytest.mark.parametrize("which", [0, 1, 2], ids=["A", "B1", "B2"])
def test_plain_encoder_independent_chunks(ctx, orc, corp, which, layout):
    """d_step_in given: parts A (from the stream's own starts: all 1424 cells) and B (every tail, every order of tile
    counts in a wave), device form and host form; the bytes between and behind the chunks stay 0xEE"""
    b = _plain_batches(corp)[which]
    lay = pb.layouts(b.sizes)[layout]
    chunks, starts, _ = b.want(orc, 0, b.starts)
    _check_blob(b, lay, _plain_dev(ctx, b, lay, b.starts), chunks, starts, "device form")
    pcm = lay.pcm(b.chunks)
    blob = np.full(lay.blob_bytes, FILL, np.uint8)
    ctx.adpcm_encode_batch(pcm, pcm.size, lay.pcm_offs, lay.sizes, lay.n, np.array(b.starts, np.int32), blob, blob.size, lay.offs)
    _check_blob(b, lay, blob, chunks, starts, "host form")


@pytest.mark.parametrize("knob", [None, "0", "map", "nosettle"])
def test_plain_encoder_one_stream_every_route(pkg, orc, corp, knob):
    """d_step_in NULL: the same batches as one stream each, by guessed starts and sweeps, without sweeps, by the exhaustive
    map at once and with the chain left unsettled -- every route writes the sequential encoder's bytes"""
    c = pkg.Context(0) if knob is None else _with_env(pkg, "AMVHIP_ADPCM_SWEEPS", knob)
    try:
        for b in _plain_batches(corp):
            chunks, starts, _ = b.want(orc)
            assert len(set(starts)) > 5, b.name
            for lay in pb.layouts(b.sizes):
                _check_blob(b, lay, _plain_dev(c, b, lay, None), chunks, starts, "AMVHIP_ADPCM_SWEEPS=%s" % knob)
    finally:
        c.close()


def test_encode_frame_carries_the_index_through_part_a(ctx, pkg, orc, corp):
    lib = pkg.load_library()
    b = corp.batch_a
    chunks, starts, ends = b.want(orc)
    idx = ctypes.c_int32(0)
    for i, seg in enumerate(b.chunks):
        out = np.full(len(chunks[i]) + 5, FILL, np.uint8)
        assert idx.value == starts[i]
        m = lib.amvhip_adpcm_encode_frame(ctx.h, seg.ctypes.data, len(seg), ctypes.byref(idx), out.ctypes.data, len(chunks[i]))
        assert m == len(chunks[i]) and idx.value == ends[i], (i, m, idx.value, ends[i])
        lay = pb.Layout([len(seg)], (0,), (4,), "frame")
        why = pb.explain(pb.Batch("part A, chunk %d" % i, [seg]), lay, out, lay.blob([chunks[i]]), lambda _: starts[i])
        assert why is None, why


def _trellis_dev(ctx, lib, batch, lay, trellis, starts, first):
    """the independent form (starts given) or the stream form -> (blob, end indices), sentinels checked"""
    import torch
    d_blob = torch.full((lay.blob_bytes,), FILL, dtype=torch.uint8, device="cuda:0")
    d_so = torch.full((lay.n + 1,), -7, dtype=torch.int32, device="cuda:0")
    d_pcm, d_po, d_ns, d_co = _t(lay.pcm(batch.chunks)), _t(lay.pcm_offs), _t(lay.sizes), _t(lay.offs)
    if starts is not None:
        d_si = _t(np.array(starts, np.int32))
        assert lib.amvhip_adpcm_encode_trellis_batch_dev(ctx.h, d_pcm.data_ptr(), d_po.data_ptr(), d_ns.data_ptr(), lay.n, d_si.data_ptr(),
                                                         trellis, d_blob.data_ptr(), d_co.data_ptr(), d_so.data_ptr(), None) == 0
    else:
        ctx.adpcm_encode_trellis_stream_dev(d_pcm, d_po, d_ns, lay.n, first, trellis, d_blob, d_co, d_so, None)
    torch.cuda.synchronize()
    so = d_so.cpu().numpy()
    assert so[-1] == -7
    return d_blob.cpu().numpy(), so[:-1]


@pytest.mark.parametrize("trellis", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("which", ["D", "A"])
def test_trellis_independent_chunks_and_streams(ctx, pkg, orc, corp, which, trellis):
    """parts A and D (ties, duplicates at the rails, full frontiers, renormalisation, squares past int32, the freeze +-2,
    the odd counts of the nsamp & ~1 rule) through both trellis entries: bytes, end indices, sentinels.  Part D's
    independent chunks in every layout.  A launch is as long as its longest chunk's search and a stream takes up to
    sixteen sweeps, so the streams, and part A's 1378-sample chunks in either form, go through one layout per frontier
    size, another for each: the five sizes cover the five layouts"""
    lib = pkg.load_library()
    b = corp.batch_d if which == "D" else corp.batch_a
    names = getattr(b, "names", None)
    for k, lay in enumerate(pb.layouts(b.sizes)):
        first = (0, 88, 33, 7, 61)[k]
        for starts in (b.starts, None) if k == trellis - 1 else (b.starts,) if which == "D" else ():
            chunks, _, ends = b.want(orc, trellis, starts, first if starts is None else 0)
            what = "trellis %d, %s" % (trellis, "independent chunks" if starts else "one stream from index %d" % first)
            blob, so = _trellis_dev(ctx, lib, b, lay, trellis, starts, first)
            _check_blob(b, lay, blob, chunks, None, what, plain=False)
            bad = np.flatnonzero(so != np.array(ends))
            assert bad.size == 0, (what, lay.name, "end index of chunk", int(bad[0]), names[int(bad[0])] if names else "", int(so[bad[0]]),
                                   ends[int(bad[0])])


def _decode_and_check(ctx, name, chunks, want_pcm, want_state, lay, names):
    """chunks through amvhip_adpcm_decode_batch_dev into a patterned buffer: every sample, both words of final_state, the PCM
    outside the chunks and the sentinel untouched"""
    import torch
    pattern = ((np.arange(lay.pcm_samples + 1) * 7 + 3) & 0x7fff).astype(np.int16)
    d_pcm = _t(pattern)
    d_fin = torch.full((lay.n + 1, 2), -7, dtype=torch.int32, device="cuda:0")
    ctx.adpcm_decode_batch_dev(_t(lay.blob(chunks)), lay.blob_bytes, _t(lay.offs), _t(lay.lens), lay.n, d_pcm, _t(lay.pcm_offs), d_fin, None)
    torch.cuda.synchronize()
    got, fin = d_pcm.cpu().numpy(), d_fin.cpu().numpy()
    want = pattern.copy()
    for o, w in zip(lay.pcm_offs, want_pcm):
        want[int(o):int(o) + len(w)] = w
    bad = np.flatnonzero(got != want)
    if bad.size:
        at = int(bad[0])
        i = int(np.searchsorted(lay.pcm_offs, at, "right")) - 1
        k = at - int(lay.pcm_offs[i])
        where = "sample %d of its %d" % (k, lay.sizes[i]) if k < lay.sizes[i] else "a spare sample behind it"
        raise AssertionError("%s, layout %s: %d samples differ, the first at %d = chunk %d (%s), %s: got %d, want %d"
                             % (name, lay.name, bad.size, at, i, names[i], where, int(got[at]), int(want[at])))
    assert (fin[-1] == -7).all()
    bad = np.flatnonzero((fin[:-1] != np.array(want_state, np.int32)).any(axis=1))
    assert bad.size == 0, (name, lay.name, "final_state of chunk", int(bad[0]), names[int(bad[0])], fin[int(bad[0])].tolist(), want_state[int(bad[0])])


@pytest.fixture(scope="module")
def decoder_sets(orc, corp):
    """name -> (chunks, their names, the oracle's samples, the model's end states), computed once"""
    encoded, enc_names = [], []
    for b in [corp.batch_a] + corp.batches_b + [corp.batch_d]:
        for i, chunk in enumerate(b.want(orc, 0, b.starts)[0]):
            if len(chunk) > 8:
                encoded.append(chunk)
                enc_names.append("%s chunk %d" % (b.name, i))
    only, only_names = [], []
    for k, (name, chunk) in enumerate(corp.decoder_only):
        if k % 389 == 0:                                   # between ordinary chunks
            only.append(encoded[(k // 389) % len(encoded)])
            only_names.append("ordinary: " + enc_names[(k // 389) % len(encoded)])
        only.append(chunk)
        only_names.append(name)
    sets = {}
    for key, chunks, names in (("encoded", encoded, enc_names), ("decoder-only", only, only_names)):
        sets[key] = (chunks, names, [orc.adpcm_decode_chunk(c)[0] for c in chunks], [pb.decode_chunk(c)[1] for c in chunks])
    return sets


@pytest.mark.parametrize("layout", range(NLAYOUTS), ids=[l[0] for l in pb.LAYOUTS])
@pytest.mark.parametrize("which", ["encoded", "decoder-only"])
def test_decoder(ctx, decoder_sets, which, layout):
    """the oracle-encoded chunks of parts A, B and D (every cell again, from the decoder's side) and the chunks no encoder
    writes (every byte value from every index, header indices past 88, runs that saturate predictor and index inside a
    lane's 12 bytes, across lanes and across 768-byte tiles)"""
    chunks, names, want_pcm, want_state = decoder_sets[which]
    lay = pb.Layout([2 * (len(c) - 8) for c in chunks], pb.LAYOUTS[layout][1], pb.LAYOUTS[layout][2], pb.LAYOUTS[layout][0])
    assert (lay.lens == [len(c) for c in chunks]).all()
    _decode_and_check(ctx, which, chunks, want_pcm, want_state, lay, names)
