"""`-trellis N` for a whole stream (amvhip_adpcm_encode_trellis_stream_dev): the step index chained on the device.  The
expected bytes are always the oracle's sequential loop over adpcm_encode_chunk_trellis with the index carried."""
import ctypes
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, SEED

pytestmark = pytest.mark.gpu

SIZES = [1378, 1380, 1376, 128, 130, 126, 256, 2, 0, 4, 640, 2048]
KNOB = "AMVHIP_ADPCM_TRELLIS_SWEEPS"


class Stream:
    """chunks of one PCM array, laid out in a blob with `gap` spare bytes between and behind them"""

    def __init__(self, pcm, sizes, gap=0):
        self.pcm = np.ascontiguousarray(pcm, np.int16)
        self.sizes = np.array(sizes, np.uint32)
        self.n = len(sizes)
        self.pcm_offs = np.cumsum([0] + list(sizes))[:-1].astype(np.uint64)
        self.lens = [8 + int(s) // 2 for s in sizes]
        self.offs = np.cumsum([0] + [l + gap for l in self.lens])[:-1].astype(np.uint64)
        self.blob_bytes = int(sum(self.lens)) + gap * self.n
        self._want = {}

    def want(self, orc, trellis, first=0):
        """(chunks, starts, ends) of the sequential encoder (trellis 0: the plain one); computed once per (trellis, first)"""
        key = (trellis, first)
        if key not in self._want:
            chunks, starts, ends, idx = [], [], [], min(max(first, 0), 88)
            for i in range(self.n):
                starts.append(idx)
                o, m = int(self.pcm_offs[i]), int(self.sizes[i])
                if m:
                    seg = self.pcm[o:o + m]
                    chunk, idx = orc.adpcm_encode_chunk_trellis(seg, idx, trellis) if trellis else orc.adpcm_encode_chunk(seg, idx)
                else:
                    chunk = bytes([0, 0, idx, 0, 0, 0, 0, 0])
                chunks.append(chunk)
                ends.append(idx)
            self._want[key] = (chunks, starts, ends)
        return self._want[key]

    def want_blob(self, orc, trellis, first=0, fill=0xEE):
        blob = np.full(self.blob_bytes, fill, np.uint8)
        for o, c in zip(self.offs, self.want(orc, trellis, first)[0]):
            blob[int(o):int(o) + len(c)] = np.frombuffer(c, np.uint8)
        return blob


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).to("cuda:0")


def run_dev(ctx, s, trellis, first=0, want_steps=True, fill=0xEE):
    """the device form on stream s -> (blob, step_out or None)"""
    import torch
    d_pcm, d_po, d_ns, d_co = _dev(s.pcm), _dev(s.pcm_offs), _dev(s.sizes), _dev(s.offs)
    d_blob = torch.full((s.blob_bytes + 1,), fill, dtype=torch.uint8, device="cuda:0")
    d_so = torch.full((s.n + 1,), -7, dtype=torch.int32, device="cuda:0") if want_steps else None
    ctx.adpcm_encode_trellis_stream_dev(d_pcm, d_po, d_ns, s.n, first, trellis, d_blob, d_co, d_so, None)
    torch.cuda.synchronize()
    blob = d_blob.cpu().numpy()
    assert blob[-1] == fill
    if not want_steps:
        return blob[:-1], None
    so = d_so.cpu().numpy()
    assert so[-1] == -7
    return blob[:-1], so[:-1]


def check(ctx, orc, s, trellis, first=0):
    blob, so = run_dev(ctx, s, trellis, first)
    want = s.want_blob(orc, trellis, first)
    bad = np.flatnonzero(blob != want)
    assert bad.size == 0, (trellis, "first differing byte", int(bad[0]), "chunk", int(np.searchsorted(s.offs, bad[0], "right")) - 1)
    assert so.tolist() == s.want(orc, trellis, first)[2], trellis


def _with_env(pkg, value):
    """a context created while the knob holds `value` (it is read at creation)"""
    old = os.environ.get(KNOB)
    os.environ[KNOB] = value
    try:
        return pkg.Context(0)
    finally:
        if old is None:
            os.environ.pop(KNOB, None)
        else:
            os.environ[KNOB] = old


def _content(orc, rng, total):
    """clipping noise, silence and quiet noise in synthetic audio, as test_adpcm_trellis_matches_oracle builds"""
    pcm = orc.synth_audio(SEED, 4242, total + 2)

    def put(lo, values):
        hi = min(lo + len(values), pcm.size)
        if lo < hi:
            pcm[lo:hi] = values[:hi - lo]
    put(1400, rng.integers(-32768, 32768, 1300))
    put(3000, np.zeros(600, np.int16))
    put(5000, rng.integers(-3000, 3000, 2000))
    k = total // 2
    put(k, rng.integers(-32768, 32768, 3000))
    put(k + 4000, np.zeros(5000, np.int16))
    put(k + 9000, rng.integers(-300, 300, 3000))
    return pcm


def _ragged(orc, seed, n, gap, among=SIZES):
    rng = np.random.default_rng(seed)
    sizes = [among[int(k)] for k in rng.integers(0, len(among), n)]
    return Stream(_content(orc, rng, int(sum(sizes))), sizes, gap)


@pytest.fixture(scope="module")
def ragged(orc):
    """about 200 ragged chunks: more than two workgroups of the passes, a first list longer than a wave"""
    return _ragged(orc, 2024, 200, 5)


def _walk(n):
    """two-sample chunks {a, a} (index - 2) and {a, a + 20000} (index - 1 + 8), steered by the plain quantiser's arithmetic to
    stay where nothing clamps: every chunk's end depends on its start, so each sweep settles exactly one more chunk"""
    rng = np.random.default_rng(99)
    pcm = np.zeros(2 * n, np.int16)
    idx = 0
    for i in range(n):
        up = idx < 20 or (idx < 60 and rng.integers(0, 4) == 0)
        pcm[2 * i] = -10000
        pcm[2 * i + 1] = 10000 if up else -10000
        idx += 7 if up else -2
    return Stream(pcm, [2] * n)


@pytest.fixture(scope="module")
def walks():
    return {300: _walk(300), 70: _walk(70)}


def test_reference_produced_stream(ctx, orc):
    """the 15 chunks the reference's adpcm_ima_amv encoder coded with -trellis 3 (tests/golden/reference_outputs.json)"""
    ref = json.load(open(os.path.join(GOLDEN, "reference_outputs.json")))
    a, basis = ref["adpcm_ima_amv_encode"], int(ref["fnv_basis"], 16)
    fs, k = a["frame_size"], a["chunks"]
    s = Stream(orc.synth_audio(ref["seed"], 0, k * fs), [fs] * k)
    blob, so = run_dev(ctx, s, a["trellis3"]["trellis"])
    hh = basis
    for i in range(k):
        hh = orc.fnv1a64(hh, blob[int(s.offs[i]):int(s.offs[i]) + s.lens[i]])
    assert ("%016x" % hh, int(so[-1])) == (a["trellis3"]["fnv"], a["trellis3"]["end_index"])


@pytest.mark.parametrize("trellis", [1, 2, 3, 4, 5])
def test_every_frontier_ragged_chunks(ctx, orc, ragged, trellis):
    """every frontier size on ragged chunks (the freeze boundary +-1, tiny and empty ones) of loud, silent, clipping content:
    every byte, every end index, the bytes between and behind the chunks untouched, and a chain that settled in its sweeps"""
    assert ragged.n > 128 and set(ragged.sizes.tolist()) == set(SIZES)
    check(ctx, orc, ragged, trellis)
    st = ctx.adpcm_trellis_chain_stats()
    rec = st["recoded"]
    print("trellis %d: recoded per sweep %s" % (trellis, rec))
    assert not st["exhaustive"], st
    assert (rec[0] if rec else 0) < ragged.n and all(a >= b for a, b in zip(rec, rec[1:])), st


@pytest.mark.parametrize("trellis", [1, 3, 5])
def test_chain_that_does_not_settle(ctx, orc, walks, trellis):
    for n in (300, 70):
        s = walks[n]
        starts = s.want(orc, trellis)[1]
        assert len(set(starts)) > 20 and 15 <= min(starts[8:]) and max(starts[8:]) <= 70, (n, min(starts[8:]), max(starts), len(set(starts)))
        check(ctx, orc, s, trellis)
        if n == 300:
            assert ctx.adpcm_trellis_chain_stats()["exhaustive"]


@pytest.mark.parametrize("knob", ["0", "map"])
def test_every_route_by_the_knob(pkg, orc, ragged, walks, knob):
    """no sweeps at all, and the fall-back at once: the same bytes; the statistics say where the fall-back wrote them"""
    c = _with_env(pkg, knob)
    try:
        for s in (ragged, walks[300], walks[70]):
            check(c, orc, s, 3)
            st = c.adpcm_trellis_chain_stats()
            assert st["recoded"] == [], st
            if knob == "map" or s is not ragged:
                # forced -- or the walk without sweeps: a guess over two samples from index 0 ends below 15, no true start does
                assert st["exhaustive"], (knob, s.n, st)
    finally:
        c.close()


def test_windows(ctx, pkg, orc):
    """a track coded in windows, each from the end index of the one before, is the track coded in one call; and a one-chunk
    stream from a given index is the independent form from that index"""
    import torch
    lib = pkg.load_library()
    s = _ragged(orc, 7, 40, 0)
    whole, so = run_dev(ctx, s, 3)
    assert (whole == s.want_blob(orc, 3)).all()
    idx, parts, at = 0, [], 0
    for k in (13, 1, 26):
        sizes = s.sizes[at:at + k].tolist()
        lo = int(s.pcm_offs[at])
        w = Stream(s.pcm[lo:lo + int(sum(sizes))], sizes)
        blob, wso = run_dev(ctx, w, 3, idx)
        parts.append(blob)
        idx = int(wso[-1])
        at += k
    assert np.concatenate(parts).tobytes() == whole.tobytes() and idx == int(so[-1])
    one = Stream(orc.synth_audio(SEED, 99, 1378), [1378])
    for first in (0, 57, 88):
        blob, eso = run_dev(ctx, one, 3, first)
        d_blob = torch.zeros(one.blob_bytes, dtype=torch.uint8, device="cuda:0")
        d_so = torch.zeros(1, dtype=torch.int32, device="cuda:0")
        assert lib.amvhip_adpcm_encode_trellis_batch_dev(ctx.h, _dev(one.pcm).data_ptr(), _dev(one.pcm_offs).data_ptr(),
                                                         _dev(one.sizes).data_ptr(), 1, _dev(np.array([first], np.int32)).data_ptr(), 3,
                                                         d_blob.data_ptr(), _dev(one.offs).data_ptr(), d_so.data_ptr(), None) == 0
        torch.cuda.synchronize()
        assert blob.tobytes() == d_blob.cpu().numpy().tobytes() and int(eso[0]) == int(d_so[0]) and blob[2] == first


def test_edges(pkg, orc):
    import torch
    lib = pkg.load_library()
    c = pkg.Context(0)
    try:
        out = (ctypes.c_uint32 * 64)()
        assert lib.amvhip_adpcm_trellis_chain_stats(c.h, out) == pkg.ERR_ARG              # no stream call yet
        s = _ragged(orc, 11, 9, 3)
        d = [_dev(s.pcm), _dev(s.pcm_offs), _dev(s.sizes), None, _dev(s.offs)]
        d_blob = torch.full((s.blob_bytes,), 0xEE, dtype=torch.uint8, device="cuda:0")
        d_so = torch.full((s.n,), -7, dtype=torch.int32, device="cuda:0")
        d[3] = d_blob

        def call(args, n, trellis, so=d_so):
            p = [a.data_ptr() if a is not None else None for a in args]
            return lib.amvhip_adpcm_encode_trellis_stream_dev(c.h, p[0], p[1], p[2], n, 0, trellis, p[3], p[4], so.data_ptr() if so is not None else None,
                                                              None)
        # refusals, and n = 0: nothing is written
        assert call(d, s.n, 0) == pkg.ERR_ARG and call(d, s.n, 6) == pkg.ERR_ARG
        for k in range(5):
            assert call([None if j == k else a for j, a in enumerate(d)], s.n, 3) == pkg.ERR_ARG, k
        assert call(d, 0, 3) == pkg.OK and call([None] * 5, 0, 3, None) == pkg.OK
        torch.cuda.synchronize()
        assert bool((d_blob == 0xEE).all()) and bool((d_so == -7).all())
        assert lib.amvhip_adpcm_trellis_chain_stats(c.h, out) == pkg.ERR_ARG
        # the plain chain's statistics are the plain chain's
        plain = Stream(orc.synth_audio(SEED, 5, 1378 * 40), [1378] * 40)
        pb = np.zeros(plain.blob_bytes, np.uint8)
        c.adpcm_encode_batch(plain.pcm, plain.pcm.size, plain.pcm_offs, plain.sizes, plain.n, None, pb, pb.size, plain.offs)
        before = c.adpcm_chain_stats()
        # n = 1; a stream of zero-sample chunks only (the index passes through); no d_step_out; the host-buffer form
        check(c, orc, Stream(s.pcm[:1378], [1378]), 3)
        zeros = Stream(np.zeros(2, np.int16), [0] * 5)
        blob, so = run_dev(c, zeros, 3, 57)
        assert blob.tobytes() == bytes([0, 0, 57, 0, 0, 0, 0, 0]) * 5 and so.tolist() == [57] * 5
        blob, none = run_dev(c, s, 3, want_steps=False)
        assert none is None and (blob == s.want_blob(orc, 3)).all()
        for first in (0, 200, -3):
            h_blob = np.full(s.blob_bytes, 0xEE, np.uint8)
            h_so = np.full(s.n, -7, np.int32)
            c.adpcm_encode_trellis_stream(s.pcm, s.pcm.size, s.pcm_offs, s.sizes, s.n, first, 3, h_blob, h_blob.size, s.offs, h_so)
            assert (h_blob == s.want_blob(orc, 3, first)).all() and h_so.tolist() == s.want(orc, 3, first)[2]
            assert (h_blob == run_dev(c, s, 3, first)[0]).all()
        assert lib.amvhip_adpcm_encode_trellis_stream(c.h, s.pcm.ctypes.data, s.pcm.size, s.pcm_offs.ctypes.data, s.sizes.ctypes.data, s.n, 0, 3,
                                                      h_blob.ctypes.data, int(s.offs[-1]) + s.lens[-1] - 1, s.offs.ctypes.data, None) == pkg.ERR_SPACE
        assert c.adpcm_chain_stats() == before
    finally:
        c.close()


@pytest.mark.parametrize("trellis", [2, 4])
def test_several_streams_on_one_context(pkg, orc, trellis):
    """streams of different sizes one after the other on one context: the workspaces are reused, grown and reused again
    (what is checked here is the reuse, so the chunks are the shorter ones: a launch is as long as its longest chunk)"""
    c = pkg.Context(0)
    try:
        for seed, n in ((21, 50), (22, 400), (23, 130), (24, 257)):
            check(c, orc, _ragged(orc, seed, n, 1, [s for s in SIZES if s <= 640]), trellis)
    finally:
        c.close()


def run_plain_dev(ctx, s, fill=0xEE):
    """the plain encoder's chained device form (no start indices: the step index runs through the stream) -> blob"""
    import torch
    d_pcm, d_po, d_ns, d_co = _dev(s.pcm), _dev(s.pcm_offs), _dev(s.sizes), _dev(s.offs)
    d_blob = torch.full((s.blob_bytes + 1,), fill, dtype=torch.uint8, device="cuda:0")
    ctx.adpcm_encode_batch_dev(d_pcm, d_po, d_ns, s.n, None, d_blob, d_co, None)
    torch.cuda.synchronize()
    blob = d_blob.cpu().numpy()
    assert blob[-1] == fill
    return blob[:-1]


def test_both_encoders_alternate_on_one_context(pkg, orc, walks):
    """The plain chain and the trellis stream share one workspace plan and one set of device pieces: the two in turn on ONE
    context, n shrinking between calls.  300 chunks: more than one 256-chunk map block and more than two 128-lane workgroups;
    70: a wave and a partial wave; 130: a workgroup and two lanes.  After every call every byte is the sequential encoder's,
    the bytes between and behind the chunks are untouched, and each encoder's statistics are what a fresh context reports
    after making only that encoder's last call: one encoder's run moves neither the other's counters nor where they are read."""
    gap = 3
    w300, w70 = (Stream(walks[n].pcm, walks[n].sizes.tolist(), gap) for n in (300, 70))
    r130 = _ragged(orc, 31, 130, gap)
    assert (w300.n, w70.n, r130.n) == (300, 70, 130) and 0 in r130.sizes and 2048 in r130.sizes

    def call(c, kind, s):
        if kind == "plain":
            blob, trellis = run_plain_dev(c, s), 0
        else:
            (blob, so), trellis = run_dev(c, s, 1), 1
            assert so.tolist() == s.want(orc, 1)[2], (kind, s.n)
        bad = np.flatnonzero(blob != s.want_blob(orc, trellis))      # (the gaps and what lies behind are 0xEE in both)
        assert bad.size == 0, (kind, s.n, "first differing byte", int(bad[0]), "chunk", int(np.searchsorted(s.offs, bad[0], "right")) - 1)

    def stats(c, kind):
        return c.adpcm_chain_stats() if kind == "plain" else c.adpcm_trellis_chain_stats()

    def fresh(kind, s):
        c = pkg.Context(0)
        try:
            call(c, kind, s)
            return stats(c, kind)
        finally:
            c.close()

    c = pkg.Context(0)
    try:
        last = {}
        for kind, s in (("plain", w300), ("trellis", w70), ("plain", r130), ("trellis", w300)):
            call(c, kind, s)
            last[kind] = fresh(kind, s)
            for k, want in last.items():
                got = stats(c, k)
                print("after %s of %d chunks: %s %s (fresh context: %s)" % (kind, s.n, k, got, want))
                assert got == want, (kind, s.n, k)
    finally:
        c.close()
