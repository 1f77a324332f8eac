"""Reduced-size decode (lowres 1, 2, 3) on a real MI355X: every comparison byte for byte against tests/lowres_ref.py, whose
block arithmetic tests/golden/ref_lowres.json pins to the reference's own `ffmpeg -lowres`.

Every output buffer is filled with a pattern and has a sentinel byte behind its last frame; the frames lie back to back at
amvhip_lowres_frame_bytes (odd for most sizes here), so a store outside a frame shows in its neighbour or in the sentinel."""
import numpy as np
import pytest

import coef_builder as cb
import lowres_ref as R
from test_gpu_parity import _blob_of, _t

pytestmark = pytest.mark.gpu

FILL = 0x5A
LEVELS = (1, 2, 3)
# 16x16: one MCU; 160x120: h % 16 = 8; 130x98: the row shift, W_L and H_L odd at L = 2 and 3; 336x32: 21 MCUs per row, three
# segments, the last one partial; 37x23: odd everywhere, one partial MCU column; 128x96: the first frames of AMV1.amv
GEOMETRIES = ((16, 16, 8), (160, 120, 4), (130, 98, 3), (336, 32, 3), (37, 23, 5), (128, 96, 6))
ROUND_WALKERS = 512          # amv_segment.h: kRoundWalkers, the most walkers a round launch of any back half has


def _chunks(orc, amv1, w, h, n, first=0):
    """n chunks of a w x h stream: AMV1.amv's at its own size, else the oracle's encoder on whole MCUs (it wants even sizes;
    the scan depends on the MCU grid alone)"""
    if (w, h) == (128, 96):
        return [bytes(c) for c in amv1["video"][first: first + n]]
    ew, eh = (w + 15) // 16 * 16, (h + 15) // 16 * 16
    return [bytes(orc.encode_frame(orc.synth_frame(0x10E5, first + t, ew, eh), ew, eh)) for t in range(n)]


class Expect:
    """the restatement's frames, computed once per (chunk, geometry, level)"""

    def __init__(self, orc):
        self.orc, self.tables, self.seen = orc, R.q60_tables(orc), {}

    def frame(self, chunk, w, h, L):
        key = (chunk, w, h, L)
        if key not in self.seen:
            nb = ((w + 15) // 16) * ((h + 15) // 16) * 6
            done, _ = self.orc.entropy_blocks(chunk, nb)
            coef = np.zeros((nb, 64), np.int16)
            coef[: len(done)] = done
            _, st, ok = self.orc.decode_frame_ffmpeg(chunk, w, h)
            self.seen[key] = (R.picture(coef, w, h, L, ok, self.tables), st)
        return self.seen[key]

    def frames(self, chunks, w, h, L):
        got = [self.frame(c, w, h, L) for c in chunks]
        return np.stack([g[0] for g in got]), np.array([g[1] for g in got], np.int32)


@pytest.fixture(scope="module")
def expect(orc):
    return Expect(orc)


def _decode(ctx, pkg, chunks, w, h, L, fmt=None, stride=None, frame_bytes=None):
    """-> (frames [n, frame bytes], statuses); checks the sentinel behind the last frame"""
    import torch
    n = len(chunks)
    fmt = pkg.PIX_YUVJ420P if fmt is None else fmt
    fb = frame_bytes or ctx.lowres_frame_bytes(w, h, L)
    blob, offs, lens, nbytes = _blob_of(chunks, pad_front=1)
    d_out = torch.full((n * fb + 1,), FILL, dtype=torch.uint8, device="cuda:0")
    d_st = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    ctx.decode_lowres_batch_dev(_t(blob), nbytes, _t(offs), _t(lens), n, w, h, pkg.FLAG_FFMPEG, L, fmt, d_out,
                                stride or ctx.lowres_dim(w, L), d_st, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert out[-1] == FILL, "the byte behind the last frame was written (%dx%d lowres %d)" % (w, h, L)
    return out[:-1].reshape(n, fb), d_st.cpu().numpy()


def _same(got, want, what):
    if not (got == want).all():
        f, at = np.argwhere(got != want)[0]
        pytest.fail("%s: frame %d byte %d: got %d, want %d (%d bytes differ)" % (what, f, at, got[f, at], want[f, at], int((got != want).sum())))


@pytest.mark.parametrize("entropy", ["auto", "serial"])
@pytest.mark.parametrize("w,h,n", GEOMETRIES, ids=["%dx%d" % g[:2] for g in GEOMETRIES])
def test_whole_path(ctx, pkg, orc, amv1, expect, w, h, n, entropy):
    """both entropy modes (AMVHIP_ENTROPY_SERIAL sends every frame through the round launches, kRound), every level"""
    chunks = _chunks(orc, amv1, w, h, n)
    ctx.set_entropy_mode(pkg.ENTROPY_SERIAL if entropy == "serial" else pkg.ENTROPY_AUTO)
    try:
        for L in LEVELS:
            assert ctx.lowres_frame_bytes(w, h, L) == R.frame_bytes(w, h, L)
            want, want_st = expect.frames(chunks, w, h, L)
            got, st = _decode(ctx, pkg, chunks, w, h, L)
            assert (st == want_st).all() and (st == 0).all()
            _same(got, want, "%dx%d lowres %d %s" % (w, h, L, entropy))
    finally:
        ctx.set_entropy_mode(pkg.ENTROPY_AUTO)


def test_round_launch_walks(ctx, pkg, orc, amv1, expect):
    """the smallest batch whose round launch makes a workgroup walk to a second item: one more frame than the launch has
    walkers (amv_piece_map.h: for_each_launch, min(items, kRoundWalkers)), in the mode that sends every frame through the
    rounds; 16x16"""
    w = h = 16
    n = ROUND_WALKERS + 1
    few = _chunks(orc, amv1, w, h, 7)
    chunks = [few[(i * 3) % 7] for i in range(n)]
    ctx.set_entropy_mode(pkg.ENTROPY_SERIAL)
    try:
        for L in LEVELS:
            want, _ = expect.frames(chunks, w, h, L)
            got, st = _decode(ctx, pkg, chunks, w, h, L)
            assert (st == 0).all()
            _same(got, want, "16x16 x %d lowres %d, round launch" % (n, L))
    finally:
        ctx.set_entropy_mode(pkg.ENTROPY_AUTO)


def _damage(orc, chunk, w, h, bit, start):
    """the first single-bit flip at or after byte `start` that gives the chunk a status with `bit` set, some MCUs before it"""
    for pos in range(start, len(chunk) - 2):
        for k in range(8):
            c = bytearray(chunk)
            c[pos] ^= 1 << k
            _, st, ok = orc.decode_frame_ffmpeg(bytes(c), w, h)
            if st & bit and ok > 0:
                return bytes(c)
    raise AssertionError("no such flip")


def test_damaged_chunks(ctx, pkg, orc, amv1, expect):
    """three AMV1 chunks: truncated, a flipped bit (a code no table has), an overrun (a run past coefficient 63): the statuses
    are those of amvhip_decode_batch_dev and everything from the failing MCU on is zero"""
    import torch
    w, h = 128, 96
    a, b, c = (bytes(x) for x in amv1["video"][3:6])
    chunks = [a, a[: len(a) // 2], _damage(orc, b, w, h, pkg.ST_FORMAT, len(b) // 2), _damage(orc, c, w, h, pkg.ST_OVERRUN, len(c) // 3), c]
    blob, offs, lens, nbytes = _blob_of(chunks, pad_front=1)
    d_full = torch.empty((len(chunks), ctx.yuv420_frame_bytes(w, h)), dtype=torch.uint8, device="cuda:0")
    d_st = torch.full((len(chunks),), -1, dtype=torch.int32, device="cuda:0")
    ctx.decode_batch_dev(_t(blob), nbytes, _t(offs), _t(lens), len(chunks), w, h, pkg.FLAG_FFMPEG, d_full, d_st,
                         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    full_st = d_st.cpu().numpy()
    assert full_st[0] == 0 and full_st[4] == 0 and full_st[1] & pkg.ST_TRUNCATED and full_st[2] & pkg.ST_FORMAT and full_st[3] & pkg.ST_OVERRUN, full_st
    for L in LEVELS:
        want, want_st = expect.frames(chunks, w, h, L)
        got, st = _decode(ctx, pkg, chunks, w, h, L)
        assert (st == full_st).all() and (st == want_st).all(), (st, full_st, want_st)
        _same(got, want, "damaged chunks, lowres %d" % L)
        bs = 8 >> L
        for i in (1, 2, 3):       # 128x96 is the exact flip: MCU (my, mx) shows in luma rows H_L - (my + 1) * 2bs .., columns mx * 2bs ..
            ok = orc.decode_frame_ffmpeg(chunks[i], w, h)[2]
            assert 0 < ok < 48 or (i == 1 and ok == 48)      # (the cut chunk's zero tail still decodes as blocks)
            y = R.split(got[i], R.plane_sizes(w, h, L))[0]
            for m in range(48):
                my, mx = divmod(m, 8)
                area = y[y.shape[0] - (my + 1) * 2 * bs: y.shape[0] - my * 2 * bs, mx * 2 * bs: (mx + 1) * 2 * bs]
                assert m < ok or not area.any(), (i, L, m)
            assert y[y.shape[0] - 2 * bs:, : 2 * bs].any()


# ---- crafted coefficients through amvhip_reconstruct_lowres_dev ---------------------------------------------------------

def _level(target, q, dc):
    """the int16 level whose dequantised value (int16)(level * q) (+ 1024 on the DC) is nearest to `target` (an odd step
    reaches every value)"""
    v = np.arange(-32768, 32768, dtype=np.int64)
    miss = np.abs(R.wrap16(v * int(q) + (1024 if dc else 0)) - target)
    best = np.nonzero(miss == miss.min())[0]
    return int(v[best[np.argmin(np.abs(v[best]))]])


def _line(nat, comp):
    """an 8x8 block of dequantised TARGETS in natural order -> the scan-order line of levels that makes it (Q60 tables)"""
    nat = np.asarray(nat, np.int64).reshape(64)
    line = np.zeros(64, np.int64)
    for p in sorted(set(np.nonzero(nat)[0].tolist()) | {0}):      # (the DC always: 1024 is added to it)
        s = int(cb.SCAN_OF_NATURAL[p])
        line[s] = _level(int(nat[p]), int(cb.Q60[comp][s]), p == 0)
    return line


def _block(**at):
    nat = np.zeros((8, 8), np.int64)
    for k, v in at.items():
        nat[int(k[1]), int(k[2])] = v
    return nat


def _crafted_blocks():
    """[(name, natural-order targets)]"""
    rng = np.random.default_rng(0x10F4)
    out = []
    # the four d2 / d6 shapes, in a row and in a column; for d2 == 0, d6 != 0 values on which 10703 against 10704 reaches a pixel
    for axis in ("row", "column"):
        p = (lambda k: (0, k)) if axis == "row" else (lambda k: (k, 0))
        found = 0
        while found < 6:
            nat = np.zeros((8, 8), np.int64)
            nat[0, 0], nat[p(3)] = rng.integers(0, 2040), rng.integers(-2000, 2000)
            nat[p(2)] = 8 * rng.integers(-40, 40) * (found & 1)                    # (luma's step at (0, 2) is 8)
            if (np.clip(R.rev_dct4(nat[None]), 0, 255) != np.clip(R.rev_dct4(nat[None], folded=True), 0, 255)).any():
                out.append(("d2=0,d6 in a %s #%d" % (axis, found), nat))
                found += 1
        for d2, d6 in ((1, 1), (1, 0), (0, 0)):
            for k in range(3):
                nat = np.zeros((8, 8), np.int64)
                nat[0, 0], nat[p(2)] = rng.integers(0, 2040), rng.integers(-600, 600)
                nat[p(1)], nat[p(3)] = d2 * rng.integers(1, 900) * (-1) ** k, d6 * rng.integers(1, 900)
                out.append(("d2=%d,d6=%d in a %s #%d" % (d2, d6, axis, k), nat))
    # a DC-only row beside a full row, both ways round
    out.append(("dc-only row over a full row", _block(a00=900, a10=-300, a11=250, a12=-200, a13=150)))
    out.append(("full row over a dc-only row", _block(a00=900, a01=-300, a02=250, a03=-200, a10=400)))
    out.append(("dc-only rows 1 and 3", _block(a00=700, a01=90, a10=-500, a30=333)))
    # data[0] + 4 and d0 << PASS1_BITS at the int16 wrap
    for dc in (32763, 32764, 32767, -32768, -32765, 8187, 8188, 8191, 8192, -8197, -8196, -8193, 16380, -16388, 24572):
        out.append(("dc %d alone" % dc, _block(a00=dc)))
        out.append(("dc %d over a row" % dc, _block(a00=dc, a10=40, a11=-30)))
        out.append(("dc %d in a full row" % dc, _block(a00=dc, a01=25, a02=-12, a03=7)))
    # outputs at -1, 0, 255, 256 and far beyond the clamp (a flat block gives (dc + 4) >> 3)
    for dc in (-13, -12, -5, -4, 3, 4, 2035, 2036, 2043, 2044, 2051, 2052, 9000, -9000, 30000, -30000):
        out.append(("flat %d" % dc, _block(a00=dc)))
        out.append(("flat %d with a ripple" % dc, _block(a00=dc, a01=9, a10=-9, a11=5)))
    # non-zero coefficients only outside the corner a level reads
    out.append(("outside 4x4", _block(a00=1000, a04=500, a40=-500, a44=300, a77=-900, a34=700, a43=-700)))
    out.append(("outside 2x2", _block(a00=1000, a02=500, a20=-500, a22=300, a13=-900, a31=700)))
    out.append(("outside 1x1", _block(a00=1000, a01=500, a10=-500, a11=300)))
    return out


@pytest.fixture(scope="module")
def crafted(orc):
    """frames of 48x32 (6 MCUs): ordinary, the crafted blocks packed into whole frames (a block's targets in a luma and in a
    chroma slot), ordinary, and an ordinary frame at nmcu_ok 0, 1 and one short of the frame"""
    w, h, nm = 48, 32, 6
    rng = np.random.default_rng(0xC0F5)
    blocks = _crafted_blocks()
    lines = [(name, comp, _line(nat, comp)) for name, nat in blocks for comp in (0, 1)]
    luma, chroma = [l for l in lines if l[1] == 0], [l for l in lines if l[1] == 1]
    frames, names = [cb.ordinary(rng, w, h)], ["ordinary"]
    per = nm * 4
    for f in range((len(luma) + per - 1) // per):
        coef = np.zeros((nm * 6, 64), np.int64)
        held = []
        for m in range(nm):
            for k in range(6):
                src, i = (luma, f * per + m * 4 + k) if k < 4 else (chroma, (f * nm * 2 + m * 2 + k - 4) % len(chroma))
                if i < len(src):
                    coef[m * 6 + k] = src[i][2]
                    held.append(src[i][0])
        frames.append(coef)
        names.append("crafted frame %d (%s ... %s)" % (f, held[0], held[-1]))
    frames.append(cb.ordinary(rng, w, h))
    names.append("ordinary")
    oks = [nm] * len(frames)
    for ok in (0, 1, nm - 1):
        frames.append(cb.ordinary(rng, w, h))
        names.append("ordinary, nmcu_ok %d" % ok)
        oks.append(ok)
    coef = np.stack(frames)
    assert coef.min() >= -32768 and coef.max() <= 32767
    return {"w": w, "h": h, "coef": np.ascontiguousarray(coef.astype(np.int16)), "ok": np.array(oks, np.uint32), "names": names,
            "blocks": blocks, "tables": R.q60_tables(orc)}


def test_crafted_blocks_are_what_they_claim(crafted):
    """(no device needed beyond the fixture) the levels hit the dequantised targets the names state, where the table's step
    allows, and the 'outside' blocks give the DC picture"""
    for name, nat in crafted["blocks"]:
        for comp in (0, 1):
            line = _line(nat, comp)
            coef = np.zeros((6, 64), np.int64)
            coef[0 if comp == 0 else 4] = line
            deq = R.dequantise(coef, crafted["tables"])[0 if comp == 0 else 4]
            steps = crafted["tables"][comp][cb.SCAN_OF_NATURAL].reshape(8, 8)
            assert (2 * np.abs(deq - nat) <= steps).all() and not deq[nat == 0].any(), (name, comp)
            if name.startswith("d2=0,d6 in") and comp == 0:      # (luma's steps there are odd: the targets are hit exactly)
                assert (deq == nat).all()
                assert (np.clip(R.rev_dct4(deq[None]), 0, 255) != np.clip(R.rev_dct4(deq[None], folded=True), 0, 255)).any(), name
            if name.startswith("outside"):
                bs = {"outside 4x4": 4, "outside 2x2": 2, "outside 1x1": 1}[name]
                alone = coef.copy()
                alone[:, 1:] = 0
                for L in LEVELS:
                    if 8 >> L <= bs:
                        assert (R.block_pixels(coef, L, crafted["tables"]) == R.block_pixels(alone, L, crafted["tables"])).all(), (name, L)


def test_crafted_coefficients(ctx, pkg, crafted):
    import torch
    w, h, coef, ok = crafted["w"], crafted["h"], crafted["coef"], crafted["ok"]
    n = len(coef)
    d_coef, d_ok = _t(coef), _t(ok)
    for L in LEVELS:
        fb = ctx.lowres_frame_bytes(w, h, L)
        want = np.stack([R.picture(coef[i], w, h, L, int(ok[i]), crafted["tables"]) for i in range(n)])
        d_out = torch.full((n * fb + 1,), FILL, dtype=torch.uint8, device="cuda:0")
        ctx.reconstruct_lowres_dev(d_coef, d_ok, n, w, h, L, d_out, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        assert out[-1] == FILL
        got = out[:-1].reshape(n, fb)
        for i in range(n):
            if not (got[i] == want[i]).all():
                at = int(np.flatnonzero(got[i] != want[i])[0])
                pytest.fail("%s, lowres %d: byte %d: got %d, want %d" % (crafted["names"][i], L, at, got[i, at], want[i, at]))
        assert not got[-3].any() and got[-2].any() and got[-1].any()             # nmcu_ok 0: all zero


@pytest.mark.parametrize("w,h", [(16, 16), (176, 16)], ids=["16x16", "176x16"])
def test_reconstruct_launch_in_parts(ctx, pkg, orc, monkeypatch, w, h):
    """a default launch in parts (amv_piece_map.h: for_each_launch with item_base): 7 frames through
    amvhip_reconstruct_lowres_dev in parts of 3 (AMVHIP_RECON_MOST, read at every launch), at one segment per MCU row and
    at two with the second one short (11 MCUs); every level, byte for byte the same as the call in one part and as the
    restatement"""
    import torch
    n, nm = 7, ((w + 15) // 16) * ((h + 15) // 16)
    rng = np.random.default_rng(0x9A27)
    coef = np.ascontiguousarray(np.stack([cb.ordinary(rng, w, h) for _ in range(n)]).astype(np.int16))
    ok = np.array([nm, nm, 0, nm, max(nm - 1, 0), nm, nm], np.uint32)
    d_coef, d_ok = _t(coef), _t(ok)
    tables = R.q60_tables(orc)
    for L in LEVELS:
        fb = ctx.lowres_frame_bytes(w, h, L)
        want = np.stack([R.picture(coef[i], w, h, L, int(ok[i]), tables) for i in range(n)])
        got = {}
        for most in (None, "3"):
            if most:
                monkeypatch.setenv("AMVHIP_RECON_MOST", most)
            else:
                monkeypatch.delenv("AMVHIP_RECON_MOST", raising=False)
            d_out = torch.full((n * fb + 1,), FILL, dtype=torch.uint8, device="cuda:0")
            ctx.reconstruct_lowres_dev(d_coef, d_ok, n, w, h, L, d_out, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            out = d_out.cpu().numpy()
            assert out[-1] == FILL
            got[most] = out[:-1].reshape(n, fb)
        monkeypatch.delenv("AMVHIP_RECON_MOST", raising=False)
        _same(got["3"], got[None], "%dx%d lowres %d, in parts of 3 against one part" % (w, h, L))
        _same(got["3"], want, "%dx%d lowres %d, in parts of 3" % (w, h, L))


def test_dst_fmt(ctx, pkg, orc, amv1):
    """RGB24 and GRAY8 at 130x98, lowres 2 (33 x 25), rows wider than the picture: the YUVJ420P result put through
    amvhip_img_convert_dev, and the bytes between the rows untouched"""
    import torch
    w, h, L, n = 130, 98, 2, 3
    wl, hl = ctx.lowres_dim(w, L), ctx.lowres_dim(h, L)
    assert (wl, hl) == (33, 25)
    chunks = _chunks(orc, amv1, w, h, n, first=4)
    planes, st = _decode(ctx, pkg, chunks, w, h, L)
    assert (st == 0).all()
    cw, ch = (wl + 1) // 2, (hl + 1) // 2
    y, cbp, crp = (_t(np.ascontiguousarray(planes[:, a:b])) for a, b in ((0, wl * hl), (wl * hl, wl * hl + cw * ch), (wl * hl + cw * ch, wl * hl + 2 * cw * ch)))
    for fmt, bpp, stride in ((pkg.PIX_RGB24, 3, 33 * 3 + 5), (pkg.PIX_GRAY8, 1, 33 + 7)):
        fb = stride * hl
        assert fb == ctx.lib.amvhip_pix_frame_bytes(fmt, stride, hl)
        got, st = _decode(ctx, pkg, chunks, w, h, L, fmt=fmt, stride=stride, frame_bytes=fb)
        assert (st == 0).all()
        d_want = torch.full((n, fb), FILL, dtype=torch.uint8, device="cuda:0")
        ctx.img_convert_dev(pkg.PIX_YUVJ420P, ((y, cbp, crp), wl, cw, wl * hl, cw * ch), fmt, ((d_want,), stride, 0, fb, 0), wl, hl, n,
                            torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        want = d_want.cpu().numpy()
        rows = want.reshape(n, hl, stride)
        assert (rows[:, :, wl * bpp:] == FILL).all() and (rows[:, :, : wl * bpp] != FILL).any()
        _same(got, want, "dst_fmt %d" % fmt)


def test_full_size_unchanged_and_refusals(ctx, pkg, orc, amv1, expect):
    """amvhip_decode_batch_dev with AMVHIP_FLAG_FFMPEG gives the same bytes on one context before and after reduced-size
    calls; a live context refuses what the header says it refuses, and writes nothing"""
    import torch
    w, h, n = 130, 98, 3
    chunks = _chunks(orc, amv1, w, h, n)
    blob, offs, lens, nbytes = _blob_of(chunks, pad_front=1)
    d_blob, d_offs, d_lens = _t(blob), _t(offs), _t(lens)

    def full():
        d_out = torch.full((n, ctx.yuv420_frame_bytes(w, h)), FILL, dtype=torch.uint8, device="cuda:0")
        d_st = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
        ctx.decode_batch_dev(d_blob, nbytes, d_offs, d_lens, n, w, h, pkg.FLAG_FFMPEG, d_out, d_st, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return d_out.cpu().numpy(), d_st.cpu().numpy()

    before, st0 = full()
    want = np.stack([orc.decode_frame_ffmpeg(c, w, h)[0] for c in chunks])
    assert (before == want).all() and (st0 == 0).all()
    for L in LEVELS:
        got, _ = _decode(ctx, pkg, chunks, w, h, L)
        _same(got, expect.frames(chunks, w, h, L)[0], "130x98 lowres %d" % L)
    after, st1 = full()
    assert (after == before).all() and (st1 == st0).all()

    d_out = torch.full((4096,), FILL, dtype=torch.uint8, device="cuda:0")
    d_st = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    F, K, Y = pkg.FLAG_FFMPEG, pkg.FLAG_FFMPEG_KEEP, pkg.PIX_YUVJ420P
    call = lambda flags, L, fmt, stride: ctx.lib.amvhip_decode_lowres_batch_dev(ctx.h, d_blob.data_ptr(), nbytes, d_offs.data_ptr(), d_lens.data_ptr(), n, w,
                                                                                 h, flags, L, fmt, d_out.data_ptr(), stride, d_st.data_ptr(), None)
    for flags, L, fmt, stride in ((F, 0, Y, 130), (F, 4, Y, 9), (0, 1, Y, 65), (pkg.FLAG_ZIGZAG_FIXED, 1, Y, 65), (F | K, 1, Y, 65),
                                  (F | pkg.FLAG_ZIGZAG_FIXED, 1, Y, 65), (F, 1, Y, 66), (F, 1, Y, 64), (F, 1, Y, 130), (F, 2, pkg.PIX_RGB24, 98),
                                  (F, 1, pkg.PIX_YUYV422, 130), (F, 1, 99, 65)):
        assert call(flags, L, fmt, stride) == pkg.ERR_ARG, (flags, L, fmt, stride)
    for L in (0, 4):
        assert ctx.lib.amvhip_reconstruct_lowres_dev(ctx.h, d_out.data_ptr(), d_st.data_ptr(), 1, 16, 16, L, d_out.data_ptr(), None) == pkg.ERR_ARG
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == FILL).all() and (d_st.cpu().numpy() == -1).all()
