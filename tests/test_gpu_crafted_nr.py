"""The -nr kernels (amv_nr_sums_kernel, amv_nr_chain_kernel, the kNr instantiations of transform_block in
amv_encode_frame_kernel and amv_forward_kernel) on a real MI355X over the crafted corpus of tests/nr_builder.py: every case
from its start state, against tests/nr_ref.py and tests/nr_trellis_ref.py -- every chunk byte for byte, d_offs, d_lens, the
fill pattern behind the last chunk and all 65 words of the state that comes out.  Integers and bytes: no tolerance.

What each case is there for, that it reaches it, and that each named fault of nr_ref.faults_of would change these very
expectations is tests/test_nr_builder.py's (no GPU).  Every start state is inside the bound of amv_nr_plan.h; no state outside
it is run here.

Rows are padded with a poison byte and the blob is filled with a pattern.  Streams of more than one frame are also run split
into two calls with the state carried on the device.  A failure names the case, the entry, the mode, the first differing
frame and the first differing (MCU, block, coefficient) -- found by decoding the GPU's chunk with the oracle's
entropy_blocks -- or says that only the state differs, which points at the sums kernel or the chain."""
import numpy as np
import pytest

import nr_builder as B
import nr_ref as N
import nr_trellis_ref as NT
import pixel_builder as pb
from test_gpu_parity import _t

pytestmark = pytest.mark.gpu

POISON = 0xEE
_MODEL = {}


@pytest.fixture(scope="module")
def cases(orc):
    return B.corpus(orc)[0]


def _pattern(n):
    return ((np.arange(n, dtype=np.int64) * 7 + 3) & 0xFF).astype(np.uint8)


def _model(key, frames, c, qbias, lam=None):
    """the model's (chunks, zig-zag lines per frame, state afterwards) of the case's stream, made once per key"""
    if key not in _MODEL:
        st = c.state.copy()
        if lam is None:
            lines = N.encode_stream(frames, c.w, c.h, c.nr, state=st, qbias=qbias, want_coef=True)
        else:
            lines = NT.encode_stream(frames, c.w, c.h, c.nr, lam, state=st, qbias=qbias, want_coef=True)
        _MODEL[key] = ([N._chunk(zz) for zz in lines], lines, st)
    return _MODEL[key]


def _pack(frames, w, h, pad=8):
    n, cw, ch = len(frames), w // 2, h // 2
    ys, cs = w + pad, cw + pad
    Y, Cb, Cr = np.full((n, h, ys), POISON, np.uint8), np.full((n, ch, cs), POISON, np.uint8), np.full((n, ch, cs), POISON, np.uint8)
    for i, (y, cb, cr) in enumerate(frames):
        Y[i, :, :w], Cb[i, :, :cw], Cr[i, :, :cw] = y, cb, cr
    return Y, Cb, Cr, ys, cs


def _grey(frames, w, h):
    """R = G = B = Y of the luma planes -> pixels [n, h, stride], rows padded with the poison byte"""
    stride = w * 3 + 5
    pix = np.full((len(frames), h, stride), POISON, np.uint8)
    for i, (y, _, _) in enumerate(frames):
        pix[i, :, : w * 3] = np.repeat(y, 3, axis=1)
    return pix, stride


def _call(ctx, entry, c, frames, qbias, lam, bgr, d_state):
    """one call of `entry` on these frames of the case -> (blob, offs, lens, cap) as numpy; d_state is read and written"""
    import torch
    n, w, h = len(frames), c.w, c.h
    cap = ctx.encode_bound(w, h) * n
    d_blob = _t(_pattern(cap + 64))
    d_offs = torch.full((n,), -1, dtype=torch.int64, device="cuda:0")
    d_lens = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    out = (d_blob, cap, d_offs, d_lens)
    if entry == "rgb":
        pix, stride = _grey(frames, w, h)
        ctx.encode_nr_stream_dev(_t(pix), stride, bgr, n, w, h, qbias, c.nr, d_state, *out)
    else:
        Y, Cb, Cr, ys, cs = _pack(frames, w, h)
        args = (_t(Y), _t(Cb), _t(Cr), ys, cs, h * ys, (h // 2) * cs, n, w, h, qbias)
        if entry == "nr":
            ctx.encode_yuv420_nr_stream_dev(*args, c.nr, d_state, *out)
        else:
            ctx.encode_yuv420_nr_trellis_stream_dev(*args, c.nr, lam, d_state, *out)
    torch.cuda.synchronize()
    return d_blob.cpu().numpy(), d_offs.cpu().numpy(), d_lens.cpu().numpy(), cap


def _where(orc, got, lines):
    """the first differing (MCU, block, coefficient) of a chunk the GPU made"""
    mine, st = orc.entropy_blocks(got, len(lines)) if len(got) >= 4 else (lines[:0], 1)
    bad = next((k for k in range(len(lines)) if k >= len(mine) or (mine[k] != lines[k]).any()), None)
    if bad is None:
        return "every coefficient decodes as the model's: the coder's stuffing, padding or trailer"
    if bad >= len(mine):
        return "MCU %d, block %d: not decoded (status %d)" % (bad // 6, bad % 6, st)
    k = int(np.flatnonzero(mine[bad] != lines[bad])[0])
    nat = int(pb.NATURAL_OF_SCAN[k])
    return "MCU %d, block %d, coefficient %d in scan order (row %d, column %d): got %d, want %d" % (
        bad // 6, bad % 6, k, nat >> 3, nat & 7, mine[bad][k], lines[bad][k])


def _compare(orc, what, parts, want, lines, want_state, got_state):
    """parts: [(blob, offs, lens, cap)] of the calls in order -> None or the description of the first difference"""
    i = 0
    for blob, offs, lens, cap in parts:
        pos = 0
        for j in range(len(offs)):
            o, l = int(offs[j]), int(lens[j])
            got = blob[o: o + max(l, 0)].tobytes() if 0 <= o <= len(blob) else b""
            if (o, l) != (pos, len(want[i])) or got != want[i]:
                at = next((k for k in range(min(len(got), len(want[i]))) if got[k] != want[i][k]), min(len(got), len(want[i])))
                return "%s: frame %d at %d + %d (want %d + %d), chunk byte %d: %s" % (what, i, o, l, pos, len(want[i]), at, _where(orc, got, lines[i]))
            pos += l
            i += 1
        if not (blob[pos:] == _pattern(len(blob))[pos:]).all():
            return "%s: the fill pattern behind the last chunk (byte %d of a blob of %d + 64) was written" % (what, pos, cap)
    if not (got_state == want_state).all():
        bad = np.flatnonzero(got_state != want_state)
        return "%s: every chunk is right and only the state differs -- the sums kernel or the chain: words %s, got %s, want %s" % (
            what, bad[:8], got_state[bad[:4]], want_state[bad[:4]])
    return None


def _run_all(ctx, orc, cases, entry, mode, qbias=None, lam=None, bgr=0):
    failures = []
    for c in cases:
        q = c.qbias if qbias is None else qbias
        frames = c.frames
        if entry == "rgb":
            frames = [pb.to_planes(orc, np.repeat(y[:, :, None], 3, axis=2), c.w, c.h, bgr) for y, _, _ in c.frames]
        want, lines, want_state = _model((c.name, entry if entry != "rgb" else ("rgb", bgr), q, lam), frames, c, q, lam)
        splits = [[(0, len(frames))]] + ([[(0, 1), (1, len(frames))]] if len(frames) > 1 else [])
        for split in splits:
            d_state = _t(c.state.astype(np.int32))
            parts = [_call(ctx, entry, c, c.frames[lo:hi], q, lam, bgr, d_state) for lo, hi in split]
            what = "%s [%dx%d x %d, nr %d, qbias %d%s] entry %s%s, %s, %s" % (
                c.name, c.w, c.h, len(frames), c.nr, q, "" if lam is None else ", lambda %d" % lam, entry, (" bgr", " rgb")[1 - bgr] if entry == "rgb" else "",
                mode, "one call" if len(split) == 1 else "two calls with the state carried")
            bad = _compare(orc, what, parts, want, lines, want_state, d_state.cpu().numpy().astype(np.int64))
            if bad:
                failures.append(bad)
    assert not failures, "%d runs over %d cases differ:\n%s" % (len(failures), len(cases), "\n".join(failures[:6]))


@pytest.fixture
def in_mode(ctx, pkg):
    def run(mode, fn):
        try:
            ctx.set_entropy_mode(pkg.ENTROPY_SERIAL if mode == "serial" else pkg.ENTROPY_AUTO)
            fn()
        finally:
            ctx.set_entropy_mode(pkg.ENTROPY_AUTO)
    return run


@pytest.mark.parametrize("qbias", [0, 128])
@pytest.mark.parametrize("mode", ["auto", "serial"])
def test_nr_entry(ctx, orc, cases, in_mode, mode, qbias):
    """amvhip_encode_yuv420_nr_stream_dev: the one-kernel route (auto) and the amv_forward_kernel route (serial)"""
    in_mode(mode, lambda: _run_all(ctx, orc, cases, "nr", mode, qbias=qbias))


@pytest.mark.parametrize("lam", [0, 3481])
@pytest.mark.parametrize("mode", ["auto", "serial"])
def test_nr_trellis_entry(ctx, orc, cases, in_mode, mode, lam):
    """amvhip_encode_yuv420_nr_trellis_stream_dev: the search runs on what the dead zone left"""
    in_mode(mode, lambda: _run_all(ctx, orc, cases, "trellis", mode, lam=lam))


@pytest.mark.parametrize("bgr", [0, 1])
@pytest.mark.parametrize("mode", ["auto", "serial"])
def test_rgb_entry(ctx, orc, cases, in_mode, mode, bgr):
    """amvhip_encode_nr_stream_dev on grey pixels R = G = B = Y of each case's luma plane: the expected planes are the
    oracle's rgb24_to_yuvj420p of them, and the model runs on those"""
    in_mode(mode, lambda: _run_all(ctx, orc, cases, "rgb", mode, bgr=bgr))
