"""The reconstruction kernel's stage C pack and both stage D paths, against the oracle, on a real MI355X.

Stage C (amv_reconstruct.hip, clamp_pack): the column pass hands over x >> 7 and the clamp of x >> 14 to -256 .. 255 is
a saturating pack to int16 followed by a packed shift by 7.  Blocks are crafted -- DC only, and DC + one AC -- so that
the column sums x put x >> 14 on -258 -257 -256 -255 -1 0 254 255 256 257 and x >> 7 on +-32767 / +-32768 / +-32769,
in luma and in chroma blocks, under both zig-zag tables, one 16x16 frame per block; and blocks at the largest magnitudes
the stage accessor promises (DC at the ends of int16, one AC with |AC * step| at 100 000).  The sums come from a model
of the two passes written out below; before anything is launched the model's x >> 14 is checked against the oracle's
own values in front of its clamp (coef_builder.preclamp) in all 64 places of every targeted block.

Stage D: the whole-segment body (all ten MCUs decoded, 160 pixels, 16 rows) and the general loop beside it, by
geometry: 160x16 one whole segment; 160x24 a whole-segment row above a row of 8 lines; 16x16 and 130x98 short segments,
the right edge inside a patch and the byte tail; 336x32 whole segments with a short one behind them in the row; 176x144
the five-row workgroups.  In every batch: whole frames, a frame whose nmcu_ok ends inside a segment and one whose
nmcu_ok ends where a segment ends, random coefficients from a fixed seed, every byte of a pattern-filled buffer compared
with the builder's picture (row padding included).  160x16 also as scans: through the records form, and through the
serial entropy kernel, whose frames the round launch (FrameSel) reconstructs.
"""
import numpy as np
import pytest

import coef_builder as cb
import scan_builder as sb
from test_gpu_parity import _blob_of, _t

pytestmark = pytest.mark.gpu

W1, W2, W3, W5, W6, W7 = 2841, 2676, 2408, 1609, 1108, 565


def _pass(v, column):
    """one 8-point pass of the kernel's idct8 over the last axis of an int64 array (no 32-bit wrap: small inputs only);
    column=True: the sums x in front of the final shift"""
    v = [v[..., i] for i in range(8)]
    rnd, down = (4, 3) if column else (0, 0)
    a0 = (v[0] * 256 + 8192) if column else (v[0] * 2048 + 128)
    a1 = v[4] * (256 if column else 2048)
    i2, i3, i4, i5, i6, i7 = v[6], v[2], v[1], v[7], v[5], v[3]
    a4 = (W1 * i4 + W7 * i5 + rnd) >> down
    a5 = (W7 * i4 - W1 * i5 + rnd) >> down
    a6 = (W5 * i6 + W3 * i7 + rnd) >> down
    a7 = (W3 * i6 - W5 * i7 + rnd) >> down
    t = a0 + a1
    a0 = a0 - a1
    a2 = (W6 * i3 - W2 * i2 + rnd) >> down
    a3 = (W2 * i3 + W6 * i2 + rnd) >> down
    a1 = a4 + a6
    a4 = a4 - a6
    a6 = a5 + a7
    a5 = a5 - a7
    a7 = t + a3
    t = t - a3
    a3 = a0 + a2
    a0 = a0 - a2
    a2 = (181 * (a4 + a5) + 128) >> 8
    a4 = (181 * (a4 - a5) + 128) >> 8
    out = np.stack([a7 + a1, a3 + a2, a0 + a4, t + a6, t - a6, a0 - a4, a3 - a2, a7 - a1], -1)
    return out if column else out >> 8


def column_sums(nat):
    """[..., 8, 8] dequantised blocks in natural order -> [..., 8, 8] the column pass's sums x (the pixel is x >> 14, clamped)"""
    rows = _pass(np.asarray(nat, np.int64), False)
    return np.swapaxes(_pass(np.swapaxes(rows, -1, -2), True), -1, -2)


SHIFT14 = (-258, -257, -256, -255, -1, 0, 254, 255, 256, 257)
SHIFT7 = (32767, 32768, 32769, -32767, -32768, -32769)
AC_SCANS = (1, 2, 4, cb.QUIRK_STD, cb.QUIRK_SCAN)      # (0,1), (1,0), (1,1) and the two places the tables disagree about


def _lines(comp, flags):
    """{(what, target): a line that reaches it} for the blocks of one component under one zig-zag table"""
    found = {}
    dcs = np.arange(-420, 421)

    def note(lines, kind):
        slots = np.zeros((len(lines) * 6, 64), np.int64)
        at = 0 if comp == 0 else 4
        slots[at::6] = lines
        x = column_sums(cb.dequantised(slots, flags)[at::6]).reshape(len(lines), 64)
        for what, shift, targets in (("x >> 14", 14, SHIFT14), ("x >> 7", 7, SHIFT7)):
            for t in targets:
                hit = np.nonzero(((x >> shift) == t).any(1))[0]
                if hit.size and (kind, what, t) not in found:
                    found[(kind, what, t)] = lines[hit[len(hit) // 2]].copy()

    flat = np.zeros((dcs.size, 64), np.int64)
    flat[:, 0] = dcs
    note(flat, "DC")
    for s in AC_SCANS:
        for ac in list(range(1, 41)) + list(range(-40, 0)):
            lines = np.zeros((dcs.size, 64), np.int64)
            lines[:, 0] = dcs
            lines[:, s] = ac
            note(lines, "DC+AC%d" % s)
    return found


def _largest(comp):
    q, out = cb.QUANT[comp], []
    for s in (1, 2, 4, cb.QUIRK_STD, cb.QUIRK_SCAN, 63):
        v = min(cb.AC_BOUND // int(q[s]), 32767)
        for dc in (32767, -32767, -32768):
            out += [cb.one(s, v, dc=dc), cb.one(s, -v, dc=dc)]
    out += [cb.one(0, dc) for dc in (32767, -32767, -32768)]
    return out


def _frame_of(line, comp):
    """a 16x16 frame: the line in all four luma blocks, or in both chroma blocks beside a mid-grey luma"""
    coef = np.zeros((6, 64), np.int64)
    if comp == 0:
        coef[:4] = line
    else:
        coef[4:] = line
    return coef


@pytest.fixture(scope="module")
def clamp_cases(orc):
    """{flags: (names, coef [n, 6, 64] int16, want [n, 16, stride])}; the targets are checked against the oracle here"""
    out = {}
    for flags in (0, 1):
        names, frames = [], []
        for comp in (0, 1):
            found = _lines(comp, flags)
            kinds = {k[0] for k in found}
            for t in SHIFT14:       # a flat luma block reaches every level; chroma's DC step of 9 skips one level in nine
                assert comp == 1 or ("DC", "x >> 14", t) in found, (comp, t)
                assert any((k, "x >> 14", t) in found for k in kinds - {"DC"}), (comp, flags, t)
            for t in SHIFT7:
                assert any((k, "x >> 7", t) in found for k in kinds - {"DC"}), (comp, flags, t)
            for (kind, what, t), line in sorted(found.items()):
                # the oracle's own values in front of its clamp, in all 64 places, against the model's x >> 14
                slots = np.zeros((6, 64), np.int64)
                slots[0 if comp == 0 else 4] = line
                x = column_sums(cb.dequantised(slots, flags)[0 if comp == 0 else 4]).reshape(64)
                pre = cb.preclamp(orc, line, comp, flags)
                assert pre is not None and (pre == (x >> 14)).all(), (comp, flags, kind, what, t)
                assert ((x >> (14 if what == "x >> 14" else 7)) == t).any()
                names.append("%s %s %s = %d" % ("luma" if comp == 0 else "chroma", kind, what, t))
                frames.append(_frame_of(line, comp))
            for i, line in enumerate(_largest(comp)):
                names.append("%s largest #%d" % ("luma" if comp == 0 else "chroma", i))
                frames.append(_frame_of(line, comp))
        coef = np.stack(frames).astype(np.int16)
        want = np.stack([cb.picture(orc, c, 16, 16, 1, flags) for c in coef])
        out[flags] = (names, coef, want)
    return out


def _reconstruct(ctx, coef, oks, w, h, flags):
    import torch
    n = len(coef)
    d_out = torch.full((n, h, ctx.stride(w)), 0x5A, dtype=torch.uint8, device="cuda:0")
    ctx.reconstruct_dev(_t(np.ascontiguousarray(coef, np.int16)), _t(np.asarray(oks, np.uint32)), n, w, h, flags, d_out)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def _same(got, want, names, what):
    for i in range(len(want)):
        if not (got[i] == want[i]).all():
            at = int(np.flatnonzero(got[i].reshape(-1) != want[i].reshape(-1))[0])
            row, col = divmod(at, got.shape[-1])
            pytest.fail("%s, %s: stored row %d, byte %d: got %d, want %d (%d bytes differ)" % (
                what, names[i], row, col, got[i, row, col], want[i, row, col], int((got[i] != want[i]).sum())))


@pytest.mark.parametrize("flags", [0, 1])
def test_clamp_boundaries(ctx, clamp_cases, flags):
    names, coef, want = clamp_cases[flags]
    assert len(names) >= 2 * (len(SHIFT14) + len(SHIFT7))
    got = _reconstruct(ctx, coef, np.ones(len(coef), np.uint32), 16, 16, flags)
    _same(got, want, names, "zig-zag flag %d" % flags)


# ------------------------------------------------------------------------------------------------ stage D

GEOMETRIES = ((160, 16), (160, 24), (16, 16), (130, 98), (336, 32), (176, 144))


def _random_frame(rng, w, h):
    """coefficients a scan can carry, sized so that most pixels stay between their clamps: every block another DC, a third
    of the twenty lowest ACs and a twentieth of the others non-zero"""
    nb = sb.mcus(w, h) * 6
    coef = rng.integers(-2, 3, (nb, 64)) * (rng.random((nb, 64)) < 0.05)
    coef[:, 1:21] = rng.integers(-7, 8, (nb, 20)) * (rng.random((nb, 20)) < 0.3)
    coef[:, 0] = rng.integers(-70, 71, nb)
    return coef


def _cuts(w, h):
    """(an nmcu_ok inside a segment, one where a segment ends) -- a segment is ten MCUs of an MCU row, or what is left of it"""
    mcw, nm = (w + 15) // 16, sb.mcus(w, h)
    inside = [m for m in range(1, nm) if (m % mcw) % 10]
    at_end = [m for m in range(1, nm) if not (m % mcw) % 10]
    return (inside[len(inside) // 2] if inside else None), (at_end[len(at_end) // 2] if at_end else 0)


@pytest.fixture(scope="module")
def geometry_batches(orc):
    rng = np.random.default_rng(0xD5EED)
    out = {}
    for w, h in GEOMETRIES:
        nm = sb.mcus(w, h)
        inside, at_end = _cuts(w, h)
        oks = [nm, inside, nm, at_end, nm, None if inside is None else max(1, inside - 3)]
        oks = [ok for ok in oks if ok is not None]
        coef = np.stack([_random_frame(rng, w, h) for _ in oks]).astype(np.int16)
        want = np.stack([cb.picture(orc, c, w, h, ok, 0) for c, ok in zip(coef, oks)])
        out[(w, h)] = (coef, np.array(oks, np.uint32), want)
    return out


@pytest.mark.parametrize("w,h", GEOMETRIES)
def test_stage_d_paths(ctx, geometry_batches, w, h):
    coef, oks, want = geometry_batches[(w, h)]
    assert len(coef) <= 8
    got = _reconstruct(ctx, coef, oks, w, h, 0)
    _same(got, want, ["frame %d (nmcu_ok %d of %d)" % (i, ok, sb.mcus(w, h)) for i, ok in enumerate(oks)], "%dx%d" % (w, h))


@pytest.mark.parametrize("entropy", ["auto", "serial"])
def test_whole_segment_from_scans(ctx, pkg, orc, entropy):
    """160x16 as scans: the records form, and -- the serial entropy kernel -- dense lines a round at a time (FrameSel)"""
    import torch
    w, h, n = 160, 16, 8
    rng = np.random.default_rng(0x5CA2)
    coef = np.stack([_random_frame(rng, w, h) for _ in range(n)]).astype(np.int16)
    want = np.stack([cb.picture(orc, c, w, h, sb.mcus(w, h), 0) for c in coef])
    chunks = [sb.assemble(sb.blocks_from_coefficients(c)).chunk for c in coef]
    blob, offs, lens, nbytes = _blob_of(chunks, pad_front=1)
    ctx.set_entropy_mode(pkg.ENTROPY_SERIAL if entropy == "serial" else pkg.ENTROPY_AUTO)
    try:
        d_out = torch.full((n, h, ctx.stride(w)), 0x5A, dtype=torch.uint8, device="cuda:0")
        d_st = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
        ctx.decode_batch_dev(_t(blob), nbytes, _t(offs), _t(lens), n, w, h, 0, d_out, d_st, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert (d_st.cpu().numpy() == 0).all()
        _same(d_out.cpu().numpy(), want, ["frame %d" % i for i in range(n)], "160x16, entropy %s" % entropy)
    finally:
        ctx.set_entropy_mode(pkg.ENTROPY_AUTO)
