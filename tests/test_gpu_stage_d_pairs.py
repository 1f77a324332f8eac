"""Stage D's byte pairs, the seeded row pass and the loader's hoisted loads, against the oracle, on a real MI355X.

The frames of tests/stage_d_frames.py through amvhip_reconstruct_dev and, as scans, through the whole decode, under
both zig-zag flags, every byte of a pattern-filled buffer compared with the oracle's picture:

    160x16  one whole segment                       160x64  four waves, each with content of its own
    160x24  a whole row above a row of eight lines  16x16   a single MCU
    160x80  five MCU rows: the five-wave kernel     18x10   the 1-3-pixel tail and an odd row pair

Before anything runs on the GPU the expected array is checked: each of the twelve bytes of a patch row, in both rows
of a patch, is somewhere 0 from a negative sum, somewhere 255 from a sum above 255 and somewhere strictly between (the
second pack of a dword writes its high half in place: a place that was only ever tested unclamped would not show a
pack that loses the other half).  One frame of each batch through the accessor is damaged (nmcu_ok inside a segment);
as scans, 160x80 has a frame whose scan breaks inside a segment and a frame that the entropy stage hands to the serial kernel (a run
of FF bytes past the unstuffer's look-back) among record frames: the loader asks memory about a frame once, up front,
and must leave both as they were.
"""
import numpy as np
import pytest

import coef_builder as cb
import scan_builder as sb
import stage_d_frames as sd
from test_gpu_parity import _blob_of, _t
from test_reconstruct_pack_and_paths import _reconstruct, _same

pytestmark = pytest.mark.gpu


def _inside_a_segment(w, h):
    """an nmcu_ok that ends inside a segment (ten MCUs of an MCU row, or what is left of it), as far in as there is one"""
    mcw, nm = (w + 15) // 16, sd.mcus(w, h)
    inside = [m for m in range(1, nm) if (m % mcw) % 10]
    return inside[len(inside) * 2 // 3] if inside else nm


@pytest.fixture(scope="module")
def accessor_cases(orc):
    """{(w, h, flags): (coef, oks, want)}: the whole frames meet the condition, then the last one is damaged"""
    out = {}
    for w, h in sd.SIZES:
        coefs = sd.frames(w, h)
        nm = sd.mcus(w, h)
        for flags in (0, 1):
            whole = sd.assert_covered(orc, coefs, [nm] * len(coefs), w, h, flags)
            oks = np.array([nm] * (len(coefs) - 1) + [_inside_a_segment(w, h)], np.uint32)
            want = whole.copy()
            want[-1] = cb.picture(orc, coefs[-1], w, h, int(oks[-1]), flags)
            out[(w, h, flags)] = (coefs, oks, want)
    return out


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("w,h", sd.SIZES)
def test_reconstruct_accessor(ctx, accessor_cases, w, h, flags):
    coefs, oks, want = accessor_cases[(w, h, flags)]
    assert len(coefs) <= 3
    got = _reconstruct(ctx, coefs, oks, w, h, flags)
    _same(got, want, ["frame %d (nmcu_ok %d of %d)" % (i, ok, sd.mcus(w, h)) for i, ok in enumerate(oks)],
          "%dx%d, zig-zag flag %d" % (w, h, flags))


def _chunks_of(coefs, w, h):
    """the frames as scans; 160x80: the second with a run of ones that is no code in MCU 23 (inside the third row's
    segment), the third with a run of FF bytes in its scan"""
    chunks = [sb.assemble(sb.blocks_from_coefficients(c)).chunk for c in coefs]
    if (w, h) == (160, 80):
        blocks = sb.blocks_from_coefficients(coefs[1])
        blocks[23 * 6 + 1] = (blocks[23 * 6 + 1][0], ["1" * 17], False)
        chunks[1] = sb.assemble(blocks).chunk
        at = len(chunks[2]) // 2
        chunks[2] = chunks[2][:at] + b"\xff" * 40 + chunks[2][at:]               # (invalid: every decoder must agree on what it does)
    return chunks


@pytest.fixture(scope="module")
def scan_cases(orc):
    out = {}
    for w, h in sd.SIZES:
        coefs = sd.frames(w, h)
        chunks = _chunks_of(coefs, w, h)
        for flags in (0, 1):
            sd.assert_covered(orc, coefs, [sd.mcus(w, h)] * len(coefs), w, h, flags)
            dec = [orc.decode_frame(c, w, h, flags) for c in chunks]
            want, st, oks = np.stack([d[0] for d in dec]), np.array([d[1] for d in dec]), [d[2] for d in dec]
            if (w, h) == (160, 80):
                assert st[0] == 0 and oks[0] == 50 and st[1] != 0 and oks[1] == 23 and 0 < oks[2] < 50, (st, oks)
            else:      # what the oracle makes of the scans is what it makes of the coefficients
                assert (st == 0).all() and (want == sd.expected(orc, coefs, oks, w, h, flags)).all()
            out[(w, h, flags)] = (chunks, want, st)
    return out


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("w,h", sd.SIZES)
def test_decode_from_scans(ctx, scan_cases, w, h, flags):
    import torch
    chunks, want, want_st = scan_cases[(w, h, flags)]
    n = len(chunks)
    assert n <= 3
    blob, offs, lens, nbytes = _blob_of(chunks, pad_front=1)
    d_out = torch.full((n, h, ctx.stride(w)), 0x5A, dtype=torch.uint8, device="cuda:0")
    d_st = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    ctx.decode_batch_dev(_t(blob), nbytes, _t(offs), _t(lens), n, w, h, flags, d_out, d_st, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (d_st.cpu().numpy() == want_st).all()
    _same(d_out.cpu().numpy(), want, ["frame %d" % i for i in range(n)], "%dx%d as scans, zig-zag flag %d" % (w, h, flags))
    if (w, h) == (160, 80):   # the frame with the FF run went to the serial kernel, the other two stayed records
        assert ctx.entropy_stats(False)["handed_to_serial"] == 1
