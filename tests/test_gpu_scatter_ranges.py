"""The record reader's range handling (amv_block_load.h) on segments of every length.

A wave asks for its segment's records 768 at a time (three pieces of 256 words), turns the words past the range's end into
fillers in the one piece that holds the end, and on a second or third trip refills only the lanes whose words are inside
the range -- the others keep the trip before's.  The frames here are crafted so that the record ranges of their MCU-row
segments end everywhere: below one piece, inside each of the three, just around 768 and 1 536, inside a second and a third
trip.  Every block of a segment carries the same number m of non-zero ACs (distinct values, so a record that lands in the
wrong place or a stale one that is taken shows), m differing by segment and frame; 176x144 adds rows of two segments (ten
MCUs and one), i.e. ranges with foreign blocks at both ends and every alignment of the block field.  Between the clean
frames sits a frame with 24 bytes of its middle overwritten (pixels after its first error are zero, as the oracle's).

Decoded through amvhip_decode_batch_dev with one lane per frame (the kernel a chip-filling batch gets), 2, 8, 16 and 64
lanes, the default choice and AMVHIP_ENTROPY_SERIAL, in both zig-zag modes, against the oracle's decode of the same chunks; and through
amvhip_huffman_decode_dev (the records expanded to dense lines by the same reader) against the oracle's coefficients.
"""
import os

import numpy as np
import pytest

import scan_builder as sb
from test_gpu_parity import _blob_of, _gpu_decode, _oracle_decode, _t

pytestmark = pytest.mark.gpu


def _frame(w, h, k):
    mcw, mch = (w + 15) // 16, (h + 15) // 16
    nb = mcw * mch * 6
    coef = np.zeros((nb, 64), np.int64)
    blk = np.arange(nb)
    coef[:, 0] = (blk * 7 + k) % 23 - 11
    counts = []
    for row in range(mch):
        for seg0 in range(0, mcw, 10):
            cnt = min(10, mcw - seg0)
            m = (5 * k + 7 * row + 3 * (seg0 // 10)) % 41          # 0 .. 40 non-zero ACs in every block of the segment
            first = (row * mcw + seg0) * 6
            for b in range(first, first + cnt * 6):
                i = np.arange(1, m + 1)
                coef[b, 1:m + 1] = ((b * 5 + i * 3 + k) % 9 + 1) * np.where((b + i) & 1, -1, 1)
            counts.append(cnt * 6 * (m + 1))
    return coef, counts


def _frames(w, h, n):
    coefs, counts = [], []
    for k in range(n):
        c, cn = _frame(w, h, k)
        coefs.append(c)
        counts += cn
    return coefs, counts


def _contexts(pkg):
    keep = os.environ.get("AMVHIP_SYNC_LANES")
    out = {}
    try:
        for lanes in (None, "1", "2", "8", "16", "64"):
            if lanes is None:
                os.environ.pop("AMVHIP_SYNC_LANES", None)
            else:
                os.environ["AMVHIP_SYNC_LANES"] = lanes
            out[lanes] = pkg.Context(0)
    finally:
        if keep is None:
            os.environ.pop("AMVHIP_SYNC_LANES", None)
        else:
            os.environ["AMVHIP_SYNC_LANES"] = keep
    return out


@pytest.mark.parametrize("w,h,n", [(160, 120, 41), (176, 144, 41)])
def test_segments_of_every_record_count(pkg, orc, w, h, n):
    import torch
    coefs, counts = _frames(w, h, n)
    # symbols that carry a value, per segment (a lower bound of its record range, which also holds fillers): the ranges
    # end below one piece, inside every piece of the first trip and inside a second and a third trip
    counts = np.array(counts)
    for lo, hi in ((1, 256), (256, 512), (512, 768), (768, 1024), (1024, 1536), (1536, 1792), (1792, 2304), (2304, 2461)):
        assert ((counts >= lo) & (counts < hi)).any(), (lo, hi)
    chunks = [sb.assemble(sb.blocks_from_coefficients(c.astype(np.int16))).chunk for c in coefs]
    cut = n // 2
    bad = bytearray(chunks[cut])                                     # a damaged frame between clean ones
    bad[len(bad) // 2: len(bad) // 2 + 24] = bytes(np.random.default_rng(0).integers(0, 255, 24).astype(np.uint8))
    chunks.insert(cut, bytes(bad))
    want = {f: _oracle_decode(orc, chunks, w, h, f) for f in (0, 1)}
    assert want[0][1][cut] != 0 and (np.delete(want[0][1], cut) == 0).all()
    ref = [orc.decode_frame(c, w, h, 0, want_coef=True) for c in chunks]
    assert 0 < ref[cut][2] < orc.nmcu(w, h)                          # its first error lies inside the picture
    ctxs = _contexts(pkg)
    try:
        for lanes, c in list(ctxs.items()) + [("serial", ctxs[None])]:
            c.set_entropy_mode(pkg.ENTROPY_SERIAL if lanes == "serial" else pkg.ENTROPY_AUTO)
            for flags in (0, 1):
                got, st = _gpu_decode(c, chunks, w, h, flags, pad_front=1)
                assert (st == want[flags][1]).all(), (lanes, flags, st, want[flags][1])
                bad = [i for i in range(len(chunks)) if not (got[i] == want[flags][0][i]).all()]
                assert not bad, (lanes, flags, bad)
                if lanes != "serial":
                    # the clean frames stayed records (a frame the entropy kernels hand to the serial one goes round the
                    # reader under test); the damaged one may be handed back
                    handed = c.entropy_stats(False)["handed_to_serial"]
                    print("lanes %s flags %d: handed_to_serial %d" % (lanes, flags, handed))
                    assert handed <= 1, (lanes, flags, handed)
            # the same records as dense lines
            blob, offs, lens, nbytes = _blob_of(chunks, 1)
            nblk = orc.nmcu(w, h) * 6
            d_coef = torch.full((len(chunks), nblk, 64), 77, dtype=torch.int16, device="cuda:0")
            d_st = torch.full((len(chunks),), -1, dtype=torch.int32, device="cuda:0")
            d_ok = torch.full((len(chunks),), -1, dtype=torch.int32, device="cuda:0")
            c.huffman_decode_dev(_t(blob), nbytes, _t(offs), _t(lens), len(chunks), w, h, d_coef, d_st, d_ok)
            torch.cuda.synchronize()
            lines, ok = d_coef.cpu().numpy(), d_ok.cpu().numpy()
            for i, r in enumerate(ref):
                assert ok[i] == r[2], (lanes, i)
                upto = int(r[2]) * 6
                assert (lines[i, :upto] == r[3][:upto]).all(), (lanes, i)
    finally:
        for c in ctxs.values():
            c.set_entropy_mode(pkg.ENTROPY_AUTO)
            c.close()
