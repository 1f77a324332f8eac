"""The arithmetic the reconstruction's record scatter and its row/column hand-over rely on, as NumPy models (no GPU).

`amv_block_load.h` turns a record word (index | block field << 6 | filler << 15 | value << 16, the field counting from
the frame's end modulo 64) into an LDS address with: granule bits XOR-ed with the field's low three bits, ONE
add-and-shift, one mask, one unsigned compare.  The model below is that sequence; it is held against the definition
(block in segment = (field - first field) mod 64; taken iff no filler and the block was decoded; byte offset 2 * index
with its 16-byte granule XOR-ed by what the block's lane reads with) for every word, every first field and every count
of decoded blocks, and the lane-side gather is shown to return dense scan-order lines.

`amv_reconstruct.hip` hands rows 0 and 4 to the column pass masked instead of shifted down and up again:
((s >> 8) << 8) == s & ~255 and (((s + 128) >> 8) << 8) + 8192 == (s + 128 + 8192) & ~255 modulo 2^32.
"""
import os
import re

import numpy as np

U32 = np.uint32


def _header_constants():
    """the scatter's named constants, read out of amv_block_load.h: the model below runs on the header's numbers"""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "amv-codec-tools_amd", "csrc", "amv_block_load.h")
    text = open(path).read()
    found = {}
    for name in ("kScatterSwizzleMask", "kScatterAddressMask", "kScatterFieldShift"):
        m = re.search(r"constexpr uint32_t %s = (0x[0-9a-fA-F]+|\d+)u;" % name, text)
        assert m, name
        found[name] = int(m.group(1), 0)
    return found["kScatterSwizzleMask"], found["kScatterAddressMask"], found["kScatterFieldShift"], 1   # (the add-and-shift doubles)


SWZ_MASK, AT_MASK, FIRST_SHIFT, ADD_SHL = _header_constants()


def _scatter_address(w, first_field, blocks_ok):
    """the kernel's sequence, 32-bit: (address, taken)"""
    w = w.astype(U32)
    first6 = U32((64 - first_field) << FIRST_SHIFT)
    q = w ^ ((w >> U32(3)) & U32(SWZ_MASK))
    t = ((q + first6) << U32(ADD_SHL)).astype(U32)
    at = t & U32(AT_MASK)
    return at, at < U32(blocks_ok << 7)


def _all_words():
    index = np.arange(64, dtype=U32)
    field = np.arange(64, dtype=U32)
    filler = np.array([0, 1], dtype=U32)
    value = np.array([0x0000, 0x0001, 0x7FFF, 0x8000, 0xFFFF, 0x5A5A], dtype=U32)   # the high half must never matter
    i, f, d, v = np.meshgrid(index, field, filler, value, indexing="ij")
    return (i | (f << U32(6)) | (d << U32(15)) | (v << U32(16))).ravel(), i.ravel(), f.ravel(), d.ravel()


def test_scatter_address_is_the_definition():
    w, index, field, filler = _all_words()
    for first_field in range(64):
        bseg = (field - U32(first_field)) & U32(63)
        want_at = bseg * U32(128) + ((index * U32(2)) ^ ((field & U32(7)) << U32(4)))
        for blocks_ok in (0, 1, 5, 6, 59, 60):
            at, taken = _scatter_address(w, first_field, blocks_ok)
            want_taken = (filler == 0) & (bseg < blocks_ok)
            assert (taken == want_taken).all(), (first_field, blocks_ok)
            assert (at[taken] == want_at[taken]).all(), (first_field, blocks_ok)
            assert (at[taken] < 60 * 128).all()


def test_the_filler_word_is_rejected_whatever_the_segment():
    for first_field in range(64):
        _, taken = _scatter_address(np.array([0x8000], dtype=U32), first_field, 60)
        assert not taken[0]


def test_gather_returns_dense_scan_order_lines():
    rng = np.random.default_rng(7)
    for first_field in (0, 3, 4, 37, 63):
        nb = 60
        coef = rng.integers(-1023, 1024, size=(nb, 64)).astype(np.int16)
        coef[rng.random((nb, 64)) < 0.8] = 0
        img = np.zeros(nb * 64 + 64, np.int16)   # + the spare slots
        b, i = np.nonzero(coef)
        w = (i.astype(U32) | (((b.astype(U32) + U32(first_field)) & U32(63)) << U32(6))
             | (coef[b, i].astype(np.uint16).astype(U32) << U32(16)))
        # four foreign blocks on either side and fillers, as a range's ends carry them
        foreign = np.array([(5 | (((first_field - 1) & 63) << 6) | (77 << 16)), (9 | (((first_field + 60) & 63) << 6) | (78 << 16)),
                            0x8000], dtype=U32)
        w = np.concatenate([foreign, w, foreign])
        at, taken = _scatter_address(w, first_field, nb)
        assert taken.sum() == len(b)
        img[at[taken] >> 1] = (w[taken] >> U32(16)).astype(np.uint16).view(np.int16)
        for lane in range(nb):
            swz = (lane + first_field) & 7
            line = np.concatenate([img[lane * 64 + ((g ^ swz) * 8): lane * 64 + ((g ^ swz) * 8) + 8] for g in range(8)])
            assert (line == coef[lane]).all(), (first_field, lane)


def test_rows_0_and_4_masked_instead_of_shifted():
    rng = np.random.default_rng(11)
    s = np.concatenate([rng.integers(-2**31, 2**31, size=200000, dtype=np.int64),
                        np.array([-2**31, -2**31 + 1, -8321, -8320, -257, -256, -255, -129, -128, -1, 0, 1, 127, 128, 255, 256,
                                  2**31 - 8321, 2**31 - 8320, 2**31 - 129, 2**31 - 128, 2**31 - 1], dtype=np.int64)])
    wrap = lambda x: ((x + 2**31) % 2**32 - 2**31)   # int32 arithmetic with wrap, as the kernels are compiled
    # row 4: the row result (s >> 8), times 256 in the column pass
    assert (wrap((s >> 8) * 256) == (s & ~255)).all()
    # row 0: s is the row's sum before its bias; (s + 128) >> 8, then * 256 + 8192 in the column pass
    row = wrap(s + 128)
    assert (wrap((row >> 8) * 256 + 8192) == (wrap(row + 8192) & ~255)).all()
