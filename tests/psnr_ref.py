"""The `-psnr` figures restated for the tests: what the encoder's d_sse must be for a chunk it returned, built from the
oracle library's exported functions only.

A chunk's levels come back through amvo_entropy_blocks (DC absolute), the tables of amv_tables.h (the tests' own copy of
them, tests/coef_builder.py) are applied --
v[natural] = (int16)(level[scan] * Q[scan]), + 1024 on the DC -- and amvo_simple_idct_put writes each block into a padded
canvas in bitstream coordinates (canvas row k is picture row height - 1 - k: the encoder's placement, bottom-up).  The
canvas is cropped to the visible samples (w x h luma, w/2 x h/2 chroma), turned the right way up, and the squares are summed
in numpy.  With the Q60 tables in the place of the encoder's the same routine is the FFmpeg-compat decoder
(test_psnr_ref.py pins the placement so)."""
import os
import re

import numpy as np

import coef_builder as cb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TABLES = {}


def tables():
    """the tables the restatement applies, under amv_tables.h's names: the tests' own copy of the wire format's data
    (tests/coef_builder.py: amvlib's quantiser steps AmvJpeg.c:30-61, sp5x.h's Q60 tables, the standard zig-zag), not the
    product's header -- test_psnr_ref.py checks that the header says the same"""
    if not _TABLES:
        _TABLES.update({"kQuantLuma": cb.QUANT[0], "kQuantChroma": cb.QUANT[1], "kQ60Luma": cb.Q60[0], "kQ60Chroma": cb.Q60[1],
                        "kScanOfNatural": np.asarray(cb.SCAN_OF_NATURAL, np.int64)})
    return _TABLES


def header_tables():
    """the same five tables as amv-codec-tools_amd/csrc/amv_tables.h states them"""
    text = open(os.path.join(ROOT, "amv-codec-tools_amd", "csrc", "amv_tables.h")).read()
    out = {}
    for name in ("kQuantLuma", "kQuantChroma", "kQ60Luma", "kQ60Chroma", "kScanOfNatural"):
        body = re.search(r"%s\[64\] = \{([^}]*)\}" % name, text).group(1)
        out[name] = np.array([int(x) for x in body.replace("\n", " ").split(",")], np.int64)
    return out


def canvases(orc, chunk, w, h, q60=False, unclipped=False):
    """the chunk's blocks through dequantisation and simple_idct_put -> canvases (Y [mch*16, mcw*16], Cb, Cr [mch*8, mcw*8])
    uint8 in bitstream coordinates; unclipped: (lowest, highest) value of simple_idct before the clip instead"""
    t = tables()
    q = (t["kQ60Luma"], t["kQ60Chroma"]) if q60 else (t["kQuantLuma"], t["kQuantChroma"])
    scan = t["kScanOfNatural"]
    mcw, mch = (w + 15) // 16, (h + 15) // 16
    nblocks = mcw * mch * 6
    coef, status = orc.entropy_blocks(chunk, nblocks)
    assert status == 0 and len(coef) == nblocks, "the chunk does not decode: status %d after %d blocks" % (status, len(coef))
    L = orc.lib()
    Y = np.zeros((mch * 16, mcw * 16), np.uint8)
    C = [np.zeros((mch * 8, mcw * 8), np.uint8) for _ in range(2)]
    lo, hi = 1 << 20, -(1 << 20)
    for b in range(nblocks):
        mcu, k6 = divmod(b, 6)
        my, mx = divmod(mcu, mcw)
        level = coef[b].astype(np.int64)
        v = level[scan] * q[k6 >= 4][scan]
        v[0] += 1024
        blk = np.ascontiguousarray(v.astype(np.int16))                 # DCTELEM: the store wraps
        if unclipped:
            L.amvo_simple_idct(blk.ctypes.data)
            lo, hi = min(lo, int(blk.min())), max(hi, int(blk.max()))
            continue
        if k6 < 4:
            plane, r, c = Y, my * 16 + (k6 >> 1) * 8, mx * 16 + (k6 & 1) * 8
        else:
            plane, r, c = C[k6 - 4], my * 8, mx * 8
        L.amvo_simple_idct_put(plane.ctypes.data + r * plane.shape[1] + c, plane.shape[1], blk.ctypes.data)
    return (lo, hi) if unclipped else (Y, C[0], C[1])


def reconstruct(orc, chunk, w, h, q60=False):
    """-> the visible planes (Y [h, w], Cb, Cr [h/2, w/2]) the right way up"""
    Y, Cb, Cr = canvases(orc, chunk, w, h, q60)
    cw, ch = w // 2, h // 2
    return Y[:h, :w][::-1], Cb[:ch, :cw][::-1], Cr[:ch, :cw][::-1]


def sse(orc, chunk, planes, w, h):
    """[3] squared error of the handed picture (Y, Cb, Cr; any row pitch, the first w or w/2 columns count) against the
    reconstruction of the chunk's levels"""
    rec = reconstruct(orc, chunk, w, h)
    out = []
    for p, (src, got) in enumerate(zip(planes, rec)):
        rows, cols = got.shape
        d = np.asarray(src)[:rows, :cols].astype(np.int64) - got.astype(np.int64)
        out.append(int((d * d).sum()))
    return out


def sse_of_stream(orc, chunks, frames, w, h):
    """[n, 3] uint64 for a stream's chunks and the pictures they were made of"""
    return np.array([sse(orc, c, f, w, h) for c, f in zip(chunks, frames)], np.uint64).reshape(len(chunks), 3)
