"""amvhip_entropy_trace for the one-lane-per-frame entropy kernel (where the waves of a launch
that fills the chip run, and when they end).  With gathering on, a decode through amv_huffman_fast_kernel leaves one line per
task of 64 frames; the frames are the same bytes whether gathering is on or not."""
import os

import numpy as np
import pytest

from test_gpu_parity import _gpu_decode, _oracle_decode, _synth_chunks

pytestmark = pytest.mark.gpu


def _one_lane_context(pkg):
    old = os.environ.get("AMVHIP_SYNC_LANES")
    os.environ["AMVHIP_SYNC_LANES"] = "1"
    try:
        return pkg.Context(0)
    finally:
        if old is None:
            os.environ.pop("AMVHIP_SYNC_LANES", None)
        else:
            os.environ["AMVHIP_SYNC_LANES"] = old


def test_one_lane_trace_has_a_line_per_task(pkg, orc):
    """327 frames of 48x32 (five full tasks and a ragged one of seven frames; one chunk cut short, one damaged): a line per
    task -- begin before end on the constant-rate clock, shader clocks that fit the duration at any plausible clock rate,
    whole line groups of strides within what 36 blocks can need, the workgroup and wave of a six-workgroup launch of four
    waves, one lane per frame -- and gathering changes no byte: statuses are the oracle's, and so are the sound frames"""
    w, h, n = 48, 32, 327
    blocks = 3 * 2 * 6
    base = _synth_chunks(orc, 40, w, h)
    chunks = [base[i % 40] for i in range(n)]
    chunks[70] = chunks[70][: len(chunks[70]) // 2]
    bad = bytearray(chunks[200])
    bad[len(bad) // 3] ^= 0x10
    chunks[200] = bytes(bad)
    want, want_st = _oracle_decode(orc, chunks, w, h)
    c = _one_lane_context(pkg)
    try:
        plain, st0 = _gpu_decode(c, chunks, w, h)
        c.entropy_stats(True)
        traced, st1 = _gpu_decode(c, chunks, w, h)
        tr = c.entropy_trace(64)
        c.entropy_stats(False)
        assert (st0 == st1).all() and (plain == traced).all()
        assert (st1 == want_st).all()
        ok = want_st == 0
        assert ok.sum() >= n - 2 and (traced[ok] == want[ok]).all()
        tasks = (n + 63) // 64
        assert (tr[:tasks, 1] != 0).all() and (tr[tasks:] == 0).all()
        tr = tr[:tasks]
        dur = (tr[:, 1] - tr[:, 0]).astype(np.int64)                            # 100 MHz ticks
        assert (dur > 0).all() and (dur < 100 * 1000 * 50).all()                # under 50 ms each
        clocks = tr[:, 2].astype(np.int64)
        assert (clocks > 0).all() and (clocks < dur * 40).all()                 # a shader clock under 4 GHz
        strides = tr[:, 3].astype(np.int64)
        # eight symbols a stride, at least a DC and an end-of-block symbol per block, at most 64 symbols; lines leave every fourth
        assert (strides % 4 == 0).all() and (strides >= blocks * 2 // 8).all() and (strides <= blocks * 64 // 8 + 4).all()
        assert (tr[:, 4] == 0).all() and (tr[:, 6] == 0).all()
        assert ((tr[:, 7] & np.uint64(0xffff)) == 1).all()
        assert (((tr[:, 7] >> np.uint64(16)) & np.uint64(0xffff)) < 4).all()    # workgroups of four waves for so few tasks
        assert ((tr[:, 7] >> np.uint64(32)) < tasks).all()                      # a workgroup per task at most
    finally:
        c.close()
