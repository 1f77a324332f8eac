"""The reconstruction's two row passes and the entropy stage's mark, on crafted scans, against the oracle, on a real MI355X.

A records frame in which the entropy stage met no AC of ten magnitude bits takes the row pass on paired 16-bit halves
(tests/test_row_dot2_model.py has the arithmetic); a frame with such an AC leaves the entropy stage marked and takes
the general form.  Scans written with tests/scan_builder.py, every byte compared with the oracle's picture:

    160x16  one whole segment        16x16  a short segment, the general stage D        176x32  a whole and a short segment a row

    * every AC position in turn at + 511 and - 511, in a luma and in a chroma block (the largest values the paired
      form must carry, at every step of both tables);
    * blocks with all 63 ACs at +- 511;
    * the same with one AC at +- 512 and at +- 1023, at the step-61 position and at a step-5 position: marked;
    * a DC chain that climbs by 2047 a block until the predictor wraps, both ways, under +- 511 ACs;
    * a marked frame whose scan breaks inside a block;
    * marked and unmarked frames alternating in the batch, which holds frames on both sides of the heavy / light split;
    * both zig-zag tables; 1, 2, 16 and 64 entropy lanes per frame.

The marked-frame count (entropy_stats) equals the frames written with a ten-bit AC, and is 0 for frames of the
synthetic source; the records accessor gives the oracle's coefficients for marked frames as for the others.
"""
import os

import numpy as np
import pytest

import scan_builder as sb
from coef_builder import QUANT
from conftest import SEED
from test_gpu_parity import _blob_of, _t

pytestmark = pytest.mark.gpu

SIZES = ((160, 16), (16, 16), (176, 32))
LANES = (1, 2, 16, 64)
# (64 lanes on a 16x16 frame: every lane has a record or two and rounds them up to eight, 512 slots where the frame's
# record space has 480 -- such a frame goes to the serial kernel whatever it holds, and carries no mark)
CASES = [(w, h, lanes) for w, h in SIZES for lanes in LANES if not ((w, h) == (16, 16) and lanes == 64)]
KNOBS = ("AMVHIP_SYNC_LANES", "AMVHIP_SPLIT", "AMVHIP_LAYOUT")
STEP61, STEP5 = 56, 5          # scan positions of the luma table's largest step and of a step of 5
assert int(np.asarray(QUANT[0]).ravel()[STEP61]) == 61 == int(np.asarray(QUANT[0]).max()) and int(np.asarray(QUANT[0]).ravel()[STEP5]) == 5


def _quiet(rng, coef, b):
    """a block with a few small coefficients"""
    for p in rng.choice(np.arange(1, 64), 3, replace=False):
        coef[b, p] = rng.integers(-20, 21)


def _position_frames(rng, nblk):
    """every AC position at + 511 and - 511 once in a luma and once in a chroma block, alone in its block"""
    pools = ([(p, s) for p in range(1, 64) for s in (511, -511)], [(p, s) for p in range(1, 64) for s in (511, -511)])
    out = []
    while pools[0] or pools[1]:
        coef = np.zeros((nblk, 64), np.int64)
        coef[:, 0] = rng.integers(-200, 201, nblk)
        for b in range(nblk):
            pool = pools[0 if b % 6 < 4 else 1]
            if pool:
                p, s = pool.pop(0)
                coef[b, p] = s
            else:
                _quiet(rng, coef, b)
        out.append(coef)
    return out


def _full_blocks(nblk, k):
    """the blocks that carry all 63 ACs: the first and the last MCU's; of a one-MCU picture block k alone (64 lanes on a
    frame round every lane's records up to eight: a fuller frame would not fit its record space at every lane count)"""
    return [k] if nblk == 6 else list(range(6)) + list(range(nblk - 6, nblk))


def _full_frame(rng, nblk, k=0, big=None):
    """all 63 ACs at +- 511 in _full_blocks (big: at scan position big[0] the value big[1] instead), a DC and one small
    AC in the others"""
    coef = np.zeros((nblk, 64), np.int64)
    coef[:, 0] = rng.integers(-1000, 1001, nblk)
    coef[np.arange(nblk), rng.integers(1, 64, nblk)] = rng.integers(1, 21, nblk)
    for b in _full_blocks(nblk, k):
        coef[b, 1:] = rng.choice(np.array([511, -511]), 63)
        if big:
            coef[b, big[0]] = big[1]
    return coef


def _frames(w, h):
    """[(name, chunk, marked)], marked and unmarked alternating as far as they go"""
    rng = np.random.default_rng(w * 1000 + h)
    nblk = sb.mcus(w, h) * 6
    chunk = lambda coef: sb.assemble(sb.blocks_from_coefficients(coef)).chunk
    plain = [("position frame %d" % i, chunk(c), False) for i, c in enumerate(_position_frames(rng, nblk))]
    plain += [("all 63 at +-511, #%d" % i, chunk(_full_frame(rng, nblk, k)), False) for i, k in enumerate((0, 4))]
    for sign in (1, -1):   # the DC climbs (falls) by 2047 a block of its component, under two +-511 ACs
        blocks = [(sign * 2047, [(0, 511 if b & 1 else -511), (3, -511 if b & 2 else 511)], True) for b in range(nblk)]
        dcs = sb.expected_coefficients(blocks)[:, 0].astype(np.int64)
        if nblk >= 60:     # the luma predictor passes +-32767 and wraps
            assert (sign * dcs).max() > 30000 and (sign * dcs).min() < -30000, (w, h, sign)
        plain.append(("DC chain %+d" % sign, sb.assemble(blocks).chunk, False))
    marked = []
    for pos in (STEP61, STEP5):
        for big in (512, -512, 1023, -1023):
            marked.append(("all 63 at +-511 but %+d at scan %d" % (big, pos), chunk(_full_frame(rng, nblk, 0, (pos, big))), True))
    blocks = sb.blocks_from_coefficients(_full_frame(rng, nblk, 0, (STEP61, 1023)))
    at = sb.mcus(w, h) * 2 // 3 * 6 + 4     # (the Cb block of the MCU two thirds into the frame)
    blocks[at] = (blocks[at][0], blocks[at][1][:7] + ["1" * 17], False)     # no code of any table: the decoder stops there
    marked.append(("marked and damaged in block %d" % at, sb.assemble(blocks).chunk, True))
    # quiet frames until the full ones are heavy: longer than twice the batch's mean chunk (amv_split_kernel), with room
    lens = [len(f[1]) for f in plain + marked]
    while max(lens) < 2.2 * np.mean(lens):
        coef = np.zeros((nblk, 64), np.int64)
        coef[:, 0] = rng.integers(-200, 201, nblk)
        coef[np.arange(nblk), rng.integers(1, 64, nblk)] = rng.integers(1, 21, nblk)
        plain.append(("quiet frame", chunk(coef), False))
        assert len(plain) < 100
        lens.append(len(plain[-1][1]))
    out = []
    for i in range(max(len(plain), len(marked))):
        out += plain[i:i + 1] + marked[i:i + 1]
    return out


@pytest.fixture(scope="module")
def cases(orc):
    """{(w, h): {"names", "chunks", "marked", 0: (pictures, status, oks, coefficients), 1: (pictures, status)}}"""
    out = {}
    for w, h in SIZES:
        fr = _frames(w, h)
        chunks = [f[1] for f in fr]
        c = {"names": [f[0] for f in fr], "chunks": chunks, "marked": np.array([f[2] for f in fr])}
        # every frame fits its record space with every lane count it meets -- each lane rounds its records up to eight, the
        # one-lane kernel writes eight slots per eight symbols in lines of 32 -- so none goes to the serial kernel
        most = max(lanes for cw, ch, lanes in CASES if (cw, ch) == (w, h))
        for name, ch in zip(c["names"], chunks):
            if "damaged" not in name:
                rec, sym = sb.records_of(sb.blocks_from_coefficients(orc.decode_frame(ch, w, h, 0, want_coef=True)[3]))
                assert max(rec + 7 * min(most, rec), sym + 40) <= sb.record_space(len(ch), sb.mcus(w, h) * 6), (w, h, name, rec, sym)
        dec = [orc.decode_frame(ch, w, h, 0, want_coef=True) for ch in chunks]
        c[0] = (np.stack([d[0] for d in dec]), np.array([d[1] for d in dec]), np.array([d[2] for d in dec]), np.stack([d[3] for d in dec]))
        dec = [orc.decode_frame(ch, w, h, 1) for ch in chunks]
        c[1] = (np.stack([d[0] for d in dec]), np.array([d[1] for d in dec]))
        st, oks = c[0][1], c[0][2]
        damaged = [i for i, n in enumerate(c["names"]) if "damaged" in n]
        assert len(damaged) == 1 and st[damaged[0]] != 0 and oks[damaged[0]] == sb.mcus(w, h) * 2 // 3
        assert (np.delete(st, damaged) == 0).all() and (np.delete(oks, damaged) == sb.mcus(w, h)).all() and c["marked"].sum() == 9
        out[(w, h)] = c
    return out


@pytest.fixture(scope="module")
def ctxs(pkg):
    keep = {k: os.environ.get(k) for k in KNOBS}
    made = {}
    try:
        for k in KNOBS:
            os.environ.pop(k, None)
        for lanes in LANES:
            os.environ["AMVHIP_SYNC_LANES"] = str(lanes)
            made[lanes] = pkg.Context(0)
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    yield made
    for c in made.values():
        c.close()


def _decode(c, chunks, w, h, flags):
    import torch
    blob, offs, lens, nbytes = _blob_of(chunks, pad_front=1)
    n = len(chunks)
    d_out = torch.full((n, h, c.stride(w)), 0x5A, dtype=torch.uint8, device="cuda:0")
    d_st = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    c.decode_batch_dev(_t(blob), nbytes, _t(offs), _t(lens), n, w, h, flags, d_out, d_st, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), d_st.cpu().numpy()


def _assert_same(case, got, st, flags, what):
    want, wst = case[flags][0], case[flags][1]
    assert (st == wst).all(), (what, [case["names"][i] for i in np.nonzero(st != wst)[0][:6]])
    bad = np.nonzero((got != want).reshape(len(want), -1).any(1))[0]
    assert bad.size == 0, (what, [case["names"][i] for i in bad[:6]])


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("w,h,lanes", CASES)
def test_both_row_passes_decode_as_the_oracle(ctxs, cases, w, h, flags, lanes):
    c, case = ctxs[lanes], cases[(w, h)]
    got, st = _decode(c, case["chunks"], w, h, flags)
    _assert_same(case, got, st, flags, "%dx%d, zig-zag flag %d, %d lanes" % (w, h, flags, lanes))
    assert c.entropy_stats(False)["handed_to_serial"] == 0
    if lanes == 1:     # a one-lane batch gives its heavy frames sixteen lanes: both kernels write marks in this batch
        split = c.decode_split_stats()
        assert split["heavy"] > 0 and split["light"] > 0, split


@pytest.mark.parametrize("w,h,lanes", CASES)
def test_marked_frames_are_counted(ctxs, cases, w, h, lanes):
    c, case = ctxs[lanes], cases[(w, h)]
    c.entropy_stats(True)
    try:
        got, st = _decode(c, case["chunks"], w, h, 0)
    finally:
        stats = c.entropy_stats(False)
    _assert_same(case, got, st, 0, "%dx%d with gathering on, %d lanes" % (w, h, lanes))
    assert stats["handed_to_serial"] == 0 and stats["frames"] == len(case["chunks"])
    assert stats["big_ac_frames"] == int(case["marked"].sum()), stats


@pytest.mark.parametrize("lanes", LANES)
def test_no_frame_of_the_synthetic_source_is_marked(ctxs, orc, lanes):
    w, h, n = 160, 120, 64
    chunks = [orc.encode_frame(orc.synth_frame(SEED, t, w, h), w, h) for t in range(n)]
    c = ctxs[lanes]
    c.entropy_stats(True)
    try:
        _, st = _decode(c, chunks, w, h, 0)
    finally:
        stats = c.entropy_stats(False)
    assert (st == 0).all()
    assert stats["frames"] == n and stats["big_ac_frames"] == 0 and stats["handed_to_serial"] == 0, stats


@pytest.mark.parametrize("w,h,lanes", CASES)
def test_the_records_accessor_gives_marked_frames_their_lines(ctxs, cases, w, h, lanes):
    import torch
    c, case = ctxs[lanes], cases[(w, h)]
    chunks = case["chunks"]
    n, nblk = len(chunks), sb.mcus(w, h) * 6
    blob, offs, lens, nbytes = _blob_of(chunks, pad_front=1)
    d_coef = torch.full((n, nblk, 64), 77, dtype=torch.int16, device="cuda:0")
    d_st = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    d_ok = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    c.huffman_decode_dev(_t(blob), nbytes, _t(offs), _t(lens), n, w, h, d_coef, d_st, d_ok)
    torch.cuda.synchronize()
    coef, st, ok = d_coef.cpu().numpy(), d_st.cpu().numpy(), d_ok.cpu().numpy()
    _, wst, woks, wcoef = case[0]
    assert (st == wst).all() and (ok == woks).all()
    for i in range(n):
        upto = int(woks[i]) * 6
        assert (coef[i, :upto] == wcoef[i, :upto]).all(), case["names"][i]
