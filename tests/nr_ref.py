"""The reference's -nr noise reduction restated in Python (a helper of the tests, imported as scan_builder is).

    update_noise_reduction   libavcodec/mpegvideo.c:861-876        at the start of every frame
    denoise_dct_c            libavcodec/mpegvideo_enc.c:2937-2959  every block, between fdct and quantiser

State per stream: 64 sums of coefficient magnitudes (index = the fdct output's row-major order; the six blocks of an MCU
share the array) and the count of blocks, here one int64 array of 65 (the layout of the product's `d_state`).  Two
quantiser modes share the two functions:

    reference mode   the reference's amv encoder as it is: un-shifted samples, ff_mpeg1_default_intra_matrix at -qscale 8
                     (the matrix itself, mpegvideo_enc.c:2866-2877), DC (b0 + 32) / 64 against a predictor of 128, AC
                     |level * qmat| >> 22 with the sign (dct_quantize_c :3663-3717, bias 0), the picture flipped
                     (mjpegenc.c:454-472).  tests/golden/ref_nr.json pins it to the reference's own ffmpeg.
    product mode     what the product codes: samples - 128, so the fdct outputs are the reference's except at position 0,
                     where reference DC = ours + 8192 exactly; D = x + 8192 is summed and denoised, x' = D' - 8192 goes on
                     into the oracle's amvo_quantize_block.  Blocks are taken as the oracle's encode_planes takes them
                     (bottom-up, edge samples repeated into the padding blocks).

Both entropy-code with scan_builder.  Python ints do not wrap: the model is the reference wherever the reference's int
arithmetic does not wrap, which is what the product's argument bound (amv_nr_plan.h) guarantees.

frame_start, denoise_blocks and encode_stream take `faults` (faults_of): named wrong implementations, none by default, with
which tests/test_nr_builder.py proves that the crafted corpus of tests/nr_builder.py would notice each of them.
"""
import os
import sys

import numpy as np

import scan_builder as sb

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
import amv_oracle_py as orc  # noqa: E402

DC_SHIFT = 8192                      # 64 samples x 128 x 8 (the fdct's DC gain) / 64
HALVE_ABOVE = 1 << 16
# the MPEG-1 default intra matrix (ISO/IEC 11172-2, 2.4.3.2), row-major
MPEG1_INTRA = np.array([8, 16, 19, 22, 26, 27, 29, 34, 16, 16, 22, 24, 27, 29, 34, 37, 19, 22, 26, 27, 29, 34, 34, 38,
                        22, 22, 26, 27, 29, 34, 37, 40, 22, 26, 27, 29, 32, 35, 40, 48, 26, 27, 29, 32, 35, 40, 48, 58,
                        26, 27, 29, 34, 38, 46, 56, 69, 27, 29, 35, 38, 46, 56, 69, 83], np.int64)


def _zigzag():
    order = sorted(range(64), key=lambda i: (i // 8 + i % 8, (i // 8) if (i // 8 + i % 8) & 1 else (i % 8)))
    return np.array(order)           # scan position -> row-major index


ZIGZAG = _zigzag()


def new_state():
    return np.zeros(65, np.int64)


def _cdiv(a, b):
    """C's int division (towards zero) on int64 arrays, b != 0"""
    q = np.abs(a) // np.abs(b)
    return np.where((a < 0) != (b < 0), -q, q)


FAULTS = ("signed_offsets", "swapped_pair", "untransposed", "dead_zone_plus_1", "dead_zone_minus_1", "sign_lost", "dc_unshifted",
          "dc_unclamped", "dc_sum_unshifted", "no_truncation", "no_halving", "halve_at_65536", "halve_rounds_up", "padding_not_summed",
          "magnitude_pair_swapped")


def faults_of(faults):
    """Named faults: each one wrong implementation a kernel could plausibly be, for proving that a corpus would notice it
    (tests/nr_builder.py).  `faults` is a collection of names, or a dict name -> where: dead_zone_plus_1 / dead_zone_minus_1
    take (position, sign, component) -- row-major position, sign +1 / -1 of the coefficient, component 0 luma / 1 chroma --
    to confine the fault to that one; None is everywhere.  -> dict.

      signed_offsets      an offset of 32768 or more is taken as offset - 65536 (the halves of a word read as signed)
      swapped_pair        the two offsets of one 32-bit word, as the column pass consumes them (entry c * 8 + r: rows r
                          and r ^ 1 of a column), change places
      untransposed        position r * 8 + c takes the offset of c * 8 + r
      dead_zone_plus_1    abs(x) - offset + 1 (AC positions)
      dead_zone_minus_1   abs(x) - offset - 1 (AC positions)
      sign_lost           a negative output comes back positive
      dc_unshifted        the DC is denoised as x, not as x + 8192
      dc_unclamped        D - offset is not held at 0
      dc_sum_unshifted    the DC sum takes abs(x)
      no_truncation       the offset is not stored as uint16_t (truncate=False)
      no_halving          no halving (halve=False)
      halve_at_65536      halves at count >= 65536
      halve_rounds_up     halves with (v + 1) >> 1
      padding_not_summed  blocks wholly outside the picture do not enter sums or count
      magnitude_pair_swapped  the fault chosen in how the sums kernel packs its 16-bit magnitudes: the two magnitudes of a
                          32-bit word of the block's line (positions r * 8 + c and r * 8 + (c ^ 1)) change places on the way
                          to the sums -- pack16's arguments the wrong way round, or the halves read in the other byte order
    """
    f = dict(faults) if isinstance(faults, dict) else {k: None for k in faults}
    assert set(f) <= set(FAULTS), sorted(set(f) - set(FAULTS))
    return f


_I = np.arange(64)
_TRANSPOSED = (_I % 8) * 8 + _I // 8
_PAIR_IN_COLUMN = ((_I // 8) ^ 1) * 8 + _I % 8
_PAIR_IN_ROW = _I ^ 1


def frame_start(state, nr, truncate=True, halve=True, faults=()):
    """update_noise_reduction: halve sums and count when the count is above 65536, then the 64 offsets.  state changes in
    place; truncate=False leaves out the uint16_t store, halve=False the halving (what the fixtures' maker tells apart;
    the faults no_truncation and no_halving are the same switches)"""
    f = faults_of(faults)
    truncate, halve = truncate and "no_truncation" not in f, halve and "no_halving" not in f
    if halve and (state[64] >= HALVE_ABOVE if "halve_at_65536" in f else state[64] > HALVE_ABOVE):
        if "halve_rounds_up" in f:
            state[:] += 1
        state[:] >>= 1
    off = _cdiv(nr * state[64] + _cdiv(state[:64], np.int64(2)), state[:64] + 1)
    return off & 0xFFFF if truncate else off


def denoise_blocks(state, offsets, coef, dc_shift=0, faults=(), outside=None):
    """denoise_dct_c over the blocks of one frame (coef [B, 64] fdct outputs, row-major, MCU order; position 0 is the
    reference's when dc_shift is added): state changes in place, the denoised outputs come back.  outside: [B] bool, the
    blocks wholly outside the picture (the fault padding_not_summed alone asks for it)"""
    f = faults_of(faults)
    c = np.asarray(coef, np.int64).copy()
    c[:, 0] += dc_shift
    mag = np.abs(c)
    summed = mag.copy()
    if "dc_sum_unshifted" in f:
        summed[:, 0] = np.abs(c[:, 0] - dc_shift)
    if "magnitude_pair_swapped" in f:
        summed = summed[:, _PAIR_IN_ROW]
    if "padding_not_summed" in f:
        summed = summed[~np.asarray(outside, bool)]
    state[:64] += summed.sum(axis=0)
    state[64] += summed.shape[0]
    offsets = np.asarray(offsets, np.int64)
    if "signed_offsets" in f:
        offsets = np.where(offsets >= 32768, offsets - 65536, offsets)
    if "swapped_pair" in f:
        offsets = offsets[_PAIR_IN_COLUMN]
    if "untransposed" in f:
        offsets = offsets[_TRANSPOSED]
    kept = mag - offsets[None, :]
    for name, step in (("dead_zone_plus_1", 1), ("dead_zone_minus_1", -1)):
        if name in f:
            where = np.ones(c.shape, bool)
            if f[name] is not None:
                pos, sign, comp = f[name]
                where[:] = False
                where[:, pos] = (np.sign(c[:, pos]) == sign) & ((np.arange(c.shape[0]) % 6 >= 4) == bool(comp))
            where[:, 0] = False
            kept = kept + step * where
    out = np.sign(c) * np.maximum(kept, 0)
    if "sign_lost" in f:
        out = np.abs(out)
    if "dc_unclamped" in f:
        out[:, 0] = kept[:, 0]
    if "dc_unshifted" in f:
        x = c[:, 0] - dc_shift
        out[:, 0] = np.sign(x) * np.maximum(np.abs(x) - offsets[0], 0) + dc_shift
    out[:, 0] -= dc_shift
    return out


# ---- the transform ---------------------------------------------------------------------------------------------------------

def _s16(x):
    return ((x + 32768) & 0xFFFF) - 32768


def _fdct_pass(d, shift, first):
    """one pass of jfdctint.c over the last axis of d (int64), outputs truncated to DCTELEM"""
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    half = 1 << (shift - 1)
    o = np.empty_like(d)
    if first:
        o[..., 0], o[..., 4] = (t10 + t11) << 4, (t10 - t11) << 4
    else:
        o[..., 0], o[..., 4] = (t10 + t11 + 8) >> 4, (t10 - t11 + 8) >> 4
    z1 = (t12 + t13) * 4433
    o[..., 2] = (z1 + t13 * 6270 + half) >> shift
    o[..., 6] = (z1 - t12 * 15137 + half) >> shift
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[..., 7] = (t4 + z1 + z3 + half) >> shift
    o[..., 5] = (t5 + z2 + z4 + half) >> shift
    o[..., 3] = (t6 + z2 + z3 + half) >> shift
    o[..., 1] = (t7 + z1 + z4 + half) >> shift
    return _s16(o)


def fdct(blocks):
    """ff_jpeg_fdct_islow over [B, 64] sample blocks (row-major) -> [B, 64] int64; tests pin it to amvo_fdct_islow"""
    d = np.asarray(blocks, np.int64).reshape(-1, 8, 8)
    d = _fdct_pass(d, 13 - 4, True)
    d = _fdct_pass(d.transpose(0, 2, 1), 13 + 4, False).transpose(0, 2, 1)
    return d.reshape(-1, 64)


def frame_blocks(y, cb, cr, w, h, shift):
    """the blocks of one YUVJ420P picture as the oracle's encode_planes takes them: MCU order, Y0 Y1 Y2 Y3 Cb Cr, the
    picture bottom-up, rows and columns beyond it repeating the nearest edge sample -> [blocks, 64] samples - shift"""
    mcw, mch = (w + 15) // 16, (h + 15) // 16

    def padded(p, pw, ph, W, H):
        p = np.asarray(p, np.int64)[:ph, :pw][::-1]
        rows = np.minimum(np.arange(H), ph - 1)
        cols = np.minimum(np.arange(W), pw - 1)
        return p[rows][:, cols] - shift

    Y = padded(y, w, h, mcw * 16, mch * 16).reshape(mch, 2, 8, mcw, 2, 8).transpose(0, 3, 1, 4, 2, 5)      # my, mx, by, bx, i, j
    C = [padded(p, w // 2, h // 2, mcw * 8, mch * 8).reshape(mch, 8, mcw, 8).transpose(0, 2, 1, 3) for p in (cb, cr)]
    out = np.empty((mch, mcw, 6, 64), np.int64)
    out[:, :, :4] = Y.reshape(mch, mcw, 4, 64)
    out[:, :, 4] = C[0].reshape(mch, mcw, 64)
    out[:, :, 5] = C[1].reshape(mch, mcw, 64)
    return out.reshape(-1, 64)


def outside_blocks(w, h):
    """[blocks] bool, MCU order: the blocks wholly outside the picture (every sample a repeated edge sample)"""
    mcw, mch = (w + 15) // 16, (h + 15) // 16
    out = np.zeros((mch, mcw, 6), bool)
    for my in range(mch):
        for mx in range(mcw):
            for k in range(4):
                out[my, mx, k] = my * 16 + (k >> 1) * 8 >= h or mx * 16 + (k & 1) * 8 >= w
            out[my, mx, 4:] = my * 8 >= h // 2 or mx * 8 >= w // 2
    return out.reshape(-1)


# ---- the two encoders ------------------------------------------------------------------------------------------------------

def _chunk(zz):
    return sb.assemble(sb.blocks_from_coefficients(zz)).chunk


def quantize_reference(coef):
    """dct_quantize_c for the amv encoder at -qscale 8 -> zig-zag lines, the DC less the predictor's start of 128"""
    coef = np.asarray(coef, np.int64)
    qmat = (1 << 22) // (8 * MPEG1_INTRA)
    level = coef * qmat[None, :]
    q = np.sign(level) * (np.abs(level) >> 22)
    q[:, 0] = (coef[:, 0] + 32) // 64 - 128          # block[0] is not negative (:3674)
    return q[:, ZIGZAG]


def quantize_product(coef, qbias=0):
    """the oracle's amvo_quantize_block, block by block -> zig-zag lines"""
    L = orc.lib()
    coef = np.ascontiguousarray(coef, np.int16)
    zz = np.zeros_like(coef)
    for b in range(coef.shape[0]):
        L.amvo_quantize_block(coef[b].ctypes.data, 0 if b % 6 < 4 else 1, qbias, zz[b].ctypes.data)
    return zz


def _int16(coef):
    """what the quantiser is handed: DCTELEM (only a faulty model's outputs ever leave it)"""
    return _s16(np.asarray(coef, np.int64))


def encode_stream(frames, w, h, nr, state=None, mode="product", qbias=0, truncate=True, halve=True, want_coef=False, faults=()):
    """frames: [(y, cb, cr)] planes of 2-D uint8 -> the chunks (or, want_coef, the zig-zag lines per frame); state (65
    int64, new_state() when None) changes in place.  nr = 0 leaves it alone, as the reference allocates nothing then.
    faults: see faults_of; none by default"""
    if state is None:
        state = new_state()
    ref = mode == "reference"
    outside = outside_blocks(w, h) if "padding_not_summed" in faults_of(faults) else None
    out = []
    for y, cb, cr in frames:
        coef = fdct(frame_blocks(y, cb, cr, w, h, 0 if ref else 128))
        if nr:
            offsets = frame_start(state, nr, truncate, halve, faults)
            coef = denoise_blocks(state, offsets, coef, 0 if ref else DC_SHIFT, faults, outside)
            if faults:
                coef = _int16(coef)
        zz = quantize_reference(coef) if ref else quantize_product(coef, qbias)
        out.append(zz if want_coef else _chunk(zz))
    return out


# ---- seeded inputs (the fixtures' maker and the tests make the same pictures) ------------------------------------------------

def picture(w, h, kind, seed):
    """(y, cb, cr) uint8: "ramp" = ramps + noise of +-12, "flat" = 128 everywhere, "texture" = a coarse random pattern +
    noise, "noise" = full-range noise"""
    rng = np.random.default_rng(seed)
    cw, ch = w // 2, h // 2

    def plane(pw, ph, k):
        yy, xx = np.mgrid[:ph, :pw]
        if kind == "flat":
            return np.full((ph, pw), 128, np.uint8)
        if kind == "noise":
            return rng.integers(0, 256, (ph, pw)).astype(np.uint8)
        if kind == "ramp":
            base = (xx * (3 + k) + yy * (5 - k) + 40 * k) % 256
            return np.clip(base + rng.integers(-12, 13, (ph, pw)), 0, 255).astype(np.uint8)
        coarse = rng.integers(0, 256, ((ph + 3) // 4, (pw + 3) // 4))
        base = np.kron(coarse, np.ones((4, 4), np.int64))[:ph, :pw]
        return np.clip(base + rng.integers(-20, 21, (ph, pw)), 0, 255).astype(np.uint8)

    return plane(w, h, 0), plane(cw, ch, 1), plane(cw, ch, 2)


def stream(w, h, kinds, seed):
    return [picture(w, h, k, seed + i) for i, k in enumerate(kinds)]


def raw_bytes(frames):
    return b"".join(p.tobytes() for f in frames for p in f)


def split_chunks(data):
    """a rawvideo file of amv chunks -> the chunks (FF D8 ... FF D9; inside a scan every FF is followed by 00)"""
    out, p = [], 0
    while p < len(data):
        assert data[p:p + 2] == b"\xff\xd8", "no SOI at %d" % p
        q = data.index(b"\xff\xd9", p + 2) + 2
        out.append(data[p:q])
        p = q
    return out


FNV_BASIS, FNV_PRIME = 0xCBF29CE484222325, 0x100000001B3


def fnv1a64(data, h=FNV_BASIS):
    return int(orc.lib().amvo_fnv1a64(h, bytes(data), len(data)))
