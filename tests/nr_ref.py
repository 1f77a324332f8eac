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


def frame_start(state, nr, truncate=True, halve=True):
    """update_noise_reduction: halve sums and count when the count is above 65536, then the 64 offsets.  state changes in
    place; truncate=False leaves out the uint16_t store, halve=False the halving (what the fixtures' maker tells apart)"""
    if halve and state[64] > HALVE_ABOVE:
        state[:] >>= 1
    off = _cdiv(nr * state[64] + _cdiv(state[:64], np.int64(2)), state[:64] + 1)
    return off & 0xFFFF if truncate else off


def denoise_blocks(state, offsets, coef, dc_shift=0):
    """denoise_dct_c over the blocks of one frame (coef [B, 64] fdct outputs, row-major; position 0 is the reference's
    when dc_shift is added): state changes in place, the denoised outputs come back"""
    c = np.asarray(coef, np.int64).copy()
    c[:, 0] += dc_shift
    mag = np.abs(c)
    state[:64] += mag.sum(axis=0)
    state[64] += c.shape[0]
    out = np.sign(c) * np.maximum(mag - offsets[None, :], 0)
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


def encode_stream(frames, w, h, nr, state=None, mode="product", qbias=0, truncate=True, halve=True, want_coef=False):
    """frames: [(y, cb, cr)] planes of 2-D uint8 -> the chunks (or, want_coef, the zig-zag lines per frame); state (65
    int64, new_state() when None) changes in place.  nr = 0 leaves it alone, as the reference allocates nothing then."""
    if state is None:
        state = new_state()
    ref = mode == "reference"
    out = []
    for y, cb, cr in frames:
        coef = fdct(frame_blocks(y, cb, cr, w, h, 0 if ref else 128))
        if nr:
            offsets = frame_start(state, nr, truncate, halve)
            coef = denoise_blocks(state, offsets, coef, 0 if ref else DC_SHIFT)
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
