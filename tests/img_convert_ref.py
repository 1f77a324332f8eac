"""CPU restatement of the reference's img_convert (AMVmuxer/ffmpeg/libavcodec/imgconvert.c:2329-2571) for the routes
amvhip_img_convert_dev offers, and of the control flow of the sws_scale shim (imgresample.c:599-690).  TEST INFRASTRUCTURE:
numpy, whole planes at a time; written from reading the reference, pinned to outputs of the real reference by
tests/golden/ref_img_convert.json (test_img_convert.py).

A picture is a list of 2-D uint8 planes: three for the planar YUV formats, one for the others (a packed row is the row's
bytes: w * bpp columns).  4:2:0 chroma planes are (w + 1) / 2 x (h + 1) / 2, as the decoder makes them."""
import numpy as np

(YUV420P, YUVJ420P, YUV422P, YUVJ422P, YUV444P, YUVJ444P, YUYV422, UYVY422, RGB24, BGR24, RGB32, RGB565, RGB555,
 GRAY8) = range(14)
NAMES = ["yuv420p", "yuvj420p", "yuv422p", "yuvj422p", "yuv444p", "yuvj444p", "yuyv422", "uyvy422", "rgb24", "bgr24", "rgb32",
         "rgb565", "rgb555", "gray"]          # the reference's own names (pix_fmt_info, imgconvert.c:65-382)
BPP = {YUYV422: 2, UYVY422: 2, RGB24: 3, BGR24: 3, RGB32: 4, RGB565: 2, RGB555: 2}
PLANAR = (YUV420P, YUVJ420P, YUV422P, YUVJ422P, YUV444P, YUVJ444P)
JPEG = (YUVJ420P, YUVJ422P, YUVJ444P)
P420, P422, P444 = (YUV420P, YUVJ420P), (YUV422P, YUVJ422P), (YUV444P, YUVJ444P)

SCALEBITS = 10
ONE_HALF = 1 << (SCALEBITS - 1)


def FIX(x):                                   # colorspace.h:32
    return int(x * (1 << SCALEBITS) + 0.5)


def cm(v):                                    # ff_cropTbl + MAX_NEG_CROP: clamp to 0..255
    return np.clip(v, 0, 255)


def range_tables():
    """the four 256-entry tables img_convert_init fills (imgconvert.c:1216-1233) from colorspace.h:69-84"""
    i = np.arange(256, dtype=np.int64)
    y_c2j = cm((i * FIX(255.0 / 219.0) + (ONE_HALF - 16 * FIX(255.0 / 219.0))) >> SCALEBITS)
    y_j2c = (i * FIX(219.0 / 255.0) + (ONE_HALF + (16 << SCALEBITS))) >> SCALEBITS
    c_c2j = cm(((i - 128) * FIX(127.0 / 112.0) + (ONE_HALF + (128 << SCALEBITS))) >> SCALEBITS)
    c_j2c = np.maximum(((i - 128) * FIX(112.0 / 127.0) + (ONE_HALF + (128 << SCALEBITS))) >> SCALEBITS, 16)
    return {"y_ccir_to_jpeg": y_c2j.astype(np.uint8), "y_jpeg_to_ccir": y_j2c.astype(np.uint8),
            "c_ccir_to_jpeg": c_c2j.astype(np.uint8), "c_jpeg_to_ccir": c_j2c.astype(np.uint8)}


TABLES = range_tables()


def fnv1a64(data):
    h = 0xCBF29CE484222325
    for b in bytes(data):
        h = ((h ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


# ---- geometry ------------------------------------------------------------------------------------------------------------

def plane_shapes(fmt, w, h):
    """[(rows, row bytes)] of the planes of a w x h picture"""
    if fmt in PLANAR:
        cw = w if fmt in P444 else (w + 1) // 2
        ch = (h + 1) // 2 if fmt in P420 else h
        return [(h, w), (ch, cw), (ch, cw)]
    return [(h, w * BPP.get(fmt, 1))]


def frame_bytes(fmt, w, h):
    return sum(r * c for r, c in plane_shapes(fmt, w, h))


def split(fmt, w, h, buf):
    """a tight frame (the raw-video layout: planes back to back) -> planes"""
    buf = np.frombuffer(bytes(buf), np.uint8) if not isinstance(buf, np.ndarray) else buf
    out, pos = [], 0
    for r, c in plane_shapes(fmt, w, h):
        out.append(buf[pos:pos + r * c].reshape(r, c))
        pos += r * c
    return out


def join(planes):
    return np.concatenate([np.ascontiguousarray(p).reshape(-1) for p in planes])


def make_picture(fmt, w, h, kind, seed=0):
    """seeded test pictures: noise, zeros, ones (all 255), ramp (16 .. 235 along the diagonals: the nominal CCIR range)"""
    n = frame_bytes(fmt, w, h)
    if kind == "noise":
        buf = np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)
    elif kind == "zeros":
        buf = np.zeros(n, np.uint8)
    elif kind == "ones":
        buf = np.full(n, 255, np.uint8)
    elif kind == "ramp":
        planes = []
        for r, c in plane_shapes(fmt, w, h):
            planes.append((16 + (np.arange(c)[None, :] * 3 + np.arange(r)[:, None] * 5 + seed) % 220).astype(np.uint8))
        return planes
    else:
        raise ValueError(kind)
    return split(fmt, w, h, buf)


# ---- which pairs -----------------------------------------------------------------------------------------------------------

def route(src, dst):
    """the one-step routes (None: the reference needs an intermediate picture, :2514-2571, or the formats are equal)"""
    if src == dst:
        return None
    if src in PLANAR and dst in P420:
        return "planes"
    if src in P420 and dst == GRAY8:
        return "gray"
    if src in (YUYV422, UYVY422) and dst == YUV420P:
        return "packed_in"
    if src == YUV420P and dst in (YUYV422, UYVY422):
        return "packed_out"
    if (src in (RGB24, BGR24, RGB32) and dst == YUV420P) or (src == RGB24 and dst == YUVJ420P):
        return "rgb_in"
    if src in P420 and dst in (RGB24, BGR24, RGB32, RGB565, RGB555):
        return "rgb_out"
    return None


def supported_pairs():
    return [(s, d) for s in range(14) for d in range(14) if route(s, d)]


def any_size(src, dst):
    """routes that take odd sizes (the others want even width and height)"""
    r = route(src, dst)
    return r in ("gray", "rgb_out") or (r == "planes" and src in P420)


# ---- the routes ------------------------------------------------------------------------------------------------------------

def _apply(table, plane):
    return TABLES[table][plane]


def _planes(src, p, dst, w, h):
    """imgconvert.c:2415-2513: luma copied, chroma through ff_img_copy_plane / shrink12 (:1318) / ff_shrink22 (:1351), then
    the range tables on the destination.  Between two 4:2:0 formats the whole chroma planes are taken (the library's
    rule; the reference stops at w >> 1 x h >> 1, which is the same for even sizes)."""
    y = p[0]
    out = []
    for c in p[1:]:
        c = c.astype(np.int32)
        if src in P420:
            out.append(c)
        elif src in P422:                                        # 1x2 -> 1x1: (a + b) >> 1
            out.append((c[0::2] + c[1::2]) >> 1)
        else:                                                    # 2x2 -> 1x1: (a + b + c + d + 2) >> 2
            out.append((c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + 2) >> 2)
    res = [y] + [c.astype(np.uint8) for c in out]
    if (src in JPEG) != (dst in JPEG):
        ty, tc = ("y_jpeg_to_ccir", "c_jpeg_to_ccir") if src in JPEG else ("y_ccir_to_jpeg", "c_ccir_to_jpeg")
        res = [_apply(ty, res[0]), _apply(tc, res[1]), _apply(tc, res[2])]
    return res


def _gray(src, p):                                               # :2399-2413
    return [p[0].copy() if src in JPEG else _apply("y_ccir_to_jpeg", p[0])]


def _packed_in(src, p, w, h):                                    # :867-978: chroma of the even lines
    q = p[0].reshape(h, w // 2, 4)
    yo, uo, vo = ((0, 2), 1, 3) if src == YUYV422 else ((1, 3), 0, 2)
    y = np.stack([q[:, :, yo[0]], q[:, :, yo[1]]], axis=2).reshape(h, w)
    return [y, q[0::2, :, uo].copy(), q[0::2, :, vo].copy()]


def _packed_out(p, dst, w, h):                                   # :1150-1214: a chroma line serves two lines
    q = np.zeros((h, w // 2, 4), np.uint8)
    yo, uo, vo = ((0, 2), 1, 3) if dst == YUYV422 else ((1, 3), 0, 2)
    q[:, :, yo[0]] = p[0][:, 0::2]
    q[:, :, yo[1]] = p[0][:, 1::2]
    q[:, :, uo] = np.repeat(p[1], 2, axis=0)
    q[:, :, vo] = np.repeat(p[2], 2, axis=0)
    return [q.reshape(h, w * 2)]


def _rgb_of(src, plane, w, h):
    """RGB_IN of the format (imgconvert.c:1662-1727): r, g, b as int planes"""
    q = plane.reshape(h, w, BPP[src]).astype(np.int32)
    if src == RGB24:
        return q[:, :, 0], q[:, :, 1], q[:, :, 2]
    return q[:, :, 2], q[:, :, 1], q[:, :, 0]                    # BGR24; RGB32 = the word a r g b, little-endian: B G R A


def _rgb_in(src, p, dst, w, h):
    """imgconvert_template.h:218-323 (towards YUV420P: the _CCIR macros, colorspace.h:99-109) and :654- (RGB24 towards
    YUVJ420P: colorspace.h:87-97); even sizes: luma per pixel, chroma from the 2x2 sums with shift 2"""
    r, g, b = _rgb_of(src, p[0], w, h)
    ys, cs, yadd = (1.0, 1.0, 0) if dst == YUVJ420P else (219.0 / 255.0, 224.0 / 255.0, 16 << SCALEBITS)
    y = (FIX(0.29900 * ys) * r + FIX(0.58700 * ys) * g + FIX(0.11400 * ys) * b + ONE_HALF + yadd) >> SCALEBITS
    s = lambda c: c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2]
    r1, g1, b1 = s(r), s(g), s(b)
    rnd = (ONE_HALF << 2) - 1
    u = ((-FIX(0.16874 * cs) * r1 - FIX(0.33126 * cs) * g1 + FIX(0.50000 * cs) * b1 + rnd) >> (SCALEBITS + 2)) + 128
    v = ((FIX(0.50000 * cs) * r1 - FIX(0.41869 * cs) * g1 - FIX(0.08131 * cs) * b1 + rnd) >> (SCALEBITS + 2)) + 128
    return [y.astype(np.uint8), u.astype(np.uint8), v.astype(np.uint8)]


def _rgb_out(src, p, dst, w, h):
    """imgconvert_template.h:30-216: YUV_TO_RGB1/2_CCIR (colorspace.h:34-50) from YUV420P, YUV_TO_RGB1/2 (:52-67) from
    YUVJ420P; every size (a chroma sample serves up to 2 x 2 pixels), RGB_OUT of the format (imgconvert.c:1628-1732)"""
    up = lambda c: np.repeat(np.repeat(c.astype(np.int32), 2, axis=0), 2, axis=1)[:h, :w]
    cb, cr = up(p[1]) - 128, up(p[2]) - 128
    if src == YUVJ420P:
        y = p[0].astype(np.int32) << SCALEBITS
        s = 1.0
    else:
        y = (p[0].astype(np.int32) - 16) * FIX(255.0 / 219.0)
        s = 255.0 / 224.0
    r = cm((y + FIX(1.40200 * s) * cr + ONE_HALF) >> SCALEBITS)
    g = cm((y - FIX(0.34414 * s) * cb - FIX(0.71414 * s) * cr + ONE_HALF) >> SCALEBITS)
    b = cm((y + FIX(1.77200 * s) * cb + ONE_HALF) >> SCALEBITS)
    if dst == RGB24:
        q = np.stack([r, g, b], axis=2)
    elif dst == BGR24:
        q = np.stack([b, g, r], axis=2)
    elif dst == RGB32:
        q = np.stack([b, g, r, np.full_like(r, 255)], axis=2)
    else:
        v = ((r >> 3) << 11) | ((g >> 2) << 5) | (b >> 3) if dst == RGB565 else ((r >> 3) << 10) | ((g >> 3) << 5) | (b >> 3)
        q = np.stack([v & 255, v >> 8], axis=2)
    return [q.astype(np.uint8).reshape(h, -1)]


def convert(src, planes, dst, w, h):
    """one supported img_convert; planes in, planes out"""
    r = route(src, dst)
    if r is None:
        raise ValueError("no one-step route %s -> %s" % (NAMES[src], NAMES[dst]))
    if not any_size(src, dst) and (w & 1 or h & 1):
        raise ValueError("%s -> %s wants even sizes" % (NAMES[src], NAMES[dst]))
    if r == "planes":
        return _planes(src, planes, dst, w, h)
    if r == "gray":
        return _gray(src, planes)
    if r == "packed_in":
        return _packed_in(src, planes, w, h)
    if r == "packed_out":
        return _packed_out(planes, dst, w, h)
    if r == "rgb_in":
        return _rgb_in(src, planes, dst, w, h)
    return _rgb_out(src, planes, dst, w, h)


def sws_scale(src, planes, sw, sh, dst, dw, dh, resample):
    """the shim (imgresample.c:599-690).  resample(frame bytes, sw, sh, dw, dh) -> frame bytes is img_resample on a tight
    YUV420P picture with (w >> 1) x (h >> 1) chroma (the oracle's); even sizes where a picture is rescaled."""
    if (sw, sh) == (dw, dh):
        return [p.copy() for p in planes] if src == dst else convert(src, planes, dst, dw, dh)
    if src != YUV420P:
        planes = convert(src, planes, YUV420P, sw, sh)
    out = split(YUV420P, dw, dh, resample(join(planes), sw, sh, dw, dh))
    return out if dst == YUV420P else convert(YUV420P, out, dst, dw, dh)
