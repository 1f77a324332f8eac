"""CPU restatement of the stages of ffmpeg's video front end around the sws_scale shim: avpicture_deinterlace
(AMVmuxer/ffmpeg/libavcodec/imgconvert.c:2673-2864, the C branch), av_picture_crop (:2224-2244), av_picture_pad (:2246-2304),
-padcolor (ffmpeg.c:2246-2271) and the order do_video_out and pre_process_video_frame run them in (ffmpeg.c:579-623, :730-765).
TEST INFRASTRUCTURE: numpy, whole planes at a time; written from reading the reference, pinned to outputs of the real
reference's command line by tests/golden/ref_frontend.json (test_frontend_ref.py).  The rescale and convert steps are
img_convert_ref.sws_scale's.

Pictures are lists of 2-D uint8 planes as in img_convert_ref.  Bands are (top, bottom, left, right)."""
import numpy as np

import img_convert_ref as R

DEINTERLACED = (R.YUV420P, R.YUV422P, R.YUV444P, R.GRAY8)     # avpicture_deinterlace's list among our formats (:2824-2828)
DEFAULT_COLOR = (16, 128, 128)                                # ffmpeg.c:114


def deinterlace_supported(fmt, w, h):
    return fmt in DEINTERLACED and w > 0 and h > 0 and w % 4 == 0 and h % 4 == 0


def deinterlace_plane(p):
    """deinterlace_bottom_field (:2765-2792): even rows copied; odd row 2k + 1 from rows 2k - 1 .. 2k + 3 with weights
    -1 4 2 4 -1, rounded, >> 3, clamped; above row 1 stands row 0, below the last row the last row itself, twice"""
    h = p.shape[0]
    s = p.astype(np.int32)
    out = p.copy()
    odd = np.arange(1, h, 2)
    m2 = np.where(odd >= 2, odd - 2, 0)
    p1 = np.where(odd == h - 1, odd, odd + 1)
    p2 = np.where(odd == h - 1, odd, np.minimum(odd + 2, h - 1))
    total = -s[m2] + 4 * s[odd - 1] + 2 * s[odd] + 4 * s[p1] - s[p2]
    out[odd] = np.clip((total + 4) >> 3, 0, 255).astype(np.uint8)
    return out


def deinterlace_plane_inplace(p):
    """deinterlace_bottom_field_inplace (:2794-2817) line by line as deinterlace_line_inplace (:2719-2760) runs: `buf` keeps
    what the row two above held before it was overwritten"""
    p = p.copy()
    h = p.shape[0]
    buf = p[0].astype(np.int32)
    for y in range(0, h - 2, 2):
        m1, s0, p1, p2 = (p[y + k].astype(np.int32) for k in range(4))
        total = -buf + 4 * m1 + 2 * s0 + 4 * p1 - p2
        buf = s0
        p[y + 1] = np.clip((total + 4) >> 3, 0, 255)
    m1, s0 = p[h - 2].astype(np.int32), p[h - 1].astype(np.int32)
    p[h - 1] = np.clip((-buf + 4 * m1 + 2 * s0 + 4 * s0 - s0 + 4) >> 3, 0, 255)
    return p


def deinterlace(fmt, planes, w, h, inplace=False):
    if not deinterlace_supported(fmt, w, h):
        raise ValueError("avpicture_deinterlace refuses %s at %dx%d" % (R.NAMES[fmt], w, h))
    return [(deinterlace_plane_inplace if inplace else deinterlace_plane)(p) for p in planes]


def shifts(fmt):
    """x_chroma_shift, y_chroma_shift of a planar YUV format"""
    return (0 if fmt in R.P444 else 1), (1 if fmt in R.P420 else 0)


def crop(fmt, planes, w, h, bands):
    """av_picture_crop moves the plane origins by top, left (chroma: >> the shifts); the picture's size becomes the cropped
    one (ffmpeg.c:1685-1686).  Planar YUV only."""
    top, bottom, left, right = bands
    if fmt not in R.PLANAR:
        raise ValueError("av_picture_crop refuses %s" % R.NAMES[fmt])
    cw, ch = w - left - right, h - top - bottom
    xs, ys = shifts(fmt)
    out = []
    for i, ((rows, cols), p) in enumerate(zip(R.plane_shapes(fmt, cw, ch), planes)):
        oy, ox = (top >> ys, left >> xs) if i else (top, left)
        out.append(p[oy:oy + rows, ox:ox + cols].copy())
    return out, cw, ch


def deinterlace_window(fmt, planes, w, h, bands):
    """what the device makes of deinterlace-then-crop: only the kept rows and columns, a row's rule taken from its index
    in the full plane -- restated on its own, so that test_frontend_ref can hold it against crop(deinterlace(...))"""
    top, bottom, left, right = bands
    cw, ch = w - left - right, h - top - bottom
    xs, ys = shifts(fmt)
    out = []
    for i, ((rows, cols), p) in enumerate(zip(R.plane_shapes(fmt, cw, ch), planes)):
        oy, ox = (top >> ys, left >> xs) if i else (top, left)
        full_h = p.shape[0]
        s = p.astype(np.int32)
        win = np.zeros((rows, cols), np.uint8)
        for r in range(rows):
            y = oy + r
            if y % 2 == 0:
                win[r] = p[y, ox:ox + cols]
                continue
            m2 = y - 2 if y >= 2 else 0
            p1, p2 = (y, y) if y == full_h - 1 else (y + 1, min(y + 2, full_h - 1))
            total = -s[m2] + 4 * s[y - 1] + 2 * s[y] + 4 * s[p1] - s[p2]
            win[r] = np.clip((total[ox:ox + cols] + 4) >> 3, 0, 255)
        out.append(win)
    return out


def pad(window, width, height, bands, color=DEFAULT_COLOR):
    """the encoder's YUVJ420P picture width x height: `window` (planes of (width - left - right) x (height - top - bottom))
    placed at top, left, every other byte of plane i the byte color[i] (band sizes >> 1 on the chroma planes)"""
    top, bottom, left, right = bands
    out = []
    for i, p in enumerate(window):
        s = 1 if i else 0
        full = np.full((height >> s, width >> s), color[i], np.uint8)
        rows, cols = (height - top - bottom) >> s, (width - left - right) >> s
        assert p.shape == (rows, cols), (p.shape, rows, cols)
        full[top >> s:(top >> s) + rows, left >> s:(left >> s) + cols] = p
        out.append(full)
    return out


def pad_color_from_rgb(rrggbb):
    """opt_pad_color: RGB_TO_Y, RGB_TO_U(.., 0), RGB_TO_V(.., 0) of ffmpeg.c:2246-2256 on r = rgb >> 16, g, b; the ints reach
    the planes through memset, that is as bytes"""
    r, g, b = rrggbb >> 16, (rrggbb >> 8) & 255, rrggbb & 255
    F = R.FIX
    y = (F(0.29900) * r + F(0.58700) * g + F(0.11400) * b + R.ONE_HALF) >> R.SCALEBITS
    u = ((-F(0.16874) * r - F(0.33126) * g + F(0.50000) * b + R.ONE_HALF - 1) >> R.SCALEBITS) + 128
    v = ((F(0.50000) * r - F(0.41869) * g - F(0.08131) * b + R.ONE_HALF - 1) >> R.SCALEBITS) + 128
    return (y & 255, u & 255, v & 255)


def frontend(fmt, planes, w, h, width, height, resample, deint=False, crop_bands=(0, 0, 0, 0), pad_bands=(0, 0, 0, 0),
             color=DEFAULT_COLOR):
    """pre_process_video_frame + do_video_out up to the encoder's input: deinterlace (skipped where the routine refuses,
    ffmpeg.c:602-608), crop, the shim into the window, the bands.  resample as in img_convert_ref.sws_scale."""
    if deint and deinterlace_supported(fmt, w, h):
        planes = deinterlace(fmt, planes, w, h)
    if any(crop_bands):
        planes, w, h = crop(fmt, planes, w, h, crop_bands)
    top, bottom, left, right = pad_bands
    iw, ih = width - left - right, height - top - bottom
    window = R.sws_scale(fmt, planes, w, h, R.YUVJ420P, iw, ih, resample)
    return pad(window, width, height, pad_bands, color) if any(pad_bands) else window
