// amvhip_pixfmt.hip -- pixel formats behind the C ABI: img_convert, the sws_scale shim, the shim joined to the encoder and
// the decoder, the stages of ffmpeg's video front end around it (deinterlace, crop, pad), and the decode-side postprocessing.
#include "amvhip_ctx.h"

using namespace amv;

namespace {

int pix_picture_ok(int f, const PixPicture& pic, uint32_t w, uint32_t h) {
    for (uint32_t p = 0; p < 3; ++p) {
        uint32_t rb, rows;
        pix_plane_size(f, p, w, h, &rb, &rows);
        if (!rows) continue;
        if (!pic.p[p] || ((uintptr_t)pic.p[p] & 3u) || pic.stride[p] < rb) return 0;
    }
    return 1;
}

// one supported pair, n frames, on st (the context is locked); every argument checked by the caller
int convert_launch(amvhip_ctx* c, int src_fmt, const PixPicture& src, int dst_fmt, const PixPicture& dst, uint32_t w, uint32_t h, uint32_t n,
                   hipStream_t st) {
    Timed t(c, AMVHIP_K_PIXFMT, st);
    switch (pix_route(src_fmt, dst_fmt)) {
        case kRoutePlanes: case kRouteGray: {
            const bool to_jpeg = !pix_jpeg(src_fmt) && (dst_fmt == AMVHIP_PIX_GRAY8 || pix_jpeg(dst_fmt));
            const bool to_ccir = pix_jpeg(src_fmt) && dst_fmt != AMVHIP_PIX_GRAY8 && !pix_jpeg(dst_fmt);
            PixPlaneJobs jobs{};
            jobs.count = dst_fmt == AMVHIP_PIX_GRAY8 ? 1u : 3u;
            // 4:2:0 to 4:2:0 takes the chroma planes whole, (w + 1) / 2 x (h + 1) / 2; the shrinking routes have even sizes
            const uint32_t cw = (w + 1) / 2, chh = (h + 1) / 2;
            for (uint32_t p = 0; p < jobs.count; ++p) {
                PixPlaneJob& j = jobs.j[p];
                j = PixPlaneJob{src.p[p], dst.p[p], src.stride[p], dst.stride[p], src.frame[p], dst.frame[p], p ? cw : w, p ? chh : h, kPixCopy,
                                kPixRangeNone};
                if (p) j.resize = pix_420(src_fmt) ? kPixCopy : (pix_444(src_fmt) ? kPixShrink22 : kPixShrink12);
                if (to_jpeg) j.range = p ? kPixCCcirToJpeg : kPixYCcirToJpeg;
                if (to_ccir) j.range = p ? kPixCJpegToCcir : kPixYJpegToCcir;
            }
            launch_pix_planes(jobs, n, st);
            break;
        }
        case kRoutePackedIn: {
            const bool uyvy = src_fmt == AMVHIP_PIX_UYVY422;
            PixPicture d = dst;
            if (uyvy) { std::swap(d.p[1], d.p[2]); std::swap(d.stride[1], d.stride[2]); std::swap(d.frame[1], d.frame[2]); }
            launch_pix_packed_in(src, d, w, h, uyvy, n, st);
            break;
        }
        case kRoutePackedOut: {
            const bool uyvy = dst_fmt == AMVHIP_PIX_UYVY422;
            PixPicture s = src;
            if (uyvy) { std::swap(s.p[1], s.p[2]); std::swap(s.stride[1], s.stride[2]); std::swap(s.frame[1], s.frame[2]); }
            launch_pix_packed_out(s, dst, w, h, uyvy, n, st);
            break;
        }
        case kRouteRgbIn: {
            // RGB_TO_Y_CCIR / _U_CCIR / _V_CCIR (colorspace.h:99-109) towards YUV420P, RGB_TO_Y / _U / _V (:87-97) towards YUVJ420P
            const bool jpeg = dst_fmt == AMVHIP_PIX_YUVJ420P;
            const double ys = jpeg ? 1.0 : 219.0 / 255.0, cs = jpeg ? 1.0 : 224.0 / 255.0;
            const int yr = pix_fix(0.29900 * ys), yg = pix_fix(0.58700 * ys), yb = pix_fix(0.11400 * ys);
            const int ur = -pix_fix(0.16874 * cs), ug = -pix_fix(0.33126 * cs), ub = pix_fix(0.50000 * cs);
            const int vr = pix_fix(0.50000 * cs), vg = -pix_fix(0.41869 * cs), vb = -pix_fix(0.08131 * cs);
            const bool red_first = src_fmt == AMVHIP_PIX_RGB24;   // BGR24 and RGB32 (B G R A in memory) have blue at +0
            PixRgbIn k;
            k.y[0] = red_first ? yr : yb; k.y[1] = yg; k.y[2] = red_first ? yb : yr;
            k.yadd = 512 + (jpeg ? 0 : 16 << 10);
            k.u[0] = red_first ? ur : ub; k.u[1] = ug; k.u[2] = red_first ? ub : ur;
            k.v[0] = red_first ? vr : vb; k.v[1] = vg; k.v[2] = red_first ? vb : vr;
            launch_pix_rgb_in(src, dst, w, h, pix_bpp(src_fmt), k, n, st);
            break;
        }
        case kRouteRgbOut: {
            // YUV_TO_RGB1_CCIR / 2_CCIR (colorspace.h:34-50) from YUV420P, YUV_TO_RGB1 / 2 (:52-67) from YUVJ420P
            const bool jpeg = src_fmt == AMVHIP_PIX_YUVJ420P;
            const double s = jpeg ? 1.0 : 255.0 / 224.0;
            const int r[2] = {0, pix_fix(1.40200 * s)}, g[2] = {-pix_fix(0.34414 * s), -pix_fix(0.71414 * s)}, b[2] = {pix_fix(1.77200 * s), 0};
            const bool blue_first = dst_fmt == AMVHIP_PIX_BGR24 || dst_fmt == AMVHIP_PIX_RGB32;
            PixRgbOut k;
            k.ymul = jpeg ? 1024 : pix_fix(255.0 / 219.0);
            k.yoff = jpeg ? 0 : 16;
            for (int i = 0; i < 2; ++i) { k.c0[i] = blue_first ? b[i] : r[i]; k.c1[i] = g[i]; k.c2[i] = blue_first ? r[i] : b[i]; }
            k.rshift = dst_fmt == AMVHIP_PIX_RGB565 ? 11u : 10u;
            k.gdrop = dst_fmt == AMVHIP_PIX_RGB565 ? 2u : 3u;
            launch_pix_rgb_out(src, dst, w, h, pix_bpp(dst_fmt), k, n, st);
            break;
        }
        default: return fail(c, AMVHIP_ERR_ARG, "img_convert: no one-step route from format %d to format %d", src_fmt, dst_fmt);
    }
    return check_launch(c, "img_convert");
}

// av_picture_copy (imgconvert.c:808-863) for two pictures of one format
int copy_launch(amvhip_ctx* c, int fmt, const PixPicture& src, const PixPicture& dst, uint32_t w, uint32_t h, uint32_t n, hipStream_t st) {
    Timed t(c, AMVHIP_K_PIXFMT, st);
    PixPlaneJobs jobs{};
    for (uint32_t p = 0; p < 3; ++p) {
        uint32_t rb, rows;
        pix_plane_size(fmt, p, w, h, &rb, &rows);
        if (!rows) continue;
        jobs.j[jobs.count++] = PixPlaneJob{src.p[p], dst.p[p], src.stride[p], dst.stride[p], src.frame[p], dst.frame[p], rb, rows, kPixCopy,
                                           kPixRangeNone};
    }
    launch_pix_planes(jobs, n, st);
    return check_launch(c, "picture copy");
}

// what both img_convert entry points ask of the pair and of the size
int convert_args_ok(amvhip_ctx* c, int src_fmt, int dst_fmt, uint32_t w, uint32_t h) {
    if (pix_route(src_fmt, dst_fmt) == kRouteNone)
        return fail(c, AMVHIP_ERR_ARG, "img_convert: no one-step route from format %d to format %d", src_fmt, dst_fmt);
    if (!pix_size_ok(src_fmt, dst_fmt, w, h)) return fail(c, AMVHIP_ERR_ARG, "img_convert: bad size %ux%u (this route wants even sizes)", w, h);
    return AMVHIP_OK;
}

// sws_scale (imgresample.c:599-690), the context locked.  Towards YUVJ420P at another size the closing YUV420P -> YUVJ420P
// step rides in the rescaler's store: no pass of its own.
int sws_core(amvhip_ctx* c, int src_fmt, const PixPicture& src, uint32_t src_w, uint32_t src_h, int dst_fmt, const PixPicture& dst,
             uint32_t dst_w, uint32_t dst_h, uint32_t n, hipStream_t st) {
    if (src_w == dst_w && src_h == dst_h) {
        if (src_fmt == dst_fmt) return copy_launch(c, src_fmt, src, dst, dst_w, dst_h, n, st);
        return convert_launch(c, src_fmt, src, dst_fmt, dst, dst_w, dst_h, n, st);
    }
    PixPicture in = src;
    if (src_fmt != AMVHIP_PIX_YUV420P) {
        const uint64_t fb = amvhip_yuv420_frame_bytes(src_w, src_h);
        if (int r = ensure(c, c->pix_in, fb * n)) return r;
        in = tight_420((uint8_t*)c->pix_in.p, src_w, src_h);
        if (int r = convert_launch(c, src_fmt, src, AMVHIP_PIX_YUV420P, in, src_w, src_h, n, st)) return r;
    }
    if (dst_fmt == AMVHIP_PIX_YUV420P || dst_fmt == AMVHIP_PIX_YUVJ420P)
        return resample_launch(c, in, src_w, src_h, dst, dst_w, dst_h, n, dst_fmt == AMVHIP_PIX_YUVJ420P, st);
    const uint64_t fb = amvhip_yuv420_frame_bytes(dst_w, dst_h);
    if (int r = ensure(c, c->pix_out, fb * n)) return r;
    const PixPicture mid = tight_420((uint8_t*)c->pix_out.p, dst_w, dst_h);
    // img_resample writes (w >> 1) x (h >> 1) chroma, the routines out of YUV420P read (w + 1) / 2 x (h + 1) / 2: the reference
    // leaves an odd picture's last chroma column and row undefined, here they are 128 (no colour) whatever the workspace held
    if (((dst_w | dst_h) & 1) && dst_fmt != AMVHIP_PIX_GRAY8) HIP_TRY(c, hipMemsetAsync(c->pix_out.p, 128, fb * n, st));
    if (int r = resample_launch(c, in, src_w, src_h, mid, dst_w, dst_h, n, false, st)) return r;
    return convert_launch(c, AMVHIP_PIX_YUV420P, mid, dst_fmt, dst, dst_w, dst_h, n, st);
}

// the checks of amvhip_sws_scale_dev, shared with the entries built on it
// (dst == nullptr: the destination is the context's own)
int sws_args_ok(amvhip_ctx* c, int src_fmt, const PixPicture& src, uint32_t src_w, uint32_t src_h, int dst_fmt, const PixPicture* dst,
                uint32_t dst_w, uint32_t dst_h) {
    if (src_fmt < 0 || src_fmt >= AMVHIP_PIX_COUNT || dst_fmt < 0 || dst_fmt >= AMVHIP_PIX_COUNT)
        return fail(c, AMVHIP_ERR_ARG, "sws_scale: unknown pixel format");
    if (!size_ok(src_w, src_h) || !size_ok(dst_w, dst_h)) return fail(c, AMVHIP_ERR_ARG, "sws_scale: bad picture size");
    if (src_w == dst_w && src_h == dst_h) {
        if (src_fmt != dst_fmt && (pix_route(src_fmt, dst_fmt) == kRouteNone || !pix_size_ok(src_fmt, dst_fmt, dst_w, dst_h)))
            return fail(c, AMVHIP_ERR_ARG, "sws_scale: no one-step route from format %d to format %d at %ux%u", src_fmt, dst_fmt, dst_w, dst_h);
    } else {
        if (src_w < 2 || src_h < 2 || dst_w < 2 || dst_h < 2) return fail(c, AMVHIP_ERR_ARG, "sws_scale: a rescaled picture is at least 2x2");
        if (src_fmt != AMVHIP_PIX_YUV420P &&
            (pix_route(src_fmt, AMVHIP_PIX_YUV420P) == kRouteNone || !pix_size_ok(src_fmt, AMVHIP_PIX_YUV420P, src_w, src_h)))
            return fail(c, AMVHIP_ERR_ARG, "sws_scale: no one-step route from format %d to YUV420P at %ux%u", src_fmt, src_w, src_h);
        if (dst_fmt != AMVHIP_PIX_YUV420P && dst_fmt != AMVHIP_PIX_YUVJ420P &&
            (pix_route(AMVHIP_PIX_YUV420P, dst_fmt) == kRouteNone || !pix_size_ok(AMVHIP_PIX_YUV420P, dst_fmt, dst_w, dst_h)))
            return fail(c, AMVHIP_ERR_ARG, "sws_scale: no one-step route from YUV420P to format %d at %ux%u", dst_fmt, dst_w, dst_h);
    }
    if (!pix_picture_ok(src_fmt, src, src_w, src_h) || (dst && !pix_picture_ok(dst_fmt, *dst, dst_w, dst_h)))
        return fail(c, AMVHIP_ERR_ARG, "sws_scale: null or misaligned plane, or a row pitch below the row");
    return AMVHIP_OK;
}

}  // namespace

int amv::pix_convert_launch(amvhip_ctx* c, int src_fmt, const PixPicture& src, int dst_fmt, const PixPicture& dst, uint32_t w, uint32_t h, uint32_t n,
                            hipStream_t st) {
    return convert_launch(c, src_fmt, src, dst_fmt, dst, w, h, n, st);
}

extern "C" uint64_t amvhip_pix_frame_bytes(int fmt, uint32_t stride, uint32_t height) { return pix_frame_bytes(fmt, stride, height); }

extern "C" int amvhip_img_convert_supported(int src_fmt, int dst_fmt, uint32_t w, uint32_t h) {
    return pix_route(src_fmt, dst_fmt) != kRouteNone && pix_size_ok(src_fmt, dst_fmt, w, h);
}

extern "C" int amvhip_img_convert_dev(amvhip_ctx* c, int src_fmt, const uint8_t* d_src0, const uint8_t* d_src1, const uint8_t* d_src2,
                                      uint32_t src_stride, uint32_t src_c_stride, uint64_t src_frame_stride, uint64_t src_c_frame_stride,
                                      int dst_fmt, uint8_t* d_dst0, uint8_t* d_dst1, uint8_t* d_dst2, uint32_t dst_stride, uint32_t dst_c_stride,
                                      uint64_t dst_frame_stride, uint64_t dst_c_frame_stride, uint32_t w, uint32_t h, uint32_t n, void* stream) {
    if (!c) return AMVHIP_ERR_ARG;
    if (int r = convert_args_ok(c, src_fmt, dst_fmt, w, h)) return r;
    const PixPicture src = make_picture(d_src0, d_src1, d_src2, src_stride, src_c_stride, src_frame_stride, src_c_frame_stride);
    const PixPicture dst = make_picture(d_dst0, d_dst1, d_dst2, dst_stride, dst_c_stride, dst_frame_stride, dst_c_frame_stride);
    if (!pix_picture_ok(src_fmt, src, w, h) || !pix_picture_ok(dst_fmt, dst, w, h))
        return fail(c, AMVHIP_ERR_ARG, "img_convert: null or misaligned plane, or a row pitch below the row");
    if (n == 0) return AMVHIP_OK;
    if (int r = use_device(c)) return r;
    std::lock_guard<std::mutex> lk(c->mu);
    return convert_launch(c, src_fmt, src, dst_fmt, dst, w, h, n, (hipStream_t)stream);
}

// host buffers: the planes are staged tight on the device (rows of exactly the row's bytes), `launch`ed on (staged source,
// staged destination, stream; the context locked), and the destination rows copied back row by row -- bytes between the
// caller's rows and frames are never touched
template <class Launch>
static int host_staged(amvhip_ctx* c, const char* what, int src_fmt, const PixPicture& hs, int dst_fmt, const PixPicture& hd, uint32_t w, uint32_t h,
                uint32_t n, Launch launch) {
    PixPicture ds{}, dd{};
    uint64_t bytes[2] = {0, 0};
    for (int side = 0; side < 2; ++side) {
        const int f = side ? dst_fmt : src_fmt;
        const PixPicture& hp = side ? hd : hs;
        PixPicture& dp = side ? dd : ds;
        uint64_t off[4] = {0, 0, 0, 0};
        for (uint32_t p = 0; p < 3; ++p) {
            uint32_t rb, rows;
            pix_plane_size(f, p, w, h, &rb, &rows);
            if (rows && (!hp.p[p] || hp.stride[p] < rb)) return fail(c, AMVHIP_ERR_ARG, "%s: null plane, or a row pitch below the row", what);
            dp.stride[p] = rb;
            off[p + 1] = off[p] + (((uint64_t)rb * rows + 15u) & ~15ull);    // every staged plane starts 16-byte aligned
        }
        for (uint32_t p = 0; p < 3; ++p) {
            dp.frame[p] = off[3];
            dp.p[p] = (uint8_t*)off[p];                                      // offset for now
        }
        bytes[side] = off[3] * n;
    }
    if (n == 0) return AMVHIP_OK;
    hipStream_t st;
    if (int r = host_stream(c, &st)) return r;
    std::lock_guard<std::mutex> hlk(c->hmu);
    if (int r = ensure(c, c->h_in, bytes[0])) return r;
    if (int r = ensure(c, c->h_out, bytes[1])) return r;
    for (uint32_t p = 0; p < 3; ++p) {
        ds.p[p] = (uint8_t*)c->h_in.p + (uintptr_t)ds.p[p];
        dd.p[p] = (uint8_t*)c->h_out.p + (uintptr_t)dd.p[p];
    }
    for (int side = 0; side < 2; ++side) {
        const int f = side ? dst_fmt : src_fmt;
        if (side) {
            std::lock_guard<std::mutex> lk(c->mu);
            if (int r = launch(ds, dd, st)) return r;
        }
        for (uint32_t p = 0; p < 3; ++p) {
            uint32_t rb, rows;
            pix_plane_size(f, p, w, h, &rb, &rows);
            if (!rows) continue;
            for (uint32_t i = 0; i < n; ++i) {
                if (!side)
                    HIP_TRY(c, hipMemcpy2DAsync(ds.p[p] + i * ds.frame[p], rb, hs.p[p] + i * hs.frame[p], hs.stride[p], rb, rows,
                                                hipMemcpyHostToDevice, st));
                else
                    HIP_TRY(c, hipMemcpy2DAsync(hd.p[p] + i * hd.frame[p], hd.stride[p], dd.p[p] + i * dd.frame[p], rb, rb, rows,
                                                hipMemcpyDeviceToHost, st));
            }
        }
    }
    HIP_TRY(c, hipStreamSynchronize(st));
    return AMVHIP_OK;
}

extern "C" int amvhip_img_convert(amvhip_ctx* c, int src_fmt, const uint8_t* src0, const uint8_t* src1, const uint8_t* src2,
                                  uint32_t src_stride, uint32_t src_c_stride, uint64_t src_frame_stride, uint64_t src_c_frame_stride,
                                  int dst_fmt, uint8_t* dst0, uint8_t* dst1, uint8_t* dst2, uint32_t dst_stride, uint32_t dst_c_stride,
                                  uint64_t dst_frame_stride, uint64_t dst_c_frame_stride, uint32_t w, uint32_t h, uint32_t n) {
    if (!c) return AMVHIP_ERR_ARG;
    if (int r = convert_args_ok(c, src_fmt, dst_fmt, w, h)) return r;
    return host_staged(c, "img_convert", src_fmt, make_picture(src0, src1, src2, src_stride, src_c_stride, src_frame_stride, src_c_frame_stride),
                       dst_fmt, make_picture(dst0, dst1, dst2, dst_stride, dst_c_stride, dst_frame_stride, dst_c_frame_stride), w, h, n,
                       [&](const PixPicture& ds, const PixPicture& dd, hipStream_t st) {
                           return convert_launch(c, src_fmt, ds, dst_fmt, dd, w, h, n, st);
                       });
}

extern "C" int amvhip_sws_scale_dev(amvhip_ctx* c, int src_fmt, const uint8_t* d_src0, const uint8_t* d_src1, const uint8_t* d_src2,
                                    uint32_t src_stride, uint32_t src_c_stride, uint64_t src_frame_stride, uint64_t src_c_frame_stride,
                                    uint32_t src_w, uint32_t src_h, int dst_fmt, uint8_t* d_dst0, uint8_t* d_dst1, uint8_t* d_dst2,
                                    uint32_t dst_stride, uint32_t dst_c_stride, uint64_t dst_frame_stride, uint64_t dst_c_frame_stride,
                                    uint32_t dst_w, uint32_t dst_h, uint32_t n, void* stream) {
    if (!c) return AMVHIP_ERR_ARG;
    const PixPicture src = make_picture(d_src0, d_src1, d_src2, src_stride, src_c_stride, src_frame_stride, src_c_frame_stride);
    const PixPicture dst = make_picture(d_dst0, d_dst1, d_dst2, dst_stride, dst_c_stride, dst_frame_stride, dst_c_frame_stride);
    if (int r = sws_args_ok(c, src_fmt, src, src_w, src_h, dst_fmt, &dst, dst_w, dst_h)) return r;
    if (n == 0) return AMVHIP_OK;
    if (int r = use_device(c)) return r;
    std::lock_guard<std::mutex> lk(c->mu);   // the intermediates are the context's
    return sws_core(c, src_fmt, src, src_w, src_h, dst_fmt, dst, dst_w, dst_h, n, (hipStream_t)stream);
}

// ffmpeg.c:757-814 for any supported source: the shim to YUVJ420P, then the encoder
extern "C" int amvhip_encode_fmt_scaled_batch_dev(amvhip_ctx* c, int src_fmt, const uint8_t* d_src0, const uint8_t* d_src1,
                                                  const uint8_t* d_src2, uint32_t src_stride, uint32_t src_c_stride,
                                                  uint64_t src_frame_stride, uint64_t src_c_frame_stride, uint32_t src_w, uint32_t src_h,
                                                  uint32_t n, uint32_t w, uint32_t h, uint32_t qbias, uint8_t* d_blob, uint64_t blob_cap,
                                                  uint64_t* d_offs, uint32_t* d_lens, void* stream) {
    if (!c) return AMVHIP_ERR_ARG;
    if (!encode_size_ok(w, h, qbias) || (n && (!d_blob || !d_offs || !d_lens)))
        return fail(c, AMVHIP_ERR_ARG, "encode_fmt: bad argument (width/height must be even)");
    const bool same = src_w == w && src_h == h;
    // the two sources the encoder reads itself (its colour stage is the reference's rgb24_to_yuvj420p; BGR24 is that routine
    // with the weights exchanged, as amvhip_encode_batch_dev has always taken it)
    if (same && (src_fmt == AMVHIP_PIX_RGB24 || src_fmt == AMVHIP_PIX_BGR24)) {
        if (src_frame_stride != (uint64_t)src_stride * h && n > 1)
            return fail(c, AMVHIP_ERR_ARG, "encode_fmt: RGB frames at the target size lie back to back (frame stride = stride * height)");
        return amvhip_encode_batch_dev(c, d_src0, src_stride, src_fmt == AMVHIP_PIX_BGR24, n, w, h, qbias, d_blob, blob_cap, d_offs, d_lens, stream);
    }
    if (same && src_fmt == AMVHIP_PIX_YUVJ420P)
        return amvhip_encode_yuv420_batch_dev(c, d_src0, d_src1, d_src2, src_stride, src_c_stride, src_frame_stride, src_c_frame_stride, n, w, h,
                                              qbias, d_blob, blob_cap, d_offs, d_lens, stream);
    const PixPicture src = make_picture(d_src0, d_src1, d_src2, src_stride, src_c_stride, src_frame_stride, src_c_frame_stride);
    if (int r = sws_args_ok(c, src_fmt, src, src_w, src_h, AMVHIP_PIX_YUVJ420P, nullptr, w, h)) return r;
    if (n == 0) return AMVHIP_OK;
    if (int r = use_device(c)) return r;
    // the planes in between are the context's: the lock is held from their allocation to the last launch that reads them
    std::lock_guard<std::mutex> lk(c->mu);
    if (int r = ensure(c, c->scaled, amvhip_yuv420_frame_bytes(w, h) * n)) return r;
    const PixPicture dst = tight_420((uint8_t*)c->scaled.p, w, h);
    if (int r = sws_core(c, src_fmt, src, src_w, src_h, AMVHIP_PIX_YUVJ420P, dst, w, h, n, (hipStream_t)stream)) return r;
    return encode_scaled_tail(c, n, w, h, qbias, PlainQuant{}, d_blob, blob_cap, d_offs, d_lens, (hipStream_t)stream);
}

// the decoder of the patched FFmpeg, then img_convert towards what the next stage wants (ffmpeg -i x.amv -pix_fmt ...)
extern "C" int amvhip_decode_fmt_batch_dev(amvhip_ctx* c, const uint8_t* d_blob, uint64_t blob_bytes, const uint64_t* d_offs,
                                           const uint32_t* d_lens, uint32_t n, uint32_t w, uint32_t h, uint32_t flags, int dst_fmt,
                                           uint8_t* d_out, uint32_t out_stride, int32_t* d_status, void* stream) {
    if (!c) return AMVHIP_ERR_ARG;
    if (!(flags & AMVHIP_FLAG_FFMPEG)) return fail(c, AMVHIP_ERR_ARG, "decode_fmt: AMVHIP_FLAG_FFMPEG is required (the planes are that decoder's)");
    if (flags & AMVHIP_FLAG_FFMPEG_KEEP) return fail(c, AMVHIP_ERR_ARG, "decode_fmt: AMVHIP_FLAG_FFMPEG_KEEP needs the caller's planes; d_out is not in plane form");
    if (pix_route(AMVHIP_PIX_YUVJ420P, dst_fmt) == kRouteNone)
        return fail(c, AMVHIP_ERR_ARG, "decode_fmt: no one-step route from YUVJ420P to format %d", dst_fmt);
    if (int r = decode_args_ok(c, d_blob, d_offs, d_lens, n, w, h, flags, d_out, d_status)) return r;
    const uint64_t out_frame = amvhip_pix_frame_bytes(dst_fmt, out_stride, h);
    PixPicture dst = make_picture(d_out, nullptr, nullptr, out_stride, (out_stride + 1) / 2, out_frame, out_frame);
    if (dst_fmt == AMVHIP_PIX_YUV420P) {
        dst.p[1] = d_out + (uint64_t)out_stride * h;
        dst.p[2] = dst.p[1] + (uint64_t)dst.stride[1] * ((h + 1) / 2);
    }
    if (out_stride < w * pix_bpp(dst_fmt)) return fail(c, AMVHIP_ERR_ARG, "decode_fmt: out_stride below the row");
    if (n == 0) return AMVHIP_OK;
    if (int r = use_device(c)) return r;
    std::lock_guard<std::mutex> lk(c->mu);
    const uint64_t fb = amvhip_yuv420_frame_bytes(w, h);
    if (int r = ensure(c, c->pix_dec, fb * n)) return r;
    if (int r = decode_core(c, d_blob, blob_bytes, d_offs, d_lens, n, w, h, flags, (uint8_t*)c->pix_dec.p, d_status, c->set[0],
                            (hipStream_t)stream, (hipStream_t)stream))
        return r;
    return convert_launch(c, AMVHIP_PIX_YUVJ420P, tight_420((uint8_t*)c->pix_dec.p, w, h), dst_fmt, dst, w, h, n, (hipStream_t)stream);
}


// ---- the video front end: pre_process_video_frame (ffmpeg.c:579-623) and do_video_out up to the encoder (:730-765) ------
namespace {

// avpicture_deinterlace over the window `win` of every plane (the whole planes: win = full), n frames, on st
int deinterlace_launch(amvhip_ctx* c, const PixPicture& src, const PixPicture& dst, uint32_t planes, const FrontRect* full, const FrontRect* win,
                       uint32_t n, hipStream_t st) {
    Timed t(c, AMVHIP_K_PIXFMT, st);
    DeintJobs jobs{};
    jobs.count = planes;
    for (uint32_t p = 0; p < planes; ++p)
        jobs.j[p] = DeintPlane{src.p[p], dst.p[p], src.stride[p], dst.stride[p], src.frame[p], dst.frame[p], win[p].x, win[p].y, win[p].w, win[p].h,
                               full[p].h};
    launch_deinterlace(jobs, n, st);
    return check_launch(c, "deinterlace");
}

// the bytes [first, end) the n frames of plane p touch
void plane_span(int fmt, const PixPicture& pic, uint32_t p, uint32_t w, uint32_t h, uint32_t n, uintptr_t* first, uintptr_t* end) {
    uint32_t rb, rows;
    pix_plane_size(fmt, p, w, h, &rb, &rows);
    *first = (uintptr_t)pic.p[p];
    *end = rows && n ? *first + (uint64_t)(n - 1) * pic.frame[p] + (uint64_t)(rows - 1) * pic.stride[p] + rb : *first;
}

int deinterlace_args_ok(amvhip_ctx* c, int fmt, uint32_t w, uint32_t h) {
    if (!deinterlace_ok(fmt, w, h))
        return fail(c, AMVHIP_ERR_ARG, "deinterlace: format %d at %ux%u is not taken (YUV420P, YUV422P, YUV444P, GRAY8; sizes multiples of 4)", fmt, w, h);
    return AMVHIP_OK;
}

int deinterlace_whole(amvhip_ctx* c, int fmt, const PixPicture& src, const PixPicture& dst, uint32_t w, uint32_t h, uint32_t n, hipStream_t st) {
    FrontRect full[3] = {};
    uint32_t planes = 0;
    for (uint32_t i = 0; i < 3; ++i) {
        uint32_t rb, rows;
        pix_plane_size(fmt, i, w, h, &rb, &rows);
        if (!rows) continue;
        full[i] = FrontRect{0, 0, rb, rows};
        planes = i + 1;
    }
    return deinterlace_launch(c, src, dst, planes, full, full, n, st);
}

// the stages in the reference's order into dst (YUVJ420P, width x height); c->mu held, every argument checked
int frontend_core(amvhip_ctx* c, int src_fmt, const PixPicture& src, uint32_t n, const amvhip_frontend* fe, const FrontPlan& p, const PixPicture& dst,
                  hipStream_t st) {
    PixPicture cur = src;
    if (p.deinterlace) {
        // deinterlace, then crop: only what the crop keeps is made, tight, in the source's format
        if (int r = ensure(c, c->fe_deint, p.deint_frame_bytes * n)) return r;
        PixPicture d{};
        for (uint32_t i = 0; i < p.src_planes; ++i) {
            d.p[i] = (uint8_t*)c->fe_deint.p + p.deint_plane_off[i];
            d.stride[i] = p.src_win[i].w;
            d.frame[i] = p.deint_frame_bytes;
        }
        if (int r = deinterlace_launch(c, src, d, p.src_planes, p.src_full, p.src_win, n, st)) return r;
        cur = d;
    } else if (p.crop) {
        for (uint32_t i = 0; i < p.src_planes; ++i) cur.p[i] += (uint64_t)p.src_win[i].y * cur.stride[i] + p.src_win[i].x;   // av_picture_crop
    }
    PixPicture win = dst;                                            // resampling_dst: a cropped view of the padded picture
    for (uint32_t i = 0; i < 3; ++i) win.p[i] += (uint64_t)p.dst_win[i].y * win.stride[i] + p.dst_win[i].x;
    if (int r = sws_core(c, src_fmt, cur, p.crop_w, p.crop_h, AMVHIP_PIX_YUVJ420P, win, p.win_w, p.win_h, n, st)) return r;
    if (!p.pad) return AMVHIP_OK;
    Timed t(c, AMVHIP_K_PIXFMT, st);
    PadBandJobs jobs{};
    for (uint32_t i = 0; i < 3; ++i)
        jobs.j[i] = PadBandPlane{dst.p[i], dst.stride[i], dst.frame[i], p.dst_full[i].w, p.dst_full[i].h, p.dst_win[i].x, p.dst_win[i].y,
                                 p.dst_win[i].w, p.dst_win[i].h, (fe ? fe->pad_color[i] : 0u) * 0x01010101u};
    launch_pad_bands(jobs, n, st);
    return check_launch(c, "pad bands");
}

// what both front-end entries ask of the source and of the bands; *p filled
int frontend_args_ok(amvhip_ctx* c, int src_fmt, const PixPicture& src, uint32_t src_w, uint32_t src_h, const amvhip_frontend* fe, uint32_t w,
                     uint32_t h, FrontPlan* p) {
    *p = front_plan(src_fmt, src_w, src_h, fe, w, h);
    if (p->refusal) return fail(c, AMVHIP_ERR_ARG, "video front end: %s", front_refusal_text(p->refusal));
    if (!pix_picture_ok(src_fmt, src, src_w, src_h))
        return fail(c, AMVHIP_ERR_ARG, "video front end: null or misaligned source plane, or a row pitch below the row");
    return AMVHIP_OK;
}

}  // namespace

extern "C" void amvhip_pad_color_from_rgb(uint32_t rrggbb, uint8_t out[3]) {
    if (out) pad_color_from_rgb(rrggbb, out);
}

extern "C" int amvhip_deinterlace_supported(int fmt, uint32_t w, uint32_t h) { return deinterlace_ok(fmt, w, h); }

extern "C" int amvhip_deinterlace_dev(amvhip_ctx* c, int fmt, const uint8_t* d_src0, const uint8_t* d_src1, const uint8_t* d_src2,
                                      uint32_t src_stride, uint32_t src_c_stride, uint64_t src_frame_stride, uint64_t src_c_frame_stride,
                                      uint8_t* d_dst0, uint8_t* d_dst1, uint8_t* d_dst2, uint32_t dst_stride, uint32_t dst_c_stride,
                                      uint64_t dst_frame_stride, uint64_t dst_c_frame_stride, uint32_t w, uint32_t h, uint32_t n, void* stream) {
    if (!c) return AMVHIP_ERR_ARG;
    if (int r = deinterlace_args_ok(c, fmt, w, h)) return r;
    const PixPicture src = make_picture(d_src0, d_src1, d_src2, src_stride, src_c_stride, src_frame_stride, src_c_frame_stride);
    const PixPicture dst = make_picture(d_dst0, d_dst1, d_dst2, dst_stride, dst_c_stride, dst_frame_stride, dst_c_frame_stride);
    if (!pix_picture_ok(fmt, src, w, h) || !pix_picture_ok(fmt, dst, w, h))
        return fail(c, AMVHIP_ERR_ARG, "deinterlace: null or misaligned plane, or a row pitch below the row");
    // out of place only: a lane reads rows that another lane writes
    const uint32_t planes = fmt == AMVHIP_PIX_GRAY8 ? 1u : 3u;
    for (uint32_t i = 0; i < planes; ++i)
        for (uint32_t k = 0; k < planes; ++k) {
            uintptr_t s0, s1, d0, d1;
            plane_span(fmt, src, i, w, h, n, &s0, &s1);
            plane_span(fmt, dst, k, w, h, n, &d0, &d1);
            if (s0 < d1 && d0 < s1) return fail(c, AMVHIP_ERR_ARG, "deinterlace: source and destination overlap");
        }
    if (n == 0) return AMVHIP_OK;
    if (int r = use_device(c)) return r;
    std::lock_guard<std::mutex> lk(c->mu);
    return deinterlace_whole(c, fmt, src, dst, w, h, n, (hipStream_t)stream);
}

extern "C" int amvhip_deinterlace(amvhip_ctx* c, int fmt, const uint8_t* src0, const uint8_t* src1, const uint8_t* src2, uint32_t src_stride,
                                  uint32_t src_c_stride, uint64_t src_frame_stride, uint64_t src_c_frame_stride, uint8_t* dst0, uint8_t* dst1,
                                  uint8_t* dst2, uint32_t dst_stride, uint32_t dst_c_stride, uint64_t dst_frame_stride,
                                  uint64_t dst_c_frame_stride, uint32_t w, uint32_t h, uint32_t n) {
    if (!c) return AMVHIP_ERR_ARG;
    if (int r = deinterlace_args_ok(c, fmt, w, h)) return r;
    const PixPicture hs = make_picture(src0, src1, src2, src_stride, src_c_stride, src_frame_stride, src_c_frame_stride);
    const PixPicture hd = make_picture(dst0, dst1, dst2, dst_stride, dst_c_stride, dst_frame_stride, dst_c_frame_stride);
    const uint32_t planes = fmt == AMVHIP_PIX_GRAY8 ? 1u : 3u;
    for (uint32_t i = 0; i < planes; ++i)
        for (uint32_t k = 0; k < planes; ++k) {
            if (!hs.p[i] || !hd.p[k]) return fail(c, AMVHIP_ERR_ARG, "deinterlace: null plane");
            uintptr_t s0, s1, d0, d1;
            plane_span(fmt, hs, i, w, h, n, &s0, &s1);
            plane_span(fmt, hd, k, w, h, n, &d0, &d1);
            if (s0 < d1 && d0 < s1) return fail(c, AMVHIP_ERR_ARG, "deinterlace: source and destination overlap");
        }
    return host_staged(c, "deinterlace", fmt, hs, fmt, hd, w, h, n, [&](const PixPicture& ds, const PixPicture& dd, hipStream_t st) {
        return deinterlace_whole(c, fmt, ds, dd, w, h, n, st);
    });
}

extern "C" int amvhip_video_frontend_dev(amvhip_ctx* c, int src_fmt, const uint8_t* d_src0, const uint8_t* d_src1, const uint8_t* d_src2,
                                         uint32_t src_stride, uint32_t src_c_stride, uint64_t src_frame_stride, uint64_t src_c_frame_stride,
                                         uint32_t src_w, uint32_t src_h, uint32_t n, const amvhip_frontend* fe, uint8_t* d_y, uint8_t* d_cb,
                                         uint8_t* d_cr, uint32_t y_stride, uint32_t c_stride, uint64_t y_frame_stride, uint64_t c_frame_stride,
                                         uint32_t w, uint32_t h, void* stream) {
    if (!c) return AMVHIP_ERR_ARG;
    const PixPicture src = make_picture(d_src0, d_src1, d_src2, src_stride, src_c_stride, src_frame_stride, src_c_frame_stride);
    const PixPicture dst = make_picture(d_y, d_cb, d_cr, y_stride, c_stride, y_frame_stride, c_frame_stride);
    FrontPlan p;
    if (int r = frontend_args_ok(c, src_fmt, src, src_w, src_h, fe, w, h, &p)) return r;
    if (!pix_picture_ok(AMVHIP_PIX_YUVJ420P, dst, w, h))
        return fail(c, AMVHIP_ERR_ARG, "video front end: null or misaligned destination plane, or a row pitch below the row");
    if (n == 0) return AMVHIP_OK;
    if (int r = use_device(c)) return r;
    std::lock_guard<std::mutex> lk(c->mu);   // the intermediates are the context's
    return frontend_core(c, src_fmt, src, n, fe, p, dst, (hipStream_t)stream);
}

extern "C" int amvhip_encode_frontend_batch_dev(amvhip_ctx* c, int src_fmt, const uint8_t* d_src0, const uint8_t* d_src1, const uint8_t* d_src2,
                                                uint32_t src_stride, uint32_t src_c_stride, uint64_t src_frame_stride,
                                                uint64_t src_c_frame_stride, uint32_t src_w, uint32_t src_h, uint32_t n,
                                                const amvhip_frontend* fe, uint32_t w, uint32_t h, uint32_t qbias, uint8_t* d_blob,
                                                uint64_t blob_cap, uint64_t* d_offs, uint32_t* d_lens, void* stream) {
    if (!c) return AMVHIP_ERR_ARG;
    // no stage asked for: the entry without them, its fused and direct routes included
    if (front_is_identity(fe))
        return amvhip_encode_fmt_scaled_batch_dev(c, src_fmt, d_src0, d_src1, d_src2, src_stride, src_c_stride, src_frame_stride, src_c_frame_stride,
                                                  src_w, src_h, n, w, h, qbias, d_blob, blob_cap, d_offs, d_lens, stream);
    if (!encode_size_ok(w, h, qbias) || (n && (!d_blob || !d_offs || !d_lens)))
        return fail(c, AMVHIP_ERR_ARG, "encode_frontend: bad argument (width/height must be even)");
    const PixPicture src = make_picture(d_src0, d_src1, d_src2, src_stride, src_c_stride, src_frame_stride, src_c_frame_stride);
    FrontPlan p;
    if (int r = frontend_args_ok(c, src_fmt, src, src_w, src_h, fe, w, h, &p)) return r;
    if (n == 0) return AMVHIP_OK;
    if (int r = use_device(c)) return r;
    // the padded picture is the context's: the lock is held from its allocation to the last launch that reads it
    std::lock_guard<std::mutex> lk(c->mu);
    if (int r = ensure(c, c->scaled, p.padded_frame_bytes * n)) return r;
    if (int r = frontend_core(c, src_fmt, src, n, fe, p, tight_420((uint8_t*)c->scaled.p, w, h), (hipStream_t)stream)) return r;
    return encode_scaled_tail(c, n, w, h, qbias, PlainQuant{}, d_blob, blob_cap, d_offs, d_lens, (hipStream_t)stream);
}

// amvhip_encode_frontend_batch_dev with a quantiser request in the place of qbias: the pictures always go through the
// context's workspace (the identity front end too: the shim's conversion or copy), and the encoder behind them takes the
// request -- what amvhip_video_frontend_dev into tight planes and the YUV420 entry of the request give in two calls.
// err: where the _psnr form wants the frames' error (the error of the workspace pictures against what was coded of them)
static int frontend_quant(amvhip_ctx* c, int src_fmt, const uint8_t* d_src0, const uint8_t* d_src1, const uint8_t* d_src2, uint32_t src_stride,
                          uint32_t src_c_stride, uint64_t src_frame_stride, uint64_t src_c_frame_stride, uint32_t src_w, uint32_t src_h, uint32_t n,
                          const amvhip_frontend* fe, uint32_t w, uint32_t h, const amvhip_quant* q, uint8_t* d_blob, uint64_t blob_cap,
                          uint64_t* d_offs, uint32_t* d_lens, const ErrorSink& err, void* stream, const QnsArg& qns = kNoQns) {
    if (!c) return AMVHIP_ERR_ARG;
    QuantRequest req;
    if (int r = quant_request_of(c, q, &req)) return r;
    if (!encode_size_ok(w, h, q->qbias) || (n && (!d_blob || !d_offs || !d_lens)))
        return fail(c, AMVHIP_ERR_ARG, "encode_frontend: bad argument (width/height must be even)");
    if (int r = quant_args_ok(c, n, w, h, req)) return r;
    if (int r = error_sink_ok(c, n, err)) return r;
    if (int r = qns_args_ok(c, qns)) return r;
    const PixPicture src = make_picture(d_src0, d_src1, d_src2, src_stride, src_c_stride, src_frame_stride, src_c_frame_stride);
    FrontPlan p;
    if (int r = frontend_args_ok(c, src_fmt, src, src_w, src_h, fe, w, h, &p)) return r;
    if (n == 0) return AMVHIP_OK;
    if (int r = use_device(c)) return r;
    // the padded picture is the context's: the lock is held from its allocation to the last launch that reads it
    std::lock_guard<std::mutex> lk(c->mu);
    if (int r = ensure(c, c->scaled, p.padded_frame_bytes * n)) return r;
    if (int r = frontend_core(c, src_fmt, src, n, fe, p, tight_420((uint8_t*)c->scaled.p, w, h), (hipStream_t)stream)) return r;
    return encode_scaled_tail(c, n, w, h, q->qbias, req, d_blob, blob_cap, d_offs, d_lens, (hipStream_t)stream, err.wanted ? err.sse : nullptr,
                              qns);
}

extern "C" int amvhip_encode_frontend_quant_stream_dev(amvhip_ctx* c, int src_fmt, const uint8_t* d_src0, const uint8_t* d_src1,
                                                       const uint8_t* d_src2, uint32_t src_stride, uint32_t src_c_stride,
                                                       uint64_t src_frame_stride, uint64_t src_c_frame_stride, uint32_t src_w, uint32_t src_h,
                                                       uint32_t n, const amvhip_frontend* fe, uint32_t w, uint32_t h, const amvhip_quant* q,
                                                       uint8_t* d_blob, uint64_t blob_cap, uint64_t* d_offs, uint32_t* d_lens, void* stream) {
    return frontend_quant(c, src_fmt, d_src0, d_src1, d_src2, src_stride, src_c_stride, src_frame_stride, src_c_frame_stride, src_w, src_h, n, fe,
                          w, h, q, d_blob, blob_cap, d_offs, d_lens, kNoError, stream);
}

extern "C" int amvhip_encode_frontend_quant_psnr_stream_dev(amvhip_ctx* c, int src_fmt, const uint8_t* d_src0, const uint8_t* d_src1,
                                                            const uint8_t* d_src2, uint32_t src_stride, uint32_t src_c_stride,
                                                            uint64_t src_frame_stride, uint64_t src_c_frame_stride, uint32_t src_w,
                                                            uint32_t src_h, uint32_t n, const amvhip_frontend* fe, uint32_t w, uint32_t h,
                                                            const amvhip_quant* q, uint8_t* d_blob, uint64_t blob_cap, uint64_t* d_offs,
                                                            uint32_t* d_lens, uint64_t* d_sse, void* stream) {
    return frontend_quant(c, src_fmt, d_src0, d_src1, d_src2, src_stride, src_c_stride, src_frame_stride, src_c_frame_stride, src_w, src_h, n, fe,
                          w, h, q, d_blob, blob_cap, d_offs, d_lens, ErrorSink{d_sse, true}, stream);
}

// ... with qns, lambda2 behind the request (amv_qns_plan.h); d_sse NULL = errors not wanted
extern "C" int amvhip_encode_frontend_qns_stream_dev(amvhip_ctx* c, int src_fmt, const uint8_t* d_src0, const uint8_t* d_src1, const uint8_t* d_src2,
                                                     uint32_t src_stride, uint32_t src_c_stride, uint64_t src_frame_stride,
                                                     uint64_t src_c_frame_stride, uint32_t src_w, uint32_t src_h, uint32_t n,
                                                     const amvhip_frontend* fe, uint32_t w, uint32_t h, const amvhip_quant* q, uint32_t qns,
                                                     uint32_t lambda2, uint8_t* d_blob, uint64_t blob_cap, uint64_t* d_offs, uint32_t* d_lens,
                                                     uint64_t* d_sse, void* stream) {
    return frontend_quant(c, src_fmt, d_src0, d_src1, d_src2, src_stride, src_c_stride, src_frame_stride, src_c_frame_stride, src_w, src_h, n, fe,
                          w, h, q, d_blob, blob_cap, d_offs, d_lens, ErrorSink{d_sse, d_sse != nullptr}, stream, QnsArg{qns, lambda2});
}

// ... with a byte budget per frame (amv_rate_plan.h): the pictures are made in the workspace as above, and the rate route
// (amvhip_encode.hip: rate_core) runs behind them -- amvhip_video_frontend_dev into tight planes and
// amvhip_encode_yuv420_rate_stream_dev in one call
extern "C" int amvhip_encode_frontend_rate_stream_dev(amvhip_ctx* c, int src_fmt, const uint8_t* d_src0, const uint8_t* d_src1, const uint8_t* d_src2,
                                                      uint32_t src_stride, uint32_t src_c_stride, uint64_t src_frame_stride,
                                                      uint64_t src_c_frame_stride, uint32_t src_w, uint32_t src_h, uint32_t n,
                                                      const amvhip_frontend* fe, uint32_t w, uint32_t h, const amvhip_quant* q,
                                                      const amvhip_rate* rate_in, uint8_t* d_blob, uint64_t blob_cap, uint64_t* d_offs,
                                                      uint32_t* d_lens, uint32_t* d_rung, void* stream) {
    if (!c) return AMVHIP_ERR_ARG;
    QuantRequest req;
    RateArg rate;
    if (int r = rate_request_of(c, q, rate_in, &req, &rate)) return r;
    if (!encode_size_ok(w, h, q->qbias) || (n && (!d_blob || !d_offs || !d_lens)))
        return fail(c, AMVHIP_ERR_ARG, "encode_frontend: bad argument (width/height must be even)");
    if (int r = rate_args_ok(c, n, w, h, req, d_rung)) return r;
    const PixPicture src = make_picture(d_src0, d_src1, d_src2, src_stride, src_c_stride, src_frame_stride, src_c_frame_stride);
    FrontPlan p;
    if (int r = frontend_args_ok(c, src_fmt, src, src_w, src_h, fe, w, h, &p)) return r;
    if (n == 0) return AMVHIP_OK;
    if (int r = use_device(c)) return r;
    // the padded picture is the context's: the lock is held from its allocation to the last launch that reads it
    std::lock_guard<std::mutex> lk(c->mu);
    if (int r = ensure(c, c->scaled, p.padded_frame_bytes * n)) return r;
    if (int r = frontend_core(c, src_fmt, src, n, fe, p, tight_420((uint8_t*)c->scaled.p, w, h), (hipStream_t)stream)) return r;
    return rate_scaled_tail(c, n, w, h, q->qbias, req, rate, d_blob, blob_cap, d_offs, d_lens, d_rung, (hipStream_t)stream);
}

// ... with a byte budget for the whole call above it (amv_clip_plan.h): the same, through rate_core with the clip
extern "C" int amvhip_encode_frontend_clip_stream_dev(amvhip_ctx* c, int src_fmt, const uint8_t* d_src0, const uint8_t* d_src1, const uint8_t* d_src2,
                                                      uint32_t src_stride, uint32_t src_c_stride, uint64_t src_frame_stride,
                                                      uint64_t src_c_frame_stride, uint32_t src_w, uint32_t src_h, uint32_t n,
                                                      const amvhip_frontend* fe, uint32_t w, uint32_t h, const amvhip_quant* q,
                                                      const amvhip_rate* rate_in, uint64_t total, uint8_t* d_blob, uint64_t blob_cap,
                                                      uint64_t* d_offs, uint32_t* d_lens, uint32_t* d_rung, uint64_t* d_clip, void* stream) {
    if (!c) return AMVHIP_ERR_ARG;
    QuantRequest req;
    RateArg rate;
    if (int r = rate_request_of(c, q, rate_in, &req, &rate)) return r;
    if (!encode_size_ok(w, h, q->qbias) || (n && (!d_blob || !d_offs || !d_lens)))
        return fail(c, AMVHIP_ERR_ARG, "encode_frontend: bad argument (width/height must be even)");
    if (int r = rate_args_ok(c, n, w, h, req, d_rung)) return r;
    if (int r = clip_args_ok(c, n, d_clip)) return r;
    const PixPicture src = make_picture(d_src0, d_src1, d_src2, src_stride, src_c_stride, src_frame_stride, src_c_frame_stride);
    FrontPlan p;
    if (int r = frontend_args_ok(c, src_fmt, src, src_w, src_h, fe, w, h, &p)) return r;
    if (n == 0) return AMVHIP_OK;
    if (int r = use_device(c)) return r;
    // the padded picture is the context's: the lock is held from its allocation to the last launch that reads it
    std::lock_guard<std::mutex> lk(c->mu);
    if (int r = ensure(c, c->scaled, p.padded_frame_bytes * n)) return r;
    if (int r = frontend_core(c, src_fmt, src, n, fe, p, tight_420((uint8_t*)c->scaled.p, w, h), (hipStream_t)stream)) return r;
    return clip_scaled_tail(c, n, w, h, q->qbias, req, rate, ClipArg{total, d_clip}, d_blob, blob_cap, d_offs, d_lens, d_rung,
                            (hipStream_t)stream);
}

// ---- `-psnr`: the host arithmetic, and picture against picture ------------------------------------------------------------
extern "C" double amvhip_psnr_db(uint64_t sse, uint64_t samples) { return psnr_db(sse, samples); }

extern "C" void amvhip_psnr_report(const uint64_t* sse, uint32_t n, uint32_t w, uint32_t h, double out[4]) {
    if (out && (sse || !n)) psnr_report(sse, n, w, h, out);
}

extern "C" int amvhip_picture_sse_supported(int fmt, uint32_t w, uint32_t h) { return picture_sse_ok(fmt, w, h); }

namespace {

// both pictures' planes as the kernel's jobs; 0: a plane is missing or a pitch is below the row
int sse_jobs(int fmt, const PixPicture& a, const PixPicture& b, uint32_t w, uint32_t h, SseJobs* jobs) {
    *jobs = SseJobs{};
    for (uint32_t p = 0; p < 3; ++p) {
        uint32_t rb, rows;
        pix_plane_size(fmt, p, w, h, &rb, &rows);
        if (!rows) continue;
        if (!a.p[p] || !b.p[p] || a.stride[p] < rb || b.stride[p] < rb) return 0;
        jobs->j[jobs->count++] = SsePlane{a.p[p], b.p[p], a.stride[p], b.stride[p], a.frame[p], b.frame[p], rb, rows, p, pix_bpp(fmt) == 3u ? 3u : 1u, 0u, 0u};
    }
    return 1;
}

int sse_launch(amvhip_ctx* c, const SseJobs& jobs, uint32_t n, uint64_t* d_sse, hipStream_t st) {
    HIP_TRY(c, hipMemsetAsync(d_sse, 0, (size_t)n * 24u, st));
    {
        Timed t(c, AMVHIP_K_PIXFMT, st);
        launch_picture_sse(jobs, n, d_sse, st);
    }
    return check_launch(c, "picture_sse");
}

}  // namespace

extern "C" int amvhip_picture_sse_dev(amvhip_ctx* c, int fmt, const uint8_t* d_a0, const uint8_t* d_a1, const uint8_t* d_a2, uint32_t a_stride,
                                      uint32_t a_c_stride, uint64_t a_frame_stride, uint64_t a_c_frame_stride, const uint8_t* d_b0,
                                      const uint8_t* d_b1, const uint8_t* d_b2, uint32_t b_stride, uint32_t b_c_stride, uint64_t b_frame_stride,
                                      uint64_t b_c_frame_stride, uint32_t w, uint32_t h, uint32_t n, uint64_t* d_sse, void* stream) {
    if (!c) return AMVHIP_ERR_ARG;
    if (!picture_sse_ok(fmt, w, h)) return fail(c, AMVHIP_ERR_ARG, "picture_sse: format %d at %ux%u is not taken (planar YUV, GRAY8, RGB24, BGR24)", fmt, w, h);
    SseJobs jobs;
    if (!sse_jobs(fmt, make_picture(d_a0, d_a1, d_a2, a_stride, a_c_stride, a_frame_stride, a_c_frame_stride),
                  make_picture(d_b0, d_b1, d_b2, b_stride, b_c_stride, b_frame_stride, b_c_frame_stride), w, h, &jobs))
        return fail(c, AMVHIP_ERR_ARG, "picture_sse: null plane, or a row pitch below the row");
    if (n && (!d_sse || ((uintptr_t)d_sse & 7u))) return fail(c, AMVHIP_ERR_ARG, "picture_sse: d_sse is null or not 8-byte aligned");
    if (n == 0) return AMVHIP_OK;
    if (int r = use_device(c)) return r;
    std::lock_guard<std::mutex> lk(c->mu);   // (the timing records are the context's)
    return sse_launch(c, jobs, n, d_sse, (hipStream_t)stream);
}

// host buffers: both pictures staged tight in c->h_in (a's planes, then b's, every plane 16-byte aligned), the sums in c->h_out
extern "C" int amvhip_picture_sse(amvhip_ctx* c, int fmt, const uint8_t* a0, const uint8_t* a1, const uint8_t* a2, uint32_t a_stride,
                                  uint32_t a_c_stride, uint64_t a_frame_stride, uint64_t a_c_frame_stride, const uint8_t* b0, const uint8_t* b1,
                                  const uint8_t* b2, uint32_t b_stride, uint32_t b_c_stride, uint64_t b_frame_stride, uint64_t b_c_frame_stride,
                                  uint32_t w, uint32_t h, uint32_t n, uint64_t* sse) {
    if (!c) return AMVHIP_ERR_ARG;
    if (!picture_sse_ok(fmt, w, h)) return fail(c, AMVHIP_ERR_ARG, "picture_sse: format %d at %ux%u is not taken (planar YUV, GRAY8, RGB24, BGR24)", fmt, w, h);
    const PixPicture host[2] = {make_picture(a0, a1, a2, a_stride, a_c_stride, a_frame_stride, a_c_frame_stride),
                                make_picture(b0, b1, b2, b_stride, b_c_stride, b_frame_stride, b_c_frame_stride)};
    SseJobs jobs;
    if (!sse_jobs(fmt, host[0], host[1], w, h, &jobs)) return fail(c, AMVHIP_ERR_ARG, "picture_sse: null plane, or a row pitch below the row");
    if (n && !sse) return fail(c, AMVHIP_ERR_ARG, "picture_sse: sse is null");
    if (n == 0) return AMVHIP_OK;
    uint64_t off[4] = {0, 0, 0, 0};          // of one picture's planes in a staged frame
    for (uint32_t p = 0; p < 3; ++p) {
        uint32_t rb, rows;
        pix_plane_size(fmt, p, w, h, &rb, &rows);
        off[p + 1] = off[p] + (((uint64_t)rb * rows + 15u) & ~15ull);
    }
    const uint64_t side = off[3] * n;
    hipStream_t st;
    if (int r = host_stream(c, &st)) return r;
    std::lock_guard<std::mutex> hlk(c->hmu);
    if (int r = ensure(c, c->h_in, 2u * side)) return r;
    if (int r = ensure(c, c->h_out, (size_t)n * 24u)) return r;
    for (uint32_t k = 0; k < jobs.count; ++k) {
        SsePlane& j = jobs.j[k];
        const uint32_t p = j.entry;
        for (uint32_t s = 0; s < 2; ++s) {
            uint8_t* d = (uint8_t*)c->h_in.p + s * side + off[p];
            for (uint32_t i = 0; i < n; ++i)
                HIP_TRY(c, hipMemcpy2DAsync(d + i * off[3], j.row_bytes, host[s].p[p] + i * host[s].frame[p], host[s].stride[p], j.row_bytes,
                                            j.rows, hipMemcpyHostToDevice, st));
            (s ? j.b : j.a) = d;
            (s ? j.bstride : j.astride) = j.row_bytes;
            (s ? j.bframe : j.aframe) = off[3];
        }
    }
    {
        std::lock_guard<std::mutex> lk(c->mu);
        if (int r = sse_launch(c, jobs, n, (uint64_t*)c->h_out.p, st)) return r;
    }
    HIP_TRY(c, hipMemcpyAsync(sse, c->h_out.p, (size_t)n * 24u, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    return AMVHIP_OK;
}

// ---- decode-side postprocessing: the reference's pp_postprocess for hb / vb / dr (amv_postprocess.hip, amv_pp_plan.h) -----
namespace {

// what the entries ask of mode, format and size; *qp: the QP of every frame that d_qp does not give
int pp_args_ok(amvhip_ctx* c, const char* what, int fmt, const amvhip_pp_mode* m, uint32_t w, uint32_t h, int* qp) {
    if (fmt != AMVHIP_PIX_YUV420P && fmt != AMVHIP_PIX_YUVJ420P) return fail(c, AMVHIP_ERR_ARG, "%s: format %d is not YUV420P / YUVJ420P", what, fmt);
    if (!m) return fail(c, AMVHIP_ERR_ARG, "%s: mode is NULL", what);
    if (!pp_mode_ok(m->lum_mode & ~kPpForceQuant) || !pp_mode_ok(m->chrom_mode & ~kPpForceQuant))
        return fail(c, AMVHIP_ERR_ARG, "%s: mode bits beyond hb, vb, dr, or dr without vb (its output is no function of the picture)", what);
    const bool forced = m->lum_mode & kPpForceQuant;
    if (forced && (m->forced_quant < 0 || m->forced_quant > 63)) return fail(c, AMVHIP_ERR_ARG, "%s: forced QP %d outside 0 .. 63", what, m->forced_quant);
    if (!pp_size_ok(w, h))
        return fail(c, AMVHIP_ERR_ARG, "%s: %ux%u is not taken (widths multiples of 16, even heights, 16x16 .. %ux%u)", what, w, h, kPpMaxWidth, kPpMaxHeight);
    *qp = forced ? m->forced_quant : 1;
    return AMVHIP_OK;
}

// tight planes on both sides (the caller checked), n frames, on st; the context is locked
int pp_launch(amvhip_ctx* c, const amvhip_pp_mode* m, int qp, const PixPicture& src, const PixPicture& dst, uint32_t w, uint32_t h, uint32_t n,
              const uint8_t* d_qp, hipStream_t st) {
    Timed t(c, AMVHIP_K_PIXFMT, st);
    PpJobs jobs{};
    // a plane whose mode has none of the three filters is copied: all the reference's loop does then is its block copy
    for (uint32_t p = 0; p < 3; ++p)
        jobs.j[p] = PpPlaneJob{src.p[p], dst.p[p], src.frame[p], dst.frame[p], p ? w / 2 : w, p ? h / 2 : h, (p ? m->chrom_mode : m->lum_mode) & kPpFilterBits};
    jobs.qp = qp;
    jobs.base_dc_diff = m->base_dc_diff;
    jobs.flat_thr = m->flatness_threshold;
    jobs.d_qp = d_qp;
    launch_postprocess(jobs, n, st);
    return check_launch(c, "postprocess");
}

int pp_tight(const PixPicture& pic, uint32_t w) {
    if (pic.stride[0] != w || pic.stride[1] != w / 2 || pic.stride[2] != w / 2) return 0;
    for (uint32_t p = 0; p < 3; ++p)
        if (pic.frame[p] & 3u) return 0;
    return 1;
}

}  // namespace

extern "C" int amvhip_postprocess_supported(uint32_t w, uint32_t h) { return pp_size_ok(w, h) ? 1 : 0; }

extern "C" int amvhip_postprocess_dev(amvhip_ctx* c, int fmt, const amvhip_pp_mode* mode, const uint8_t* d_src0, const uint8_t* d_src1,
                                      const uint8_t* d_src2, uint32_t src_stride, uint32_t src_c_stride, uint64_t src_frame_stride,
                                      uint64_t src_c_frame_stride, uint8_t* d_dst0, uint8_t* d_dst1, uint8_t* d_dst2, uint32_t dst_stride,
                                      uint32_t dst_c_stride, uint64_t dst_frame_stride, uint64_t dst_c_frame_stride, uint32_t w, uint32_t h,
                                      uint32_t n, const uint8_t* d_qp, void* stream) {
    if (!c) return AMVHIP_ERR_ARG;
    int qp;
    if (int r = pp_args_ok(c, "postprocess", fmt, mode, w, h, &qp)) return r;
    const PixPicture src = make_picture(d_src0, d_src1, d_src2, src_stride, src_c_stride, src_frame_stride, src_c_frame_stride);
    const PixPicture dst = make_picture(d_dst0, d_dst1, d_dst2, dst_stride, dst_c_stride, dst_frame_stride, dst_c_frame_stride);
    if (!pix_picture_ok(fmt, src, w, h) || !pix_picture_ok(fmt, dst, w, h)) return fail(c, AMVHIP_ERR_ARG, "postprocess: null or misaligned plane");
    if (!pp_tight(src, w) || !pp_tight(dst, w))
        return fail(c, AMVHIP_ERR_ARG, "postprocess: row pitches must be width and width / 2 (the dering's row-end window reads the next row's first "
                                       "columns), frame pitches multiples of 4");
    for (uint32_t i = 0; i < 3; ++i)
        for (uint32_t k = 0; k < 3; ++k) {
            uintptr_t s0, s1, d0, d1;
            plane_span(fmt, src, i, w, h, n, &s0, &s1);
            plane_span(fmt, dst, k, w, h, n, &d0, &d1);
            if (s0 < d1 && d0 < s1) return fail(c, AMVHIP_ERR_ARG, "postprocess: source and destination overlap");
        }
    if (n == 0) return AMVHIP_OK;
    if (int r = use_device(c)) return r;
    std::lock_guard<std::mutex> lk(c->mu);
    return pp_launch(c, mode, qp, src, dst, w, h, n, d_qp, (hipStream_t)stream);
}

extern "C" int amvhip_postprocess(amvhip_ctx* c, int fmt, const amvhip_pp_mode* mode, const uint8_t* src0, const uint8_t* src1, const uint8_t* src2,
                                  uint32_t src_stride, uint32_t src_c_stride, uint64_t src_frame_stride, uint64_t src_c_frame_stride, uint8_t* dst0,
                                  uint8_t* dst1, uint8_t* dst2, uint32_t dst_stride, uint32_t dst_c_stride, uint64_t dst_frame_stride,
                                  uint64_t dst_c_frame_stride, uint32_t w, uint32_t h, uint32_t n, const uint8_t* qp_of_frame) {
    if (!c) return AMVHIP_ERR_ARG;
    int qp;
    if (int r = pp_args_ok(c, "postprocess", fmt, mode, w, h, &qp)) return r;
    const PixPicture hs = make_picture(src0, src1, src2, src_stride, src_c_stride, src_frame_stride, src_c_frame_stride);
    const PixPicture hd = make_picture(dst0, dst1, dst2, dst_stride, dst_c_stride, dst_frame_stride, dst_c_frame_stride);
    for (uint32_t i = 0; i < 3; ++i)
        for (uint32_t k = 0; k < 3; ++k) {
            if (!hs.p[i] || !hd.p[k]) return fail(c, AMVHIP_ERR_ARG, "postprocess: null plane");
            uintptr_t s0, s1, d0, d1;
            plane_span(fmt, hs, i, w, h, n, &s0, &s1);
            plane_span(fmt, hd, k, w, h, n, &d0, &d1);
            if (s0 < d1 && d0 < s1) return fail(c, AMVHIP_ERR_ARG, "postprocess: source and destination overlap");
        }
    for (uint32_t i = 0; qp_of_frame && i < n; ++i)
        if (qp_of_frame[i] > 63) return fail(c, AMVHIP_ERR_ARG, "postprocess: QP %u of frame %u is above 63", qp_of_frame[i], i);
    // the staged planes are tight (rows of exactly the row's bytes, planes 16-byte aligned): what the kernel asks for
    return host_staged(c, "postprocess", fmt, hs, fmt, hd, w, h, n, [&](const PixPicture& ds, const PixPicture& dd, hipStream_t st) {
        const uint8_t* d_qp = nullptr;
        if (qp_of_frame) {
            if (int r = stage(c, c->h_aux, n, qp_of_frame, n, st)) return r;
            d_qp = (const uint8_t*)c->h_aux.p;
        }
        return pp_launch(c, mode, qp, ds, dd, w, h, n, d_qp, st);
    });
}

// the decoder of the patched FFmpeg, the postprocessing, then the planes or img_convert: amvhip_decode_lowres_batch_dev's route
extern "C" int amvhip_decode_pp_batch_dev(amvhip_ctx* c, const uint8_t* d_blob, uint64_t blob_bytes, const uint64_t* d_offs, const uint32_t* d_lens,
                                          uint32_t n, uint32_t w, uint32_t h, uint32_t flags, int dst_fmt, uint8_t* d_out, uint32_t out_stride,
                                          int32_t* d_status, const amvhip_pp_mode* mode, const uint8_t* d_qp, void* stream) {
    if (!c) return AMVHIP_ERR_ARG;
    if (!(flags & AMVHIP_FLAG_FFMPEG)) return fail(c, AMVHIP_ERR_ARG, "decode_pp: AMVHIP_FLAG_FFMPEG is required (the planes are that decoder's)");
    if (flags & AMVHIP_FLAG_FFMPEG_KEEP) return fail(c, AMVHIP_ERR_ARG, "decode_pp: AMVHIP_FLAG_FFMPEG_KEEP needs the caller's planes; d_out is not in plane form");
    const bool planes_out = dst_fmt == AMVHIP_PIX_YUVJ420P;
    if (!planes_out && pix_route(AMVHIP_PIX_YUVJ420P, dst_fmt) == kRouteNone)
        return fail(c, AMVHIP_ERR_ARG, "decode_pp: no one-step route from YUVJ420P to format %d", dst_fmt);
    int qp;
    if (int r = pp_args_ok(c, "decode_pp", AMVHIP_PIX_YUVJ420P, mode, w, h, &qp)) return r;
    if (int r = decode_args_ok(c, d_blob, d_offs, d_lens, n, w, h, flags, d_out, d_status)) return r;
    if (planes_out ? out_stride != w : out_stride < w * pix_bpp(dst_fmt))
        return fail(c, AMVHIP_ERR_ARG, "decode_pp: out_stride below the row (YUVJ420P: it must equal the width)");
    const uint64_t out_frame = amvhip_pix_frame_bytes(dst_fmt, out_stride, h);
    PixPicture dst = make_picture(d_out, nullptr, nullptr, out_stride, (out_stride + 1) / 2, out_frame, out_frame);
    if (dst_fmt == AMVHIP_PIX_YUV420P) {
        dst.p[1] = d_out + (uint64_t)out_stride * h;
        dst.p[2] = dst.p[1] + (uint64_t)dst.stride[1] * ((h + 1) / 2);
    }
    if (n == 0) return AMVHIP_OK;
    if (int r = use_device(c)) return r;
    std::lock_guard<std::mutex> lk(c->mu);
    hipStream_t st = (hipStream_t)stream;
    const uint64_t fb = amvhip_yuv420_frame_bytes(w, h);
    if (int r = ensure(c, c->pix_dec, fb * n)) return r;
    if (!planes_out)
        if (int r = ensure(c, c->pp_planes, fb * n)) return r;
    if (int r = decode_core(c, d_blob, blob_bytes, d_offs, d_lens, n, w, h, flags, (uint8_t*)c->pix_dec.p, d_status, c->set[0], st, st)) return r;
    const PixPicture decoded = tight_420((uint8_t*)c->pix_dec.p, w, h), cleaned = tight_420(planes_out ? d_out : (uint8_t*)c->pp_planes.p, w, h);
    if (int r = pp_launch(c, mode, qp, decoded, cleaned, w, h, n, d_qp, st)) return r;
    if (planes_out) return AMVHIP_OK;
    return convert_launch(c, AMVHIP_PIX_YUVJ420P, cleaned, dst_fmt, dst, w, h, n, st);
}
