// amv_host_plan.h -- the host side's arithmetic: table images, buffer sizes, filter banks, pixel-format routes.
//
// Plain C++ that no device call enters, so that a CPU program can walk it (tests/c/host_plan_test.cc).  The files of
// the C ABI take the sizes and the tables they hand to the kernels from here.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/amvhip.h"
#include "amv_segment.h"
#include "amv_tables.h"

namespace amv {

inline int size_ok(uint32_t w, uint32_t h) { return w > 0 && h > 0 && w <= AMVHIP_MAX_DIM && h <= AMVHIP_MAX_DIM; }

// ---- table images ---------------------------------------------------------------------------

inline const uint8_t* symbols_of(int t) {
    return t < 2 ? kHuffDcSymbols : (t == 2 ? kHuffAcLumaSymbols : kHuffAcChromaSymbols);
}

// canonical code assignment of JPEG Annex C (what AmvJpeg.c:1454-1481 and mjpeg.c:129-147 both
// derive): codes of each length are consecutive, and the first code of length l+1 is
// (last code of length l + 1) << 1
inline void build_images(HuffDecodeImage& dec, HuffEncodeImage& enc) {
    memset(&dec, 0, sizeof dec);
    memset(&enc, 0, sizeof enc);
    int pages = 0;
    for (int t = 0; t < 4; ++t) {
        const uint8_t* syms = symbols_of(t);
        uint32_t code = 0;
        int k = 0;
        for (int len = 1; len <= 16; ++len) {
            for (int j = 0; j < kHuffCount[t][len - 1]; ++j, ++code) {
                const uint32_t sym = syms[k++];
                enc.code[t][sym] = code | ((uint32_t)len << 16);
                const uint16_t entry = (uint16_t)(sym | ((uint32_t)len << 8));
                if (len <= kLut1Bits) {
                    const uint32_t lo = code << (kLut1Bits - len);
                    for (uint32_t x = 0; x < (1u << (kLut1Bits - len)); ++x) dec.l1[t][lo + x] = entry;
                } else {
                    const int rest = len - kLut1Bits;  // 1..7
                    const uint32_t prefix = code >> rest;
                    if (!(dec.l1[t][prefix] & 0x8000u)) dec.l1[t][prefix] = (uint16_t)(0x8000u | (uint32_t)pages++);
                    const uint32_t page = dec.l1[t][prefix] & 0xffu;
                    const uint32_t lo = (code & ((1u << rest) - 1u)) << (kLut2Bits - rest);
                    for (uint32_t x = 0; x < (1u << (kLut2Bits - rest)); ++x) dec.l2[page][lo + x] = entry;
                }
            }
            code <<= 1;
        }
    }
    if (pages > kLut2Pages) abort();  // static property of the K.3 tables (11 pages)
    // the one-lane-per-frame walk's form (amv_tables.h)
    auto fast = [](uint16_t e, int t) -> uint32_t {
        const uint32_t len = (e >> 8) & 31u, sym = e & 0xffu, size = sym & 15u;
        if (len == 0) return kFastInvalid | (1u << 24);   // one bit used, no advance: what a guessed start does with it
        const bool dc = t < 2;
        const uint32_t adv = dc ? 1u : (sym == 0 ? kFastEobAdvance : (sym >> 4) + 1u);
        return size | ((dc || size) ? kFastEmit : 0u) | (adv << 16) | ((len + size) << 24);
    };
    for (int t = 0; t < 4; ++t) {
        for (int i = 0; i < (1 << kLut1Bits); ++i) {
            const uint16_t e = dec.l1[t][i];
            dec.fast[t][i] = (e & 0x8000u) ? 0u : fast(e, t);
        }
        for (uint32_t w16 = kFastLongFirst; w16 < 0x10000u; ++w16) {
            const uint16_t e1 = dec.l1[t][w16 >> (16 - kLut1Bits)];
            if (e1 & 0x8000u)
                dec.fast[t][kFastM2Word + 1u + (w16 - kFastLongFirst)] =
                    fast(dec.l2[e1 & 0xffu][(w16 >> (16 - kLut1Bits - kLut2Bits)) & ((1u << kLut2Bits) - 1u)], t);
        }
    }
}

// The image as the device gets it: kFastBigAc on the entries of the two AC tables with ten magnitude bits or more
// (amv_tables.h).  A step of its own behind build_images, whose image stays the documented entry and nothing else.
inline void mark_big_ac(HuffDecodeImage& dec) {
    for (int t = 2; t < 4; ++t)
        for (uint32_t& e : dec.fast[t])
            if ((e & 15u) >= 10u) e |= kFastBigAc;   // (the size field; "no such code" and end-of-block have 0 there)
}

// ---- video decode: what the entropy stage of n frames in blob_bytes of chunks is given -------------------------------

struct EntropyPlan {
    uint64_t ws_lines;    // 16-byte pieces of the unstuffed scans' workspace
    uint32_t hi_rec;      // most record words a frame gets
    uint32_t add_rec;     // record words a frame gets on top of two per byte of its chunk
    uint64_t cap_lines;   // 128-byte lines of the record space
    uint32_t segs;        // MCU-row segments per frame
};

inline EntropyPlan entropy_plan(uint32_t n, uint64_t blob_bytes, const FrameGeom& g) {
    EntropyPlan p;
    // Window per frame for the unstuffed scan in the global workspace: the frame's own chunk length + the zeroed tail of its
    // last 16-byte piece + a piece of slack, in 16-byte pieces laid out on the device (round 4; 5/16 byte per pixel for every
    // frame before: a chunk over 1.6x the usual size went to the serial kernel, the others used 60 % of their window).  The
    // total is bounded by what the chunks occupy; chunks that overlap in the blob make the layout run out, and the frames
    // past its end take the serial kernel.
    p.ws_lines = (blob_bytes + (uint64_t)n * 48u) / 16u + 4u;
    if (p.ws_lines > 0xffffffffull) p.ws_lines = 0xffffffffull;
    // Between the two stages coefficients travel as records (one word per DC and per non-zero AC coefficient), every frame
    // in space of its own, sized from ITS chunk (round 4; one stride for all, from the batch's mean chunk, before: a heavy
    // frame in a light stream was silently decoded by the one-lane serial kernel).  A record costs at least 3 bits of scan,
    // in practice ~6, and every block has a DC symbol and (nearly always) an end-of-block symbol, which take a slot each in
    // the one-lane kernel's stride-aligned form: 2 words per byte of chunk + 2 per block + a stride's slack (never more than a
    // frame with every coefficient non-zero could fill; a frame denser than 2 records per byte goes to the serial kernel), in
    // whole 128-byte lines.  The space is laid out on
    // the device (the lengths are there); its total is bounded here by what the chunks occupy (chunks that overlap make the
    // sum larger than that: the layout saturates and the frames past the end are handed to the serial kernel).
    p.hi_rec = (g.blocks * 66u + 95u) & ~31u;   // every coefficient of every block non-zero, an end-of-block slot each
    p.add_rec = g.blocks * 2u + 64u;
    p.cap_lines = (uint64_t)n * (p.hi_rec / 32u);
    const uint64_t by_stream = (2u * blob_bytes + (uint64_t)n * (p.add_rec + 31u)) / 32u + 1u;
    if (by_stream < p.cap_lines) p.cap_lines = by_stream;
    if (p.cap_lines > 0xffffffffull) p.cap_lines = 0xffffffffull;
    p.segs = segs_per_row(g) * g.mcu_rows;
    return p;
}

// Frames per round of a fall-back route (the context keeps a round's worth of dense coefficient lines): the whole batch
// up to `most` frames, beyond `parts` times that a `parts`-th of it, else `most`.  Never more than 2 GB of lines, though,
// nor fewer than 64 frames: at 640x480 a block line is 128 bytes x 7 200 blocks, and 16 384 frames of that would be 15 GB
// kept for rounds that usually find nothing.
inline uint32_t fallback_round(uint32_t n, const FrameGeom& g, uint32_t most, uint32_t parts) {
    uint32_t round = n <= most ? n : (n / parts > most ? (n + parts - 1u) / parts : most);
    const uint64_t by_bytes = (2ull << 30) / ((uint64_t)g.blocks * 128u);
    if (round > by_bytes) round = by_bytes > 64u ? (uint32_t)by_bytes : 64u;
    return round < n ? round : n;
}

// ---- reduced-size decode (lowres 1..3: pictures of 1/2, 1/4, 1/8 the size) ---------------------------------------------

// what avcodec_set_dimensions makes of a size (utils.c:141-142): ceil(full / 2^lowres); 0 for lowres > 3
inline uint32_t lowres_dim(uint32_t full, uint32_t lowres) { return lowres > 3u ? 0u : (full + (1u << lowres) - 1u) >> lowres; }

// the three tight planes of a reduced picture: Y W_L x H_L, then Cb, Cr of (W_L + 1) / 2 x (H_L + 1) / 2
inline uint64_t lowres_frame_bytes(uint32_t w, uint32_t h, uint32_t lowres) {
    if (lowres > 3u) return 0;
    const uint64_t wl = lowres_dim(w, lowres), hl = lowres_dim(h, lowres);
    return wl * hl + 2u * ((wl + 1u) / 2u) * ((hl + 1u) / 2u);
}

// the full-size start row of a component (mjpegdec.c:675): canvas row r lands at plane row start - r
inline int ffmpeg_start_row(uint32_t height, bool chroma) {
    const uint32_t mcu_rows = (height + 15u) / 16u;
    return (chroma ? 1 : 2) * (int)(8u * mcu_rows - ((height >> 1) & 7u)) - 1;
}

// ... scaled down: reduced canvas row r_L (= full-size canvas row >> lowres) lands at plane row lowres_start_row - r_L.
// start + 1 is the count of plane rows the full-size formula can reach; the reduced count is that, rounded up.
inline int lowres_start_row(uint32_t height, uint32_t lowres, bool chroma) {
    return ((ffmpeg_start_row(height, chroma) + 1 + (1 << lowres) - 1) >> lowres) - 1;
}

// rows of a reduced plane
inline uint32_t lowres_plane_rows(uint32_t height, uint32_t lowres, bool chroma) {
    const uint32_t hl = lowres_dim(height, lowres);
    return chroma ? (hl + 1u) / 2u : hl;
}

// plane rows 0 .. lowres_rows_reached - 1 are the ones the rule sends a canvas row to.  All of them for h % 16 <= 8; the
// other heights leave the bottom rows of the plane without a canvas row, as the full-size formula does (the caller
// clears the output first: lowres_store_covers_planes)
inline uint32_t lowres_rows_reached(uint32_t height, uint32_t lowres, bool chroma) {
    const uint32_t rows = lowres_plane_rows(height, lowres, chroma);
    const int reach = lowres_start_row(height, lowres, chroma) + 1;
    return reach < (int)rows ? (uint32_t)(reach > 0 ? reach : 0) : rows;
}

inline bool lowres_store_covers_planes(uint32_t height, uint32_t lowres) {
    return lowres_rows_reached(height, lowres, false) == lowres_plane_rows(height, lowres, false) &&
           lowres_rows_reached(height, lowres, true) == lowres_plane_rows(height, lowres, true);
}

// ---- picture rescale --------------------------------------------------------------------------

// av_build_filter(filter, factor, NB_TAPS = 4, NB_PHASES = 16, 1 << FILTER_BITS, type 0) -- libavcodec/resample2.c:93-140
// as img_resample_full_init calls it (imgresample.c:468-471): cubic, first-order derivative -0.5, every phase
// normalised to 256; host arithmetic in double / float exactly as there.
inline void build_resample_filter(int16_t* filter, uint32_t out_size, uint32_t in_size) {
    double factor = (float)out_size / (float)in_size;
    if (factor > 1.0) factor = 1.0;                          // upsampling only interpolates
    for (int ph = 0; ph < 16; ++ph) {
        double tab[4], norm = 0;
        for (int i = 0; i < 4; ++i) {
            const float d = -0.5f;
            const double x = fabs(((double)(i - 1) - (double)ph / 16) * factor);
            const double y = x < 1.0 ? 1 - 3 * x * x + 2 * x * x * x + d * (-x * x + x * x * x)
                                     : d * (-4 + 8 * x - 5 * x * x + x * x * x);
            tab[i] = y;
            norm += y;
        }
        for (int i = 0; i < 4; ++i) {
            const long v = lrintf((float)(tab[i] * 256 / norm));
            filter[ph * 4 + i] = (int16_t)(v < -32768 ? -32768 : (v > 32767 ? 32767 : v));
        }
    }
}

// the 16.16 step through the source per destination sample (imgresample.c:465-466)
inline int resample_incr(uint32_t src_size, uint32_t dst_size) { return (int)(((uint64_t)src_size << 16) / dst_size); }

// ---- pixel formats: the routes of img_convert ---------------------------------------------------------

enum PixRoute { kRouteNone = 0, kRoutePlanes, kRouteGray, kRoutePackedIn, kRoutePackedOut, kRouteRgbIn, kRouteRgbOut };

inline bool pix_planar_yuv(int f) { return f >= AMVHIP_PIX_YUV420P && f <= AMVHIP_PIX_YUVJ444P; }
inline bool pix_jpeg(int f) { return f == AMVHIP_PIX_YUVJ420P || f == AMVHIP_PIX_YUVJ422P || f == AMVHIP_PIX_YUVJ444P; }
inline bool pix_420(int f) { return f == AMVHIP_PIX_YUV420P || f == AMVHIP_PIX_YUVJ420P; }
inline bool pix_444(int f) { return f == AMVHIP_PIX_YUV444P || f == AMVHIP_PIX_YUVJ444P; }
inline uint32_t pix_bpp(int f) {   // bytes per pixel of plane 0
    switch (f) {
        case AMVHIP_PIX_YUYV422: case AMVHIP_PIX_UYVY422: case AMVHIP_PIX_RGB565: case AMVHIP_PIX_RGB555: return 2;
        case AMVHIP_PIX_RGB24: case AMVHIP_PIX_BGR24: return 3;
        case AMVHIP_PIX_RGB32: return 4;
        default: return 1;
    }
}

// the routes the reference reaches in one step: a routine of convert_table (imgconvert.c:1940-2190), the planar route
// (:2415-2513) or the gray route (:2399-2413)
inline PixRoute pix_route(int src, int dst) {
    if (src < 0 || src >= AMVHIP_PIX_COUNT || dst < 0 || dst >= AMVHIP_PIX_COUNT || src == dst) return kRouteNone;
    if (pix_planar_yuv(src) && pix_420(dst)) return kRoutePlanes;
    if (pix_420(src) && dst == AMVHIP_PIX_GRAY8) return kRouteGray;
    if ((src == AMVHIP_PIX_YUYV422 || src == AMVHIP_PIX_UYVY422) && dst == AMVHIP_PIX_YUV420P) return kRoutePackedIn;
    if (src == AMVHIP_PIX_YUV420P && (dst == AMVHIP_PIX_YUYV422 || dst == AMVHIP_PIX_UYVY422)) return kRoutePackedOut;
    if ((src == AMVHIP_PIX_RGB24 || src == AMVHIP_PIX_BGR24 || src == AMVHIP_PIX_RGB32) && dst == AMVHIP_PIX_YUV420P) return kRouteRgbIn;
    if (src == AMVHIP_PIX_RGB24 && dst == AMVHIP_PIX_YUVJ420P) return kRouteRgbIn;
    if (pix_420(src) && (dst == AMVHIP_PIX_RGB24 || dst == AMVHIP_PIX_BGR24 || dst == AMVHIP_PIX_RGB32 || dst == AMVHIP_PIX_RGB565 ||
                         dst == AMVHIP_PIX_RGB555))
        return kRouteRgbOut;
    return kRouteNone;
}

// rows and bytes per row of plane p of a w x h picture; rows 0: the format has no such plane.  4:2:0 chroma rounds up (what
// the decoder makes, mjpegdec.c:312); a to-4:2:0 route from another sampling wants even sizes anyway
inline void pix_plane_size(int f, uint32_t p, uint32_t w, uint32_t h, uint32_t* row_bytes, uint32_t* rows) {
    *row_bytes = 0;
    *rows = 0;
    if (p == 0) { *row_bytes = w * pix_bpp(f); *rows = h; return; }
    if (!pix_planar_yuv(f)) return;
    *row_bytes = pix_444(f) ? w : (w + 1) / 2;
    *rows = pix_420(f) ? (h + 1) / 2 : h;
}

// what a pair asks of the picture size (0: refused)
inline int pix_size_ok(int src_fmt, int dst_fmt, uint32_t w, uint32_t h) {
    if (!size_ok(w, h)) return 0;
    const PixRoute r = pix_route(src_fmt, dst_fmt);
    const bool any = r == kRouteGray || r == kRouteRgbOut || (r == kRoutePlanes && pix_420(src_fmt));
    return any || (!(w & 1) && !(h & 1));
}

// bytes of one frame: plane 0 with rows `stride` apart, the chroma planes (if any) behind it at their own width
inline uint64_t pix_frame_bytes(int fmt, uint32_t stride, uint32_t height) {
    if (fmt < 0 || fmt >= AMVHIP_PIX_COUNT) return 0;
    if (!pix_planar_yuv(fmt)) return (uint64_t)stride * height;
    const uint64_t cs = pix_444(fmt) ? stride : (stride + 1) / 2, cr = pix_420(fmt) ? (height + 1) / 2 : height;
    return (uint64_t)stride * height + 2 * cs * cr;
}

// ---- `-psnr`: from summed squared errors to the figures ffmpeg prints ---------------------------------------------------

// psnr() of ffmpeg.c:849-852 on d = sse / (samples * 255^2): INFINITY at d == 0; NaN where there are no samples
inline double psnr_db(uint64_t sse, uint64_t samples) {
    if (samples == 0) return NAN;
    const double d = (double)sse / ((double)samples * 255.0 * 255.0);
    if (d == 0) return INFINITY;
    return -10.0 * log(d) / log(10.0);
}

// the last-report line of ffmpeg.c:953-972 over n frames of width x height whose plane errors are sse[n][3]: Y, U, V and *
// (the summed errors over the summed scales).  The luma scale is width * height * 255^2 * n, a chroma scale a quarter of it.
inline void psnr_report(const uint64_t* sse, uint32_t n, uint32_t width, uint32_t height, double out[4]) {
    double error_sum = 0, scale_sum = 0;
    for (int j = 0; j < 3; ++j) {
        uint64_t e = 0;
        for (uint32_t i = 0; i < n; ++i) e += sse[(size_t)i * 3 + j];
        const double error = (double)e;
        double scale = (double)((uint64_t)width * height) * 255.0 * 255.0 * n;
        if (j) scale /= 4;
        error_sum += error;
        scale_sum += scale;
        out[j] = scale == 0 ? NAN : (error == 0 ? INFINITY : -10.0 * log(error / scale) / log(10.0));
    }
    out[3] = scale_sum == 0 ? NAN : (error_sum == 0 ? INFINITY : -10.0 * log(error_sum / scale_sum) / log(10.0));
}

// what amvhip_picture_sse_dev takes: the six planar YUV formats, GRAY8, RGB24 and BGR24, at every size the decoder takes
inline int picture_sse_ok(int fmt, uint32_t w, uint32_t h) {
    const bool listed = pix_planar_yuv(fmt) || fmt == AMVHIP_PIX_GRAY8 || fmt == AMVHIP_PIX_RGB24 || fmt == AMVHIP_PIX_BGR24;
    return listed && size_ok(w, h);
}

// ---- video front end: deinterlace, crop, rescale / convert, pad (pre_process_video_frame + do_video_out) --------------

// avpicture_deinterlace's own list (imgconvert.c:2824-2831) among our formats; the YUVJ formats are not in it
inline int deinterlace_ok(int fmt, uint32_t w, uint32_t h) {
    const bool listed = fmt == AMVHIP_PIX_YUV420P || fmt == AMVHIP_PIX_YUV422P || fmt == AMVHIP_PIX_YUV444P || fmt == AMVHIP_PIX_GRAY8;
    return listed && size_ok(w, h) && !(w & 3) && !(h & 3);
}

// opt_pad_color (ffmpeg.c:2246-2271): RGB_TO_Y / _U / _V with shift 0 on r = rgb >> 16 (unmasked, as there), the ints
// then written as bytes by av_picture_pad's memset
inline void pad_color_from_rgb(uint32_t rrggbb, uint8_t out[3]) {
    auto fix = [](double x) { return (int)(x * 1024 + 0.5); };
    const int r = (int)(rrggbb >> 16), g = (int)((rrggbb >> 8) & 255u), b = (int)(rrggbb & 255u);
    out[0] = (uint8_t)((fix(0.29900) * r + fix(0.58700) * g + fix(0.11400) * b + 512) >> 10);
    out[1] = (uint8_t)(((-fix(0.16874) * r - fix(0.33126) * g + fix(0.50000) * b + 511) >> 10) + 128);
    out[2] = (uint8_t)(((fix(0.50000) * r - fix(0.41869) * g - fix(0.08131) * b + 511) >> 10) + 128);
}

// chroma shifts of a planar YUV format (pix_fmt_info's x_chroma_shift / y_chroma_shift); 0, 0 for the others
inline uint32_t pix_xshift(int f) { return pix_planar_yuv(f) && !pix_444(f) ? 1u : 0u; }
inline uint32_t pix_yshift(int f) { return pix_420(f) ? 1u : 0u; }

struct FrontRect { uint32_t x, y, w, h; };   // samples of one plane

enum FrontRefusal { kFrontOk = 0, kFrontOddBand, kFrontCropNotPlanar, kFrontCropTooLarge, kFrontPadTooLarge, kFrontOddTarget, kFrontNoRoute };

inline const char* front_refusal_text(int r) {
    switch (r) {
        case kFrontOddBand: return "crop and pad bands are even";
        case kFrontCropNotPlanar: return "only planar YUV sources are cropped (av_picture_crop)";
        case kFrontCropTooLarge: return "the crop bands leave less than 2x2 of the source";
        case kFrontPadTooLarge: return "the pad bands leave a window of less than 2x2";
        case kFrontOddTarget: return "bad source or target size (the target's width and height are even)";
        case kFrontNoRoute: return "the shim has no route from the source format to YUVJ420P at these sizes";
        default: return "";
    }
}

struct FrontPlan {
    int refusal;                 // kFrontOk: the rest is valid
    bool deinterlace;            // the stage runs (asked for and avpicture_deinterlace takes the format and size)
    bool crop, pad;
    bool rescale;                // ffmpeg.c:1653-1659: the sizes or the format differ -> sws_scale; else the copy route
    uint32_t src_planes;         // planes of the source format
    uint32_t crop_w, crop_h;     // the rescaler's source size
    uint32_t win_w, win_h;       // the rescaler's target size
    FrontRect src_full[3];       // x = y = 0: the source planes (w in bytes of a row)
    FrontRect src_win[3];        // what the crop keeps of them
    FrontRect dst_full[3];       // the encoder's YUVJ420P planes
    FrontRect dst_win[3];        // the window the rescaler (or the copy) fills; the rest of dst_full is bands
    uint64_t deint_frame_bytes;  // workspace per frame: the deinterlaced window, tight, planes 16-byte aligned (0: stage off)
    uint64_t deint_plane_off[3];
    uint64_t padded_frame_bytes; // workspace per frame of the encoder's picture (tight YUV420P layout)
};

// every band of *fe zero (fe == NULL too)
inline bool front_is_identity(const amvhip_frontend* fe) {
    return !fe || !(fe->deinterlace | fe->crop_top | fe->crop_bottom | fe->crop_left | fe->crop_right | fe->pad_top | fe->pad_bottom |
                    fe->pad_left | fe->pad_right);
}

// the shim's own demands on a pair of sizes towards YUVJ420P (what amvhip_sws_scale_dev checks before it looks at pointers)
inline bool front_shim_ok(int src_fmt, uint32_t sw, uint32_t sh, uint32_t dw, uint32_t dh) {
    if (src_fmt < 0 || src_fmt >= AMVHIP_PIX_COUNT || !size_ok(sw, sh) || !size_ok(dw, dh)) return false;
    if (sw == dw && sh == dh)
        return src_fmt == AMVHIP_PIX_YUVJ420P || (pix_route(src_fmt, AMVHIP_PIX_YUVJ420P) != kRouteNone && pix_size_ok(src_fmt, AMVHIP_PIX_YUVJ420P, dw, dh));
    if (sw < 2 || sh < 2 || dw < 2 || dh < 2) return false;
    return src_fmt == AMVHIP_PIX_YUV420P || (pix_route(src_fmt, AMVHIP_PIX_YUV420P) != kRouteNone && pix_size_ok(src_fmt, AMVHIP_PIX_YUV420P, sw, sh));
}

inline FrontPlan front_plan(int src_fmt, uint32_t src_w, uint32_t src_h, const amvhip_frontend* fe, uint32_t width, uint32_t height) {
    static const amvhip_frontend none = {};
    const amvhip_frontend& f = fe ? *fe : none;
    FrontPlan p;
    memset(&p, 0, sizeof p);
    auto refuse = [&p](int why) { p.refusal = why; return p; };
    if (src_fmt < 0 || src_fmt >= AMVHIP_PIX_COUNT || !size_ok(src_w, src_h) || !size_ok(width, height) || (width & 1) || (height & 1))
        return refuse(kFrontOddTarget);
    if ((f.crop_top | f.crop_bottom | f.crop_left | f.crop_right | f.pad_top | f.pad_bottom | f.pad_left | f.pad_right) & 1u) return refuse(kFrontOddBand);
    p.crop = (f.crop_top | f.crop_bottom | f.crop_left | f.crop_right) != 0;
    p.pad = (f.pad_top | f.pad_bottom | f.pad_left | f.pad_right) != 0;
    if (p.crop && !pix_planar_yuv(src_fmt)) return refuse(kFrontCropNotPlanar);
    if ((uint64_t)f.crop_top + f.crop_bottom + 2u > src_h || (uint64_t)f.crop_left + f.crop_right + 2u > src_w) return refuse(kFrontCropTooLarge);
    if ((uint64_t)f.pad_top + f.pad_bottom + 2u > height || (uint64_t)f.pad_left + f.pad_right + 2u > width) return refuse(kFrontPadTooLarge);
    p.crop_w = src_w - f.crop_left - f.crop_right;
    p.crop_h = src_h - f.crop_top - f.crop_bottom;
    p.win_w = width - f.pad_left - f.pad_right;
    p.win_h = height - f.pad_top - f.pad_bottom;
    if (!front_shim_ok(src_fmt, p.crop_w, p.crop_h, p.win_w, p.win_h)) return refuse(kFrontNoRoute);
    p.rescale = p.crop_w != p.win_w || p.crop_h != p.win_h || src_fmt != AMVHIP_PIX_YUVJ420P;
    p.deinterlace = f.deinterlace && deinterlace_ok(src_fmt, src_w, src_h);
    const uint32_t xs = pix_xshift(src_fmt), ys = pix_yshift(src_fmt);
    for (uint32_t i = 0; i < 3; ++i) {
        uint32_t rb, rows;
        pix_plane_size(src_fmt, i, src_w, src_h, &rb, &rows);
        if (!rows) continue;
        p.src_planes = i + 1;
        p.src_full[i] = FrontRect{0, 0, rb, rows};
        if (!p.crop) { p.src_win[i] = p.src_full[i]; continue; }
        // av_picture_crop (imgconvert.c:2236-2238): the origin moves by the band >> shift; the size is the cropped picture's plane
        uint32_t wb, wr;
        pix_plane_size(src_fmt, i, p.crop_w, p.crop_h, &wb, &wr);
        p.src_win[i] = FrontRect{i ? f.crop_left >> xs : f.crop_left, i ? f.crop_top >> ys : f.crop_top, wb, wr};
    }
    for (uint32_t i = 0; i < 3; ++i) {
        const uint32_t s = i ? 1u : 0u;
        p.dst_full[i] = FrontRect{0, 0, width >> s, height >> s};
        p.dst_win[i] = FrontRect{f.pad_left >> s, f.pad_top >> s, p.win_w >> s, p.win_h >> s};
    }
    if (p.deinterlace) {
        uint64_t off = 0;
        for (uint32_t i = 0; i < p.src_planes; ++i) {
            p.deint_plane_off[i] = off;
            off += ((uint64_t)p.src_win[i].w * p.src_win[i].h + 15u) & ~15ull;
        }
        p.deint_frame_bytes = off;
    }
    p.padded_frame_bytes = (uint64_t)width * height + 2ull * (width / 2) * (height / 2);
    return p;
}

// The bands of one padded plane as items of up to four bytes, for amv_pad_bands_kernel: the rows above and below the window
// whole (ceil(W / 4) items a row), then the columns left and right of the window on its own rows.  Host and device count
// and place them with these functions.
struct PadPlane {
    uint32_t W, H;               // the plane
    uint32_t wx, wy, ww, wh;     // the window inside it
    uint32_t color;              // the byte, four times over
};
struct PadItem { uint32_t row, col, len; };
#if defined(__HIPCC__)
#define AMV_HD __host__ __device__
#else
#define AMV_HD
#endif
AMV_HD inline uint32_t pad_items(const PadPlane& q) {
    const uint32_t right = q.W - q.wx - q.ww;
    return (q.H - q.wh) * ((q.W + 3u) >> 2) + q.wh * (((q.wx + 3u) >> 2) + ((right + 3u) >> 2));
}
AMV_HD inline PadItem pad_item(const PadPlane& q, uint32_t t) {
    const uint32_t per_row = (q.W + 3u) >> 2, full = (q.H - q.wh) * per_row;
    if (t < full) {
        const uint32_t r = t / per_row, k = t - r * per_row, col = 4u * k;
        return PadItem{r < q.wy ? r : r + q.wh, col, q.W - col < 4u ? q.W - col : 4u};
    }
    t -= full;
    const uint32_t right = q.W - q.wx - q.ww, nl = (q.wx + 3u) >> 2, per = nl + ((right + 3u) >> 2);
    const uint32_t r = t / per, k = t - r * per;
    if (k < nl) return PadItem{q.wy + r, 4u * k, q.wx - 4u * k < 4u ? q.wx - 4u * k : 4u};
    const uint32_t off = 4u * (k - nl);
    return PadItem{q.wy + r, q.wx + q.ww + off, right - off < 4u ? right - off : 4u};
}

// ---- audio resample -----------------------------------------------------------------------------

constexpr uint32_t kBankPhases = 1024;   // kAudioPhases of amv_kernels.h (the audio entry points assert that they agree)

// av_resample_init (resample2.c:183-190) as audio_resample_init calls it (resample.c:165): 16 taps, cutoff 0.8
inline uint32_t audio_filter_length(uint32_t in_rate, uint32_t out_rate) {
    const double f = out_rate * 0.8 / in_rate, factor = f > 1.0 ? 1.0 : f;
    const int fl = (int)ceil(16 / factor);
    return fl > 1 ? (uint32_t)fl : 1u;
}

inline int64_t audio_index0(uint32_t fl) { return -(int64_t)kBankPhases * ((fl - 1) / 2); }

inline double kaiser_bessel(double x) {   // bessel() of resample2.c:74-85
    double v = 1, t = 1;
    x = x * x / 4;
    for (int i = 1; i < 50; i++) {
        t *= x / (i * i);
        v += t;
    }
    return v;
}

// av_build_filter(filter, factor, fl, 1024, 1 << 15, 9) -- resample2.c:93-139, the Kaiser sibling of build_resample_filter:
// same double / float operations in the same order; rows padded with zero taps to fl_pad
inline void build_audio_bank(std::vector<int16_t>& bank, uint32_t in_rate, uint32_t out_rate, uint32_t fl, uint32_t fl_pad) {
    const double f = out_rate * 0.8 / in_rate;
    const double factor = f > 1.0 ? 1.0 : f;
    const int center = ((int)fl - 1) / 2;
    std::vector<double> tab(fl);
    bank.assign((size_t)kBankPhases * fl_pad, 0);
    for (int ph = 0; ph < (int)kBankPhases; ph++) {
        double norm = 0;
        for (int i = 0; i < (int)fl; i++) {
            const double x = M_PI * ((double)(i - center) - (double)ph / (int)kBankPhases) * factor;
            double y = x == 0 ? 1.0 : sin(x) / x;
            const double w = 2.0 * x / (factor * (int)fl * M_PI);
            y *= kaiser_bessel(9 * sqrt(1 - w * w > 0 ? 1 - w * w : 0));
            tab[i] = y;
            norm += y;
        }
        for (int i = 0; i < (int)fl; i++) {
            const long v = lrintf((float)(tab[i] * (1 << 15) / norm));
            bank[(size_t)ph * fl_pad + i] = (int16_t)(v < -32768 ? -32768 : (v > 32767 ? 32767 : v));
        }
    }
}

// the state av_resample leaves after `count` outputs (resample2.c:288-293, :307-316): index and frac move on, the input
// frames the index has passed are consumed (returned)
inline uint64_t audio_advance(int64_t& index, uint64_t& frac, uint64_t count, uint64_t D, uint32_t out_rate) {
    const uint64_t total = frac + count * D;
    int64_t next = index + (int64_t)(total / out_rate);
    frac = total % out_rate;
    const uint64_t consumed = next > 0 ? (uint64_t)next >> 10 : 0;
    if (next >= 0) next &= kBankPhases - 1;
    index = next;
    return consumed;
}

// ---- ADPCM ------------------------------------------------------------------------------------

// launched sweeps of the chained encode of n chunks: until the list is expected to be a couple of hundred entries (it
// starts at ~0.41 n and shrinks ~3.7x per sweep on ordinary audio; counted here as n shrinking 3.3x).  The front sweep
// behind them (a workgroup per entry, four chunks looked ahead) and the one-workgroup settle kernel take the rest
inline uint32_t adpcm_default_sweeps(uint32_t n) {
    uint32_t sweeps = 0;
    for (uint64_t left = n; left > 512u; left = left * 3u / 10u) ++sweeps;
    if (n <= 64u) sweeps = 0u;
    return sweeps;
}

// The trellis stream (amvhip_adpcm_encode_trellis_stream_dev).  A chunk's start is guessed by a search over the end of
// its predecessor's m samples (m even): from the last freeze point but one (adpcm.c:405-417 keeps only the best node at
// samples 127, 255, ...), so that the guess freezes where the real search does -- 129 to 256 samples, 226 of a
// 1378-sample chunk.  On 300 chunks of the synthetic audio that guessed wrong 115 / 87 / 77 / 60 / 48 times at
// N = 1 .. 5, against 128 / 110 / 102 / 87 / 72 for the last 128 samples and 119 / 102 / 94 / 82 / 54 for the last 256
// (CPU model over the oracle).
AMV_HD inline uint32_t adpcm_trellis_tail(uint32_t m) { return m <= 256u ? m : m - ((m + 127u) / 128u - 2u) * 128u; }

// sweeps launched behind the guess pass.  The model's lists of 1378-sample chunks were empty after 2 to 4 sweeps at every
// N; a run of k chunks of a few samples each (their ends follow their starts, and a guess over two samples is no guess)
// takes k sweeps more, and streams with a quarter of their chunks that short needed up to 11.  A sweep over an empty
// list is a launch that leaves at once, so the count is generous; past it the fall-back writes the bytes.
constexpr uint32_t kTrellisSweeps = 16;

// The chain workspace of both encoders (launch_adpcm_stream, launch_adpcm_trellis_stream), n chunks:
//   state[n]       {start the chunk's bytes were coded from, end reached}, exchanged as one 64-bit word;
//   list[2][n]     chunk numbers, the two generations in turn;
//   counters       kChainCounterWords words, named below;
//   bits           (plain route) a bit per chunk: listed already by the front sweep;
//   map[n][96]     the exhaustive route's maps: where each of the 89 starts of a chunk ends;
//   bmap, bstart   (plain route) the composed map and the start index of every block of kChainBlock chunks.
// Counters and bits are what a call zeroes, and they lie together: [zero, zero + zero_bytes), whole 16-byte pieces from
// a 16-byte boundary of the buffer, so that the memset is one fill.
constexpr uint32_t kChainBlock = 256;        // chunks whose maps one workgroup composes through LDS (24 KB)
constexpr uint32_t kChainGenerations = 64;   // list generations (and sweeps) that have a counter word of their own
constexpr uint32_t kChainCounterWords = 2u * kChainGenerations + 4u;   // (need, done and two spare words)
constexpr uint32_t chain_word_list(uint32_t k) { return k; }                           // entries of list generation k
constexpr uint32_t chain_word_recoded(uint32_t k) { return kChainGenerations + k; }    // chunks coded again by sweep k (trellis)
// not zero: the stream is not the sequential encoder's yet, the exhaustive route runs (the chunks it takes on, counted
// from the stream's end -- the trellis fall-back recodes those alone)
constexpr uint32_t kChainWordNeed = 2u * kChainGenerations;
constexpr uint32_t kChainWordDone = kChainWordNeed + 1u;   // workgroups of the plain route's chain kernel that have written their map
// most launched sweeps.  Sweep k reads generation k and appends to k + 1; the plain route's front and settle kernels
// behind its sweeps take two generations more
constexpr uint32_t kAdpcmSweepsMost = 59, kTrellisSweepsMost = 60;
static_assert(kAdpcmSweepsMost + 2u < kChainGenerations && kTrellisSweepsMost + 1u < kChainGenerations, "a counter word per generation");
static_assert(kTrellisSweeps <= kTrellisSweepsMost, "the default is a permitted count");

struct ChainPlan {
    uint64_t state, list[2], counters, bits, map, bmap, bstart;   // byte offsets
    uint64_t zero, zero_bytes;                                    // the span a call zeroes
    uint64_t bytes;                                               // the whole
    uint32_t blocks;                                              // blocks of kChainBlock chunks (0: the trellis route)
};
inline ChainPlan adpcm_chain_plan(uint32_t n, bool blocked) {
    ChainPlan p;
    p.blocks = blocked ? (uint32_t)(((uint64_t)n + kChainBlock - 1u) / kChainBlock) : 0u;
    p.state = 0;
    p.list[0] = (uint64_t)n * 8u;
    p.list[1] = p.list[0] + (uint64_t)n * 4u;
    p.counters = p.list[1] + (uint64_t)n * 4u;
    p.bits = p.counters + kChainCounterWords * 4u;
    p.map = p.bits + (blocked ? (((uint64_t)n + 127u) / 128u) * 16u : 0u);
    p.bmap = p.map + (uint64_t)n * 96u;
    p.bstart = p.bmap + (uint64_t)p.blocks * 96u;
    p.bytes = p.bstart + (uint64_t)p.blocks * 4u;
    p.zero = p.counters;
    p.zero_bytes = p.map - p.counters;
    return p;
}
inline ChainPlan adpcm_plain_chain_plan(uint32_t n) { return adpcm_chain_plan(n, true); }
inline ChainPlan adpcm_trellis_chain_plan(uint32_t n) { return adpcm_chain_plan(n, false); }

// ---- video encode: the rate entries' workspace (amv_rate_plan.h; amvhip_encode.hip: rate_core, probe_core) ---------------
// For n frames of `blocks` blocks and a ladder of `rungs`: the zeroed span -- a row of 32 counters (word p, p = 1 .. rungs - 1:
// the frames redo pass p codes again; word `rungs` takes what the last check appends, which is nothing) and the bits table
// uint32 [n][rungs] -- then the frames' lambdas uint32 [n], the two lists that take turns uint32 [n] each, a probe's copy of the -nr
// state, and the quantised DCs int16 [n][blocks] on their way between the probe's two launches.
struct RatePlan {
    uint64_t counters, bits, lambda, list[2], state, dc;   // byte offsets
    uint64_t zero, zero_bytes;                             // the span a call zeroes
    uint64_t bytes;                                        // the whole
};
inline RatePlan rate_plan(uint32_t n, uint32_t rungs, uint32_t blocks) {
    RatePlan p;
    p.counters = 0;
    p.bits = 32u * 4u;
    p.lambda = p.bits + (uint64_t)n * rungs * 4u;
    p.list[0] = p.lambda + (uint64_t)n * 4u;
    p.list[1] = p.list[0] + (uint64_t)n * 4u;
    p.state = p.list[1] + (uint64_t)n * 4u;
    p.dc = (p.state + 65u * 4u + 15u) & ~15ull;
    p.bytes = p.dc + (uint64_t)n * blocks * 2u;
    p.zero = p.counters;
    p.zero_bytes = p.lambda - p.counters;
    return p;
}

// ---- video encode: what a clip entry's workspace holds beyond the rate plan (amv_clip_plan.h; budget_passes) ---------------
// All of it zeroed by a call: the counters of the passes -- word p, p = 1 .. clip_passes_most - 1: the frames redo pass p codes
// again; the word behind the last takes what the last check and settle append, which is nothing -- the floor sums uint64 [16]
// and the clip's state (ClipState, amv_kernels.h).  The rate plan's own counters lie idle in a clip call.
struct ClipPlan {
    uint64_t counters, F, state;   // byte offsets
    uint64_t bytes;                // the whole
};
inline ClipPlan clip_plan() {
    ClipPlan p;
    p.counters = 0;
    p.F = 160u * 4u;               // >= clip_passes_most(16) + 1 = 137 words
    p.state = p.F + 16u * 8u;
    p.bytes = p.state + 16u;
    return p;
}

}  // namespace amv
