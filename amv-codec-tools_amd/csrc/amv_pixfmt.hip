// amv_pixfmt.hip -- the pixel-format step on both sides of the codec: img_convert of the reference
// (AMVmuxer/ffmpeg/libavcodec/imgconvert.c:2329-2571) for the formats that meet the AMV codec, as the sws_scale shim
// (imgresample.c:599-690) calls it in front of and behind img_resample.
//
// Five streaming byte kernels, one per family of routes:
//   amv_pix_planes_kernel    planar YUV -> planar 4:2:0 (:2415-2513): luma copied, chroma copied or shrunk (shrink12 :1318-1348,
//                            ff_shrink22 :1351-1381), the range tables (:1216-1233, colorspace.h:69-84) on what was written;
//                            also planar YUV -> GRAY8 (:2399-2413) and plane copies
//   amv_pix_packed_in_kernel YUYV422 / UYVY422 -> YUV420P (:867-978): chroma of the even lines
//   amv_pix_packed_out_kernel YUV420P -> YUYV422 / UYVY422 (:1150-1214): a chroma line serves two picture lines
//   amv_pix_rgb_in_kernel    RGB24 / BGR24 / RGB32 -> YUV420P and RGB24 -> YUVJ420P (imgconvert_template.h:218-323, :654-):
//                            10-bit fixed-point luma per pixel, chroma from the 2x2 sums
//   amv_pix_rgb_out_kernel   YUV420P / YUVJ420P -> RGB24 / BGR24 / RGB32 / RGB565 / RGB555 (imgconvert_template.h:30-216)
//
// A lane takes 16 luma columns of one line (planes) or of a pair of lines (the 4:2:0 routes): 16-byte loads and stores
// where a row segment is whole and 16-byte aligned, unaligned dwords where it is whole, single bytes for the ragged last
// segment of a row -- no byte beyond the picture's width and no row beyond its height is read or written.  The four
// 256-entry range tables are affine maps with a clamp, so they are computed in registers (multiply-add, shift, median):
// three VALU operations a byte against a byte gather from LDS that serialises on bank conflicts (profiles/r04_lds_lookup.txt).
#include "amv_kernels.h"

namespace amv {

namespace {

struct __attribute__((packed, aligned(1))) U32u { uint32_t v; };   // a dword at any address

__device__ __forceinline__ uint32_t byte_of(uint32_t w, int k) { return (w >> (8 * k)) & 255u; }
// four values 0..255 side by side, lowest first
__device__ __forceinline__ uint32_t pack4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    const uint32_t lo = __builtin_amdgcn_perm(b, a, 0x0c0c0400u), hi = __builtin_amdgcn_perm(d, c, 0x0c0c0400u);
    return __builtin_amdgcn_perm(hi, lo, 0x05040100u);
}
__device__ __forceinline__ int clamp8(int v) { return min(max(v, 0), 255); }   // the reference's cm[] (ff_cropTbl)

// kWords dwords from p, of which `valid` bytes exist (the rest read as zero)
template <int kWords>
__device__ __forceinline__ void load_words(const uint8_t* p, int valid, uint32_t (&w)[kWords]) {
    if (valid == kWords * 4) {
        if (kWords % 4 == 0 && ((uintptr_t)p & 15u) == 0) {
#pragma unroll
            for (int i = 0; i < kWords / 4; ++i) {
                const uint4 v = ((const uint4*)p)[i];
                w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int i = 0; i < kWords; ++i) w[i] = ((const U32u*)p)[i].v;
        }
    } else {
#pragma unroll
        for (int i = 0; i < kWords; ++i) {
            uint32_t v = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (4 * i + b < valid) v |= (uint32_t)p[4 * i + b] << (8 * b);
            w[i] = v;
        }
    }
}

// the first `valid` bytes of kWords dwords to p; vector stores only
template <int kWords>
__device__ __forceinline__ void store_words(uint8_t* p, int valid, const uint32_t (&w)[kWords]) {
    if (valid == kWords * 4) {
        if (kWords % 4 == 0 && ((uintptr_t)p & 15u) == 0) {
#pragma unroll
            for (int i = 0; i < kWords / 4; ++i) ((uint4*)p)[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
        } else {
#pragma unroll
            for (int i = 0; i < kWords; ++i) ((U32u*)p)[i].v = w[i];
        }
    } else {
#pragma unroll
        for (int i = 0; i < kWords; ++i) {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (4 * i + b < valid) p[4 * i + b] = (uint8_t)byte_of(w[i], b);
        }
    }
}

__device__ __forceinline__ uint32_t range1(const PixRange& r, uint32_t v) {
    return (uint32_t)min(max(((int)v * r.mul + r.add) >> 10, r.lo), 255);
}
__device__ __forceinline__ uint32_t range4(const PixRange& r, uint32_t w) {
    return pack4(range1(r, byte_of(w, 0)), range1(r, byte_of(w, 1)), range1(r, byte_of(w, 2)), range1(r, byte_of(w, 3)));
}

// which 16-column tile of which row (or row pair) a lane takes; false: none
__device__ __forceinline__ bool tile_of(uint32_t w, uint32_t rows, uint32_t& x0, uint32_t& row, int& valid) {
    const uint32_t tiles = (w + 15u) >> 4, t = blockIdx.x * 256u + threadIdx.x;
    if (t >= tiles * rows) return false;
    row = t / tiles;
    x0 = (t - row * tiles) << 4;
    valid = (int)min(16u, w - x0);
    return true;
}

}  // namespace

// ---- planar -> planar / gray / copy --------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void amv_pix_planes_kernel(PixPlaneJobs jobs, uint32_t frame_base) {
    const PixPlaneJob& j = jobs.j[blockIdx.y];
    uint32_t x0, y;
    int valid;
    if (!tile_of(j.w, j.h, x0, y, valid)) return;
    const uint64_t frame = frame_base + blockIdx.z;
    const uint8_t* s = j.src + frame * j.sframe;
    uint32_t o[4];
    if (j.resize == kPixCopy) {
        load_words<4>(s + (uint64_t)y * j.sstride + x0, valid, o);
    } else if (j.resize == kPixShrink12) {                                  // (a + b) >> 1 over two lines
        uint32_t a[4], b[4];
        load_words<4>(s + (uint64_t)(2 * y) * j.sstride + x0, valid, a);
        load_words<4>(s + (uint64_t)(2 * y + 1) * j.sstride + x0, valid, b);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            o[i] = pack4((byte_of(a[i], 0) + byte_of(b[i], 0)) >> 1, (byte_of(a[i], 1) + byte_of(b[i], 1)) >> 1,
                         (byte_of(a[i], 2) + byte_of(b[i], 2)) >> 1, (byte_of(a[i], 3) + byte_of(b[i], 3)) >> 1);
    } else {                                                                // (a0 + a1 + b0 + b1 + 2) >> 2 over 2 x 2
        uint32_t a[8], b[8];
        load_words<8>(s + (uint64_t)(2 * y) * j.sstride + 2 * x0, 2 * valid, a);
        load_words<8>(s + (uint64_t)(2 * y + 1) * j.sstride + 2 * x0, 2 * valid, b);
        uint32_t q[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            q[i] = ((byte_of(a[i], 0) + byte_of(a[i], 1) + byte_of(b[i], 0) + byte_of(b[i], 1) + 2u) >> 2) |
                   (((byte_of(a[i], 2) + byte_of(a[i], 3) + byte_of(b[i], 2) + byte_of(b[i], 3) + 2u) >> 2) << 8);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = __builtin_amdgcn_perm(q[2 * i + 1], q[2 * i], 0x05040100u);
    }
    if (j.range.mul != 1024) {
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = range4(j.range, o[i]);
    }
    store_words<4>(j.dst + frame * j.dframe + (uint64_t)y * j.dstride + x0, valid, o);
}

// ---- YUYV422 / UYVY422 -> YUV420P ------------------------------------------------------------------------------------
// uyvy: every dword U Y V Y is turned into Y V Y U, which is YUYV with the chroma planes exchanged (the host hands them so)
__global__ __launch_bounds__(256) void amv_pix_packed_in_kernel(PixPicture src, PixPicture dst, uint32_t w, uint32_t h, uint32_t uyvy,
                                                                uint32_t frame_base) {
    uint32_t x0, r;
    int valid;
    if (!tile_of(w, h >> 1, x0, r, valid)) return;
    const uint64_t frame = frame_base + blockIdx.z;
    const uint8_t* s = src.p[0] + frame * src.frame[0] + (uint64_t)(2 * r) * src.stride[0] + 2 * x0;
    uint32_t a[8], b[8];
    load_words<8>(s, 2 * valid, a);
    load_words<8>(s + src.stride[0], 2 * valid, b);
    if (uyvy) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            a[i] = __builtin_amdgcn_alignbit(a[i], a[i], 8);
            b[i] = __builtin_amdgcn_alignbit(b[i], b[i], 8);
        }
    }
    uint32_t y0[4], y1[4], cb[2], cr[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        y0[i] = __builtin_amdgcn_perm(a[2 * i + 1], a[2 * i], 0x06040200u);
        y1[i] = __builtin_amdgcn_perm(b[2 * i + 1], b[2 * i], 0x06040200u);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        cb[i] = pack4(byte_of(a[4 * i], 1), byte_of(a[4 * i + 1], 1), byte_of(a[4 * i + 2], 1), byte_of(a[4 * i + 3], 1));
        cr[i] = pack4(byte_of(a[4 * i], 3), byte_of(a[4 * i + 1], 3), byte_of(a[4 * i + 2], 3), byte_of(a[4 * i + 3], 3));
    }
    uint8_t* dy = dst.p[0] + frame * dst.frame[0] + (uint64_t)(2 * r) * dst.stride[0] + x0;
    store_words<4>(dy, valid, y0);
    store_words<4>(dy + dst.stride[0], valid, y1);
    store_words<2>(dst.p[1] + frame * dst.frame[1] + (uint64_t)r * dst.stride[1] + (x0 >> 1), valid >> 1, cb);
    store_words<2>(dst.p[2] + frame * dst.frame[2] + (uint64_t)r * dst.stride[2] + (x0 >> 1), valid >> 1, cr);
}

// ---- YUV420P -> YUYV422 / UYVY422 ------------------------------------------------------------------------------------
// uyvy: Y V Y U (the host hands the chroma planes exchanged) rotated into U Y V Y
__global__ __launch_bounds__(256) void amv_pix_packed_out_kernel(PixPicture src, PixPicture dst, uint32_t w, uint32_t h, uint32_t uyvy,
                                                                 uint32_t frame_base) {
    uint32_t x0, r;
    int valid;
    if (!tile_of(w, h >> 1, x0, r, valid)) return;
    const uint64_t frame = frame_base + blockIdx.z;
    const uint8_t* sy = src.p[0] + frame * src.frame[0] + (uint64_t)(2 * r) * src.stride[0] + x0;
    uint32_t y0[4], y1[4], cb[2], cr[2];
    load_words<4>(sy, valid, y0);
    load_words<4>(sy + src.stride[0], valid, y1);
    load_words<2>(src.p[1] + frame * src.frame[1] + (uint64_t)r * src.stride[1] + (x0 >> 1), valid >> 1, cb);
    load_words<2>(src.p[2] + frame * src.frame[2] + (uint64_t)r * src.stride[2] + (x0 >> 1), valid >> 1, cr);
    uint32_t a[8], b[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t u = byte_of(cb[i >> 2], i & 3), v = byte_of(cr[i >> 2], i & 3);
        const int k = 2 * (i & 1);
        a[i] = pack4(byte_of(y0[i >> 1], k), u, byte_of(y0[i >> 1], k + 1), v);
        b[i] = pack4(byte_of(y1[i >> 1], k), u, byte_of(y1[i >> 1], k + 1), v);
        if (uyvy) {
            a[i] = __builtin_amdgcn_alignbit(a[i], a[i], 24);
            b[i] = __builtin_amdgcn_alignbit(b[i], b[i], 24);
        }
    }
    uint8_t* d = dst.p[0] + frame * dst.frame[0] + (uint64_t)(2 * r) * dst.stride[0] + 2 * x0;
    store_words<8>(d, 2 * valid, a);
    store_words<8>(d + dst.stride[0], 2 * valid, b);
}

// ---- RGB24 / BGR24 / RGB32 -> YUV420P, RGB24 -> YUVJ420P -------------------------------------------------------------
// the channel order is folded into the weights (k.y[0] belongs to the byte at +0); 2x2 chroma sums, shift 2
template <int kBpp>
__global__ __launch_bounds__(256) void amv_pix_rgb_in_kernel(PixPicture src, PixPicture dst, uint32_t w, uint32_t h, PixRgbIn k,
                                                             uint32_t frame_base) {
    uint32_t x0, r;
    int valid;
    if (!tile_of(w, h >> 1, x0, r, valid)) return;
    const uint64_t frame = frame_base + blockIdx.z;
    const uint8_t* s = src.p[0] + frame * src.frame[0] + (uint64_t)(2 * r) * src.stride[0] + (uint64_t)kBpp * x0;
    uint32_t a[4 * kBpp], b[4 * kBpp];
    load_words<4 * kBpp>(s, kBpp * valid, a);
    load_words<4 * kBpp>(s + src.stride[0], kBpp * valid, b);
    int ya[16], yb[16], s0[8], s1[8], s2[8];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int o = kBpp * i;
        const int a0 = byte_of(a[o >> 2], o & 3), a1 = byte_of(a[(o + 1) >> 2], (o + 1) & 3), a2 = byte_of(a[(o + 2) >> 2], (o + 2) & 3);
        const int b0 = byte_of(b[o >> 2], o & 3), b1 = byte_of(b[(o + 1) >> 2], (o + 1) & 3), b2 = byte_of(b[(o + 2) >> 2], (o + 2) & 3);
        ya[i] = (k.y[0] * a0 + k.y[1] * a1 + k.y[2] * a2 + k.yadd) >> 10;
        yb[i] = (k.y[0] * b0 + k.y[1] * b1 + k.y[2] * b2 + k.yadd) >> 10;
        if (i & 1) { s0[i >> 1] += a0 + b0; s1[i >> 1] += a1 + b1; s2[i >> 1] += a2 + b2; }
        else { s0[i >> 1] = a0 + b0; s1[i >> 1] = a1 + b1; s2[i >> 1] = a2 + b2; }
    }
    uint32_t y0[4], y1[4], cb[2], cr[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        y0[i] = pack4(ya[4 * i], ya[4 * i + 1], ya[4 * i + 2], ya[4 * i + 3]);
        y1[i] = pack4(yb[4 * i], yb[4 * i + 1], yb[4 * i + 2], yb[4 * i + 3]);
    }
    int u[8], v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        u[i] = ((k.u[0] * s0[i] + k.u[1] * s1[i] + k.u[2] * s2[i] + 2047) >> 12) + 128;
        v[i] = ((k.v[0] * s0[i] + k.v[1] * s1[i] + k.v[2] * s2[i] + 2047) >> 12) + 128;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        cb[i] = pack4(u[4 * i], u[4 * i + 1], u[4 * i + 2], u[4 * i + 3]);
        cr[i] = pack4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
    }
    uint8_t* dy = dst.p[0] + frame * dst.frame[0] + (uint64_t)(2 * r) * dst.stride[0] + x0;
    store_words<4>(dy, valid, y0);
    store_words<4>(dy + dst.stride[0], valid, y1);
    store_words<2>(dst.p[1] + frame * dst.frame[1] + (uint64_t)r * dst.stride[1] + (x0 >> 1), valid >> 1, cb);
    store_words<2>(dst.p[2] + frame * dst.frame[2] + (uint64_t)r * dst.stride[2] + (x0 >> 1), valid >> 1, cr);
}

// ---- YUV420P / YUVJ420P -> RGB24 / BGR24 / RGB32 / RGB565 / RGB555 -----------------------------------------------------
// every size: chroma planes are (w + 1) / 2 x (h + 1) / 2, the last column and row serve one pixel (the routines' tail code)
template <int kBpp>
__device__ __forceinline__ void rgb_row(const PixRgbOut& k, const uint32_t (&yw)[4], const int (&add0)[8], const int (&add1)[8],
                                        const int (&add2)[8], uint8_t* d, int valid) {
    uint32_t c0[16], c1[16], c2[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int y = ((int)byte_of(yw[i >> 2], i & 3) - k.yoff) * k.ymul;
        c0[i] = (uint32_t)clamp8((y + add0[i >> 1]) >> 10);
        c1[i] = (uint32_t)clamp8((y + add1[i >> 1]) >> 10);
        c2[i] = (uint32_t)clamp8((y + add2[i >> 1]) >> 10);
    }
    if (kBpp == 4) {                                                  // (a << 24) | (r << 16) | (g << 8) | b, a = 0xff
        uint32_t o[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) o[i] = pack4(c0[i], c1[i], c2[i], 255u);
        store_words<16>(d, 4 * valid, o);
    } else if (kBpp == 3) {
        uint32_t o[12];
#pragma unroll
        for (int i = 0; i < 4; ++i) {                                 // four pixels in three dwords
            o[3 * i] = pack4(c0[4 * i], c1[4 * i], c2[4 * i], c0[4 * i + 1]);
            o[3 * i + 1] = pack4(c1[4 * i + 1], c2[4 * i + 1], c0[4 * i + 2], c1[4 * i + 2]);
            o[3 * i + 2] = pack4(c2[4 * i + 2], c0[4 * i + 3], c1[4 * i + 3], c2[4 * i + 3]);
        }
        store_words<12>(d, 3 * valid, o);
    } else {                                                          // c0 = r, c2 = b: 5-6-5 or 5-5-5, native 16-bit words
        uint32_t o[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint32_t p = ((c0[2 * i] >> 3) << k.rshift) | ((c1[2 * i] >> k.gdrop) << 5) | (c2[2 * i] >> 3);
            const uint32_t q = ((c0[2 * i + 1] >> 3) << k.rshift) | ((c1[2 * i + 1] >> k.gdrop) << 5) | (c2[2 * i + 1] >> 3);
            o[i] = p | (q << 16);
        }
        store_words<8>(d, 2 * valid, o);
    }
}

template <int kBpp>
__global__ __launch_bounds__(256) void amv_pix_rgb_out_kernel(PixPicture src, PixPicture dst, uint32_t w, uint32_t h, PixRgbOut k,
                                                              uint32_t frame_base) {
    uint32_t x0, r;
    int valid;
    if (!tile_of(w, (h + 1u) >> 1, x0, r, valid)) return;
    const uint64_t frame = frame_base + blockIdx.z;
    const int cvalid = (valid + 1) >> 1;
    uint32_t cb[2], cr[2];
    load_words<2>(src.p[1] + frame * src.frame[1] + (uint64_t)r * src.stride[1] + (x0 >> 1), cvalid, cb);
    load_words<2>(src.p[2] + frame * src.frame[2] + (uint64_t)r * src.stride[2] + (x0 >> 1), cvalid, cr);
    int add0[8], add1[8], add2[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int u = (int)byte_of(cb[i >> 2], i & 3) - 128, v = (int)byte_of(cr[i >> 2], i & 3) - 128;
        add0[i] = k.c0[0] * u + k.c0[1] * v + 512;
        add1[i] = k.c1[0] * u + k.c1[1] * v + 512;
        add2[i] = k.c2[0] * u + k.c2[1] * v + 512;
    }
    const uint8_t* sy = src.p[0] + frame * src.frame[0] + (uint64_t)(2 * r) * src.stride[0] + x0;
    uint8_t* d = dst.p[0] + frame * dst.frame[0] + (uint64_t)(2 * r) * dst.stride[0] + (uint64_t)kBpp * x0;
    uint32_t yw[4];
    load_words<4>(sy, valid, yw);
    rgb_row<kBpp>(k, yw, add0, add1, add2, d, valid);
    if (2 * r + 1 < h) {
        load_words<4>(sy + src.stride[0], valid, yw);
        rgb_row<kBpp>(k, yw, add0, add1, add2, d + dst.stride[0], valid);
    }
}

// ---- launches ----------------------------------------------------------------------------------------------------------
namespace {
constexpr uint32_t kFramesPerLaunch = 65535u;
inline uint32_t blocks_of(uint32_t w, uint32_t rows) { return (((w + 15u) >> 4) * rows + 255u) / 256u; }
}  // namespace

void launch_pix_planes(const PixPlaneJobs& jobs, uint32_t n, hipStream_t s) {
    uint32_t blocks = 0;
    for (uint32_t p = 0; p < jobs.count; ++p) blocks = blocks_of(jobs.j[p].w, jobs.j[p].h) > blocks ? blocks_of(jobs.j[p].w, jobs.j[p].h) : blocks;
    if (!blocks) return;
    for (uint32_t base = 0; base < n; base += kFramesPerLaunch)
        hipLaunchKernelGGL(amv_pix_planes_kernel, dim3(blocks, jobs.count, n - base < kFramesPerLaunch ? n - base : kFramesPerLaunch), dim3(256),
                           0, s, jobs, base);
}

void launch_pix_packed_in(const PixPicture& src, const PixPicture& dst, uint32_t w, uint32_t h, bool uyvy, uint32_t n, hipStream_t s) {
    for (uint32_t base = 0; base < n; base += kFramesPerLaunch)
        hipLaunchKernelGGL(amv_pix_packed_in_kernel, dim3(blocks_of(w, h >> 1), 1, n - base < kFramesPerLaunch ? n - base : kFramesPerLaunch),
                           dim3(256), 0, s, src, dst, w, h, uyvy ? 1u : 0u, base);
}

void launch_pix_packed_out(const PixPicture& src, const PixPicture& dst, uint32_t w, uint32_t h, bool uyvy, uint32_t n, hipStream_t s) {
    for (uint32_t base = 0; base < n; base += kFramesPerLaunch)
        hipLaunchKernelGGL(amv_pix_packed_out_kernel, dim3(blocks_of(w, h >> 1), 1, n - base < kFramesPerLaunch ? n - base : kFramesPerLaunch),
                           dim3(256), 0, s, src, dst, w, h, uyvy ? 1u : 0u, base);
}

void launch_pix_rgb_in(const PixPicture& src, const PixPicture& dst, uint32_t w, uint32_t h, uint32_t bpp, const PixRgbIn& k, uint32_t n,
                       hipStream_t s) {
    for (uint32_t base = 0; base < n; base += kFramesPerLaunch) {
        const dim3 grid(blocks_of(w, h >> 1), 1, n - base < kFramesPerLaunch ? n - base : kFramesPerLaunch);
        if (bpp == 3) hipLaunchKernelGGL(amv_pix_rgb_in_kernel<3>, grid, dim3(256), 0, s, src, dst, w, h, k, base);
        else hipLaunchKernelGGL(amv_pix_rgb_in_kernel<4>, grid, dim3(256), 0, s, src, dst, w, h, k, base);
    }
}

void launch_pix_rgb_out(const PixPicture& src, const PixPicture& dst, uint32_t w, uint32_t h, uint32_t bpp, const PixRgbOut& k, uint32_t n,
                        hipStream_t s) {
    for (uint32_t base = 0; base < n; base += kFramesPerLaunch) {
        const dim3 grid(blocks_of(w, (h + 1u) >> 1), 1, n - base < kFramesPerLaunch ? n - base : kFramesPerLaunch);
        if (bpp == 3) hipLaunchKernelGGL(amv_pix_rgb_out_kernel<3>, grid, dim3(256), 0, s, src, dst, w, h, k, base);
        else if (bpp == 4) hipLaunchKernelGGL(amv_pix_rgb_out_kernel<4>, grid, dim3(256), 0, s, src, dst, w, h, k, base);
        else hipLaunchKernelGGL(amv_pix_rgb_out_kernel<2>, grid, dim3(256), 0, s, src, dst, w, h, k, base);
    }
}

}  // namespace amv
