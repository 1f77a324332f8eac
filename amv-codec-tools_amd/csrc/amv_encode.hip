// amv_encode.hip -- AMV video encode kernels for gfx950 (MI355X).
//
// Reference path: AMVmuxer/ffmpeg (lavc = libavcodec):
//   RGB24 -> YUVJ420P          lavc/imgconvert_template.h:654-, colorspace.h:30-97
//   vertical flip              lavc/mjpegenc.c:454-472 (amv_encode_picture)
//   forward DCT                lavc/jfdctint.c:184-343 (ff_jpeg_fdct_islow)
//   quantise                   lavc/mpegvideo_enc.c:3647-3724 (dct_quantize_c), :70-91, :492-496
//   run/size Huffman           lavc/mjpegenc.c:357-450, code book lavc/mjpeg.c:129-147
//   stuffing, FF escaping, EOI lavc/mjpegenc.c:282-355; SOI only :201-204
// The reference encoder quantises with a matrix no AMV decoder uses; this
// one uses amvlib's fixed tables (AmvJpeg.c:30-61) and a true -128 level shift so that amvlib
// and the patched FFmpeg both decode it.
//
//   amv_forward_kernel  data parallel: one wave per MCU-row segment; colour conversion of 4x2-pixel
//                       patches into LDS planes, then one 8x8 block per lane held in registers:
//                       row passes, column passes, quantise, scan order, one 128-byte line out.
//   amv_pack_kernel     serial inside a frame (DC prediction + variable-length output), so
//                       one lane per frame; a wave stages block b of its 64 frames in LDS with
//                       whole-line loads and every lane codes its own block from there.
//   amv_scan_kernel / amv_gather_kernel   prefix sum of chunk lengths and compaction.
#include "amv_encode_common.h"

namespace amv {

using namespace enc;

// One wave per MCU-row segment of up to kSegMcus MCUs: stage 1 (colour conversion into LDS planes) and stage 2 (one
// 8x8 block per lane: fdct, quantise, scan order) of amv_encode_common.h, then one 128-byte line per block out.
// What amvhip_encode_coefs_dev hands out, the serial route (AMVHIP_ENTROPY_SERIAL) and the frames
// amv_encode_frame_kernel hands back go through here; sel: which frames (FrameSel, as in the decoder's rounds).
// Nr: nothing (the plain kernel, its signature and code as they always were), or one `const uint16_t*` -- the noise-reduction
// offsets of the call's frames (64 uint16 per frame, amv_nr_plan.h): a frame's 128 bytes go to LDS and transform_block
// denoises with them between the column pass and the quantiser; or one TrellisArg -- the AC outputs leave transform_block
// un-quantised, go to the lane's line in the planes' space, and trellis_lane makes the levels there; or one NrTrellisArg --
// both: the outputs are denoised with the offsets and trellis_lane searches on what is left; or a TrellisFrames / an
// NrTrellisFrames -- those two with the lambda read at the frame's own index (the rate entries).
template <bool kYuv, class... Nr>
__global__ __launch_bounds__(kWave) void amv_forward_kernel(Source in, uint32_t n, FrameSel sel, FrameGeom g, uint32_t nseg, uint32_t per_seg,
                                                            uint32_t qbias, int16_t* __restrict__ coef, Nr... nr) {
    constexpr bool kNr = OptKind<Nr...>::kNr, kTrellis = OptKind<Nr...>::kTrellis;
    static_assert(sizeof...(Nr) == 0 || kNr || kTrellis, "the offsets, lambda, both, or nothing");
    __shared__ __attribute__((aligned(16))) int16_t s_planes[kPlaneSamples];
    __shared__ __attribute__((aligned(16))) uint32_t s_qmul[kQuantMulWords];
    uint32_t* s_nr_off = nullptr;
    if constexpr (kNr) {
        __shared__ __attribute__((aligned(16))) uint32_t s_off[32];
        s_nr_off = s_off;
    }
    const TrellisTables* s_trellis = nullptr;
    if constexpr (kTrellis) {
        __shared__ __attribute__((aligned(16))) TrellisTables s_tab;
        load_trellis_tables(&s_tab, threadIdx.x, kWave);
        s_trellis = &s_tab;
    }
    load_quant_mul(s_qmul, threadIdx.x, kWave);
    int16_t* const s_y = s_planes;
    int16_t* const s_cb = s_planes + 16 * kPitchY;
    int16_t* const s_cr = s_cb + 8 * kPitchC;

    const uint32_t lane = threadIdx.x;
    const uint32_t segs = g.mcu_rows * nseg;
    uint32_t my, m0, cnt;
    if (!seg_place(SegSplit{nseg, per_seg}, g, blockIdx.x % segs, my, m0, cnt)) return;
    const uint32_t nb = cnt * 6;
    // default: one frame per workgroup column.  A round: the launch is small (the round usually has nothing to do and
    // the host cannot know) and its workgroups walk the round's items: item i = frame list[base + i], lines in slot i.
    const uint32_t first = blockIdx.x / segs, stride = gridDim.x / segs;
    const uint32_t items = sel_items(sel, n);
    for (uint32_t slot = first; slot < items; slot += stride) {
        const uint32_t f = sel_frame(sel, slot);
        convert_segment<kYuv>(in, f, g, my, m0, cnt, lane, s_y, s_cb, s_cr);
        if (kNr && lane < 32u) s_nr_off[lane] = reinterpret_cast<const uint32_t*>(nr_offsets_of(nr...) + (uint64_t)f * 64u)[lane];
        __syncthreads();
        uint4* const dst = reinterpret_cast<uint4*>(coef + ((uint64_t)slot * g.mcus + (uint64_t)my * g.mcu_cols + m0) * 384u + lane * 64u);
        if constexpr (kTrellis) {
            uint32_t out[32], nz_lo, nz_hi;
            if (lane < nb)
                transform_block<kNr, true>(s_y, s_cb, s_cr, s_qmul, lane, qbias, out, nz_lo, nz_hi, reinterpret_cast<const uint16_t*>(s_nr_off));
            __syncthreads();               // every lane has its samples: the planes become the lines
            if (lane < nb) {
                uint8_t* const region = reinterpret_cast<uint8_t*>(s_planes);
                store_line(region, lane, out);
                trellis_lane(region, lane, *s_trellis, qbias, frame_lambda_of(f, nr...), nz_lo, nz_hi);
#pragma unroll
                for (uint32_t i = 0; i < 8; ++i) dst[i] = load_line_granule(region, lane, i);
            }
        } else if (lane < nb) {
            uint32_t out[32], nz_lo, nz_hi;
            transform_block<kNr>(s_y, s_cb, s_cr, s_qmul, lane, qbias, out, nz_lo, nz_hi, reinterpret_cast<const uint16_t*>(s_nr_off));
#pragma unroll
            for (int i = 0; i < 8; ++i) dst[i] = make_uint4(out[4 * i], out[4 * i + 1], out[4 * i + 2], out[4 * i + 3]);
        }
        __syncthreads();                   // the planes are free again
    }
}

void launch_forward(const Source& in, uint32_t n, const FrameSel& sel, uint32_t items, const FrameGeom& g, uint32_t qbias,
                    const Quantiser& quant, int16_t* coef, hipStream_t s) {
    if (items == 0) return;
    const SegSplit sp = seg_split(g);
    const uint64_t grid = (uint64_t)(sel.round && items > 64u ? 64u : items) * g.mcu_rows * sp.nseg;
    with_instantiation(in, quant, [&](auto yuv, auto... opt) {
        hipLaunchKernelGGL((amv_forward_kernel<decltype(yuv)::value, decltype(opt)...>), dim3((uint32_t)grid), dim3(kWave), 0, s, in, n, sel, g,
                           sp.nseg, sp.per_seg, qbias, coef, opt...);
    });
}

// ============================================================================================
// entropy coder
// ============================================================================================

namespace {

struct BitWriter {
    uint8_t* out;
    uint32_t pos;
    uint64_t acc;  // pending bits, right aligned
    int nacc;
};

// escape_FF (mjpegenc.c:282-336): every FF of the scan is followed by a 00
__device__ __forceinline__ void emit_byte(BitWriter& w, uint32_t b) {
    w.out[w.pos++] = (uint8_t)b;
    if (b == 0xffu) w.out[w.pos++] = 0;
}

__device__ __forceinline__ void put_bits(BitWriter& w, int nbits, uint32_t value) {
    w.acc = (w.acc << nbits) | value;
    w.nacc += nbits;
    while (w.nacc >= 8) {
        w.nacc -= 8;
        emit_byte(w, (uint32_t)(w.acc >> w.nacc) & 0xffu);
    }
}

// ff_mjpeg_encode_dc / the AC branch of encode_block (mjpegenc.c:357-377, 411-424)
__device__ __forceinline__ void put_coef(BitWriter& w, const uint32_t* book, int run, int val) {
    int mant = val;
    if (val < 0) { val = -val; mant--; }
    const int nb = 32 - __clz(val);
    const uint32_t e = book[(run << 4) | nb];
    put_bits(w, (int)(e >> 16) + nb, ((e & 0xffffu) << nb) | ((uint32_t)mant & ((1u << nb) - 1u)));
}

__device__ __forceinline__ uint32_t slot_offset(uint32_t lane, uint32_t k) { return line_offset(lane, k); }

}  // namespace

__global__ __launch_bounds__(kWave) void amv_pack_kernel(
    const int16_t* __restrict__ coef, uint32_t n, FrameSel sel, uint32_t blocks_per_frame,
    const HuffEncodeImage* __restrict__ img, uint8_t* __restrict__ tmp, uint32_t bound,
    uint32_t* __restrict__ lens) {
    __shared__ uint32_t s_book[4][256];
    __shared__ __attribute__((aligned(16))) uint4 s_slots[kWave * 8];
    __shared__ uint32_t s_frame[kWave];

    // default: frames 0 .. n, a frame's lines at its own place.  A round (frames amv_encode_frame_kernel handed back):
    // items base .. base + round, item p = frame list[p] (p < *count), lines in slot p - base.
    const uint32_t lane = threadIdx.x;
    const uint32_t f0 = blockIdx.x * kWave;
    const uint32_t items = sel_items(sel, n);
    if (f0 >= items) return;
    const uint32_t slot = f0 + lane;
    const uint32_t frame = slot < items ? sel_frame(sel, slot) : 0xffffffffu;
    s_frame[lane] = slot < items ? slot : 0xffffffffu;
    const bool live = frame != 0xffffffffu;
    for (int i = lane; i < 4 * 256; i += kWave) (&s_book[0][0])[i] = (&img->code[0][0])[i];

    BitWriter w;
    w.out = tmp + (uint64_t)(live ? frame : 0) * bound;
    w.pos = 0;
    w.acc = 0;
    w.nacc = 0;
    if (live) { w.out[0] = 0xff; w.out[1] = 0xd8; w.pos = 2; }   // SOI only, mjpegenc.c:201-204
    int pred0 = 0, pred1 = 0, pred2 = 0;
    const char* slot_bytes = reinterpret_cast<const char*>(s_slots);

    uint32_t k6 = 0;
    for (uint32_t b = 0; b < blocks_per_frame; ++b) {
        __syncthreads();
#pragma unroll
        for (uint32_t i = 0; i < 8; ++i) {   // block b of 64 frames: 64 whole lines
            const uint32_t c = i * kWave + lane;
            const uint32_t s = c >> 3, part = c & 7u;
            uint4 v = make_uint4(0, 0, 0, 0);
            const uint32_t fr = s_frame[s];
            if (fr != 0xffffffffu)
                v = reinterpret_cast<const uint4*>(coef + ((uint64_t)fr * blocks_per_frame + b) * 64u)[part];
            s_slots[s * 8u + (part ^ (s & 7u))] = v;
        }
        __syncthreads();
        if (live) {   // encode_block, mjpegenc.c:379-435
            const int cls = k6 < 4 ? 0 : 1;
            const int dc = *reinterpret_cast<const int16_t*>(slot_bytes + slot_offset(lane, 0));
            int diff;
            if (k6 < 4) { diff = dc - pred0; pred0 = dc; }
            else if (k6 == 4) { diff = dc - pred1; pred1 = dc; }
            else { diff = dc - pred2; pred2 = dc; }
            if (diff == 0) put_bits(w, (int)(s_book[cls][0] >> 16), s_book[cls][0] & 0xffffu);
            else put_coef(w, s_book[cls], 0, diff);
            const uint32_t* ac = s_book[2 + cls];
            int run = 0;
            for (uint32_t k = 1; k < 64; ++k) {
                const int v = *reinterpret_cast<const int16_t*>(slot_bytes + slot_offset(lane, k));
                if (v == 0) { ++run; continue; }
                while (run >= 16) { put_bits(w, (int)(ac[0xf0] >> 16), ac[0xf0] & 0xffffu); run -= 16; }
                put_coef(w, ac, run, v);
                run = 0;
            }
            if (run) put_bits(w, (int)(ac[0] >> 16), ac[0] & 0xffffu);   // EOB, :430-431
        }
        if (++k6 == 6) k6 = 0;
    }
    if (live) {
        if (w.nacc) put_bits(w, 8 - w.nacc, (1u << (8 - w.nacc)) - 1u);   // ff_mjpeg_encode_stuffing :338-343
        w.out[w.pos++] = 0xff;                                           // EOI :354
        w.out[w.pos++] = 0xd9;
        lens[frame] = w.pos;
    }
}

void launch_pack(const int16_t* coef, uint32_t n, const FrameSel& sel, uint32_t items, const FrameGeom& g,
                 const HuffEncodeImage* d_img, uint8_t* tmp, uint32_t bound, uint32_t* lens, hipStream_t s) {
    if (items == 0) return;
    const uint32_t grid = (items + kWave - 1) / kWave;   // a round: upper bound, surplus groups exit at once
    hipLaunchKernelGGL(amv_pack_kernel, dim3(grid), dim3(kWave), 0, s, coef, n, sel, g.blocks, d_img, tmp, bound, lens);
}

// ============================================================================================
// compaction: offs = exclusive scan(lens); blob[offs[i] ..) = tmp[i*bound ..)
// ============================================================================================

__global__ __launch_bounds__(1024) void amv_scan_kernel(const uint32_t* __restrict__ lens, uint32_t n,
                                                        uint64_t* __restrict__ offs, uint64_t cap,
                                                        int32_t* __restrict__ overflow) {
    __shared__ uint64_t s_part[1024];
    const uint32_t t = threadIdx.x;
    const uint32_t per = (n + 1023u) / 1024u;
    const uint32_t lo = min(n, t * per), hi = min(n, lo + per);
    uint64_t sum = 0;
    for (uint32_t i = lo; i < hi; ++i) sum += lens[i];
    s_part[t] = sum;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {   // Hillis-Steele inclusive scan
        const uint64_t add = t >= d ? s_part[t - d] : 0;
        __syncthreads();
        s_part[t] += add;
        __syncthreads();
    }
    uint64_t run = s_part[t] - sum;
    for (uint32_t i = lo; i < hi; ++i) { offs[i] = run; run += lens[i]; }
    if (t == 1023) *overflow = s_part[1023] > cap ? 1 : 0;
}

__global__ __launch_bounds__(256) void amv_gather_kernel(const uint8_t* __restrict__ tmp, uint32_t bound,
                                                         uint32_t* __restrict__ lens,
                                                         const uint64_t* __restrict__ offs,
                                                         uint8_t* __restrict__ blob, uint64_t cap) {
    struct __attribute__((packed, aligned(1))) Bytes16 { uint32_t w[4]; };   // a chunk lands at any byte of the blob
    const uint32_t i = blockIdx.x;
    const uint32_t len = lens[i];
    const uint64_t off = offs[i];
    if (off + len > cap) {   // does not fit the caller's blob: not written, and its length says so
        if (threadIdx.x == 0) lens[i] = 0;
        return;
    }
    const uint8_t* src = tmp + (uint64_t)i * bound;
    uint8_t* dst = blob + off;
    const uint32_t whole = len & ~15u;
    for (uint32_t k = threadIdx.x * 16u; k < whole; k += 256u * 16u)
        *reinterpret_cast<Bytes16*>(dst + k) = *reinterpret_cast<const Bytes16*>(src + k);
    if (threadIdx.x < len - whole) dst[whole + threadIdx.x] = src[whole + threadIdx.x];
}

void launch_compact(const uint8_t* tmp, uint32_t bound, uint32_t* lens, uint32_t n,
                    uint64_t* offs, uint8_t* blob, uint64_t blob_cap, int32_t* overflow, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(amv_scan_kernel, dim3(1), dim3(1024), 0, s, lens, n, offs, blob_cap, overflow);
    hipLaunchKernelGGL(amv_gather_kernel, dim3(n), dim3(256), 0, s, tmp, bound, lens, offs, blob, blob_cap);
}

}  // namespace amv
