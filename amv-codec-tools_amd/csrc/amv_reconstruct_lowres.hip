// amv_reconstruct_lowres.hip -- the FFmpeg-compat back half at 1/2, 1/4 and 1/8 size: what the reference's `-lowres 1|2|3`
// computes per block (libavcodec/utils.c:707, dsputil.c:3870-3889, mjpegdec.c:711) -- decode_block's dequantisation
// with the sp5x "Q60" tables and last_dc = 1024 (amv_reconstruct_ff.hip), then j_rev_dct4 / j_rev_dct2 / j_rev_dct1
// (jrevdct.c:952-1156) over the top-left 4x4 / 2x2 / 1x1 coefficients and put_pixels_clamped4_c / 2_c /
// ff_jref_idct1_put (dsputil.c:461-493, 3774-3801).  DCTELEM is int16: every value the reference stores into the block
// is wrapped here too, `data[0] += 4` included; j_rev_dct1's (data[0] + 4) >> 3 is int arithmetic and is not.
//
// The placement is the full-size kernel's, scaled down (amv_host_plan.h: lowres_start_row); the reference's own cannot
// serve: its AMV flip takes the start row from the full-size 8 * mb_height without a shift (mjpegdec.c:675), and
// ffmpeg.c:2699 sets CODEC_FLAG_EMU_EDGE with lowres, which the flip asserts against (mjpegdec.c:674).
//
// The work split is the shared frame of amv_block_load.h: one wave per MCU-row segment (<= 10 MCUs), one block per lane.  A
// lane's block is 4, 2 or 1 bytes wide, so the segment's reduced rows are staged in LDS (the blocks' image is free once
// the blocks are in registers) and the lanes then write the rows' pieces, a dword where the destination holds one.
#include "amv_ff_dequant.h"
#include "amv_host_plan.h"

namespace amv {

namespace {

// the even part of j_rev_dct4, rows (jrevdct.c:1003-1048) and columns (:1081-1126) alike.  Its four branches are not
// one formula: with d2 == 0 the reference multiplies -d6 by FIX_1_306562965 = 10703, where the general branch gives
// d6 * (FIX_0_541196100 - FIX_1_847759065) = d6 * -10704.  Selected per call, as sidct_row selects its DC shortcut.
__device__ __forceinline__ void dct4_even(int d0, int d2, int d4, int d6, int& t10, int& t11, int& t12, int& t13) {
    constexpr int F0541 = 4433, F0765 = 6270, F1306 = 10703, F1847 = 15137;
    const int z1 = (d2 + d6) * F0541;
    int tmp2 = z1 - d6 * F1847, tmp3 = z1 + d2 * F0765;                 // d2 != 0, d6 != 0
    if (d6 == 0) { tmp2 = d2 * F0541; tmp3 = d2 * F1306; }              // d2 != 0, d6 == 0
    if (d2 == 0) { tmp2 = -d6 * F1306; tmp3 = d6 * F0541; }             // d2 == 0 (d6 == 0 too: both are 0)
    const int tmp0 = (d0 + d4) << 13, tmp1 = (d0 - d4) << 13;
    t10 = tmp0 + tmp3; t13 = tmp0 - tmp3; t11 = tmp1 + tmp2; t12 = tmp1 - tmp2;
}

// v: the block's top-left bs x bs dequantised coefficients, row-major with pitch bs -> its bs x bs bytes
template <int L>
__device__ __forceinline__ void reduced_idct(int (&v)[(8 >> L) * (8 >> L)]) {
    if constexpr (L == 1) {
        v[0] = s16(v[0] + 4);                                           // :965
#pragma unroll
        for (int r = 0; r < 4; ++r) {                                   // pass 1, :969-1058
            int &d0 = v[4 * r], &d2 = v[4 * r + 1], &d4 = v[4 * r + 2], &d6 = v[4 * r + 3];
            const bool dc_only = (d2 | d4 | d6) == 0;
            const int flat = s16(d0 << 2);                              // :986-999, (DCTELEM)(d0 << PASS1_BITS)
            int t10, t11, t12, t13;
            dct4_even(d0, d2, d4, d6, t10, t11, t12, t13);
            d0 = dc_only ? flat : s16((t10 + 1024) >> 11);
            d2 = dc_only ? flat : s16((t11 + 1024) >> 11);
            d4 = dc_only ? flat : s16((t12 + 1024) >> 11);
            d6 = dc_only ? flat : s16((t13 + 1024) >> 11);
        }
#pragma unroll
        for (int col = 0; col < 4; ++col) {                             // pass 2, :1065-1136: no shortcut
            int t10, t11, t12, t13;
            dct4_even(v[col], v[4 + col], v[8 + col], v[12 + col], t10, t11, t12, t13);
            v[col] = crop(s16(t10 >> 18));
            v[4 + col] = crop(s16(t11 >> 18));
            v[8 + col] = crop(s16(t12 >> 18));
            v[12 + col] = crop(s16(t13 >> 18));
        }
    } else if constexpr (L == 2) {                                      // j_rev_dct2, :1139-1152
        v[0] = s16(v[0] + 4);
        const int d00 = v[0] + v[1], d01 = v[0] - v[1], d10 = v[2] + v[3], d11 = v[2] - v[3];
        v[0] = crop(s16((d00 + d10) >> 3));
        v[1] = crop(s16((d01 + d11) >> 3));
        v[2] = crop(s16((d00 - d10) >> 3));
        v[3] = crop(s16((d01 - d11) >> 3));
    } else {                                                            // ff_jref_idct1_put, dsputil.c:3796-3801
        v[0] = crop((v[0] + 4) >> 3);
    }
}

// The LDS staging of a segment's reduced rows.  Rows: 2 * bs of luma (20 blocks wide), then bs of Cb and bs of Cr (10
// blocks wide).  A row is written out as "slots": the dwords of the DESTINATION (which may begin anywhere in a
// dword: frames and rows of odd sizes lie back to back), so a row of len bytes has up to len / 4 + 1 of them and the
// first and the last may be partial.  In LDS a row has a dword of padding in front and behind, so that the two
// aligned dwords around any slot can be read; the pitches (in dwords: 23 / 13, 13 / 8, 8 / 6) keep successive rows on
// different banks.
template <int L>
struct Stage {
    static constexpr uint32_t bs = 8u >> L;
    static constexpr uint32_t len_y = 20u * bs, len_c = 10u * bs;
    static constexpr uint32_t slots_y = (len_y + 3u) / 4u + 1u, slots_c = (len_c + 3u) / 4u + 1u;
    static constexpr uint32_t pitch_y = (slots_y + 2u) * 4u, pitch_c = (slots_c + 2u) * 4u;
    static constexpr uint32_t rows_y = 2u * bs, rows_c = 2u * bs;      // (Cb and Cr together)
    static constexpr uint32_t off_c = rows_y * pitch_y;
    static constexpr uint32_t bytes = off_c + rows_c * pitch_c;
    static constexpr uint32_t items_y = rows_y * slots_y, items = items_y + rows_c * slots_c;
};

}  // namespace

// what the kernel needs of the reduced picture (amv_host_plan.h)
struct LowresGeom {
    uint32_t w, h, cw, ch;       // the planes
    int start_y, start_c;        // lowres_start_row
    uint64_t frame_bytes;
};

// out: per frame, Y plane W_L x H_L, then Cb and Cr of ((W_L + 1) / 2) x ((H_L + 1) / 2), rows tight
// kRound: a round launch (FrameSel::round != 0), whose workgroups walk the items of the round
template <int L, bool kRound>
__global__ __launch_bounds__(kWave) void amv_reconstruct_yuv_lowres_kernel(
    SyncSinks in, const uint32_t* __restrict__ nmcu_ok, uint32_t n, FrameSel sel, FrameGeom g, PieceMap pm, LowresGeom lg,
    uint8_t* __restrict__ out) {
    using S = Stage<L>;
    constexpr uint32_t bs = S::bs;
    static_assert(S::bytes <= kSegImageBytes, "the staged rows fit the blocks' image");
    __shared__ __attribute__((aligned(16))) uint8_t s_img[kSegImageBytes + 128];   // + a spare slot per lane (load_segment_blocks)
    const uint32_t lane = threadIdx.x;
    uint32_t item, my, seg;
    if (!locate_piece(pm, blockIdx.x, item, my, seg)) return;
    do {
    uint32_t f, slot;
    if (!select_frame(sel, n, item, f, slot)) return;
    const Segment sg = segment_of(f, slot, nmcu_ok, g, pm.nseg, my, seg);
    const uint32_t m0 = sg.m0, cnt = sg.cnt;

    uint32_t c[32];
    bool skip;
    const bool has = load_segment_blocks(in, sg, kRound, g, lane, s_img, c, skip);
    if (!skip) {   // (the same in every lane)
    seg_sync();    // every lane has its block: the image becomes the staged rows
    if (has) {
        const FfBlock b = ff_block(in, sg, lane);
        const uint32_t m = b.m, k6 = b.k6;
        const bool chroma = b.chroma, decoded = b.decoded;   // blocks at or after a frame's first error stay zero
        int v[bs * bs];
        q60_dequantise<(8 >> L)>(c, chroma, v);
        reduced_idct<L>(v);
        const uint32_t row0 = chroma ? (k6 - 4u) * bs : (k6 >> 1) * bs;
        const uint32_t col0 = (chroma ? m : 2u * m + (k6 & 1u)) * bs;
        uint8_t* at = s_img + (chroma ? S::off_c + row0 * S::pitch_c : row0 * S::pitch_y) + 4u + col0;
        const uint32_t pitch = chroma ? S::pitch_c : S::pitch_y;
#pragma unroll
        for (uint32_t i = 0; i < bs; ++i) {
            if constexpr (L == 1) {
                const uint32_t px = (uint32_t)v[4 * i] | ((uint32_t)v[4 * i + 1] << 8) | ((uint32_t)v[4 * i + 2] << 16) | ((uint32_t)v[4 * i + 3] << 24);
                *reinterpret_cast<uint32_t*>(at + i * pitch) = decoded ? px : 0u;
            } else if constexpr (L == 2) {
                const uint32_t px = (uint32_t)v[2 * i] | ((uint32_t)v[2 * i + 1] << 8);
                *reinterpret_cast<uint16_t*>(at + i * pitch) = (uint16_t)(decoded ? px : 0u);
            } else {
                at[0] = (uint8_t)(decoded ? v[0] : 0);
            }
        }
    }
    seg_sync();
    // the rows' pieces: every lane takes slots, whether it held a block or not
    uint8_t* frame = out + (uint64_t)f * lg.frame_bytes;
    for (uint32_t t = lane; t < S::items; t += kWave) {
        const bool luma = t < S::items_y;
        const uint32_t u = luma ? t : t - S::items_y;
        const uint32_t row = luma ? u / S::slots_y : u / S::slots_c;           // (divisions by constants)
        const uint32_t j = luma ? u - row * S::slots_y : u - row * S::slots_c;
        const uint32_t crow = row % bs;                                        // chroma: the row inside Cb or Cr
        const bool second = !luma && row >= bs;                                // Cr
        const uint32_t pw = luma ? lg.w : lg.cw, ph = luma ? lg.h : lg.ch;
        const int p = luma ? lg.start_y - (int)(my * 2u * bs + row) : lg.start_c - (int)(my * bs + crow);
        if (p < 0 || p >= (int)ph) continue;                                   // rows the rule sends outside the plane are dropped
        const uint32_t x0 = m0 * (luma ? 2u * bs : bs);                        // the segment's first column (< pw)
        const uint32_t len = min(cnt * (luma ? 2u * bs : bs), pw - x0);        // ... and columns beyond the plane
        uint8_t* d = frame + (luma ? 0ull : (uint64_t)lg.w * lg.h + (second ? (uint64_t)lg.cw * lg.ch : 0ull)) + (uint64_t)p * pw + x0;
        const uint32_t a = (uint32_t)((uintptr_t)d & 3u);
        const int first = (int)(4u * j) - (int)a;                              // the row's byte at the slot's byte 0
        if (first >= (int)len) continue;
        const uint8_t* src = s_img + (luma ? row * S::pitch_y : S::off_c + row * S::pitch_c);
        const uint32_t off = 4u + 4u * j - a;                                  // >= 1: the padding dword in front
        const uint32_t* q = reinterpret_cast<const uint32_t*>(src) + (off >> 2);
        const uint32_t word = (uint32_t)((((uint64_t)q[1] << 32) | q[0]) >> (8u * (off & 3u)));
        uint8_t* dw = d + first;                                               // 4-byte aligned
        if (first >= 0 && first + 4 <= (int)len) {
            *reinterpret_cast<uint32_t*>(dw) = word;
        } else {                                                               // a row's ragged ends
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (first + b >= 0 && first + b < (int)len) dw[b] = (uint8_t)(word >> (8 * b));
        }
    }
    }
    } while (next_item<kRound>(pm, item));   // (the image is free again)
}

template <int L, class... Args>
static void launch_lowres(const FrameGeom& g, Args... args) {
    launch_segments(amv_reconstruct_yuv_lowres_kernel<L, false>, amv_reconstruct_yuv_lowres_kernel<L, true>, kWave, g.mcu_rows, args...);
}

void launch_reconstruct_yuv_lowres(const SyncSinks& sinks, const uint32_t* nmcu_ok, uint32_t n, const FrameSel& sel, uint32_t items,
                                   const FrameGeom& g, uint32_t lowres, uint8_t* out, hipStream_t s) {
    if (lowres < 1u || lowres > 3u) return;
    LowresGeom lg;
    lg.w = lowres_dim(g.width, lowres);
    lg.h = lowres_dim(g.height, lowres);
    lg.cw = (lg.w + 1u) / 2u;
    lg.ch = (lg.h + 1u) / 2u;
    lg.start_y = lowres_start_row(g.height, lowres, false);
    lg.start_c = lowres_start_row(g.height, lowres, true);
    lg.frame_bytes = lowres_frame_bytes(g.width, g.height, lowres);
    if (lowres == 1u) launch_lowres<1>(g, sinks, nmcu_ok, n, sel, items, g, s, lg, out);
    else if (lowres == 2u) launch_lowres<2>(g, sinks, nmcu_ok, n, sel, items, g, s, lg, out);
    else launch_lowres<3>(g, sinks, nmcu_ok, n, sel, items, g, s, lg, out);
}

}  // namespace amv
