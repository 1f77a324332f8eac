// amv_reconstruct_ff.hip -- the FFmpeg-compat back half of the decoder (AMVHIP_FLAG_FFMPEG): what the patched
// FFmpeg's amv_decoder computes after its Huffman stage -- decode_block's dequantisation with the sp5x "Q60"
// tables and last_dc = 1024 (libavcodec/mjpegdec.c:376-430,805; sp5xdec.c:40,60-61), the standard zig-zag
// (dsputil.c:50-59), simple_idct_put (simple_idct.c:78-181,183-247,390-398) and the planar YUVJ420P store with
// the AMV flip (mjpegdec.c:672-677,708-716).  No colour conversion: FFmpeg hands out the three planes.
//
// The work split is the shared frame of amv_block_load.h: one wave per MCU-row segment (<= 10 MCUs), one 8x8 block per
// lane, held in registers through both passes; a lane then owns 8 rows of 8 output bytes and stores them itself.
// DCTELEM is int16 in the reference: every value that it stores into a block (dequantised coefficients, row-pass
// results) is wrapped to 16 bits here too, and the DC-only shortcut of idctRowCondDC -- which is NOT the general
// row formula (8*dc against (16383*dc + 1024) >> 11) -- is taken per row by a select.
#include "amv_simple_idct.h"

namespace amv {

// out: per frame, Y plane width*height, then Cb and Cr of ((w+1)/2) x ((h+1)/2), rows tight
// kRound: a round launch (FrameSel::round != 0), whose workgroups walk the items of the round
template <bool kRound>
__global__ __launch_bounds__(kWave) void amv_reconstruct_yuv_kernel(
    SyncSinks in, const uint32_t* __restrict__ nmcu_ok, uint32_t n, FrameSel sel, FrameGeom g, PieceMap pm, uint64_t yuv_frame_bytes,
    uint8_t* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) uint8_t s_img[kSegImageBytes + 128];   // + a spare slot per lane (load_segment_blocks)
    const uint32_t lane = threadIdx.x;
    uint32_t item, my, seg;   // (one MCU row per workgroup: the row group is the row)
    if (!locate_piece(pm, blockIdx.x, item, my, seg)) return;
    do {
    uint32_t f, slot;
    if (!select_frame(sel, n, item, f, slot)) return;
    const Segment sg = segment_of(f, slot, nmcu_ok, g, pm.nseg, my, seg);
    const uint32_t m0 = sg.m0;

    uint32_t c[32];
    bool skip;
    if (load_segment_blocks(in, sg, kRound, g, lane, s_img, c, skip)) {
    const FfBlock b = ff_block(in, sg, lane);
    const uint32_t m = b.m, k6 = b.k6;
    const bool chroma = b.chroma, decoded = b.decoded;
    const bool keep = in.ok_in_blocks != 0u;
    int v[64];   // q60_dequantise<8> written out: as the function it costs the round kernel a vector register (181, not 180)
#pragma unroll
    for (int nat = 0; nat < 64; ++nat) {
        const int scan = kScanOfNatural[nat];
        const int step = chroma ? (int)kQ60Chroma[scan] : (int)kQ60Luma[scan];
        v[nat] = s16(coef_at(c, scan) * step + (nat == 0 ? 1024 : 0));
    }
#pragma unroll
    for (int r = 0; r < 8; ++r)
        sidct_row(v[8 * r], v[8 * r + 1], v[8 * r + 2], v[8 * r + 3], v[8 * r + 4], v[8 * r + 5], v[8 * r + 6], v[8 * r + 7]);
#pragma unroll
    for (int col = 0; col < 8; ++col)
        sidct_col(v[col], v[8 + col], v[16 + col], v[24 + col], v[32 + col], v[40 + col], v[48 + col], v[56 + col]);

    // mjpeg_decode_scan's placement (:672-677,708-716): component rows run upwards from
    // start = v * (8 * mb_height - ((height / 2) & 7)) - 1; rows the formula sends outside the plane are dropped
    const uint32_t cw = (g.width + 1u) >> 1, ch = (g.height + 1u) >> 1;
    const uint32_t pw = chroma ? cw : g.width, ph = chroma ? ch : g.height;
    const int vs = chroma ? 1 : 2;
    const int start = vs * (int)(8u * g.mcu_rows - ((g.height >> 1) & 7u)) - 1;
    const uint32_t sx = (chroma ? m0 + m : 2u * (m0 + m) + (k6 & 1u)) * 8u;
    const int sy = (int)((chroma ? my : 2u * my + (k6 >> 1)) * 8u);
    uint8_t* plane = out + (uint64_t)f * yuv_frame_bytes +
                     (chroma ? (uint64_t)g.width * g.height + (k6 == 5u ? (uint64_t)cw * ch : 0ull) : 0ull);
    if (sx < pw) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int p = start - (sy + i);
        if (p < 0 || p >= (int)ph) continue;
        if (keep && !decoded) continue;      // the caller's buffer is left as it was (FFmpeg: whatever the picture held)
        uint32_t lo = 0, hi = 0;
        if (decoded) {   // MCUs at or after a frame's first error stay zero
            lo = (uint32_t)v[8 * i] | ((uint32_t)v[8 * i + 1] << 8) | ((uint32_t)v[8 * i + 2] << 16) | ((uint32_t)v[8 * i + 3] << 24);
            hi = (uint32_t)v[8 * i + 4] | ((uint32_t)v[8 * i + 5] << 8) | ((uint32_t)v[8 * i + 6] << 16) | ((uint32_t)v[8 * i + 7] << 24);
        }
        uint8_t* d = plane + (uint64_t)p * pw + sx;
        if (sx + 8u <= pw && ((uintptr_t)d & 7u) == 0u) {
            *reinterpret_cast<uint2*>(d) = make_uint2(lo, hi);
        } else {
#pragma unroll
            for (uint32_t j = 0; j < 8u; ++j)
                if (sx + j < pw) d[j] = (uint8_t)((j < 4u ? lo >> (8u * j) : hi >> (8u * (j - 4u))) & 0xffu);
        }
    }
    }
    }
    } while (next_item<kRound>(pm, item));   // (the image is free again)
}

// true when every row of every plane is reached by mjpegdec.c:672-677's formula (then the kernel writes each
// output byte and no clearing pass is needed); heights of 16k+14 or 16k+15 leave the bottom rows untouched
bool yuv_store_covers_planes(const FrameGeom& g) {
    const int start_y = 2 * (int)(8u * g.mcu_rows - ((g.height >> 1) & 7u)) - 1;
    const int start_c = (int)(8u * g.mcu_rows - ((g.height >> 1) & 7u)) - 1;
    return start_y >= (int)g.height - 1 && start_c >= (int)((g.height + 1u) >> 1) - 1;
}

void launch_reconstruct_yuv(const SyncSinks& sinks, const uint32_t* nmcu_ok, uint32_t n, const FrameSel& sel, uint32_t items,
                            const FrameGeom& g, uint64_t yuv_frame_bytes, uint8_t* out, hipStream_t s) {
    launch_segments(amv_reconstruct_yuv_kernel<false>, amv_reconstruct_yuv_kernel<true>, kWave, g.mcu_rows, sinks, nmcu_ok, n, sel, items, g, s,
                    yuv_frame_bytes, out);
}

}  // namespace amv
