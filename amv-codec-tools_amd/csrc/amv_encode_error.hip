// amv_encode_error.hip -- the encoder's own error (`ffmpeg -psnr`): per frame and plane, the squared error between the
// picture the encoder was handed and the reconstruction of the levels it coded, summed over the visible samples.
//
// Reference path: encode_thread adds up sse(new_picture, dest) per plane, macroblock by macroblock, clipped to the picture
// (mpegvideo_enc.c:2590-2606); `dest` is what its own idct_put (simple_idct_put) made of the block it coded.
// Here the reconstruction is the FFmpeg-compat back half's block arithmetic (amv_reconstruct_ff.hip) with the encoder's own
// tables in the place of Q60: v[natural] = (int16)(level[scan] * Q[scan]), + 1024 on the DC, simple_idct_put and its
// 0..255 clip -- the pixel-domain form of the trellis search's distortion model ("level * Q").  It is NOT the reference's
// number (MPV_decode_mb unquantises with the MPEG-1 intra rule and the MPEG matrix, which fits neither AMV decoder), and
// it is not amvlib's picture either (that differs by its IDCT's rounding, its one scan quirk and the colour step):
// amvhip_picture_sse_dev measures against a decoder's picture.
//
//   amv_encode_error_kernel   one wave per MCU-row segment, as amv_forward_kernel: stage 1 of the encoder rebuilds the
//                             segment's planes in LDS (the handed picture: for RGB / BGR sources the planes of the fused
//                             rgb24_to_yuvj420p), a lane reads its block's dense line (what launch_forward wrote for the
//                             call's quantiser), dequantises, runs both IDCT passes in registers, squares the
//                             differences over the samples inside the picture (rows and columns an edge MCU replicates
//                             do not count), and the wave's three sums go to sse[frame][plane] by 64-bit atomic adds.
//                             Integer sums: the order of the adds does not matter.
#include "amv_encode_common.h"
#include "amv_simple_idct.h"
#include "amv_wave.h"

namespace amv {

using namespace enc;

template <bool kYuv>
__global__ __launch_bounds__(kWave) void amv_encode_error_kernel(Source in, uint32_t n, FrameSel sel, FrameGeom g, uint32_t nseg, uint32_t per_seg,
                                                                 const int16_t* __restrict__ coef, unsigned long long* __restrict__ sse) {
    __shared__ __attribute__((aligned(16))) int16_t s_planes[kPlaneSamples];
    int16_t* const s_y = s_planes;
    int16_t* const s_cb = s_planes + 16 * kPitchY;
    int16_t* const s_cr = s_cb + 8 * kPitchC;

    const uint32_t lane = threadIdx.x;
    const uint32_t segs = g.mcu_rows * nseg;
    uint32_t my, m0, cnt;
    if (!seg_place(SegSplit{nseg, per_seg}, g, blockIdx.x % segs, my, m0, cnt)) return;
    const uint32_t nb = cnt * 6;
    // the lane's block, where it lies in its plane (bitstream rows: row k is picture row height - 1 - k), and how much of it
    // is inside the picture
    const uint32_t m = lane / 6u, k6 = lane - 6u * m;
    const bool chroma = k6 >= 4u;
    const uint32_t pw = chroma ? g.width >> 1 : g.width, ph = chroma ? g.height >> 1 : g.height;
    const uint32_t sx = (chroma ? m0 + m : 2u * (m0 + m) + (k6 & 1u)) * 8u;
    const uint32_t sy = (chroma ? my : 2u * my + (k6 >> 1)) * 8u;
    const uint32_t cols = lane < nb && sx < pw ? min(8u, pw - sx) : 0u;
    const uint32_t rows = lane < nb && sy < ph ? min(8u, ph - sy) : 0u;
    const int16_t* const src = chroma ? (k6 == 4u ? s_cb : s_cr) + m * 8u : s_y + ((k6 >> 1) * 8u) * kPitchY + m * 16u + (k6 & 1u) * 8u;
    const uint32_t pitch = chroma ? kPitchC : kPitchY;

    // the same walk as amv_forward_kernel's: item `slot` of the launch is frame sel_frame(sel, slot), its lines in slot `slot`
    const uint32_t first = blockIdx.x / segs, stride = gridDim.x / segs;
    const uint32_t items = sel_items(sel, n);
    for (uint32_t slot = first; slot < items; slot += stride) {
        const uint32_t f = sel_frame(sel, slot);
        convert_segment<kYuv>(in, f, g, my, m0, cnt, lane, s_y, s_cb, s_cr);
        __syncthreads();
        uint32_t sum = 0u;                      // 64 squares of at most 255^2: inside 32 bits (a plane's sum is not)
        if (rows && cols) {
            const uint4* const line = reinterpret_cast<const uint4*>(coef + ((uint64_t)slot * g.mcus + (uint64_t)my * g.mcu_cols + m0) * 384u + lane * 64u);
            uint32_t c[32];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const uint4 q = line[i];
                c[4 * i] = q.x; c[4 * i + 1] = q.y; c[4 * i + 2] = q.z; c[4 * i + 3] = q.w;
            }
            int v[64];
#pragma unroll
            for (int nat = 0; nat < 64; ++nat) {
                const int scan = kScanOfNatural[nat];
                const int step = chroma ? (int)kQuantChroma[scan] : (int)kQuantLuma[scan];
                const int level = (int)(int16_t)(c[scan >> 1] >> (16 * (scan & 1)));
                v[nat] = s16(level * step + (nat == 0 ? 1024 : 0));
            }
#pragma unroll
            for (int r = 0; r < 8; ++r)
                sidct_row(v[8 * r], v[8 * r + 1], v[8 * r + 2], v[8 * r + 3], v[8 * r + 4], v[8 * r + 5], v[8 * r + 6], v[8 * r + 7]);
#pragma unroll
            for (int col = 0; col < 8; ++col)
                sidct_col(v[col], v[8 + col], v[16 + col], v[24 + col], v[32 + col], v[40 + col], v[48 + col], v[56 + col]);
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const uint4 q = *reinterpret_cast<const uint4*>(src + r * pitch);
                const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int sample = (int)(int16_t)(w[j >> 1] >> (16 * (j & 1))) + 128;   // the planes hold samples - 128
                    const int d = sample - v[8 * r + j];
                    if ((uint32_t)r < rows && (uint32_t)j < cols) sum += (uint32_t)(d * d);
                }
            }
        }
        const uint32_t sum_y = wave_sum(k6 < 4u ? sum : 0u), sum_cb = wave_sum(k6 == 4u ? sum : 0u), sum_cr = wave_sum(k6 == 5u ? sum : 0u);
        if (lane < 3u) {
            const uint32_t mine = lane == 0u ? sum_y : (lane == 1u ? sum_cb : sum_cr);
            if (mine) atomicAdd(sse + (uint64_t)f * 3u + lane, (unsigned long long)mine);
        }
        __syncthreads();                        // the planes are free again
    }
}

void launch_encode_error(const Source& in, uint32_t n, const FrameSel& sel, uint32_t items, const FrameGeom& g, const int16_t* coef,
                         uint64_t* sse, hipStream_t s) {
    if (items == 0) return;
    const SegSplit sp = seg_split(g);
    const uint64_t grid = (uint64_t)(sel.round && items > 64u ? 64u : items) * g.mcu_rows * sp.nseg;
    with_source_kind(in, [&](auto yuv) {
        hipLaunchKernelGGL((amv_encode_error_kernel<decltype(yuv)::value>), dim3((uint32_t)grid), dim3(kWave), 0, s, in, n, sel, g, sp.nseg,
                           sp.per_seg, coef, reinterpret_cast<unsigned long long*>(sse));
    });
}

}  // namespace amv
