// amv_encode_nr.hip -- the reference's -nr noise reduction for a whole stream: the per-stream state it carries from frame
// to frame (update_noise_reduction lavc/mpegvideo.c:861-876, denoise_dct_c lavc/mpegvideo_enc.c:2937-2959) carried on the
// device.  The arithmetic is amv_nr_plan.h's.
//
// denoise_dct_c sums the fdct outputs' magnitudes BEFORE it applies the offset, so the offsets of frame f depend on the
// pictures of the frames before it alone, not on what was coded.  Three passes:
//
//   A  amv_nr_sums_kernel    a workgroup per frame, a wave per MCU-row segment, a lane per block -- the encoder's own walk
//                            (convert_segment, fdct_row_packed, fdct8<1> of amv_encode_common.h, padding blocks included):
//                            the 64 magnitudes of every block go to LDS as a 128-byte line, lane p sums position p over the
//                            segment's lines; registers over the frame's segments, the four waves through LDS, one plain
//                            store per position.  No atomics: integer sums in a fixed order.
//   B  amv_nr_chain_kernel   one wave, lane = position, the n frames in order: halve if due, the frame's 64 offsets, add
//                            the frame's sums and block count.  Reads the caller's state, writes the state after the call.
//   C  the encoder kernels' second instantiation (amv_encode_frame_kernel and amv_forward_kernel with the offsets as
//      one more argument): the frame's 128 bytes of offsets in LDS, transform_block<true> denoises between the column pass and the quantiser.
//
// The fdct runs twice (A and C): coefficients never leave the chip.
#include "amv_encode_common.h"

namespace amv {

using namespace enc;

template <bool kYuv>
__global__ __launch_bounds__(kLanes) void amv_nr_sums_kernel(Source in, FrameGeom g, uint32_t nseg, uint32_t per_seg,
                                                             uint32_t* __restrict__ sums) {
    __shared__ __attribute__((aligned(16))) uint8_t s_region[kWaves][kRegionBytes];
    __shared__ uint32_t s_part[kWaves][kWave];

    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t f = blockIdx.x;
    uint8_t* const region = s_region[wave];
    int16_t* const s_y = reinterpret_cast<int16_t*>(region);
    int16_t* const s_cb = s_y + 16 * kPitchY;
    int16_t* const s_cr = s_cb + 8 * kPitchC;

    const uint32_t segs = g.mcu_rows * nseg;
    uint32_t acc = 0;                                  // position `lane` over this wave's segments (<= blocks x 16320 < 2^31)
    for (uint32_t s = wave; s < segs; s += kWaves) {   // (a wave's own region: no workgroup barrier inside)
        uint32_t my, m0, cnt;
        if (!seg_place(SegSplit{nseg, per_seg}, g, s, my, m0, cnt)) continue;
        const uint32_t nb = cnt * 6u;
        convert_segment<kYuv>(in, f, g, my, m0, cnt, lane, s_y, s_cb, s_cr);
        wave_sync();
        uint32_t line[32];                             // the block's magnitudes, position order, uint16 pairs
        if (lane < nb) {
            int d[8][8];
            block_row_passes(s_y, s_cb, s_cr, lane, d);
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                int col[8];
#pragma unroll
                for (int r = 0; r < 8; ++r) col[r] = d[r][c];
                fdct8<1>(col);
#pragma unroll
                for (int r = 0; r < 8; ++r) d[r][c] = (int)((r == 0 && c == 0) ? nr_magnitude_dc(col[r]) : nr_magnitude(col[r]));
            }
#pragma unroll
            for (int r = 0; r < 8; ++r)
#pragma unroll
                for (int c = 0; c < 8; c += 2) line[r * 4 + (c >> 1)] = pack16(d[r][c], d[r][c + 1]);
        }
        wave_sync();                                   // every lane has its samples: the planes become the lines
        if (lane < nb) store_line(region, lane, line);
        wave_sync();
        for (uint32_t l = 0; l < nb; ++l)              // the 64 lanes read one line's 128 bytes: two lanes a bank, the same word
            acc += *reinterpret_cast<const uint16_t*>(region + line_offset(l, lane));
        wave_sync();                                   // the lines are read: the region is free for the next segment's planes
    }
    s_part[wave][lane] = acc;
    __syncthreads();
    if (wave == 0u) sums[(uint64_t)f * 64u + lane] = s_part[0][lane] + s_part[1][lane] + s_part[2][lane] + s_part[3][lane];
}

void launch_nr_sums(const Source& in, uint32_t n, const FrameGeom& g, uint32_t* sums, hipStream_t s) {
    if (n == 0) return;
    const SegSplit sp = seg_split(g);                  // the encoder's split
    with_source_kind(in, [&](auto yuv) {
        hipLaunchKernelGGL(amv_nr_sums_kernel<decltype(yuv)::value>, dim3(n), dim3(kLanes), 0, s, in, g, sp.nseg, sp.per_seg, sums);
    });
}

// Serial in n, one integer division per frame and lane.  Between two halvings it is a plain prefix sum over the frames'
// sums; that form is not built.
__global__ __launch_bounds__(kWave) void amv_nr_chain_kernel(const uint32_t* __restrict__ sums, uint32_t n, uint32_t blocks, uint32_t nr,
                                                             int32_t* __restrict__ state, uint16_t* __restrict__ offs) {
    const uint32_t lane = threadIdx.x;
    int32_t sum = state[lane], count = state[64];
    const uint32_t at = nr_consumed_index(lane);
    uint32_t next = n ? sums[lane] : 0u;
    for (uint32_t f = 0; f < n; ++f) {
        const uint32_t add = next;
        if (f + 1u < n) next = sums[(uint64_t)(f + 1u) * 64u + lane];   // on its way during the division
        if (nr_halving_due(count)) { sum >>= 1; count >>= 1; }
        offs[(uint64_t)f * 64u + at] = nr_offset(nr, count, sum);
        sum = (int32_t)((uint32_t)sum + add);
        count = (int32_t)((uint32_t)count + blocks);
    }
    __builtin_amdgcn_wave_barrier();                   // every lane has read state[64]
    state[lane] = sum;
    if (lane == 0u) state[64] = count;
}

void launch_nr_chain(const uint32_t* sums, uint32_t n, uint32_t blocks, uint32_t nr, int32_t* state, uint16_t* offs, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(amv_nr_chain_kernel, dim3(1), dim3(kWave), 0, s, sums, n, blocks, nr, state, offs);
}

}  // namespace amv
