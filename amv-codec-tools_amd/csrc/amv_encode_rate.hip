// amv_encode_rate.hip -- a byte budget per frame, met by a search over the trellis quantiser's lambda: the kernels behind the
// rate entries (amvhip_encode.hip: rate_core, probe_core).  The arithmetic is amv_rate_plan.h's.
//
//   amv_rate_probe_kernel   one wave per MCU-row segment, a block per lane, as amv_forward_kernel: colour conversion into the
//                           LDS planes, row and column passes (denoised where offsets are given), the DC quantised -- once.
//                           The un-quantised line stays in the lane's registers (32 dwords); per rung of the ladder it goes
//                           back to the lane's LDS line, trellis_block (unchanged) turns it into levels there, the block's
//                           AC + EOB bits are read off the levels, summed over the wave, and one atomic add per wave and
//                           rung goes to bits[frame][rung].  Integer sums: the order of the adds does not show.
//                           The block's quantised DC goes to a workspace, int16 [n][blocks].
//   amv_rate_dc_kernel      the DC term, which does not depend on lambda: a lane per block, the difference to the block's
//                           predecessor of the same component (which may sit in another wave's segment: hence a second
//                           launch), its code and magnitude bits, summed and added to every rung of the frame.
//   amv_rate_choose_kernel  a lane per frame: the first floor-fit -> the frame's rung and lambda.
//   amv_rate_check_kernel   a lane per coded frame: over its budget and not final -> the next floor-fit, a place in the next
//                           pass's list.
// Nothing packs a byte here and nothing is read back: the chunks themselves are amv_forward_kernel's (its instantiations with
// a lambda per frame) and amv_pack_kernel's.
#include "amv_encode_common.h"
#include "amv_rate_plan.h"
#include "amv_wave.h"

namespace amv {

using namespace enc;

__device__ const RateDcLen kRateDcLen = make_rate_dc_len();

template <bool kYuv, bool kNr>
__global__ __launch_bounds__(kWave) void amv_rate_probe_kernel(Source in, uint32_t n, FrameGeom g, uint32_t nseg, uint32_t per_seg, uint32_t qbias,
                                                               const uint16_t* __restrict__ offsets, RateLadder ladder,
                                                               int16_t* __restrict__ dc, uint32_t* __restrict__ bits) {
    __shared__ __attribute__((aligned(16))) int16_t s_planes[kPlaneSamples];
    __shared__ __attribute__((aligned(16))) uint32_t s_qmul[kQuantMulWords];
    __shared__ __attribute__((aligned(16))) uint32_t s_nr_off[32];
    __shared__ __attribute__((aligned(16))) TrellisTables s_tab;
    load_trellis_tables(&s_tab, threadIdx.x, kWave);
    load_quant_mul(s_qmul, threadIdx.x, kWave);
    int16_t* const s_y = s_planes;
    int16_t* const s_cb = s_planes + 16 * kPitchY;
    int16_t* const s_cr = s_cb + 8 * kPitchC;

    const uint32_t lane = threadIdx.x;
    const uint32_t segs = g.mcu_rows * nseg;
    const uint32_t f = blockIdx.x / segs;
    uint32_t my, m0, cnt;
    if (f >= n || !seg_place(SegSplit{nseg, per_seg}, g, blockIdx.x % segs, my, m0, cnt)) return;
    const uint32_t nb = cnt * 6u;
    convert_segment<kYuv>(in, f, g, my, m0, cnt, lane, s_y, s_cb, s_cr);
    if (kNr && lane < 32u) s_nr_off[lane] = reinterpret_cast<const uint32_t*>(offsets + (uint64_t)f * 64u)[lane];
    __syncthreads();
    uint32_t out[32], nz_lo, nz_hi;
    if (lane < nb) transform_block<kNr, true>(s_y, s_cb, s_cr, s_qmul, lane, qbias, out, nz_lo, nz_hi, reinterpret_cast<const uint16_t*>(s_nr_off));
    __syncthreads();                       // every lane has its samples: the planes become the lines
    uint8_t* const region = reinterpret_cast<uint8_t*>(s_planes);
    if (lane < nb) dc[(uint64_t)f * g.blocks + ((uint64_t)my * g.mcu_cols + m0) * 6u + lane] = (int16_t)(out[0] & 0xffffu);
    const uint8_t* const len = s_tab.len[lane % 6u >= 4u ? 1 : 0];
    for (uint32_t r = 0; r < ladder.rungs; ++r) {
        uint32_t block_bits = 0;
        if (lane < nb) {
            store_line(region, lane, out);  // the lane's own line: the walk before left levels in it
            trellis_lane(region, lane, s_tab, qbias, ladder.lambda[r], nz_lo, nz_hi);
            block_bits = rate_block_bits(LdsLine{region, lane}, len);
        }
        const uint32_t sum = wave_sum(block_bits);
        if (lane == 0u) atomicAdd(bits + (uint64_t)f * ladder.rungs + r, sum);
    }
}

constexpr uint32_t kRateDcLanes = 256;
__global__ __launch_bounds__(kRateDcLanes) void amv_rate_dc_kernel(const int16_t* __restrict__ dc, uint32_t n, uint32_t blocks, uint32_t chunks,
                                                                   uint32_t rungs, uint32_t* __restrict__ bits) {
    const uint32_t f = blockIdx.x / chunks, b = (blockIdx.x - f * chunks) * kRateDcLanes + threadIdx.x;
    if (f >= n) return;
    uint32_t mine = 0;
    if (b < blocks) {
        const int16_t* const frame = dc + (uint64_t)f * blocks;
        const int64_t before = rate_dc_predecessor(b);
        const int32_t diff = (int32_t)frame[b] - (before < 0 ? 0 : (int32_t)frame[before]);
        mine = rate_dc_bits(kRateDcLen.len[b % 6u >= 4u ? 1 : 0], diff);
    }
    const uint32_t sum = wave_sum(mine);
    const uint32_t lane = threadIdx.x & 63u;
    if (sum && lane < rungs) atomicAdd(bits + (uint64_t)f * rungs + lane, sum);
}

void launch_rate_probe(const Source& in, uint32_t n, const FrameGeom& g, uint32_t qbias, const uint16_t* offsets, const RateLadder& ladder,
                       int16_t* dc, uint32_t* bits, hipStream_t s) {
    if (n == 0) return;
    const SegSplit sp = seg_split(g);
    const uint64_t grid = (uint64_t)n * g.mcu_rows * sp.nseg;
    with_source_kind(in, [&](auto yuv) {
        if (offsets)
            hipLaunchKernelGGL((amv_rate_probe_kernel<decltype(yuv)::value, true>), dim3((uint32_t)grid), dim3(kWave), 0, s, in, n, g, sp.nseg,
                               sp.per_seg, qbias, offsets, ladder, dc, bits);
        else
            hipLaunchKernelGGL((amv_rate_probe_kernel<decltype(yuv)::value, false>), dim3((uint32_t)grid), dim3(kWave), 0, s, in, n, g, sp.nseg,
                               sp.per_seg, qbias, offsets, ladder, dc, bits);
    });
    launch_rate_dc(dc, n, g.blocks, ladder.rungs, bits, s);
}

void launch_rate_dc(const int16_t* dc, uint32_t n, uint32_t blocks, uint32_t rungs, uint32_t* bits, hipStream_t s) {
    if (n == 0) return;
    const uint32_t chunks = (blocks + kRateDcLanes - 1u) / kRateDcLanes;
    hipLaunchKernelGGL(amv_rate_dc_kernel, dim3((uint32_t)((uint64_t)n * chunks)), dim3(kRateDcLanes), 0, s, dc, n, blocks, chunks, rungs, bits);
}

// ---- the choice -----------------------------------------------------------------------------------------------------------

constexpr uint32_t kRateChoiceLanes = 256;
__global__ __launch_bounds__(kRateChoiceLanes) void amv_rate_choose_kernel(const uint32_t* __restrict__ bits, RateLadder ladder,
                                                                           const uint32_t* __restrict__ budgets, uint32_t budget, uint32_t n,
                                                                           uint32_t* __restrict__ rung, uint32_t* __restrict__ lambda) {
    const uint32_t i = blockIdx.x * kRateChoiceLanes + threadIdx.x;
    if (i >= n) return;
    const uint32_t record = rate_choose(bits + (uint64_t)i * ladder.rungs, ladder.rungs, budgets ? budgets[i] : budget);
    rung[i] = record;
    lambda[i] = ladder.lambda[record & ~kRateOver];
}

// The launch is small (a pass usually has few frames or none, and the host cannot know): its lanes walk the list.
__global__ __launch_bounds__(kRateChoiceLanes) void amv_rate_check_kernel(const uint32_t* __restrict__ bits, RateLadder ladder,
                                                                          const uint32_t* __restrict__ budgets, uint32_t budget, uint32_t n,
                                                                          const uint32_t* __restrict__ lens, const uint32_t* __restrict__ list,
                                                                          const uint32_t* __restrict__ count, uint32_t* __restrict__ rung,
                                                                          uint32_t* __restrict__ lambda, uint32_t* __restrict__ next,
                                                                          uint32_t* __restrict__ next_count) {
    const uint32_t items = list ? min(*count, n) : n;
    for (uint32_t p = blockIdx.x * kRateChoiceLanes + threadIdx.x; p < items; p += gridDim.x * kRateChoiceLanes) {
        const uint32_t i = list ? list[p] : p;
        uint32_t record = rung[i];
        if (!rate_check(bits + (uint64_t)i * ladder.rungs, ladder.rungs, budgets ? budgets[i] : budget, lens[i], record)) {
            rung[i] = record;              // (the flag alone may have changed)
            continue;
        }
        rung[i] = record;
        lambda[i] = ladder.lambda[record & ~kRateOver];
        next[atomicAdd(next_count, 1u)] = i;   // a frame is in a pass's list once: at most n entries
    }
}

void launch_rate_choose(const uint32_t* bits, const RateLadder& ladder, const uint32_t* budgets, uint32_t budget, uint32_t n, uint32_t* rung,
                        uint32_t* lambda, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(amv_rate_choose_kernel, dim3((n + kRateChoiceLanes - 1u) / kRateChoiceLanes), dim3(kRateChoiceLanes), 0, s, bits, ladder,
                       budgets, budget, n, rung, lambda);
}

void launch_rate_check(const uint32_t* bits, const RateLadder& ladder, const uint32_t* budgets, uint32_t budget, uint32_t n, const uint32_t* lens,
                       const uint32_t* list, const uint32_t* count, uint32_t* rung, uint32_t* lambda, uint32_t* next, uint32_t* next_count,
                       hipStream_t s) {
    if (n == 0) return;
    const uint32_t full = (n + kRateChoiceLanes - 1u) / kRateChoiceLanes;
    hipLaunchKernelGGL(amv_rate_check_kernel, dim3(list && full > 8u ? 8u : full), dim3(kRateChoiceLanes), 0, s, bits, ladder, budgets, budget, n,
                       lens, list, count, rung, lambda, next, next_count);
}

}  // namespace amv
