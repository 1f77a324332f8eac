// amv_requant.hip -- AMV chunks requantised in the coefficient domain: the kernels behind the requant entries
// (amvhip_requant.hip).  The arithmetic is amv_requant_plan.h's; the search itself is trellis_lane (amv_encode_common.h),
// the coder amv_pack_kernel, the choice amv_rate_choose_kernel / amv_rate_check_kernel -- all as they are.
//
// The front is the decoder's entropy stage.  What it leaves -- records, or the serial kernel's lines -- is brought to ONE
// form before these kernels run: a round of dense lines in the context's coefficient workspace (records through
// amv_expand_records_kernel, a round of frames at a time).  Reading the records here instead would mean the reconstruction's
// segment reader (stage A, its LDS image, its piece map) inside a kernel whose time is the walk's, twice over for the frames
// the serial kernel decodes anyway; the dense round costs one write and one read of 128 bytes a block, the same traffic
// amv_forward_kernel -> amv_pack_kernel has, and keeps one loader for both entropy modes.
//
//   amv_requant_kernel        stands where amv_forward_kernel's front half stands: one wave per MCU-row segment, a block per
//                             lane.  The lane's line of levels goes from the round to LDS (line_offset's layout), is checked
//                             against the range rule and scaled to level * 8 Q into the lane's line of the search region,
//                             exactly as transform_block<.., true> + store_line leave it; trellis_lane with qbias 128 and the
//                             frame's lambda; the block's error against the levels kept; the line back to the round, IN
//                             PLACE -- amv_pack_kernel reads it there.  A frame that is not coded (its decode reported
//                             something or stopped early; in the records pass: the serial kernel's frame) gets lines of
//                             zeros, a block out of range too (and the frame's flag): whatever the coder is handed has a code.
//   amv_requant_probe_kernel  the same front, then per rung: scale again, walk, read the bits off the levels, one atomic add per
//                             wave and rung; the DCs to the workspace amv_rate_dc_kernel reads.
//   amv_requant_finish_kernel a lane per frame: the decode's status, `ended early` and the range flag become d_status; a frame
//                             that is not coded loses its length, its error, its bits, and gets the last rung, flagged.
#include "amv_encode_common.h"
#include "amv_rate_plan.h"
#include "amv_requant_plan.h"
#include "amv_wave.h"

namespace amv {

using namespace enc;

namespace {

// Which frames of a launch are coded at all (uniform over a wave: all of it per frame)
struct RequantFrames {
    const int32_t* status;        // the entropy stage's
    const uint32_t* nmcu_ok;      // whole MCUs decoded
    const uint32_t* rec_count;    // the records pass: a frame whose count is ~0 is the serial kernel's (nullptr: every frame is here)
};
__device__ __forceinline__ bool frame_here(const RequantFrames& fr, uint32_t f) { return !fr.rec_count || fr.rec_count[f] != 0xffffffffu; }
__device__ __forceinline__ bool frame_coded(const RequantFrames& fr, uint32_t f, uint32_t mcus) {
    return frame_here(fr, f) && fr.status[f] == 0 && fr.nmcu_ok[f] >= mcus;
}

// the lane's line from the round into its LDS line (a granule keeps its place in line_offset's layout)
__device__ __forceinline__ void fetch_line(const int16_t* src, uint8_t* region, uint32_t lane) {
    const uint4* const s = reinterpret_cast<const uint4*>(src);
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i) *reinterpret_cast<uint4*>(region + lane * 128u + ((i ^ (lane & 7u)) << 4)) = s[i];
}

}  // namespace

__global__ __launch_bounds__(kWave) void amv_requant_kernel(int16_t* __restrict__ coef, uint32_t n, FrameSel sel, FrameGeom g, uint32_t nseg,
                                                            uint32_t per_seg, RequantFrames fr, uint32_t lambda,
                                                            const uint32_t* __restrict__ lambdas, uint32_t* __restrict__ flags,
                                                            unsigned long long* __restrict__ err) {
    __shared__ __attribute__((aligned(16))) uint8_t s_old[64 * 128];     // the chunk's levels
    __shared__ __attribute__((aligned(16))) uint8_t s_line[64 * 128];    // level * 8 Q, then the path's levels
    __shared__ __attribute__((aligned(16))) TrellisTables s_tab;
    load_trellis_tables(&s_tab, threadIdx.x, kWave);
    __syncthreads();

    const uint32_t lane = threadIdx.x;
    const uint32_t segs = g.mcu_rows * nseg;
    uint32_t my, m0, cnt;
    if (!seg_place(SegSplit{nseg, per_seg}, g, blockIdx.x % segs, my, m0, cnt)) return;
    const uint32_t nb = cnt * 6u;
    const uint32_t comp = lane % 6u >= 4u ? 1u : 0u;
    // frames as amv_forward_kernel takes them: item i = frame sel_frame(i), lines in slot i
    const uint32_t first = blockIdx.x / segs, stride = gridDim.x / segs;
    const uint32_t items = sel_items(sel, n);
    for (uint32_t slot = first; slot < items; slot += stride) {
        const uint32_t f = sel_frame(sel, slot);
        int16_t* const mine = coef + ((uint64_t)slot * g.mcus + (uint64_t)my * g.mcu_cols + m0) * 384u + lane * 64u;
        const bool coded = frame_coded(fr, f, g.mcus);
        uint32_t e = 0;
        if (lane < nb) {
            bool ok = false;
            if (coded) {
                fetch_line(mine, s_old, lane);
                LdsLine before{s_old, lane}, line{s_line, lane};
                ok = requant_scale_block(before, s_tab.q[comp], line);
                if (ok) {
                    uint32_t nz_lo, nz_hi;
                    trellis_lane(s_line, lane, s_tab, kRequantQbias, lambdas ? lambdas[f] : lambda, nz_lo, nz_hi);
                    if (err) e = requant_block_error(before, line, s_tab.q[comp]);
                } else {
                    atomicOr(flags + f, 1u);
                }
            }
            uint4* const dst = reinterpret_cast<uint4*>(mine);
#pragma unroll
            for (uint32_t i = 0; i < 8; ++i) dst[i] = ok ? load_line_granule(s_line, lane, i) : make_uint4(0u, 0u, 0u, 0u);
        }
        if (err && coded) {        // (uniform over the wave)
            const uint32_t k6 = lane % 6u;
            const uint32_t y = wave_sum(k6 < 4u ? e : 0u), cb = wave_sum(k6 == 4u ? e : 0u), cr = wave_sum(k6 == 5u ? e : 0u);
            if (lane == 0u) {
                if (y) atomicAdd(err + (uint64_t)f * 3u, (unsigned long long)y);
                if (cb) atomicAdd(err + (uint64_t)f * 3u + 1u, (unsigned long long)cb);
                if (cr) atomicAdd(err + (uint64_t)f * 3u + 2u, (unsigned long long)cr);
            }
        }
    }
}

__global__ __launch_bounds__(kWave) void amv_requant_probe_kernel(const int16_t* __restrict__ coef, uint32_t n, FrameSel sel, FrameGeom g,
                                                                  uint32_t nseg, uint32_t per_seg, RequantFrames fr, RateLadder ladder,
                                                                  uint32_t* __restrict__ flags, int16_t* __restrict__ dc,
                                                                  uint32_t* __restrict__ bits) {
    __shared__ __attribute__((aligned(16))) uint8_t s_old[64 * 128];
    __shared__ __attribute__((aligned(16))) uint8_t s_line[64 * 128];
    __shared__ __attribute__((aligned(16))) TrellisTables s_tab;
    load_trellis_tables(&s_tab, threadIdx.x, kWave);
    __syncthreads();

    const uint32_t lane = threadIdx.x;
    const uint32_t segs = g.mcu_rows * nseg;
    uint32_t my, m0, cnt;
    if (!seg_place(SegSplit{nseg, per_seg}, g, blockIdx.x % segs, my, m0, cnt)) return;
    const uint32_t nb = cnt * 6u;
    const uint32_t comp = lane % 6u >= 4u ? 1u : 0u;
    const uint8_t* const len = s_tab.len[comp];
    const uint32_t first = blockIdx.x / segs, stride = gridDim.x / segs;
    const uint32_t items = sel_items(sel, n);
    for (uint32_t slot = first; slot < items; slot += stride) {
        const uint32_t f = sel_frame(sel, slot);
        if (!frame_here(fr, f)) continue;                          // the serial kernel's frame: its pass fills the row
        const uint64_t blk = ((uint64_t)my * g.mcu_cols + m0) * 6u + lane;
        const bool coded = frame_coded(fr, f, g.mcus);
        LdsLine before{s_old, lane}, line{s_line, lane};
        bool ok = false;
        if (lane < nb) {
            if (coded) {
                fetch_line(coef + ((uint64_t)slot * g.blocks + blk) * 64u, s_old, lane);
                ok = requant_scale_block(before, s_tab.q[comp], line);
                if (!ok) atomicOr(flags + f, 1u);
            }
            dc[(uint64_t)f * g.blocks + blk] = ok ? (int16_t)before.get(0) : (int16_t)0;   // (every difference the DC launch forms has a code)
        }
        if (!coded) continue;
        for (uint32_t r = 0; r < ladder.rungs; ++r) {
            uint32_t block_bits = 0;
            if (ok) {
                if (r) requant_scale_block(before, s_tab.q[comp], line);   // the walk before left levels in the line
                uint32_t nz_lo, nz_hi;
                trellis_lane(s_line, lane, s_tab, kRequantQbias, ladder.lambda[r], nz_lo, nz_hi);
                block_bits = rate_block_bits(line, len);
            }
            const uint32_t sum = wave_sum(block_bits);
            if (lane == 0u) atomicAdd(bits + (uint64_t)f * ladder.rungs + r, sum);
        }
    }
}

constexpr uint32_t kRequantFinishLanes = 256;
__global__ __launch_bounds__(kRequantFinishLanes) void amv_requant_finish_kernel(uint32_t n, uint32_t mcus, int32_t* __restrict__ status,
                                                                                 const uint32_t* __restrict__ nmcu_ok,
                                                                                 const uint32_t* __restrict__ flags, uint32_t* __restrict__ lens,
                                                                                 unsigned long long* __restrict__ err, uint32_t* __restrict__ rung,
                                                                                 uint32_t* __restrict__ bits, uint32_t rungs) {
    const uint32_t i = blockIdx.x * kRequantFinishLanes + threadIdx.x;
    if (i >= n) return;
    uint32_t st = (uint32_t)status[i];
    if (!st && nmcu_ok[i] < mcus) st = kStTruncated;           // (a decode that stops early says why; should one not, this is why)
    else if (!st && flags[i]) st = kStRange;
    if (!st) return;
    status[i] = (int32_t)st;
    if (lens) lens[i] = 0u;
    if (err) err[(uint64_t)i * 3u] = err[(uint64_t)i * 3u + 1u] = err[(uint64_t)i * 3u + 2u] = 0ull;
    if (rung) rung[i] = (rungs - 1u) | kRateOver;
    if (bits)
        for (uint32_t r = 0; r < rungs; ++r) bits[(uint64_t)i * rungs + r] = 0u;
}

static uint32_t requant_grid(const FrameSel& sel, uint32_t items, const FrameGeom& g, const SegSplit& sp) {
    return (uint32_t)((uint64_t)(sel.round && sel.list && items > 64u ? 64u : items) * g.mcu_rows * sp.nseg);
}

void launch_requant(int16_t* coef, uint32_t n, const FrameSel& sel, uint32_t items, const FrameGeom& g, const RequantSource& src, uint32_t lambda,
                    const uint32_t* lambdas, uint32_t* flags, uint64_t* err, hipStream_t s) {
    if (items == 0) return;
    const SegSplit sp = seg_split(g);
    hipLaunchKernelGGL(amv_requant_kernel, dim3(requant_grid(sel, items, g, sp)), dim3(kWave), 0, s, coef, n, sel, g, sp.nseg, sp.per_seg,
                       RequantFrames{src.status, src.nmcu_ok, src.rec_count}, lambda, lambdas, flags, (unsigned long long*)err);
}

void launch_requant_probe(const int16_t* coef, uint32_t n, const FrameSel& sel, uint32_t items, const FrameGeom& g, const RequantSource& src,
                          const RateLadder& ladder, uint32_t* flags, int16_t* dc, uint32_t* bits, hipStream_t s) {
    if (items == 0) return;
    const SegSplit sp = seg_split(g);
    hipLaunchKernelGGL(amv_requant_probe_kernel, dim3(requant_grid(sel, items, g, sp)), dim3(kWave), 0, s, coef, n, sel, g, sp.nseg, sp.per_seg,
                       RequantFrames{src.status, src.nmcu_ok, src.rec_count}, ladder, flags, dc, bits);
}

void launch_requant_finish(uint32_t n, const FrameGeom& g, int32_t* status, const uint32_t* nmcu_ok, const uint32_t* flags, uint32_t* lens,
                           uint64_t* err, uint32_t* rung, uint32_t* bits, uint32_t rungs, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(amv_requant_finish_kernel, dim3((n + kRequantFinishLanes - 1u) / kRequantFinishLanes), dim3(kRequantFinishLanes), 0, s, n,
                       g.mcus, status, nmcu_ok, flags, lens, (unsigned long long*)err, rung, bits, rungs);
}

}  // namespace amv
