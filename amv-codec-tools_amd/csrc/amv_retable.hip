// amv_retable.hip -- chunks coded against foreign quantiser tables re-expressed in AMV's, in the coefficient domain: the
// kernels behind the re-table entries (amvhip_requant.hip).  The arithmetic is amv_retable_plan.h's; the front (the dense
// round of lines, the frames that are coded, the in-place write-back amv_pack_kernel reads), the search, the coder and the
// choice are amv_requant.hip's, word for word: see there.  What is new:
//
//   the source tables   the call's tables (up to 64 of 128 bytes: luma then chroma, scan order) are copied to LDS once per
//                       workgroup; a frame's table is table_of[f] (nullptr: table 0).  An index that names no table makes the
//                       frame one that is not coded (lines of zeros) and sets kRetableFlagTable in its flag word.
//   amv_retable_kernel        amv_requant_kernel with retable_scale_block / retable_block_error: c = level * 8 Qs, the NEW DC
//                             in the line, the error over all 64 positions against what the chunk meant.
//   amv_retable_probe_kernel  amv_requant_probe_kernel likewise; the NEW DC goes to the workspace amv_rate_dc_kernel reads.
//   amv_retable_status_kernel behind amv_requant_finish_kernel, which reads any flag as `out of range`: a frame whose flag word
//                             has kRetableFlagTable gets AMVHIP_ST_TABLE in the place of AMVHIP_ST_RANGE.  (A frame with a
//                             bad index is never scaled, so the two flags never meet.)
#include "amv_encode_common.h"
#include "amv_rate_plan.h"
#include "amv_retable_plan.h"
#include "amv_wave.h"

namespace amv {

using namespace enc;

namespace {

struct RetableFrames {
    const int32_t* status;        // the entropy stage's
    const uint32_t* nmcu_ok;      // whole MCUs decoded
    const uint32_t* rec_count;    // the records pass: a frame whose count is ~0 is the serial kernel's (nullptr: every frame is here)
};
__device__ __forceinline__ bool frame_here(const RetableFrames& fr, uint32_t f) { return !fr.rec_count || fr.rec_count[f] != 0xffffffffu; }
__device__ __forceinline__ bool frame_coded(const RetableFrames& fr, uint32_t f, uint32_t mcus) {
    return frame_here(fr, f) && fr.status[f] == 0 && fr.nmcu_ok[f] >= mcus;
}

// the lane's line from the round into its LDS line (a granule keeps its place in line_offset's layout)
__device__ __forceinline__ void fetch_line(const int16_t* src, uint8_t* region, uint32_t lane) {
    const uint4* const s = reinterpret_cast<const uint4*>(src);
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i) *reinterpret_cast<uint4*>(region + lane * 128u + ((i ^ (lane & 7u)) << 4)) = s[i];
}

// the call's tables into LDS, by words (count <= kRetableTablesMax: the entry checks it)
__device__ __forceinline__ void load_source_tables(uint8_t* s_src, const RetableTables& rt, uint32_t tid, uint32_t nthreads) {
    const uint32_t words = (rt.count < kRetableTablesMax ? rt.count : kRetableTablesMax) * (kRetableTableBytes / 4u);
    for (uint32_t i = tid; i < words; i += nthreads) reinterpret_cast<uint32_t*>(s_src)[i] = reinterpret_cast<const uint32_t*>(rt.tables)[i];
}
// the frame's table, or count where its index names none (uniform over a wave)
__device__ __forceinline__ uint32_t table_of_frame(const RetableTables& rt, uint32_t f) {
    const uint32_t t = rt.table_of ? rt.table_of[f] : 0u;
    return t < rt.count && t < kRetableTablesMax ? t : rt.count;
}

}  // namespace

__global__ __launch_bounds__(kWave) void amv_retable_kernel(int16_t* __restrict__ coef, uint32_t n, FrameSel sel, FrameGeom g, uint32_t nseg,
                                                            uint32_t per_seg, RetableFrames fr, RetableTables rt, uint32_t lambda,
                                                            const uint32_t* __restrict__ lambdas, uint32_t* __restrict__ flags,
                                                            unsigned long long* __restrict__ err) {
    __shared__ __attribute__((aligned(16))) uint8_t s_old[64 * 128];     // the chunk's levels
    __shared__ __attribute__((aligned(16))) uint8_t s_line[64 * 128];    // level * 8 Qs, then the path's levels
    __shared__ __attribute__((aligned(16))) uint8_t s_src[kRetableTablesMax * kRetableTableBytes];
    __shared__ __attribute__((aligned(16))) TrellisTables s_tab;
    load_trellis_tables(&s_tab, threadIdx.x, kWave);
    load_source_tables(s_src, rt, threadIdx.x, kWave);
    __syncthreads();

    const uint32_t lane = threadIdx.x;
    const uint32_t segs = g.mcu_rows * nseg;
    uint32_t my, m0, cnt;
    if (!seg_place(SegSplit{nseg, per_seg}, g, blockIdx.x % segs, my, m0, cnt)) return;
    const uint32_t nb = cnt * 6u;
    const uint32_t comp = lane % 6u >= 4u ? 1u : 0u;
    const uint32_t first = blockIdx.x / segs, stride = gridDim.x / segs;
    const uint32_t items = sel_items(sel, n);
    for (uint32_t slot = first; slot < items; slot += stride) {
        const uint32_t f = sel_frame(sel, slot);
        int16_t* const mine = coef + ((uint64_t)slot * g.mcus + (uint64_t)my * g.mcu_cols + m0) * 384u + lane * 64u;
        const uint32_t t = table_of_frame(rt, f);
        bool coded = frame_coded(fr, f, g.mcus);
        if (coded && t == rt.count) {                                   // (uniform over the wave)
            if (lane == 0u) atomicOr(flags + f, kRetableFlagTable);
            coded = false;
        }
        uint32_t e = 0;
        if (lane < nb) {
            bool ok = false;
            if (coded) {
                const uint8_t* const qs = s_src + t * kRetableTableBytes + comp * 64u;
                fetch_line(mine, s_old, lane);
                LdsLine before{s_old, lane}, line{s_line, lane};
                ok = retable_scale_block(before, qs, s_tab.q[comp], line);
                if (ok) {
                    uint32_t nz_lo, nz_hi;
                    trellis_lane(s_line, lane, s_tab, kRetableQbias, lambdas ? lambdas[f] : lambda, nz_lo, nz_hi);
                    if (err) e = retable_block_error(before, line, qs, s_tab.q[comp]);
                } else {
                    atomicOr(flags + f, kRetableFlagRange);
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

__global__ __launch_bounds__(kWave) void amv_retable_probe_kernel(const int16_t* __restrict__ coef, uint32_t n, FrameSel sel, FrameGeom g,
                                                                  uint32_t nseg, uint32_t per_seg, RetableFrames fr, RetableTables rt,
                                                                  RateLadder ladder, uint32_t* __restrict__ flags, int16_t* __restrict__ dc,
                                                                  uint32_t* __restrict__ bits) {
    __shared__ __attribute__((aligned(16))) uint8_t s_old[64 * 128];
    __shared__ __attribute__((aligned(16))) uint8_t s_line[64 * 128];
    __shared__ __attribute__((aligned(16))) uint8_t s_src[kRetableTablesMax * kRetableTableBytes];
    __shared__ __attribute__((aligned(16))) TrellisTables s_tab;
    load_trellis_tables(&s_tab, threadIdx.x, kWave);
    load_source_tables(s_src, rt, threadIdx.x, kWave);
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
        const uint32_t t = table_of_frame(rt, f);
        bool coded = frame_coded(fr, f, g.mcus);
        if (coded && t == rt.count) {                              // (uniform over the wave)
            if (lane == 0u) atomicOr(flags + f, kRetableFlagTable);
            coded = false;
        }
        const uint8_t* const qs = s_src + (coded ? t : 0u) * kRetableTableBytes + comp * 64u;
        LdsLine before{s_old, lane}, line{s_line, lane};
        bool ok = false;
        if (lane < nb) {
            if (coded) {
                fetch_line(coef + ((uint64_t)slot * g.blocks + blk) * 64u, s_old, lane);
                ok = retable_scale_block(before, qs, s_tab.q[comp], line);
                if (!ok) atomicOr(flags + f, kRetableFlagRange);
            }
            dc[(uint64_t)f * g.blocks + blk] = ok ? (int16_t)line.get(0) : (int16_t)0;   // the new DC (every difference the DC launch forms has a code)
        }
        if (!coded) continue;
        for (uint32_t r = 0; r < ladder.rungs; ++r) {
            uint32_t block_bits = 0;
            if (ok) {
                if (r) retable_scale_block(before, qs, s_tab.q[comp], line);   // the walk before left levels in the line
                uint32_t nz_lo, nz_hi;
                trellis_lane(s_line, lane, s_tab, kRetableQbias, ladder.lambda[r], nz_lo, nz_hi);
                block_bits = rate_block_bits(line, len);
            }
            const uint32_t sum = wave_sum(block_bits);
            if (lane == 0u) atomicAdd(bits + (uint64_t)f * ladder.rungs + r, sum);
        }
    }
}

constexpr uint32_t kRetableStatusLanes = 256;
__global__ __launch_bounds__(kRetableStatusLanes) void amv_retable_status_kernel(uint32_t n, int32_t* __restrict__ status,
                                                                                 const uint32_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * kRetableStatusLanes + threadIdx.x;
    if (i >= n) return;
    if ((uint32_t)status[i] == kStRange && (flags[i] & kRetableFlagTable)) status[i] = (int32_t)kStTable;
}

static uint32_t retable_grid(const FrameSel& sel, uint32_t items, const FrameGeom& g, const SegSplit& sp) {
    return (uint32_t)((uint64_t)(sel.round && sel.list && items > 64u ? 64u : items) * g.mcu_rows * sp.nseg);
}

void launch_retable(int16_t* coef, uint32_t n, const FrameSel& sel, uint32_t items, const FrameGeom& g, const RequantSource& src,
                    const RetableTables& rt, uint32_t lambda, const uint32_t* lambdas, uint32_t* flags, uint64_t* err, hipStream_t s) {
    if (items == 0) return;
    const SegSplit sp = seg_split(g);
    hipLaunchKernelGGL(amv_retable_kernel, dim3(retable_grid(sel, items, g, sp)), dim3(kWave), 0, s, coef, n, sel, g, sp.nseg, sp.per_seg,
                       RetableFrames{src.status, src.nmcu_ok, src.rec_count}, rt, lambda, lambdas, flags, (unsigned long long*)err);
}

void launch_retable_probe(const int16_t* coef, uint32_t n, const FrameSel& sel, uint32_t items, const FrameGeom& g, const RequantSource& src,
                          const RetableTables& rt, const RateLadder& ladder, uint32_t* flags, int16_t* dc, uint32_t* bits, hipStream_t s) {
    if (items == 0) return;
    const SegSplit sp = seg_split(g);
    hipLaunchKernelGGL(amv_retable_probe_kernel, dim3(retable_grid(sel, items, g, sp)), dim3(kWave), 0, s, coef, n, sel, g, sp.nseg, sp.per_seg,
                       RetableFrames{src.status, src.nmcu_ok, src.rec_count}, rt, ladder, flags, dc, bits);
}

void launch_retable_status(uint32_t n, int32_t* status, const uint32_t* flags, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(amv_retable_status_kernel, dim3((n + kRetableStatusLanes - 1u) / kRetableStatusLanes), dim3(kRetableStatusLanes), 0, s, n,
                       status, flags);
}

}  // namespace amv
