// amv_requant.hip -- AMV chunks requantised in the coefficient domain, and chunks coded against foreign quantiser tables
// re-expressed in AMV's: the kernels behind the requant and the re-table entries (amvhip_requant.hip).  The arithmetic is
// amv_requant_plan.h's and amv_retable_plan.h's; the search itself is trellis_lane (amv_encode_common.h), the coder
// amv_pack_kernel, the choice amv_rate_choose_kernel / amv_rate_check_kernel -- all as they are.
//
// The front is the decoder's entropy stage.  What it leaves -- records, or the serial kernel's lines -- is brought to ONE
// form before these kernels run: a round of dense lines in the context's coefficient workspace (records through
// amv_expand_records_kernel, a round of frames at a time).  Reading the records here instead would mean the reconstruction's
// segment reader (stage A, its LDS image, its piece map) inside a kernel whose time is the walk's, twice over for the frames
// the serial kernel decodes anyway; the dense round costs one write and one read of 128 bytes a block, the same traffic
// amv_forward_kernel -> amv_pack_kernel has, and keeps one loader for both entropy modes.
//
// The two families share their bodies: search_body and probe_body are written once, over a TABLE RULE that says what the
// chunk's levels were coded against.
//   OwnTables    AMV's own: c = level * 8 Q (requant_scale_block), the error over the levels kept, the DC as it came.  No LDS.
//   CallTables   the call's tables (up to 64 of 128 bytes: luma then chroma, scan order), copied to LDS once per workgroup; a
//                frame's table is table_of[f] (nullptr: table 0).  An index that names no table makes the frame one that is
//                not coded (lines of zeros) and sets kRetableFlagTable in its flag word.  c = level * 8 Qs, the NEW DC in the
//                line (retable_scale_block), the error over all 64 positions against what the chunk meant.
// A body holds the LDS every kernel here has (each kernel its own: a body is inlined into one); the four entry points add
// their rule's and call a body:
//   amv_requant_kernel        stands where amv_forward_kernel's front half stands: one wave per MCU-row segment, a block per
//   amv_retable_kernel        lane.  The lane's line of levels goes from the round to LDS (line_offset's layout), is checked
//                             against the range rule and scaled into the lane's line of the search region, exactly as
//                             transform_block<.., true> + store_line leave it; trellis_lane with qbias 128 and the frame's
//                             lambda; the block's error; the line back to the round, IN PLACE -- amv_pack_kernel reads it
//                             there.  A frame that is not coded (its decode reported something or stopped early; in the
//                             records pass: the serial kernel's frame) gets lines of zeros, a block out of range too (and the
//                             frame's flag): whatever the coder is handed has a code.
//   amv_requant_probe_kernel  the same front, then per rung: scale again, walk, read the bits off the levels, one atomic add per
//   amv_retable_probe_kernel  wave and rung; the DCs (the rule says which) to the workspace amv_rate_dc_kernel reads.
//   amv_requant_finish_kernel a lane per frame: the decode's status, `ended early` and the range flag become d_status; a frame
//                             that is not coded loses its length, its error, its bits, and gets the last rung, flagged.
//   amv_retable_status_kernel behind amv_requant_finish_kernel, which reads any flag as `out of range`: a frame whose flag word
//                             has kRetableFlagTable gets AMVHIP_ST_TABLE in the place of AMVHIP_ST_RANGE.  (A frame with a
//                             bad index is never scaled, so the two flags never meet.)
#include "amv_encode_common.h"
#include "amv_rate_plan.h"
#include "amv_requant_plan.h"
#include "amv_retable_plan.h"
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

// ---- the table rules ------------------------------------------------------------------------------------------------------
// kLdsBytes: the LDS the rule's entry points declare and hand it (OwnTables has none); load: that LDS filled, ahead of the
// barrier; start: once per coded frame, false = not coded after all (uniform over the wave); scale / error: the plan's; dc:
// the DC the rate workspace takes; kQbias, kFlagRange: the search's rounding term, the flag of a block out of range.
struct OwnTables {
    static constexpr uint32_t kQbias = kRequantQbias, kFlagRange = 1u;
    __device__ __forceinline__ void load(uint32_t) const {}
    __device__ __forceinline__ bool start(uint32_t, uint32_t, uint32_t, uint32_t*) const { return true; }
    __device__ __forceinline__ bool scale(const LdsLine& before, const uint8_t* q, LdsLine& line) const { return requant_scale_block(before, q, line); }
    __device__ __forceinline__ uint32_t error(const LdsLine& before, const LdsLine& line, const uint8_t* q) const {
        return requant_block_error(before, line, q);
    }
    __device__ __forceinline__ int16_t dc(const LdsLine& before, const LdsLine&) const { return (int16_t)before.get(0); }
};

struct CallTables {
    static constexpr uint32_t kLdsBytes = kRetableTablesMax * kRetableTableBytes, kQbias = kRetableQbias, kFlagRange = kRetableFlagRange;
    RetableTables rt;
    uint8_t* s_src;               // kLdsBytes of LDS
    const uint8_t* qs;            // the frame's table, the lane's component (set by start)
    // the call's tables into LDS, by words (count <= kRetableTablesMax: the entry checks it)
    __device__ __forceinline__ void load(uint32_t tid) const {
        const uint32_t words = (rt.count < kRetableTablesMax ? rt.count : kRetableTablesMax) * (kRetableTableBytes / 4u);
        for (uint32_t i = tid; i < words; i += kWave) reinterpret_cast<uint32_t*>(s_src)[i] = reinterpret_cast<const uint32_t*>(rt.tables)[i];
    }
    __device__ __forceinline__ bool start(uint32_t f, uint32_t lane, uint32_t comp, uint32_t* flags) {
        const uint32_t t = rt.table_of ? rt.table_of[f] : 0u;
        if (!(t < rt.count && t < kRetableTablesMax)) {                 // the index names no table
            if (lane == 0u) atomicOr(flags + f, kRetableFlagTable);
            return false;
        }
        qs = s_src + t * kRetableTableBytes + comp * 64u;
        return true;
    }
    __device__ __forceinline__ bool scale(const LdsLine& before, const uint8_t* q, LdsLine& line) const {
        return retable_scale_block(before, qs, q, line);
    }
    __device__ __forceinline__ uint32_t error(const LdsLine& before, const LdsLine& line, const uint8_t* q) const {
        return retable_block_error(before, line, qs, q);
    }
    __device__ __forceinline__ int16_t dc(const LdsLine&, const LdsLine& line) const { return (int16_t)line.get(0); }   // the new DC
};

// ---- the two bodies -------------------------------------------------------------------------------------------------------
// Where a wave sits: its segment (MCU row my, MCUs m0 .. m0 + nb / 6), and the slots it takes -- frames as amv_forward_kernel
// takes them: item i = frame sel_frame(i), lines in slot i.  false: the wave has no segment.
struct Seat {
    uint32_t my, m0, nb, first, stride, items;
};
__device__ __forceinline__ bool seat_of(const FrameGeom& g, uint32_t nseg, uint32_t per_seg, const FrameSel& sel, uint32_t n, Seat& p) {
    const uint32_t segs = g.mcu_rows * nseg;
    uint32_t cnt;
    if (!seg_place(SegSplit{nseg, per_seg}, g, blockIdx.x % segs, p.my, p.m0, cnt)) return false;
    p.nb = cnt * 6u;
    p.first = blockIdx.x / segs;
    p.stride = gridDim.x / segs;
    p.items = sel_items(sel, n);
    return true;
}

template <class Rule>
__device__ __forceinline__ void search_body(Rule rule, int16_t* __restrict__ coef, uint32_t n, const FrameSel& sel, const FrameGeom& g,
                                            uint32_t nseg, uint32_t per_seg, const RequantFrames& fr, uint32_t lambda,
                                            const uint32_t* __restrict__ lambdas, uint32_t* __restrict__ flags,
                                            unsigned long long* __restrict__ err) {
    __shared__ __attribute__((aligned(16))) uint8_t s_old[64 * 128];     // the chunk's levels
    __shared__ __attribute__((aligned(16))) uint8_t s_line[64 * 128];    // the scaled coefficients, then the path's levels
    __shared__ __attribute__((aligned(16))) TrellisTables s_tab;
    const uint32_t lane = threadIdx.x;
    load_trellis_tables(&s_tab, lane, kWave);
    rule.load(lane);
    __syncthreads();

    Seat p;
    if (!seat_of(g, nseg, per_seg, sel, n, p)) return;
    const uint32_t comp = lane % 6u >= 4u ? 1u : 0u;
    for (uint32_t slot = p.first; slot < p.items; slot += p.stride) {
        const uint32_t f = sel_frame(sel, slot);
        int16_t* const mine = coef + ((uint64_t)slot * g.mcus + (uint64_t)p.my * g.mcu_cols + p.m0) * 384u + lane * 64u;
        const bool coded = frame_coded(fr, f, g.mcus) && rule.start(f, lane, comp, flags);   // (uniform over the wave)
        uint32_t e = 0;
        if (lane < p.nb) {
            bool ok = false;
            if (coded) {
                fetch_line(mine, s_old, lane);
                LdsLine before{s_old, lane}, line{s_line, lane};
                ok = rule.scale(before, s_tab.q[comp], line);
                if (ok) {
                    uint32_t nz_lo, nz_hi;
                    trellis_lane(s_line, lane, s_tab, Rule::kQbias, lambdas ? lambdas[f] : lambda, nz_lo, nz_hi);
                    if (err) e = rule.error(before, line, s_tab.q[comp]);
                } else {
                    atomicOr(flags + f, Rule::kFlagRange);
                }
            }
            uint4* const dst = reinterpret_cast<uint4*>(mine);
#pragma unroll
            for (uint32_t i = 0; i < 8; ++i) dst[i] = ok ? load_line_granule(s_line, lane, i) : make_uint4(0u, 0u, 0u, 0u);
        }
        if (err && coded) {        // the planes' error (uniform over the wave)
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

template <class Rule>
__device__ __forceinline__ void probe_body(Rule rule, const int16_t* __restrict__ coef, uint32_t n, const FrameSel& sel,
                                           const FrameGeom& g, uint32_t nseg, uint32_t per_seg, const RequantFrames& fr, const RateLadder& ladder,
                                           uint32_t* __restrict__ flags, int16_t* __restrict__ dc, uint32_t* __restrict__ bits) {
    __shared__ __attribute__((aligned(16))) uint8_t s_old[64 * 128];     // the chunk's levels
    __shared__ __attribute__((aligned(16))) uint8_t s_line[64 * 128];    // the scaled coefficients, then the path's levels
    __shared__ __attribute__((aligned(16))) TrellisTables s_tab;
    const uint32_t lane = threadIdx.x;
    load_trellis_tables(&s_tab, lane, kWave);
    rule.load(lane);
    __syncthreads();

    Seat p;
    if (!seat_of(g, nseg, per_seg, sel, n, p)) return;
    const uint32_t comp = lane % 6u >= 4u ? 1u : 0u;
    const uint8_t* const len = s_tab.len[comp];
    for (uint32_t slot = p.first; slot < p.items; slot += p.stride) {
        const uint32_t f = sel_frame(sel, slot);
        if (!frame_here(fr, f)) continue;                          // the serial kernel's frame: its pass fills the row
        const uint64_t blk = ((uint64_t)p.my * g.mcu_cols + p.m0) * 6u + lane;
        const bool coded = frame_coded(fr, f, g.mcus) && rule.start(f, lane, comp, flags);   // (uniform over the wave)
        LdsLine before{s_old, lane}, line{s_line, lane};
        bool ok = false;
        if (lane < p.nb) {
            if (coded) {
                fetch_line(coef + ((uint64_t)slot * g.blocks + blk) * 64u, s_old, lane);
                ok = rule.scale(before, s_tab.q[comp], line);
                if (!ok) atomicOr(flags + f, Rule::kFlagRange);
            }
            dc[(uint64_t)f * g.blocks + blk] = ok ? rule.dc(before, line) : (int16_t)0;   // (every difference the DC launch forms has a code)
        }
        if (!coded) continue;
        for (uint32_t r = 0; r < ladder.rungs; ++r) {
            uint32_t block_bits = 0;
            if (ok) {
                if (r) rule.scale(before, s_tab.q[comp], line);   // the walk before left levels in the line
                uint32_t nz_lo, nz_hi;
                trellis_lane(s_line, lane, s_tab, Rule::kQbias, ladder.lambda[r], nz_lo, nz_hi);
                block_bits = rate_block_bits(line, len);
            }
            const uint32_t sum = wave_sum(block_bits);
            if (lane == 0u) atomicAdd(bits + (uint64_t)f * ladder.rungs + r, sum);
        }
    }
}

}  // namespace

__global__ __launch_bounds__(kWave) void amv_requant_kernel(int16_t* __restrict__ coef, uint32_t n, FrameSel sel, FrameGeom g, uint32_t nseg,
                                                            uint32_t per_seg, RequantFrames fr, uint32_t lambda,
                                                            const uint32_t* __restrict__ lambdas, uint32_t* __restrict__ flags,
                                                            unsigned long long* __restrict__ err) {
    search_body(OwnTables{}, coef, n, sel, g, nseg, per_seg, fr, lambda, lambdas, flags, err);
}

__global__ __launch_bounds__(kWave) void amv_requant_probe_kernel(const int16_t* __restrict__ coef, uint32_t n, FrameSel sel, FrameGeom g,
                                                                  uint32_t nseg, uint32_t per_seg, RequantFrames fr, RateLadder ladder,
                                                                  uint32_t* __restrict__ flags, int16_t* __restrict__ dc,
                                                                  uint32_t* __restrict__ bits) {
    probe_body(OwnTables{}, coef, n, sel, g, nseg, per_seg, fr, ladder, flags, dc, bits);
}

__global__ __launch_bounds__(kWave) void amv_retable_kernel(int16_t* __restrict__ coef, uint32_t n, FrameSel sel, FrameGeom g, uint32_t nseg,
                                                            uint32_t per_seg, RequantFrames fr, RetableTables rt, uint32_t lambda,
                                                            const uint32_t* __restrict__ lambdas, uint32_t* __restrict__ flags,
                                                            unsigned long long* __restrict__ err) {
    __shared__ __attribute__((aligned(16))) uint8_t s_src[CallTables::kLdsBytes];
    search_body(CallTables{rt, s_src, s_src}, coef, n, sel, g, nseg, per_seg, fr, lambda, lambdas, flags, err);
}

__global__ __launch_bounds__(kWave) void amv_retable_probe_kernel(const int16_t* __restrict__ coef, uint32_t n, FrameSel sel, FrameGeom g,
                                                                  uint32_t nseg, uint32_t per_seg, RequantFrames fr, RetableTables rt,
                                                                  RateLadder ladder, uint32_t* __restrict__ flags, int16_t* __restrict__ dc,
                                                                  uint32_t* __restrict__ bits) {
    __shared__ __attribute__((aligned(16))) uint8_t s_src[CallTables::kLdsBytes];
    probe_body(CallTables{rt, s_src, s_src}, coef, n, sel, g, nseg, per_seg, fr, ladder, flags, dc, bits);
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

constexpr uint32_t kRetableStatusLanes = 256;
__global__ __launch_bounds__(kRetableStatusLanes) void amv_retable_status_kernel(uint32_t n, int32_t* __restrict__ status,
                                                                                 const uint32_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * kRetableStatusLanes + threadIdx.x;
    if (i >= n) return;
    if ((uint32_t)status[i] == kStRange && (flags[i] & kRetableFlagTable)) status[i] = (int32_t)kStTable;
}

static uint32_t requant_grid(const FrameSel& sel, uint32_t items, const FrameGeom& g, const SegSplit& sp) {
    return (uint32_t)((uint64_t)(sel.round && sel.list && items > 64u ? 64u : items) * g.mcu_rows * sp.nseg);
}

void launch_requant(int16_t* coef, uint32_t n, const FrameSel& sel, uint32_t items, const FrameGeom& g, const RequantSource& src,
                    const RetableTables& rt, uint32_t lambda, const uint32_t* lambdas, uint32_t* flags, uint64_t* err, hipStream_t s) {
    if (items == 0) return;
    const SegSplit sp = seg_split(g);
    const dim3 grid(requant_grid(sel, items, g, sp));
    const RequantFrames fr{src.status, src.nmcu_ok, src.rec_count};
    if (rt.tables)
        hipLaunchKernelGGL(amv_retable_kernel, grid, dim3(kWave), 0, s, coef, n, sel, g, sp.nseg, sp.per_seg, fr, rt, lambda, lambdas, flags,
                           (unsigned long long*)err);
    else
        hipLaunchKernelGGL(amv_requant_kernel, grid, dim3(kWave), 0, s, coef, n, sel, g, sp.nseg, sp.per_seg, fr, lambda, lambdas, flags,
                           (unsigned long long*)err);
}

void launch_requant_probe(const int16_t* coef, uint32_t n, const FrameSel& sel, uint32_t items, const FrameGeom& g, const RequantSource& src,
                          const RetableTables& rt, const RateLadder& ladder, uint32_t* flags, int16_t* dc, uint32_t* bits, hipStream_t s) {
    if (items == 0) return;
    const SegSplit sp = seg_split(g);
    const dim3 grid(requant_grid(sel, items, g, sp));
    const RequantFrames fr{src.status, src.nmcu_ok, src.rec_count};
    if (rt.tables)
        hipLaunchKernelGGL(amv_retable_probe_kernel, grid, dim3(kWave), 0, s, coef, n, sel, g, sp.nseg, sp.per_seg, fr, rt, ladder, flags, dc, bits);
    else
        hipLaunchKernelGGL(amv_requant_probe_kernel, grid, dim3(kWave), 0, s, coef, n, sel, g, sp.nseg, sp.per_seg, fr, ladder, flags, dc, bits);
}

void launch_requant_finish(uint32_t n, const FrameGeom& g, int32_t* status, const uint32_t* nmcu_ok, const uint32_t* flags, uint32_t* lens,
                           uint64_t* err, uint32_t* rung, uint32_t* bits, uint32_t rungs, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(amv_requant_finish_kernel, dim3((n + kRequantFinishLanes - 1u) / kRequantFinishLanes), dim3(kRequantFinishLanes), 0, s, n,
                       g.mcus, status, nmcu_ok, flags, lens, (unsigned long long*)err, rung, bits, rungs);
}

void launch_retable_status(uint32_t n, int32_t* status, const uint32_t* flags, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(amv_retable_status_kernel, dim3((n + kRetableStatusLanes - 1u) / kRetableStatusLanes), dim3(kRetableStatusLanes), 0, s, n,
                       status, flags);
}

}  // namespace amv
