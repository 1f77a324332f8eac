// amv_encode_clip.hip -- a byte budget per clip: the layer above the per-frame search of amv_encode_rate.hip.  The kernels
// behind the clip entries (amvhip_encode.hip: clip_core; amvhip_requant.hip).  The arithmetic is amv_clip_plan.h's.
//
//   amv_clip_floor_kernel   a lane per frame: from the frame's row of the bits table its part of the floor sum F(c) for
//                           every clip rung c (clip_floor), summed over the wave, one 64-bit atomic add per wave and rung
//                           into F[rungs].  Integer sums: the order of the adds does not show.
//   amv_clip_start_kernel   a lane per frame: the first c whose F(c) <= total (every lane reads it off F, which nothing
//                           writes any more) -> the frame's record and lambda at that c, in the place of
//                           amv_rate_choose_kernel; the first lane notes c in the clip's state.
//   amv_clip_settle_kernel  behind every amv_rate_check_kernel.  One workgroup.  The check left a list: nothing to do, the
//                           redo passes go on.  It left none: every frame is settled at the clip rung, so the lengths are
//                           summed to S (a partial sum per wave in LDS) and the clip step is taken (clip_step): final -> the
//                           clip record is written and `done` set, after which every later check and settle finds an empty
//                           list and `done` and leaves; otherwise the frames below the new rung move (clip_move), get
//                           their lambda and form the next pass's list.  A move that lists no frame changes no length: the
//                           next step follows at once.
// A frame the requant entry does not code (ClipFrames) adds nothing to F or S and never moves.
// Nothing packs a byte here and nothing is read back.
#include "amv_clip_plan.h"
#include "amv_kernels.h"
#include "amv_wave.h"

namespace amv {

namespace {

__device__ __forceinline__ bool clip_coded(const ClipFrames& fr, uint32_t i) {
    return !fr.status || (fr.status[i] == 0 && fr.nmcu_ok[i] >= fr.mcus && fr.flags[i] == 0u);
}
// the sum of v over the wave, in every lane: 16 bits at a time through wave_sum (64 * 65535 < 2^32)
__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
    uint64_t sum = 0;
#pragma unroll
    for (uint32_t part = 0; part < 4u; ++part) sum += (uint64_t)wave_sum((uint32_t)(v >> (16u * part)) & 0xffffu) << (16u * part);
    return sum;
}

}  // namespace

constexpr uint32_t kClipLanes = 256;
constexpr uint32_t kClipSettleLanes = 1024;

__global__ __launch_bounds__(kClipLanes) void amv_clip_floor_kernel(const uint32_t* __restrict__ bits, uint32_t rungs,
                                                                    const uint32_t* __restrict__ budgets, uint32_t budget, uint32_t n,
                                                                    ClipFrames fr, unsigned long long* __restrict__ F) {
    const uint32_t i = blockIdx.x * kClipLanes + threadIdx.x;
    const bool live = i < n && clip_coded(fr, i);
    uint32_t row[kRateRungsMax];
    uint32_t mine = 0;
    if (live) {
        mine = budgets ? budgets[i] : budget;
#pragma unroll
        for (uint32_t r = 0; r < kRateRungsMax; ++r) row[r] = r < rungs ? bits[(uint64_t)i * rungs + r] : 0u;
    }
    for (uint32_t c = 0; c < rungs; ++c) {
        const uint64_t sum = wave_sum64(live ? (uint64_t)clip_floor(row, rungs, mine, c) : 0ull);
        if ((threadIdx.x & (kWave - 1u)) == 0u && sum) atomicAdd(F + c, (unsigned long long)sum);
    }
}

__global__ __launch_bounds__(kClipLanes) void amv_clip_start_kernel(const uint32_t* __restrict__ bits, RateLadder ladder,
                                                                    const uint32_t* __restrict__ budgets, uint32_t budget, uint32_t n,
                                                                    ClipFrames fr, const unsigned long long* __restrict__ F, uint64_t total,
                                                                    ClipState* __restrict__ state, uint32_t* __restrict__ rung,
                                                                    uint32_t* __restrict__ lambda) {
    const uint32_t i = blockIdx.x * kClipLanes + threadIdx.x;
    uint64_t sums[kRateRungsMax];
#pragma unroll
    for (uint32_t c = 0; c < kRateRungsMax; ++c) sums[c] = c < ladder.rungs ? (uint64_t)F[c] : 0ull;
    const uint32_t c0 = clip_first_rung(sums, ladder.rungs, total, 0u);
    if (i == 0u) state->c = c0;
    if (i >= n) return;
    const uint32_t last = (ladder.rungs - 1u) | kRateOver;
    const uint32_t record =
        clip_coded(fr, i) ? clip_record_at(bits + (uint64_t)i * ladder.rungs, ladder.rungs, budgets ? budgets[i] : budget, c0) : last;
    rung[i] = record;
    lambda[i] = ladder.lambda[record & ~kRateOver];
}

__global__ __launch_bounds__(kClipSettleLanes) void amv_clip_settle_kernel(const uint32_t* __restrict__ bits, RateLadder ladder,
                                                                           const uint32_t* __restrict__ budgets, uint32_t budget, uint32_t n,
                                                                           ClipFrames fr, const uint32_t* __restrict__ lens,
                                                                           const unsigned long long* __restrict__ F, uint64_t total,
                                                                           ClipState* __restrict__ state, uint32_t* __restrict__ rung,
                                                                           uint32_t* __restrict__ lambda, uint32_t* __restrict__ next,
                                                                           uint32_t* __restrict__ next_count, unsigned long long* __restrict__ clip) {
    __shared__ uint64_t s_part[kClipSettleLanes / kWave];
    __shared__ uint64_t s_F[kRateRungsMax];
    __shared__ uint32_t s_idle, s_c, s_final, s_moved;
    const uint32_t lane = threadIdx.x, rungs = ladder.rungs;
    if (lane == 0u) s_idle = (*next_count != 0u || state->done != 0u) ? 1u : 0u;   // (one read: the lanes below append to the list)
    if (lane < kRateRungsMax) s_F[lane] = lane < rungs ? (uint64_t)F[lane] : 0ull;
    __syncthreads();
    if (s_idle) return;

    uint64_t mine = 0;
    for (uint32_t i = lane; i < n; i += kClipSettleLanes)
        if (clip_coded(fr, i)) mine += lens[i];
    const uint64_t wave = wave_sum64(mine);
    if ((lane & (kWave - 1u)) == 0u) s_part[lane / kWave] = wave;
    __syncthreads();
    uint64_t S = 0;
    for (uint32_t w = 0; w < kClipSettleLanes / kWave; ++w) S += s_part[w];

    uint32_t c = state->c;                       // (written below by lane 0 alone, behind a barrier every lane has passed)
    for (;;) {
        if (lane == 0u) {
            uint64_t record[2];
            uint32_t to = c;
            s_final = clip_step(s_F, rungs, total, S, to, record) ? 1u : 0u;
            s_c = to;
            s_moved = 0u;
            if (s_final) {
                clip[0] = record[0];
                clip[1] = record[1];
                state->done = 1u;
            }
        }
        __syncthreads();
        if (s_final) return;
        c = s_c;
        for (uint32_t i = lane; i < n; i += kClipSettleLanes) {
            if (!clip_coded(fr, i)) continue;
            uint32_t record = rung[i];
            if (!clip_move(bits + (uint64_t)i * rungs, rungs, budgets ? budgets[i] : budget, c, record)) continue;
            rung[i] = record;
            lambda[i] = ladder.lambda[record & ~kRateOver];
            next[atomicAdd(next_count, 1u)] = i;   // a frame is in a pass's list once: at most n entries
            s_moved = 1u;
        }
        __syncthreads();
        if (s_moved) {
            if (lane == 0u) state->c = c;
            return;
        }
        __syncthreads();                           // (lane 0 rewrites s_moved above)
    }
}

void launch_clip_floor(const uint32_t* bits, uint32_t rungs, const uint32_t* budgets, uint32_t budget, uint32_t n, const ClipFrames& fr,
                       uint64_t* F, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(amv_clip_floor_kernel, dim3((n + kClipLanes - 1u) / kClipLanes), dim3(kClipLanes), 0, s, bits, rungs, budgets, budget, n, fr,
                       (unsigned long long*)F);
}

void launch_clip_start(const uint32_t* bits, const RateLadder& ladder, const uint32_t* budgets, uint32_t budget, uint32_t n, const ClipFrames& fr,
                       const uint64_t* F, uint64_t total, ClipState* state, uint32_t* rung, uint32_t* lambda, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(amv_clip_start_kernel, dim3((n + kClipLanes - 1u) / kClipLanes), dim3(kClipLanes), 0, s, bits, ladder, budgets, budget, n, fr,
                       (const unsigned long long*)F, total, state, rung, lambda);
}

void launch_clip_settle(const uint32_t* bits, const RateLadder& ladder, const uint32_t* budgets, uint32_t budget, uint32_t n, const ClipFrames& fr,
                        const uint32_t* lens, const uint64_t* F, uint64_t total, ClipState* state, uint32_t* rung, uint32_t* lambda, uint32_t* next,
                        uint32_t* next_count, uint64_t* clip, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(amv_clip_settle_kernel, dim3(1), dim3(kClipSettleLanes), 0, s, bits, ladder, budgets, budget, n, fr, lens,
                       (const unsigned long long*)F, total, state, rung, lambda, next, next_count, (unsigned long long*)clip);
}

}  // namespace amv
