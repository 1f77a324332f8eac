// amv_clip_plan.h -- the arithmetic of the byte budget per CLIP, free of HIP: what the kernels of amv_encode_clip.hip and
// tests/c/clip_plan_test.cc both run.  It stands on amv_rate_plan.h (the ladder, floors, the first fit per frame).
//
// The definition (include/amvhip.h): for a clip rung c, frame i is coded at r_c(i), the first r >= c with len_r(i) <= B(i)
// (none: the last rung, flagged); S(c) is the sum of those lengths; the clip is coded at c*, the FIRST c with S(c) <= total
// (none: the last rung, flagged).  S is not monotone in c and ladders may repeat or descend, so nothing here bisects.
//
// The walk.  A frame's record is amv_rate_plan.h's (its rung, kRateOver once final).  At a clip rung c every frame starts at
// rho_c(i), its first floor-fit at or after c (none: the last rung, flagged), and rate_check moves it along its floor-fits
// until its real length fits: when a check leaves an empty list every frame sits at r_c(i) and the sum of the lengths is S(c).
//   S(c) <= total: final.  Otherwise the clip moves to the next c' > c whose floor sum F(c') <= total -- none: to the last
//   rung -- and there every frame whose rung is below c' moves to rho_c'(i) and is coded again; a frame at or above c' keeps
//   its chunk (r_c(i) >= c' implies r_c'(i) = r_c(i): the rungs between were tried and did not fit).  The last rung is final
//   whatever its sum, flagged when the sum is over.
//
// The floor sum F(c) = sum_i clip_floor(i, c) is a lower bound of S(c), so a c with F(c) > total is passed without coding.
// Per frame the bound is floor(bits[i][rho_c(i)]) when the frame is sure to stay there.  With a per-frame budget it need not:
// escapes can push len over B(i), the frame moves to a later floor-fit, and that one may be SMALLER than the floor it left.
// A chunk of `bits` is at most rate_most_bytes(bits) long (every scan byte an FF), so the frame is sure to stay where that
// fits B(i); otherwise the bound is the least floor over the floor-fits it may still reach (the last rung among them, where
// a frame with nothing left ends).  With no per-frame cap (B = 0xffffffff) this is floor(bits[i][c]) exactly.
//
// The pass bound.  The host queues the passes without knowing their counts; most find an empty list and leave at once.
//   At a clip rung c every listed frame is coded at a rung >= c that is strictly above the rung it was coded at last, so the
//   k-th pass at c (k = 0: the pass that arrives at c) codes at rungs >= c + k: at most rungs - c passes at c.  A move of
//   the clip with no frame below c' codes nothing: the walk takes the next step at once (the sum is unchanged).  c rises
//   strictly.  So a call codes in at most sum_c (rungs - c) = rungs (rungs + 1) / 2 passes, the first over all frames
//   included -- clip_passes_most.  tests/test_clip_ref.py holds a table that takes every one of them.
//
// Sums are uint64: n < 2^32 frames of less than 2^32 bytes each.  The rate entries' limit of kRateBlocksMost blocks holds.
#pragma once
#include <stdint.h>

#include "amv_rate_plan.h"

namespace amv {

constexpr uint64_t kClipOver = kRateOver;         // or-ed into the clip record's word 0 (AMVHIP_RATE_OVER)

AMV_HD inline uint32_t clip_passes_most(uint32_t rungs) { return rungs * (rungs + 1u) / 2u; }
static_assert(kRateRungsMax * (kRateRungsMax + 1u) / 2u == 136u, "the counters of clip_plan (amv_host_plan.h)");

// the longest chunk `bits` of scan can make: 4 + 2 * ceil(bits / 8) (no wrap: uint64)
AMV_HD inline uint64_t rate_most_bytes(uint32_t bits) { return 4ull + 2ull * ((uint64_t)bits / 8u + ((bits & 7u) ? 1u : 0u)); }

// a frame's part of F(c): see above.  row: the frame's bits at every rung
AMV_HD inline uint32_t clip_floor(const uint32_t* row, uint32_t rungs, uint32_t budget, uint32_t c) {
    uint32_t least = 0xffffffffu;
    for (uint32_t r = rate_first_fit(row, rungs, budget, c); r < rungs; r = rate_first_fit(row, rungs, budget, r + 1u)) {
        const uint32_t f = rate_floor_bytes(row[r]);
        least = f < least ? f : least;
        if (rate_most_bytes(row[r]) <= budget) return least;     // the frame stays here at the latest
    }
    const uint32_t last = rate_floor_bytes(row[rungs - 1u]);      // it may end on the last rung, fitting or not
    return last < least ? last : least;
}

// where a frame stands when the clip arrives at rung c: rate_choose from c on
AMV_HD inline uint32_t clip_record_at(const uint32_t* row, uint32_t rungs, uint32_t budget, uint32_t c) {
    const uint32_t r = rate_first_fit(row, rungs, budget, c);
    return r < rungs ? r : (rungs - 1u) | kRateOver;
}
// the clip has moved to c: true = the frame moves (record is rewritten) and is to be coded again
AMV_HD inline bool clip_move(const uint32_t* row, uint32_t rungs, uint32_t budget, uint32_t c, uint32_t& record) {
    if ((record & ~kRateOver) >= c) return false;                 // (a final record is on the last rung: never below c)
    record = clip_record_at(row, rungs, budget, c);
    return true;
}

// the first c >= from with F[c] <= total; none: the last rung
AMV_HD inline uint32_t clip_first_rung(const uint64_t* F, uint32_t rungs, uint64_t total, uint32_t from) {
    for (uint32_t c = from; c < rungs; ++c)
        if (F[c] <= total) return c;
    return rungs - 1u;
}
// One clip step, every frame settled at c with the lengths summing to S.  true: final, clip[] is written; false: the clip
// moves to c (rewritten, > the old one).
AMV_HD inline bool clip_step(const uint64_t* F, uint32_t rungs, uint64_t total, uint64_t S, uint32_t& c, uint64_t* clip) {
    if (S <= total || c == rungs - 1u) {
        clip[0] = (uint64_t)c | (S <= total ? 0ull : kClipOver);
        clip[1] = S;
        return true;
    }
    c = clip_first_rung(F, rungs, total, c + 1u);
    return false;
}

}  // namespace amv
