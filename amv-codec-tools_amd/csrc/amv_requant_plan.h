// amv_requant_plan.h -- the arithmetic of requantising AMV chunks in the coefficient domain, free of HIP: what the kernels of
// amv_requant.hip and tests/c/requant_plan_test.cc both run.
//
// AMV's quantiser tables are fixed, so the levels of a chunk are already the coefficients the trellis quantiser
// (amv_trellis_plan.h) searches on: level * Q, in the fdct's scale level * 8 Q.  The rule, per block of a chunk whose entropy
// decode is clean (lines in scan order, the DC absolute):
//   1. the DC level is carried unchanged;
//   2. the AC levels are searched by trellis_block, handed c[i] = level[i] * 8 Q[i], the caller's lambda and the rounding term
//      one half (qbias 128: bias = 128 << 14 = 2^21).  The levels are rounded already: no caller's qbias exists here;
//   3. the lines are coded by the entropy coder of every encoder entry (amv_pack_kernel).
//
// ---- the first candidate is the chunk's own level ---------------------------------------------------------------------------
// For a coded position, a = |level| >= 1 and |c| = a * 8 Q.  qmat = floor(2^22 / 8 Q) = (2^22 - r) / 8 Q with 0 <= r < 8 Q, so
// |L| = |c| * qmat = a * 2^22 - a r, and 0 <= a r < a * 8 Q = |c| <= kRequantCoefMost < 2^21.  Hence
//   |L| > 2^22 - 2^21 - 1 = t1                  the position is above the threshold: `last` is the chunk's last non-zero position;
//   a * 2^22 <= |L| + 2^21 < (a + 1) * 2^22     the first candidate (|L| + bias) >> 22 is a itself, the second a - 1.
// With qbias 0 the first candidate of an exact multiple would be a - 1 whenever r > 0: qmat is a floor.
// A position with level 0 has c = 0: below the threshold, the one candidate 1.
// lambda = 0: bits cost nothing, and every coded position's first candidate has the distortion -c^2, the lowest there is at
// its position (the second candidate's is 64 Q^2 - c^2, a level 1 over a zero costs +64 Q^2, a skipped position 0): the
// cheapest path codes exactly the chunk's levels.  Ties do not arise: every other choice is strictly dearer.
//
// ---- the range rule -----------------------------------------------------------------------------------------------------------
// (a) per AC coefficient  |level| * 8 Q <= kRequantCoefMost = 8193 + 8 * 61 = 8681.
//     amv_trellis_plan.h proves its fits for fdct outputs, |c| <= 8193.  A picture's own level stands for level * 8 Q, which
//     exceeds the fdct output it was rounded from by less than 8 Q (the rounding share: (|x| qmat + bias) >> 22 with bias <
//     2^22 gives a * 8 Q < |x| + 8 Q (1 + e); the level 1 of the search sits below 8 Q + 1), and Q <= 61.  So every chunk an
//     encoder of 8-bit samples writes with these tables is inside.  The plan's fits at kRequantCoefMost:
//       the line is int16:          8681 < 32768;
//       L = c * qmat inside 31 bits: |c| * qmat <= |level| * 2^22 and |level| <= 8681 / 40 = 217 (8 Q >= 40): below 2^30;
//       the magnitude bits:          |level| <= 217 is inside 8 bits, so kTrellisBitsMost = 59 (which allows 10) stands;
//       a step's gain:               the error of a candidate is 0 or -8 Q at a coded position and +8 Q over a zero: d <=
//                                    64 Q^2 < kTrellisStepMost, so the bound on lambda stands as it is;
//       ac * ac and e * e:           at most 8681^2 = 75 359 761.
// (b) per block  sum of c[i]^2 over its AC positions <= kRequantEnergyMost = 2^30.
//     What a score can lose: a coded position gives d >= -c^2, everything else the walk adds is not negative, so a score, and
//     any sum the walk forms from one (d + bits * lambda first, which lies in [-c_i^2, kTrellisStepMost + 59 lambda], then the
//     survivor's score over the positions before i), is at least minus the block's energy: >= -2^30, half of what an int32
//     holds; the upper side is amv_trellis_plan.h's, which does not look at c.  Any cap up to 2^31 would do; 2^30 keeps a
//     factor of two and still is far from what pictures reach: a block of 8-bit samples has fdct energy <= 2^26 (Parseval), its
//     levels' c lie within 8 Q of the outputs, so its energy is below (2^13 + sqrt(63) * 488)^2 < 2^28.
//     63 coefficients at kRequantCoefMost would be 4.7e9: the sum is taken in 64 bits.
// (c) the DC: |level| <= kRequantDcMost = 1023.  It is carried, not searched, but the entropy coder codes the difference to
//     the component's predecessor, and AMV's DC code has sizes 0 .. 11 only: two DCs inside +-1023 differ by at most 2046,
//     which is 11 bits.  A clean decode can exceed it only by adding up differences over many blocks (8-bit samples stay
//     inside +-128); such a chunk's int16 lines could even wrap, and the coder would have no code for what it finds.
// A frame with a block outside (a), (b) or (c) is not coded (AMVHIP_ST_RANGE).
//
// ---- the error --------------------------------------------------------------------------------------------------------------
// d_err of a plane: the sum of ((new - old) * Q)^2 over the AC positions of its blocks; by Parseval the unclipped pixel error
// between the two decodes.  At a coded position new is 0, old or old -+ 1 towards zero; a zero inside `last` may become +1
// (it can shorten a run).  So a block's sum is at most its energy / 64 + 63 * 61^2 <= 2^24 + 234 423: the (at most 40) luma
// blocks of a wave's segment sum inside 32 bits, frames in 64.
#pragma once
#include <stdint.h>

#include "amv_trellis_plan.h"

namespace amv {

constexpr uint32_t kRequantQbias = 128;                       // the rounding term one half: 128 << 14 = 2^21
constexpr int32_t kRequantCoefMost = 8193 + 8 * (int32_t)kTrellisQMost;
constexpr uint64_t kRequantEnergyMost = 1ull << 30;
constexpr int32_t kRequantDcMost = 1023;
constexpr uint32_t kStRange = 8u;                             // AMVHIP_ST_RANGE

static_assert(kRequantCoefMost == 8681 && kRequantCoefMost < 32768, "the line is int16");
static_assert((uint64_t)(kRequantCoefMost / 40) << kTrellisQmatShift < (1ull << 31), "L inside 31 bits");
static_assert(kRequantCoefMost / 40 < 256, "levels inside 8 bits");
static_assert((uint64_t)kRequantCoefMost * kRequantCoefMost < (1ull << 31), "c * c");
static_assert(kRequantCoefMost < (1 << 21), "a r < |c| < the rounding term: the first candidate is the level");
static_assert(64u * kTrellisQMost * kTrellisQMost < kTrellisStepMost, "a step's gain");
static_assert(kRequantEnergyMost + (uint64_t)kRequantCoefMost * kRequantCoefMost <= (1ull << 31), "no sum wraps at the low end");
static_assert(63ull * (kTrellisStepMost + (uint64_t)kTrellisBitsMost * kTrellisLambdaMax) < (uint64_t)kTrellisNoScore, "... nor at the high end");
constexpr uint32_t kRequantBlockErrorMost = (uint32_t)(kRequantEnergyMost / 64u) + 63u * kTrellisQMost * kTrellisQMost;
static_assert(40ull * kRequantBlockErrorMost < (1ull << 32), "a wave's luma error inside 32 bits");

// One block of a chunk, lines in scan order.  levels: get(k); out: set(k, c) receives what trellis_block is handed -- the DC
// level at 0, level * 8 Q at 1 .. 63.  false: out of range (what `out` holds then is not to be searched).
template <class In, class Out>
AMV_HD inline bool requant_scale_block(const In& levels, const uint8_t* q, Out& out) {
    const int32_t dc = levels.get(0);
    bool ok = dc >= -kRequantDcMost && dc <= kRequantDcMost;
    out.set(0, dc);
    uint64_t energy = 0;
    for (uint32_t k = 1; k < 64u; ++k) {
        const int32_t c = levels.get(k) * 8 * (int32_t)q[k];   // |level| <= 32768, 8 Q <= 488: inside 25 bits
        ok = ok && c >= -kRequantCoefMost && c <= kRequantCoefMost;
        energy += (uint64_t)((int64_t)c * c);
        out.set(k, ok ? c : 0);
    }
    return ok && energy <= kRequantEnergyMost;
}

// ((new - old) * Q)^2 over the AC positions of one block; inside 32 bits for a block in range (above)
template <class Old, class New>
AMV_HD inline uint32_t requant_block_error(const Old& before, const New& after, const uint8_t* q) {
    uint32_t sum = 0;
    for (uint32_t k = 1; k < 64u; ++k) {
        const int32_t d = (after.get(k) - before.get(k)) * (int32_t)q[k];
        sum += (uint32_t)(d * d);
    }
    return sum;
}

// the whole rule for one block in plain memory (the CPU's form): levels in, levels out, the block's error; false: out of range,
// nothing written
AMV_HD inline bool requant_block(const int16_t* in, const TrellisTables& tab, uint32_t comp, uint32_t lambda, int16_t* out, uint32_t* err) {
    int16_t c[64];
    TrellisPlainLine from{const_cast<int16_t*>(in)}, line{c};
    if (!requant_scale_block(from, tab.q[comp], line)) return false;
    TrellisLane ws;
    trellis_block(line, tab, comp, kRequantQbias, lambda, ws);
    *err = requant_block_error(from, line, tab.q[comp]);
    for (uint32_t k = 0; k < 64u; ++k) out[k] = c[k];
    return true;
}

}  // namespace amv
