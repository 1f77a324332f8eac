// amv_retable_plan.h -- the arithmetic of re-tabling: chunks whose levels were written against quantiser tables that are not
// AMV's, re-expressed in AMV's tables in the coefficient domain.  Free of HIP: what the kernels of amv_retable.hip and
// tests/c/retable_plan_test.cc both run.
//
// Every AMV decoder dequantises with AMV's fixed tables Qd (TrellisTables::q).  A chunk written against other tables Qs -- the
// reference's own amv encoder writes clip8(ff_mpeg1_default_intra_matrix * qscale >> 3), mpegvideo_enc.c:2866-2877 -- MEANS
// level * Qs and is READ as level * Qd.  The rule, per block of a chunk whose entropy decode is clean (lines in scan order,
// the DC absolute; Qs 64 bytes per component class in scan order, every entry 1 .. 255):
//   1. DC:  v = level * Qs[0]; the new level is v / Qd[0] rounded to nearest, halves away from zero:
//           sign(v) * ((2 |v| + Qd[0]) / (2 Qd[0])).  With Qs[0] == Qd[0] that is the level itself.
//   2. AC:  c[k] = level[k] * 8 Qs[k] (the fdct's scale) is searched by trellis_block as it is, with the rounding term one
//           half (qbias 128) and the caller's lambda, against Qd;
//   3. the lines are coded by the entropy coder of every encoder entry (amv_pack_kernel).
//
// ---- the range rule -----------------------------------------------------------------------------------------------------------
// (a) per AC coefficient  |c| = |level| * 8 Qs <= kRetableCoefMost = 8193.
//     amv_trellis_plan.h proves its fits -- the int16 line, L = c * qmat inside 31 bits, levels inside 10 bits, a step's gain
//     below kTrellisStepMost, hence the bound on lambda -- from |c| <= 8193 "and nothing else of c" (its words for the -nr
//     route): they hold for ANY integer c inside that cap, which is what c is here.  amv_requant_plan.h's wider cap of 8681
//     rests on c being a multiple of 8 Qd (the first candidate is then the level itself and errors are 0 or 8 Qd); that
//     argument does not transfer to foreign tables, so the cap here is the plan's own.  What differs from requant's domain:
//     a chunk in AMV's own tables with a level whose level * 8 Q lies in 8194 .. 8681 -- a rounding share above an fdct
//     output at the very edge of what 8-bit samples reach -- is coded by requant and is out of range here.
//     The reference's encoder truncates (bias 0): its |level| * 8 Qs never exceeds the fdct output it came from, <= 8193.
// (b) per block  the sum of c[k]^2 over its AC positions <= kRetableEnergyMost = 2^30.
//     amv_requant_plan.h (b) word for word: a score, and any sum the walk forms from one, is at least minus the block's
//     energy; it uses d >= -c^2 and nothing else of c.  2^30 + 8193^2 < 2^31.
// (c) the NEW DC: |level| <= kRetableDcMost = 1023, for the reason of amv_requant_plan.h (c): the coder codes differences, and
//     AMV's DC code has sizes 0 .. 11.  The old DC is an int16 line entry and Qs[0] <= 255: |v| < 2^23, 2 |v| + Qd inside int32.
// A frame with a block outside (a), (b) or (c) is not coded (AMVHIP_ST_RANGE), as in requant.
//
// ---- the half-step bound at lambda = 0 ------------------------------------------------------------------------------------------
// Claim: at lambda = 0 every AC position comes back with |new * 8 Qd - c| <= 4 Qd + 1.
// With lambda = 0 bits cost nothing, a path's score is the sum of its positions' d, and positions are independent but for
// `last`; the walk takes, per position, the cheapest of what it is offered (skipping a position costs d = 0).
//   qmat = floor(2^22 / 8 Qd), so with x = |c| / 8 Qd:  x - e < |L| / 2^22 <= x,  e = |c| / 2^22 <= 8193 / 2^22  (qmat's floor
//   costs |c| qmat' with qmat' < 1 per 2^22: less than |c| / 2^22 of a level), and 8 Qd e <= 8193 * 488 / 2^22 < 1.
//   Above the threshold (|L| > 2^21 - 1): a = floor(|L| / 2^22 + 1/2) lies in (x - e - 1/2, x + 1/2], so
//     a * 8 Qd - |c| lies in (-4 Qd - 8 Qd e, 4 Qd]: |.| < 4 Qd + 1.  The second candidate a - 1 and the skip are offered too;
//     the walk takes the least d = err^2 - c^2, i.e. the least |err|, so the result is no worse than a.
//   Not above (|L| <= 2^21 - 1, so x < 1/2 + e): the candidates are the level 1 and the skip.  The skip leaves |c| =
//     8 Qd x < 4 Qd + 8 Qd e < 4 Qd + 1.  Level 1 is taken only where |8 Qd - |c|| < |c|, a smaller error still.
//   Above `last` everything is skipped, and every position there is not above the threshold: the second case.
// Integers: |err| <= 4 Qd + 1 stands as stated (static_assert below for e's share).
//
// ---- the error --------------------------------------------------------------------------------------------------------------
// d_err of a plane: the sum over ALL 64 positions of its blocks of (new * Qd - old * Qs)^2, the DC included; by Parseval the
// unclipped pixel error between what the chunk meant and what the new chunk decodes to.
//   DC: |new * Qd[0] - v| <= Qd[0] / 2 <= 4 (Qd[0] is 8 or 9): at most 16.
//   AC: new * Qd - old * Qs = (new * 8 Qd - c) / 8 exactly.  A coded candidate's error is inside 8 Qd + 2 (the trellis plan's
//   step bound) or smaller than |c| (the second candidate); a skipped position's is |c|.  So the square is at most
//   c^2 / 64 + (Qd + 1)^2, and a block's sum at most energy / 64 + 63 * 62^2 + 16 = kRetableBlockErrorMost < 2^24 + 2^18:
//   the (at most 40) luma blocks of a wave's segment sum inside 32 bits, frames in 64.
#pragma once
#include <stdint.h>

#include "amv_requant_plan.h"
#include "amv_trellis_plan.h"

namespace amv {

constexpr uint32_t kRetableQbias = 128;                       // the rounding term one half: 128 << 14 = 2^21
constexpr int32_t kRetableCoefMost = 8193;                    // what amv_trellis_plan.h proves its fits for
constexpr uint64_t kRetableEnergyMost = 1ull << 30;
constexpr int32_t kRetableDcMost = 1023;
constexpr uint32_t kRetableTablesMax = 64;                    // AMVHIP_RETABLE_TABLES_MAX
constexpr uint32_t kRetableTableBytes = 128;                  // luma then chroma, 64 steps each, scan order
constexpr uint32_t kStTable = 16u;                            // AMVHIP_ST_TABLE
constexpr uint32_t kRetableFlagRange = 1u, kRetableFlagTable = 2u;   // a frame's flag word

static_assert(kRetableCoefMost < 32768, "the line is int16");
static_assert((uint64_t)kRetableCoefMost * ((1u << kTrellisQmatShift) / 40u) < (1ull << 31), "L inside 31 bits (8 Qd >= 40)");
static_assert(kRetableCoefMost / 40 + 1 < 1024, "levels inside 10 bits: kTrellisBitsMost stands");
static_assert((uint64_t)kRetableCoefMost * 8u * kTrellisQMost < (1ull << kTrellisQmatShift), "8 Qd e < 1: the half-step bound's + 1");
static_assert((uint64_t)kRetableCoefMost * 8u * kTrellisQMost / (1u << kTrellisQmatShift) + 8u * kTrellisQMost + 1u <= 8u * kTrellisQMost + 2u,
              "a step's gain stays inside kTrellisStepMost");
static_assert(kRetableEnergyMost + (uint64_t)kRetableCoefMost * kRetableCoefMost <= (1ull << 31), "no sum wraps at the low end");
static_assert(63ull * (kTrellisStepMost + (uint64_t)kTrellisBitsMost * kTrellisLambdaMax) < (uint64_t)kTrellisNoScore, "... nor at the high end");
static_assert(32768ll * 255 * 2 + 9 < (1ll << 31), "the DC's rounding inside int32");
constexpr uint32_t kRetableBlockErrorMost =
    (uint32_t)(kRetableEnergyMost / 64u) + 63u * (kTrellisQMost + 1u) * (kTrellisQMost + 1u) + 16u;
static_assert(40ull * kRetableBlockErrorMost < (1ull << 32), "a wave's luma error inside 32 bits");

// v / q to nearest, halves away from zero (q >= 1, |v| < 2^30)
AMV_HD inline int32_t retable_round_div(int32_t v, int32_t q) {
    const int32_t a = v < 0 ? -v : v;
    const int32_t r = (2 * a + q) / (2 * q);
    return v < 0 ? -r : r;
}
// the DC level against Qd[0] that stands for level * Qs[0]
AMV_HD inline int32_t retable_dc(int32_t level, uint32_t qs, uint32_t qd) { return retable_round_div(level * (int32_t)qs, (int32_t)qd); }

// One block of a chunk, lines in scan order.  levels: get(k); qs: the table the chunk was written against, qd: AMV's; out:
// set(k, c) receives what trellis_block is handed -- the NEW DC level at 0, level * 8 Qs at 1 .. 63.  false: out of range (what
// `out` holds then is not to be searched).
template <class In, class Out>
AMV_HD inline bool retable_scale_block(const In& levels, const uint8_t* qs, const uint8_t* qd, Out& out) {
    const int32_t dc = retable_dc(levels.get(0), qs[0], qd[0]);
    bool ok = dc >= -kRetableDcMost && dc <= kRetableDcMost;
    out.set(0, ok ? dc : 0);
    uint64_t energy = 0;
    for (uint32_t k = 1; k < 64u; ++k) {
        const int32_t c = levels.get(k) * 8 * (int32_t)qs[k];   // |level| <= 32768, 8 Qs <= 2040: inside 27 bits
        ok = ok && c >= -kRetableCoefMost && c <= kRetableCoefMost;
        energy += (uint64_t)((int64_t)c * c);
        out.set(k, ok ? c : 0);
    }
    return ok && energy <= kRetableEnergyMost;
}

// (new * Qd - old * Qs)^2 over all 64 positions of one block; inside 32 bits for a block in range (above)
template <class Old, class New>
AMV_HD inline uint32_t retable_block_error(const Old& before, const New& after, const uint8_t* qs, const uint8_t* qd) {
    uint32_t sum = 0;
    for (uint32_t k = 0; k < 64u; ++k) {
        const int32_t d = after.get(k) * (int32_t)qd[k] - before.get(k) * (int32_t)qs[k];
        sum += (uint32_t)(d * d);
    }
    return sum;
}

// the whole rule for one block in plain memory (the CPU's form): levels in, levels out, the block's error; false: out of range,
// nothing written
AMV_HD inline bool retable_block(const int16_t* in, const uint8_t* qs, const TrellisTables& tab, uint32_t comp, uint32_t lambda, int16_t* out,
                                 uint32_t* err) {
    int16_t c[64];
    TrellisPlainLine from{const_cast<int16_t*>(in)}, line{c};
    if (!retable_scale_block(from, qs, tab.q[comp], line)) return false;
    TrellisLane ws;
    trellis_block(line, tab, comp, kRetableQbias, lambda, ws);
    *err = retable_block_error(from, line, qs, tab.q[comp]);
    for (uint32_t k = 0; k < 64u; ++k) out[k] = c[k];
    return true;
}

// The reference's amv encoder's tables at a qscale (mpegvideo_enc.c:2866-2877: clip8(ff_mpeg1_default_intra_matrix[i] * qscale
// >> 3), entry 0 = 8, one matrix for luma and chroma), in scan order.  The matrix is ISO/IEC 11172-2, 2.4.3.2, row-major.
// false (nothing written): qscale outside 1 .. 31.
constexpr uint8_t kMpeg1Intra[64] = {8,  16, 19, 22, 26, 27, 29, 34, 16, 16, 22, 24, 27, 29, 34, 37, 19, 22, 26, 27, 29, 34, 34, 38,
                                     22, 22, 26, 27, 29, 34, 37, 40, 22, 26, 27, 29, 32, 35, 40, 48, 26, 27, 29, 32, 35, 40, 48, 58,
                                     26, 27, 29, 34, 38, 46, 56, 69, 27, 29, 35, 38, 46, 56, 69, 83};
inline bool retable_ffmpeg_amv_tables(uint32_t qscale, uint8_t tables[2][64]) {
    if (qscale < 1u || qscale > 31u) return false;
    for (uint32_t i = 0; i < 64u; ++i) {                        // i: the natural position
        uint32_t v = ((uint32_t)kMpeg1Intra[i] * qscale) >> 3;
        v = v > 255u ? 255u : v;                                // (83 * 31 >> 3 = 321: the clip is reached; the least is 16 * 1 >> 3 = 2)
        tables[0][kScanOfNatural[i]] = tables[1][kScanOfNatural[i]] = (uint8_t)(i ? v : 8u);
    }
    return true;
}

}  // namespace amv
