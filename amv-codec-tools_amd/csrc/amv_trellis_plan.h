// amv_trellis_plan.h -- the arithmetic of the video encoder's trellis quantiser, free of HIP: what the trellis instantiations
// of amv_forward_kernel and amv_encode_frame_kernel (amv_encode_common.h: trellis_lane) and tests/c/trellis_plan_test.cc
// both run.
//
// Reference path (lavc = libavcodec): dct_quantize_trellis_c, lavc/mpegvideo_enc.c:2961-3247, with start_i = 1 -- per 8x8
// block the levels that minimise distortion + lambda * bits.  The reference never ran it for its amv encoder (no
// intra_ac_vlc_length is set for MJPEG); here the rate is AMV's fixed AC code itself, ZRL and EOB included, and the
// reconstruction is the one every AMV decoder applies, level * Q (AmvJpeg.c:1040) -- in the fdct's scale, level * Q * 8.
//
// Per block: c[64] this encoder's fdct outputs (samples - 128) in SCAN order, position 0 already the quantised DC
// (the plain quantiser's rule, (x + q / 2) / q with q = 8 Q[0]: the DC takes no part in the search).  The AC levels come back in place.
//   1. qmat_i = (1 << 22) / (8 Q[i]), L_i = c[i] * qmat_i, bias = qbias << 14, t1 = (1 << 22) - bias - 1;
//      last = the highest i with |L_i| > t1; none: every AC level is 0.
//   2. candidates at i <= last: |L_i| > t1: a = (|L_i| + bias) >> 22, then a - 1 when a >= 2; otherwise the one level 1.
//      The sign is c[i]'s, + for 0 (the reference's (level >> 31) | 1).
//   3. cost of |v| at i behind r zeros: d = (|v| * Q[i] * 8 - |c[i]|)^2 - c[i]^2,
//      bits = (r >> 4) * len[0xF0] + len[(r & 15) << 4 | nbits(|v|)] + nbits(|v|).
//   4. the walk (:3073-3176): score[1] = 0, survivors = [1]; at i the candidates in order, the survivors newest first,
//      s = d + bits * lambda + score[survivor], strictly smaller wins; score[i + 1] = best; survivors leave from the
//      newest end while their score is > best (last <= 27) or > best + lambda (last > 27); i + 1 joins.
//   5. the end (:3178-3191, exact instead of a flat 2 lambda): over i = survivors[0] .. last + 1,
//      s = score[i] + (i - 1 < 63 ? len[0x00] * lambda : 0), strictly smaller wins; backtrack as :3236-3244.
#pragma once
#include <stdint.h>

#include "amv_segment.h"
#include "amv_tables.h"

namespace amv {

constexpr int32_t kTrellisNoScore = 256 * 256 * 256 * 120;   // best_score's start, :3081
constexpr int32_t kTrellisQmatShift = 22;
constexpr uint32_t kTrellisLastNarrow = 27;                  // :3163

// ---- the tables: AC code lengths, steps and multipliers of the two component classes, scan order ------------------------
struct TrellisTables {
    uint8_t len[2][256];      // len[comp][symbol]: AMV's AC code (ff_mjpeg_build_huffman_codes over the fixed specification); 0 = no code
    uint8_t q[2][64];         // Q[i]
    uint32_t qmat[2][64];     // (1 << 22) / (8 Q[i])
};
constexpr TrellisTables make_trellis_tables() {
    TrellisTables t{};
    for (int comp = 0; comp < 2; ++comp) {
        int k = 0;
        for (int l = 1; l <= 16; ++l)
            for (int n = 0; n < kHuffCount[2 + comp][l - 1]; ++n, ++k)
                t.len[comp][comp ? kHuffAcChromaSymbols[k] : kHuffAcLumaSymbols[k]] = (uint8_t)l;
        for (int i = 0; i < 64; ++i) {
            const uint32_t q = comp ? kQuantChroma[i] : kQuantLuma[i];
            t.q[comp][i] = (uint8_t)q;
            t.qmat[comp][i] = (1u << kTrellisQmatShift) / (8u * q);
        }
    }
    return t;
}

// ---- the rate ---------------------------------------------------------------------------------------------------------
AMV_HD inline uint32_t trellis_nbits(uint32_t a) { return a ? 32u - (uint32_t)__builtin_clz(a) : 0u; }
// bits of level magnitude a (1 .. 1023) behind a run of r (0 .. 62) zeros: ZRLs, the run/size code, the magnitude bits
AMV_HD inline uint32_t trellis_bits(const uint8_t* len, uint32_t r, uint32_t a) {
    const uint32_t nb = trellis_nbits(a);
    return (r >> 4) * len[0xF0] + len[((r & 15u) << 4) | nb] + nb;
}
// ... and of the end-of-block code behind a block whose last coded position is p (none after position 63, mjpegenc.c:430-431)
AMV_HD inline uint32_t trellis_eob_bits(const uint8_t* len, uint32_t p) { return p < 63u ? len[0x00] : 0u; }

// ---- the candidates ---------------------------------------------------------------------------------------------------
// c: the fdct output; -> how many candidates (1 or 2) and the first one's magnitude a (the second is a - 1); above: whether
// |L| > t1 (what `last` is made of)
AMV_HD inline int32_t trellis_bias(uint32_t qbias) { return (int32_t)(qbias << 14); }
AMV_HD inline uint32_t trellis_candidates(int32_t c, uint32_t qmat, int32_t bias, uint32_t& a, bool& above) {
    const int32_t L = c * (int32_t)qmat;                       // |c| <= 8193, qmat <= 2^22 / 40: inside 31 bits
    const uint32_t aL = (uint32_t)(L < 0 ? -L : L);
    above = aL > (uint32_t)((1 << kTrellisQmatShift) - bias - 1);
    a = above ? (aL + (uint32_t)bias) >> kTrellisQmatShift : 1u;
    return a >= 2u ? 2u : 1u;
}
AMV_HD inline int32_t trellis_distortion(int32_t c, uint32_t a, uint32_t q) {
    const int32_t ac = c < 0 ? -c : c;
    const int32_t e = (int32_t)(a * q * 8u) - ac;
    return e * e - ac * ac;
}

// ---- the bound on lambda ----------------------------------------------------------------------------------------------
// Scores are int.  What a score can lose: every coded position gives d >= -c^2, and the sum of c^2 over a block of 8-bit
// samples is about 2^26 (Parseval: 64 samples inside +-128, the fdct's gain of 8), nowhere near INT32_MIN.  What it can
// gain, per position:
//   d, first candidate above the threshold: with x = |c| / (8 Q) and b = bias / 2^22 < 1, |L| / 2^22 lies in (x - e, x], e <
//     8193 / 2^22 (the floor in qmat), so a lies in (x + b - 1 - e, x + b] and a * 8 Q - |c| in (-8 Q (1 + e), 8 Q): |.| < 8 Q + 2;
//   d, second candidate (a >= 2): 0 < (a - 1) * 8 Q < |c|, so the error is smaller than |c| and d < 0;
//   d, the level 1 below the threshold: |c| * qmat < 2^22 gives |c| < 8 Q + 1: the error 8 Q - |c| lies in (-1, 8 Q];
//   so d <= (8 Qmax + 2)^2 = kTrellisStepMost, Qmax = 61;
//   bits <= 3 * len[0xF0] + 16 + 10 = 59 (a run of up to 62, the longest code, a magnitude inside 10 bits: levels are at
//     most 8193 / 40 + 1).
// score[i + 1] <= score[i] + (that), since the newest survivor is always i itself (run 0, first candidate), and any sum the
// walk forms is a score plus one such step, the end rule's a score plus len[0x00] * lambda <= 59 lambda: with 63 positions
// nothing the walk forms is above 63 * (kTrellisStepMost + 59 lambda).  lambda is taken while that is below
// kTrellisNoScore (< 2^31): no sum wraps, and none reaches the value `best` starts from.
// Behind -nr (the NrTrellisArg instantiations) the walk is handed denoised outputs: nr_denoise (amv_nr_plan.h) keeps the sign
// and only shrinks the magnitude, |c'| <= |c| <= 8193.  Every step above uses |c| <= 8193 and nothing else of c, so the
// 16-bit fit of the line and this bound stand as they are (tests/c/nr_trellis_plan_test.cc walks denoised blocks in 64 bits).
constexpr uint32_t kTrellisQMost = 61;
constexpr uint32_t kTrellisStepMost = (8u * kTrellisQMost + 2u) * (8u * kTrellisQMost + 2u);
constexpr uint32_t kTrellisBitsMost = 59;
constexpr uint32_t kTrellisLambdaMax = (((uint32_t)kTrellisNoScore - 1u) / 63u - kTrellisStepMost) / kTrellisBitsMost;
static_assert(63ull * (kTrellisStepMost + (uint64_t)kTrellisBitsMost * kTrellisLambdaMax) < (uint64_t)kTrellisNoScore, "the bound holds at its edge");
static_assert(63ull * (kTrellisStepMost + (uint64_t)kTrellisBitsMost * (kTrellisLambdaMax + 1u)) >= (uint64_t)kTrellisNoScore, "... and is the largest");
AMV_HD inline uint32_t trellis_lambda_max() { return kTrellisLambdaMax; }
// the reference's lambda for a qscale: lambda = qscale * FF_QP2LAMBDA, lambda2 = (lambda^2 + 64) >> 7 (:144-147), and the
// trellis takes lambda2 >> (FF_LAMBDA_SHIFT - 6) (:2985).  0: above the bound (or qscale 0)
AMV_HD inline uint32_t trellis_lambda_of_qscale(uint32_t qscale) {
    const uint64_t lambda = (uint64_t)qscale * 118u;
    const uint64_t l = ((lambda * lambda + 64u) >> 7) >> 1;
    return qscale > 65535u || l > kTrellisLambdaMax ? 0u : (uint32_t)l;
}

// ---- a lane's workspace -----------------------------------------------------------------------------------------------
// The survivor list, oldest first, up to 63 entries at a time: an entry's position and, beside it, its score -- the only scores
// read again.  (The text's end rule looks at every position from survivors[0] on; one that has left the list cannot win it:
// it left because a later position's score was strictly lower -- by the slack at least, which is not negative -- and that
// position, or one lower still that replaced it, is in the list with an end term that is no larger.  So the list's scores
// are all the walk needs, and the inner loop's two loads, position and score, do not depend on one another.)
// Per position i + 1, how the best path arrives at i: the run (6 bits) and which candidate (bit 6); the level itself is
// made again from c[i] when the path is walked back.  388 bytes.
struct TrellisLane {
    int32_t score[64];
    uint8_t position[64];
    uint8_t back[65];
};
constexpr uint32_t kTrellisLaneBytes = 392;
static_assert(sizeof(TrellisLane) <= kTrellisLaneBytes, "a lane's workspace");

#if defined(__clang__)
#define AMV_TRELLIS_UNROLL _Pragma("unroll 4")
#else
#define AMV_TRELLIS_UNROLL
#endif

// ---- the whole block ----------------------------------------------------------------------------------------------------
// line: get(k) / set(k, v) over the block's 64 values in scan order (the kernels': the lane's swizzled LDS line).  Returns the
// mask of the non-zero AC levels (bit k: position k).
// The text tries the first candidate against every survivor, then the second; here one pass over the survivors serves both
// (each keeps its own best, strictly smaller wins, newest first) and the second candidate takes over only where its best is
// strictly smaller than the first's: the same winner, with one load of a survivor instead of two.
template <class Line>
AMV_HD inline uint64_t trellis_block(Line& line, const TrellisTables& tab, uint32_t comp, uint32_t qbias, uint32_t lambda, TrellisLane& ws) {
    const uint8_t* len = tab.len[comp];
    const uint8_t* q = tab.q[comp];
    const uint32_t* qmat = tab.qmat[comp];
    const int32_t bias = trellis_bias(qbias);
    const uint32_t zrl = len[0xF0];
    uint32_t last = 0;
    for (uint32_t i = 1; i < 64u; ++i) {
        uint32_t a;
        bool above;
        trellis_candidates(line.get(i), qmat[i], bias, a, above);
        if (above) last = i;
    }
    uint32_t end = 1;                                           // the walk's last_i: position end - 1 is the last one coded
    if (last) {
        ws.score[0] = 0;
        ws.position[0] = 1;
        uint32_t count = 1;
        const int32_t slack = last > kTrellisLastNarrow ? (int32_t)lambda : 0;
        for (uint32_t i = 1; i <= last; ++i) {
            const int32_t c = line.get(i);
            uint32_t a;
            bool above;
            const bool two = trellis_candidates(c, qmat[i], bias, a, above) == 2u;
            const uint32_t nb0 = trellis_nbits(a), nb1 = trellis_nbits(a - 1u);
            // distortion + the magnitude bits' share, per candidate (the second one's only where there is one)
            const int32_t d0 = trellis_distortion(c, a, q[i]) + (int32_t)(nb0 * lambda);
            const int32_t d1 = two ? trellis_distortion(c, a - 1u, q[i]) + (int32_t)(nb1 * lambda) : 0;
            int32_t best0 = kTrellisNoScore, best1 = kTrellisNoScore;
            uint32_t run0 = 0, run1 = 0;
            AMV_TRELLIS_UNROLL
            for (uint32_t j = count; j-- > 0u;) {
                const uint32_t run = i - ws.position[j];
                const int32_t from = ws.score[j];
                const uint32_t sym = (run & 15u) << 4, zrls = (run >> 4) * zrl;
                const int32_t s0 = d0 + (int32_t)((zrls + len[sym | nb0]) * lambda) + from;
                if (s0 < best0) {
                    best0 = s0;
                    run0 = run;
                }
                if (two) {
                    const int32_t s1 = d1 + (int32_t)((zrls + len[sym | nb1]) * lambda) + from;
                    if (s1 < best1) {
                        best1 = s1;
                        run1 = run;
                    }
                }
            }
            const bool second = best1 < best0;
            const int32_t best = second ? best1 : best0;
            ws.back[i + 1] = (uint8_t)(second ? run1 | 64u : run0);
            while (count && ws.score[count - 1u] > best + slack) --count;
            ws.score[count] = best;
            ws.position[count++] = (uint8_t)(i + 1u);
        }
        int32_t best = kTrellisNoScore;
        for (uint32_t j = 0; j < count; ++j) {
            const uint32_t i = ws.position[j];
            const int32_t s = ws.score[j] + (int32_t)(trellis_eob_bits(len, i - 1u) * lambda);
            if (s < best) {
                best = s;
                end = i;
            }
        }
    }
    // back along the path, from the top: a position the path codes gets its level, every other one 0
    uint64_t mask = 0;
    uint32_t coded = end - 1u;                                  // the next position down that the path codes (0: none left)
    for (uint32_t p = 63; p >= 1u; --p) {
        int32_t v = 0;
        if (p == coded) {
            const int32_t c = line.get(p);
            uint32_t a;
            bool above;
            trellis_candidates(c, qmat[p], bias, a, above);
            const uint32_t how = ws.back[p + 1u];
            a -= how >> 6;
            v = c < 0 ? -(int32_t)a : (int32_t)a;
            coded = p - (how & 63u) - 1u;
            mask |= 1ull << p;
        }
        line.set(p, v);
    }
    return mask;
}

// a block in plain memory (the CPU's form of the kernels' LDS line)
struct TrellisPlainLine {
    int16_t* v;
    AMV_HD int32_t get(uint32_t k) const { return v[k]; }
    AMV_HD void set(uint32_t k, int32_t x) { v[k] = (int16_t)x; }
};

}  // namespace amv
