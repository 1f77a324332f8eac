// amv_qns_plan.h -- the arithmetic of the video encoder's quantizer noise shaping (`-qns`), free of HIP: what
// amv_qns_refine_kernel (amv_encode_qns.hip) and tests/c/qns_plan_test.cc both run.
//
// Reference path (lavc = libavcodec): dct_quantize_refine, lavc/mpegvideo_enc.c:3271-3645, called from encode_mb_internal
// (:1665-1671) behind whichever quantiser is installed (:1654-1664), with the visual weights of get_vissual_weight
// (:1434-1455, called at :1637-1649) -- per 8x8 block, one +-1 change of a level at a time, each the one that lowers the
// weighted error of the reconstruction in the pixel domain plus lambda * bits the most.  The reference cannot run it for its
// amv encoder: it unquantises by the H.263 rule qmul * level +- qadd (:3302-3303, :3372-3373) and reads intra_ac_vlc_length,
// which is NULL for MJPEG.  Here the walk, the roundings and the weights are the reference's; the reconstruction is the one
// every AMV decoder applies, level * Q (AmvJpeg.c:1040), and the rate is the length of what amv_pack_kernel writes for the
// block's AC part -- ZRLs, run/size codes, magnitude bits and the EOB (trellis_bits / trellis_eob_bits of amv_trellis_plan.h) --
// exact where the reference approximates (:3477-3551), with no |level| < 63 exemption.  So the numbers are neither the
// reference's own nor those of amvlib's picture (that differs by its IDCT's rounding: amv_encode_error.hip).
//
// Per block: p[64] the samples the encoder transforms (0 .. 255, row-major, edge replication included), level[64] in SCAN
// order as the call's quantiser left them (position 0 the DC, absolute), the component class, qns 1 .. 3, lambda2.
//   weights   w0[x + 8 y] = 36 * ff_sqrt(count * sqr - sum^2) / count over the 3x3 neighbourhood clipped to the block
//             (:1434-1455; ff_sqrt: the floor square root of libavutil/internal.h:183-199), then w' = |w0| + 144,
//             w = 15 + (48 * 144 + w' / 2) / w', 16 .. 63 (:3345-3359); lambda = (sum of w^2 * lambda2) >> 19 (:3360).
//   basis     basis[8 i + j][8 x + y] = lrintf(s cos(pi / 8 i (x + 1/2)) cos(pi / 8 j (y + 1/2))), s = 0.25 * 2^16, times
//             sqrt(1/2) for i = 0 and again for j = 0 (:3255-3268, the identity permutation): 64 x 64 int16, made on the host.
//   remainder RECON_SHIFT is 6: rem[k] = DCq * 8 + 32 - ((p[k] - 128) << 6) with DCq = level[0] * Q[0] (:3315-3340: the
//             reference's q = dc_scale << 3 is Q[0] * 8, its un-shifted samples are p - 128 as this encoder's fdct has
//             them), then add_8x8basis(rem, basis[natural(i)], level[i] * Q[i]) per non-zero AC level (:3366-3381);
//             add_8x8basis: rem += (basis * scale + 512) >> 10 (dsputil.c:3128-3134), rem an int16.
//   score     try_8x8basis (dsputil.c:3113-3126): (sum of ((w b)^2 >> 4)) >> 2, b = (rem + ((basis * D + 512) >> 10)) >> 6,
//             an unsigned sum; D is the change of the reconstructed coefficient, +-Q[i] -- for the DC too (the reference
//             hands its DC candidates q * change with q already in the remainder's scale, eight times the change its own
//             remainder makes, :3425-3435; level * Q is kept consistent here).  best_score starts at D = 0 (:3391).
//   rate      lambda * (ac_bits(after) - ac_bits(before)); only the symbol at i, the next non-zero's run and the EOB can
//             differ, so it is had from the previous and the next non-zero position (qns_local_bits).  DC changes carry
//             none (:3419-3443).
//   the walk  (:3390-3636) candidates in order DC -1, DC +1, then scan positions 1 .. 63, each -1 then +1; a strictly smaller
//             score wins.  A DC candidate is skipped unless 0 <= new * Q[0] + 1024 < 2048, an AC one unless
//             |new * Q[i]| < 2048 (:3432, :3480).  qns < 3: stop at i > last_non_zero + 1 (:3456).  qns < 2: skip a candidate
//             whose magnitude grows (:3474).  The gradient rule (:3398-3417, :3496-3500), when last_non_zero > 2 or
//             qns >= 3: d1 = ff_jpeg_fdct_islow of (rem * w^2 + 2^17) >> 18, and a zero level may become +-1 only against
//             the sign of d1 at its position.  The best change is applied, rem and last_non_zero follow, and the walk
//             repeats until nothing wins or kQnsIterations changes were made.
#pragma once
#include <math.h>
#include <stdint.h>

#include "amv_trellis_plan.h"

namespace amv {

constexpr int kQnsReconShift = 6, kQnsBasisShift = 16;
constexpr int kQnsBasisRound = 1 << (kQnsBasisShift - kQnsReconShift - 1), kQnsBasisDown = kQnsBasisShift - kQnsReconShift;
constexpr uint32_t kQnsMost = 3;                 // the largest -qns
// The cap.  Every accepted change strictly lowers the walk's score (weighted error + lambda * bits), which is bounded below,
// so the walk ends by itself; a device loop has a stated bound all the same.  Measured with tests/qns_ref.py: over 20 000
// seeded blocks of reference_samples' four kinds at qns 3, lambda2 0 (`python tests/qns_ref.py`) the most changes one block
// took was 39; over every block of tests/test_gpu_encode_qns.py, at the tests' own settings, 90 (its last test checks it).
// kQnsChangesSeen is the larger; the cap is the next power of two above four times that.  A block that reaches the cap stops
// there, in the model and in the kernel alike.
constexpr uint32_t kQnsChangesSeen = 90;
constexpr uint32_t kQnsIterations = 512;
static_assert(kQnsIterations > 4u * kQnsChangesSeen && kQnsIterations / 2u <= 4u * kQnsChangesSeen, "the next power of two above four times the count");

// ---- the basis -------------------------------------------------------------------------------------------------------------
struct QnsBasis {
    int16_t b[64][64];                           // [natural coefficient 8 i + j][sample 8 x + y]
};
inline void qns_build_basis(QnsBasis& t) {       // host only (:3252-3269)
    for (int i = 0; i < 8; ++i)
        for (int j = 0; j < 8; ++j)
            for (int y = 0; y < 8; ++y)
                for (int x = 0; x < 8; ++x) {
                    double s = 0.25 * (1 << kQnsBasisShift);
                    if (i == 0) s *= sqrt(0.5);
                    if (j == 0) s *= sqrt(0.5);
                    t.b[8 * i + j][8 * x + y] = (int16_t)lrintf((float)(s * cos((M_PI / 8.0) * i * (x + 0.5)) * cos((M_PI / 8.0) * j * (y + 0.5))));
                }
}
// scan position -> natural (row-major) index
struct QnsScan { uint8_t natural[64]; };
constexpr QnsScan make_qns_scan() {
    QnsScan s{};
    for (int n = 0; n < 64; ++n) s.natural[kScanOfNatural[n]] = (uint8_t)n;
    return s;
}

// ---- the weights -----------------------------------------------------------------------------------------------------------
AMV_HD inline int32_t qns_sqrt(int32_t a) {      // ff_sqrt: the floor square root (its table for a < 128 holds the same)
    int32_t ret = 0;
    for (int s = 30; s >= 0; s -= 2) {
        ret += ret;
        const int32_t b = (1 + 2 * ret) << s;
        if (b <= a) {
            a -= b;
            ret++;
        }
    }
    return ret;
}
// count, sum and sum of squares of a sample's clipped neighbourhood -> its weight, 16 .. 63.  (count * sqr - sum^2 does not
// change when every sample moves by the same amount: the planes' samples - 128 give the weights of the samples.)
AMV_HD inline int32_t qns_weight(int32_t count, int32_t sum, int32_t sqr) {
    const int32_t w0 = 36 * qns_sqrt(count * sqr - sum * sum) / count;       // count * sqr <= 81 * 255^2: inside 23 bits
    const int32_t w = (w0 < 0 ? -w0 : w0) + 4 * 36;
    return 15 + (48 * 4 * 36 + w / 2) / w;
}
template <class Get>                             // get(k): sample k of the block, row-major
AMV_HD inline int32_t qns_weight_at(Get&& get, int32_t x, int32_t y) {
    int32_t count = 0, sum = 0, sqr = 0;
    for (int32_t y2 = y > 0 ? y - 1 : 0; y2 < (y + 2 < 8 ? y + 2 : 8); ++y2)
        for (int32_t x2 = x > 0 ? x - 1 : 0; x2 < (x + 2 < 8 ? x + 2 : 8); ++x2) {
            const int32_t v = get(x2 + 8 * y2);
            sum += v;
            sqr += v * v;
            ++count;
        }
    return qns_weight(count, sum, sqr);
}
AMV_HD inline int32_t qns_lambda(uint32_t sum_w2, uint32_t lambda2) { return (int32_t)(((uint64_t)sum_w2 * lambda2) >> 19); }

// ---- the remainder and the score ---------------------------------------------------------------------------------------------
AMV_HD inline int32_t qns_s16(int32_t x) { return (int16_t)(uint16_t)(uint32_t)x; }
AMV_HD inline int32_t qns_rem_start(int32_t dc_level, int32_t q0, int32_t sample_less_128) {
    return qns_s16(dc_level * q0 * 8 + (1 << (kQnsReconShift - 1)) - sample_less_128 * (1 << kQnsReconShift));
}
AMV_HD inline int32_t qns_basis_step(int32_t basis, int32_t scale) { return (basis * scale + kQnsBasisRound) >> kQnsBasisDown; }
AMV_HD inline int32_t qns_rem_add(int32_t rem, int32_t basis, int32_t scale) { return qns_s16(rem + qns_basis_step(basis, scale)); }
// one sample's term of try_8x8basis: ((w b)^2) >> 4 with b = (rem + step) >> 6, as unsigned arithmetic
AMV_HD inline uint32_t qns_term(int32_t rem, int32_t w, int32_t step) {
    const int32_t b = (rem + step) >> kQnsReconShift;
    const uint32_t wb = (uint32_t)(w * b);
    return (wb * wb) >> 4;
}
AMV_HD inline int32_t qns_gradient_in(int32_t rem, int32_t w) { return qns_s16((rem * w * w + (1 << (kQnsReconShift + 12 - 1))) >> (kQnsReconShift + 12)); }

// one 8-point pass of ff_jpeg_fdct_islow (jfdctint.c:184-343) over d[0], d[stride] ..: the row pass (first) or the column
// pass; outputs truncated to DCTELEM as the reference stores them
AMV_HD inline void qns_fdct_pass(int32_t* d, int stride, bool first) {
    const int shift = first ? 13 - 4 : 13 + 4;
    const int32_t half = 1 << (shift - 1);
    const int32_t t0 = d[0] + d[7 * stride], t7 = d[0] - d[7 * stride];
    const int32_t t1 = d[stride] + d[6 * stride], t6 = d[stride] - d[6 * stride];
    const int32_t t2 = d[2 * stride] + d[5 * stride], t5 = d[2 * stride] - d[5 * stride];
    const int32_t t3 = d[3 * stride] + d[4 * stride], t4 = d[3 * stride] - d[4 * stride];
    const int32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    d[0] = qns_s16(first ? (t10 + t11) * 16 : (t10 + t11 + 8) >> 4);
    d[4 * stride] = qns_s16(first ? (t10 - t11) * 16 : (t10 - t11 + 8) >> 4);
    const int32_t e1 = (t12 + t13) * 4433;
    d[2 * stride] = qns_s16((e1 + t13 * 6270 + half) >> shift);
    d[6 * stride] = qns_s16((e1 - t12 * 15137 + half) >> shift);
    const int32_t z5 = (t4 + t6 + t5 + t7) * 9633;
    const int32_t z1 = (t4 + t7) * -7373, z2 = (t5 + t6) * -20995, z3 = (t4 + t6) * -16069 + z5, z4 = (t5 + t7) * -3196 + z5;
    d[7 * stride] = qns_s16((t4 * 2446 + z1 + z3 + half) >> shift);
    d[5 * stride] = qns_s16((t5 * 16819 + z2 + z4 + half) >> shift);
    d[3 * stride] = qns_s16((t6 * 25172 + z2 + z3 + half) >> shift);
    d[stride] = qns_s16((t7 * 12299 + z1 + z4 + half) >> shift);
}

// ---- the rate ----------------------------------------------------------------------------------------------------------------
// What the AC part's length owes to position i holding magnitude a (0: nothing coded there): i's own symbol behind the run
// from the previous non-zero position prev (0: none), and what follows it -- the next non-zero position next (0: none) with
// magnitude a_next behind its run, or the EOB behind the block's last coded position.  ac_bits(after) - ac_bits(before) is
// the difference of two of these.
AMV_HD inline int32_t qns_local_bits(const uint8_t* len, uint32_t i, uint32_t prev, uint32_t next, uint32_t a_next, uint32_t a) {
    const uint32_t from = a ? i : prev;
    uint32_t bits = a ? trellis_bits(len, i - prev - 1u, a) : 0u;
    bits += next ? trellis_bits(len, next - from - 1u, a_next) : trellis_eob_bits(len, from);
    return (int32_t)bits;
}

// ---- a candidate's gates -------------------------------------------------------------------------------------------------------
AMV_HD inline bool qns_dc_allowed(int32_t new_level, int32_t q0) {
    const int32_t v = new_level * q0 + 1024;
    return v >= 0 && v < 2048;
}
// level -> level + change at AC position i: the range (:3480), the -qns 1 rule (:3474), the gradient rule (:3496-3500; g: d1 at
// the position when the rule applies, else 0)
AMV_HD inline bool qns_ac_allowed(int32_t level, int32_t change, int32_t q, uint32_t qns, int32_t g) {
    const int32_t nl = level + change;
    const int32_t an = nl < 0 ? -nl : nl, al = level < 0 ? -level : level;
    if (qns < 2u && an > al) return false;
    if (nl == 0) return true;
    if (an * q >= 2048) return false;
    if (level == 0 && g && (g ^ nl) >= 0) return false;
    return true;
}

// ---- the bounds ----------------------------------------------------------------------------------------------------------------
// rem.  rem / 64 is (reconstruction - sample) + 1/2, up to the add_8x8basis roundings (at most 1/2 of 1/64 per coded
// coefficient).  The basis is orthonormal (0.25 C_i C_j cos cos), so the largest error of one sample is at most the norm of
// the coefficients' errors.  Behind the plain quantiser and the trellis a level is within one step of c / (8 Q)
// (amv_trellis_plan.h: the error of a candidate is below 8 Q + 2 in the fdct's scale, Q + 1/4 in a coefficient's), so the walk
// starts with |reconstruction - sample| <= sqrt(sum of (Q + 1/4)^2) = 273 (luma), 367 (chroma) and |rem| < 367 * 64 + 64 <
// 2^15, and a candidate's b = (rem + step) >> 6, |step| <= 61 * 2^14 / 2^10 + 1 = 977, starts inside the +-512 the reference
// asserts (dsputil.c:3121).  What is NOT proven is that every later remainder stays there (a change may trade a larger error
// in a busy sample for a smaller weighted sum), nor anything behind -nr, whose dead zone is not bounded by a step.  So nothing
// relies on the range: rem is kept as the int16 the reference keeps (qns_s16) and the sums are unsigned, which makes the
// kernel, this header and the model agree on every input; the model asserts the ranges on every block it walks, and
// tests/c/qns_plan_test.cc measures them on blocks made to push them (|rem| <= 16 281, |b| <= 257 there).
// The unsigned sum.  w <= 63, |b| <= 512: (w b)^2 <= 2^30 + ..., a term is below 2^26 and 64 of them below 2^32: the sum
// does not wrap, and try_8x8basis's result, sum >> 2, is below 2^30 = kQnsScoreMost.
// Delta-bits * lambda + score.  |Delta-bits| is at most two symbols and an EOB replaced by one symbol, below 3 * 59 =
// kQnsBitsMost (kTrellisBitsMost: the longest run/size code with its ZRLs and magnitude bits; levels inside +-2047 / 5 keep
// within the 10 bits that takes).  With sum of w^2 <= 64 * 63^2, lambda <= (64 * 63^2 * lambda2) >> 19, and lambda2 is
// taken while kQnsBitsMost * lambda + kQnsScoreMost stays inside int32.
constexpr uint32_t kQnsScoreMost = 1u << 30;
constexpr uint32_t kQnsBitsMost = 3u * kTrellisBitsMost;
constexpr uint32_t kQnsSumW2Most = 64u * 63u * 63u;
constexpr uint32_t kQnsLambdaMost = (0x7fffffffu - kQnsScoreMost) / kQnsBitsMost;
constexpr uint32_t kQnsLambda2Max = (uint32_t)(((((uint64_t)kQnsLambdaMost + 1u) << 19) - 1u) / kQnsSumW2Most);
static_assert((((uint64_t)kQnsSumW2Most * kQnsLambda2Max) >> 19) <= kQnsLambdaMost, "the bound holds at its edge");
static_assert((((uint64_t)kQnsSumW2Most * (kQnsLambda2Max + 1ull)) >> 19) > kQnsLambdaMost, "... and is the largest");
static_assert((uint64_t)kQnsBitsMost * kQnsLambdaMost + kQnsScoreMost <= 0x7fffffffull, "Delta-bits * lambda + score fits int32");
static_assert(64ull * ((63ull * 512ull) * (63ull * 512ull) >> 4) < (1ull << 32), "the unsigned sum does not wrap");
AMV_HD inline uint32_t qns_lambda2_max() { return kQnsLambda2Max; }
// the reference's lambda2 for a qscale: lambda = qscale * FF_QP2LAMBDA, lambda2 = (lambda^2 + 64) >> 7 (:144-147).  0: above
// the bound (or qscale 0)
AMV_HD inline uint32_t qns_lambda2_of_qscale(uint32_t qscale) {
    const uint64_t lambda = (uint64_t)qscale * 118u;
    const uint64_t l = (lambda * lambda + 64u) >> 7;
    return qscale > 65535u || l > kQnsLambda2Max ? 0u : (uint32_t)l;
}

// ---- the whole block -------------------------------------------------------------------------------------------------------------
// p: the samples, 0 .. 255, row-major; level: scan order, refined in place; cap: kQnsIterations (a test hands less to walk the
// cap's path).  -> the changes made.
inline uint32_t qns_block(const int16_t* p, int16_t* level, const QnsBasis& basis, const TrellisTables& tab, uint32_t comp, uint32_t qns,
                          uint32_t lambda2, uint32_t cap = kQnsIterations) {
    constexpr QnsScan scan = make_qns_scan();
    const uint8_t* len = tab.len[comp];
    const uint8_t* q = tab.q[comp];
    int32_t w[64], rem[64], d1[64];
    uint32_t sum_w2 = 0;
    for (int k = 0; k < 64; ++k) {
        w[k] = qns_weight_at([&](int32_t at) { return (int32_t)p[at]; }, k & 7, k >> 3);
        sum_w2 += (uint32_t)(w[k] * w[k]);
    }
    const int32_t lambda = qns_lambda(sum_w2, lambda2);
    for (int k = 0; k < 64; ++k) rem[k] = qns_rem_start(level[0], q[0], p[k] - 128);
    for (int i = 1; i < 64; ++i)
        if (level[i])
            for (int k = 0; k < 64; ++k) rem[k] = qns_rem_add(rem[k], basis.b[scan.natural[i]][k], level[i] * q[i]);
    uint32_t changes = 0;
    while (changes < cap) {
        uint32_t last = 0;
        for (uint32_t i = 1; i < 64u; ++i)
            if (level[i]) last = i;
        uint32_t sum0 = 0;
        for (int k = 0; k < 64; ++k) sum0 += qns_term(rem[k], w[k], 0);
        int32_t best = (int32_t)(sum0 >> 2), best_at = -1, best_change = 0;
        const bool gradient = last > 2u || qns >= 3u;
        if (gradient) {
            for (int k = 0; k < 64; ++k) d1[k] = qns_gradient_in(rem[k], w[k]);
            for (int r = 0; r < 8; ++r) qns_fdct_pass(d1 + 8 * r, 1, true);
            for (int c = 0; c < 8; ++c) qns_fdct_pass(d1 + c, 8, false);
        }
        uint32_t prev = 0;
        for (uint32_t i = 0; i < 64u; ++i) {
            if (i && qns < 3u && i > last + 1u) break;
            uint32_t next = 0;
            for (uint32_t k = i + 1u; i && k < 64u && !next; ++k)
                if (level[k]) next = k;
            const uint32_t a_next = next ? (uint32_t)(level[next] < 0 ? -level[next] : level[next]) : 0u;
            const int16_t* b = basis.b[scan.natural[i]];
            for (int32_t change = -1; change <= 1; change += 2) {
                const int32_t nl = level[i] + change;
                if (i == 0 ? !qns_dc_allowed(nl, q[0]) : !qns_ac_allowed(level[i], change, q[i], qns, gradient ? d1[scan.natural[i]] : 0)) continue;
                uint32_t sum = 0;
                for (int k = 0; k < 64; ++k) sum += qns_term(rem[k], w[k], qns_basis_step(b[k], change * q[i]));
                int32_t score = (int32_t)(sum >> 2);
                if (i) {
                    const uint32_t a_old = (uint32_t)(level[i] < 0 ? -level[i] : level[i]), a_new = (uint32_t)(nl < 0 ? -nl : nl);
                    score += (qns_local_bits(len, i, prev, next, a_next, a_new) - qns_local_bits(len, i, prev, next, a_next, a_old)) * lambda;
                }
                if (score < best) {
                    best = score;
                    best_at = (int32_t)i;
                    best_change = change;
                }
            }
            if (i && level[i]) prev = i;
        }
        if (best_at < 0) break;
        level[best_at] = (int16_t)(level[best_at] + best_change);
        for (int k = 0; k < 64; ++k) rem[k] = qns_rem_add(rem[k], basis.b[scan.natural[best_at]][k], best_change * q[best_at]);
        ++changes;
    }
    return changes;
}

}  // namespace amv
