// amv_reconstruct.hip -- everything after the entropy stage: dequantise, inverse DCT, YCbCr->BGR,
// bottom-up store (IQtIZzBlock / Fast_IDCT / GetYUV / StoreBuffer, AmvJpeg.c:1010-1059, 754-840).
//
// One wave per MCU-row segment (<= 10 MCUs = 60 blocks = 160 pixels of 16 rows); which segment, the walk over a round's
// items and the launches are the frame amv_block_load.h gives all three back halves:
//   A. lane b loads block b's 64 coefficients into registers: from its dense 128-byte line, or --
//      records form -- after the wave has scattered the segment's (block, index, value) records and
//      DC values into a zeroed LDS image of the 60 blocks (16-byte granules XOR-swizzled by block so
//      that the per-lane 128-byte reads do not collide on banks);
//   B. the whole 8x8 block stays in that lane's registers: de-zig-zag is register renaming (plus
//      one select for amvlib's [3][4] table entry), dequantisation one multiply per coefficient,
//      then 8 row transforms and 8 column transforms with the reference's exact integer
//      arithmetic -- no transposition, no LDS between the passes.  The row pass has two forms: a records frame in
//      which the entropy stage met no AC of ten magnitude bits takes it as dot products over pairs of 16-bit
//      halves (idct8_row_pairs), every other frame and every dense line the general 32-bit form;
//   C. results go to 16-row Y and 8-row U/V planes in LDS (one 16-byte store per block row; the
//      planes reuse the space of the records' image, which every lane has read by then);
//   D. colour conversion of a 4x2-pixel patch per lane step, two bytes per instruction in packed
//      16-bit arithmetic, paired in the order they leave; the 12 bytes of each patch row go
//      straight to the frame (the lanes of a step cover consecutive 12-byte pieces of a row, so a
//      wave store is one contiguous run; the picture is stored bottom-up, AmvJpeg.c:800).  A segment that is whole
//      (ten decoded MCUs, 16 rows inside the picture) takes five unrolled steps without a test per lane; the picture's
//      edges and damaged frames take the general loop.
//
// Pixels of MCUs at or after a frame's first decode error are zero (AMVDec.c:283 + the reference
// stopping at the error).  Compiled with -fwrapv, as the reference's arithmetic wraps.
#include "amv_block_load.h"

namespace amv {

namespace {

struct __attribute__((aligned(4))) Px12 { uint32_t w[3]; };   // four BGR pixels

// Waves per workgroup: four consecutive MCU rows of a frame.  The waves share nothing (a segment's LDS is its wave's);
// the workgroup only exists so that the chip launches a quarter as many of them -- 1.28 M single-wave workgroups per
// 160 000 frames of 160x120 cost 8 % of the kernel's time in launches (profiles/r02_launch_rate.txt).
constexpr int kRowsPerGroup = 4;   // (five where fours leave too many slots idle: launch_reconstruct)

// 8-point inverse DCT of AmvJpeg.c: idctrow (:1082-1128) when kColumn == false, idctcol
// (:1130-1175, without its final clamp and with 7 of its final 14 bits of shift: clamp_pack has the rest) when true.
// The reference's all-AC-zero shortcuts (:1087-1092, :1134-1140) are not branched on.  They are special cases of this arithmetic only while the general
// formula does not leave 32 bits where the shortcut stays inside them: the row shortcut's 8 * dc is
// (dc * 2048 + 128) >> 8 for -2^20 <= dc < 2^20, the column shortcut's (x + 32) >> 6 is (x * 256 + 8192) >> 14 for
// -2^23 <= x <= 2^23 - 33.  Every coefficient block a scan can carry stays inside both (DC any int16, |AC| <= 1023:
// a row's first element is at most 32768 * 9 or 1023 * 61, a row-0 result at most 3.9 M), and so does every block whose
// |AC * step| <= 100 000 ("What the stage accessor promises"); beyond that -- through amvhip_reconstruct_dev
// only -- the kernel wraps where the reference's shortcut does not, and the pixels of such a block differ.
// The products are written per input (W1*a4 + W7*a5 instead of W7*(a4+a5) + (W1-W7)*a4): the same numbers
// modulo 2^32, which is what the reference's int arithmetic computes, but every factor is an INPUT of the
// pass and those always fit 24 bits -- a quantised coefficient times a step in the row pass, a value
// shifted right by 8 in the column pass -- so each product is one full-rate 24-bit multiply-add instead
// of a quarter-rate 32-bit multiply (a sum of two inputs can need 25 bits).  Only the two 181* products
// take arbitrary 32-bit operands.
// x * w + c with x and w inside 24 bits: one full-rate instruction, the low 32 bits of the exact result
__device__ __forceinline__ int mad24(int x, int w, int c) {
    int d;
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(d) : "v"(x), "s"(w), "v"(c));
    return d;
}

// The column pass takes its v0 and v4 -- results of rows 0 and 4 -- as 256 * v0 + 8192 and 256 * v4.  ((s >> 8) << 8 is
// s & ~255 for every 32-bit s, and 8192 is a multiple of 256, so (((s + 128) >> 8) << 8) + 8192 is (s + 128 + 8192) & ~255.)
// Those two rows therefore leave the row pass masked instead of shifted (kRow0 with the column's bias on top of the
// row's, kRow4 without), and the column pass neither shifts them up again nor adds: the same numbers modulo 2^32.
enum RowKind { kRowPlain, kRow0, kRow4 };

// The row pass's two 181-products carry their + 128 in from the odd products.  181 is odd, so there is an s with
// 181 * 2 s == 128 modulo 2^32: s = 64 / 181 modulo 2^31.  With + s in the chain of W1 x4 + W7 x5 and - s in that of
// W5 x6 + W3 x7 (the addends of their inner multiply-adds, zero otherwise) the sum of the two is what it was, their
// difference carries + 2 s, and both 181 * (that difference +- the other one) come out with the 128 in them: exact in
// the ring of the reference's wrapping int arithmetic.  Not in the column pass: its products are shifted right by 3
// before they meet, and a seed in front of an arithmetic shift is not exact once the sum wraps.
constexpr uint32_t inverse_of_odd(uint32_t a) {   // modulo 2^32 (Newton: each step doubles the bits that are right)
    uint32_t x = a;
    for (int i = 0; i < 5; ++i) x *= 2u - a * x;
    return x;
}
constexpr int kRowSeed = (int)((64u * inverse_of_odd(181u)) & 0x7fffffffu);
static_assert(181u * 2u * (uint32_t)kRowSeed == 128u, "the seed puts 128 into both 181-products");

// What follows the eight linear forms of a pass: the butterflies, the two 181-products, the shift or mask on the way out.
template <bool kColumn, RowKind kKind>
__device__ __forceinline__ void idct8_tail(int t, int a0, int a2, int a3, int a4, int a5, int a6, int a7,
                                           int& v0, int& v1, int& v2, int& v3, int& v4, int& v5, int& v6, int& v7) {
    constexpr int kOut = kColumn ? 7 : 8, kHalf = kColumn ? 128 : 0;
    int a1 = a4 + a6;
    a4 -= a6;
    a6 = a5 + a7;
    a5 -= a7;
    a7 = t + a3;
    t -= a3;
    a3 = a0 + a2;
    a0 -= a2;
    a2 = (181 * (a4 + a5) + kHalf) >> 8;      // (the row pass: the 128 came in with the seeds)
    a4 = (181 * (a4 - a5) + kHalf) >> 8;
    v0 = a7 + a1;
    v1 = a3 + a2;
    v2 = a0 + a4;
    v3 = t + a6;
    v4 = t - a6;
    v5 = a0 - a4;
    v6 = a3 - a2;
    v7 = a7 - a1;
    if (kKind == kRowPlain) {
        v0 >>= kOut; v1 >>= kOut; v2 >>= kOut; v3 >>= kOut; v4 >>= kOut; v5 >>= kOut; v6 >>= kOut; v7 >>= kOut;
    } else {
        v0 &= ~255; v1 &= ~255; v2 &= ~255; v3 &= ~255; v4 &= ~255; v5 &= ~255; v6 &= ~255; v7 &= ~255;
    }
}

template <bool kColumn, RowKind kKind = kRowPlain>
__device__ __forceinline__ void idct8(int& v0, int& v1, int& v2, int& v3, int& v4, int& v5, int& v6, int& v7) {
    constexpr int W1 = 2841, W2 = 2676, W3 = 2408, W5 = 1609, W6 = 1108, W7 = 565;
    constexpr int kBias = kKind == kRow0 ? 128 + 8192 : 128;
    constexpr int kRound = kColumn ? 4 : 0;
    constexpr int kDown = kColumn ? 3 : 0;
    constexpr int kSeed = kColumn ? 0 : kRowSeed;
    int a0 = kColumn ? v0 : v0 * 2048 + kBias, a1 = kColumn ? v4 : v4 * 2048;   // (<<11; the column's <<8 is done)
    const int i2 = v6, i3 = v2, i4 = v1, i5 = v7, i6 = v5, i7 = v3;
    int t;
    int a4 = mad24(i4, W1, mad24(i5, W7, kRound + kSeed)) >> kDown;     // W7*(x4+x5) + (W1-W7)*x4
    int a5 = mad24(i4, W7, mad24(i5, -W1, kRound)) >> kDown;    // W7*(x4+x5) - (W1+W7)*x5
    int a6 = mad24(i6, W5, mad24(i7, W3, kRound - kSeed)) >> kDown;     // W3*(x6+x7) - (W3-W5)*x6
    int a7 = mad24(i6, W3, mad24(i7, -W5, kRound)) >> kDown;    // W3*(x6+x7) - (W3+W5)*x7
    t = a0 + a1;
    a0 -= a1;
    int a2 = mad24(i3, W6, mad24(i2, -W2, kRound)) >> kDown;    // W6*(x3+x2) - (W2+W6)*x2
    int a3 = mad24(i3, W2, mad24(i2, W6, kRound)) >> kDown;     // W6*(x3+x2) + (W2-W6)*x3
    idct8_tail<kColumn, kKind>(t, a0, a2, a3, a4, a5, a6, a7, v0, v1, v2, v3, v4, v5, v6, v7);
}

// the quantiser steps, scan order, four to a dword: [0] luma, [1] chroma.  A lane reads its component's sixteen dwords
// once and multiplies by bytes of them (a select between two literals per coefficient cost 40 instructions a block).
struct QuantWords { uint32_t w[2][16]; };
constexpr QuantWords pack_quant() {
    QuantWords q{};
    for (int i = 0; i < 64; ++i) {
        q.w[0][i >> 2] |= (uint32_t)kQuantLuma[i] << (8 * (i & 3));
        q.w[1][i >> 2] |= (uint32_t)kQuantChroma[i] << (8 * (i & 3));
    }
    return q;
}
__device__ const QuantWords kQuantWords = pack_quant();

// ---- Stage B for a records frame without the entropy stage's mark (load_segment_blocks: small_ac): the row pass on
// paired 16-bit halves.  The eight linear forms in front of a row's butterflies are two-element dot products over the
// pairs (n0, n4), (n1, n7), (n5, n3), (n2, n6) of the row's dequantised inputs: v_dot2_i32_i16 with the weights in a
// scalar register and the bias or seed as its accumulator, the low 32 bits of the exact sum as mad24 gives them.  That
// needs every input as an int16: an AC of at most nine magnitude bits times the largest step does fit (asserted below),
// one of ten need not -- what the mark is for.  The DC times its step does not fit either; it enters row 0's even forms
// alone and stays a 32-bit number there.
constexpr uint32_t pair16(int lo, int hi) { return ((uint32_t)lo & 0xffffu) | ((uint32_t)hi << 16); }   // two int16 in a dword
constexpr int kPairCol[4][2] = {{0, 4}, {1, 7}, {5, 3}, {2, 6}};   // columns of a row's pair q: low half, high half
constexpr int pair_scan(int pair, int half) { return kScanOfNatural[8 * (pair >> 2) + kPairCol[pair & 3][half]]; }   // pair = 4 * row + q
constexpr int largest_step() {
    int m = 0;
    for (int i = 0; i < 64; ++i) m = kQuantLuma[i] > m ? kQuantLuma[i] : m;
    for (int i = 0; i < 64; ++i) m = kQuantChroma[i] > m ? kQuantChroma[i] : m;
    return m;
}
static_assert(largest_step() * 511 <= 32767, "nine magnitude bits times any step is an int16");
constexpr bool pairs_cover_the_scan() {   // the 64 halves are the 64 scan positions, each once; the DC is pair 0's low half
    bool seen[64] = {};
    for (int pair = 0; pair < 32; ++pair)
        for (int half = 0; half < 2; ++half) {
            if (seen[pair_scan(pair, half)]) return false;
            seen[pair_scan(pair, half)] = true;
        }
    return pair_scan(0, 0) == 0;
}
static_assert(pairs_cover_the_scan(), "kPairCol through kScanOfNatural");
static_assert(kAmvlibQuirkNatural % 8 == kPairCol[0][1], "amvlib's entry is the high half of its row's first pair");

// Dequantisation into pair registers: one multiply per coefficient as in the general form -- a sign-extended word of c[]
// times a byte of qw[] -- whose product's low 16 bits go to one half of the pair.  The low half's multiply writes the
// whole register, the high half's (dst_sel:WORD_1, UNUSED_PRESERVE) the upper half in place.  Written as the
// instructions, volatile, so that they stand in the order they are called in: a row's four low halves, its four high
// halves, then its dot products, first those of the pair whose high half was written first -- nothing reads a register
// straight after half of it was written.  (Row by row, not the whole block's low halves before all its high ones: with
// c[], qw[] and 32 pairs alive at once the kernel does not fit the 96 registers of five waves a SIMD.)
template <int kScan>
__device__ __forceinline__ void pair_lo(uint32_t& d, const uint32_t (&c)[32], const uint32_t (&qw)[16]) {
    asm volatile("v_mul_i32_i24_sdwa %0, sext(%1), %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_%3 src1_sel:BYTE_%4"
                 : "=v"(d) : "v"(c[kScan >> 1]), "v"(qw[kScan >> 2]), "n"(kScan & 1), "n"(kScan & 3));
}
template <int kScan>
__device__ __forceinline__ void pair_hi(uint32_t& d, const uint32_t (&c)[32], const uint32_t (&qw)[16]) {
    asm volatile("v_mul_i32_i24_sdwa %0, sext(%1), %2 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:WORD_%3 src1_sel:BYTE_%4"
                 : "+v"(d) : "v"(c[kScan >> 1]), "v"(qw[kScan >> 2]), "n"(kScan & 1), "n"(kScan & 3));
}
// pair 0 has no low half to keep (the DC goes its own way): its high half's multiply zeroes the rest
template <int kScan>
__device__ __forceinline__ void pair_hi_alone(uint32_t& d, const uint32_t (&c)[32], const uint32_t (&qw)[16]) {
    asm volatile("v_mul_i32_i24_sdwa %0, sext(%1), %2 dst_sel:WORD_1 dst_unused:UNUSED_PAD src0_sel:WORD_%3 src1_sel:BYTE_%4"
                 : "=v"(d) : "v"(c[kScan >> 1]), "v"(qw[kScan >> 2]), "n"(kScan & 1), "n"(kScan & 3));
}
// the four pairs of row kRow (amvlib: its table reads scan position 37 at natural (3,4), one more half write in row 3)
template <int kRow>
__device__ __forceinline__ void dequant_row_pairs(uint32_t (&p)[4], const uint32_t (&c)[32], const uint32_t (&qw)[16], bool amvlib) {
    constexpr int k = 4 * kRow;
    if (kRow != 0) pair_lo<pair_scan(k, 0)>(p[0], c, qw);
    pair_lo<pair_scan(k + 1, 0)>(p[1], c, qw);
    pair_lo<pair_scan(k + 2, 0)>(p[2], c, qw);
    pair_lo<pair_scan(k + 3, 0)>(p[3], c, qw);
    if (kRow != 0) pair_hi<pair_scan(k, 1)>(p[0], c, qw);
    else pair_hi_alone<pair_scan(k, 1)>(p[0], c, qw);
    if (kRow == kAmvlibQuirkNatural / 8 && amvlib) pair_hi<kAmvlibQuirkScan>(p[0], c, qw);
    pair_hi<pair_scan(k + 1, 1)>(p[1], c, qw);
    pair_hi<pair_scan(k + 2, 1)>(p[2], c, qw);
    pair_hi<pair_scan(k + 3, 1)>(p[3], c, qw);
}

// a.lo * w.lo + a.hi * w.hi (+ acc), 32-bit wrapping: the weights in a scalar register, the accumulator a vector one
// (this family takes one scalar operand an instruction) or the inline constant 0
__device__ __forceinline__ int dot2(uint32_t a, uint32_t w, int acc) {
    int d;
    asm("v_dot2_i32_i16 %0, %1, %2, %3" : "=v"(d) : "v"(a), "s"(w), "v"(acc));
    return d;
}
__device__ __forceinline__ int dot2(uint32_t a, uint32_t w) {
    int d;
    asm("v_dot2_i32_i16 %0, %1, %2, 0" : "=v"(d) : "v"(a), "s"(w));
    return d;
}
// One row from its four pairs; what it leaves in v0..v7 is what idct8<false, kKind> leaves.  even: the accumulator of
// the two even forms -- the bias, and in row 0 the DC's 2048 * dc + bias on top (its pair's low half is 0).
template <RowKind kKind>
__device__ __forceinline__ void idct8_row_pairs(uint32_t p04, uint32_t p17, uint32_t p53, uint32_t p26, int even,
                                                int& v0, int& v1, int& v2, int& v3, int& v4, int& v5, int& v6, int& v7) {
    constexpr int W1 = 2841, W2 = 2676, W3 = 2408, W5 = 1609, W6 = 1108, W7 = 565;
    const int t = dot2(p04, pair16(2048, 2048), even);
    const int a0 = dot2(p04, pair16(2048, -2048), even);
    const int a4 = dot2(p17, pair16(W1, W7), kRowSeed);
    const int a5 = dot2(p17, pair16(W7, -W1));
    const int a6 = dot2(p53, pair16(W5, W3), -kRowSeed);
    const int a7 = dot2(p53, pair16(W3, -W5));
    const int a2 = dot2(p26, pair16(W6, -W2));
    const int a3 = dot2(p26, pair16(W2, W6));
    idct8_tail<false, kKind>(t, a0, a2, a3, a4, a5, a6, a7, v0, v1, v2, v3, v4, v5, v6, v7);
}
// row kRow of the block: dequantised into its pairs, transformed into v[8 kRow ..]
template <int kRow>
__device__ __forceinline__ void pair_row(const uint32_t (&c)[32], const uint32_t (&qw)[16], bool amvlib, int even, int (&v)[64]) {
    uint32_t p[4];
    dequant_row_pairs<kRow>(p, c, qw, amvlib);
    int* const o = v + 8 * kRow;
    idct8_row_pairs<kRow == 0 ? kRow0 : (kRow == 4 ? kRow4 : kRowPlain)>(p[0], p[1], p[2], p[3], even, o[0], o[1], o[2], o[3], o[4], o[5], o[6], o[7]);
}

// iclp[] of AmvJpeg.c:1073-1080 (table spans -512..511; beyond it the reference reads out of bounds, defined here as
// saturation) of two column sums x >> 14, as two int16 in a dword.  The column pass hands over x >> 7, and for every
// 32-bit x  clamp(x >> 14, -256, 255) == sat_i16(x >> 7) >> 7: the shifts are arithmetic, so both sides are monotone
// in x and (x >> 7) >> 7 is x >> 14; -32768 >> 7 is -256 and 32767 >> 7 is 255.  v_cvt_pk_i16_i32 saturates both
// halves as it packs, and one packed shift finishes the pair: two instructions where two clamps and a permute stood.
// (Written as the instructions: the compiler must not pick a pack of its own here)
__device__ __forceinline__ uint32_t clamp_pack(int lo, int hi) {
    uint32_t p, d;
    asm("v_cvt_pk_i16_i32 %0, %1, %2" : "=v"(p) : "v"(lo), "v"(hi));
    asm("v_pk_ashrrev_i16 %0, %1, %2" : "=v"(d) : "s"(0x00070007u), "v"(p));   // (the count in both halves of a scalar)
    return d;
}

// a.lo * w.lo + a.hi * w.hi + 32768 (16-bit signed halves): the three-operand form, so that the bias stays in its
// register (the builtin becomes the accumulating form plus a move to reload the accumulator)
__device__ __forceinline__ uint32_t dot2_bias(uint32_t a, uint32_t w) {
    uint32_t d;
    asm("v_dot2_i32_i16 %0, %1, %2, %3" : "=v"(d) : "v"(a), "s"(w), "v"(32768u));
    return d;
}

// Stage D's arithmetic for one 4x2 patch (both of its loops use it), on byte pairs in the order they leave.  The twelve
// bytes of a patch row are (B0 G0)(R0 B1)(G1 R1)(B2 G2)(R2 B3)(G3 R3): each bracket is one packed add of a luma pair
// and a chroma pair, and one saturating pack.
// The chroma pairs of the patch's two chroma samples (uu, vv: two int16 each): (u, v) of sample e as one pair of int16;
// each term (:808-810, +128) is one two-element dot product, and bytes 1-2 of two of them -- the terms >> 8 -- make
// the pairs (b, g), (r, b) and (g, r) with one byte permute each.
struct ChromaTerms { uint32_t bg[2], rb[2], gr[2]; };
__device__ __forceinline__ ChromaTerms chroma_terms(uint32_t uu, uint32_t vv) {
    ChromaTerms c;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const uint32_t uv = __builtin_amdgcn_perm(vv, uu, e ? 0x07060302u : 0x05040100u);
        const uint32_t r = dot2_bias(uv, pair16(18, 367));
        const uint32_t gg = dot2_bias(uv, pair16(-159, -220));
        const uint32_t b = dot2_bias(uv, pair16(411, -29));
        c.bg[e] = __builtin_amdgcn_perm(gg, b, 0x06050201u);
        c.rb[e] = __builtin_amdgcn_perm(b, r, 0x06050201u);
        c.gr[e] = __builtin_amdgcn_perm(r, gg, 0x06050201u);
    }
    return c;
}
// One dword of the row: (ya + c0.lo, yb + c0.hi, yc + c1.lo, yd + c1.hi) clamped to 0..255 (:812-827), a byte each.
// The luma of a bracket is (y.lo, y.lo), (y.lo, y.hi) or (y.hi, y.hi) of one luma pair: kLo / kHi say which half of y
// goes to the add's low / high result (op_sel and op_sel_hi of the first operand: no instruction of their own).  The
// first pack writes bytes 0-1 of the dword and zeroes the rest, the second (SDWA, UNUSED_PRESERVE) its high half in place.
// (Nothing but the frame store reads such a dword: the compiler does not see into these statements and pads no hazard
// for them, and the one this chip has behind a write of half a register concerns a vector instruction that reads it.)
template <int kLo, int kHi>
__device__ __forceinline__ uint32_t pair_sum(uint32_t yy, uint32_t cc) {
    uint32_t sum;
    if (kLo == 0 && kHi == 0) asm("v_pk_add_i16 %0, %1, %2 op_sel_hi:[0,1]" : "=v"(sum) : "v"(yy), "v"(cc));
    else if (kLo == 0 && kHi == 1) asm("v_pk_add_i16 %0, %1, %2" : "=v"(sum) : "v"(yy), "v"(cc));
    else asm("v_pk_add_i16 %0, %1, %2 op_sel:[1,0]" : "=v"(sum) : "v"(yy), "v"(cc));
    static_assert(kLo <= kHi, "(hi, lo) is not a bracket of the row");
    return sum;
}
__device__ __forceinline__ uint32_t sat_quad(uint32_t lo, uint32_t hi) {
    uint32_t d;
    asm("v_sat_pk_u8_i16 %0, %1" : "=v"(d) : "v"(lo));
    asm("v_sat_pk_u8_i16_sdwa %0, %1 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD" : "+v"(d) : "v"(hi));
    return d;
}
// ... and the twelve bytes of one of its rows (yy: four int16 of luma), :829-831 B,G,R
__device__ __forceinline__ Px12 patch_row(uint2 yy, const ChromaTerms& c) {
    Px12 v;
    v.w[0] = sat_quad(pair_sum<0, 0>(yy.x, c.bg[0]), pair_sum<0, 1>(yy.x, c.rb[0]));   // B0 G0 R0 B1
    v.w[1] = sat_quad(pair_sum<1, 1>(yy.x, c.gr[0]), pair_sum<0, 0>(yy.y, c.bg[1]));   // G1 R1 B2 G2
    v.w[2] = sat_quad(pair_sum<0, 1>(yy.y, c.rb[1]), pair_sum<1, 1>(yy.y, c.gr[1]));   // R2 B3 G3 R3
    return v;
}

// The column pass over a block whose rows are done, and stage C: GetYUV (AmvJpeg.c:754-787), one 16-byte row at a time.
// The +128 of IQtIZzBlock (:1023,1047) joins the chroma terms in stage D (it cannot ride through the column pass on the
// DC term: the reference's 32-bit arithmetic wraps on absurd coefficients, and the parity tests hold the kernel to that).
// s_mem: the segment's planes -- 16 rows of Y, 8 of U, 8 of V; lane: the block in the segment.
__device__ __forceinline__ void columns_to_plane(int (&v)[64], uint32_t lane, int16_t* s_mem) {
    constexpr uint32_t kPitchY = kSegMcus * 16, kPitchC = kSegMcus * 8;   // int16 units
#pragma unroll
    for (int col = 0; col < 8; ++col)
        idct8<true>(v[col], v[8 + col], v[16 + col], v[24 + col], v[32 + col], v[40 + col], v[48 + col], v[56 + col]);
    const uint32_t m = lane / 6u, k6 = lane % 6u;
    const bool chroma = k6 >= 4u;
    int16_t* dst = chroma ? s_mem + 16 * kPitchY + (k6 == 4u ? 0u : 8 * kPitchC) + m * 8u
                          : s_mem + ((k6 >> 1) * 8u) * kPitchY + m * 16u + (k6 & 1u) * 8u;
    const uint32_t pitch = chroma ? kPitchC : kPitchY;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        uint32_t w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) w[q] = clamp_pack(v[8 * r + 2 * q], v[8 * r + 2 * q + 1]);
        *reinterpret_cast<uint4*>(dst + r * pitch) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

}  // namespace

// kRound: a round launch (FrameSel::round != 0), whose workgroups walk the items of the round
template <bool kRound, int kRows>
__global__ __launch_bounds__(kWave * kRows) void amv_reconstruct_kernel(
    SyncSinks in, const uint32_t* __restrict__ nmcu_ok, uint32_t n, FrameSel sel,
    FrameGeom g, PieceMap pm, uint32_t flags, uint8_t* __restrict__ out) {
    constexpr uint32_t kPitchY = kSegMcus * 16, kPitchC = kSegMcus * 8;   // int16 units
    // 7 680 bytes (+ the scatter's spare slots): first the records' image of the 60 blocks (128 bytes each), then the three planes
    __shared__ __attribute__((aligned(16))) int16_t s_all[kRows][16 * kPitchY + 2 * 8 * kPitchC + 64];
    static_assert((16 * kPitchY + 2 * 8 * kPitchC) * 2 == kSegImageBytes, "the planes reuse the image");
    // (the wave's number as a scalar: what follows from it -- its MCU row, its LDS, the scatter's constants -- stays out of the vector registers)
    const uint32_t lane = threadIdx.x & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint32_t item, row_group, seg;
    if (!locate_piece(pm, blockIdx.x, item, row_group, seg)) return;
    const uint32_t my = row_group * kRows + wave;
    if (my >= g.mcu_rows) return;                   // (the whole wave)
    int16_t* const s_mem = s_all[wave];
    int16_t* const s_y = s_mem;
    int16_t* const s_u = s_mem + 16 * kPitchY;
    int16_t* const s_v = s_u + 8 * kPitchC;
    uint8_t* const s_img = reinterpret_cast<uint8_t*>(s_mem);

    uint32_t qw[16];   // this lane's quantiser steps (blocks 4 and 5 of an MCU are chroma), on their way while stage A runs
    {
        const uint4* q4 = reinterpret_cast<const uint4*>(kQuantWords.w[lane % 6u >= 4u ? 1 : 0]);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint4 q = q4[i];
            qw[4 * i] = q.x; qw[4 * i + 1] = q.y; qw[4 * i + 2] = q.z; qw[4 * i + 3] = q.w;
        }
    }
    do {
    uint32_t f, slot;
    if (!select_frame(sel, n, item, f, slot)) return;
    const Segment sg = segment_of(f, slot, nmcu_ok, g, pm.nseg, my, seg);
    const uint32_t m0 = sg.m0, cnt = sg.cnt, ok = sg.ok, mcu0 = sg.mcu0;

    // ---- A + B + C: one block per lane
    BlockForm form;
    bool skip;
    if (stage_segment_blocks(in, sg, kRound, g, lane, s_img, form, skip)) {
        uint32_t c[32];
        int v[64];
        // Stage B's row pass in two forms; each fetches its block itself (fetched in front of the branch, the 32 registers
        // that come from LDS or from dense lines have two readers, the compiler keeps both sets, and the kernel no longer
        // fits the 96 registers of five waves a SIMD).
        if (form.small_ac) {   // (wave-uniform) no AC of the frame has ten magnitude bits: the row pass on paired halves
            fetch_block(in, sg, g, lane, s_img, BlockForm{true, true, form.dc_base}, c);
            const bool amvlib = !(flags & kFlagZigzagFixed);
            const int dc = coef_at(c, 0) * (int)(qw[0] & 255u);
            pair_row<0>(c, qw, amvlib, dc * 2048 + (128 + 8192), v);
            pair_row<1>(c, qw, amvlib, 128, v);
            pair_row<2>(c, qw, amvlib, 128, v);
            pair_row<3>(c, qw, amvlib, 128, v);
            pair_row<4>(c, qw, amvlib, 128, v);
            pair_row<5>(c, qw, amvlib, 128, v);
            pair_row<6>(c, qw, amvlib, 128, v);
            pair_row<7>(c, qw, amvlib, 128, v);
        } else {   // the general form: marked frames, dense lines
        fetch_block(in, sg, g, lane, s_img, form, c);
        // IQtIZzBlock's gather (AmvJpeg.c:1035-1042): out[nat] = coef[scan(nat)] * step[scan(nat)], a row at a time in
        // front of the row's transform and held there (sched_barrier): all 64 products ahead of the rows, as the compiler
        // places them when left alone, need seven registers more than the kernel has beside the other form
#pragma unroll
        for (int r = 0; r < 8; ++r) {
#pragma unroll
            for (int nat = 8 * r; nat < 8 * r + 8; ++nat) {
                const int scan = kScanOfNatural[nat];
                v[nat] = coef_at(c, scan) * (int)((qw[scan >> 2] >> (8 * (scan & 3))) & 255u);
            }
            if (r == kAmvlibQuirkNatural / 8 && !(flags & kFlagZigzagFixed))     // amvlib's table reads scan position 37 at natural (3,4)
                v[kAmvlibQuirkNatural] = coef_at(c, kAmvlibQuirkScan) * (int)((qw[kAmvlibQuirkScan >> 2] >> (8 * (kAmvlibQuirkScan & 3))) & 255u);
            if (r == 0) idct8<false, kRow0>(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]);
            else if (r == 4) idct8<false, kRow4>(v[32], v[33], v[34], v[35], v[36], v[37], v[38], v[39]);
            else idct8<false>(v[8 * r], v[8 * r + 1], v[8 * r + 2], v[8 * r + 3], v[8 * r + 4], v[8 * r + 5], v[8 * r + 6], v[8 * r + 7]);
            __builtin_amdgcn_sched_barrier(0);
        }
        }
        columns_to_plane(v, lane, s_mem);
    }
    if (skip) return;   // (wave-uniform) not this launch's frame
    seg_sync();

    // ---- D: StoreBuffer (AmvJpeg.c:789-840), straight to the frame.  A lane takes a 4x2-pixel patch: the two rows
    // share their chroma samples, whose three products (:808-810) are formed once, with luma's +128 folded in:
    // (256 (y + 128) + c) >> 8 == y + ((c + 32768) >> 8) exactly.  Everything that follows fits 16 bits (|y| <= 256,
    // |c >> 8| <= 440), so two bytes go through each instruction, paired as they lie in the row (patch_row): v_pk_add_i16
    // adds a pair of luma values to a pair of chroma terms, v_sat_pk_u8_i16 clamps both sums to 0..255 (:812-827) and packs
    // them into two bytes of their dword -- twelve instructions a row, nothing to interleave afterwards.  MCUs that
    // were not decoded get y = -1024, c = 0: every channel clamps to 0.
    const uint32_t vr = min(16u, g.height - my * 16u);                 // rows of this MCU row inside the picture (:798); even
    const uint32_t px = min(cnt * 16u, g.width - m0 * 16u);            // pixels of this segment inside it (:803)
    const uint32_t groups = cnt * 4u;
    const bool all_decoded = mcu0 + cnt <= ok;                         // wave-uniform: the usual case skips the per-patch test
    // one base per wave (scalar) + 32-bit byte offsets inside the frame: picture row my*16+i is destination row
    // H-1-(my*16+i) (:800)
    uint8_t* const frame = out + (uint64_t)f * g.frame_bytes;
    const uint32_t row0 = (g.height - 1u - my * 16u) * g.stride + m0 * 48u;
    // Patch t = lane, lane + 64, ...: row pair i2 = t / groups, group gi = t % groups.  In bytes: a row pair is
    // 4 * kPitchY of luma and 2 * kPitchC of each chroma plane in LDS and 2 * stride back in the frame, a group 8, 4 and 12 on.
    constexpr uint32_t kPairY = 4u * kPitchY, kPairC = 2u * kPitchC, kPlaneU = 32u * kPitchY, kPlaneV = kPlaneU + 16u * kPitchC;
    if (all_decoded && cnt == kSegMcus && px == kSegMcus * 16u && vr == 16u) {
        // A whole segment (wave-uniform; every wave of a 160x120 frame but its bottom row's): 40 groups in 8 row pairs,
        // five trips, nothing to test per lane and every row a 12-byte store.  64 k patches on, trip k is q row pairs
        // and r groups further; the lanes whose group then lies past the row's end (b + r >= 40) are one more row pair
        // on and 40 groups back: a select between two fixed values of the lane, never a lane mask.  The 40 groups of a
        // chroma row are its 160 bytes: patch t's chroma is at 4 t.  What depends on k alone is a constant of the LDS
        // read or goes into the trip's scalar base (the lane's part of the frame offset stays positive: the MCU row has
        // 15 picture rows below its first in the buffer, and the lane's part goes back at most four).
        constexpr uint32_t kGroups = kSegMcus * 4u, kTrips = kGroups * 8u / kWave;
        static_assert(kGroups * 8u % kWave == 0u && kGroups < kWave && kPairC == kGroups * 4u, "whole trips; chroma is linear in t");
        const uint32_t a = lane >= kGroups ? 1u : 0u, b = lane - a * kGroups;
        const uint8_t* const ly = s_img + a * kPairY + b * 8u;
        const uint8_t* const ly_past = ly + (kPairY - kGroups * 8u);
        const uint8_t* const lc = s_img + kPlaneU + lane * 4u;
        const uint32_t off0 = row0 - a * 2u * g.stride + b * 12u;
        const uint32_t off0_past = off0 - 2u * g.stride - kGroups * 12u;
#pragma unroll
        for (uint32_t k = 0; k < kTrips; ++k) {
            const uint32_t q = k * kWave / kGroups, r = k * kWave % kGroups;
            const bool past = r != 0u && b >= kGroups - r;
            const uint8_t* const y = (past ? ly_past : ly) + (q * kPairY + r * 8u);
            const uint2 ya = *reinterpret_cast<const uint2*>(y);
            const uint2 yb = *reinterpret_cast<const uint2*>(y + 2u * kPitchY);
            const uint32_t uu = *reinterpret_cast<const uint32_t*>(lc + k * kWave * 4u);
            const uint32_t vv = *reinterpret_cast<const uint32_t*>(lc + k * kWave * 4u + (kPlaneV - kPlaneU));
            const ChromaTerms c = chroma_terms(uu, vv);
            uint8_t* const upper = frame + (int64_t)(int32_t)(r * 12u - q * 2u * g.stride);   // (scalar)
            const uint32_t off = past ? off0_past : off0;
            *reinterpret_cast<Px12*>(upper + off) = patch_row(ya, c);
            *reinterpret_cast<Px12*>(upper - g.stride + off) = patch_row(yb, c);
        }
        continue;   // (to next_item)
    }
    // Everything else -- the picture's bottom and right edges, short segments, damaged frames: i2 and gi kept up by
    // addition, the offsets formed from them on every trip (carried along and corrected where a group runs past the
    // row's end they cost more instructions than the multiplies they replace: DESIGN.md, Appendix A.3)
    const uint32_t pairs = (vr + 1u) >> 1;
    const uint32_t step_i2 = kWave / groups, step_gi = kWave - step_i2 * groups;
    uint32_t i2 = lane / groups, gi = lane - i2 * groups;
    for (; i2 < pairs; i2 += step_i2, gi += step_gi) {
        if (gi >= groups) { gi -= groups; ++i2; if (i2 >= pairs) break; }
        const uint32_t lc = gi * 4u;
        uint2 ya = *reinterpret_cast<const uint2*>(s_y + (2u * i2) * kPitchY + lc);
        uint2 yb = *reinterpret_cast<const uint2*>(s_y + (2u * i2 + 1u) * kPitchY + lc);
        uint32_t uu = *reinterpret_cast<const uint32_t*>(s_u + i2 * kPitchC + (lc >> 1));
        uint32_t vv = *reinterpret_cast<const uint32_t*>(s_v + i2 * kPitchC + (lc >> 1));
        if (!all_decoded && (mcu0 + (gi >> 2)) >= ok) {
            constexpr uint32_t kDark = 0xfc00fc00u;                    // two int16 of -1024
            ya.x = ya.y = yb.x = yb.y = kDark;
            uu = vv = 0u;
        }
        const ChromaTerms c = chroma_terms(uu, vv);                    // the chroma term of both pixels of a pair
        if (lc >= px) continue;                                        // right of the picture
        uint32_t off = row0 - 2u * i2 * g.stride + lc * 3u;
#pragma unroll
        for (int row = 0; row < 2; ++row) {
            const Px12 v = patch_row(row ? yb : ya, c);
            if (2u * i2 + (uint32_t)row >= vr) break;                      // odd picture height
            if (lc + 4u <= px) {                                           // rows are 4-byte aligned (AmvJpeg.c:1524), lc*3 is 0 mod 4
                *reinterpret_cast<Px12*>(frame + off) = v;
            } else {                                                       // the picture's last 1-3 pixels
#pragma unroll
                for (uint32_t q = 0; q < 9u; ++q)
                    if (q < (px - lc) * 3u) frame[off + q] = (uint8_t)(v.w[q >> 2] >> (8u * (q & 3u)));
            }
            off -= g.stride;
        }
    }
    } while (next_item<kRound>(pm, item));   // (the planes are free again)
}

template <int kRows, class... Args>
static void launch_rows(const FrameGeom& g, Args... args) {
    launch_segments(amv_reconstruct_kernel<false, kRows>, amv_reconstruct_kernel<true, kRows>, kWave * kRows, (g.mcu_rows + kRows - 1) / kRows, args...);
}

void launch_reconstruct(const SyncSinks& sinks, const uint32_t* nmcu_ok, uint32_t n, const FrameSel& sel, uint32_t items,
                        const FrameGeom& g, uint32_t flags, uint8_t* out, hipStream_t s) {
    // A workgroup's waves are consecutive MCU rows of one frame, and the last workgroup of a frame has idle slots unless
    // the rows divide.  Fives only where fours waste a tenth of the slots more than fives do (176x144, 9 rows: 4.80 ms
    // per 100 000 frames against 5.04): five waves do not spread evenly over a CU's four SIMDs, and 320x240 (15 rows,
    // one slot in sixteen idle in fours) takes 6.29 ms per 64 000 frames in fives against 5.87 in fours.
    const uint32_t slots4 = (g.mcu_rows + 3u) / 4u * 4u, slots5 = (g.mcu_rows + 4u) / 5u * 5u;
    const uint32_t waste4 = slots4 - g.mcu_rows, waste5 = slots5 - g.mcu_rows;
    if (10u * waste4 * slots5 >= 10u * waste5 * slots4 + slots4 * slots5) launch_rows<5>(g, sinks, nmcu_ok, n, sel, items, g, s, flags, out);
    else launch_rows<kRowsPerGroup>(g, sinks, nmcu_ok, n, sel, items, g, s, flags, out);
}

// Records -> dense lines (amvhip_huffman_decode_dev, not on the decode path): stage A of the kernel above for one
// (frame, MCU-row segment) per wave, then every lane with a block stores it as the block's 128-byte line.  The waves
// walk a flat list of (frame, segment) pairs.
__global__ __launch_bounds__(kWave * 4) void amv_expand_records_kernel(SyncSinks in, const uint32_t* __restrict__ nmcu_ok, uint32_t n,
                                                                        FrameGeom g, uint32_t nseg, int16_t* __restrict__ coef) {
    __shared__ __attribute__((aligned(16))) uint8_t s_img[4][kSegImageBytes + 128];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t segs = g.mcu_rows * nseg;
    const uint64_t pairs = (uint64_t)n * segs;
    for (uint64_t p = (uint64_t)blockIdx.x * 4u + wave; p < pairs; p += (uint64_t)gridDim.x * 4u) {
        const uint32_t f = (uint32_t)(p / segs), segidx = (uint32_t)(p % segs);
        const Segment sg = segment_of(f, f, nmcu_ok, g, nseg, segidx / nseg, segidx % nseg);
        uint32_t c[32];
        bool skip;   // (a frame the serial kernel decodes: its lines are that kernel's)
        if (load_segment_blocks(in, sg, false, g, lane, s_img[wave], c, skip)) {
            const uint32_t blk = sg.mcu0 * 6u + lane;
            if (blk >= (in.ok_in_blocks ? sg.ok : sg.ok * 6u)) {   // at or after the first error: no records, but the DC base was added
#pragma unroll
                for (int i = 0; i < 32; ++i) c[i] = 0u;
            }
            uint4* d = reinterpret_cast<uint4*>(coef + ((uint64_t)f * g.blocks + blk) * 64u);
#pragma unroll
            for (int i = 0; i < 8; ++i) d[i] = make_uint4(c[4 * i], c[4 * i + 1], c[4 * i + 2], c[4 * i + 3]);
        }
        seg_sync();   // every lane has read the image
    }
}

void launch_expand_records(const SyncSinks& sinks, const uint32_t* nmcu_ok, uint32_t n, const FrameGeom& g, int16_t* coef,
                           hipStream_t s) {
    const uint32_t nseg = segs_per_row(g);
    const uint64_t groups = ((uint64_t)n * g.mcu_rows * nseg + 3u) / 4u;
    if (groups == 0) return;
    hipLaunchKernelGGL(amv_expand_records_kernel, dim3(groups < 65536u ? (uint32_t)groups : 65536u), dim3(kWave * 4), 0, s, sinks,
                       nmcu_ok, n, g, nseg, coef);
}

}  // namespace amv
