// amv_rate_plan.h -- the arithmetic of the video encoder's byte budget per frame, free of HIP: what the kernels of
// amv_encode_rate.hip and tests/c/rate_plan_test.cc both run.
//
// AMV's quantiser tables are fixed, so the reference's -b does nothing for its amv encoder (mpegvideo_enc.c:492-496 fixes the
// qscale).  The lever here is the trellis quantiser's lambda (amv_trellis_plan.h): a caller hands a ladder of lambdas in the
// order of preference and a budget of bytes per frame, and every frame is coded at the FIRST rung whose chunk fits.
//
// A chunk is FF D8, the scan, FF D9: its length is 4 + ceil(bits / 8) + escapes, where bits is what the entropy coder writes
// for the scan (the DC codes and magnitudes, the AC run/size codes, magnitudes, ZRLs and EOBs) and escapes the number of FF
// bytes of the padded scan (each followed by a 00, mjpegenc.c:282-336).  Bits follow from the levels alone; escapes do not.
//   floor(bits) = 4 + ceil(bits / 8) <= len:  a rung whose floor misses the budget cannot fit; one whose floor meets it fits
//   unless escapes push it over.  The first rung that truly fits lies at or after the first floor-fit, and no rung between two
//   consecutive floor-fits can fit: walking the floor-fits in order and checking real lengths reaches exactly the first fit.
// Sizes are not monotone in lambda (a larger lambda can cost a byte), so nothing here bisects.
//
// The bound: a frame's bits against 2^32.  amvhip_encode_bound allows 4 bytes per coefficient, doubled for escapes, + 4:
// bits <= 4 * (bound - 4) = blocks * 64 * 32.  That is below 2^32 while blocks * 2048 < 2^32: up to kRateBlocksMost blocks
// (349 525 MCUs; 9456 x 9456 is inside).  The rate entries refuse larger pictures.
#pragma once
#include <stdint.h>

#include "amv_segment.h"
#include "amv_tables.h"
#include "amv_trellis_plan.h"

namespace amv {

constexpr uint32_t kRateRungsMax = 16;            // AMVHIP_RATE_RUNGS_MAX
constexpr uint32_t kRateOver = 0x80000000u;       // AMVHIP_RATE_OVER
constexpr uint32_t kRateBitsPerBlockMost = 64u * 32u;
constexpr uint32_t kRateBlocksMost = 0xffffffffu / kRateBitsPerBlockMost;
static_assert((uint64_t)kRateBlocksMost * kRateBitsPerBlockMost <= 0xffffffffull, "a frame's bits fit 32");
AMV_HD inline bool rate_blocks_ok(uint32_t blocks) { return blocks <= kRateBlocksMost; }

// ---- the DC term ----------------------------------------------------------------------------------------------------------
// len[comp][size]: AMV's DC code (ff_mjpeg_build_huffman_codes over the fixed specification, both classes; size 0 .. 11)
struct RateDcLen {
    uint8_t len[2][12];
};
constexpr RateDcLen make_rate_dc_len() {
    RateDcLen t{};
    for (int comp = 0; comp < 2; ++comp) {
        int k = 0;
        for (int l = 1; l <= 16; ++l)
            for (int n = 0; n < kHuffCount[comp][l - 1]; ++n, ++k) t.len[comp][kHuffDcSymbols[k]] = (uint8_t)l;
    }
    return t;
}
// bits of the difference `diff` between a block's quantised DC and its component's predecessor (ff_mjpeg_encode_dc,
// mjpegenc.c:357-377): the size's code, then the magnitude
AMV_HD inline uint32_t rate_dc_bits(const uint8_t* dc_len, int32_t diff) {
    const uint32_t nb = trellis_nbits((uint32_t)(diff < 0 ? -diff : diff));
    return dc_len[nb] + nb;
}
// the block of the same component coded before block b of a frame (MCU order: Y0 Y1 Y2 Y3 Cb Cr), or -1 for the first
AMV_HD inline int64_t rate_dc_predecessor(uint32_t b) {
    const uint32_t k6 = b % 6u;
    if (k6 >= 1u && k6 <= 3u) return (int64_t)b - 1;
    if (b < 6u) return -1;
    return k6 == 0u ? (int64_t)b - 3 : (int64_t)b - 6;
}

// ---- a block's AC bits ----------------------------------------------------------------------------------------------------
// line: get(k) over the block's levels in scan order (as trellis_block left them); len: the component class's AC code
// lengths (TrellisTables::len[comp]) -> the run/size codes, magnitudes and ZRLs of positions 1 .. 63, and the EOB
template <class Line>
AMV_HD inline uint32_t rate_block_bits(const Line& line, const uint8_t* len) {
    uint32_t bits = 0, coded = 0;                 // coded: the last position with a level (0: none yet)
    for (uint32_t k = 1; k < 64u; ++k) {
        const int32_t v = line.get(k);
        if (!v) continue;
        bits += trellis_bits(len, k - coded - 1u, (uint32_t)(v < 0 ? -v : v));
        coded = k;
    }
    return bits + trellis_eob_bits(len, coded);
}

// ---- floors and the first fit -----------------------------------------------------------------------------------------------
AMV_HD inline uint32_t rate_floor_bytes(uint32_t bits) { return 4u + bits / 8u + ((bits & 7u) ? 1u : 0u); }   // (no wrap at 2^32 - 1)
// the first rung at or after `from` whose floor is <= budget, or `rungs`
AMV_HD inline uint32_t rate_first_fit(const uint32_t* row, uint32_t rungs, uint32_t budget, uint32_t from) {
    for (uint32_t r = from; r < rungs; ++r)
        if (rate_floor_bytes(row[r]) <= budget) return r;
    return rungs;
}

// ---- one step of the choice, as the device takes it -------------------------------------------------------------------------
// A frame's record is its rung with kRateOver or-ed in once it is final.  rate_choose: where a frame starts.  rate_check:
// what a coded length does to a frame that is not final -- true: the frame is to be coded again (at the new record's rung).
AMV_HD inline uint32_t rate_choose(const uint32_t* row, uint32_t rungs, uint32_t budget) {
    const uint32_t r = rate_first_fit(row, rungs, budget, 0u);
    return r < rungs ? r : (rungs - 1u) | kRateOver;
}
AMV_HD inline bool rate_check(const uint32_t* row, uint32_t rungs, uint32_t budget, uint32_t len, uint32_t& record) {
    if ((record & kRateOver) || len <= budget) return false;
    const uint32_t at = record, r = rate_first_fit(row, rungs, budget, at + 1u);
    record = r < rungs ? r : (rungs - 1u) | kRateOver;
    return r < rungs || at != rungs - 1u;         // (over on the last rung itself: its chunk is the one that stands)
}

}  // namespace amv
