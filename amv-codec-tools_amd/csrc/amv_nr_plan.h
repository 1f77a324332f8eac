// amv_nr_plan.h -- the arithmetic of the reference's -nr noise reduction, free of HIP: what the kernels of amv_encode_nr.hip,
// the denoise step of amv_encode_common.h and tests/c/nr_plan_test.cc all run.
//
// Reference path (lavc = libavcodec):
//   update_noise_reduction     lavc/mpegvideo.c:861-876, from MPV_frame_start :997-1000 -- at the start of every frame
//   denoise_dct_c              lavc/mpegvideo_enc.c:2937-2959, from dct_quantize_c :3660-3661 -- every block, between
//                              fdct and quantiser
// State per stream (the intra halves; AMV is intra only): int dct_error_sum[64], int dct_count, and the offsets
// uint16_t dct_offset[64] made from them at every frame start.  Index i is the fdct output's own row-major order; the six
// blocks of an MCU share the one array.  The sums are taken BEFORE the offset is applied (:2948, :2952), so the offsets of
// frame f are a function of the sums over the frames before it and of no earlier offset.
//
// This encoder's fdct runs on samples - 128, the reference's on the samples themselves; the outputs differ at position 0
// alone, where reference DC = ours + 8192 exactly (64 samples x 128 x 8 / 8).  The DC rule follows: D = x + 8192 is summed
// and denoised, x' = D' - 8192 goes on to the quantiser.
#pragma once
#include <stdint.h>

#include "amv_segment.h"

namespace amv {

constexpr uint32_t kNrStateWords = 65;          // the caller's state: 64 sums (reference index order), then the count
constexpr int32_t kNrHalveAbove = 1 << 16;      // mpegvideo.c:865
constexpr int32_t kNrDcShift = 8192;            // reference DC - this encoder's DC
constexpr uint32_t kNrLargest = 16320;          // the largest magnitude a position can hold: the un-shifted DC of a block of 255s

// ---- the argument bound ---------------------------------------------------------------------------------------------
// B = blocks per frame (padding blocks included).  A frame starts by halving a count above 65536, then codes B blocks:
//   count after the halving <= C0 = max(65536, B)   (c <= C0 + B before it, and (C0 + B) / 2 <= C0 since B <= C0)
//   count at any time       <= C1 = C0 + B
// A sum grows by at most 16320 a block, and the halving floors sum and count separately, which lets a sum run ahead of
// 16320 x count by at most 16320 (e -> e / 2 + 8160 per halving): sum <= 16320 x (count + 1) throughout.
// Nothing wraps when   16320 x (C1 + 1) + 1 <= INT32_MAX            (the sum, and the divisor sum + 1)
//                and   nr x C0 + 16320 x (C0 + 1) / 2 <= INT32_MAX  (the dividend, made after the halving).
AMV_HD inline uint32_t nr_count_start_most(uint32_t blocks) { return blocks > (uint32_t)kNrHalveAbove ? blocks : (uint32_t)kNrHalveAbove; }
AMV_HD inline uint64_t nr_count_most(uint32_t blocks) { return (uint64_t)nr_count_start_most(blocks) + blocks; }
AMV_HD inline bool nr_frame_ok(uint32_t blocks) {
    return blocks > 0u && (uint64_t)kNrLargest * (nr_count_most(blocks) + 1u) + 1u <= 0x7fffffffull;
}
// the largest nr a frame of `blocks` blocks takes; 0: the frame is too large for any (nr = 0 is the plain encoder)
AMV_HD inline uint32_t nr_max(uint32_t blocks) {
    if (!nr_frame_ok(blocks)) return 0u;
    const uint64_t c0 = nr_count_start_most(blocks);
    return (uint32_t)((0x7fffffffull - (uint64_t)kNrLargest * (c0 + 1u) / 2u) / c0);
}

// ---- update_noise_reduction, one position -----------------------------------------------------------------------------
AMV_HD inline bool nr_halving_due(int32_t count) { return count > kNrHalveAbove; }
// dct_offset[i] after the halving: int arithmetic, stored as uint16_t -- the truncation is the reference's behaviour.
// Inside the bound nothing here wraps.  A state the caller made up may hold anything: the arithmetic is then done on
// two's complement wrap, and a divisor that is not positive gives offset 0, so that no state can trap.
AMV_HD inline uint16_t nr_offset(uint32_t nr, int32_t count, int32_t sum) {
    const int32_t den = (int32_t)((uint32_t)sum + 1u);
    if (den <= 0) return 0;
    const int32_t num = (int32_t)(nr * (uint32_t)count + (uint32_t)(sum / 2));
    return (uint16_t)(num / den);
}

// ---- denoise_dct_c, one coefficient -------------------------------------------------------------------------------------
// x: this encoder's fdct output at a position other than 0
AMV_HD inline uint32_t nr_magnitude(int32_t x) { return (uint32_t)(x < 0 ? -x : x); }
AMV_HD inline int32_t nr_denoise(int32_t x, uint32_t offset) {
    const int32_t a = (int32_t)nr_magnitude(x) - (int32_t)offset;
    const int32_t kept = a > 0 ? a : 0;
    return x < 0 ? -kept : kept;
}
// ... and at position 0: the reference's DC is x + 8192 >= 0
AMV_HD inline uint32_t nr_magnitude_dc(int32_t x) { return (uint32_t)(x + kNrDcShift); }
AMV_HD inline int32_t nr_denoise_dc(int32_t x, uint32_t offset) {
    const int32_t d = x + kNrDcShift - (int32_t)offset;
    return (d > 0 ? d : 0) - kNrDcShift;
}

// ---- whole-state forms (the chain kernel does the same a position per lane) -----------------------------------------------
// state: 64 sums, then the count.  offset: reference index order.
AMV_HD inline void nr_frame_start(int32_t* state, uint32_t nr, uint16_t* offset) {
    if (nr_halving_due(state[64])) {
        for (int i = 0; i < 64; ++i) state[i] >>= 1;
        state[64] >>= 1;
    }
    for (int i = 0; i < 64; ++i) offset[i] = nr_offset(nr, state[64], state[i]);
}
// one block of this encoder's fdct outputs, in place
AMV_HD inline void nr_block(int32_t* state, const uint16_t* offset, int16_t* block) {
    state[64] = (int32_t)((uint32_t)state[64] + 1u);
    state[0] = (int32_t)((uint32_t)state[0] + nr_magnitude_dc(block[0]));
    block[0] = (int16_t)nr_denoise_dc(block[0], offset[0]);
    for (int i = 1; i < 64; ++i) {
        state[i] = (int32_t)((uint32_t)state[i] + nr_magnitude(block[i]));
        block[i] = (int16_t)nr_denoise(block[i], offset[i]);
    }
}

// ---- workspace of a call of n frames ----------------------------------------------------------------------------------------
// sums: uint32 [n][64], a frame's magnitudes per position (reference index order; at most blocks x 16320 < 2^31 each);
// offsets: uint16 [n][64], a frame's offsets in the order the column pass consumes them -- entry c * 8 + r belongs to
// row r of column c, as kQuantMul is laid out -- 128 bytes a frame.
struct NrPlan { uint64_t sums, offsets, bytes; };
AMV_HD inline NrPlan nr_plan(uint32_t n) {
    NrPlan p;
    p.sums = 0u;
    p.offsets = (uint64_t)n * 256u;
    p.bytes = p.offsets + (uint64_t)n * 128u;
    return p;
}
AMV_HD inline uint32_t nr_consumed_index(uint32_t i) { return (i & 7u) * 8u + (i >> 3); }   // position i = r * 8 + c -> c * 8 + r

}  // namespace amv
