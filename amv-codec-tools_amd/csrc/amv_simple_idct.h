// amv_simple_idct.h -- simple_idct_put (libavcodec/simple_idct.c:78-181,183-247,390-398) a block per lane, in registers:
// what the FFmpeg-compat back half of the decoder (amv_reconstruct_ff.hip) and the encoder's own error measurement
// (amv_encode_error.hip; the reference encoder's idct_put is this routine too) both run.
// DCTELEM is int16 in the reference: every value that it stores into a block is wrapped to 16 bits here too, and the
// DC-only shortcut of idctRowCondDC -- which is NOT the general row formula (8*dc against (16383*dc + 1024) >> 11) -- is
// taken per row by a select.
#pragma once
#include "amv_ff_dequant.h"

namespace amv {

// idctRowCondDC, simple_idct.c:78-181
__device__ __forceinline__ void sidct_row(int& r0, int& r1, int& r2, int& r3, int& r4, int& r5, int& r6, int& r7) {
    constexpr int W1 = 22725, W2 = 21407, W3 = 19266, W4 = 16383, W5 = 12873, W6 = 8867, W7 = 4520;
    const bool dc_only = (r1 | r2 | r3 | r4 | r5 | r6 | r7) == 0;
    const int flat = s16(r0 << 3);                                  // :107-117
    int a0 = W4 * r0 + (1 << 10), a1 = a0, a2 = a0, a3 = a0;
    a0 += W2 * r2; a1 += W6 * r2; a2 -= W6 * r2; a3 -= W2 * r2;
    int b0 = W1 * r1 + W3 * r3, b1 = W3 * r1 - W7 * r3, b2 = W5 * r1 - W1 * r3, b3 = W7 * r1 - W5 * r3;
    a0 += W4 * r4 + W6 * r6; a1 += -W4 * r4 - W2 * r6; a2 += -W4 * r4 + W2 * r6; a3 += W4 * r4 - W6 * r6;
    b0 += W5 * r5 + W7 * r7; b1 += -W1 * r5 - W5 * r7; b2 += W7 * r5 + W3 * r7; b3 += W3 * r5 - W1 * r7;
    r0 = dc_only ? flat : s16((a0 + b0) >> 11);
    r7 = dc_only ? flat : s16((a0 - b0) >> 11);
    r1 = dc_only ? flat : s16((a1 + b1) >> 11);
    r6 = dc_only ? flat : s16((a1 - b1) >> 11);
    r2 = dc_only ? flat : s16((a2 + b2) >> 11);
    r5 = dc_only ? flat : s16((a2 - b2) >> 11);
    r3 = dc_only ? flat : s16((a3 + b3) >> 11);
    r4 = dc_only ? flat : s16((a3 - b3) >> 11);
}

// idctSparseColPut, simple_idct.c:183-247 (its `if (col[..])` guards only skip additions of zero); the clip is
// ff_cropTbl (0..255 over -1024..1279)
__device__ __forceinline__ void sidct_col(int& c0, int& c1, int& c2, int& c3, int& c4, int& c5, int& c6, int& c7) {
    constexpr int W1 = 22725, W2 = 21407, W3 = 19266, W4 = 16383, W5 = 12873, W6 = 8867, W7 = 4520;
    int a0 = W4 * (c0 + 32), a1 = a0, a2 = a0, a3 = a0;              // (1 << 19) / W4 = 32
    a0 += W2 * c2; a1 += W6 * c2; a2 -= W6 * c2; a3 -= W2 * c2;
    int b0 = W1 * c1 + W3 * c3, b1 = W3 * c1 - W7 * c3, b2 = W5 * c1 - W1 * c3, b3 = W7 * c1 - W5 * c3;
    a0 += W4 * c4; a1 -= W4 * c4; a2 -= W4 * c4; a3 += W4 * c4;
    b0 += W5 * c5; b1 -= W1 * c5; b2 += W7 * c5; b3 += W3 * c5;
    a0 += W6 * c6; a1 -= W2 * c6; a2 += W2 * c6; a3 -= W6 * c6;
    b0 += W7 * c7; b1 -= W5 * c7; b2 += W3 * c7; b3 -= W1 * c7;
    c0 = crop((a0 + b0) >> 20); c1 = crop((a1 + b1) >> 20); c2 = crop((a2 + b2) >> 20); c3 = crop((a3 + b3) >> 20);
    c4 = crop((a3 - b3) >> 20); c5 = crop((a2 - b2) >> 20); c6 = crop((a1 - b1) >> 20); c7 = crop((a0 - b0) >> 20);
}

}  // namespace amv
