// amv_ff_dequant.h -- what the FFmpeg-compat back halves (amv_reconstruct_ff.hip, amv_reconstruct_lowres.hip) share around
// their inverse transforms: which block a lane has and whether it counts as decoded, the "Q60" dequantisation, the clip.
#pragma once
#include "amv_block_load.h"
namespace amv {
// DCTELEM is int16 in the reference: every value it stores into a block is wrapped to 16 bits
__device__ __forceinline__ int s16(int x) { return (int)(int16_t)x; }

// ff_cropTbl: 0..255 (saturation beyond the table too, where the reference reads outside it).  Written as an explicit
// v_med3: hipcc 7.2 folds pairs of `clamp(x >> 20, 0, 255)` into gfx950's v_ashr_pk_u8_i32, whose results differed from
// the plain arithmetic on MI355X in the parity tests.
__device__ __forceinline__ int crop(int x) {
    int d;
    asm("v_med3_i32 %0, %1, 0, %2" : "=v"(d) : "v"(x), "s"(255));
    return d;
}
// The block of lane `lane` (< sg.cnt * 6): block k6 of the segment's MCU m, blocks 4 and 5 being Cb and Cr.
// decoded: it belongs to an MCU before the frame's first error -- or, AMVHIP_FLAG_FFMPEG_KEEP (SyncSinks::ok_in_blocks: ok
// counts blocks then), it is a whole block before it: what mjpeg_decode_scan has put into the picture when decode_block
// fails (mjpegdec.c:699-716).
struct FfBlock { uint32_t m, k6; bool chroma, decoded; };
__device__ __forceinline__ FfBlock ff_block(const SyncSinks& in, const Segment& sg, uint32_t lane) {
    const uint32_t m = lane / 6u, k6 = lane % 6u;
    return FfBlock{m, k6, k6 >= 4u, in.ok_in_blocks ? (sg.mcu0 + m) * 6u + k6 < sg.ok : sg.mcu0 + m < sg.ok};
}
// decode_block's dequantisation (mjpegdec.c:388-390,417,424) of the block's top-left kN x kN coefficients, natural order,
// row-major with pitch kN: v = (DCTELEM)(level * q).  The DC arrives as the running sum of differences, FFmpeg keeps
// 1024 + q0 * that sum (:805, last_dc = 1024) -- equal modulo 2^16, which is all an int16 store keeps.
template <int kN>
__device__ __forceinline__ void q60_dequantise(const uint32_t (&c)[32], bool chroma, int (&v)[kN * kN]) {
#pragma unroll
    for (int i = 0; i < kN * kN; ++i) {
        const int nat = 8 * (i / kN) + i % kN, scan = kScanOfNatural[nat];
        const int step = chroma ? (int)kQ60Chroma[scan] : (int)kQ60Luma[scan];
        v[i] = s16(coef_at(c, scan) * step + (nat == 0 ? 1024 : 0));
    }
}
}  // namespace amv
