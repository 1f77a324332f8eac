// amv_encode_qns.hip -- the encoder's quantizer noise shaping (`ffmpeg -qns`): between amv_forward_kernel and amv_pack_kernel,
// every block's levels are refined in place in the round's dense lines, one +-1 change at a time, each the one that lowers
// the visually weighted error of the reconstruction plus lambda * bits the most.  The arithmetic is amv_qns_plan.h's
// (dct_quantize_refine, mpegvideo_enc.c:3271-3645, against AMV's reconstruction and AMV's fixed AC code); qns_block there is
// the same walk in serial form, and tests/qns_ref.py the model both are held to.
//
//   amv_qns_refine_kernel   a workgroup of kQnsWaves waves per MCU-row segment, as amv_encode_error_kernel places them: wave
//                           0 rebuilds the segment's planes in LDS (stage 1 of the encoder), then a wave takes one block at
//                           a time, lane = scan position (lane 0: the DC).  Per workgroup, once: the basis in LDS,
//                           transposed to [sample][scan position] with a pitch of 66 int16 -- the 64 lanes of a scoring step
//                           read consecutive int16 of one row, and the lanes of a remainder update (lane = sample, one
//                           coefficient) read rows 33 dwords apart, a bank each -- and the AC length tables beside it.  Per
//                           wave: rem and w of the 64 samples as one dword each, read as broadcasts by the scoring loop,
//                           and the 64 words d1's fdct runs in.
//                           An iteration: the non-zero mask is a ballot, a lane's previous and next non-zero positions are
//                           bit scans of it; when the gradient rule applies, lanes 0 .. 7 run the fdct's eight rows and then
//                           its eight columns; every lane sums the 64 terms of its two candidates (and of the unchanged
//                           block: best_score) and adds the rate; the argmin is a wave reduction over (score, candidate
//                           order), so the earliest candidate wins a tie as the serial strict `<` has it; the winner's
//                           lane changes its level, every lane (as a sample) moves its rem.  At most kQnsIterations
//                           iterations.  Every LDS index is made of the lane, the wave and constants; the line's address of
//                           the slot, the segment and the block (< cnt * 6), all inside the round's workspace.
#include "amv_encode_common.h"
#include "amv_qns_plan.h"
#include "amv_wave.h"

namespace amv {

using namespace enc;

constexpr uint32_t kQnsWaves = 4;
constexpr uint32_t kQnsBasisPitch = 66;          // int16 per sample row: 33 dwords, so rows start a bank apart
__device__ const QnsScan kQnsScanTab = make_qns_scan();

__device__ __forceinline__ long long wave_min(long long v) {
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) {
        const long long o = __shfl_xor(v, d, kWave);
        v = o < v ? o : v;
    }
    return v;
}

template <bool kYuv>
__global__ __launch_bounds__(kWave * kQnsWaves) void amv_qns_refine_kernel(Source in, uint32_t n, FrameSel sel, FrameGeom g, uint32_t nseg,
                                                                           uint32_t per_seg, int16_t* __restrict__ coef,
                                                                           const int16_t* __restrict__ basis_t, uint32_t qns, uint32_t lambda2) {
    __shared__ __attribute__((aligned(16))) int16_t s_planes[kPlaneSamples];
    __shared__ int16_t s_basis[64 * kQnsBasisPitch];
    __shared__ uint8_t s_len[2][256];
    __shared__ uint32_t s_rw[kQnsWaves][64];     // rem (low half, int16) and w (high half) per sample
    __shared__ int32_t s_d[kQnsWaves][64];
    int16_t* const s_y = s_planes;
    int16_t* const s_cb = s_planes + 16 * kPitchY;
    int16_t* const s_cr = s_cb + 8 * kPitchC;

    const uint32_t tid = threadIdx.x, lane = tid & (kWave - 1u), wave = tid / kWave;
    const uint32_t segs = g.mcu_rows * nseg;
    uint32_t my, m0, cnt;
    if (!seg_place(SegSplit{nseg, per_seg}, g, blockIdx.x % segs, my, m0, cnt)) return;
    for (uint32_t i = tid; i < 64u * 64u; i += kWave * kQnsWaves) s_basis[(i >> 6) * kQnsBasisPitch + (i & 63u)] = basis_t[i];
    for (uint32_t i = tid; i < 512u; i += kWave * kQnsWaves) (&s_len[0][0])[i] = (&kTrellisTab.len[0][0])[i];
    const uint32_t nb = cnt * 6u;
    uint32_t* const rw = s_rw[wave];
    int32_t* const sd = s_d[wave];
    const uint32_t nat = kQnsScanTab.natural[lane];
    const uint32_t sx = lane & 7u, sy = lane >> 3;

    const uint32_t first = blockIdx.x / segs, stride = gridDim.x / segs;
    const uint32_t items = sel_items(sel, n);
    for (uint32_t slot = first; slot < items; slot += stride) {
        const uint32_t f = sel_frame(sel, slot);
        if (wave == 0u) convert_segment<kYuv>(in, f, g, my, m0, cnt, lane, s_y, s_cb, s_cr);
        __syncthreads();                        // the planes (and, the first time, the tables) are there
        for (uint32_t b = wave; b < nb; b += kQnsWaves) {
            const uint32_t m = b / 6u, k6 = b - 6u * m;
            const bool chroma = k6 >= 4u;
            const uint32_t comp = chroma ? 1u : 0u;
            const int16_t* const src = chroma ? (k6 == 4u ? s_cb : s_cr) + m * 8u : s_y + ((k6 >> 1) * 8u) * kPitchY + m * 16u + (k6 & 1u) * 8u;
            const uint32_t pitch = chroma ? kPitchC : kPitchY;
            const uint8_t* const len = s_len[comp];
            int16_t* const line = coef + ((uint64_t)slot * g.mcus + (uint64_t)my * g.mcu_cols + m0) * 384u + b * 64u;
            const int32_t lev0 = line[lane];
            int32_t lev = lev0;
            const int32_t q = kTrellisTab.q[comp][lane];
            // the lane as a sample: its weight (the planes hold samples - 128, which the variance does not see) and remainder
            const int32_t w = qns_weight_at([&](int32_t at) { return (int32_t)src[(uint32_t)(at >> 3) * pitch + (uint32_t)(at & 7)]; }, (int32_t)sx, (int32_t)sy);
            const int32_t lambda = qns_lambda(wave_sum((uint32_t)(w * w)), lambda2);
            int32_t rem = qns_rem_start(__shfl(lev, 0, kWave), __shfl(q, 0, kWave), (int32_t)src[sy * pitch + sx]);
            const int32_t levq = lev * q;
            for (uint64_t mm = __ballot(lev != 0 && lane != 0u); mm; mm &= mm - 1u) {
                const uint32_t i = (uint32_t)__builtin_ctzll(mm);
                rem = qns_rem_add(rem, s_basis[lane * kQnsBasisPitch + i], __shfl(levq, (int)i, kWave));
            }
            wave_sync();                         // (the block before this one is done with the wave's words)
            rw[lane] = ((uint32_t)rem & 0xffffu) | ((uint32_t)w << 16);
            wave_sync();
            for (uint32_t changes = 0; changes < kQnsIterations; ++changes) {
                const uint64_t mask = __ballot(lev != 0 && lane != 0u);
                const uint32_t last = mask ? 63u - (uint32_t)__builtin_clzll(mask) : 0u;
                const bool gradient = last > 2u || qns >= 3u;
                int32_t gr = 0;
                if (gradient) {                  // (the same in every lane)
                    sd[lane] = qns_gradient_in(rem, w);
                    wave_sync();
                    if (lane < 8u) qns_fdct_pass(sd + 8u * lane, 1, true);
                    wave_sync();
                    if (lane < 8u) qns_fdct_pass(sd + lane, 8, false);
                    wave_sync();
                    gr = sd[nat];
                    wave_sync();
                }
                // the lane as a scan position: the unchanged block's sum and its two candidates'
                uint32_t sum0 = 0u, sum_minus = 0u, sum_plus = 0u;
#pragma unroll 8
                for (uint32_t k = 0; k < 64u; ++k) {
                    const uint32_t v = rw[k];
                    const int32_t r = (int32_t)(int16_t)(v & 0xffffu), ww = (int32_t)(v >> 16);
                    const int32_t bs = s_basis[k * kQnsBasisPitch + lane];
                    sum0 += qns_term(r, ww, 0);
                    sum_minus += qns_term(r, ww, qns_basis_step(bs, -q));
                    sum_plus += qns_term(r, ww, qns_basis_step(bs, q));
                }
                const int32_t base = (int32_t)(sum0 >> 2);
                const uint64_t lo = mask & ((1ull << lane) - 1ull), hi = lane < 63u ? mask >> (lane + 1u) : 0ull;
                const uint32_t prev = lo ? 63u - (uint32_t)__builtin_clzll(lo) : 0u;
                const uint32_t next = hi ? lane + 1u + (uint32_t)__builtin_ctzll(hi) : 0u;
                const uint32_t a_lev = (uint32_t)(lev < 0 ? -lev : lev);
                const uint32_t a_next = (uint32_t)__shfl((int)a_lev, (int)next, kWave);
                const bool reached = qns >= 3u || lane <= last + 1u;
                long long key = 0x7fffffffffffffffll;
#pragma unroll
                for (int32_t change = 1; change >= -1; change -= 2) {      // (the smaller key wins, whichever comes first here)
                    const int32_t nl = lev + change;
                    const bool ok = lane == 0u ? qns_dc_allowed(nl, q) : reached && qns_ac_allowed(lev, change, q, qns, gradient ? gr : 0);
                    int32_t score = (int32_t)((change < 0 ? sum_minus : sum_plus) >> 2);
                    if (ok && lane != 0u) {
                        const uint32_t a_new = (uint32_t)(nl < 0 ? -nl : nl);
                        score += (qns_local_bits(len, lane, prev, next, a_next, a_new) - qns_local_bits(len, lane, prev, next, a_next, a_lev)) * lambda;
                    }
                    const long long mine = (long long)score * 256ll + (long long)(2u * lane + (change > 0 ? 1u : 0u));
                    if (ok && mine < key) key = mine;
                }
                key = wave_min(key);
                if (key == 0x7fffffffffffffffll || (int32_t)(key >> 8) >= base) break;
                const uint32_t at = ((uint32_t)key & 255u) >> 1;
                const int32_t change = ((uint32_t)key & 1u) ? 1 : -1;
                if (lane == at) lev += change;
                rem = qns_rem_add(rem, s_basis[lane * kQnsBasisPitch + at], change * __shfl(q, (int)at, kWave));
                wave_sync();                     // every lane has read the old remainders
                rw[lane] = ((uint32_t)rem & 0xffffu) | ((uint32_t)w << 16);
                wave_sync();
            }
            if (lev != lev0) line[lane] = (int16_t)lev;
        }
        __syncthreads();                        // the planes are free again
    }
}

void launch_qns_refine(const Source& in, uint32_t n, const FrameSel& sel, uint32_t items, const FrameGeom& g, int16_t* coef, const int16_t* basis_t,
                       uint32_t qns, uint32_t lambda2, hipStream_t s) {
    if (items == 0) return;
    const SegSplit sp = seg_split(g);
    const uint64_t grid = (uint64_t)(sel.round && items > 64u ? 64u : items) * g.mcu_rows * sp.nseg;
    with_source_kind(in, [&](auto yuv) {
        hipLaunchKernelGGL((amv_qns_refine_kernel<decltype(yuv)::value>), dim3((uint32_t)grid), dim3(kWave * kQnsWaves), 0, s, in, n, sel, g, sp.nseg,
                           sp.per_seg, coef, basis_t, qns, lambda2);
    });
}

}  // namespace amv
