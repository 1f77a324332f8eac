// amv_audio_resample.hip -- the audio half of AMVmuxer/Makefile:16 (`-ac 1 -ar 22050`): audio_resample of the reference
// (AMVmuxer/ffmpeg/libavcodec/resample.c:129-242), a channel mix in front of av_resample (resample2.c:182-324) as the
// reference ships it: int16 filter bank (FILTER_SHIFT 15, Kaiser window beta 9), 1024 phases, sums in 32 bits that wrap.
//
// Output k of a stream sits at I_k = base + floor((frac0 + k * in_rate * 1024) / out_rate) -- the index / frac recurrence
// of :288-293 unrolled; filter row I_k & 1023, first input frame I_k >> 10.  Outputs with I_k < 0 (the first few of a
// stream) read the mirrored head src[|s + i| % src_size] (:263-265) straight from memory; every other output reads a span
// of frames that its workgroup staged in LDS (2 -> 1 mixed down (l + r) >> 1 on the way, :198-201), takes its taps as
// v_dot2_i32_i16 on sample pairs (a lane whose first frame is odd realigns the pairs with v_alignbit_b32), and rounds
// (val + 2^14) >> 15 with the saturation of :285.  The bank (1024 rows, built on the host as av_build_filter does,
// zero-padded to a multiple of 8 taps) is read through the caches as 16-byte row pieces: 80 KB at 44.1 kHz -> 22.05 kHz,
// 180 KB at 96 kHz, more than LDS holds beside the span at the larger ratios.
//
// One lane per output, a tile of up to 256 consecutive outputs of one stream per workgroup pass.  A one-workgroup scan
// (amv_audio_tiles_kernel) counts every stream's tiles; the resampling workgroups walk the tiles grid-stride and find
// their stream by binary search, so that a ragged batch needs no host round trip.
#include "amv_kernels.h"

namespace amv {

namespace {
constexpr uint32_t kBlock = 256, kScan = 1024;
typedef short v2i16 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int dot2(uint32_t x, uint32_t f, int acc) {   // v_dot2_i32_i16, no clamp: wraps like FELEM2 int32_t
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(v2i16, x), __builtin_bit_cast(v2i16, f), acc, false);
}

__device__ __forceinline__ int16_t round_clip(uint32_t acc) {
    const int v = (int)(acc + (1u << 14)) >> 15;                        // (val + (1 << 14)) >> 15 on the int32 sum
    return (int16_t)min(max(v, -32768), 32767);                        // (unsigned)(val + 32768) > 65535 ? (val >> 31) ^ 32767 : val
}

__device__ __forceinline__ uint64_t stream_outputs(const AudioResampleArgs& a, uint64_t src) {
    if (src == 0 || (src >> 32)) return 0;                              // empty streams, and 2^32 frames and more, make nothing
    const uint64_t c = audio_out_count(src, a.base, a.frac0, a.D, a.out_rate, a.fl);
    return c < a.cap ? c : a.cap;
}
}  // namespace

// tiles[i] = tiles of the streams before i, tiles[n] = all of them (one workgroup)
__global__ __launch_bounds__(kScan) void amv_audio_tiles_kernel(AudioResampleArgs a) {
    __shared__ uint32_t s[kScan];
    uint32_t carry = 0;
    for (uint32_t b = 0; b < a.n; b += kScan) {
        const uint32_t i = b + threadIdx.x;
        uint32_t v = 0;
        if (i < a.n) v = (uint32_t)((stream_outputs(a, a.nsamp[i]) + a.tile - 1) / a.tile);
        s[threadIdx.x] = v;
        __syncthreads();
        for (uint32_t d = 1; d < kScan; d <<= 1) {
            const uint32_t add = threadIdx.x >= d ? s[threadIdx.x - d] : 0u;
            __syncthreads();
            s[threadIdx.x] += add;
            __syncthreads();
        }
        if (i < a.n) a.tiles[i] = carry + s[threadIdx.x] - v;
        carry += s[kScan - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) a.tiles[a.n] = carry;
}

__global__ __launch_bounds__(kBlock) void amv_audio_resample_kernel(AudioResampleArgs a) {
    __shared__ __attribute__((aligned(16))) int16_t s_x[2][kAudioSpan + 64];
    const uint32_t total = a.tiles[a.n];
    const bool two = a.in_ch == 2 && a.out_ch == 2;                    // filter_channels (resample.c:152-157)
    const uint32_t dst_incr = (uint32_t)(a.D / a.out_rate), dst_frac = (uint32_t)(a.D % a.out_rate);
    const uint32_t j = threadIdx.x;
    for (uint32_t t = blockIdx.x; t < total; t += gridDim.x) {
        uint32_t lo = 0, hi = a.n;                                      // tiles[lo] <= t < tiles[hi]
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (a.tiles[mid] <= t) lo = mid; else hi = mid;
        }
        const uint32_t st = lo;
        const uint64_t src = a.nsamp[st];
        const uint64_t n_out = stream_outputs(a, src);
        const uint64_t k0 = (uint64_t)(t - a.tiles[st]) * a.tile;
        const uint64_t num = a.frac0 + k0 * a.D;
        const int64_t i0 = a.base + (int64_t)(num / a.out_rate);        // position of the tile's first output
        const uint32_t r0 = (uint32_t)(num % a.out_rate);
        const uint32_t last = (uint32_t)min((uint64_t)a.tile, n_out - k0) - 1;
        // r0 + j * dst_frac < 256 * out_rate < 2^26: the per-lane part of the position divides in 32 bits
        const int64_t i_last = i0 + (int64_t)last * dst_incr + (r0 + last * dst_frac) / a.out_rate;
        const int64_t s0 = i0 >= 0 ? (i0 >> 10) : 0;                  // first frame of the span
        const uint32_t span = i_last >= 0 ? (uint32_t)((i_last >> 10) - s0) + a.fl_pad + 2 : 0;
        const int16_t* in = a.pcm + a.pcm_offs[st];

        for (uint32_t f = j; f < span; f += kBlock) {                  // stage the span (zeros past the stream's end)
            const uint64_t fr = (uint64_t)s0 + f;
            int16_t l = 0, r = 0;
            if (fr < src) {
                if (a.in_ch == 2) { l = in[2 * fr]; r = in[2 * fr + 1]; } else { l = in[fr]; }
            }
            if (two) { s_x[0][f] = l; s_x[1][f] = r; }
            else s_x[0][f] = a.in_ch == 2 ? (int16_t)(((int)l + (int)r) >> 1) : l;
        }
        __syncthreads();

        const uint64_t k = k0 + j;
        if (j <= last) {
            const int64_t I = i0 + (int64_t)j * dst_incr + (r0 + j * dst_frac) / a.out_rate;
            const int16_t* row = a.bank + (size_t)(I & (kAudioPhases - 1)) * a.fl_pad;
            uint32_t acc0 = 0, acc1 = 0;
            if (I >= 0) {
                const uint32_t rel = (uint32_t)((I >> 10) - s0);
                const uint32_t sh = (rel & 1u) * 16u;
                const uint32_t* x0 = (const uint32_t*)s_x[0] + (rel >> 1);
                const uint32_t* x1 = (const uint32_t*)s_x[1] + (rel >> 1);
                const uint4* f4 = (const uint4*)row;
                uint32_t p0 = x0[0], p1 = two ? x1[0] : 0u;
                int a0 = 0, a1 = 0;
                for (uint32_t q = 0; q < a.fl_pad / 8; ++q) {
                    const uint4 f = f4[q];
                    const uint32_t fw[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const uint32_t n0 = x0[4 * q + e + 1];
                        a0 = dot2(__builtin_amdgcn_alignbit(n0, p0, sh), fw[e], a0);
                        p0 = n0;
                        if (two) {
                            const uint32_t n1 = x1[4 * q + e + 1];
                            a1 = dot2(__builtin_amdgcn_alignbit(n1, p1, sh), fw[e], a1);
                            p1 = n1;
                        }
                    }
                }
                acc0 = (uint32_t)a0;
                acc1 = (uint32_t)a1;
            } else {                                                    // the mirrored head: src[|s + i| % src_size]
                const int32_t s = (int32_t)(I >> 10);
                const uint32_t size = (uint32_t)src;
                for (uint32_t i = 0; i < a.fl; ++i) {
                    const int32_t v = s + (int32_t)i;
                    const uint32_t fr = (uint32_t)(v < 0 ? -v : v) % size;
                    const int32_t c = row[i];
                    if (a.in_ch == 1) {
                        acc0 += (uint32_t)((int32_t)in[fr] * c);
                    } else if (!two) {
                        acc0 += (uint32_t)((((int32_t)in[2 * fr] + (int32_t)in[2 * fr + 1]) >> 1) * c);
                    } else {
                        acc0 += (uint32_t)((int32_t)in[2 * fr] * c);
                        acc1 += (uint32_t)((int32_t)in[2 * fr + 1] * c);
                    }
                }
            }
            int16_t* o = a.out + a.out_offs[st];
            const int16_t v0 = round_clip(acc0);
            if (a.out_ch == 1) {
                o[k] = v0;
            } else {
                o[2 * k] = v0;
                o[2 * k + 1] = two ? round_clip(acc1) : v0;             // 1 -> 2 duplicates (mono_to_stereo, :221-222)
            }
        }
        __syncthreads();
    }
}

// outputs per tile: the span of a tile's inputs must fit the LDS span
uint32_t audio_resample_tile(uint32_t in_rate, uint32_t out_rate, uint32_t fl_pad) {
    const uint64_t room = kAudioSpan - fl_pad - 4;
    uint64_t t = room * out_rate / in_rate;
    if (t > kBlock) t = kBlock;
    return t ? (uint32_t)t : 1u;
}

void launch_audio_resample(const AudioResampleArgs& a, uint32_t blocks, hipStream_t s) {
    if (a.n == 0) return;
    hipLaunchKernelGGL(amv_audio_tiles_kernel, dim3(1), dim3(kScan), 0, s, a);
    hipLaunchKernelGGL(amv_audio_resample_kernel, dim3(blocks), dim3(kBlock), 0, s, a);
}

}  // namespace amv
