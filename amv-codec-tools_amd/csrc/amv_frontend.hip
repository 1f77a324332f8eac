// amv_frontend.hip -- the two pixel stages of ffmpeg's video front end that are not the shim's: -deinterlace
// (avpicture_deinterlace, AMVmuxer/ffmpeg/libavcodec/imgconvert.c:2673-2864, the C branch) in front of everything else
// (pre_process_video_frame, ffmpeg.c:579-623) and the bands of av_picture_pad (imgconvert.c:2246-2304) behind the rescaler
// (do_video_out, ffmpeg.c:730-765).
//
//   amv_deinterlace_kernel  per plane: even rows copied, odd row 2k + 1 = cm[(-r[2k-1] + 4 r[2k] + 2 r[2k+1] + 4 r[2k+2]
//                           - r[2k+3] + 4) >> 3]; r[-1] is row 0, and below the last row stands the last row itself
//                           (deinterlace_bottom_field :2765-2792).  Out of place, and only over a WINDOW of the plane:
//                           the rows and columns a crop behind it keeps.  A row's parity and the first / last row rules
//                           come from its index in the full plane, so deinterlace-then-crop costs the kept area and needs
//                           no full-size picture in between.
//   amv_pad_bands_kernel    the band bytes of the three planes of a padded picture and nothing else: it never touches the
//                           window, so it is independent of the rescaler's stores into it.
//
// A lane makes four bytes of one row: dwords where the addresses allow (pointer and pitch multiples of 4, a whole group),
// single bytes otherwise (odd pitches, chroma widths such as 18, windows that start at column 2) -- no byte beyond a row's
// width and no row beyond the height is read or written.
#include "amv_host_plan.h"
#include "amv_kernels.h"

namespace amv {

namespace {

__device__ __forceinline__ int byte_at(uint32_t w, int k) { return (int)((w >> (8 * k)) & 255u); }

// four bytes (`valid` of them exist) of row y of a plane whose column group starts at s
__device__ __forceinline__ uint32_t load4(const uint8_t* s, uint32_t stride, uint32_t y, int valid, bool wide) {
    const uint8_t* p = s + (uint64_t)y * stride;
    if (wide) return *(const uint32_t*)p;
    uint32_t v = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b)
        if (b < valid) v |= (uint32_t)p[b] << (8 * b);
    return v;
}

__device__ __forceinline__ void store4(uint8_t* d, uint32_t v, int valid) {
    if (valid == 4 && ((uintptr_t)d & 3u) == 0) {
        *(uint32_t*)d = v;
        return;
    }
#pragma unroll
    for (int b = 0; b < 4; ++b)
        if (b < valid) d[b] = (uint8_t)(v >> (8 * b));
}

}  // namespace

__global__ __launch_bounds__(256) void amv_deinterlace_kernel(DeintJobs jobs, uint32_t frame_base) {
    const DeintPlane& j = jobs.j[blockIdx.y];
    const uint32_t groups = (j.w + 3u) >> 2, t = blockIdx.x * 256u + threadIdx.x;
    if (t >= groups * j.h) return;
    const uint32_t r = t / groups, c = (t - r * groups) << 2;
    const int valid = (int)min(4u, j.w - c);
    const uint64_t frame = frame_base + blockIdx.z;
    const uint8_t* s = j.src + frame * j.sframe + j.x0 + c;
    const bool wide = valid == 4 && ((((uintptr_t)s) | j.sstride) & 3u) == 0;
    const uint32_t row = j.y0 + r, last = j.full_h - 1u;          // the row's index in the full plane
    uint32_t o;
    if (!(row & 1u)) {
        o = load4(s, j.sstride, row, valid, wide);
    } else {
        const uint32_t m2 = load4(s, j.sstride, row >= 2u ? row - 2u : row - 1u, valid, wide);   // src_m2 = src_m1 = src1 at the top
        const uint32_t m1 = load4(s, j.sstride, row - 1u, valid, wide);
        const uint32_t s0 = load4(s, j.sstride, row, valid, wide);
        uint32_t p1 = s0, p2 = s0;                                                              // the last line: src_0 three times
        if (row < last) {
            p1 = load4(s, j.sstride, row + 1u, valid, wide);
            p2 = load4(s, j.sstride, min(row + 2u, last), valid, wide);
        }
        uint32_t q[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int sum = -byte_at(m2, b) + 4 * byte_at(m1, b) + 2 * byte_at(s0, b) + 4 * byte_at(p1, b) - byte_at(p2, b);
            q[b] = (uint32_t)min(max((sum + 4) >> 3, 0), 255);
        }
        // packed by byte permutes, as amv_pixfmt.hip packs: written as shifts and ORs, the compiler fuses shift, clamp and pack of
        // two bytes into one instruction that leaves the upper half of its result as it was -- 0xffff behind a negative sum
        const uint32_t lo = __builtin_amdgcn_perm(q[1], q[0], 0x0c0c0400u), hi = __builtin_amdgcn_perm(q[3], q[2], 0x0c0c0400u);
        o = __builtin_amdgcn_perm(hi, lo, 0x05040100u);
    }
    store4(j.dst + frame * j.dframe + (uint64_t)r * j.dstride + c, o, valid);
}

__global__ __launch_bounds__(256) void amv_pad_bands_kernel(PadBandJobs jobs, uint32_t frame_base) {
    const PadBandPlane& j = jobs.j[blockIdx.y];
    const PadPlane q{j.W, j.H, j.wx, j.wy, j.ww, j.wh, j.color};
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= pad_items(q)) return;
    const PadItem it = pad_item(q, t);
    store4(j.dst + (uint64_t)(frame_base + blockIdx.z) * j.frame + (uint64_t)it.row * j.stride + it.col, j.color, (int)it.len);
}

namespace {
constexpr uint32_t kFramesPerLaunch = 65535u;
}

void launch_deinterlace(const DeintJobs& jobs, uint32_t n, hipStream_t s) {
    uint32_t blocks = 0;
    for (uint32_t p = 0; p < jobs.count; ++p) {
        const uint32_t b = (((jobs.j[p].w + 3u) >> 2) * jobs.j[p].h + 255u) / 256u;
        blocks = b > blocks ? b : blocks;
    }
    if (!blocks) return;
    for (uint32_t base = 0; base < n; base += kFramesPerLaunch)
        hipLaunchKernelGGL(amv_deinterlace_kernel, dim3(blocks, jobs.count, n - base < kFramesPerLaunch ? n - base : kFramesPerLaunch), dim3(256),
                           0, s, jobs, base);
}

void launch_pad_bands(const PadBandJobs& jobs, uint32_t n, hipStream_t s) {
    uint32_t blocks = 0;
    for (uint32_t p = 0; p < 3; ++p) {
        const PadBandPlane& j = jobs.j[p];
        const uint32_t b = (pad_items(PadPlane{j.W, j.H, j.wx, j.wy, j.ww, j.wh, j.color}) + 255u) / 256u;
        blocks = b > blocks ? b : blocks;
    }
    if (!blocks) return;
    for (uint32_t base = 0; base < n; base += kFramesPerLaunch)
        hipLaunchKernelGGL(amv_pad_bands_kernel, dim3(blocks, 3, n - base < kFramesPerLaunch ? n - base : kFramesPerLaunch), dim3(256), 0, s,
                           jobs, base);
}

}  // namespace amv
