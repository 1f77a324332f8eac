// amv_picture_sse.hip -- picture against picture: per frame, the squared error between two pictures of one format, summed
// per plane (planar YUV, GRAY8) or per byte of the pixel (RGB24 / BGR24).  What `ffmpeg -psnr` reports is made of such
// sums (mpegvideo_enc.c:2590-2606, ffmpeg.c:849-852,953-972); here it is a tool of its own: a source against what a
// decoder shows for it.
//
//   amv_picture_sse_kernel   a workgroup per tile of kSseTileBytes x kSseTileRows bytes of one plane of one frame (a
//                            packed RGB plane is a plane of 3 * width bytes whose byte x belongs to entry x % 3); a lane
//                            walks its columns down the tile's rows -- only a row's own bytes, never the pitch's rest --
//                            with up to three 32-bit sums (64 squares of at most 255^2 each), the workgroup adds them up
//                            (at most 2^14 squares: inside 32 bits) and three lanes add into sse[frame][entry] by
//                            64-bit atomic adds.  Integer sums: the order of the adds does not matter.
#include "amv_kernels.h"
#include "amv_wave.h"

namespace amv {

namespace {

constexpr uint32_t kSseThreads = 256, kSseWaves = kSseThreads / kWave;
constexpr uint32_t kSseTileBytes = 4 * kSseThreads, kSseTileRows = 16;

}  // namespace

__global__ __launch_bounds__(kSseThreads) void amv_picture_sse_kernel(SseJobs jobs, uint32_t frame0, unsigned long long* __restrict__ sse) {
    __shared__ uint32_t s_part[kSseWaves][3];
    uint32_t tile = blockIdx.x, p = 0;
    while (p + 1u < jobs.count && tile >= jobs.j[p].tiles) { tile -= jobs.j[p].tiles; ++p; }
    const SsePlane& job = jobs.j[p];
    if (tile >= job.tiles) return;
    const uint32_t frame = frame0 + blockIdx.y;
    const uint32_t ty = tile / job.tiles_x, tx = tile - ty * job.tiles_x;
    const uint32_t row0 = ty * kSseTileRows, rows = min(kSseTileRows, job.rows - row0);
    const uint8_t* a = job.a + (uint64_t)frame * job.aframe + (uint64_t)row0 * job.astride;
    const uint8_t* b = job.b + (uint64_t)frame * job.bframe + (uint64_t)row0 * job.bstride;
    uint32_t acc[3] = {0u, 0u, 0u};
#pragma unroll
    for (uint32_t k = 0; k < kSseTileBytes / kSseThreads; ++k) {
        const uint32_t x = tx * kSseTileBytes + k * kSseThreads + threadIdx.x;
        if (x >= job.row_bytes) break;
        const uint32_t e = job.interleave == 3u ? x % 3u : 0u;
        uint32_t sum = 0u;
        for (uint32_t r = 0; r < rows; ++r) {
            const int d = (int)a[(uint64_t)r * job.astride + x] - (int)b[(uint64_t)r * job.bstride + x];
            sum += (uint32_t)(d * d);
        }
        acc[0] += e == 0u ? sum : 0u;
        acc[1] += e == 1u ? sum : 0u;
        acc[2] += e == 2u ? sum : 0u;
    }
    const uint32_t wave = threadIdx.x / kWave;
#pragma unroll
    for (uint32_t e = 0; e < 3; ++e) {
        const uint32_t s = wave_sum(acc[e]);
        if (threadIdx.x % kWave == 0u) s_part[wave][e] = s;
    }
    __syncthreads();
    if (threadIdx.x < 3u) {
        uint32_t s = 0u;
        for (uint32_t w = 0; w < kSseWaves; ++w) s += s_part[w][threadIdx.x];
        // a plane's own sum is in acc[0]: entry job.entry; a packed plane's three are entries 0, 1, 2
        const uint32_t e = job.interleave == 3u ? threadIdx.x : job.entry;
        if (s) atomicAdd(sse + (uint64_t)frame * 3u + e, (unsigned long long)s);
    }
}

void launch_picture_sse(SseJobs jobs, uint32_t n, uint64_t* sse, hipStream_t s) {
    uint32_t tiles = 0;
    for (uint32_t p = 0; p < jobs.count; ++p) {
        SsePlane& j = jobs.j[p];
        j.tiles_x = (j.row_bytes + kSseTileBytes - 1u) / kSseTileBytes;
        j.tiles = j.tiles_x * ((j.rows + kSseTileRows - 1u) / kSseTileRows);
        tiles += j.tiles;
    }
    if (!tiles) return;
    for (uint32_t base = 0; base < n; base += 65535u)
        hipLaunchKernelGGL(amv_picture_sse_kernel, dim3(tiles, n - base < 65535u ? n - base : 65535u), dim3(kSseThreads), 0, s, jobs, base,
                           reinterpret_cast<unsigned long long*>(sse));
}

}  // namespace amv
