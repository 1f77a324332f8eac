// amv_postprocess.hip -- the reference's decode-side postprocessing (AMVmuxer/ffmpeg/libpostproc, pp_postprocess: the hb, vb
// and dr filters of its C path) on planes whose pitch is their width.  The arithmetic and the reasons for the order are in
// amv_pp_plan.h; pp_plane_rolling there is this kernel on the host, phase for phase.
//
//   amv_postprocess_kernel   a workgroup of one wave per plane of a frame (grid: 3 planes x frames).  The plane moves through
//                            a ring of 16 lines in LDS (lines y-1 .. y+12 of strip y: the extent the reference's loop
//                            touches).  Per strip of 8 lines: the fresh lines come in (behind the plane's end: what the
//                            reference's tempSrc / tempDst hold there); vertical deblock, a lane per column, the eight lanes of
//                            a block adding their classification counts through LDS; horizontal deblock, a lane per line of
//                            an edge, in three steps -- classify, publish the edge's last column as it will leave it (it
//                            does not depend on the edge before), filter with the edge before's published column as the
//                            first tap; dering, the ranges of all calls first, then the calls one behind the other (a call's
//                            sign masks need the call before's last column), each a wavefront of skew 2 over its 8 x 8
//                            pixels, a lane per line, 22 steps (a plane 8 columns wide, whose one call's window folds onto
//                            itself, runs it in raster order on one lane: pp_dering_serial); the strip's 8 lines go out.
//                            A plane whose mode is 0 is copied.  Everything is synchronised by the workgroup's barrier; no
//                            kernel waits on another workgroup, and every loop's trip count is fixed by the geometry.
//                            Global traffic is 4 bytes a lane: planes and frame pitches are 4-byte aligned (the entry checks).
#include "amv_kernels.h"
#include "amv_pp_plan.h"

namespace amv {

namespace {

constexpr uint32_t kPpThreads = 64;

__device__ inline void pp_line_in(uint8_t* ring, int r, const uint8_t* src, int line, int w, uint32_t lane) {
    uint32_t* d = reinterpret_cast<uint32_t*>(ring + pp_ring_at(r, 0, w));
    const uint32_t* s = reinterpret_cast<const uint32_t*>(src + (size_t)line * w);
    for (uint32_t i = lane; i < (uint32_t)w / 4u; i += kPpThreads) d[i] = s[i];
}

}  // namespace

__global__ __launch_bounds__(kPpThreads) void amv_postprocess_kernel(PpJobs jobs, uint32_t frame0) {
    __shared__ __attribute__((aligned(16))) uint8_t s_ring[kPpRing * kPpMaxWidth];
    __shared__ uint8_t s_new7[kPpMaxWidth];
    __shared__ uint32_t s_stat[kPpThreads];
    __shared__ uint8_t s_mn[kPpMaxWidth / 8], s_mx[kPpMaxWidth / 8];
    __shared__ uint32_t s_line[10];
    const PpPlaneJob& job = jobs.j[blockIdx.x];
    const uint32_t frame = frame0 + blockIdx.y, lane = threadIdx.x;
    const uint8_t* src = job.src + (uint64_t)frame * job.sframe;
    uint8_t* dst = job.dst + (uint64_t)frame * job.dframe;
    const int w = (int)job.w, h = (int)job.h;
    if (!job.mode) {
        const uint32_t* s = reinterpret_cast<const uint32_t*>(src);
        uint32_t* d = reinterpret_cast<uint32_t*>(dst);
        for (uint32_t i = lane; i < (uint32_t)(w * h) / 4u; i += kPpThreads) d[i] = s[i];
        return;
    }
    int qp = jobs.d_qp ? (int)jobs.d_qp[frame] : jobs.qp;
    qp = qp > 63 ? 63 : qp;
    const PpParams p = pp_params(job.mode, qp, jobs.base_dc_diff, jobs.flat_thr);
    const int ca = pp_copy_ahead(p.mode);
    for (int r = 0; r < ca; ++r) pp_line_in(s_ring, r, src, r, w, lane);
    __syncthreads();
    for (int y = 0; y < h; y += 8) {
        // the fresh lines
        if (y + 15 >= h)
            for (int r = h; r < y + ca; ++r) {
                uint32_t* d = reinterpret_cast<uint32_t*>(s_ring + pp_ring_at(r, 0, w));
                const uint32_t* s = reinterpret_cast<const uint32_t*>(s_ring + pp_ring_at(h - 1, 0, w));
                for (uint32_t i = lane; i < (uint32_t)w / 4u; i += kPpThreads) d[i] = s[i];
            }
        for (int i = ca; i < ca + 8; ++i) pp_line_in(s_ring, y + i, src, pp_fresh_source_line(y, i, h), w, lane);
        __syncthreads();
        // vertical deblock: a lane per column
        if ((p.mode & kPpVDeblock) && y + 8 < h) {
            for (int x0 = 0; x0 < w; x0 += (int)kPpThreads) {
                const int x = x0 + (int)lane;
                const bool active = x < w;
                int v[10];
                if (active) {
#pragma unroll
                    for (int i = 0; i < 10; ++i) v[i] = s_ring[pp_ring_at(y + 3 + i, x, w)];
                    s_stat[lane] = pp_stat(v, x & 3, p);
                }
                __syncthreads();
                if (active) {
                    uint32_t sum = 0;
#pragma unroll
                    for (int k = 0; k < 8; ++k) sum += s_stat[(lane & ~7u) + k];
                    const int t = pp_class(sum, p);
                    if (t == 1) {
                        int out[8];
                        pp_low_pass(v, p.qp, out);
#pragma unroll
                        for (int i = 0; i < 8; ++i) s_ring[pp_ring_at(y + 4 + i, x, w)] = (uint8_t)out[i];
                    } else if (t == 2) {
                        const int d = pp_def_delta(v, p.qp);
                        s_ring[pp_ring_at(y + 7, x, w)] = (uint8_t)(v[4] - d);
                        s_ring[pp_ring_at(y + 8, x, w)] = (uint8_t)(v[5] + d);
                    }
                }
                __syncthreads();
            }
        }
        // horizontal deblock: a lane per line of an edge; item k = (edge - 1) * 8 + line
        if (p.mode & kPpHDeblock) {
            const int items = w - 8;
            for (int k0 = 0; k0 < items; k0 += (int)kPpThreads) {
                const int k = k0 + (int)lane, x = (k >> 3) * 8 + 8, r = k & 7;
                const bool active = k < items;
                int v[10];
                if (active) {
#pragma unroll
                    for (int i = 0; i < 10; ++i) v[i] = s_ring[pp_ring_at(y + r, x - 5 + i, w)];
                    s_stat[lane] = pp_stat(v, r & 3, p);
                }
                __syncthreads();
                int t = 0;
                if (active) {
                    uint32_t sum = 0;
#pragma unroll
                    for (int j = 0; j < 8; ++j) sum += s_stat[(lane & ~7u) + j];
                    t = pp_class(sum, p);
                    int out[8];
                    pp_low_pass(v, p.qp, out);                   // out[7] does not depend on v[0]
                    s_new7[k] = (uint8_t)(t == 1 ? out[7] : v[8]);
                }
                __syncthreads();
                if (active) {
                    if (k >= 8) v[0] = s_new7[k - 8];            // the edge before's last column, as that edge leaves it
                    if (t == 1) {
                        int out[8];
                        pp_low_pass(v, p.qp, out);
#pragma unroll
                        for (int i = 0; i < 8; ++i) s_ring[pp_ring_at(y + r, x - 4 + i, w)] = (uint8_t)out[i];
                    } else if (t == 2) {
                        const int d = pp_def_delta(v, p.qp);
                        s_ring[pp_ring_at(y + r, x - 1, w)] = (uint8_t)(v[4] - d);
                        s_ring[pp_ring_at(y + r, x, w)] = (uint8_t)(v[5] + d);
                    }
                }
                __syncthreads();
            }
        }
        // dering: the ranges of all calls, then the calls one behind the other
        if ((p.mode & kPpDering) && y > 0) {
            const int calls = w / 8, qp2 = p.qp / 2 + 1;
            for (int b = (int)lane; b < calls; b += (int)kPpThreads) {
                int mn = 255, mx = 0;
                for (int k = 0; k < 64; ++k) {
                    const int v = s_ring[pp_ring_at(y + (k >> 3), b * 8 + 1 + (k & 7), w)];
                    mn = v < mn ? v : mn;
                    mx = v > mx ? v : mx;
                }
                s_mn[b] = (uint8_t)mn;
                s_mx[b] = (uint8_t)mx;
            }
            __syncthreads();
            for (int b = 0; b < calls; ++b) {
                const int mn = s_mn[b], mx = s_mx[b];
                if (mx - mn < kPpDeringThreshold) continue;      // the same for every lane
                const int avg = (mn + mx + 1) >> 1, x0 = b * 8;
                if (lane < 10u) {
                    int px[10];
#pragma unroll
                    for (int i = 0; i < 10; ++i) px[i] = s_ring[pp_ring_at(y - 1 + (int)lane, x0 + i, w)];
                    s_line[lane] = pp_dering_line_mask(px, avg);
                }
                __syncthreads();
                if (pp_dering_serial(w)) {                       // the window folds onto itself: raster order, one lane
                    if (lane == 0u)
                        for (int k = 0; k < 64; ++k) {
                            const int r = k >> 3, c = k & 7;
                            if (!(pp_dering_join(s_line[r], s_line[r + 1], s_line[r + 2]) >> (c + 1) & 1u)) continue;
                            int n[9];
#pragma unroll
                            for (int j = 0; j < 9; ++j) n[j] = s_ring[pp_ring_at(y + r - 1 + j / 3, x0 + c + j % 3, w)];
                            s_ring[pp_ring_at(y + r, x0 + 1 + c, w)] = (uint8_t)pp_dering_pixel(n, qp2);
                        }
                    __syncthreads();
                    continue;
                }
                const uint32_t mask = lane < 8u ? pp_dering_join(s_line[lane], s_line[lane + 1u], s_line[lane + 2u]) : 0u;
                for (int step = 0; step < 22; ++step) {
                    const int c = step - 2 * (int)lane;
                    int fresh = -1;
                    if (lane < 8u && c >= 0 && c <= 7 && (mask >> (c + 1) & 1u)) {
                        int n[9];
#pragma unroll
                        for (int j = 0; j < 9; ++j) n[j] = s_ring[pp_ring_at(y + (int)lane - 1 + j / 3, x0 + c + j % 3, w)];
                        fresh = pp_dering_pixel(n, qp2);
                    }
                    if (fresh >= 0) s_ring[pp_ring_at(y + (int)lane, x0 + 1 + c, w)] = (uint8_t)fresh;
                    __syncthreads();
                }
            }
        }
        for (int r = y; r < y + 8 && r < h; ++r) {
            const uint32_t* s = reinterpret_cast<const uint32_t*>(s_ring + pp_ring_at(r, 0, w));
            uint32_t* d = reinterpret_cast<uint32_t*>(dst + (size_t)r * w);
            for (uint32_t i = lane; i < (uint32_t)w / 4u; i += kPpThreads) d[i] = s[i];
        }
        __syncthreads();
    }
}

void launch_postprocess(const PpJobs& jobs, uint32_t n, hipStream_t s) {
    for (uint32_t base = 0; base < n; base += 65535u)
        hipLaunchKernelGGL(amv_postprocess_kernel, dim3(3, n - base < 65535u ? n - base : 65535u), dim3(kPpThreads), 0, s, jobs, base);
}

}  // namespace amv
