// amv_pp_plan.h -- the arithmetic of the reference's postprocessing (AMVmuxer/ffmpeg/libpostproc: postprocess.c and the C
// path of postprocess_template.c) for the hb, vb and dr filters, free of HIP: what the kernel of amv_postprocess.hip, the host
// entry's checks and tests/c/pp_plan_test.cc all run.
//
// Two walks of one plane are here.  pp_plane_serial is the reference's loop as it stands (postProcess_C :3349-3843): block by
// block, through tempSrc / tempDst where the plane ends.  pp_plane_rolling is the same function of the picture in the order the
// kernel computes it: a ring of 16 lines, per strip of 8 lines the fresh lines, the vertical deblock of all columns, the
// horizontal deblock of all edges, the dering blocks one behind the other.  The test asserts that they agree.
//
// What the kernel's order rests on (tests/pp_ref.py is the literal restatement; tests/golden/ref_postprocess.json pins it):
//   * With a forced quantiser (or none) pp_postprocess hands postProcess a QP table of stride 0, so its copy into nonBQPTable
//     has count 0 and the table stays as av_mallocz left it: nonBQP = 0, dcOffset = 1, dcThreshold = 3 whatever the QP and
//     whatever hb's / vb's first option (baseDcDiff) say.  Only flatnessThreshold and QP reach the classification.
//   * Vertical deblock of strip y decides on lines y+4 .. y+11 as copied, writes them, and reads lines y+3 and y+12 for the
//     low-pass's first / last taps alone.  Line y+3 is strip y-8's last output; that output does not depend on strip y-8's
//     own `first` (4 * first leaves the sums at sums[4]), so a column's strips depend on each other one deep.
//   * Horizontal deblock is the same turned on its side (writes columns x-4 .. x+3, taps x-5 and x+4) and sees only lines whose
//     vertical pass is complete; nothing the dering of the same strip writes (columns <= x) is read by a later edge.
//   * Dering is a recurrence: the call at block column X, strip y has the window lines y-1 .. y+8, columns X-8 .. X+1, updates
//     lines y .. y+7, columns X-7 .. X in place in raster order, and takes its range and sign masks from the window as it stands
//     when the call starts: line y+8 after V and before H, column X+1 after H and before its own dering, line y-1 and column
//     X-8 final.  The call behind the x loop has X = width: on a tight pitch columns width, width+1 are columns 0, 1 of the next
//     line.  The range of a call is taken over pixels no earlier call of the strip writes, so all ranges of a strip are known
//     before its first call; the masks are not (column X-8 is the call before's last column).
//   * Where the plane ends (y + 15 >= height) the loop works in tempDst on lines the plane does not have: copies of the last
//     source line from line max(height - y, 8) of the strip on, below that what tempSrc still holds from the strip before
//     (source lines y-8+i), and, with vb, copies of the destination's last line up to line 4.  They reach real pixels through
//     the dering's window, so the ring holds them as the reference's buffers do.
//   * Dering without vertical deblock copies one line ahead only, and its row-end window then reads a destination pixel no
//     one has written yet: the reference's output depends on what the destination held.  pp_mode_ok refuses that mode.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "amv_segment.h"

namespace amv {

constexpr int kPpVDeblock = 0x01, kPpHDeblock = 0x02, kPpDering = 0x04, kPpForceQuant = 0x200000;   // the reference's own bits
constexpr int kPpFilterBits = kPpVDeblock | kPpHDeblock | kPpDering;
constexpr int kPpDeringThreshold = 20;
constexpr int kPpRing = 16;                  // lines y-1 .. y+12 live at a time
constexpr uint32_t kPpMaxWidth = 1024, kPpMaxHeight = 1024;

struct PpParams {
    int mode;        // kPpFilterBits
    int qp;          // 0 .. 63
    int flat_thr;    // flatnessThreshold
    int dc_offset;   // ((nonBQP * baseDcDiff) >> 8) + 1 with nonBQP = 0: see above
};
AMV_HD inline PpParams pp_params(int mode, int qp, int base_dc_diff, int flat_thr) {
    const int non_b_qp = 0;
    return {mode & kPpFilterBits, qp, flat_thr, ((non_b_qp * base_dc_diff) >> 8) + 1};
}
// a plane's mode: the three bits, and dering only behind a vertical deblock (above)
AMV_HD inline bool pp_mode_ok(int mode) { return !(mode & ~kPpFilterBits) && (!(mode & kPpDering) || (mode & kPpVDeblock)); }
AMV_HD inline bool pp_size_ok(uint32_t w, uint32_t h) { return w >= 16u && h >= 16u && !(w & 15u) && !(h & 1u) && w <= kPpMaxWidth && h <= kPpMaxHeight; }
AMV_HD inline int pp_copy_ahead(int mode) { return mode & kPpVDeblock ? 5 : mode & kPpDering ? 1 : 0; }

// the source line that line i of strip y holds after the block copy (i >= copy_ahead)
AMV_HD inline int pp_fresh_source_line(int y, int i, int height) {
    if (y + 15 < height || i < height - y) return y + i;
    if (i >= (height - y > 8 ? height - y : 8)) return height - 1;
    return y - 8 + i;
}

// ---- deblock: ten taps v[0 .. 9] along the filter's direction, v[1 .. 8] the eight the filter owns -----------------------
// one lane's share of the classification: its count of near-equal neighbours (seven pairs) and, in bit 8, whether its own
// min/max probe fails.  m: the lane's index across the filter's direction, & 3
AMV_HD inline uint32_t pp_stat(const int* v, int m, const PpParams& p) {
    uint32_t cnt = 0;
    for (int i = 1; i < 8; ++i) cnt += (unsigned)(v[i] - v[i + 1] + p.dc_offset) < (unsigned)(p.dc_offset * 2 + 1);
    const int a = m == 0 ? v[1] : m == 1 ? v[3] : m == 2 ? v[5] : v[7];
    const int b = m == 0 ? v[6] : m == 1 ? v[8] : m == 2 ? v[2] : v[4];
    return cnt | ((unsigned)(a - b + 2 * p.qp) > (unsigned)(4 * p.qp) ? 0x100u : 0u);
}
// the eight lanes' stats added up -> the class: 2 not flat, 0 flat but a probe failed, 1 flat
AMV_HD inline int pp_class(uint32_t sum, const PpParams& p) { return (int)(sum & 0xffu) > p.flat_thr ? (sum >> 8 ? 0 : 1) : 2; }
AMV_HD inline int pp_abs(int a) { return a < 0 ? -a : a; }
AMV_HD inline void pp_low_pass(const int* v, int qp, int* out) {
    const int first = pp_abs(v[0] - v[1]) < qp ? v[0] : v[1];
    const int last = pp_abs(v[8] - v[9]) < qp ? v[9] : v[8];
    int s[10];
    s[0] = 4 * first + v[1] + v[2] + v[3] + 4;
    s[1] = s[0] - first + v[4];
    s[2] = s[1] - first + v[5];
    s[3] = s[2] - first + v[6];
    s[4] = s[3] - first + v[7];
    s[5] = s[4] - v[1] + v[8];
    s[6] = s[5] - v[2] + last;
    s[7] = s[6] - v[3] + last;
    s[8] = s[7] - v[4] + last;
    s[9] = s[8] - v[5] + last;
    for (int i = 0; i < 8; ++i) out[i] = (s[i] + s[i + 2] + 2 * v[i + 1]) >> 4;
}
// the default filter: the amount that leaves v[4] and joins v[5]
AMV_HD inline int pp_def_delta(const int* v, int qp) {
    const int middle = 5 * (v[5] - v[4]) + 2 * (v[3] - v[6]);
    if (pp_abs(middle) >= 8 * qp) return 0;
    const int q = (v[4] - v[5]) / 2;
    const int left = 5 * (v[3] - v[2]) + 2 * (v[1] - v[4]);
    const int right = 5 * (v[7] - v[6]) + 2 * (v[5] - v[8]);
    const int least = pp_abs(left) < pp_abs(right) ? pp_abs(left) : pp_abs(right);
    int d = pp_abs(middle) - least;
    d = d < 0 ? 0 : d;
    d = (5 * d + 32) >> 6;
    d *= -middle > 0 ? 1 : -1;
    if (q > 0) {
        d = d < 0 ? 0 : d;
        d = d > q ? q : d;
    } else {
        d = d > 0 ? 0 : d;
        d = d < q ? q : d;
    }
    return d;
}

// ---- dering ------------------------------------------------------------------------------------------------------------------
// one window line's ten pixels -> its sign mask (postprocess_template.c:1436-1454)
AMV_HD inline uint32_t pp_dering_line_mask(const int* px, int avg) {
    uint32_t t = 0;
    for (int i = 0; i < 10; ++i) t |= px[i] > avg ? 1u << i : 0u;
    t |= (~t) << 16;
    t &= (t << 1) & (t >> 1);
    return t;
}
AMV_HD inline uint32_t pp_dering_join(uint32_t above, uint32_t own, uint32_t below) {
    uint32_t t = above & own & below;
    return t | (t >> 16);
}
// n[0 .. 8]: the 3 x 3 around the pixel, row-major, n[4] the pixel itself -> its new value
AMV_HD inline int pp_dering_pixel(const int* n, int qp2) {
    int f = n[0] + 2 * n[1] + n[2] + 2 * n[3] + 4 * n[4] + 2 * n[5] + n[6] + 2 * n[7] + n[8];
    f = (f + 8) >> 4;
    if (n[4] + qp2 < f) return n[4] + qp2;
    if (n[4] - qp2 > f) return n[4] - qp2;
    return f;
}

// A call's 8 x 8 updates run as a wavefront of skew 2 (pixel (r, c) at step c + 2 r): right while no pixel of the call is another
// pixel's neighbour out of raster order.  On a plane 8 columns wide the only call is the row-end one and its window folds onto
// itself: its column 8 is the next line's column 0, so pixel (r, 7) IS the left neighbour of pixel (r + 1, 0), which the wavefront
// would run five steps earlier.  There the call runs in raster order, one pixel behind the other.
AMV_HD inline bool pp_dering_serial(int w) { return w == 8; }

// ---- the ring: line r, column c of the plane; a column behind the line's end is the next line's (a tight pitch) ----------
AMV_HD inline uint32_t pp_ring_at(int r, int c, int w) {
    if (c >= w) { c -= w; ++r; }
    return (uint32_t)((r + kPpRing) & (kPpRing - 1)) * (uint32_t)w + (uint32_t)c;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The kernel's order on the host.  Every inner loop over `lane`-like indices is one phase of the kernel: what a phase reads it
// reads before anything of the phase is written.
inline void pp_plane_rolling(const uint8_t* src, uint8_t* dst, int w, int h, const PpParams& p) {
    std::vector<uint8_t> ring((size_t)kPpRing * w), new7((size_t)w);
    std::vector<uint32_t> stat((size_t)w), cls((size_t)w);
    std::vector<int> taps((size_t)w * 10);
    const int ca = pp_copy_ahead(p.mode);
    for (int r = 0; r < ca; ++r) memcpy(&ring[pp_ring_at(r, 0, w)], src + (size_t)r * w, (size_t)w);
    for (int y = 0; y < h; y += 8) {
        const bool detour = y + 15 >= h;
        // the fresh lines
        if (detour)
            for (int r = h; r < y + ca; ++r) memcpy(&ring[pp_ring_at(r, 0, w)], &ring[pp_ring_at(h - 1, 0, w)], (size_t)w);
        for (int i = ca; i < ca + 8; ++i) memcpy(&ring[pp_ring_at(y + i, 0, w)], src + (size_t)pp_fresh_source_line(y, i, h) * w, (size_t)w);
        // vertical deblock: a lane per column
        if ((p.mode & kPpVDeblock) && y + 8 < h) {
            for (int x = 0; x < w; ++x) {
                int* v = &taps[(size_t)x * 10];
                for (int i = 0; i < 10; ++i) v[i] = ring[pp_ring_at(y + 3 + i, x, w)];
                stat[x] = pp_stat(v, x & 3, p);
            }
            for (int x = 0; x < w; ++x) {
                uint32_t sum = 0;
                for (int k = 0; k < 8; ++k) sum += stat[(x & ~7) + k];
                const int t = pp_class(sum, p);
                const int* v = &taps[(size_t)x * 10];
                if (t == 1) {
                    int out[8];
                    pp_low_pass(v, p.qp, out);
                    for (int i = 0; i < 8; ++i) ring[pp_ring_at(y + 4 + i, x, w)] = (uint8_t)out[i];
                } else if (t == 2) {
                    const int d = pp_def_delta(v, p.qp);
                    ring[pp_ring_at(y + 7, x, w)] = (uint8_t)(v[4] - d);
                    ring[pp_ring_at(y + 8, x, w)] = (uint8_t)(v[5] + d);
                }
            }
        }
        // horizontal deblock: a lane per line of an edge; item k = (edge - 1) * 8 + line
        if (p.mode & kPpHDeblock) {
            const int items = w - 8;
            for (int k = 0; k < items; ++k) {
                const int x = (k >> 3) * 8 + 8, r = k & 7;
                int* v = &taps[(size_t)k * 10];
                for (int i = 0; i < 10; ++i) v[i] = ring[pp_ring_at(y + r, x - 5 + i, w)];
                stat[k] = pp_stat(v, r & 3, p);
            }
            for (int k = 0; k < items; ++k) {
                uint32_t sum = 0;
                for (int j = 0; j < 8; ++j) sum += stat[(k & ~7) + j];
                cls[k] = (uint32_t)pp_class(sum, p);
                const int* v = &taps[(size_t)k * 10];
                int out[8];
                pp_low_pass(v, p.qp, out);                   // out[7] does not depend on v[0]
                new7[k] = (uint8_t)(cls[k] == 1u ? out[7] : v[8]);
            }
            for (int k = 0; k < items; ++k) {
                const int x = (k >> 3) * 8 + 8, r = k & 7;
                int* v = &taps[(size_t)k * 10];
                if (k >= 8) v[0] = new7[k - 8];              // the edge before's last column, as that edge leaves it
                if (cls[k] == 1u) {
                    int out[8];
                    pp_low_pass(v, p.qp, out);
                    for (int i = 0; i < 8; ++i) ring[pp_ring_at(y + r, x - 4 + i, w)] = (uint8_t)out[i];
                } else if (cls[k] == 2u) {
                    const int d = pp_def_delta(v, p.qp);
                    ring[pp_ring_at(y + r, x - 1, w)] = (uint8_t)(v[4] - d);
                    ring[pp_ring_at(y + r, x, w)] = (uint8_t)(v[5] + d);
                }
            }
        }
        // dering: the ranges of all calls first, then the calls one behind the other, each a wavefront of skew 2
        if ((p.mode & kPpDering) && y > 0) {
            const int calls = w / 8, qp2 = p.qp / 2 + 1;
            std::vector<int> mn((size_t)calls, 255), mx((size_t)calls, 0);
            for (int b = 0; b < calls; ++b)
                for (int k = 0; k < 64; ++k) {
                    const int v = ring[pp_ring_at(y + (k >> 3), b * 8 + 1 + (k & 7), w)];
                    mn[b] = v < mn[b] ? v : mn[b];
                    mx[b] = v > mx[b] ? v : mx[b];
                }
            for (int b = 0; b < calls; ++b) {
                if (mx[b] - mn[b] < kPpDeringThreshold) continue;
                const int avg = (mn[b] + mx[b] + 1) >> 1, x0 = b * 8;      // the window's first column: X - 8
                uint32_t line[10], mask[8];
                for (int t = 0; t < 10; ++t) {
                    int px[10];
                    for (int i = 0; i < 10; ++i) px[i] = ring[pp_ring_at(y - 1 + t, x0 + i, w)];
                    line[t] = pp_dering_line_mask(px, avg);
                }
                for (int r = 0; r < 8; ++r) mask[r] = pp_dering_join(line[r], line[r + 1], line[r + 2]);
                if (pp_dering_serial(w)) {
                    for (int k = 0; k < 64; ++k) {
                        const int r = k >> 3, c = k & 7;
                        if (!(mask[r] >> (c + 1) & 1u)) continue;
                        int n[9];
                        for (int j = 0; j < 9; ++j) n[j] = ring[pp_ring_at(y + r - 1 + j / 3, x0 + c + j % 3, w)];
                        ring[pp_ring_at(y + r, x0 + 1 + c, w)] = (uint8_t)pp_dering_pixel(n, qp2);
                    }
                    continue;
                }
                for (int step = 0; step < 22; ++step) {
                    int fresh[8];
                    for (int r = 0; r < 8; ++r) {
                        const int c = step - 2 * r;
                        fresh[r] = -1;
                        if (c < 0 || c > 7 || !(mask[r] >> (c + 1) & 1u)) continue;
                        int n[9];
                        for (int j = 0; j < 9; ++j) n[j] = ring[pp_ring_at(y + r - 1 + j / 3, x0 + c + j % 3, w)];
                        fresh[r] = pp_dering_pixel(n, qp2);
                    }
                    for (int r = 0; r < 8; ++r)
                        if (fresh[r] >= 0) ring[pp_ring_at(y + r, x0 + 1 + step - 2 * r, w)] = (uint8_t)fresh[r];
                }
            }
        }
        for (int r = y; r < y + 8 && r < h; ++r) memcpy(dst + (size_t)r * w, &ring[pp_ring_at(r, 0, w)], (size_t)w);
    }
}

// The reference's loop as it stands.  temp_src / temp_dst: 24 lines of w bytes each, kept by the caller from plane to plane as
// a PPContext keeps them (zeroed when made).  dst must have one line of slack in front: the loop copies the line above the
// plane into tempDst where the plane has fewer than 16 lines (and never uses it).
inline void pp_plane_serial(const uint8_t* src, uint8_t* dst, int w, int h, const PpParams& p, uint8_t* temp_src, uint8_t* temp_dst) {
    const int stride = w, ca = pp_copy_ahead(p.mode);
    auto block_copy = [&](uint8_t* d, const uint8_t* s) {
        for (int i = 0; i < 8; ++i) memcpy(d + stride * i, s + stride * i, 8);
    };
    auto classify = [&](const uint8_t* b, int step, int line) {          // b: the first of the eight along `step`
        uint32_t sum = 0;
        for (int k = 0; k < 8; ++k) {
            int v[10];
            for (int i = 0; i < 10; ++i) v[i] = b[k * line + (i - 1) * step];
            sum += pp_stat(v, k & 3, p);
        }
        return pp_class(sum, p);
    };
    auto deblock = [&](uint8_t* b, int step, int line) {
        const int t = classify(b, step, line);
        for (int k = 0; k < 8 && t; ++k) {
            int v[10], out[8];
            for (int i = 0; i < 10; ++i) v[i] = b[k * line + (i - 1) * step];
            if (t == 1) {
                pp_low_pass(v, p.qp, out);
                for (int i = 0; i < 8; ++i) b[k * line + i * step] = (uint8_t)out[i];
            } else {
                const int d = pp_def_delta(v, p.qp);
                b[k * line + 3 * step] = (uint8_t)(v[4] - d);
                b[k * line + 4 * step] = (uint8_t)(v[5] + d);
            }
        }
    };
    auto dering = [&](uint8_t* s) {
        int mn = 255, mx = 0;
        for (int y = 1; y < 9; ++y)
            for (int x = 1; x < 9; ++x) {
                const int v = s[stride * y + x];
                mx = v > mx ? v : mx;
                mn = v < mn ? v : mn;
            }
        if (mx - mn < kPpDeringThreshold) return;
        const int avg = (mn + mx + 1) >> 1, qp2 = p.qp / 2 + 1;
        uint32_t line[10];
        for (int y = 0; y < 10; ++y) {
            int px[10];
            for (int i = 0; i < 10; ++i) px[i] = s[stride * y + i];
            line[y] = pp_dering_line_mask(px, avg);
        }
        for (int y = 1; y < 9; ++y) {
            const uint32_t t = pp_dering_join(line[y - 1], line[y], line[y + 1]);
            for (int x = 1; x < 9; ++x)
                if (t >> x & 1u) {
                    uint8_t* q = s + stride * y + x;
                    int n[9];
                    for (int j = 0; j < 9; ++j) n[j] = q[(j / 3 - 1) * stride + j % 3 - 1];
                    *q = (uint8_t)pp_dering_pixel(n, qp2);
                }
        }
    };
    {
        uint8_t* dst_block = temp_dst + stride;
        for (int x = 0; x < w; x += 8) {
            block_copy(dst_block + stride * 8 + x, src + x);
            for (int i = 1; i < 4; ++i) memcpy(dst_block + stride * (8 - i) + x, dst_block + stride * 8 + x, 8);
        }
        memcpy(dst, temp_dst + 9 * stride, (size_t)ca * stride);
    }
    for (int y = 0; y < h; y += 8) {
        const uint8_t* src_block = src + (size_t)y * stride;
        uint8_t* dst_block = dst + (size_t)y * stride;
        const bool detour = y + 15 >= h;
        if (detour) {
            int n = h - y - ca > 0 ? h - y - ca : 0;
            memcpy(temp_src + stride * ca, src_block + stride * ca, (size_t)n * stride);
            for (int i = h - y > 8 ? h - y : 8; i < ca + 8; ++i) memcpy(temp_src + stride * i, src + (size_t)stride * (h - 1), (size_t)stride);
            n = h - y + 1 < ca + 1 ? h - y + 1 : ca + 1;
            memcpy(temp_dst, dst_block - stride, (size_t)n * stride);
            for (int i = h - y + 1; i <= ca; ++i) memcpy(temp_dst + stride * i, dst + (size_t)stride * (h - 1), (size_t)stride);
            dst_block = temp_dst + stride;
            src_block = temp_src;
        }
        for (int x = 0; x < w; x += 8) {
            block_copy(dst_block + stride * ca, src_block + stride * ca);
            if (y + 8 < h && (p.mode & kPpVDeblock)) deblock(dst_block + stride * 4, stride, 1);
            if (x - 8 >= 0) {
                if (p.mode & kPpHDeblock) deblock(dst_block - 4, 1, stride);
                if ((p.mode & kPpDering) && y > 0) dering(dst_block - stride - 8);
            }
            dst_block += 8;
            src_block += 8;
        }
        if ((p.mode & kPpDering) && y > 0) dering(dst_block - stride - 8);
        if (detour) memcpy(dst + (size_t)y * stride, temp_dst + stride, (size_t)(h - y) * stride);
    }
}
#endif

}  // namespace amv
