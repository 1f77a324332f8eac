// lowres_plan_test.cc -- the reduced-size decode's geometry (amv-codec-tools_amd/csrc/amv_host_plan.h: lowres_dim,
// lowres_frame_bytes, lowres_start_row, lowres_rows_reached) walked on the CPU against a brute-force "which plane row does
// canvas row r reach, which plane column does canvas column x reach", for every (w, h, lowres) with w, h <= 80.
//
// The rule (include/amvhip.h): full-size canvas row r of a component is reduced canvas row r >> L and lands at plane row
// start_L - (r >> L); canvas column x lands at plane column x >> L; what falls outside the plane is dropped.  Checked:
//   - every plane column is reached, for every size;
//   - the plane rows reached are exactly 0 .. lowres_rows_reached - 1, each by the 2^L consecutive canvas rows of one
//     reduced row (the top one of the canvas may be cut short by nothing: the canvas is whole MCUs);
//   - for h % 16 <= 8 that is every plane row (lowres_store_covers_planes), and wherever the full-size formula of
//     mjpegdec.c:675 reaches every row of its plane, the reduced one does too;
//   - for h % 16 of 0 or 8 the placement is the exact vertical flip of the reduced canvas's first H_L rows;
//   - where start + 1 is a multiple of 2^L, the plane row equals the full-size plane row >> L (the thumbnail is the
//     downscale of what the full-size mode shows); otherwise it is that or one row above it;
//   - the frame bytes are the three tight planes.
// Built with g++ and the sanitizers by tests/test_lowres_ref.py; prints "ok <cases>" last, or the first failing case.
#include <cstdio>
#include <vector>

#include "amv_host_plan.h"

using namespace amv;

int main() {
    unsigned cases = 0;
    if (lowres_dim(129, 3) != 17 || lowres_dim(128, 3) != 16 || lowres_dim(1, 3) != 1 || lowres_dim(160, 0) != 160 || lowres_dim(160, 4) != 0)
        return printf("lowres_dim\n"), 1;
    if (lowres_frame_bytes(160, 120, 4) != 0) return printf("lowres_frame_bytes: lowres 4\n"), 1;
    for (uint32_t L = 1; L <= 3; ++L)
        for (uint32_t h = 1; h <= 80; ++h)
            for (uint32_t w = 1; w <= 80; ++w) {
                const uint32_t wl = lowres_dim(w, L), hl = lowres_dim(h, L);
                if (wl != (w + (1u << L) - 1) / (1u << L) || hl != (h + (1u << L) - 1) / (1u << L)) return printf("dim %u %u %u\n", w, h, L), 1;
                if (lowres_frame_bytes(w, h, L) != (uint64_t)wl * hl + 2ull * ((wl + 1) / 2) * ((hl + 1) / 2)) return printf("bytes %u %u %u\n", w, h, L), 1;
                const uint32_t mcu_cols = (w + 15) / 16, mcu_rows = (h + 15) / 16;
                bool all_rows = true;
                for (int chroma = 0; chroma < 2; ++chroma) {
                    const uint32_t pw = chroma ? (wl + 1) / 2 : wl, ph = lowres_plane_rows(h, L, chroma);
                    if (ph != (chroma ? (hl + 1) / 2 : hl)) return printf("plane rows %u %u\n", h, L), 1;
                    const uint32_t canvas_w = mcu_cols * (chroma ? 8u : 16u), canvas_h = mcu_rows * (chroma ? 8u : 16u);
                    // columns
                    std::vector<int> col(pw, 0);
                    for (uint32_t x = 0; x < canvas_w; ++x)
                        if ((x >> L) < pw) ++col[x >> L];
                    for (uint32_t x = 0; x < pw; ++x)
                        if (col[x] != (1 << L)) return printf("column %u of %u x %u lowres %u chroma %d reached %d times\n", x, w, h, L, chroma, col[x]), 1;
                    // rows
                    const int start = ffmpeg_start_row(h, chroma), start_l = lowres_start_row(h, L, chroma);
                    if (start != (chroma ? 1 : 2) * (int)(8 * mcu_rows - ((h / 2) & 7)) - 1) return printf("start %u\n", h), 1;
                    std::vector<int> row(ph, 0);
                    for (uint32_t r = 0; r < canvas_h; ++r) {
                        const int p = start_l - (int)(r >> L);
                        if (p < 0 || p >= (int)ph) continue;
                        ++row[p];
                        const int full = start - (int)r;                  // where the full-size mode shows this canvas row
                        if (full >= 0) {
                            const int scaled = full >> L;
                            if ((start + 1) % (1 << L) == 0 ? p != scaled : (p != scaled && p != scaled + 1))
                                return printf("canvas row %u of h %u lowres %u chroma %d: plane row %d, full-size row %d\n", r, h, L, chroma, p, full), 1;
                        }
                    }
                    const uint32_t reached = lowres_rows_reached(h, L, chroma);
                    for (uint32_t p = 0; p < ph; ++p)
                        if (row[p] != (p < reached ? (1 << L) : 0))
                            return printf("plane row %u of h %u lowres %u chroma %d reached %d times (rows reached: %u)\n", p, h, L, chroma, row[p], reached), 1;
                    if (reached != ph) all_rows = false;
                    const uint32_t full_ph = chroma ? (h + 1) / 2 : h;
                    if (start >= (int)full_ph - 1 && reached != ph) return printf("h %u lowres %u chroma %d: the full-size rule covers its plane, the reduced one does not\n", h, L, chroma), 1;
                    if ((h % 16 == 0 || h % 16 == 8) && start_l != (int)ph - 1) return printf("h %u lowres %u chroma %d: not the exact flip\n", h, L, chroma), 1;
                }
                if (all_rows != lowres_store_covers_planes(h, L)) return printf("covers %u %u\n", h, L), 1;
                if (h % 16 <= 8 && !all_rows) return printf("h %u lowres %u: a plane row is not reached\n", h, L), 1;
                ++cases;
            }
    printf("ok %u\n", cases);
    return 0;
}
