// psnr_plan_test.cc -- the `-psnr` host arithmetic (amv-codec-tools_amd/csrc/amv_host_plan.h: psnr_db, psnr_report,
// picture_sse_ok) walked on the CPU against the formulas of ffmpeg.c:849-852 and :953-972 written out in long double, and
// their edges.  Built with g++ by tests/test_psnr_ref.py; prints "ok <cases>".
#include <math.h>
#include <stdio.h>

#include "amv_host_plan.h"

using namespace amv;

static bool close_db(double got, long double want) { return fabsl((long double)got - want) <= 1e-9L; }

int main() {
    unsigned cases = 0;
    // one frame, one plane: -10 log10(sse / (samples * 255^2))
    const uint64_t sses[] = {1ull, 7ull, 65025ull, 123456789ull, 4261478400ull, 0xffffffffull, 1ull << 40, 25ull * 65025ull};
    const uint64_t samples[] = {1ull, 4ull, 19200ull, 76800ull, 65536ull, 1ull << 32};
    for (uint64_t e : sses)
        for (uint64_t s : samples) {
            const long double want = -10.0L * log10l((long double)e / ((long double)s * 65025.0L));
            if (!close_db(psnr_db(e, s), want)) return printf("psnr_db(%llu, %llu) = %.12f, want %.12Lf\n", (unsigned long long)e, (unsigned long long)s, psnr_db(e, s), want), 1;
            ++cases;
        }
    // every sample off by 255 is 0 dB, by 1 is 20 log10(255)
    if (!close_db(psnr_db(65025ull * 100ull, 100ull), 0.0L) || !close_db(psnr_db(100ull, 100ull), 20.0L * log10l(255.0L))) return printf("the fixed points\n"), 1;
    if (!isinf(psnr_db(0, 100)) || psnr_db(0, 100) < 0) return printf("sse 0 is not +inf\n"), 1;
    if (!isnan(psnr_db(5, 0)) || !isnan(psnr_db(0, 0))) return printf("no samples is not NaN\n"), 1;
    cases += 3;

    // the report over n frames: luma scale w * h * 255^2 * n, chroma a quarter, * from the sums
    const uint32_t w = 160, h = 120, n = 5;
    uint64_t sse[n][3];
    long double sum[3] = {0, 0, 0};
    for (uint32_t i = 0; i < n; ++i)
        for (int p = 0; p < 3; ++p) {
            sse[i][p] = 1000ull * (i + 1) * (p + 2) + 17ull * i * i + (p == 0 ? 4000000000ull : 0ull);   // (the luma sum passes 32 bits)
            sum[p] += (long double)sse[i][p];
        }
    double out[4];
    psnr_report(&sse[0][0], n, w, h, out);
    const long double scale = (long double)w * h * 65025.0L * n;
    for (int p = 0; p < 3; ++p)
        if (!close_db(out[p], -10.0L * log10l(sum[p] / (p ? scale / 4 : scale)))) return printf("report entry %d = %.12f\n", p, out[p]), 1;
    if (!close_db(out[3], -10.0L * log10l((sum[0] + sum[1] + sum[2]) / (scale * 1.5L)))) return printf("report * = %.12f\n", out[3]), 1;
    // one frame's luma entry is the -vstats figure
    psnr_report(&sse[2][0], 1, w, h, out);
    if (out[0] != psnr_db(sse[2][0], (uint64_t)w * h) || out[1] != psnr_db(sse[2][1], (uint64_t)w * h / 4)) return printf("report of one frame against psnr_db\n"), 1;
    // nothing wrong anywhere: every entry +inf; a plane alone at 0: that entry only
    uint64_t zero[2][3] = {{0, 0, 0}, {0, 0, 0}};
    psnr_report(&zero[0][0], 2, w, h, out);
    for (int p = 0; p < 4; ++p)
        if (!isinf(out[p]) || out[p] < 0) return printf("report of zeros, entry %d\n", p), 1;
    zero[1][2] = 9;
    psnr_report(&zero[0][0], 2, w, h, out);
    if (!isinf(out[0]) || !isinf(out[1]) || isinf(out[2]) || isinf(out[3])) return printf("report with one plane off\n"), 1;
    psnr_report(&zero[0][0], 0, w, h, out);
    for (int p = 0; p < 4; ++p)
        if (!isnan(out[p])) return printf("report of no frames, entry %d\n", p), 1;
    cases += 8;

    // the formats picture against picture takes
    for (int f = -1; f <= AMVHIP_PIX_COUNT; ++f) {
        const bool want = (f >= AMVHIP_PIX_YUV420P && f <= AMVHIP_PIX_YUVJ444P) || f == AMVHIP_PIX_GRAY8 || f == AMVHIP_PIX_RGB24 || f == AMVHIP_PIX_BGR24;
        if ((picture_sse_ok(f, 17, 9) != 0) != want) return printf("picture_sse_ok(%d)\n", f), 1;
        if (picture_sse_ok(f, 0, 9) || picture_sse_ok(f, 17, 0) || picture_sse_ok(f, AMVHIP_MAX_DIM + 1u, 9)) return printf("picture_sse_ok(%d) at a bad size\n", f), 1;
        ++cases;
    }
    printf("ok %u\n", cases);
    return 0;
}
