// nr_trellis_plan_test.cc -- the trellis quantiser behind -nr, walked on the CPU: nr_block (amv_nr_plan.h) and then
// trellis_block (amv_trellis_plan.h) on whole blocks against vectors tests/nr_trellis_ref.py wrote (argv[1]), and denoised
// blocks at the edges of the bound on lambda against the 64-bit walk of trellis_plan_test.cc.  Built with g++ by
// tests/test_nr_trellis_ref.py; prints "ok <cases>".
//
// A vector file is lines of integers behind a tag:
//   N comp qbias lambda  state[65] offset[64] c[64]  ->  state[65] out[64]
//       c: fdct outputs, row-major (the reference's index order, as state and offset are); out: the denoised DC and the
//       levels, scan order
#define main trellis_plan_test_main   // that file's helpers (kTab, read_ints, wide_block, same_as_wide, rnd), not its main
#include "trellis_plan_test.cc"
#undef main

#include "amv_nr_plan.h"

static int zigzag[64];   // scan position -> row-major index
static void make_zigzag() {
    int n = 0;
    for (int s = 0; s < 15; ++s)
        for (int k = 0; k <= s; ++k) {
            const int r = (s & 1) ? k : s - k, c = s - r;
            if (r < 8 && c < 8) zigzag[n++] = r * 8 + c;
        }
}

static int nr_vectors(const char* path, unsigned& cases) {
    FILE* f = fopen(path, "r");
    if (!f) return printf("cannot open %s\n", path), 1;
    char tag[8];
    static long long v[3 + 65 + 64 + 64 + 65 + 64];
    while (fscanf(f, "%7s", tag) == 1) {
        if (strcmp(tag, "N")) return printf("unknown tag %s\n", tag), 1;
        if (!read_ints(f, v, 3 + 65 + 64 + 64 + 65 + 64)) return printf("short N vector\n"), 1;
        int32_t state[65];
        uint16_t offset[64];
        int16_t raw[64], block[64];
        for (int i = 0; i < 65; ++i) state[i] = (int32_t)v[3 + i];
        for (int i = 0; i < 64; ++i) offset[i] = (uint16_t)v[68 + i];
        for (int i = 0; i < 64; ++i) raw[i] = (int16_t)v[132 + i];
        nr_block(state, offset, raw);
        for (int i = 0; i < 65; ++i)
            if (state[i] != v[196 + i]) return printf("N case %u: state[%d] = %d, the model has %lld\n", cases, i, state[i], v[196 + i]), 1;
        for (int i = 0; i < 64; ++i) block[i] = raw[zigzag[i]];
        TrellisPlainLine line{block};
        TrellisLane ws;
        memset(&ws, 0xA5, sizeof ws);
        trellis_block(line, kTab, (uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2], ws);
        for (int i = 0; i < 64; ++i)
            if (block[i] != v[261 + i]) return printf("N case %u: level[%d] = %d, the model has %lld\n", cases, i, block[i], v[261 + i]), 1;
        ++cases;
    }
    fclose(f);
    return 0;
}

// Blocks of as much energy as a block holds (+-1024 everywhere: the sum of c^2 is 2^26, Parseval), random ones, and ones that
// straddle the offset, denoised with offsets from 0 to beyond every magnitude
// (the uint16's 65535 included), at lambda 0, the reference's, and the bound: no denoised magnitude is above the one it came
// from, the 32-bit walk gives the 64-bit walk's levels, and no sum leaves the range the bound allows.
static int denoised_edges(unsigned& cases) {
    long long most = 0, least = 0;
    uint32_t seed = 2468u;
    const uint32_t lambdas[] = {0u, 3481u, kTrellisLambdaMax};
    const uint32_t offsets[] = {0u, 1u, 37u, 500u, 8192u, 8193u, 65535u};
    for (uint32_t comp = 0; comp < 2; ++comp)
        for (uint32_t qbias : {0u, 128u, 255u})
            for (uint32_t lambda : lambdas)
                for (uint32_t off : offsets)
                    for (int kind = 0; kind < 3; ++kind) {
                        int16_t c[64];
                        for (int i = 0; i < 64; ++i) {
                            const int sign = (rnd(seed) >> 16) & 1u ? -1 : 1;
                            const int x = kind == 0 ? sign * 1024 : kind == 1 ? sign * (int)(rnd(seed) % 1449u) : sign * (int)(off + rnd(seed) % 3u);
                            const int xc = x > 8193 ? 8193 : x < -8193 ? -8193 : x;
                            const int d = nr_denoise(xc, kind == 1 ? rnd(seed) % (off + 1u) : off);
                            if (abs(d) > abs(xc) || (d && (d < 0) != (xc < 0))) return printf("nr_denoise(%d, %u) = %d\n", xc, off, d), 1;
                            c[i] = (int16_t)d;
                        }
                        if (same_as_wide(c, comp, qbias, lambda, most, least, "denoised")) return 1;
                        ++cases;
                    }
    const long long bound = 63ll * (kTrellisStepMost + (long long)kTrellisBitsMost * kTrellisLambdaMax);
    if (most > bound) return printf("a sum of %lld is above the bound's %lld\n", most, bound), 1;
    printf("denoised: sums inside %lld .. %lld, the bound allows %lld < %d\n", least, most, bound, kTrellisNoScore);
    return 0;
}

int main(int argc, char** argv) {
    unsigned cases = 0;
    make_zigzag();
    if (argc > 1 && nr_vectors(argv[1], cases)) return 1;
    if (denoised_edges(cases)) return 1;
    printf("ok %u\n", cases);
    return 0;
}
