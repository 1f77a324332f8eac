// nr_plan_test.cc -- the -nr arithmetic (amv-codec-tools_amd/csrc/amv_nr_plan.h) walked on the CPU: the frame-start update and
// the per-block denoise against vectors tests/nr_ref.py wrote (argv[1]), and the argument bound's edges against 64-bit
// arithmetic.  Built with g++ by tests/test_nr_ref.py; prints "ok <cases>".
//
// A vector file is lines of integers behind a tag:
//   F nr  state[65]                ->  state'[65] offset[64]      nr_frame_start
//   B     state[65] offset[64] block[64]  ->  state'[65] block'[64]     nr_block (this encoder's fdct outputs: DC = reference DC - 8192)
#include <stdio.h>
#include <string.h>

#include <initializer_list>

#include "amv_nr_plan.h"

using namespace amv;

static bool read_ints(FILE* f, long long* v, int n) {
    for (int i = 0; i < n; ++i)
        if (fscanf(f, "%lld", &v[i]) != 1) return false;
    return true;
}

static int vectors(const char* path, unsigned& cases) {
    FILE* f = fopen(path, "r");
    if (!f) return printf("cannot open %s\n", path), 1;
    char tag[8];
    static long long v[1 + 65 + 64 + 64 + 65 + 64];
    while (fscanf(f, "%7s", tag) == 1) {
        int32_t state[65];
        uint16_t off[64];
        if (!strcmp(tag, "F")) {
            if (!read_ints(f, v, 1 + 65 + 65 + 64)) return printf("short F vector\n"), 1;
            for (int i = 0; i < 65; ++i) state[i] = (int32_t)v[1 + i];
            nr_frame_start(state, (uint32_t)v[0], off);
            for (int i = 0; i < 65; ++i)
                if (state[i] != v[66 + i]) return printf("F case %u: state[%d] = %d, the model has %lld\n", cases, i, state[i], v[66 + i]), 1;
            for (int i = 0; i < 64; ++i)
                if (off[i] != v[131 + i]) return printf("F case %u: offset[%d] = %u, the model has %lld\n", cases, i, off[i], v[131 + i]), 1;
        } else if (!strcmp(tag, "B")) {
            if (!read_ints(f, v, 65 + 64 + 64 + 65 + 64)) return printf("short B vector\n"), 1;
            int16_t block[64];
            for (int i = 0; i < 65; ++i) state[i] = (int32_t)v[i];
            for (int i = 0; i < 64; ++i) off[i] = (uint16_t)v[65 + i];
            for (int i = 0; i < 64; ++i) block[i] = (int16_t)v[129 + i];
            nr_block(state, off, block);
            for (int i = 0; i < 65; ++i)
                if (state[i] != v[193 + i]) return printf("B case %u: state[%d] = %d, the model has %lld\n", cases, i, state[i], v[193 + i]), 1;
            for (int i = 0; i < 64; ++i)
                if (block[i] != v[258 + i]) return printf("B case %u: block[%d] = %d, the model has %lld\n", cases, i, block[i], v[258 + i]), 1;
        } else {
            return printf("unknown tag %s\n", tag), 1;
        }
        ++cases;
    }
    fclose(f);
    return 0;
}

// A stream of the heaviest frames there are (every block adds 16320 at every position) at `blocks` a frame and nr, in the
// header's 32-bit arithmetic and in 64 bits beside it: the same wherever nothing wraps.  Returns the largest dividend seen.
static long long heaviest_stream(uint32_t blocks, uint32_t nr, int frames, bool& same) {
    int32_t s32[65] = {};
    long long s64[65] = {}, top = 0;
    uint16_t off[64];
    same = true;
    for (int f = 0; f < frames; ++f) {
        nr_frame_start(s32, nr, off);
        if (s64[64] > (1 << 16))
            for (int i = 0; i < 65; ++i) s64[i] >>= 1;
        for (int i = 0; i < 64; ++i) {
            const long long num = (long long)nr * s64[64] + s64[i] / 2, den = s64[i] + 1;
            if (num > top) top = num;
            if (num > 0x7fffffffll || den > 0x7fffffffll || off[i] != (uint16_t)(num / den)) same = false;
        }
        for (int i = 0; i < 64; ++i) {
            s32[i] = (int32_t)((uint32_t)s32[i] + blocks * kNrLargest);
            s64[i] += (long long)blocks * kNrLargest;
        }
        s32[64] = (int32_t)((uint32_t)s32[64] + blocks);
        s64[64] += blocks;
        for (int i = 0; i < 65; ++i)
            if (s64[i] > 0x7fffffffll || s32[i] != s64[i]) same = false;
        if ((uint64_t)s64[64] > nr_count_most(blocks)) same = false;      // the count stays where the bound's reasoning puts it
    }
    return top;
}

int main(int argc, char** argv) {
    unsigned cases = 0;
    if (argc > 1 && vectors(argv[1], cases)) return 1;

    // the largest frame: max(65536, B) + B + 1 <= (2^31 - 2) / 16320 = 131585
    if (!nr_frame_ok(6u) || !nr_frame_ok(65536u) || !nr_frame_ok(65792u) || nr_frame_ok(65793u) || nr_frame_ok(0u) || nr_frame_ok(0xffffffffu))
        return printf("nr_frame_ok's edge\n"), 1;
    if (nr_max(65793u) != 0u || nr_max(0u) != 0u) return printf("nr_max of a refused frame\n"), 1;
    const uint32_t sizes[] = {6u, 36u, 1800u, 48960u, 65532u, 65538u, 65790u, 65792u};
    for (uint32_t b : sizes) {
        const uint32_t most = nr_max(b);
        const unsigned long long c0 = nr_count_start_most(b), half = (unsigned long long)kNrLargest * (c0 + 1u) / 2u;
        if (most * c0 + half > 0x7fffffffull || (most + 1ull) * c0 + half <= 0x7fffffffull) return printf("nr_max(%u) = %u is not the edge\n", b, most), 1;
        // frames enough to pass the first halving and several after it
        const int frames = (int)(3u * 65536u / b) + 8;
        bool same;
        const long long top = heaviest_stream(b, most, frames > 400 ? 400 : frames, same);
        if (!same) return printf("%u blocks, nr %u: the 32-bit arithmetic left the 64-bit one\n", b, most), 1;
        if (top > 0x7fffffffll) return printf("%u blocks, nr %u: dividend %lld\n", b, most, top), 1;
        ++cases;
    }
    // beyond the bound the dividend does wrap: the bound is not slack by more than the state's slack of one block
    {
        bool same;
        heaviest_stream(65790u, nr_max(65790u) + 1300u, 12, same);
        if (same) return printf("nr far above nr_max did not wrap\n"), 1;
        ++cases;
    }
    // a state no stream reaches: no trap, whatever comes out
    {
        int32_t state[65];
        uint16_t off[64];
        for (int i = 0; i < 65; ++i) state[i] = i & 1 ? -1 - i : (int32_t)0x80000000u + i;
        state[1] = -1; state[2] = -2; state[64] = 0x7fffffff;
        nr_frame_start(state, 0xffffffffu, off);
        int16_t block[64];
        for (int i = 0; i < 64; ++i) block[i] = (int16_t)(i & 1 ? 8193 : -8193);
        nr_block(state, off, block);
        ++cases;
    }
    // the workspace: sums, then offsets, nothing overlapping, 16-byte lines
    for (uint32_t n : {1u, 3u, 1000u, 0xffffffffu}) {
        const NrPlan p = nr_plan(n);
        if (p.sums != 0u || p.offsets < (uint64_t)n * 64u * 4u || p.bytes < p.offsets + (uint64_t)n * 64u * 2u || (p.offsets & 15u))
            return printf("plan at n = %u\n", n), 1;
        ++cases;
    }
    for (uint32_t i = 0; i < 64; ++i)
        if (nr_consumed_index(nr_consumed_index(i)) != i || nr_consumed_index(i) != (i % 8u) * 8u + i / 8u) return printf("consumed index %u\n", i), 1;
    printf("ok %u\n", cases);
    return 0;
}
