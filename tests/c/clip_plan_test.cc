// clip_plan_test.cc -- the arithmetic of the byte budget per clip (amv_clip_plan.h), walked on the CPU as the kernels of
// amv_encode_clip.hip walk it, against vectors tests/clip_ref.py wrote (argv[1]); its bounds, sums past 2^32, and the
// workspace plan of the clip entries (amv_host_plan.h).  Built with g++ under the address and undefined-behaviour sanitizers
// by tests/test_clip_ref.py; prints "ok <cases>".
//
// A vector file is lines of integers behind a tag:
//   C rungs n total budget[n] coded[n] bits[n][rungs] len[n][rungs] -> F[rungs] c over S record[n] passes
//       the floor sums; then the walk: clip_first_rung and clip_record_at, rate_check over the list, and with an empty list
//       clip_step and clip_move -- the clip rung, its flag, the sum, every frame's record (the flag in bit 31), and the passes
//       that coded a frame
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "amv_clip_plan.h"
#include "amv_host_plan.h"

using namespace amv;

static bool read_u64(FILE* f, std::vector<uint64_t>& v, size_t n) {
    v.resize(n);
    for (size_t i = 0; i < n; ++i) {
        unsigned long long x;
        if (fscanf(f, "%llu", &x) != 1) return false;
        v[i] = x;
    }
    return true;
}

struct Walk {
    uint64_t F[kRateRungsMax];
    uint64_t clip[2];
    std::vector<uint32_t> record;
    uint32_t passes;
};

// bits, len: [n][rungs], each row its own allocation (a read past a row is seen)
static bool walk(uint32_t rungs, uint32_t n, uint64_t total, const std::vector<uint32_t>& budget, const std::vector<uint8_t>& coded,
                 const std::vector<uint32_t*>& bits, const std::vector<uint32_t*>& len, Walk& w) {
    for (uint32_t c = 0; c < kRateRungsMax; ++c) w.F[c] = 0;
    for (uint32_t c = 0; c < rungs; ++c)
        for (uint32_t i = 0; i < n; ++i)
            if (coded[i]) w.F[c] += clip_floor(bits[i], rungs, budget[i], c);
    uint32_t c = clip_first_rung(w.F, rungs, total, 0u);
    w.record.assign(n, 0u);
    std::vector<uint32_t> length(n), list(n), next;
    for (uint32_t i = 0; i < n; ++i) {
        w.record[i] = coded[i] ? clip_record_at(bits[i], rungs, budget[i], c) : (rungs - 1u) | kRateOver;
        length[i] = len[i][w.record[i] & ~kRateOver];
        list[i] = i;
    }
    w.passes = 1;
    for (;;) {
        next.clear();
        for (uint32_t i : list)
            if (rate_check(bits[i], rungs, budget[i], length[i], w.record[i])) next.push_back(i);
        while (next.empty()) {
            uint64_t S = 0;
            for (uint32_t i = 0; i < n; ++i)
                if (coded[i]) S += length[i];
            const uint32_t before = c;
            if (clip_step(w.F, rungs, total, S, c, w.clip)) return true;
            if (c <= before || c >= rungs) return false;                      // (the clip rung rises and stays on the ladder)
            for (uint32_t i = 0; i < n; ++i)
                if (coded[i] && clip_move(bits[i], rungs, budget[i], c, w.record[i])) next.push_back(i);
        }
        list = next;
        if (++w.passes > clip_passes_most(rungs)) return false;
        for (uint32_t i : list) length[i] = len[i][w.record[i] & ~kRateOver];
    }
}

static int vectors(const char* path, unsigned& cases) {
    FILE* f = fopen(path, "r");
    if (!f) return printf("cannot open %s\n", path), 1;
    char tag[8];
    std::vector<uint64_t> head, v;
    while (fscanf(f, "%7s", tag) == 1) {
        if (strcmp(tag, "C")) return printf("unknown tag %s\n", tag), 1;
        if (!read_u64(f, head, 3)) return printf("short C vector\n"), 1;
        const uint32_t rungs = (uint32_t)head[0], n = (uint32_t)head[1];
        const uint64_t total = head[2];
        if (rungs < 1u || rungs > kRateRungsMax || n < 1u || n > 4096u) return printf("C case %u: %u rungs, %u frames\n", cases, rungs, n), 1;
        if (!read_u64(f, v, 2u * n + 2u * (size_t)n * rungs + rungs + 3u + n + 1u)) return printf("short C vector\n"), 1;
        std::vector<uint32_t> budget(n);
        std::vector<uint8_t> coded(n);
        std::vector<uint32_t*> bits(n), len(n);
        const uint64_t* p = v.data();
        for (uint32_t i = 0; i < n; ++i) budget[i] = (uint32_t)*p++;
        for (uint32_t i = 0; i < n; ++i) coded[i] = (uint8_t)*p++;
        for (std::vector<uint32_t*>* table : {&bits, &len})
            for (uint32_t i = 0; i < n; ++i) {
                (*table)[i] = (uint32_t*)malloc(rungs * sizeof(uint32_t));
                for (uint32_t r = 0; r < rungs; ++r) (*table)[i][r] = (uint32_t)*p++;
            }
        Walk w;
        const bool ended = walk(rungs, n, total, budget, coded, bits, len, w);
        for (uint32_t i = 0; i < n; ++i) free(bits[i]), free(len[i]);
        if (!ended) return printf("C case %u: the walk does not end inside clip_passes_most(%u) = %u passes\n", cases, rungs, clip_passes_most(rungs)), 1;
        for (uint32_t c = 0; c < rungs; ++c)
            if (w.F[c] != p[c]) return printf("C case %u: F(%u) = %llu, the model has %llu\n", cases, c, (unsigned long long)w.F[c], (unsigned long long)p[c]), 1;
        p += rungs;
        if ((w.clip[0] & ~kClipOver) != p[0] || ((w.clip[0] & kClipOver) != 0) != (p[1] != 0) || w.clip[1] != p[2])
            return printf("C case %u: clip %llx sum %llu, the model has %llu %llu %llu\n", cases, (unsigned long long)w.clip[0],
                          (unsigned long long)w.clip[1], (unsigned long long)p[0], (unsigned long long)p[1], (unsigned long long)p[2]), 1;
        p += 3;
        for (uint32_t i = 0; i < n; ++i)
            if (w.record[i] != p[i]) return printf("C case %u: frame %u at %x, the model has %llx\n", cases, i, w.record[i], (unsigned long long)p[i]), 1;
        if (w.passes != p[n]) return printf("C case %u: %u passes, the model has %llu\n", cases, w.passes, (unsigned long long)p[n]), 1;
        ++cases;
    }
    fclose(f);
    return 0;
}

// what the header states about its own bounds, and the edges the vectors do not reach
static int edges(unsigned& cases) {
    if (clip_passes_most(1u) != 1u || clip_passes_most(5u) != 15u || clip_passes_most(kRateRungsMax) != 136u) return printf("clip_passes_most\n"), 1;
    // the longest chunk: no wrap at the largest bits, and a floor never above it
    if (rate_most_bytes(0u) != 4u || rate_most_bytes(1u) != 6u || rate_most_bytes(8u) != 6u || rate_most_bytes(0xffffffffu) != 4ull + 0x40000000ull)
        return printf("rate_most_bytes at an edge\n"), 1;
    for (uint32_t bits : {0u, 7u, 8u, 9u, 4096u, 0xfffffff8u, 0xffffffffu})
        if (rate_floor_bytes(bits) > rate_most_bytes(bits)) return printf("a floor above the longest chunk\n"), 1;
    cases += 3;
    // a frame's part of the floor sum.  No cap: its own floor at c.  A cap: the least floor it may still reach
    const uint32_t row[4] = {800u, 80u, 400u, 8u};                            // floors 104, 14, 54, 5; longest 204, 24, 104, 6
    if (clip_floor(row, 4u, 0xffffffffu, 0u) != 104u || clip_floor(row, 4u, 0xffffffffu, 1u) != 14u || clip_floor(row, 4u, 0xffffffffu, 2u) != 54u ||
        clip_floor(row, 4u, 0xffffffffu, 3u) != 5u)
        return printf("clip_floor without a cap\n"), 1;
    // cap 110: rung 0 floor-fits but a chunk of 111 .. 204 bytes would not fit; rung 1 then holds it (24 <= 110): min(104, 14)
    if (clip_floor(row, 4u, 110u, 0u) != 14u) return printf("clip_floor: a frame that may move on\n"), 1;
    // cap 60 from rung 2: rung 2 floor-fits (54) and may not fit (104), the last rung then: min(54, 5)
    if (clip_floor(row, 4u, 60u, 2u) != 5u) return printf("clip_floor: down to the last rung\n"), 1;
    // cap 4: nothing floor-fits: the last rung's floor, where the frame is coded flagged
    if (clip_floor(row, 4u, 4u, 0u) != 5u || clip_record_at(row, 4u, 4u, 1u) != (3u | kRateOver)) return printf("clip_floor: no floor-fit\n"), 1;
    // cap 204 exactly: rung 0 holds the frame for certain
    if (clip_floor(row, 4u, 204u, 0u) != 104u || clip_floor(row, 4u, 203u, 0u) != 14u) return printf("clip_floor at the longest chunk\n"), 1;
    cases += 9;
    // a move: only a frame below the clip's rung, and a final record never
    uint32_t record = 1u;
    if (clip_move(row, 4u, 60u, 1u, record) || record != 1u) return printf("a frame at the clip's rung moved\n"), 1;
    if (!clip_move(row, 4u, 60u, 2u, record) || record != 2u) return printf("a frame below the clip's rung stayed\n"), 1;
    record = 0u;
    if (!clip_move(row, 4u, 20u, 2u, record) || record != 3u) return printf("a move past a rung that does not floor-fit\n"), 1;
    record = 0u;
    if (!clip_move(row, 4u, 4u, 2u, record) || record != (3u | kRateOver)) return printf("a move with no floor-fit left\n"), 1;
    if (clip_move(row, 4u, 4u, 3u, record) || record != (3u | kRateOver)) return printf("a final frame moved\n"), 1;
    cases += 5;
    // the clip step with sums past 2^32: final, a move past rungs whose floor sum is over, the last rung flagged or not
    const uint64_t big = 1ull << 40;
    const uint64_t F[5] = {big, big + 7u, big - 1u, big + 1u, 0xffffffffffffffffull};
    uint64_t clip[2] = {~0ull, ~0ull};
    uint32_t c = clip_first_rung(F, 5u, big - 1u, 0u);
    if (c != 2u || clip_first_rung(F, 5u, big, 0u) != 0u || clip_first_rung(F, 5u, 5u, 0u) != 4u || clip_first_rung(F, 5u, ~0ull, 4u) != 4u)
        return printf("clip_first_rung\n"), 1;
    c = 0u;
    if (clip_step(F, 5u, big, big + 1u, c, clip) || c != 2u || clip[0] != ~0ull) return printf("clip_step: a move past rung 1\n"), 1;
    if (!clip_step(F, 5u, big, big, c, clip) || c != 2u || clip[0] != 2u || clip[1] != big) return printf("clip_step: final at 2^40\n"), 1;
    if (clip_step(F, 5u, big, big + 1u, c, clip) || c != 4u) return printf("clip_step: no floor sum fits, the last rung\n"), 1;
    if (!clip_step(F, 5u, big, ~0ull, c, clip) || clip[0] != (4u | kClipOver) || clip[1] != ~0ull) return printf("clip_step: the last rung over\n"), 1;
    if (!clip_step(F, 5u, ~0ull, ~0ull, c, clip) || clip[0] != 4u) return printf("clip_step: a total of 2^64 - 1\n"), 1;
    c = 0u;
    if (!clip_step(F, 1u, 0u, 5u, c, clip) || clip[0] != (0u | kClipOver) || clip[1] != 5u) return printf("clip_step: one rung\n"), 1;
    cases += 7;
    // 70 000 frames of 100 000 bytes: the floor sum as the kernel adds it passes 2^32
    {
        const uint32_t one[1] = {8u * (100000u - 4u)};
        uint64_t sum = 0;
        for (uint32_t i = 0; i < 70000u; ++i) sum += clip_floor(one, 1u, 0xffffffffu, 0u);
        if (sum != 7000000000ull) return printf("a floor sum past 2^32\n"), 1;
        ++cases;
    }
    // the workspace plan: a counter for every pass and the one behind the last, the parts in order, none on another, 8-byte sums
    const ClipPlan p = clip_plan();
    if (p.counters != 0u || p.F < (clip_passes_most(kRateRungsMax) + 1u) * 4ull || (p.F & 7u) || p.state < p.F + kRateRungsMax * 8ull ||
        (p.state & 3u) || p.bytes < p.state + 4u * 4u)
        return printf("clip_plan\n"), 1;
    ++cases;
    printf("passes at most %u at %u rungs\n", clip_passes_most(kRateRungsMax), kRateRungsMax);
    return 0;
}

int main(int argc, char** argv) {
    unsigned cases = 0;
    if (argc > 1 && vectors(argv[1], cases)) return 1;
    if (edges(cases)) return 1;
    printf("ok %u\n", cases);
    return 0;
}
