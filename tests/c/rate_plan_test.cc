// rate_plan_test.cc -- the arithmetic of the encoder's byte budget per frame (amv_rate_plan.h), walked on the CPU against
// vectors tests/rate_ref.py wrote (argv[1]), its bounds, and the workspace plan of the rate entries (amv_host_plan.h).
// Built with g++ under the address and undefined-behaviour sanitizers by tests/test_rate_ref.py; prints "ok <cases>".
//
// A vector file is lines of integers behind a tag:
//   B comp level[64]                 -> bits      rate_block_bits of a block's levels, scan order (position 0 is not looked at)
//   D comp diff                      -> bits      rate_dc_bits
//   P block                          -> before    rate_dc_predecessor (-1: none)
//   F bits                           -> bytes     rate_floor_bytes
//   W rungs budget bits[rungs] len[rungs] -> fit[rungs + 1] rung over codings
//       rate_first_fit from every `from` 0 .. rungs; then the choice as the device makes it: rate_choose, and rate_check
//       on the chosen rung's length until it says no -- the record's rung, its flag, how often the frame was coded
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "amv_host_plan.h"
#include "amv_rate_plan.h"

using namespace amv;

static const TrellisTables kTab = make_trellis_tables();
static const RateDcLen kDc = make_rate_dc_len();

static bool read_ints(FILE* f, long long* v, int n) {
    for (int i = 0; i < n; ++i)
        if (fscanf(f, "%lld", &v[i]) != 1) return false;
    return true;
}

static int vectors(const char* path, unsigned& cases) {
    FILE* f = fopen(path, "r");
    if (!f) return printf("cannot open %s\n", path), 1;
    char tag[8];
    static long long v[4 + 4 * kRateRungsMax + 64];
    while (fscanf(f, "%7s", tag) == 1) {
        if (!strcmp(tag, "B")) {
            if (!read_ints(f, v, 66)) return printf("short B vector\n"), 1;
            int16_t block[64];
            for (int i = 0; i < 64; ++i) block[i] = (int16_t)v[1 + i];
            const TrellisPlainLine line{block};
            const uint32_t got = rate_block_bits(line, kTab.len[v[0]]);
            if (got != v[65]) return printf("B case %u: %u bits, the model has %lld\n", cases, got, v[65]), 1;
        } else if (!strcmp(tag, "D")) {
            if (!read_ints(f, v, 3)) return printf("short D vector\n"), 1;
            const uint32_t got = rate_dc_bits(kDc.len[v[0]], (int32_t)v[1]);
            if (got != v[2]) return printf("D case %u: diff %lld, %u bits, the model has %lld\n", cases, v[1], got, v[2]), 1;
        } else if (!strcmp(tag, "P")) {
            if (!read_ints(f, v, 2)) return printf("short P vector\n"), 1;
            if (rate_dc_predecessor((uint32_t)v[0]) != v[1])
                return printf("P case %u: block %lld after %lld, the model has %lld\n", cases, v[0], (long long)rate_dc_predecessor((uint32_t)v[0]), v[1]), 1;
        } else if (!strcmp(tag, "F")) {
            if (!read_ints(f, v, 2)) return printf("short F vector\n"), 1;
            if (rate_floor_bytes((uint32_t)v[0]) != v[1]) return printf("F case %u: floor(%lld) = %u\n", cases, v[0], rate_floor_bytes((uint32_t)v[0])), 1;
        } else if (!strcmp(tag, "W")) {
            if (!read_ints(f, v, 2)) return printf("short W vector\n"), 1;
            const uint32_t rungs = (uint32_t)v[0], budget = (uint32_t)v[1];
            if (rungs < 1u || rungs > kRateRungsMax) return printf("W case %u: %u rungs\n", cases, rungs), 1;
            if (!read_ints(f, v, (int)(3u * rungs + 4u))) return printf("short W vector\n"), 1;
            uint32_t* row = (uint32_t*)malloc(rungs * sizeof(uint32_t));   // (its own allocation: a read past the row is seen)
            for (uint32_t r = 0; r < rungs; ++r) row[r] = (uint32_t)v[r];
            const long long* len = v + rungs;
            const long long* fit = v + 2 * rungs;
            const long long* end = v + 3 * rungs + 1;
            for (uint32_t from = 0; from <= rungs; ++from)
                if (rate_first_fit(row, rungs, budget, from) != fit[from])
                    return printf("W case %u: first fit from %u is %u, the model has %lld\n", cases, from, rate_first_fit(row, rungs, budget, from), fit[from]), 1;
            uint32_t record = rate_choose(row, rungs, budget), codings = 1;
            while (rate_check(row, rungs, budget, (uint32_t)len[record & ~kRateOver], record)) {
                if (++codings > rungs) return printf("W case %u: the walk does not end\n", cases), 1;
            }
            free(row);
            if ((record & ~kRateOver) != end[0] || ((record & kRateOver) != 0u) != (end[1] != 0) || codings != end[2])
                return printf("W case %u: rung %u over %u after %u codings, the model has %lld %lld %lld\n", cases, record & ~kRateOver,
                              record >> 31, codings, end[0], end[1], end[2]), 1;
        } else {
            return printf("unknown tag %s\n", tag), 1;
        }
        ++cases;
    }
    fclose(f);
    return 0;
}

// what the header states about its own bounds, and the edges the vectors do not reach
static int edges(unsigned& cases) {
    // a frame's bits against 2^32 at the largest picture the rate entries take, and one block more
    if ((uint64_t)kRateBlocksMost * kRateBitsPerBlockMost > 0xffffffffull || (uint64_t)(kRateBlocksMost + 1u) * kRateBitsPerBlockMost <= 0xffffffffull)
        return printf("kRateBlocksMost is not the largest block count whose bits fit 32\n"), 1;
    if (!rate_blocks_ok(kRateBlocksMost) || rate_blocks_ok(kRateBlocksMost + 1u)) return printf("rate_blocks_ok\n"), 1;
    // no block spends more than the bound's 2048 bits: every position coded at the longest code and the largest magnitude
    for (uint32_t comp = 0; comp < 2; ++comp) {
        int16_t block[64];
        for (int i = 0; i < 64; ++i) block[i] = (i & 1) ? 1023 : -1023;
        const TrellisPlainLine line{block};
        const uint32_t dense = rate_block_bits(line, kTab.len[comp]) + rate_dc_bits(kDc.len[comp], -2047);
        if (dense > kRateBitsPerBlockMost) return printf("a dense block has %u bits\n", dense), 1;
        memset(block, 0, sizeof block);
        block[63] = 1;                                        // the longest run: three ZRLs, and no EOB behind position 63
        if (rate_block_bits(line, kTab.len[comp]) != 3u * kTab.len[comp][0xF0] + kTab.len[comp][0xE1] + 1u) return printf("a run of 62\n"), 1;
        block[63] = 0;
        if (rate_block_bits(line, kTab.len[comp]) != kTab.len[comp][0x00]) return printf("an empty block is one EOB\n"), 1;
        cases += 3;
    }
    // the floor at the ends of the range: no wrap
    if (rate_floor_bytes(0u) != 4u || rate_floor_bytes(1u) != 5u || rate_floor_bytes(8u) != 5u || rate_floor_bytes(0xffffffffu) != 4u + 0x20000000u)
        return printf("rate_floor_bytes at an edge\n"), 1;
    // a budget below every floor, and from == rungs
    const uint32_t row[3] = {80u, 0xffffffffu, 8u};
    if (rate_first_fit(row, 3u, 4u, 0u) != 3u || rate_first_fit(row, 3u, 5u, 0u) != 2u || rate_first_fit(row, 3u, 0xffffffffu, 1u) != 1u ||
        rate_first_fit(row, 3u, 0xffffffffu, 3u) != 3u)
        return printf("rate_first_fit at an edge\n"), 1;
    uint32_t record = rate_choose(row, 3u, 3u);
    if (record != (2u | kRateOver) || rate_check(row, 3u, 3u, 999u, record) || record != (2u | kRateOver)) return printf("a final frame moved\n"), 1;
    record = 2u;                                             // over on the last rung itself: flagged, not coded again
    if (rate_check(row, 3u, 5u, 6u, record) || record != (2u | kRateOver)) return printf("over on the last rung\n"), 1;
    record = 0u;                                             // over on an earlier one with no floor-fit behind it: the last rung, once more
    const uint32_t tight[3] = {8u, 800u, 800u};
    if (!rate_check(tight, 3u, 5u, 6u, record) || record != (2u | kRateOver)) return printf("over on the first rung\n"), 1;
    cases += 8;
    // the workspace plan: a counter for every pass and the last check, the parts in order, none on another, the zeroed span
    // the counters and the bits table exactly
    for (uint32_t n : {1u, 7u, 1030u})
        for (uint32_t rungs : {1u, 5u, kRateRungsMax})
            for (uint32_t blocks : {6u, 72u, 1800u}) {
                const RatePlan p = rate_plan(n, rungs, blocks);
                const uint64_t at[] = {p.counters, p.bits, p.lambda, p.list[0], p.list[1], p.state, p.dc, p.bytes};
                const uint64_t need[] = {(kRateRungsMax + 1u) * 4ull, (uint64_t)n * rungs * 4u, n * 4ull, n * 4ull, n * 4ull, 65u * 4ull,
                                         (uint64_t)n * blocks * 2u};
                for (int i = 0; i < 7; ++i)
                    if (at[i] + need[i] > at[i + 1] || (at[i] & 3u)) return printf("rate_plan(%u, %u, %u): part %d\n", n, rungs, blocks, i), 1;
                if (p.zero != p.counters || p.zero + p.zero_bytes != p.lambda || (p.dc & 15u)) return printf("rate_plan: the zeroed span\n"), 1;
                ++cases;
            }
    printf("bits per block at most %u, blocks at most %u\n", kRateBitsPerBlockMost, kRateBlocksMost);
    return 0;
}

int main(int argc, char** argv) {
    unsigned cases = 0;
    if (argc > 1 && vectors(argv[1], cases)) return 1;
    if (edges(cases)) return 1;
    printf("ok %u\n", cases);
    return 0;
}
