// retable_plan_test.cc -- the arithmetic of re-tabling (amv-codec-tools_amd/csrc/amv_retable_plan.h) walked on the CPU: whole
// blocks against vectors tests/retable_ref.py wrote (argv[1]), every DC rounding tie, the edges of the range rule and one step
// over, the half-step bound at lambda 0 on seeded blocks over the whole range, and the reference encoder's tables.  Built with
// g++ by tests/test_retable_ref.py; prints "ok <cases>".
//
// A vector file is lines of integers behind a tag:
//   T comp lambda  qs[64]  in[64]  ->  ok out[64] err    retable_block: the source table and a block's levels in scan order; in
//                                                        range or not, the levels against AMV's tables, the block's error
//   F qscale  ->  luma[64]                               retable_ffmpeg_amv_tables (chroma is the same row)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>

#include "amv_retable_plan.h"

using namespace amv;

static const TrellisTables kTab = make_trellis_tables();

static bool read_ints(FILE* f, long long* v, int n) {
    for (int i = 0; i < n; ++i)
        if (fscanf(f, "%lld", &v[i]) != 1) return false;
    return true;
}

static int vectors(const char* path, unsigned& cases) {
    FILE* f = fopen(path, "r");
    if (!f) return printf("cannot open %s\n", path), 1;
    char tag[8];
    static long long v[2 + 64 + 64 + 1 + 64 + 1];
    while (fscanf(f, "%7s", tag) == 1) {
        if (!strcmp(tag, "F")) {
            if (!read_ints(f, v, 1 + 64)) return printf("short F vector\n"), 1;
            uint8_t t[2][64];
            if (!retable_ffmpeg_amv_tables((uint32_t)v[0], t)) return printf("F qscale %lld refused\n", v[0]), 1;
            for (int k = 0; k < 64; ++k)
                if (t[0][k] != v[1 + k] || t[1][k] != v[1 + k]) return printf("F qscale %lld: step[%d] = %d, the model has %lld\n", v[0], k, t[0][k], v[1 + k]), 1;
            ++cases;
            continue;
        }
        if (strcmp(tag, "T")) return printf("unknown tag %s\n", tag), 1;
        if (!read_ints(f, v, 2 + 64 + 64 + 1 + 64 + 1)) return printf("short T vector\n"), 1;
        uint8_t qs[64];
        int16_t in[64], out[64];
        for (int i = 0; i < 64; ++i) qs[i] = (uint8_t)v[2 + i], in[i] = (int16_t)v[66 + i];
        memset(out, 0x5A, sizeof out);
        uint32_t err = 0xdeadbeefu;
        const bool ok = retable_block(in, qs, kTab, (uint32_t)v[0], (uint32_t)v[1], out, &err);
        if (ok != (v[130] != 0)) return printf("T case %u: in range %d, the model has %lld\n", cases, (int)ok, v[130]), 1;
        if (ok) {
            for (int i = 0; i < 64; ++i)
                if (out[i] != v[131 + i]) return printf("T case %u: level[%d] = %d, the model has %lld\n", cases, i, out[i], v[131 + i]), 1;
            if (err != v[195]) return printf("T case %u: error %u, the model has %lld\n", cases, err, v[195]), 1;
        } else {
            for (int i = 0; i < 64; ++i)
                if (out[i] != 0x5A5A) return printf("T case %u: a block out of range was written\n", cases), 1;
        }
        ++cases;
    }
    fclose(f);
    return 0;
}

// Every tie of the DC's rounding goes away from zero, both signs; equal steps carry the level
static int dc_rounding(unsigned& cases) {
    for (uint32_t qd : {8u, 9u})
        for (uint32_t qs = 1; qs <= 255u; ++qs)
            for (int32_t level = -2048; level <= 2047; ++level) {
                const int32_t v = level * (int32_t)qs, got = retable_dc(level, qs, qd);
                // the nearest integer to v / qd: |got * qd - v| * 2 <= qd, and at a tie the one further from zero
                const int32_t e = got * (int32_t)qd - v;
                if (2 * abs(e) > (int32_t)qd) return printf("DC %d * %u / %u = %d is not the nearest\n", level, qs, qd, got), 1;
                if (2 * abs(e) == (int32_t)qd && abs(got) * (int32_t)qd < abs(v)) return printf("DC %d * %u / %u = %d: a tie went towards zero\n", level, qs, qd, got), 1;
                if (qs == qd && got != level) return printf("DC %d moved to %d with equal steps\n", level, got), 1;
                if ((got < 0) != (v < 0) && got != 0) return printf("DC %d * %u / %u = %d: the sign\n", level, qs, qd, got), 1;
            }
    if (retable_dc(4, 9, 8) != 5 || retable_dc(-4, 9, 8) != -5 || retable_dc(9, 4, 8) != 5 || retable_dc(-9, 4, 8) != -5 || retable_dc(4, 1, 8) != 1 ||
        retable_dc(-4, 1, 8) != -1 || retable_dc(9, 4, 9) != 4 || retable_dc(1, 9, 8) != 1 || retable_dc(9, 1, 9) != 1 || retable_dc(-9, 9, 9) != -9 ||
        retable_dc(-32768, 255, 8) != -1044480 || retable_dc(32767, 255, 9) != 928398)
        return printf("the DC's examples\n"), 1;
    ++cases;
    return 0;
}

static uint32_t rnd(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

// the constants' edges and one step over, for source steps 1, 7, 61 and 255
static int refusals(unsigned& cases) {
    for (uint32_t comp = 0; comp < 2; ++comp)
        for (uint32_t step : {1u, 7u, 61u, 255u})
            for (int i = 1; i < 64; ++i)
                for (int sign = -1; sign <= 1; sign += 2) {
                    uint8_t qs[64];
                    memset(qs, (int)step, sizeof qs);
                    int16_t in[64] = {0}, c[64];
                    TrellisPlainLine from{in}, line{c};
                    const int most = kRetableCoefMost / (8 * (int)step);
                    in[i] = (int16_t)(sign * most);
                    if (!retable_scale_block(from, qs, kTab.q[comp], line) || c[i] != in[i] * 8 * (int)step) return printf("the edge level at %d, step %u, is refused\n", i, step), 1;
                    in[i] = (int16_t)(sign * (most + 1));
                    if (retable_scale_block(from, qs, kTab.q[comp], line)) return printf("a level over the edge at %d, step %u, is taken\n", i, step), 1;
                    in[i] = (int16_t)(sign * 32767 - (sign < 0));
                    if (retable_scale_block(from, qs, kTab.q[comp], line)) return printf("the largest int16 at %d is taken\n", i), 1;
                    ++cases;
                }
    // the NEW DC: 1023 is taken, 1024 is not, whatever the old level was
    for (uint32_t comp = 0; comp < 2; ++comp) {
        const int32_t qd = kTab.q[comp][0];
        for (uint32_t step : {1u, 4u, 8u, 9u, 16u, 255u}) {
            uint8_t qs[64];
            memset(qs, (int)step, sizeof qs);
            int16_t in[64] = {0}, c[64];
            TrellisPlainLine from{in}, line{c};
            int taken = 0, refused = 0;
            for (int32_t level = -32768; level <= 32767; ++level) {
                in[0] = (int16_t)level;
                const int32_t want = retable_dc(level, step, (uint32_t)qd);
                const bool ok = retable_scale_block(from, qs, kTab.q[comp], line);
                if (ok != (abs(want) <= 1023)) return printf("a new DC of %d (level %d, step %u) is %s\n", want, level, step, ok ? "taken" : "refused"), 1;
                if (ok && c[0] != want) return printf("the new DC in the line\n"), 1;
                taken += ok && abs(want) == 1023;
                refused += !ok && abs(want) == 1024;
            }
            if (step * 32767u >= 1024u * (uint32_t)qd && (!taken || !refused) && step <= (uint32_t)qd)
                return printf("step %u: the DC's edge was not met (%d at 1023, %d at 1024)\n", step, taken, refused), 1;
            ++cases;
        }
    }
    // the energy: 15 coefficients of 8192 are 15 * 2^26 < 2^30, 16 are 2^30 exactly, 16 and one more step are over
    {
        uint8_t qs[64];
        memset(qs, 4, sizeof qs);
        int16_t in[64] = {0}, c[64];
        TrellisPlainLine from{in}, line{c};
        for (int i = 1; i <= 16; ++i) in[i] = (int16_t)(i & 1 ? 256 : -256);       // 256 * 8 * 4 = 8192
        if (!retable_scale_block(from, qs, kTab.q[0], line)) return printf("energy 2^30 is refused\n"), 1;
        in[17] = 1;
        if (retable_scale_block(from, qs, kTab.q[0], line)) return printf("energy 2^30 + 1024 is taken\n"), 1;
        ++cases;
    }
    return 0;
}

// lambda 0 on seeded blocks over the whole range, source steps 1 .. 255: every AC position comes back within half an AMV step
// (+ 1) of what the chunk meant, and the error is what the levels say, inside kRetableBlockErrorMost
static int half_step(unsigned& cases) {
    uint32_t seed = 20071u;
    long long worst = -1000000;
    for (int round = 0; round < 4000; ++round) {
        const uint32_t comp = round & 1u;
        uint8_t qs[64];
        int16_t in[64] = {0}, out[64];
        const int kind = round % 5;
        unsigned long long energy = 0;
        for (int i = 0; i < 64; ++i) {
            qs[i] = (uint8_t)(kind == 0 ? 1u : kind == 1 ? 255u : 1u + rnd(seed) % 255u);
            const int most = i ? kRetableCoefMost / (8 * (int)qs[i]) : 1023 * (int)kTab.q[comp][0] / (int)qs[i];
            int level = (int)(rnd(seed) % (uint32_t)(2 * most + 1)) - most;
            if (kind >= 3 && (rnd(seed) & 3u)) level = 0;
            if (i) {
                const long long c = (long long)level * 8 * qs[i];
                if (energy + (unsigned long long)(c * c) > kRetableEnergyMost) level = 0;
                else energy += (unsigned long long)(c * c);
            }
            in[i] = (int16_t)level;
        }
        for (uint32_t lambda : {0u, 3481u, kTrellisLambdaMax}) {
            uint32_t err;
            if (!retable_block(in, qs, kTab, comp, lambda, out, &err)) return printf("half step: round %d refused\n", round), 1;
            unsigned long long want = 0;
            for (int i = 0; i < 64; ++i) {
                const long long d = (long long)out[i] * kTab.q[comp][i] - (long long)in[i] * qs[i];
                want += (unsigned long long)(d * d);
                if (i && lambda == 0u) {
                    const long long over = llabs(8 * d) - 4 * kTab.q[comp][i];
                    if (over > worst) worst = over;
                    if (over > 1) return printf("half step: round %d position %d: |new * 8 Qd - c| = %lld, 4 Qd = %d\n", round, i, llabs(8 * d), 4 * kTab.q[comp][i]), 1;
                }
            }
            if (abs((int)out[0]) > kRetableDcMost || out[0] != retable_dc(in[0], qs[0], kTab.q[comp][0])) return printf("half step: the DC\n"), 1;
            if (want != err || want > kRetableBlockErrorMost) return printf("half step: the error %u, in 64 bits %llu\n", err, want), 1;
            ++cases;
        }
    }
    printf("half step: max(|new * 8 Qd - c| - 4 Qd) = %lld at lambda 0\n", worst);
    return 0;
}

static int tables(unsigned& cases) {
    uint8_t t[2][64];
    memset(t, 0x5A, sizeof t);
    for (uint32_t q : {0u, 32u, 255u, 0xffffffffu}) {
        if (retable_ffmpeg_amv_tables(q, t)) return printf("qscale %u is taken\n", q), 1;
        for (int i = 0; i < 128; ++i)
            if (t[i / 64][i % 64] != 0x5A) return printf("qscale %u: something was written\n", q), 1;
    }
    for (uint32_t q = 1; q <= 31u; ++q) {
        if (!retable_ffmpeg_amv_tables(q, t) || t[0][0] != 8 || t[1][0] != 8 || memcmp(t[0], t[1], 64)) return printf("qscale %u\n", q), 1;
        for (int k = 1; k < 64; ++k)
            if (t[0][k] < 2) return printf("qscale %u: a step below 2\n", q), 1;
    }
    retable_ffmpeg_amv_tables(8, t);
    if (t[0][1] != 16 || t[0][2] != 16 || t[0][63] != 83) return printf("qscale 8 is the matrix itself\n"), 1;
    retable_ffmpeg_amv_tables(31, t);
    if (t[0][63] != 255) return printf("the clip at qscale 31\n"), 1;
    ++cases;
    return 0;
}

int main(int argc, char** argv) {
    unsigned cases = 0;
    if (argc > 1 && vectors(argv[1], cases)) return 1;
    if (dc_rounding(cases)) return 1;
    if (refusals(cases)) return 1;
    if (half_step(cases)) return 1;
    if (tables(cases)) return 1;
    if (kRetableCoefMost != 8193 || kRetableEnergyMost != (1ull << 30) || kRetableDcMost != 1023 || kStTable != 16u || kRetableTablesMax != 64u)
        return printf("the constants\n"), 1;
    printf("ok %u\n", cases);
    return 0;
}
