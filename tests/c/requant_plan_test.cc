// requant_plan_test.cc -- the arithmetic of requantising chunks in the coefficient domain (amv-codec-tools_amd/csrc/
// amv_requant_plan.h) walked on the CPU: whole blocks against vectors tests/requant_ref.py wrote (argv[1]), the first
// candidate against the input level for every step and every level up to kRequantCoefMost, and the walk in 64 bits at the
// edges of both range constants and of the bound on lambda.  Built with g++ by tests/test_requant_ref.py; prints "ok <cases>".
//
// A vector file is lines of integers behind a tag:
//   R comp lambda  in[64]  ->  ok out[64] err     requant_block: a block's levels in scan order; in range or not, the levels
//                                                after the search (the DC carried), the block's error
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>

#include "amv_requant_plan.h"

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
    static long long v[2 + 64 + 1 + 64 + 1];
    while (fscanf(f, "%7s", tag) == 1) {
        if (strcmp(tag, "R")) return printf("unknown tag %s\n", tag), 1;
        if (!read_ints(f, v, 2 + 64 + 1 + 64 + 1)) return printf("short R vector\n"), 1;
        int16_t in[64], out[64];
        for (int i = 0; i < 64; ++i) in[i] = (int16_t)v[2 + i];
        memset(out, 0x5A, sizeof out);
        uint32_t err = 0xdeadbeefu;
        const bool ok = requant_block(in, kTab, (uint32_t)v[0], (uint32_t)v[1], out, &err);
        if (ok != (v[66] != 0)) return printf("R case %u: in range %d, the model has %lld\n", cases, (int)ok, v[66]), 1;
        if (ok) {
            for (int i = 0; i < 64; ++i)
                if (out[i] != v[67 + i]) return printf("R case %u: level[%d] = %d, the model has %lld\n", cases, i, out[i], v[67 + i]), 1;
            if (err != v[131]) return printf("R case %u: error %u, the model has %lld\n", cases, err, v[131]), 1;
        } else {
            for (int i = 0; i < 64; ++i)
                if (out[i] != 0x5A5A) return printf("R case %u: a block out of range was written\n", cases), 1;
        }
        ++cases;
    }
    fclose(f);
    return 0;
}

// Every step of both tables, every level whose c = level * 8 Q is inside kRequantCoefMost, both signs: above the threshold,
// the first candidate the level itself, the second one less; the level 0: below the threshold.  (And what qbias 0 would give.)
static int first_candidates(unsigned& cases) {
    const int32_t half = trellis_bias(kRequantQbias);
    if (half != (1 << 21)) return printf("the rounding term is %d\n", half), 1;
    unsigned long long swept = 0, floor_misses = 0;
    for (uint32_t comp = 0; comp < 2; ++comp)
        for (int i = 1; i < 64; ++i) {
            const int32_t q8 = 8 * kTab.q[comp][i];
            for (int32_t level = 1; level * q8 <= kRequantCoefMost; ++level)
                for (int sign = -1; sign <= 1; sign += 2) {
                    uint32_t a;
                    bool above;
                    const uint32_t n = trellis_candidates(sign * level * q8, kTab.qmat[comp][i], half, a, above);
                    if (!above || a != (uint32_t)level || n != (level >= 2 ? 2u : 1u))
                        return printf("comp %u position %d level %d: above %d, first candidate %u\n", comp, i, sign * level, (int)above, a), 1;
                    if (trellis_distortion(sign * level * q8, a, kTab.q[comp][i]) != -(level * q8) * (level * q8)) return printf("the distortion of the level itself\n"), 1;
                    trellis_candidates(sign * level * q8, kTab.qmat[comp][i], 0, a, above);
                    floor_misses += a != (uint32_t)level;
                    ++swept;
                }
            uint32_t a;
            bool above;
            trellis_candidates(0, kTab.qmat[comp][i], half, a, above);
            if (above || a != 1u) return printf("a zero above the threshold\n"), 1;
            if ((kRequantCoefMost / q8 + 1) * q8 <= kRequantCoefMost) return printf("the sweep's end\n"), 1;
        }
    printf("first candidates: %llu levels are their own first candidate at one half; %llu would not be at qbias 0\n", swept, floor_misses);
    if (!floor_misses) return printf("qbias 0 was expected to miss\n"), 1;
    ++cases;
    return 0;
}

// The walk again in 64 bits, written straight from amv_trellis_plan.h's text: the levels, and the largest and smallest sum
// it ever forms (as tests/c/trellis_plan_test.cc does for fdct outputs).
struct Wide { long long most, least, product; int level[64]; };   // product: the largest |c * qmat|
static Wide wide_block(const int16_t* c, uint32_t comp, uint32_t qbias, long long lambda) {
    Wide w{0, 0, 0, {0}};
    const uint8_t* len = kTab.len[comp];
    const long long bias = (long long)qbias << 14, t1 = (1ll << 22) - bias - 1;
    long long L[64];
    int last = 0;
    for (int i = 1; i < 64; ++i) {
        L[i] = (long long)c[i] * kTab.qmat[comp][i];
        if (llabs(L[i]) > t1) last = i;
    }
    if (!last) return w;
    long long score[66];
    int survivor[66], count = 1, run_tab[66], level_tab[66];
    score[1] = 0;
    survivor[0] = 1;
    auto seen = [&](long long s) { if (s > w.most) w.most = s; if (s < w.least) w.least = s; };
    for (int i = 1; i <= last; ++i) {
        long long cand[2];
        int n = 1;
        if (llabs(L[i]) > t1) {
            cand[0] = (llabs(L[i]) + bias) >> 22;
            if (cand[0] >= 2) cand[n++] = cand[0] - 1;
        } else {
            cand[0] = 1;
        }
        if (llabs(L[i]) > w.product) w.product = llabs(L[i]);
        long long best = kTrellisNoScore;
        for (int k = 0; k < n; ++k) {
            const long long ac = llabs((long long)c[i]), e = cand[k] * kTab.q[comp][i] * 8 - ac, d = e * e - ac * ac;
            seen(e * e);
            seen(ac * ac);
            for (int j = count - 1; j >= 0; --j) {
                const int run = i - survivor[j];
                const int nb = (int)trellis_nbits((uint32_t)cand[k]);
                const long long bits = (run >> 4) * len[0xF0] + len[((run & 15) << 4) | nb] + nb;
                const long long s = d + bits * lambda + score[survivor[j]];
                seen(s);
                seen(d + bits * lambda);
                if (s < best) { best = s; run_tab[i + 1] = run; level_tab[i + 1] = (int)(c[i] < 0 ? -cand[k] : cand[k]); }
            }
        }
        score[i + 1] = best;
        const long long slack = last > 27 ? lambda : 0;
        seen(best + slack);
        while (count && score[survivor[count - 1]] > best + slack) --count;
        survivor[count++] = i + 1;
    }
    long long best = kTrellisNoScore;
    int end = 1;
    for (int i = survivor[0]; i <= last + 1; ++i) {
        const long long s = score[i] + (i - 1 < 63 ? len[0x00] * lambda : 0);
        seen(s);
        if (s < best) { best = s; end = i; }
    }
    for (int i = end; i > 1; i -= run_tab[i] + 1) w.level[i - 1] = level_tab[i];
    return w;
}

static uint32_t rnd(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

// the largest level at position i whose c is inside kRequantCoefMost
static int level_most(uint32_t comp, int i) { return kRequantCoefMost / (8 * kTab.q[comp][i]); }

static unsigned long long energy_of(const int16_t* levels, uint32_t comp) {
    unsigned long long e = 0;
    for (int i = 1; i < 64; ++i) {
        const long long c = (long long)levels[i] * 8 * kTab.q[comp][i];
        e += (unsigned long long)(c * c);
    }
    return e;
}

// Blocks of levels at the edges: every position at its largest level as far as the energy cap allows (from the front, from the
// back, scattered), the rest small or zero; one coefficient at kRequantCoefMost's edge alone; random blocks in range.  At
// lambda 0, 1, 3481, the bound - 1 and the bound: requant_block gives the 64-bit walk's levels, lambda 0 the input itself, and
// no sum leaves int32 -- nor goes below minus the cap.
static int edges(unsigned& cases) {
    long long most = 0, least = 0;
    uint32_t seed = 4711u;
    const uint32_t lambdas[] = {0u, 1u, 3481u, kTrellisLambdaMax - 1u, kTrellisLambdaMax};
    unsigned long long fullest = 0;
    for (uint32_t comp = 0; comp < 2; ++comp)
        for (int kind = 0; kind < 8; ++kind) {
            int16_t in[64] = {0};
            in[0] = (int16_t)(kind & 1 ? kRequantDcMost : -kRequantDcMost);
            for (int step = 1; step < 64; ++step) {
                const int i = kind == 0 ? step : kind == 1 ? 64 - step : kind == 2 ? 1 + (step * 37) % 63 : step;
                const int sign = (rnd(seed) >> 16) & 1u ? -1 : 1;
                int level = 0;
                switch (kind) {
                case 0: case 1: case 2: level = level_most(comp, i); break;
                case 3: level = step == 1 || step == 63 ? level_most(comp, i) : 0; break;       // a run of 61 between two at the edge
                case 4: level = step % 17 == 0 ? level_most(comp, i) : 0; break;                // runs of 16
                case 5: level = (int)(rnd(seed) % (uint32_t)(level_most(comp, i) + 1)); break;
                case 6: level = 1; break;
                default: level = (rnd(seed) % 4u) ? 0 : (int)(rnd(seed) % (uint32_t)(level_most(comp, i) + 1)); break;
                }
                in[i] = (int16_t)(sign * level);
                while (energy_of(in, comp) > kRequantEnergyMost) in[i] = (int16_t)(in[i] < 0 ? in[i] + 1 : in[i] - 1);   // down to what the cap leaves
            }
            const unsigned long long energy = energy_of(in, comp);
            if (energy > fullest) fullest = energy;
            for (uint32_t lambda : lambdas) {
                int16_t c[64], out[64];
                TrellisPlainLine from{in}, line{c};
                if (!requant_scale_block(from, kTab.q[comp], line)) return printf("edge kind %d comp %u: not in range\n", kind, comp), 1;
                const Wide w = wide_block(c, comp, kRequantQbias, lambda);
                if (w.most > most) most = w.most;
                if (w.least < least) least = w.least;
                if (w.most >= kTrellisNoScore || w.least < INT32_MIN || w.least < -(long long)kRequantEnergyMost || w.product >= (1ll << 31))
                    return printf("edge kind %d comp %u lambda %u: a sum of %lld / %lld leaves the range\n", kind, comp, lambda, w.most, w.least), 1;
                uint32_t err;
                if (!requant_block(in, kTab, comp, lambda, out, &err)) return printf("edge: refused\n"), 1;
                unsigned long long want_err = 0;
                for (int i = 1; i < 64; ++i) {
                    if (out[i] != w.level[i]) return printf("edge kind %d comp %u lambda %u: level[%d] = %d, in 64 bits %d\n", kind, comp, lambda, i, out[i], w.level[i]), 1;
                    if (lambda == 0u && out[i] != in[i]) return printf("edge kind %d comp %u: lambda 0 changed level[%d]\n", kind, comp, i), 1;
                    if (in[i] ? abs(out[i]) > abs(in[i]) || abs(out[i]) + 1 < abs(in[i]) * (out[i] != 0) || (out[i] && (out[i] < 0) != (in[i] < 0)) : out[i] != 0 && out[i] != 1)
                        return printf("edge: level[%d] went from %d to %d\n", i, in[i], out[i]), 1;
                    const long long d = (long long)(out[i] - in[i]) * kTab.q[comp][i];
                    want_err += (unsigned long long)(d * d);
                }
                if (out[0] != in[0]) return printf("edge: the DC moved\n"), 1;
                if (want_err != err || want_err > kRequantBlockErrorMost) return printf("edge: the error %u, in 64 bits %llu\n", err, want_err), 1;
                ++cases;
            }
        }
    if (fullest * 16u < kRequantEnergyMost * 15u) return printf("the fullest block holds %llu of %llu\n", fullest, (unsigned long long)kRequantEnergyMost), 1;
    printf("edges: sums inside %lld .. %lld; the fullest block's energy %llu of %llu\n", least, most, fullest, (unsigned long long)kRequantEnergyMost);
    return 0;
}

// one step over each constant is refused, the constant itself is not
static int refusals(unsigned& cases) {
    for (uint32_t comp = 0; comp < 2; ++comp)
        for (int i = 1; i < 64; ++i)
            for (int sign = -1; sign <= 1; sign += 2) {
                int16_t in[64] = {0}, c[64];
                TrellisPlainLine from{in}, line{c};
                in[i] = (int16_t)(sign * level_most(comp, i));
                if (!requant_scale_block(from, kTab.q[comp], line) || c[i] != in[i] * 8 * kTab.q[comp][i]) return printf("the edge level at %d is refused\n", i), 1;
                in[i] = (int16_t)(sign * (level_most(comp, i) + 1));
                if (requant_scale_block(from, kTab.q[comp], line)) return printf("a level over the edge at %d is taken\n", i), 1;
                in[i] = (int16_t)(sign * 32767 - (sign < 0));
                if (requant_scale_block(from, kTab.q[comp], line)) return printf("the largest int16 at %d is taken\n", i), 1;
                ++cases;
            }
    int16_t in[64] = {0}, c[64];
    TrellisPlainLine from{in}, line{c};
    for (int dc : {-1024, 1024, -32768, 32767}) {
        in[0] = (int16_t)dc;
        if (requant_scale_block(from, kTab.q[0], line)) return printf("a DC of %d is taken\n", dc), 1;
    }
    for (int dc : {-1023, 0, 1023}) {
        in[0] = (int16_t)dc;
        if (!requant_scale_block(from, kTab.q[0], line) || c[0] != dc) return printf("a DC of %d is refused\n", dc), 1;
    }
    ++cases;
    return 0;
}

int main(int argc, char** argv) {
    unsigned cases = 0;
    if (argc > 1 && vectors(argv[1], cases)) return 1;
    if (first_candidates(cases)) return 1;
    if (edges(cases)) return 1;
    if (refusals(cases)) return 1;
    if (kRequantCoefMost != 8681 || kRequantEnergyMost != (1ull << 30) || kStRange != 8u) return printf("the constants\n"), 1;
    printf("ok %u\n", cases);
    return 0;
}
