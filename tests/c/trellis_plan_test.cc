// trellis_plan_test.cc -- the trellis stream's host arithmetic (amv-codec-tools_amd/csrc/amv_host_plan.h: adpcm_trellis_tail,
// adpcm_trellis_chain_plan) walked on the CPU.  Built with g++ by tests/test_adpcm_trellis_stream.py; prints "ok <cases>".
#include <stdio.h>

#include "amv_host_plan.h"

using namespace amv;

int main() {
    unsigned cases = 0;
    // the guess's tail: the whole chunk up to 256 samples, else from the last freeze point but one -- it starts on a
    // multiple of 128 samples of the chunk (the real search has just frozen there) and is 129 .. 256 samples long
    for (uint32_t m = 0; m <= 70000u; m += 2u, ++cases) {
        const uint32_t t = adpcm_trellis_tail(m);
        if (t > m) return printf("tail %u of %u\n", t, m), 1;
        if (m <= 256u ? t != m : ((m - t) % 128u != 0u || t < 129u || t > 256u)) return printf("tail %u of %u\n", t, m), 1;
    }
    if (adpcm_trellis_tail(1378u) != 226u) return printf("tail of 1378\n"), 1;
    // the chain workspace: parts in order, none overlapping, words aligned, the counters and the maps complete
    const uint32_t ns[] = {1u, 2u, 63u, 64u, 65u, 300u, 57600u, 0xffffffffu};
    for (uint32_t n : ns) {
        const TrellisChainPlan p = adpcm_trellis_chain_plan(n);
        const uint64_t n64 = n;
        if (p.state != 0u || p.list[0] < p.state + n64 * 8u || p.list[1] < p.list[0] + n64 * 4u || p.counters < p.list[1] + n64 * 4u ||
            p.map < p.counters + kTrellisCounterWords * 4u || p.bytes < p.map + n64 * 96u)
            return printf("plan overlaps at n = %u\n", n), 1;
        if ((p.list[0] | p.list[1] | p.counters | p.map) & 3u) return printf("plan alignment at n = %u\n", n), 1;
        ++cases;
    }
    static_assert(kTrellisNeedWord < kTrellisCounterWords && 64u + kTrellisSweepsMost <= kTrellisNeedWord, "counters");
    static_assert(kTrellisSweeps <= kTrellisSweepsMost, "sweeps");
    printf("ok %u\n", cases);
    return 0;
}
