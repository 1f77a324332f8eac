// adpcm_chain_plan_test.cc -- the ADPCM chains' host arithmetic (amv-codec-tools_amd/csrc/amv_host_plan.h: adpcm_trellis_tail
// and the one ChainPlan of both encoders) walked on the CPU.  Built with g++ by tests/test_adpcm_trellis_stream.py;
// prints "ok <cases>".
#include <stdio.h>

#include "amv_host_plan.h"

using namespace amv;

// the named counter words: all distinct, all inside the block, for every sweep count either encoder may launch
static int counters_ok() {
    bool used[kChainCounterWords] = {};
    auto take = [&](uint32_t w) {
        if (w >= kChainCounterWords || used[w]) return false;
        used[w] = true;
        return true;
    };
    // the plain route with s sweeps reads and appends generations 0 .. s + 2, the trellis stream generations 0 .. s + 1
    // and counts what sweeps 0 .. s - 1 coded again
    const uint32_t gens = (kAdpcmSweepsMost + 2u > kTrellisSweepsMost + 1u ? kAdpcmSweepsMost + 2u : kTrellisSweepsMost + 1u) + 1u;
    for (uint32_t k = 0; k < gens; ++k)
        if (!take(chain_word_list(k))) return 0;
    for (uint32_t k = 0; k < kTrellisSweepsMost; ++k)
        if (!take(chain_word_recoded(k))) return 0;
    return take(kChainWordNeed) && take(kChainWordDone);
}

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
    // the chain workspace, with and without the plain route's blocked composition: parts in order, none overlapping,
    // words aligned (state: 64-bit words), the counters, the bits and the maps complete, every offset computed in 64 bits
    const uint32_t ns[] = {1u, 2u, 63u, 64u, 65u, 127u, 128u, 129u, 255u, 256u, 257u, 300u, 57600u, 200000u, 0xffffffffu};
    for (uint32_t n : ns) {
        for (int blocked = 0; blocked < 2; ++blocked, ++cases) {
            const ChainPlan p = blocked ? adpcm_plain_chain_plan(n) : adpcm_trellis_chain_plan(n);
            const uint64_t n64 = n, blocks = (n64 + 255u) / 256u, bits = blocked ? (n64 + 127u) / 128u * 16u : 0u;   // (the front sweep is the plain route's)
            if (p.blocks != (blocked ? blocks : 0u)) return printf("blocks at n = %u\n", n), 1;
            if (p.state != 0u || p.list[0] < p.state + n64 * 8u || p.list[1] < p.list[0] + n64 * 4u || p.counters < p.list[1] + n64 * 4u ||
                p.bits < p.counters + kChainCounterWords * 4u || p.map < p.bits + bits || (blocked && bits * 8u < n64) || p.bmap < p.map + n64 * 96u ||
                p.bstart < p.bmap + (uint64_t)p.blocks * 96u || p.bytes < p.bstart + (uint64_t)p.blocks * 4u)
                return printf("plan overlaps at n = %u\n", n), 1;
            if (p.state & 7u) return printf("state alignment at n = %u\n", n), 1;
            if ((p.zero | p.zero_bytes) & 15u) return printf("zero span not whole 16-byte pieces at n = %u\n", n), 1;
            if ((p.list[0] | p.list[1] | p.counters | p.bits | p.map | p.bmap | p.bstart) & 3u) return printf("plan alignment at n = %u\n", n), 1;
            // what a call zeroes: exactly the counters and the bits, nothing of the state, the lists or the maps
            if (p.zero != p.counters || p.zero + p.zero_bytes != p.bits + bits || p.zero < p.list[1] + n64 * 4u || p.zero + p.zero_bytes > p.map)
                return printf("zero span at n = %u\n", n), 1;
            // no offset wrapped at 32 bits: the whole is what its parts add up to in 64-bit arithmetic
            if (p.bytes != n64 * (8u + 4u + 4u + 96u) + kChainCounterWords * 4u + bits + (blocked ? blocks * 100u : 0u))
                return printf("plan size at n = %u\n", n), 1;
        }
    }
    if (adpcm_plain_chain_plan(0xffffffffu).bytes <= 0xffffffffull * 112u) return printf("32-bit overflow\n"), 1;
    if (!counters_ok()) return printf("counter words\n"), 1;
    static_assert(kChainWordNeed < kChainCounterWords && kChainWordDone < kChainCounterWords, "counters");
    static_assert(chain_word_recoded(0) + kTrellisSweepsMost <= kChainWordNeed && chain_word_list(0) + kChainGenerations <= chain_word_recoded(0),
                  "counters");
    static_assert(kAdpcmSweepsMost + 2u < kChainGenerations && kTrellisSweepsMost + 1u < kChainGenerations, "a word per generation");
    static_assert(kTrellisSweeps <= kTrellisSweepsMost, "sweeps");
    static_assert(kChainBlock == 256u, "bmap and bstart are sized for blocks of 256 chunks");
    printf("ok %u\n", cases);
    return 0;
}
