// amv_adpcm_chain.h -- what the ADPCM coders share on the device (amv_adpcm.hip, amv_adpcm_trellis.hip): the clips and the
// step table, and the pieces of the ONE scheme by which both encoders carry the reference's step_index from chunk to
// chunk (adpcm.c:461-498) without a serial pass over the stream.  The workspace those pieces work on is ChainPlan's
// (amv_host_plan.h).
//
// The scheme: every chunk is coded from a guessed start and notes in state[i] the start it used and the end it reached.
// The chunks whose start is not their predecessor's end are listed; a sweep codes a listed chunk again from its
// predecessor's end (unless it was coded from there already) and lists its successor if its own end moved.  Chunk 0
// starts from the true index, so after k sweeps the first k chunks are final whatever the data.  Behind the sweeps a
// check looks at every chunk once more, and what it finds wrong goes down an exhaustive route that needs no guess,
// because step_index has only 89 values: every chunk is run from all 89 starts (state only) into a 96-byte map, and the
// maps are walked along the stream.
#pragma once
#include "amv_host_plan.h"
#include "amv_kernels.h"

namespace amv {

__device__ __forceinline__ int clip16(int v) { return min(max(v, -32768), 32767); }
__device__ __forceinline__ int clip_index(int v) { return min(max(v, 0), 88); }

// the step table in LDS (indexed per lane on the critical path; a constant-memory table would be a
// dependent global load per sample)
__device__ __forceinline__ void load_steps(uint32_t* s_step) {
    for (uint32_t i = threadIdx.x; i < 89u; i += blockDim.x) s_step[i] = (uint32_t)kImaStep[i];
    __syncthreads();
}

// device words with agent scope: what one lane stores another lane of the same launch may read (never torn, possibly
// the value before -- the sweeps are written for that)
__device__ __forceinline__ uint32_t peek(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void poke(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// state[i] = {start the chunk's bytes were coded from, end reached from it}, replaced as ONE 64-bit word so that no reader
// and no second writer ever sees one chunk's start beside another coding's end; returns the end that was there.  Whoever
// changes a chunk's end lists its successor: that rule, and a listed chunk being coded again whenever its start is not its
// predecessor's end, is all the sweeps rest on.
__device__ __forceinline__ uint32_t swap_state(uint2* p, uint32_t start, uint32_t end) {
    const uint64_t old = __hip_atomic_exchange(reinterpret_cast<uint64_t*>(p), (uint64_t)start | (uint64_t)end << 32, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT);
    return (uint32_t)(old >> 32);
}

// The lanes of a wave that are `wrong` append their chunk i to the list: one atomicAdd per wave, the entries in lane
// order.  Every lane of the wave comes here.
__device__ __forceinline__ void list_wrong(bool wrong, uint32_t i, uint32_t* __restrict__ list, uint32_t* __restrict__ count) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t mask = __ballot(wrong);
    if (mask) {
        uint32_t base = 0;
        if (lane == 0u) base = atomicAdd(count, (uint32_t)__popcll(mask));
        base = (uint32_t)__shfl((int)base, 0);
        if (wrong) list[base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = i;
    }
}

// A sweep's step, first half: is the listed chunk i (never chunk 0: nobody lists it) still to do -- its predecessor's
// end is not the start it was coded from -- and from which start.  The predecessor may be in the same list, and another
// lane of the same launch may be replacing its end: the lane gets the old end or the new one, never waits, and is listed
// again by that lane if the end did move -- so the chunk is coded from the new end in the next sweep unless it already was.
__device__ __forceinline__ bool sweep_todo(const uint2* state, uint32_t i, uint32_t& start) {
    const uint32_t* sw = reinterpret_cast<const uint32_t*>(state);
    start = peek(sw + 2u * (i - 1u) + 1u);
    return start != peek(sw + 2u * i);
}

// ... second half: chunk i has been coded from `start` and ended on `end`; if that end is not the one that was there,
// the successor is listed for the next sweep.  A chunk is listed by its predecessor only, so no list holds it twice,
// and only the lane that holds it writes its state and its bytes.
__device__ __forceinline__ void sweep_publish(uint2* state, uint32_t n, uint32_t i, uint32_t start, uint32_t end,
                                              uint32_t* __restrict__ list_out, uint32_t* __restrict__ count_out) {
    if (swap_state(state + i, start, end) != end && i + 1u < n) list_out[atomicAdd(count_out, 1u)] = i + 1u;
}

// The chain's check of chunk i.  Every chunk's bytes were coded from the start its state names (states are replaced
// whole), so the stream is the sequential encoder's if and only if every chunk's start is its predecessor's end (chunk 0:
// `first`).  And the BYTES are looked at, not only the states: the step index in a chunk's header (adpcm.c:466, byte 2) is
// the start its nibbles were coded from by whichever lane wrote it last -- a chunk two lanes coded at once from different
// readings of its predecessor's end can carry a header that is not its state's start, and a state that is only a
// prediction (a start above 88) has no bytes at all and never equals a byte.  (Every chunk has a header, also one of no
// samples.)
__device__ __forceinline__ bool chain_broken(const uint2* __restrict__ state, uint32_t i, uint32_t first, const uint8_t* __restrict__ blob,
                                             const uint64_t* __restrict__ offs) {
    const uint32_t start = state[i].x;
    return start != (i ? state[i - 1u].y : first) || (uint32_t)blob[offs[i] + 2u] != start;
}

// ... and its verdict: *need = n - the first broken chunk (it stays zero when there is none).  Everything before that
// chunk is final, whatever the data; the exhaustive routes run when *need is not zero.  Every lane of the wave comes here.
__device__ __forceinline__ void note_broken(bool broken, uint32_t i, uint32_t n, uint32_t* __restrict__ need) {
    const uint64_t mask = __ballot(broken);
    if (broken && (mask & ((1ull << (threadIdx.x & 63u)) - 1ull)) == 0ull) atomicMax(need, n - i);   // the wave's first
}

// The exhaustive routes' walk: cnt 96-byte maps (map[c][s] = where chunk c ends when it starts from s) are copied into
// LDS (24 cnt words at s_map) by the workgroup's kThreads lanes, then its first `walkers` lanes walk them, each from its
// own v: step(c, v, e) is told that chunk c of the tile starts from v and ends on e.  Returns where the walk ends (to the
// lanes that walked).  kPeek: the maps were stored by other workgroups of this launch, so they are read past this CU's L1.
template <uint32_t kThreads, bool kPeek, typename Step>
__device__ __forceinline__ uint32_t walk_maps(uint32_t* s_map, const uint8_t* __restrict__ maps, uint32_t cnt, uint32_t walkers, uint32_t v,
                                              Step step) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(maps);
    __syncthreads();                                 // the tile before has been walked
    for (uint32_t k = threadIdx.x; k < cnt * 24u; k += kThreads) s_map[k] = kPeek ? peek(src + k) : src[k];
    __syncthreads();
    if (threadIdx.x < walkers) {
        const uint8_t* m8 = reinterpret_cast<const uint8_t*>(s_map);
        for (uint32_t c = 0; c < cnt; ++c) {
            const uint32_t e = m8[c * 96u + v];
            step(c, v, e);
            v = e;
        }
    }
    return v;
}

}  // namespace amv
