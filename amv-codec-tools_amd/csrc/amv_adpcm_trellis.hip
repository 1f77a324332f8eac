// amv_adpcm_trellis.hip -- IMA ADPCM (AMV chunk layout) with the reference's `-trellis N` search, gfx950: chunks with
// their start indices given, and the chunks of a call as one stream (the step index chained on the device by the
// scheme of amv_adpcm_chain.h).
//
// Reference: AMVmuxer/ffmpeg/libavcodec/adpcm.c:287-443 (adpcm_compress_trellis, IMA branch) and :461-498 (AMV framing).
#include <atomic>

#include "amv_adpcm_chain.h"

namespace amv {

// The reference's trellis search (adpcm_compress_trellis, adpcm.c:287-443, IMA branch; `-trellis N`): a beam of the
// 2^N best decoder states (sorted by squared error, at most one per decoded sample value), three candidate nibbles
// around the plain quantiser's choice for the better half of the beam and one for the rest (:333,373-385), the best
// path frozen into the output every 128 samples (:405-417).  One lane per chunk; the beam lives in LDS
// ([field][buffer][slot][lane]: a lane's accesses never meet another lane's bank), the back-pointers
// (nibble | previous path << 4, 16 bits) in a workspace laid out [64 chunks][path][lane].
//
// trellis_chunk is the search of one chunk: cnt (even) samples at x from step index index0, the lane's beam at `beam`
// (the workgroup's LDS + lane), its back-pointers at my_paths (entry e at my_paths[e * 64]).  kCode: the nibbles go to
// d + 8 (the caller writes the header).  !kCode: the index the search ends on and nothing else -- that needs the
// frontier alone, so no back-pointer is kept and no byte stored (d, my_paths unused).  Returns the end index.
namespace {

constexpr uint32_t trellis_lds_bytes(uint32_t trellis) { return 5u * 2u * (1u << trellis) * 64u * 4u; }

// adpcm.c:465-466,479: le16 first sample, le16 step index, le32 sample count
__device__ __forceinline__ void trellis_header(uint8_t* __restrict__ d, int first, int index0, uint32_t cnt) {
    d[0] = (uint8_t)(first & 0xff); d[1] = (uint8_t)((first >> 8) & 0xff);
    d[2] = (uint8_t)index0; d[3] = 0;
    d[4] = (uint8_t)cnt; d[5] = (uint8_t)(cnt >> 8); d[6] = (uint8_t)(cnt >> 16); d[7] = (uint8_t)(cnt >> 24);
}

template <bool kCode>
__device__ __forceinline__ int trellis_chunk(const int16_t* __restrict__ x, uint32_t cnt, int index0, uint8_t* __restrict__ d,
                                             uint16_t* __restrict__ my_paths, uint32_t* __restrict__ beam, uint32_t F,
                                             const uint32_t* __restrict__ s_step) {
    // node fields: [field 0..3][buffer 0..1][slot][lane]; order of the two frontiers: [buffer][rank][lane]
    uint32_t* const f_ssd = beam;
    uint32_t* const f_smp = f_ssd + 2u * F * 64u;
    uint32_t* const f_stp = f_smp + 2u * F * 64u;
    uint32_t* const f_pth = f_stp + 2u * F * 64u;
    uint32_t* const f_ord = f_pth + 2u * F * 64u;
    auto at = [&](uint32_t* field, uint32_t buf, uint32_t slot) -> uint32_t& { return field[(buf * F + slot) * 64u]; };
    constexpr uint32_t kNone = 0xffffffffu;
    const int first = cnt ? x[0] : 0;
    // nodes[0] = {ssd 0, path 0, step, sample1 = the chunk's first sample} in buffer 1 (:309-316)
    at(f_ssd, 1, 0) = 0u; at(f_smp, 1, 0) = (uint32_t)first; at(f_stp, 1, 0) = (uint32_t)index0;
    if (kCode) at(f_pth, 1, 0) = 0u;
    for (uint32_t k = 0; k < F; ++k) { at(f_ord, 0, k) = k ? kNone : 0u; at(f_ord, 1, k) = kNone; }
    uint32_t cur = 0;          // which order array holds the current frontier (its nodes live in buffer (i & 1) ^ 1)
    uint32_t pathn = 0;
    int froze = -1;
    auto put_nibble = [&](uint32_t k, uint32_t nib) {   // sample k's nibble: high half of its byte first (:485-486)
        uint8_t* b = d + 8u + (k >> 1);
        *b = (k & 1u) ? (uint8_t)((*b & 0xf0u) | nib) : (uint8_t)((*b & 0x0fu) | (nib << 4));
    };
    for (uint32_t i = 0; i < cnt; ++i) {
        const uint32_t nb = i & 1u, ob = nb ^ 1u, nxt = cur ^ 1u;
        const int sample = x[i];
        uint32_t made = 0, nn = 0;     // nodes allocated in buffer nb; entries of the next frontier
        for (uint32_t k = 0; k < F; ++k) at(f_ord, nxt, k) = kNone;
        for (uint32_t j = 0; j < F; ++j) {
            const uint32_t src = at(f_ord, cur, j);
            if (src == kNone) break;
            const int range = j < F / 2u ? 1 : 0;                                   // :333
            const int step = (int)at(f_stp, ob, src), st = (int)s_step[step];
            const int predictor = (int)at(f_smp, ob, src);
            const uint32_t base_ssd = at(f_ssd, ob, src), src_path = kCode ? at(f_pth, ob, src) : 0u;
            const int div = (sample - predictor) * 4 / st;                         // :376
            int nmin = min(max(div - range, -7), 6), nmax = min(max(div + range, -6), 7);
            if (nmin <= 0) --nmin;                                                   // distinguish -0 from +0
            if (nmax < 0) --nmax;
            for (int nidx = nmin; nidx <= nmax; ++nidx) {
                const uint32_t nibble = (uint32_t)(nidx < 0 ? 7 - nidx : nidx);
                const int look = (nibble & 8u) ? -(int)(2u * (nibble & 7u) + 1u) : (int)(2u * (nibble & 7u) + 1u);
                const int dec = clip16(predictor + (st * look) / 8);
                const int diff = sample - dec;
                const uint32_t ssd = base_ssd + (uint32_t)(diff * diff);
                if (nn == F && ssd >= at(f_ssd, nb, at(f_ord, nxt, F - 1u))) continue;   // :342
                bool dup = false;                                                    // one state per decoded value, :347-352
                for (uint32_t k = 0; k < nn; ++k) dup = dup || (int)at(f_smp, nb, at(f_ord, nxt, k)) == dec;
                if (dup) continue;
                uint32_t k = 0;
                while (k < nn && ssd >= at(f_ssd, nb, at(f_ord, nxt, k))) ++k;       // first rank it beats (:353-354)
                uint32_t u;
                if (nn == F) {
                    u = at(f_ord, nxt, F - 1u);                                      // the worst one makes room, its path id stays
                } else {
                    u = made++;
                    if (kCode) at(f_pth, nb, u) = pathn++;
                    ++nn;
                }
                at(f_ssd, nb, u) = ssd;
                at(f_stp, nb, u) = (uint32_t)clip_index(step + kImaIndexAdjust[nibble]);
                at(f_smp, nb, u) = (uint32_t)dec;
                if (kCode) my_paths[(uint64_t)at(f_pth, nb, u) * 64u] = (uint16_t)(nibble | (src_path << 4));
                for (uint32_t m = nn - 1u; m > k; --m) at(f_ord, nxt, m) = at(f_ord, nxt, m - 1u);   // memmove, :365
                at(f_ord, nxt, k) = u;
            }
        }
        cur = nxt;
        const uint32_t best = at(f_ord, cur, 0);
        if (at(f_ssd, nb, best) > (1u << 28)) {                                     // :398-402
            const uint32_t off = at(f_ssd, nb, best);
            for (uint32_t j = 1; j < F; ++j) {
                const uint32_t q = at(f_ord, cur, j);
                if (q == kNone) break;
                at(f_ssd, nb, q) -= off;
            }
            at(f_ssd, nb, best) = 0u;
        }
        if ((int)i == froze + 128) {                                                // :405-417
            if (kCode) {
                uint32_t p = at(f_pth, nb, best);
                for (int k = (int)i; k > froze; --k) {
                    const uint32_t e = my_paths[(uint64_t)p * 64u];
                    put_nibble((uint32_t)k, e & 15u);
                    p = e >> 4;
                }
            }
            froze = (int)i;
            pathn = 0;
            for (uint32_t j = 1; j < F; ++j) at(f_ord, cur, j) = kNone;
        }
    }
    if (cnt == 0u) return index0;
    const uint32_t nb = (cnt - 1u) & 1u, best = at(f_ord, cur, 0);
    if (kCode) {
        uint32_t p = at(f_pth, nb, best);
        for (int k = (int)cnt - 1; k > froze; --k) {
            const uint32_t e = my_paths[(uint64_t)p * 64u];
            put_nibble((uint32_t)k, e & 15u);
            p = e >> 4;
        }
    }
    return (int)at(f_stp, nb, best);                                                 // :429
}

// chunk i of a stream coded from `start` (0..88): header, nibbles; returns the end index
__device__ __forceinline__ int trellis_code(const int16_t* __restrict__ pcm, const uint64_t* __restrict__ pcm_offs,
                                            const uint32_t* __restrict__ nsamp, uint8_t* __restrict__ blob,
                                            const uint64_t* __restrict__ offs, uint32_t i, int start, uint16_t* __restrict__ my_paths,
                                            uint32_t* __restrict__ beam, uint32_t F, const uint32_t* __restrict__ s_step) {
    const int16_t* x = pcm + pcm_offs[i];
    const uint32_t cnt = nsamp[i] & ~1u;
    uint8_t* d = blob + offs[i];
    trellis_header(d, cnt ? x[0] : 0, start, cnt);
    return trellis_chunk<true>(x, cnt, start, d, my_paths, beam, F, s_step);
}

// the back-pointers of a workgroup's 64 lanes: [workgroup of the LAUNCH][path][lane] -- by position in the launch, not by
// chunk, so a sweep over a short list needs the first workgroups' space only
__device__ __forceinline__ uint16_t* trellis_paths(uint16_t* __restrict__ paths, uint32_t F) {
    return paths + (uint64_t)blockIdx.x * (F * 128u) * 64u + threadIdx.x;
}

}  // namespace

// Chunks are independent: the step index comes in per chunk and goes out per chunk.
__global__ __launch_bounds__(64) void amv_adpcm_trellis_kernel(
    const int16_t* __restrict__ pcm, const uint64_t* __restrict__ pcm_offs, const uint32_t* __restrict__ nsamp, uint32_t n,
    const int32_t* __restrict__ step_in, uint32_t trellis, uint8_t* __restrict__ blob, const uint64_t* __restrict__ offs,
    int32_t* __restrict__ step_out, uint16_t* __restrict__ paths) {
    extern __shared__ uint32_t s_trellis[];
    __shared__ uint32_t s_step[96];
    load_steps(s_step);
    const uint32_t F = 1u << trellis, lane = threadIdx.x;
    const uint32_t i_chunk = blockIdx.x * 64u + lane;
    if (i_chunk >= n) return;                         // (no barrier follows)
    const int end = trellis_code(pcm, pcm_offs, nsamp, blob, offs, i_chunk, clip_index(step_in[i_chunk]), trellis_paths(paths, F),
                                 s_trellis + lane, F, s_step);
    if (step_out) step_out[i_chunk] = end;
}

// ---- the trellis stream: the step index chained on the device ---------------------------------------------------------
// The chunks of a call are one stream (adpcm.c:461-498 with -trellis): chunk 0 starts from the index handed in, chunk i
// from the index chunk i - 1 ends on; nothing else crosses a chunk boundary (:464 takes the predictor from the chunk's
// first sample).  The scheme of amv_adpcm_chain.h, with launches as the only synchronisation -- a trellis chunk is
// milliseconds of one lane's time, so what an in-launch hand-off could save does not show:
//   guess   every chunk coded from a guessed start (chunk 0: the given index; the others: the ends-only search over the
//           end of the chunk before, adpcm_trellis_tail), state[i] = {start used, end reached};
//   link    lists the chunks whose predecessor ended elsewhere than they assumed;
//   sweep   (a fixed number of launches) one lane per listed chunk: coded again from its predecessor's end if that is not
//           the start it used; its successor is listed if its own end moved.  An empty list ends the launch at once;
//   link    again, as the check (chain_broken): the first chunk it finds wrong -- everything before it is final, whatever
//           the data -- sends the chunks from there on down the fall-back:
//   map     the ends-only search of each of those chunks from all 89 starts (a lane per (chunk, start)),
//   walk    one workgroup composes the maps along the stream from the last final end: state[i] = the true {start, end},
//   recode  those chunks coded from their true starts.
__global__ __launch_bounds__(64) void amv_adpcm_trellis_guess_kernel(
    const int16_t* __restrict__ pcm, const uint64_t* __restrict__ pcm_offs, const uint32_t* __restrict__ nsamp, uint32_t n,
    uint32_t first_index, uint32_t trellis, uint8_t* __restrict__ blob, const uint64_t* __restrict__ offs, uint2* __restrict__ state,
    uint16_t* __restrict__ paths) {
    extern __shared__ uint32_t s_trellis[];
    __shared__ uint32_t s_step[96];
    load_steps(s_step);
    const uint32_t F = 1u << trellis, lane = threadIdx.x;
    const uint32_t i = blockIdx.x * 64u + lane;
    if (i >= n) return;
    int start = (int)first_index;
    if (i > 0u) {
        const uint32_t mp = nsamp[i - 1u] & ~1u, tail = adpcm_trellis_tail(mp);
        start = trellis_chunk<false>(pcm + pcm_offs[i - 1u] + (mp - tail), tail, 0, nullptr, nullptr, s_trellis + lane, F, s_step);
    }
    const int end = trellis_code(pcm, pcm_offs, nsamp, blob, offs, i, start, trellis_paths(paths, F), s_trellis + lane, F, s_step);
    state[i] = make_uint2((uint32_t)start, (uint32_t)end);
}

// The chunks that break the chain (chain_broken; chunk 0 starts from the index handed in): listed (list != nullptr), and
// *need = n - the first of them (need != nullptr; zero before: the stream is the sequential encoder's).  force: the
// test knob's fall-back at once -- nothing is coded yet, so all n chunks are the fall-back's.
__global__ __launch_bounds__(256) void amv_adpcm_trellis_link_kernel(const uint2* __restrict__ state, uint32_t n, uint32_t first_index,
                                                                    const uint8_t* __restrict__ blob, const uint64_t* __restrict__ offs,
                                                                    uint32_t* __restrict__ list, uint32_t* __restrict__ count,
                                                                    uint32_t* __restrict__ need, uint32_t force) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (force) {
        if (i == 0u) *need = n;
        return;
    }
    const bool bad = i < n && chain_broken(state, i, first_index, blob, offs);
    if (list) list_wrong(bad, i, list, count);
    if (need) note_broken(bad, i, n, need);
}

__global__ __launch_bounds__(64) void amv_adpcm_trellis_sweep_kernel(
    const int16_t* __restrict__ pcm, const uint64_t* __restrict__ pcm_offs, const uint32_t* __restrict__ nsamp, uint32_t n,
    uint32_t trellis, uint8_t* __restrict__ blob, const uint64_t* __restrict__ offs, uint2* __restrict__ state,
    const uint32_t* __restrict__ list_in, const uint32_t* __restrict__ count_in, uint32_t* __restrict__ list_out,
    uint32_t* __restrict__ count_out, uint32_t* __restrict__ recoded, uint16_t* __restrict__ paths) {
    extern __shared__ uint32_t s_trellis[];
    __shared__ uint32_t s_step[96];
    const uint32_t count = *count_in;
    if (blockIdx.x * 64u >= count) return;
    load_steps(s_step);
    const uint32_t F = 1u << trellis, lane = threadIdx.x;
    if (blockIdx.x * 64u + lane >= count) return;
    const uint32_t i = list_in[blockIdx.x * 64u + lane];
    // The path pointer is made HERE, ahead of sweep_todo, on purpose.  The search inlined below is the same instruction
    // sequence either way, but where this line stands decides the registers hipcc gives it, and the kernel is one lone
    // wave's serial chain: with trellis_paths(paths, F) written in the call below, as the other kernels have it, the
    // stream call of 1000 x 1378 samples at N = 3 took 333 ms instead of 323 (the parent's form: 327), all of it in this
    // kernel by a kernel trace (MI355X; this form's figures: profiles/r14_adpcm_chain_refactor.jsonl).  Time the stream
    // call before moving it.
    uint16_t* my_paths = trellis_paths(paths, F);
    uint32_t start;
    if (!sweep_todo(state, i, start)) return;                       // coded from there already
    const uint32_t end = (uint32_t)trellis_code(pcm, pcm_offs, nsamp, blob, offs, i, (int)start, my_paths, s_trellis + lane, F, s_step);
    atomicAdd(recoded, 1u);
    sweep_publish(state, n, i, start, end, list_out, count_out);
}

// the fall-back (every kernel of it leaves at once while *need is zero): chunks n - *need .. n - 1
__global__ __launch_bounds__(64) void amv_adpcm_trellis_map_kernel(
    const int16_t* __restrict__ pcm, const uint64_t* __restrict__ pcm_offs, const uint32_t* __restrict__ nsamp, uint32_t n,
    uint32_t trellis, uint8_t* __restrict__ map /* [n][96] */, const uint32_t* __restrict__ need) {
    extern __shared__ uint32_t s_trellis[];
    __shared__ uint32_t s_step[96];
    const uint32_t left = *need;
    if (left == 0u) return;
    load_steps(s_step);
    const uint32_t F = 1u << trellis, lo = n - left;
    const uint64_t pairs = (uint64_t)left * 89u;
    for (uint64_t pair = (uint64_t)blockIdx.x * 64u + threadIdx.x; pair < pairs; pair += (uint64_t)gridDim.x * 64u) {
        const uint32_t i = lo + (uint32_t)(pair / 89u), s = (uint32_t)(pair % 89u);
        const int end = trellis_chunk<false>(pcm + pcm_offs[i], nsamp[i] & ~1u, (int)s, nullptr, nullptr, s_trellis + threadIdx.x, F, s_step);
        map[(uint64_t)i * 96u + s] = (uint8_t)end;
    }
}

// one workgroup: the maps of kChainBlock chunks at a time, walked from the last final end
__global__ __launch_bounds__(128) void amv_adpcm_trellis_walk_kernel(const uint8_t* __restrict__ map, uint32_t n, uint32_t first_index,
                                                                    uint2* __restrict__ state, const uint32_t* __restrict__ need) {
    __shared__ uint32_t s_map[kChainBlock * 24u];
    const uint32_t left = *need;
    if (left == 0u) return;
    const uint32_t lo = n - left;
    uint32_t v = lo ? state[lo - 1u].y : first_index;
    for (uint32_t t0 = lo; t0 < n; t0 += kChainBlock)
        v = walk_maps<128u, false>(s_map, map + (uint64_t)t0 * 96u, min(kChainBlock, n - t0), 1u, v,
                                   [&](uint32_t c, uint32_t from, uint32_t to) { state[t0 + c] = make_uint2(from, to); });
}

__global__ __launch_bounds__(64) void amv_adpcm_trellis_recode_kernel(
    const int16_t* __restrict__ pcm, const uint64_t* __restrict__ pcm_offs, const uint32_t* __restrict__ nsamp, uint32_t n,
    uint32_t trellis, uint8_t* __restrict__ blob, const uint64_t* __restrict__ offs, const uint2* __restrict__ state,
    const uint32_t* __restrict__ need, uint16_t* __restrict__ paths) {
    extern __shared__ uint32_t s_trellis[];
    __shared__ uint32_t s_step[96];
    const uint32_t left = *need;
    if (blockIdx.x * 64u >= left) return;
    load_steps(s_step);
    const uint32_t F = 1u << trellis, lane = threadIdx.x;
    if (blockIdx.x * 64u + lane >= left) return;
    const uint32_t i = n - left + blockIdx.x * 64u + lane;
    trellis_code(pcm, pcm_offs, nsamp, blob, offs, i, (int)state[i].x, trellis_paths(paths, F), s_trellis + lane, F, s_step);
}

__global__ __launch_bounds__(256) void amv_adpcm_trellis_ends_kernel(const uint2* __restrict__ state, uint32_t n, int32_t* __restrict__ step_out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) step_out[i] = (int32_t)state[i].y;
}

// workspace of launch_adpcm_trellis: bytes for n chunks
uint64_t adpcm_trellis_workspace(uint32_t n, uint32_t trellis) {
    return (uint64_t)((n + 63u) / 64u) * 64u * ((1u << trellis) * 128u) * sizeof(uint16_t);
}

// the search kernels' LDS is dynamic and above the 64 KB a kernel gets unasked at N = 5: raised once per device and kernel
template <typename K>
static bool trellis_lds_raised(K kernel, std::atomic<uint64_t>& raised) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (raised.load() & (1ull << (dev & 63))) return true;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)trellis_lds_bytes(5)) !=
        hipSuccess)
        return false;
    raised.fetch_or(1ull << (dev & 63));
    return true;
}

bool launch_adpcm_trellis(const int16_t* pcm, const uint64_t* pcm_offs, const uint32_t* nsamp, uint32_t n, const int32_t* step_in,
                          uint32_t trellis, uint8_t* blob, const uint64_t* offs, int32_t* step_out, uint16_t* paths, hipStream_t s) {
    if (n == 0) return true;
    static std::atomic<uint64_t> raised{0};
    if (!trellis_lds_raised(amv_adpcm_trellis_kernel, raised)) return false;
    hipLaunchKernelGGL(amv_adpcm_trellis_kernel, dim3((n + 63) / 64), dim3(64), trellis_lds_bytes(trellis), s, pcm, pcm_offs, nsamp, n,
                       step_in, trellis, blob, offs, step_out, paths);
    return true;
}

// The trellis stream.  paths: adpcm_trellis_workspace(n, trellis) bytes; work: adpcm_trellis_chain_plan(n).bytes.
// sweeps < 0: the fall-back at once.  The launches are the same whatever n and the samples: the memset of the plan's
// zero span, guess, link, `sweeps` sweeps, link, map, walk, recode (and the copy of the ends when step_out is given).
bool launch_adpcm_trellis_stream(const int16_t* pcm, const uint64_t* pcm_offs, const uint32_t* nsamp, uint32_t n, uint32_t first_index,
                                 uint32_t trellis, uint8_t* blob, const uint64_t* offs, int32_t* step_out, uint16_t* paths, void* work,
                                 int sweeps, hipStream_t s) {
    if (n == 0) return true;
    static std::atomic<uint64_t> raised[4];
    if (!trellis_lds_raised(amv_adpcm_trellis_guess_kernel, raised[0]) || !trellis_lds_raised(amv_adpcm_trellis_sweep_kernel, raised[1]) ||
        !trellis_lds_raised(amv_adpcm_trellis_map_kernel, raised[2]) || !trellis_lds_raised(amv_adpcm_trellis_recode_kernel, raised[3]))
        return false;
    const ChainPlan p = adpcm_trellis_chain_plan(n);
    uint8_t* w = static_cast<uint8_t*>(work);
    uint2* state = reinterpret_cast<uint2*>(w + p.state);
    uint32_t* list[2] = {reinterpret_cast<uint32_t*>(w + p.list[0]), reinterpret_cast<uint32_t*>(w + p.list[1])};
    uint32_t* count = reinterpret_cast<uint32_t*>(w + p.counters);
    uint32_t* need = count + kChainWordNeed;
    uint8_t* map = w + p.map;
    if (hipMemsetAsync(w + p.zero, 0, p.zero_bytes, s) != hipSuccess) return false;   // (nothing has been queued)
    const uint32_t lds = trellis_lds_bytes(trellis), groups = (n + 63u) / 64u, links = (n + 255u) / 256u;
    if (sweeps >= 0) {
        if ((uint32_t)sweeps > kTrellisSweepsMost) sweeps = (int)kTrellisSweepsMost;
        hipLaunchKernelGGL(amv_adpcm_trellis_guess_kernel, dim3(groups), dim3(64), lds, s, pcm, pcm_offs, nsamp, n, first_index, trellis, blob,
                           offs, state, paths);
        hipLaunchKernelGGL(amv_adpcm_trellis_link_kernel, dim3(links), dim3(256), 0, s, state, n, first_index, blob, offs, list[0],
                           count + chain_word_list(0), nullptr, 0u);
        for (uint32_t k = 0; k < (uint32_t)sweeps; ++k)
            hipLaunchKernelGGL(amv_adpcm_trellis_sweep_kernel, dim3(groups), dim3(64), lds, s, pcm, pcm_offs, nsamp, n, trellis, blob, offs,
                               state, list[k & 1u], count + chain_word_list(k), list[(k + 1u) & 1u], count + chain_word_list(k + 1u),
                               count + chain_word_recoded(k), paths);
    }
    hipLaunchKernelGGL(amv_adpcm_trellis_link_kernel, dim3(links), dim3(256), 0, s, state, n, first_index, blob, offs, nullptr, nullptr,
                       need, sweeps < 0 ? 1u : 0u);
    const uint64_t map_groups = ((uint64_t)n * 89u + 63u) / 64u;
    hipLaunchKernelGGL(amv_adpcm_trellis_map_kernel, dim3((uint32_t)(map_groups < 8192u ? map_groups : 8192u)), dim3(64), lds, s, pcm, pcm_offs,
                       nsamp, n, trellis, map, need);
    hipLaunchKernelGGL(amv_adpcm_trellis_walk_kernel, dim3(1), dim3(128), 0, s, map, n, first_index, state, need);
    hipLaunchKernelGGL(amv_adpcm_trellis_recode_kernel, dim3(groups), dim3(64), lds, s, pcm, pcm_offs, nsamp, n, trellis, blob, offs, state,
                       need, paths);
    if (step_out) hipLaunchKernelGGL(amv_adpcm_trellis_ends_kernel, dim3(links), dim3(256), 0, s, state, n, step_out);
    return true;
}

}  // namespace amv
