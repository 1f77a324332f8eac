// amv_block_load.h -- stage A of the reconstruction kernels: one 8x8 block of quantised coefficients per lane.
//
// A wave owns an MCU-row segment of `cnt` MCUs (<= 10, i.e. <= 60 blocks).  Lane b ends up with block b's 64
// coefficients (scan order, int16 pairs in 32 dwords): from its dense 128-byte line, or -- records form -- after
// the wave has scattered the segment's (block, index, value) records into a zeroed LDS image of the blocks (16-byte
// granules XOR-swizzled by the record's block field so that the per-lane 128-byte reads do not collide on banks) and
// added the DC base of the entropy lane that decoded the block (SyncSinks::lane_tab).
// Around it, the frame the reconstruction kernels share: select_frame, segment_of, next_item, launch_segments.
#pragma once
#include <cstdlib>

#include "amv_kernels.h"
#include "amv_piece_map.h"

namespace amv {

constexpr uint32_t kSegImageBytes = 60u * 128u;   // the LDS image of a segment's <= 60 blocks; 128 spare bytes follow it
// the scatter's numbers (tests/test_scatter_model.py restates the arithmetic on them)
constexpr uint32_t kScatterSwizzleMask = 0x38u;     // (word >> 3) & this: the block field's low three bits over the index's granule bits
constexpr uint32_t kScatterFieldShift = 6u;         // the block field's place in the word
constexpr uint32_t kScatterAddressMask = 0x11ffeu;  // doubled word: byte offset (1-6), block in segment (7-12), filler (16)

// A segment belongs to one wave and so does its LDS: what one lane wrote another lane of the same wave may read once
// the wave has passed this point (a wave's LDS operations are served in order; the fence keeps the compiler from
// moving them across).  No workgroup barrier: the waves of a workgroup work on segments of their own.
__device__ __forceinline__ void seg_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// Which frame this workgroup works on: work item `item` of the launch (FrameSel); false when there is none (past
// the end of a round's work).  slot: where the frame's dense lines live, if it has any.  A default launch has one
// item per workgroup (blockIdx.x); a round launch is small and its workgroups walk the round's items.
__device__ __forceinline__ bool select_frame(const FrameSel& sel, uint32_t n, uint32_t item, uint32_t& f, uint32_t& slot) {
    f = slot = item;
    if (!sel.round) return true;
    const uint32_t p = sel.base + item;
    if (item >= sel.round || p >= (sel.count ? *sel.count : n)) return false;
    f = sel.list ? sel.list[p] : p;
    return true;
}

// The segment a wave works on: the WAVE's, the same in every lane -- wave-uniform by contract.  The scatter keeps what it
// derives from it in scalar registers; a caller whose (item, my, seg) come from threadIdx loses nothing but those.
struct Segment {
    uint32_t f, slot;                    // the frame; where its dense lines live, if it has any (select_frame)
    uint32_t m0, cnt, ok, mcu0;          // first MCU column; MCUs (<= kSegMcus); nmcu_ok[f]; first MCU, counted in the frame
    uint32_t segidx, nsegs;              // the segment's number in the frame (my * nseg + seg); segments per frame
};
// segment `seg` (of nseg) of MCU row `my` of the frame select_frame gave
__device__ __forceinline__ Segment segment_of(uint32_t f, uint32_t slot, const uint32_t* __restrict__ nmcu_ok, const FrameGeom& g,
                                              uint32_t nseg, uint32_t my, uint32_t seg) {
    const uint32_t m0 = seg * kSegMcus;
    return {f, slot, m0, min(kSegMcus, g.mcu_cols - m0), nmcu_ok[f], my * g.mcu_cols + m0, my * nseg + seg, g.mcu_rows * nseg};
}
// The item loop of a kernel: `do { select_frame or return; segment_of; ... } while (next_item<kRound>(pm, item));`.  A
// default launch has one item per workgroup; the workgroups of a round launch walk on, the segment's LDS free again.
template <bool kRound>
__device__ __forceinline__ bool next_item(const PieceMap& pm, uint32_t& item) {
    if (!kRound) return false;
    seg_sync();
    item += piece_stride(pm);
    return true;
}

// Stage A comes in two steps, so that a kernel with more than one reader of the coefficients can fetch them where it
// reads them: stage_segment_blocks brings a records frame's segment into LDS and says what form the frame has,
// fetch_block loads the lane's block from wherever it is.  load_segment_blocks is the two in a row.
// records, small_ac: wave-uniform.  small_ac: a records frame without the entropy stage's mark (kRecCountBigAc) -- every
// AC of it has at most nine magnitude bits, |value| <= 511.  Dense lines promise nothing.
struct BlockForm { bool records, small_ac; int dc_base; };

// s_img: kSegImageBytes + 128 bytes of LDS, 16-byte aligned; the caller may reuse it after a seg_sync().
// Returns true when this lane holds a block (lane < cnt * 6).
// dense_only: a round launch -- the frame's lines are in slot `slot` whatever rec_count says.  A default launch over
// records leaves frames that went to the serial kernel alone: skip = true (for the whole workgroup), nothing loaded.
__device__ __forceinline__ bool stage_segment_blocks(const SyncSinks& in, const Segment& sg, bool dense_only, const FrameGeom& g,
                                                     uint32_t lane, uint8_t* s_img, BlockForm& form, bool& skip) {
    const uint32_t f = sg.f, segidx = sg.segidx, nsegs = sg.nsegs, mcu0 = sg.mcu0, cnt = sg.cnt, ok = sg.ok;
    const uint32_t nb = cnt * 6u;
    // What the wave must know before it can ask for its records: the form of the frame and the segment's record range
    // (asked for together here), how far the frame was decoded (segment_of's load) and where its records begin
    // (rec_line, below).  In the code object these are three waits for memory in a row, not one: the compiler sinks
    // each load behind the branch that first uses its value.  Asked for together and waited for once -- held in place
    // by empty asm statements over scalar registers -- they cost eleven scalar instructions more and bought nothing
    // that could be measured, so they are left as the compiler places them.
    uint32_t rc = 0xffffffffu, r0 = 0u, r1 = 0u;
    if (in.rec != nullptr && !dense_only) {
        // a segment's records lie in [from of its own entry, to of the next one) -- bounds, not exact positions: the range
        // may begin with records of the (<= 4) blocks before the segment and end with records of the (<= 4) blocks behind
        // it, which the block test below drops
        const uint32_t* ss = in.seg_start + ((uint64_t)f * (nsegs + 1u) + segidx) * 2u;
        rc = in.rec_count[f];
        r0 = ss[0];
        r1 = ss[3];
    }
    const bool records = rc != 0xffffffffu;
    form = BlockForm{records, records && !(rc & kRecCountBigAc), 0};
    skip = !records && in.rec != nullptr && !dense_only;   // a round launch reconstructs this frame
    if (skip) return false;
    int dc_base = 0;
    if (records) {   // records -> dense image of the segment's blocks in LDS
        // blocks of this segment that were decoded: whole MCUs' (ok counts MCUs), or -- AMVHIP_FLAG_FFMPEG_KEEP -- every
        // whole block before the frame's first error (ok counts blocks then: SyncSinks::ok_in_blocks)
        const uint32_t ok_blocks = in.ok_in_blocks ? ok : ok * 6u;
        const uint32_t blocks_ok_here = ok_blocks > mcu0 * 6u ? min(nb, ok_blocks - mcu0 * 6u) : 0u;
        if (!blocks_ok_here) r1 = r0;
        // The segment's records are asked for all at once, four consecutive ones per lane and instruction (a loop of
        // one 4-byte load per lane and trip waited for memory eight times in a row: 1.6 of the kernel's 4.4 ms); the
        // image is zeroed while they are on their way.
        struct __attribute__((packed, aligned(4))) Rec4 { uint32_t w[4]; };
        constexpr uint32_t kAhead = 3;                                   // 768 records per trip; a segment has ~500
        const uint32_t* rec = in.rec + (uint64_t)in.rec_line[f] * 32u + r0;
        const uint32_t nrec = r1 - r0;
        Rec4 q[kAhead];
#pragma unroll
        for (uint32_t j = 0; j < kAhead; ++j) {
            const uint32_t i = j * 4u * kWave + lane * 4u;
            q[j] = Rec4{{kDummyRecord, kDummyRecord, kDummyRecord, kDummyRecord}};
            if (i < nrec) q[j] = *reinterpret_cast<const Rec4*>(rec + i);   // (may read up to 3 words past r1: see ensure())
        }
        uint4* img16 = reinterpret_cast<uint4*>(s_img);
        if (nb == 60u) {   // (wave-uniform) the whole image is seven and a half stores a lane: no test per trip
            constexpr uint32_t kWhole = 60u * 8u / kWave;
#pragma unroll
            for (uint32_t j = 0; j < kWhole; ++j) img16[j * kWave + lane] = make_uint4(0, 0, 0, 0);
            if (lane < 60u * 8u - kWhole * kWave) img16[kWhole * kWave + lane] = make_uint4(0, 0, 0, 0);
        } else {
            for (uint32_t i = lane; i < nb * 8u; i += kWave) img16[i] = make_uint4(0, 0, 0, 0);
        }
        seg_sync();
        // Scatter, without a branch per record.  A word is index | block field << 6 | filler << 15 | value << 16, the
        // field counting from the frame's end modulo 64.  The index's granule bits (3-5) are XOR-ed with the field's low
        // three bits first -- the reader's swizzle, taken from the field as it stands, so the lane of block b reads with
        // (b + first block's field) & 7 -- and then ONE add-and-shift puts the segment's first block at 0 and doubles the
        // whole: byte offset in bits 1-6, block in segment in bits 7-12 (modulo 64, the carry lands in bit 13), filler in
        // bit 16.  Masked to those, one unsigned compare against "blocks decoded << 7" rejects fillers and other
        // segments' blocks alike.  A rejected record goes to the lane's spare slot behind the image.  The value is stored
        // from the word's high half as it lies.  Words past the range's end are made fillers beforehand, in the one
        // piece that holds the end (a test per record cost two instructions in every slot).
        const uint32_t field0 = (mcu0 * 6u - g.blocks) & 63u;               // the block field of the segment's first block
        const uint32_t first6 = (uint32_t)__builtin_amdgcn_readfirstlane((int)((64u - field0) << kScatterFieldShift));   // (wave-uniform by contract)
        const uint32_t ok7 = blocks_ok_here << 7;
        const uint32_t spare = kSegImageBytes + lane * 2u;
        for (uint32_t base = 0;;) {
#pragma unroll
            for (uint32_t j = 0; j < kAhead; ++j) {
                if (base + j * 4u * kWave >= nrec) break;                   // (wave-uniform) nothing of this piece is in range
                if (base + (j + 1u) * 4u * kWave > nrec) {                  // (wave-uniform) the range ends inside this piece
                    const int32_t left = (int32_t)(nrec - base - j * 4u * kWave) - (int32_t)(lane * 4u);   // records from this lane's first on
#pragma unroll
                    for (uint32_t e = 0; e < 4u; ++e)
                        if (left <= (int32_t)e) q[j].w[e] = kDummyRecord;
                }
#pragma unroll
                for (uint32_t e = 0; e < 4u; ++e) {
                    const uint32_t w = q[j].w[e];
                    // t = ((w ^ ((w >> 3) & 0x38)) + first6) << 1.  Written as the instruction because hipcc 7.2 splits
                    // first6 into -(field0 << 6) and 64 << 6 and adds twice (eight instructions a slot instead of seven);
                    // to see whether a compiler still needs it: put the C expression here and count the vector
                    // instructions between two ds_write_b16_d16_hi of amv_reconstruct_kernel<false, 4> in the disassembly.
                    uint32_t t;
                    asm("v_add_lshl_u32 %0, %1, %2, 1" : "=v"(t) : "v"(w ^ ((w >> 3) & kScatterSwizzleMask)), "s"(first6));
                    const uint32_t at = t & kScatterAddressMask;
                    *reinterpret_cast<int16_t*>(s_img + (at < ok7 ? at : spare)) = (int16_t)(w >> 16);
                }
            }
            base += kAhead * 4u * kWave;
            if (base >= nrec) break;
#pragma unroll
            for (uint32_t j = 0; j < kAhead; ++j) {   // a segment with more records than one trip holds
                const uint32_t i = base + j * 4u * kWave + lane * 4u;
                if (i < nrec) q[j] = *reinterpret_cast<const Rec4*>(rec + i);
            }
        }
        // a DC record counts from its lane's first block: the base of the lane that decoded this block's DC
        // (how many lanes decoded THIS frame is in its rec_count: a chip-filling batch gives its heavy frames several and
        // the others one, and a one-lane frame has no row in the table)
        const uint32_t frame_lanes = ((rc >> 24) & 63u) + 1u;
        if (frame_lanes > 1u) {
            // the entropy lane that decoded this block's DC symbol: the last one whose first block is not behind it (first blocks
            // ascend along the row; lanes right of the frame's end hold ~0).  A binary search by lane shuffles: as a loop of
            // readlanes over the row it cost a heavy frame's segment 13 000 cycles with 16 lanes to the frame (0.4 ms per
            // 10 000 such frames).
            const uint32_t babs = mcu0 * 6u + lane, k6 = lane % 6u;
            const uint4 ent = lane < frame_lanes ? reinterpret_cast<const uint4*>(in.lane_tab)[(uint64_t)f * in.lanes + lane]
                                                 : make_uint4(0xffffffffu, 0u, 0u, 0u);
            uint32_t at = 0u;                           // lane 0 starts the frame: base 0
#pragma unroll
            for (uint32_t step = 32u; step >= 1u; step >>= 1) {
                const uint32_t probe = at + step;
                const uint32_t first = (uint32_t)__shfl((int)ent.x, (int)(probe & 63u));
                if (probe < frame_lanes && first <= babs) at = probe;
            }
            const int by = __shfl((int)ent.y, (int)at), bu = __shfl((int)ent.z, (int)at), bv = __shfl((int)ent.w, (int)at);
            dc_base = at ? (k6 < 4u ? by : (k6 == 4u ? bu : bv)) : 0;
        }
        seg_sync();
    }
    form.dc_base = dc_base;
    return lane < nb;
}

// the block of a lane that stage_segment_blocks said holds one
__device__ __forceinline__ void fetch_block(const SyncSinks& in, const Segment& sg, const FrameGeom& g, uint32_t lane, const uint8_t* s_img,
                                            const BlockForm& form, uint32_t (&c)[32]) {
    const uint32_t mcu0 = sg.mcu0;
    if (form.records) {
        const uint4* src = reinterpret_cast<const uint4*>(s_img) + lane * 8u;
        const uint32_t swz = (lane + mcu0 * 6u - g.blocks) & 7u;   // the low bits of this block's field: the scatter's swizzle
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint4 q = src[(uint32_t)i ^ swz];
            c[4 * i] = q.x; c[4 * i + 1] = q.y; c[4 * i + 2] = q.z; c[4 * i + 3] = q.w;
        }
        c[0] = (c[0] & 0xffff0000u) | ((c[0] + (uint32_t)form.dc_base) & 0xffffu);   // int16 arithmetic, as the predictors wrap
    } else {
        const uint4* src = reinterpret_cast<const uint4*>(in.coef + (((uint64_t)sg.slot * g.mcus + mcu0) * 6u + lane) * 64u);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint4 q = src[i];
            c[4 * i] = q.x; c[4 * i + 1] = q.y; c[4 * i + 2] = q.z; c[4 * i + 3] = q.w;
        }
    }
}

__device__ __forceinline__ bool load_segment_blocks(const SyncSinks& in, const Segment& sg, bool dense_only, const FrameGeom& g,
                                                    uint32_t lane, uint8_t* s_img, uint32_t (&c)[32], bool& skip) {
    BlockForm form;
    if (!stage_segment_blocks(in, sg, dense_only, g, lane, s_img, form, skip)) return false;
    fetch_block(in, sg, g, lane, s_img, form, c);
    return true;
}

// int16 number `i` of a block held as 32 dwords
__device__ __forceinline__ int coef_at(const uint32_t (&c)[32], int i) {
    return (i & 1) ? ((int)c[i >> 1] >> 16) : (int)(int16_t)(c[i >> 1] & 0xffffu);
}

// The launches of a reconstruction call (amv_piece_map.h: for_each_launch): kernel `part` for a default launch, `walk` for a
// round (sel.round != 0), row_groups workgroups of `block` threads per item; they take (sinks, nmcu_ok, n, sel, g, pm, tail...).
template <class Kernel, class... Tail>
static inline void launch_segments(Kernel part, Kernel walk, uint32_t block, uint32_t row_groups, const SyncSinks& sinks, const uint32_t* nmcu_ok,
                            uint32_t n, const FrameSel& sel, uint32_t items, const FrameGeom& g, hipStream_t s, Tail... tail) {
    for_each_launch(row_groups, segs_per_row(g), items, sel.round != 0u, [&](const PieceMap& pm, uint32_t grid) {
        hipLaunchKernelGGL(sel.round ? walk : part, dim3(grid), dim3(block), 0, s, sinks, nmcu_ok, n, sel, g, pm, tail...);
    });
}

}  // namespace amv
