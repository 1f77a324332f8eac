// amv_segment.h -- what an MCU-row segment is: the work one wave takes in the reconstruction kernels, the entropy kernels
// that write the records per segment, and the encoder's front half.  No HIP in here (host plans and CPU tests read it).
#pragma once
#include "amv_tables.h"
#if defined(__HIPCC__)
#define AMV_HD __host__ __device__
#else
#define AMV_HD
#endif
namespace amv {
constexpr int kWave = 64;
constexpr uint32_t kSegMcus = 10;   // MCUs per wave: 60 of 64 lanes busy in the transform (one 8x8 block per lane)
AMV_HD inline uint32_t segs_per_row(const FrameGeom& g) { return (g.mcu_cols + kSegMcus - 1u) / kSegMcus; }
// The encoder's segments: an MCU row in segs_per_row pieces of equal size, the last one shorter (11 columns -> 6 + 5, not
// 10 + 1).  A frame's segments are numbered MCU row * nseg + piece.
struct SegSplit {
    uint32_t nseg, per_seg;
};
AMV_HD inline SegSplit seg_split(const FrameGeom& g) {
    const uint32_t nseg = segs_per_row(g);
    return {nseg, (g.mcu_cols + nseg - 1u) / nseg};
}
// segment s: its MCU row, first MCU column and MCUs.  false (and cnt 0): s is past the frame's last segment, or the piece
// would begin behind the row's last column (equal sizes, rounded up, may use a row up before its last piece)
AMV_HD inline bool seg_place(const SegSplit& sp, const FrameGeom& g, uint32_t s, uint32_t& my, uint32_t& m0, uint32_t& cnt) {
    my = s / sp.nseg;
    m0 = (s - my * sp.nseg) * sp.per_seg;
    const bool has = s < g.mcu_rows * sp.nseg && m0 < g.mcu_cols;
    cnt = !has ? 0u : sp.per_seg < g.mcu_cols - m0 ? sp.per_seg : g.mcu_cols - m0;
    return has;
}
constexpr uint32_t kDummyRecord = 0x8000u;   // bit 15 of a record word: a filler no block owns (the scatter drops it)
// a round launch is small (a round usually has nothing to do): at most this many items under way, their workgroups walk on
constexpr uint32_t kRoundWalkers = 512;
}  // namespace amv
