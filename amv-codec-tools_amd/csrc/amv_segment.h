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
constexpr uint32_t kDummyRecord = 0x8000u;   // bit 15 of a record word: a filler no block owns (the scatter drops it)
// a round launch is small (a round usually has nothing to do): at most this many items under way, their workgroups walk on
constexpr uint32_t kRoundWalkers = 512;
}  // namespace amv
