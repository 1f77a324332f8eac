// amv_kernels.h -- launch wrappers of the HIP kernels (internal to libamvhip.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <variant>

#include "amv_tables.h"

namespace amv {

// status bits, same values as AMVHIP_ST_* in include/amvhip.h
enum : uint32_t { kStFormat = 1u, kStOverrun = 2u, kStTruncated = 4u };
enum : uint32_t { kFlagZigzagFixed = 1u, kFlagFfmpeg = 2u, kFlagFfmpegKeep = 4u };

// ---- decode -------------------------------------------------------------------------------
// entropy stage: one lane per frame, coefficients staged per block in LDS and written out as
// whole 128-byte lines.  coef: [..][blocks][64] int16, scan order, DC already predicted.
// Work items base .. base + items: item p is frame list[p] (p < *list_count) or, without a list, frame p (p < n);
// its lines go to coef slot p - base (by_slot) or to the frame's own place.
void launch_huffman(const uint8_t* blob, uint64_t blob_bytes, const uint64_t* offs,
                    const uint32_t* lens, uint32_t n, const FrameGeom& g,
                    const HuffDecodeImage* d_img, int16_t* coef, int32_t* status,
                    uint32_t* nmcu_ok, const uint32_t* list, const uint32_t* list_count, uint32_t base, uint32_t items,
                    bool by_slot, bool ok_in_blocks, hipStream_t s);
// entropy stage with parallelism inside a frame (amv_decode_sync.hip): unstuff into a workspace
// (frame i in the 16-byte pieces ws_line[i] .. ws_line[i + 1] of ws, ws_bytes[i] = unstuffed length or ~0 when the frame is handed to
// launch_huffman through retry_list / *retry_count), then L lanes per frame synchronise and decode.
void launch_unstuff(const uint8_t* blob, uint64_t blob_bytes, const uint64_t* offs, const uint32_t* lens, uint32_t n,
                    const uint32_t* ws_line, uint32_t* ws, uint32_t* ws_bytes, uint32_t* retry_list, uint32_t* retry_count,
                    hipStream_t s);
// lanes per frame for a batch of n frames of `pixels` pixels on a device with `cus` compute units (amv_decode_sync.hip)
int huffman_sync_lanes(uint32_t n, uint32_t cus, int wanted, uint64_t pixels);
// the statistics buffer of the synchronising entropy kernel (amvhip_entropy_stats / _trace): 16 words of counters, then
// one line of eight 64-bit words per task (wave) for the first kTraceTasks tasks of a launch
constexpr uint32_t kTraceBase = 16, kTraceTasks = 16384;
constexpr size_t kStatsBytes = (size_t)(kTraceBase + 8u * kTraceTasks) * 8u;
// What the reconstruction reads.  rec == nullptr: the caller's dense coefficient lines in coef ([n][blocks][64] int16:
// amvhip_reconstruct_dev).  Otherwise what the entropy stage wrote, per frame: its lines of rec (one word per DC coefficient and
// per non-zero AC coefficient, stream order: bits 0-5 index in block (0 = DC), 6-11 (block - blocks per frame) modulo 64, bit 15 filler,
// 16-31 value; a DC value counts from the decoding lane's first block), seg_start[segs + 1][2] = {from, to} for each
// MCU-row segment of kSegMcus MCUs (what one wave of the reconstruction takes): the segment's first record is at or
// after `from` with only records of the <= 4 blocks before it in between, and the records of the segment before end
// ahead of `to`, with only records of this segment's first <= 4 blocks in between (the exact position twice, or the
// record counts around the eight symbols in which the segment began), lane_tab[lanes] = {first block,
// DC base Y, Cb, Cr} of each of the lanes that decoded the frame (a row of `lanes` entries per frame; how many of them a
// frame used is in its rec_count), rec_count (bits 0-23 total, bits 24-29 lanes that decoded the frame - 1, bit 30
// kRecCountBigAc: the frame's walk met an AC symbol of ten magnitude bits or more; or ~0 = this
// frame is in dense form in coef because it went through amv_huffman_kernel).
constexpr uint32_t kRecCountBigAc = 1u << 30;
struct SyncSinks {
    int16_t* coef;
    uint32_t* rec;
    const uint32_t* rec_line;   // [n + 1]: frame i's records live in 128-byte lines rec_line[i] .. rec_line[i + 1] of rec (launch_layout)
    uint32_t* seg_start;
    uint32_t* lane_tab;
    uint32_t lanes;
    uint32_t* rec_count;
    uint32_t* retry_list;
    uint32_t* retry_count;
    // AMVHIP_FLAG_FFMPEG_KEEP: nmcu_ok[] counts whole BLOCKS decoded before a frame's first error, not whole MCUs (the
    // entropy kernels write it so, the reconstruction reads it so) -- an internal array then, never a caller's
    uint32_t ok_in_blocks;
};
// Space per frame from the frame's own chunk length, for the unstuffed scans (a) and, when b.line != nullptr, for the record
// hand-over (b) alike: min(hi, per_byte_x2 / 2 * lens[i] + add) units, rounded up to whole lines of 1 << unit_shift units;
// line[0 .. n] = where each frame's lines begin (an exclusive scan), never past cap_lines (a frame that gets less than it
// needs is decoded by the serial kernel).  work: layout_workspace(n) bytes.
struct LayoutSpec {
    uint32_t per_byte_x2, add, hi, unit_shift, cap_lines;
    uint32_t* line;
};
uint64_t layout_workspace(uint32_t n);
void launch_layout(const uint32_t* lens, uint32_t n, const LayoutSpec& a, const LayoutSpec& b, void* work, uint32_t* zero, uint32_t nzero,
                   bool force_large, hipStream_t s);
// Frames whose chunk is more than twice the batch's mean chunk (by the pieces the layout gave their scans: ws_line) ->
// heavy[0 .. count[0]), the others -> light[0 .. count[1]); count[0..1] zeroed by the caller.  A chip-filling batch decodes
// the light ones one lane per frame and the heavy ones with several lanes each (amvhip_decode.hip: entropy_front).
void launch_split_by_weight(const uint32_t* lens, uint32_t n, const uint32_t* ws_line, uint32_t* heavy, uint32_t* light, uint32_t* count,
                            hipStream_t s);
// list/list_count: optional frame list; *queue: a zeroed task counter per launch
void launch_huffman_sync(const uint32_t* ws, const uint32_t* ws_bytes, uint32_t n, const uint32_t* list,
                         const uint32_t* list_count, const FrameGeom& g, const uint32_t* ws_line, int lanes_per_frame,
                         const HuffDecodeImage* d_img, const SyncSinks& sinks, int32_t* status, uint32_t* nmcu_ok,
                         uint32_t* queue, unsigned long long* stats, uint32_t cus, hipStream_t s);
// Which frames a reconstruction launch takes.  Default: frame = blockIdx.x for all n frames, dense lines (if any) at
// the frame's own place; frames of a records launch that went to the serial kernel (rec_count ~0) are skipped --
// a round launch picks them up.  Round: work items base .. base + round, item p = frame list[p] (p < *count) or
// frame p (p < n), dense lines in slot p - base; the launch is small (its workgroups walk the items) because the
// round usually has nothing to do and the host cannot know.
struct FrameSel {
    const uint32_t* list;
    const uint32_t* count;
    uint32_t base;
    uint32_t round;   // items of this round; 0 = default launch
};
// The encoder's kernels read a FrameSel through these two: how many items the launch has (a round: what is left of the
// list, or of the n frames, from base on, at most `round`), and the frame of item `item` (< sel_items); the item is also
// the slot of the frame's dense lines.  (The reconstruction's select_frame, amv_block_load.h, has no count to give in a
// default launch, where it trusts the grid: DESIGN.md 4.5.)
__device__ __forceinline__ uint32_t sel_items(const FrameSel& sel, uint32_t n) {
    if (!sel.round) return n;
    const uint32_t have = sel.count ? *sel.count : n;
    return have > sel.base ? min(sel.round, have - sel.base) : 0u;
}
__device__ __forceinline__ uint32_t sel_frame(const FrameSel& sel, uint32_t item) {
    return sel.round ? (sel.list ? sel.list[sel.base + item] : sel.base + item) : item;
}
// records form -> dense lines coef[n][blocks][64] (amvhip_huffman_decode_dev): one wave per MCU-row segment, through the
// reconstruction's reader (amv_block_load.h).  Frames whose rec_count is ~0 are left alone (the serial kernel writes them);
// lines of blocks at or after a frame's first error are zeros.
void launch_expand_records(const SyncSinks& sinks, const uint32_t* nmcu_ok, uint32_t n, const FrameGeom& g, int16_t* coef,
                           hipStream_t s);
// dequantise + IDCT + YCbCr->BGR + flipped store: one wave per MCU-row segment
// sinks.rec == nullptr: every frame is dense in sinks.coef; otherwise per frame as rec_count says
void launch_reconstruct(const SyncSinks& sinks, const uint32_t* nmcu_ok, uint32_t n, const FrameSel& sel, uint32_t items,
                        const FrameGeom& g, uint32_t flags, uint8_t* out, hipStream_t s);

// FFmpeg-compat back half (amv_reconstruct_ff.hip): Q60 dequantisation, simple_idct_put, YUVJ420P planes
// (Y, Cb, Cr; tight rows) flipped as mjpegdec.c:672-677 does.  yuv_store_covers_planes: false when that formula
// leaves plane rows unwritten (the caller clears the output first).
void launch_reconstruct_yuv(const SyncSinks& sinks, const uint32_t* nmcu_ok, uint32_t n, const FrameSel& sel, uint32_t items,
                            const FrameGeom& g, uint64_t yuv_frame_bytes, uint8_t* out, hipStream_t s);
bool yuv_store_covers_planes(const FrameGeom& g);
// ... at 1/2, 1/4, 1/8 size (amv_reconstruct_lowres.hip, amv_reconstruct_yuv_lowres_kernel<L, kRound>; lowres = L = 1..3):
// j_rev_dct4 / 2 / 1 over the top-left coefficients of each block, the planes of lowres_dim(w) x lowres_dim(h) placed by
// lowres_start_row (amv_host_plan.h).  The caller clears the output first where lowres_store_covers_planes says no.
void launch_reconstruct_yuv_lowres(const SyncSinks& sinks, const uint32_t* nmcu_ok, uint32_t n, const FrameSel& sel, uint32_t items,
                                   const FrameGeom& g, uint32_t lowres, uint8_t* out, hipStream_t s);

// ---- encode -------------------------------------------------------------------------------
// planar YUVJ420P source (what the reference's amv_encoder takes, mjpegenc.c:493): frame i's planes at
// y + i*y_frame, cb/cr + i*c_frame (bytes); rows y_stride / c_stride apart.  c_rows422: the chroma planes have a row
// per luma row (YUVJ422P, the other entry of pix_fmts); the two rows over a 4:2:0 sample are averaged, rounding up.
struct YuvSource {
    const uint8_t* y;
    const uint8_t* cb;
    const uint8_t* cr;
    uint32_t y_stride, c_stride;
    uint64_t y_frame, c_frame;
    uint32_t c_rows422;
};
namespace enc {
// Where a call's pixels are, as the encoder kernels take it: packed RGB24 / BGR24 frames, rows pix_stride apart (is_bgr: the
// byte order), or the planes of yuv.  planar says which half is live: the entries check that half by it, the launchers
// pick the kernels' kYuv by it (the kernels themselves do not read it).
struct Source {
    const uint8_t* pix;
    uint32_t pix_stride;
    int is_bgr;
    YuvSource yuv;
    uint32_t planar;
};
}  // namespace enc
using enc::Source;
inline Source rgb_source(const uint8_t* pix, uint32_t pix_stride, int is_bgr) { return Source{pix, pix_stride, is_bgr, YuvSource{}, 0u}; }
inline Source yuv_source(const YuvSource& yuv) { return Source{nullptr, 0u, 0, yuv, 1u}; }
// How the AC coefficients of a call become levels, one of four: rounded (dct_quantize_c); rounded after denoising with the
// noise-reduction offsets of the call's frames (uint16 [n][64], amv_nr_plan.h: launch_nr_chain writes them); searched per
// block by the trellis quantiser with this lambda (amv_trellis_plan.h); or denoised with the offsets and then searched, as
// dct_quantize_trellis_c does it (mpegvideo_enc.c:2987-2990).  Each is an instantiation of the encoder kernels (their one
// optional trailing argument: none, the offsets, the TrellisArg, the NrTrellisArg).
struct PlainQuant {};
struct TrellisArg { uint32_t lambda; };
struct NrTrellisArg { const uint16_t* offsets; uint32_t lambda; };
// ... and the two searching ones with a lambda per frame, uint32 [n] on the device, read at the frame's own index (the rate
// entries, amvhip_encode.hip: rate_core).  amv_forward_kernel alone has these instantiations: a call that carries one takes
// the two-stage route for every frame, and launch_encode_frames refuses them.
struct TrellisFrames { const uint32_t* lambda; };
struct NrTrellisFrames { const uint16_t* offsets; const uint32_t* lambda; };
using Quantiser = std::variant<PlainQuant, const uint16_t*, TrellisArg, NrTrellisArg, TrellisFrames, NrTrellisFrames>;
// The whole encoder, one workgroup per frame (amv_encode_par.hip): pixels -> FF D8 + escaped scan + FF D9 in
// tmp[i*bound..], lens[i].  Frames whose bits do not fit the kernel's LDS window are appended to retry_list /
// *retry_count for launch_forward + launch_pack (rounds).
void launch_encode_frames(const Source& in, uint32_t n, const FrameGeom& g, uint32_t qbias, const Quantiser& quant,
                          const HuffEncodeImage* d_img, uint8_t* tmp, uint32_t bound, uint32_t* lens, uint32_t* retry_list,
                          uint32_t* retry_count, hipStream_t s);
// The reference's -nr (amv_encode_nr.hip, arithmetic in amv_nr_plan.h).  launch_nr_sums: per frame, the sum of the fdct
// outputs' magnitudes per position over the encoder's own blocks -> sums uint32 [n][64] (position 0: the sum of DC + 8192).
// launch_nr_chain: one wave walks the n frames -- halve if due, the frame's offsets -> offs uint16 [n][64] (entry c * 8 + r),
// add the frame's sums and `blocks` -- from the caller's state (int32 [65] on the device) to the state after the last frame.
void launch_nr_sums(const Source& in, uint32_t n, const FrameGeom& g, uint32_t* sums, hipStream_t s);
void launch_nr_chain(const uint32_t* sums, uint32_t n, uint32_t blocks, uint32_t nr, int32_t* state, uint16_t* offs, hipStream_t s);
// The two-stage route (amv_encode.hip).  colour conversion + level shift + forward DCT + quantise -> dense lines
// coef [..][blocks][64] int16 scan order; entropy coder, one lane per frame -> tmp[frame*bound..], lens[frame].
// sel: default (round == 0) = frames 0 .. n with lines at the frame's own place; round = items base .. base + round,
// item p = frame list[p] (p < *count), lines in slot p - base.  items: upper bound of the work (grid size).
void launch_forward(const Source& in, uint32_t n, const FrameSel& sel, uint32_t items, const FrameGeom& g, uint32_t qbias,
                    const Quantiser& quant, int16_t* coef, hipStream_t s);
void launch_pack(const int16_t* coef, uint32_t n, const FrameSel& sel, uint32_t items, const FrameGeom& g,
                 const HuffEncodeImage* d_img, uint8_t* tmp, uint32_t bound, uint32_t* lens, hipStream_t s);
// The encoder's own error (amv_encode_error.hip): for the frames of `sel` whose dense lines launch_forward wrote to coef, the
// squared error between the source's planes and simple_idct_put of level * Q, summed over the samples inside the picture
// and ADDED to sse [n][3] uint64 (Y, Cb, Cr of frame f at sse[3 f ..]; the caller zeroes it).  sel and items as launch_forward's.
void launch_encode_error(const Source& in, uint32_t n, const FrameSel& sel, uint32_t items, const FrameGeom& g, const int16_t* coef,
                         uint64_t* sse, hipStream_t s);
// Quantizer noise shaping (amv_encode_qns.hip, arithmetic in amv_qns_plan.h): for the frames of `sel` whose dense lines
// launch_forward wrote to coef, every block's levels refined in place against the source's planes.  basis_t: the basis on the
// device, int16 [sample][scan position]; qns 1 .. 3, lambda2 <= kQnsLambda2Max.  sel and items as launch_forward's.
void launch_qns_refine(const Source& in, uint32_t n, const FrameSel& sel, uint32_t items, const FrameGeom& g, int16_t* coef, const int16_t* basis_t,
                       uint32_t qns, uint32_t lambda2, hipStream_t s);
// The rate probe (amv_encode_rate.hip, arithmetic in amv_rate_plan.h): the front half once per block, the trellis walk once
// per lambda of the ladder on the same fdct outputs, and the bits the entropy coder would write for the frame's scan at each
// -- DC and AC codes, magnitudes, ZRLs, EOBs, before padding and escaping -- ADDED to bits uint32 [n][rungs] (the caller
// zeroes it).  offsets: the frames' noise-reduction offsets (launch_nr_chain's) or nullptr.  dc: workspace, int16 [n][blocks]
// (the quantised DCs on their way from the probe kernel to the launch that adds the difference codes).
struct RateLadder {
    uint32_t lambda[16];
    uint32_t rungs;
};
void launch_rate_probe(const Source& in, uint32_t n, const FrameGeom& g, uint32_t qbias, const uint16_t* offsets, const RateLadder& ladder,
                       int16_t* dc, uint32_t* bits, hipStream_t s);
// The choice per frame (amv_rate_plan.h: rate_first_fit over the floors of the bits table).  budgets: uint32 [n] or nullptr
// (then `budget` for every frame).  launch_rate_choose: every frame's first floor-fit -> rung[i] (kRateOver or-ed in and the
// frame final where none fits: the last rung then), lambda[i] = the rung's.  launch_rate_check, after the frames of
// list[0 .. *count) (list nullptr: all n) were coded and lens holds their lengths: a frame that is not final and is over its
// budget moves to the next floor-fit (or to the last rung, flagged and final), gets that lambda and is appended to
// next[0 .. *next_count) -- unless it is on the last rung already, where only the flag is set.  A frame is final when
// rung[i] carries kRateOver.
void launch_rate_choose(const uint32_t* bits, const RateLadder& ladder, const uint32_t* budgets, uint32_t budget, uint32_t n, uint32_t* rung,
                        uint32_t* lambda, hipStream_t s);
void launch_rate_check(const uint32_t* bits, const RateLadder& ladder, const uint32_t* budgets, uint32_t budget, uint32_t n, const uint32_t* lens,
                       const uint32_t* list, const uint32_t* count, uint32_t* rung, uint32_t* lambda, uint32_t* next, uint32_t* next_count,
                       hipStream_t s);
// ... its second launch alone (a caller whose probe kernel is its own: amv_requant.hip)
void launch_rate_dc(const int16_t* dc, uint32_t n, uint32_t blocks, uint32_t rungs, uint32_t* bits, hipStream_t s);
// The choice per clip (amv_encode_clip.hip, arithmetic in amv_clip_plan.h), above the choice per frame.  fr: which frames are
// coded at all -- status nullptr: every one; else the requant entry's status, whole MCUs and range flags (a frame that is not
// coded adds nothing to a sum, starts on the last rung flagged and stays).  state: the clip rung the frames stand at and
// whether the clip is final (zeroed by the caller).  launch_clip_floor: the floor sums ADDED to F uint64 [rungs] (the caller
// zeroes it).  launch_clip_start: the first rung whose floor sum fits `total` -> state->c, every frame's record and lambda
// there (in launch_rate_choose's place).  launch_clip_settle, behind each launch_rate_check with that check's next /
// next_count: a list was left or the clip is final -> nothing; else the sum of lens against total: final -> clip[0] = the
// rung (kRateOver or-ed in when over), clip[1] = the sum, state->done; or the clip moves on and the frames below its new
// rung get their records and lambdas there and form next[0 .. *next_count).
struct ClipFrames {
    const int32_t* status;
    const uint32_t* nmcu_ok;
    const uint32_t* flags;
    uint32_t mcus;
};
constexpr ClipFrames kClipAllFrames{nullptr, nullptr, nullptr, 0u};
struct ClipState {
    uint32_t c, done, unused[2];
};
void launch_clip_floor(const uint32_t* bits, uint32_t rungs, const uint32_t* budgets, uint32_t budget, uint32_t n, const ClipFrames& fr,
                       uint64_t* F, hipStream_t s);
void launch_clip_start(const uint32_t* bits, const RateLadder& ladder, const uint32_t* budgets, uint32_t budget, uint32_t n, const ClipFrames& fr,
                       const uint64_t* F, uint64_t total, ClipState* state, uint32_t* rung, uint32_t* lambda, hipStream_t s);
void launch_clip_settle(const uint32_t* bits, const RateLadder& ladder, const uint32_t* budgets, uint32_t budget, uint32_t n, const ClipFrames& fr,
                        const uint32_t* lens, const uint64_t* F, uint64_t total, ClipState* state, uint32_t* rung, uint32_t* lambda, uint32_t* next,
                        uint32_t* next_count, uint64_t* clip, hipStream_t s);
// Chunks requantised in the coefficient domain, or re-tabled (amv_requant.hip, arithmetic in amv_requant_plan.h and
// amv_retable_plan.h).  coef: a round of dense lines of levels as the entropy stage's kernels leave them (slot p - base of
// item p; sel and items as launch_forward's).  src: the entropy stage's status and nmcu_ok (whole MCUs) of the call's frames,
// and, in the pass over the frames in records form, their rec_count -- a frame whose count is ~0 is not in the round (nullptr:
// every frame of sel is).  rt: the tables the chunks were written against -- tables nullptr: AMV's own (the requant kernels);
// else uint8 [count][2][64] on the device (luma then chroma, scan order, entries 1 .. 255), count 1 .. 64, and table_of:
// uint8 [n] on the device, a frame's table (nullptr: table 0) (the re-table kernels: the line's DC and dc[] are the NEW DC, err
// sums over all 64 positions).  launch_requant: a frame that is coded gets its AC levels searched at lambdas[f] (lambdas
// nullptr: `lambda`), in place, and its planes' error ADDED to err [n][3] (nullptr: not wanted; the caller zeroes it); every
// other frame of sel, and every block out of range, lines of zeros.  flags[f] (zeroed by the caller) afterwards, bit 0: the
// frame has a block out of range; bit 1: table_of[f] names no table (the frame is not coded).
// launch_requant_probe: the bits of the AC codes at every rung ADDED to bits [n][rungs], the DCs to dc [n][blocks] for
// launch_rate_dc.  launch_requant_finish: d_status takes the range flag (and AMVHIP_ST_TRUNCATED where a decode stopped early
// without saying why); a frame that is not coded gets lens 0, err 0, bits 0 and rung (rungs - 1) | kRateOver -- each where
// the pointer is not null.  launch_retable_status, behind it: the status of a frame whose index named no table becomes
// AMVHIP_ST_TABLE.
struct RequantSource {
    const int32_t* status;
    const uint32_t* nmcu_ok;
    const uint32_t* rec_count;
};
struct RetableTables {
    const uint8_t* tables;
    uint32_t count;
    const uint8_t* table_of;
};
void launch_requant(int16_t* coef, uint32_t n, const FrameSel& sel, uint32_t items, const FrameGeom& g, const RequantSource& src,
                    const RetableTables& rt, uint32_t lambda, const uint32_t* lambdas, uint32_t* flags, uint64_t* err, hipStream_t s);
void launch_requant_probe(const int16_t* coef, uint32_t n, const FrameSel& sel, uint32_t items, const FrameGeom& g, const RequantSource& src,
                          const RetableTables& rt, const RateLadder& ladder, uint32_t* flags, int16_t* dc, uint32_t* bits, hipStream_t s);
void launch_requant_finish(uint32_t n, const FrameGeom& g, int32_t* status, const uint32_t* nmcu_ok, const uint32_t* flags, uint32_t* lens,
                           uint64_t* err, uint32_t* rung, uint32_t* bits, uint32_t rungs, hipStream_t s);
void launch_retable_status(uint32_t n, int32_t* status, const uint32_t* flags, hipStream_t s);
// exclusive scan of lens -> offs (single workgroup), then gather tmp -> blob.  A chunk that would end past
// blob_cap is not copied and its lens entry becomes 0; *overflow = 1 when the total exceeds blob_cap.
void launch_compact(const uint8_t* tmp, uint32_t bound, uint32_t* lens, uint32_t n,
                    uint64_t* offs, uint8_t* blob, uint64_t blob_cap, int32_t* overflow, hipStream_t s);

// ---- picture rescale (amv_resample.hip): img_resample of libavcodec/imgresample.c ------------------------
struct ResamplePlanes {     // YUV420P frames: frame i's planes at y + i*y_frame, cb/cr + i*c_frame; chroma (w>>1) x (h>>1)
    uint8_t* y;
    uint8_t* cb;
    uint8_t* cr;
    uint32_t y_stride, c_stride;
    uint64_t y_frame, c_frame;
    uint32_t width, height;
};
struct ResampleFilters {    // img_resample_full_init (:425-472): 16 phases x 4 taps each way, 16.16 increments
    int16_t h[64], v[64];
    int h_incr, v_incr;
};
// to_jpeg: the bytes leave through y_ccir_to_jpeg / c_ccir_to_jpeg (the shim's last img_convert, YUV420P -> YUVJ420P, folded
// into the store); false: the plain routine, as it always was
void launch_resample(const ResamplePlanes& src, const ResamplePlanes& dst, const ResampleFilters& f, uint32_t n, hipStream_t s,
                     bool to_jpeg = false);

// ---- pixel formats (amv_pixfmt.hip): img_convert of libavcodec/imgconvert.c ----------------------------------------
// SCALEBITS = 10 fixed point of colorspace.h:30-32
constexpr int pix_fix(double x) { return (int)(x * 1024 + 0.5); }
// one of the four range tables of imgconvert.c:1216-1233 as min(max((v * mul + add) >> 10, lo), 255); identity: {1024, 0, 0}
struct PixRange { int mul, add, lo; };
constexpr PixRange kPixRangeNone{1024, 0, 0};
constexpr PixRange kPixYCcirToJpeg{pix_fix(255.0 / 219.0), 512 - 16 * pix_fix(255.0 / 219.0), 0};                         // colorspace.h:69-70
constexpr PixRange kPixYJpegToCcir{pix_fix(219.0 / 255.0), 512 + (16 << 10), 0};                                         // :72-73
constexpr PixRange kPixCCcirToJpeg{pix_fix(127.0 / 112.0), 512 + (128 << 10) - 128 * pix_fix(127.0 / 112.0), 0};         // :75-76
constexpr PixRange kPixCJpegToCcir{pix_fix(112.0 / 127.0), 512 + (128 << 10) - 128 * pix_fix(112.0 / 127.0), 16};        // :79-84
enum : uint32_t { kPixCopy = 0, kPixShrink12 = 1, kPixShrink22 = 2 };
struct PixPlaneJob {        // one destination plane of w x h samples; frame i at src + i*sframe, dst + i*dframe
    const uint8_t* src;
    uint8_t* dst;
    uint32_t sstride, dstride;
    uint64_t sframe, dframe;
    uint32_t w, h, resize;
    PixRange range;
};
struct PixPlaneJobs { PixPlaneJob j[3]; uint32_t count; };
struct PixPicture {         // planes (packed formats and GRAY8: plane 0 only), row and frame pitches in bytes
    uint8_t* p[3];
    uint32_t stride[3];
    uint64_t frame[3];
};
struct PixRgbIn { int y[3], yadd, u[3], v[3]; };          // weights of the bytes at +0, +1, +2 of a pixel
struct PixRgbOut {                                        // component at byte +0 / +1 / +2 (16-bit: red / green / blue)
    int ymul, yoff, c0[2], c1[2], c2[2];                  // {weight of cb - 128, weight of cr - 128}
    uint32_t rshift, gdrop;                               // 16-bit formats: 11, 2 (5-6-5) or 10, 3 (5-5-5)
};
void launch_pix_planes(const PixPlaneJobs& jobs, uint32_t n, hipStream_t s);
void launch_pix_packed_in(const PixPicture& src, const PixPicture& dst, uint32_t w, uint32_t h, bool uyvy, uint32_t n, hipStream_t s);
void launch_pix_packed_out(const PixPicture& src, const PixPicture& dst, uint32_t w, uint32_t h, bool uyvy, uint32_t n, hipStream_t s);
void launch_pix_rgb_in(const PixPicture& src, const PixPicture& dst, uint32_t w, uint32_t h, uint32_t bpp, const PixRgbIn& k, uint32_t n,
                       hipStream_t s);
void launch_pix_rgb_out(const PixPicture& src, const PixPicture& dst, uint32_t w, uint32_t h, uint32_t bpp, const PixRgbOut& k, uint32_t n,
                        hipStream_t s);

// ---- picture against picture (amv_picture_sse.hip) --------------------------------------------------------------------
struct SsePlane {           // one plane of both pictures: rows of row_bytes bytes; frame i at a + i*aframe, b + i*bframe
    const uint8_t* a;
    const uint8_t* b;
    uint32_t astride, bstride;
    uint64_t aframe, bframe;
    uint32_t row_bytes, rows;
    uint32_t entry;         // interleave 1: the plane's sum goes to entry `entry` of the frame's three
    uint32_t interleave;    // 3: a packed plane, byte x belongs to entry x % 3
    uint32_t tiles_x, tiles;   // (the launcher's)
};
struct SseJobs { SsePlane j[3]; uint32_t count; };
// the squared differences of n frames ADDED to sse [n][3] uint64 (the caller zeroes it)
void launch_picture_sse(SseJobs jobs, uint32_t n, uint64_t* sse, hipStream_t s);

// ---- video front end (amv_frontend.hip): avpicture_deinterlace and av_picture_pad's bands ------------------------------
struct DeintPlane {         // one plane: the window x0, y0, w, h of a source plane of full_h rows -> a destination of w x h
    const uint8_t* src;     // the FULL plane's origin
    uint8_t* dst;           // the window's origin
    uint32_t sstride, dstride;
    uint64_t sframe, dframe;
    uint32_t x0, y0, w, h, full_h;
};
struct DeintJobs { DeintPlane j[3]; uint32_t count; };
void launch_deinterlace(const DeintJobs& jobs, uint32_t n, hipStream_t s);

// ---- decode-side postprocessing (amv_postprocess.hip): the reference's hb / vb / dr on tight planes ------------------------
struct PpPlaneJob {         // one plane of every frame: pitch = w on both sides; mode 0: the plane is copied
    const uint8_t* src;
    uint8_t* dst;
    uint64_t sframe, dframe;
    uint32_t w, h;
    int mode;               // kPpVDeblock | kPpHDeblock | kPpDering of amv_pp_plan.h
};
struct PpJobs {
    PpPlaneJob j[3];
    int qp, base_dc_diff, flat_thr;
    const uint8_t* d_qp;    // a QP per frame, or nullptr: qp for all
};
void launch_postprocess(const PpJobs& jobs, uint32_t n, hipStream_t s);
struct PadBandPlane {       // one padded plane: geometry as PadPlane of amv_host_plan.h (the items are counted and placed there)
    uint8_t* dst;
    uint32_t stride;
    uint64_t frame;
    uint32_t W, H, wx, wy, ww, wh, color;
};
struct PadBandJobs { PadBandPlane j[3]; };
void launch_pad_bands(const PadBandJobs& jobs, uint32_t n, hipStream_t s);

// ---- audio resample (amv_audio_resample.hip): audio_resample of libavcodec/resample.c over av_resample (resample2.c) --
constexpr uint32_t kAudioPhases = 1024;                       // 1 << phase_shift (resample.c:165)
constexpr uint32_t kAudioSpan = 4096;                         // input frames of one workgroup's LDS span (per channel)
// Outputs one av_resample call makes on src_size frames from position `base` (index) and `frac0` before its break
// (:266-267): I_k = base + floor((frac0 + k * D) / out_rate), D = in_rate * 1024, exists while I_k < 0 or
// (I_k >> 10) + fl <= src_size.  Host and device use this one function.
__host__ __device__ inline uint64_t audio_out_count(uint64_t src_size, int64_t base, uint64_t frac0, uint64_t D, uint32_t out_rate,
                                                    uint32_t fl) {
    const int64_t lim = src_size + 1 > fl ? (int64_t)(src_size + 1 - fl) * (int64_t)kAudioPhases : 0;
    const int64_t m = lim - base;
    if (m <= 0) return 0;
    return ((uint64_t)m * out_rate - frac0 + D - 1) / D;
}
struct AudioResampleArgs {
    const int16_t* pcm;           // interleaved in_ch; stream i at pcm + pcm_offs[i], nsamp[i] frames
    const uint64_t* pcm_offs;
    const uint64_t* nsamp;
    int16_t* out;                 // interleaved out_ch; stream i at out + out_offs[i]
    const uint64_t* out_offs;
    const int16_t* bank;          // 1024 rows of fl_pad int16 (fl taps, then zeros), 16-byte aligned
    uint32_t* tiles;              // workspace: n + 1 words
    uint32_t n, in_ch, out_ch, out_rate, fl, fl_pad, tile;   // tile: outputs per workgroup tile (<= 256)
    uint64_t D;                   // in_rate * 1024
    int64_t base;                 // index before the first output (batch: -1024 * ((fl - 1) / 2))
    uint64_t frac0, cap;          // frac before the first output; most outputs per stream (lenout of :194)
};
uint32_t audio_resample_tile(uint32_t in_rate, uint32_t out_rate, uint32_t fl_pad);
void launch_audio_resample(const AudioResampleArgs& a, uint32_t blocks, hipStream_t s);

// ---- ADPCM --------------------------------------------------------------------------------
void launch_adpcm_decode(const uint8_t* blob, uint64_t blob_bytes, const uint64_t* offs,
                         const uint32_t* lens, uint32_t n, int16_t* pcm, const uint64_t* pcm_offs,
                         int32_t* final_state, hipStream_t s);
// The reference's step_index carry (adpcm.c:461-498) without a serial pass over the stream: every chunk coded from a
// guessed start, then `sweeps` launches, a front sweep and one settling workgroup (`settle`) that code again what started
// wrong, a check, and behind it the exhaustive route (89-way state map of every chunk, composition of the maps, every
// chunk coded from the start the maps give it), which leaves at once unless the chain did not settle; sweeps < 0: the
// exhaustive route at once.  See amv_adpcm.hip and amv_adpcm_chain.h.  work: adpcm_plain_chain_plan(n).bytes
// (amv_host_plan.h), whose zero span the launch zeroes.  Only enqueues; false: refused before anything was queued.
bool launch_adpcm_stream(const int16_t* pcm, const uint64_t* pcm_offs, const uint32_t* nsamp, uint32_t n, uint8_t* blob, const uint64_t* offs,
                         void* work, int sweeps, bool settle, hipStream_t s);
void adpcm_quotient_table(float out[89]);   // the encoder's quotient factors (see amv_adpcm.hip: compress)
// amvlib's IMA-WAV-layout frame encoder (AdpcmIma.c:43-160), one lane
void launch_adpcm_wav_encode(const int16_t* samples, int groups, int32_t* state, uint8_t* frame, hipStream_t s);
void launch_adpcm_encode(const int16_t* pcm, const uint64_t* pcm_offs, const uint32_t* nsamp,
                         uint32_t n, const int32_t* step_in, uint8_t* blob, const uint64_t* offs, const uint32_t* need,
                         hipStream_t s);

// the reference's trellis search (adpcm.c:287-443), one lane per independent chunk; paths: adpcm_trellis_workspace bytes.
// false: the device refused the kernel's LDS size
uint64_t adpcm_trellis_workspace(uint32_t n, uint32_t trellis);
bool launch_adpcm_trellis(const int16_t* pcm, const uint64_t* pcm_offs, const uint32_t* nsamp, uint32_t n, const int32_t* step_in,
                          uint32_t trellis, uint8_t* blob, const uint64_t* offs, int32_t* step_out, uint16_t* paths, hipStream_t s);
// ... and the chunks of a call as ONE stream, the step index carried from chunk to chunk on the device (guessed starts,
// a fixed number of sweeps over device-built lists, a check, and the 89-start fall-back behind it: see
// amv_adpcm_trellis.hip).  first_index 0..88; paths: adpcm_trellis_workspace(n, trellis) bytes; work:
// adpcm_trellis_chain_plan(n).bytes (amv_host_plan.h), whose zero span the launch zeroes; sweeps < 0: the fall-back at
// once.  Only enqueues; false: refused before anything was queued.
bool launch_adpcm_trellis_stream(const int16_t* pcm, const uint64_t* pcm_offs, const uint32_t* nsamp, uint32_t n, uint32_t first_index,
                                 uint32_t trellis, uint8_t* blob, const uint64_t* offs, int32_t* step_out, uint16_t* paths, void* work,
                                 int sweeps, hipStream_t s);

// ---- synthetic sources ----------------------------------------------------------------------
void launch_synth_frames(uint32_t seed, uint32_t first, uint32_t n, uint32_t w, uint32_t h,
                         uint8_t* rgb, hipStream_t s);
void launch_synth_audio(uint32_t seed, uint64_t first, uint64_t n, int16_t* pcm, hipStream_t s);

}  // namespace amv
