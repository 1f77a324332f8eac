// amvhip_ctx.h -- the context behind the C ABI of include/amvhip.h, and what its files share (internal to libamvhip.so).
//
// The ABI is split by domain: amvhip_context.hip (context, timing, statistics), amvhip_decode.hip, amvhip_encode.hip
// (encoders, picture rescale), amvhip_pixfmt.hip (img_convert, the sws_scale shim, the video front end, the postprocessing) and amvhip_audio.hip (resampler, ADPCM).
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "amv_clip_plan.h"
#include "amv_host_plan.h"
#include "amv_kernels.h"
#include "amv_nr_plan.h"
#include "amv_pp_plan.h"
#include "amv_qns_plan.h"
#include "amv_rate_plan.h"
#include "amv_requant_plan.h"
#include "amv_retable_plan.h"
#include "amv_trellis_plan.h"

namespace amv {

// grow-only device buffer (ensure), freed with its owner
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
};

// What one decode call hands from the entropy stage to the reconstruction
struct DecodeSet {
    DevBuf nmcu, retry, rec, rec_line, seg_start, lane_tab, rec_count;
    size_t cap() const { return nmcu.cap + retry.cap + rec.cap + rec_line.cap + seg_start.cap + lane_tab.cap + rec_count.cap; }
};

struct ProfRec {
    int kernel;
    hipEvent_t a, b;
};

}  // namespace amv

struct amvhip_ctx {
    using DevBuf = amv::DevBuf;
    int device = 0;
    std::string err;
    DevBuf d_dec, d_enc;   // HuffDecodeImage, HuffEncodeImage
    // workspace
    DevBuf coef, tmp, flag, enc_retry, stats, ws, ws_line, layout, ws_bytes, scaled, trellis_ws, trellis_chain, chain, split;
    // the -nr entries: the frames' sums and offsets (nr_plan of amv_nr_plan.h); the host-buffer forms' copy of the state
    DevBuf nr_ws, nr_state;
    // the -qns entries: the basis of amv_qns_plan.h as the kernel reads it, int16 [sample][scan position], uploaded once
    DevBuf qns_basis;
    // the rate entries: the bits table, the frames' lambdas, the redo lists, a probe's copy of the -nr state, the DCs
    // (rate_plan of amv_host_plan.h)
    DevBuf rate_ws;
    // the clip entries, beside rate_ws: the passes' counters, the floor sums, the clip's state (clip_plan of amv_host_plan.h)
    DevBuf clip_ws;
    // the requant entries: a flag per frame (a block out of range); the probe entry's statuses, which it does not hand out
    DevBuf requant_flags, requant_status;
    // the re-table entries: the call's source tables, uint8 [count][2][64]
    DevBuf retable_tables;
    // the shim around the rescaler: the source as YUV420P, the rescaled YUV420P ahead of a last conversion, the decoder's planes
    DevBuf pix_in, pix_out, pix_dec;
    // the video front end: the deinterlaced (and cropped) source ahead of the shim
    DevBuf fe_deint;
    // amvhip_decode_pp_batch_dev: the postprocessed planes ahead of a conversion (the decoder's own are in pix_dec)
    DevBuf pp_planes;
    // audio resampler: filter banks by (in_rate << 32 | out_rate), uploaded once and kept; the tile counts of the last call
    std::map<uint64_t, DevBuf> audio_banks;
    DevBuf audio_tiles;
    // set[0] serves every decode call but amvhip_decode_submit_dev, which takes the two in turn, so that the entropy stage
    // of one batch can run (stream `front`) beside the reconstruction of the batch before (`back`)
    amv::DecodeSet set[2];
    hipStream_t front = nullptr, back = nullptr;
    hipEvent_t ev_in = nullptr, ev_front = nullptr, ev_done[2] = {nullptr, nullptr};
    uint64_t submitted = 0, collected = 0;
    DevBuf* last_decode_retry = nullptr;   // whose first word counts the frames the LAST decode call handed to the serial kernel
    int sync_lanes = 0;   // AMVHIP_SYNC_LANES: 8/16/32/64 lanes per frame; 0 = by batch size (huffman_sync_lanes)
    bool split_heavy = true;   // AMVHIP_SPLIT=0: a one-lane-per-frame batch keeps its heavy frames on one lane too
    uint32_t heavy_lanes = 16; // AMVHIP_SPLIT=n: lanes a heavy frame gets (1, 2, 4 ... 64)
    bool last_split = false;   // the last decode call made the two lists (amvhip_decode_split_stats)
    uint32_t cus = 256;   // compute units of the device
    bool want_stats = false;
    bool layout_large = false;   // AMVHIP_LAYOUT=large: the three-launch layout whatever the batch size (test knob)
    double ws_bytes_per_frame = 0.0;
    int entropy_mode = AMVHIP_ENTROPY_AUTO;
    int adpcm_sweeps = 0;            // AMVHIP_ADPCM_SWEEPS: sweeps of the guessed-start route (-1: exhaustive route only)
    bool adpcm_sweeps_set = false;   // false: by stream length
    bool adpcm_settle = true;        // "nosettle": the chain stops after its launched sweeps (test knob: its check must notice)
    uint32_t chain_n = 0;            // chunks of the last chained ADPCM encode (where its counters are in `chain`)
    int trellis_sweeps = (int)amv::kTrellisSweeps;   // AMVHIP_ADPCM_TRELLIS_SWEEPS: sweeps of the trellis stream (-1: its fall-back at once)
    uint32_t trellis_chain_n = 0;    // chunks of the last trellis stream (where its counters are in `trellis_chain`)
    // host-pointer staging (one in-order stream of the context's own carries every host-buffer entry point)
    DevBuf h_in, h_offs, h_lens, h_out, h_status, h_aux, a_in, a_tab, a_out, r_in, r_tab, r_out;
    hipStream_t hstream = nullptr;
    // amvhip_decode_batch_async: decoded frames go back to the host on a stream of their own, out of two staging buffers used
    // in turn, so that the copy of one call runs beside the upload and the kernels of the next (a window of the amvlib reader
    // is 59 MB of frames back for 3.6 MB of chunks in)
    hipStream_t dstream = nullptr;
    DevBuf v_out[2], v_status[2];
    hipEvent_t ev_decoded = nullptr, ev_copied[2] = {nullptr, nullptr};
    uint64_t async_calls = 0;
    // timing
    bool prof = false;
    std::vector<amv::ProfRec> recs;
    std::vector<hipEvent_t> pool;
    uint64_t launches[AMVHIP_K_COUNT] = {};
    double total_ms[AMVHIP_K_COUNT] = {};
    std::mutex mu;    // the kernels' workspace: one _dev call enqueues at a time
    std::mutex hmu;   // the host-buffer staging (h_*, a_*): one host-buffer call at a time; taken before mu, never after
};

namespace amv {

// ---- amvhip_context.hip -----------------------------------------------------------------------
int fail(amvhip_ctx* c, int code, const char* fmt, ...);

#define HIP_TRY(ctx, expr)                                                                     \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail((ctx), e_ == hipErrorOutOfMemory ? AMVHIP_ERR_NOMEM : AMVHIP_ERR_DEVICE, \
                        "%s: %s", #expr, hipGetErrorString(e_));                               \
    } while (0)

int ensure(amvhip_ctx* c, DevBuf& b, size_t bytes);
// grow b to at least `room` bytes and queue the copy of `bytes` from host memory into it on st
int stage(amvhip_ctx* c, DevBuf& b, size_t room, const void* src, size_t bytes, hipStream_t st);
void drain(amvhip_ctx* c);
int check_launch(amvhip_ctx* c, const char* what);
int select_device(amvhip_ctx* c);
// Every entry point but amvhip_decode_submit_dev / _collect_dev: batches submitted earlier share the context's
// workspace with what is about to be queued, so they finish first (nothing to wait for when none is in flight).
int use_device(amvhip_ctx* c);
// How a host-buffer entry point begins: use_device, then the stream of these entry points -- created on first use,
// non-blocking (it does not order itself against the caller's other streams).  The caller locks c->hmu next.
int host_stream(amvhip_ctx* c, hipStream_t* out);

struct Timed {
    amvhip_ctx* c;
    hipStream_t s;
    ProfRec r{};
    bool on;
    Timed(amvhip_ctx* ctx, int kernel, hipStream_t st) : c(ctx), s(st), on(ctx->prof) {
        if (!on) return;
        r.kernel = kernel;
        for (hipEvent_t* e : {&r.a, &r.b}) {
            if (!c->pool.empty()) { *e = c->pool.back(); c->pool.pop_back(); }
            else if (hipEventCreate(e) != hipSuccess) { on = false; return; }
        }
        (void)hipEventRecord(r.a, s);
    }
    ~Timed() {
        if (!on) return;
        (void)hipEventRecord(r.b, s);
        c->recs.push_back(r);
    }
};

constexpr FrameSel kAllFrames{};   // a default launch: every frame of the batch, at its own place

// ---- pictures in the three forms the kernels take them ------------------------------------------------------------
inline PixPicture make_picture(const uint8_t* p0, const uint8_t* p1, const uint8_t* p2, uint32_t stride, uint32_t c_stride, uint64_t frame,
                               uint64_t c_frame) {
    return PixPicture{{const_cast<uint8_t*>(p0), const_cast<uint8_t*>(p1), const_cast<uint8_t*>(p2)}, {stride, c_stride, c_stride},
                      {frame, c_frame, c_frame}};
}

// a tight YUV420P picture series in a workspace buffer: Y (w x h), Cb, Cr ((w + 1) / 2 x (h + 1) / 2) per frame
inline PixPicture tight_420(uint8_t* p, uint32_t w, uint32_t h) {
    const uint32_t cw = (w + 1) / 2, chh = (h + 1) / 2;
    const uint64_t fb = (uint64_t)w * h + 2ull * cw * chh;
    return PixPicture{{p, p + (uint64_t)w * h, p + (uint64_t)w * h + (uint64_t)cw * chh}, {w, cw, cw}, {fb, fb, fb}};
}

inline YuvSource yuv_source_of(const PixPicture& p) {
    return YuvSource{p.p[0], p.p[1], p.p[2], p.stride[0], p.stride[1], p.frame[0], p.frame[1], 0u};
}

// ---- amvhip_decode.hip (the caller holds c->mu) ------------------------------------------------------------------------
int decode_args_ok(amvhip_ctx* c, const uint8_t* d_blob, const uint64_t* d_offs, const uint32_t* d_lens, uint32_t n, uint32_t w,
                   uint32_t h, uint32_t flags, const uint8_t* d_out, const int32_t* d_status);
// Frames the synchronising kernel does not decode go through amv_huffman_kernel, whose output is dense coefficient
// lines: all of them in AMVHIP_ENTROPY_SERIAL mode (and for pictures of >= 16384 blocks), else the few it hands back
// (oversize chunks, long FF runs, more records than the record space holds).  `items` bounds the work; with a list the
// real count sits on the device.
struct Fallback {
    const uint32_t* list;
    const uint32_t* count;
    uint32_t items;
};
// The entropy stage of a decode call into the hand-over set b (the decode entries' and the requant entries' front): records
// in `sinks`, statuses and nmcu_ok to d_status / d_nmcu_ok, fb = what is left for the serial kernel.
int entropy_records(amvhip_ctx* c, const uint8_t* d_blob, uint64_t blob_bytes, const uint64_t* d_offs, const uint32_t* d_lens, uint32_t n,
                    const FrameGeom& g, bool ok_in_blocks, int32_t* d_status, uint32_t* d_nmcu_ok, DecodeSet& b, hipStream_t st, SyncSinks& sinks,
                    Fallback& fb);
int decode_core(amvhip_ctx* c, const uint8_t* d_blob, uint64_t blob_bytes, const uint64_t* d_offs, const uint32_t* d_lens,
                uint32_t n, uint32_t w, uint32_t h, uint32_t flags, uint8_t* d_out, int32_t* d_status, DecodeSet& b,
                hipStream_t front, hipStream_t back, uint32_t lowres = 0);   // lowres 1..3: the reduced planes (flags = AMVHIP_FLAG_FFMPEG)

// ---- amvhip_pixfmt.hip (the caller holds c->mu) ------------------------------------------------------------------------
// one supported img_convert pair (pix_route), n frames, on st; every argument checked by the caller
int pix_convert_launch(amvhip_ctx* c, int src_fmt, const PixPicture& src, int dst_fmt, const PixPicture& dst, uint32_t w, uint32_t h, uint32_t n,
                       hipStream_t st);

// ---- amvhip_encode.hip (the caller holds c->mu) ------------------------------------------------------------------------
// what every encoder asks of the target size and of qbias
inline bool encode_size_ok(uint32_t w, uint32_t h, uint32_t qbias) { return size_ok(w, h) && !(w & 1) && !(h & 1) && qbias <= 255; }
// What an entry asks of the AC quantiser, one of four: nothing; the reference's -nr for a stream (amv_encode_nr.hip,
// amv_nr_plan.h) from the state the caller carries -- with nr == 0 the plain route, the state left alone; the trellis
// search (amv_trellis_plan.h; trellis_lane in amv_encode_common.h); or both, the search on what -nr left -- with nr == 0
// the trellis route, the state left alone.
struct NrRequest {
    uint32_t nr;
    int32_t* state;
};
struct NrTrellisRequest {
    uint32_t nr;
    int32_t* state;
    uint32_t lambda;
};
using QuantRequest = std::variant<PlainQuant, NrRequest, TrellisArg, NrTrellisRequest>;
// what a request asks beyond the plain entries' checks; 0 = go on
int quant_args_ok(amvhip_ctx* c, uint32_t n, uint32_t w, uint32_t h, const QuantRequest& req);
// the request an amvhip_quant stands for (its state is on the device); q == NULL and a trellis other than 0 / 1 are refused
int quant_request_of(amvhip_ctx* c, const amvhip_quant* q, QuantRequest* req);
// where a _psnr entry wants the frames' error: uint64 [n][3] on the device, 8-byte aligned (wanted == false: the entry has none)
struct ErrorSink {
    uint64_t* sse;
    bool wanted;
};
constexpr ErrorSink kNoError{nullptr, false};
int error_sink_ok(amvhip_ctx* c, uint32_t n, const ErrorSink& err);
// what a -qns entry asks behind the request's quantiser (amv_qns_plan.h): qns 0 = nothing, today's path
struct QnsArg {
    uint32_t qns, lambda2;
};
constexpr QnsArg kNoQns{0u, 0u};
int qns_args_ok(amvhip_ctx* c, const QnsArg& qns);
// the tail of the scaled encoders: the w x h pictures they made as tight_420 in c->scaled, through the request's core
// (req's state is on the device; d_sse: the frames' error, for the _psnr entry)
int encode_scaled_tail(amvhip_ctx* c, uint32_t n, uint32_t w, uint32_t h, uint32_t qbias, const QuantRequest& req, uint8_t* d_blob,
                       uint64_t blob_cap, uint64_t* d_offs, uint32_t* d_lens, hipStream_t stream, uint64_t* d_sse = nullptr,
                       const QnsArg& qns = kNoQns);
// What a rate entry asks behind the request (amv_rate_plan.h): the ladder as the kernels take it, the uniform budget, the
// budgets on the device (or nullptr).  rate_request_of: q and rate checked and turned into the request (a trellis one, its
// lambda not read) and the RateArg -- everything but the sizes and the outputs, which the entry checks as encode_dev does.
struct RateArg {
    RateLadder ladder;
    uint32_t budget;
    const uint32_t* d_budget;
};
int rate_request_of(amvhip_ctx* c, const amvhip_quant* q, const amvhip_rate* rate, QuantRequest* req, RateArg* arg);
// what is left to check once the size is known to be an encoder's: the request against it, the size against the bits' 32, d_rung
int rate_args_ok(amvhip_ctx* c, uint32_t n, uint32_t w, uint32_t h, const QuantRequest& req, const uint32_t* d_rung);
// the tail of the front-end rate entry: the w x h pictures it made as tight_420 in c->scaled, through rate_core
int rate_scaled_tail(amvhip_ctx* c, uint32_t n, uint32_t w, uint32_t h, uint32_t qbias, const QuantRequest& req, const RateArg& rate,
                     uint8_t* d_blob, uint64_t blob_cap, uint64_t* d_offs, uint32_t* d_lens, uint32_t* d_rung, hipStream_t stream);
// What a clip entry asks beyond its rate sibling (amv_clip_plan.h): the bytes of the whole clip and where the clip record goes.
// clip_args_ok: d_clip.  clip_scaled_tail: rate_scaled_tail's counterpart, through rate_core with the clip.
struct ClipArg {
    uint64_t total;
    uint64_t* d_clip;
};
int clip_args_ok(amvhip_ctx* c, uint32_t n, const uint64_t* d_clip);
int clip_scaled_tail(amvhip_ctx* c, uint32_t n, uint32_t w, uint32_t h, uint32_t qbias, const QuantRequest& req, const RateArg& rate,
                     const ClipArg& clip, uint8_t* d_blob, uint64_t blob_cap, uint64_t* d_offs, uint32_t* d_lens, uint32_t* d_rung,
                     hipStream_t stream);
// The byte-budget flow of the rate and clip entries, the encoder's and the requant side's (amvhip_requant.hip), written once:
// see its definition.  The three steps a caller brings return 0 to go on.  (std::function, not a template over callables:
// the body is amvhip_encode.hip's, the callers' lambdas two files'.)
using BudgetProbe = std::function<int(uint32_t* bits)>;
using BudgetFirstPass = std::function<int(const uint32_t* lambda)>;
using BudgetRedoRound = std::function<int(const FrameSel& sel, uint32_t items, const uint32_t* lambda)>;
int budget_passes(amvhip_ctx* c, const RateArg& rate, const ClipArg* clip, const ClipFrames& frames, uint32_t n, uint32_t blocks, uint32_t round,
                  uint32_t* d_lens, uint32_t* d_rung, const char* who, hipStream_t stream, const BudgetProbe& probe,
                  const BudgetFirstPass& first_pass, const BudgetRedoRound& redo_round);
int resample_launch(amvhip_ctx* c, const PixPicture& src, uint32_t src_w, uint32_t src_h, const PixPicture& dst, uint32_t dst_w, uint32_t dst_h,
                    uint32_t n, bool to_jpeg, hipStream_t st);

}  // namespace amv
