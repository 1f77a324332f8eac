// amvhip_decode.hip -- video decode behind the C ABI: the entropy stage into records, the reconstruction, the fall-back
// rounds through the serial kernel, and the entry points that queue them (one call, submit / collect, host buffers).
#include "amvhip_ctx.h"

using namespace amv;

// unstuffing + the synchronising kernel into the records of `sinks`; fb says what is left for the serial kernel
// lanes: lanes per frame of the synchronising kernel; heavy_lanes != 0 (a batch that gets ONE lane per frame):
// frames whose chunk is over twice the batch's mean get that many lanes instead -- a wave's 64 frames finish together, and one
// noise frame among 63 quiet ones kept them all waiting for six times their own length (a stream with every 16th frame noise
// spent 4.3 ms per 160 000 frames in the entropy kernel for 1.3 times the uniform stream's symbols).  The split is made on the
// device (the lengths are there): two frame lists, two launches that take their frames from them.
static int entropy_front(amvhip_ctx* c, const uint8_t* d_blob, uint64_t blob_bytes, const uint64_t* d_offs, const uint32_t* d_lens, uint32_t n,
                         const FrameGeom& g, SyncSinks sinks, int32_t* d_status, uint32_t* d_nmcu_ok, DevBuf& retry, hipStream_t st,
                         Fallback& fb, int lanes, int heavy_lanes, uint64_t ws_lines, const LayoutSpec& rec_layout) {
    if (c->entropy_mode == AMVHIP_ENTROPY_SERIAL || g.blocks >= 16384u) {
        HIP_TRY(c, hipMemsetAsync(sinks.rec_count, 0xff, (size_t)n * 4, st));   // every frame dense
        fb = Fallback{nullptr, nullptr, n};
        c->last_split = false;
        return AMVHIP_OK;
    }
    if (int r = ensure(c, retry, ((size_t)n + 8) * 4)) return r;   // [retry count, task counter, 6 spare | retry list n]
    if (int r = ensure(c, c->ws, (size_t)ws_lines * 16 + 64)) return r;
    if (int r = ensure(c, c->ws_line, ((size_t)n + 1) * 4)) return r;
    if (int r = ensure(c, c->ws_bytes, (size_t)n * 4)) return r;
    if (int r = ensure(c, c->layout, layout_workspace(n))) return r;
    uint32_t* retry_count = (uint32_t*)retry.p;
    uint32_t* retry_list = retry_count + 8;
    sinks.retry_list = retry_list;
    sinks.retry_count = retry_count;
    // (the layout launch also clears the retry counter and the task queues behind it: retry_count[0 .. 8))
    launch_layout(d_lens, n, LayoutSpec{2u, 32u, 0xffffffe0u, 4u, (uint32_t)ws_lines, (uint32_t*)c->ws_line.p}, rec_layout, c->layout.p,
                  retry_count, 8u, c->layout_large, st);
    if (int r = check_launch(c, "layout")) return r;
    {
        Timed t(c, AMVHIP_K_UNSTUFF, st);
        launch_unstuff(d_blob, blob_bytes, d_offs, d_lens, n, (const uint32_t*)c->ws_line.p, (uint32_t*)c->ws.p, (uint32_t*)c->ws_bytes.p,
                       retry_list, retry_count, st);
    }
    if (int r = check_launch(c, "unstuff")) return r;
    unsigned long long* stats = c->want_stats ? (unsigned long long*)c->stats.p : nullptr;
    const HuffDecodeImage* dec = (const HuffDecodeImage*)c->d_dec.p;
    c->last_split = heavy_lanes != 0;
    if (heavy_lanes) {
        if (int r = ensure(c, c->split, ((size_t)n * 2 + 8) * 4)) return r;   // [heavy count, light count, 6 spare | heavy list n | light list n]
        uint32_t* split_count = (uint32_t*)c->split.p;
        uint32_t *heavy = split_count + 8, *light = heavy + n;
        HIP_TRY(c, hipMemsetAsync(split_count, 0, 32, st));
        launch_split_by_weight(d_lens, n, (const uint32_t*)c->ws_line.p, heavy, light, split_count, st);
        if (int r = check_launch(c, "split")) return r;
        Timed t(c, AMVHIP_K_HUFFMAN, st);
        // the heavy frames first: their launch is a few waves deep and as long as its slowest frame's chain, the light
        // frames' launch behind it fills the chip
        launch_huffman_sync((const uint32_t*)c->ws.p, (const uint32_t*)c->ws_bytes.p, n, heavy, split_count, g, (const uint32_t*)c->ws_line.p,
                            heavy_lanes, dec, sinks, d_status, d_nmcu_ok, retry_count + 2, stats, c->cus, st);
        launch_huffman_sync((const uint32_t*)c->ws.p, (const uint32_t*)c->ws_bytes.p, n, light, split_count + 1, g, (const uint32_t*)c->ws_line.p,
                            lanes, dec, sinks, d_status, d_nmcu_ok, retry_count + 1, stats, c->cus, st);
    } else {
        Timed t(c, AMVHIP_K_HUFFMAN, st);
        launch_huffman_sync((const uint32_t*)c->ws.p, (const uint32_t*)c->ws_bytes.p, n, nullptr, nullptr, g, (const uint32_t*)c->ws_line.p,
                            lanes, dec, sinks, d_status, d_nmcu_ok, retry_count + 1, stats, c->cus, st);
    }
    fb = Fallback{retry_list, retry_count, n};
    return check_launch(c, "huffman_sync");
}

// Which back half a call's (flags, lowres) ask for, and what follows from that for its output: decided once per call.
struct BackHalf {
    enum Kind { kBgr, kYuv, kYuvLowres } kind;   // amvlib's BGR; the patched FFmpeg's YUVJ420P planes; ... at 1/2, 1/4, 1/8 size
    uint32_t flags, lowres;
    uint64_t frame_bytes;                        // of the output
    bool covered;   // false: bytes no kernel writes (row padding, AMVDec.c:283; plane rows mjpegdec.c:672-677 skips) are cleared first
};
static BackHalf back_half(uint32_t flags, uint32_t lowres, const FrameGeom& g) {
    const bool keep = (flags & AMVHIP_FLAG_FFMPEG_KEEP) != 0;
    if (lowres)
        return {BackHalf::kYuvLowres, flags, lowres, lowres_frame_bytes(g.width, g.height, lowres), keep || lowres_store_covers_planes(g.height, lowres)};
    if (flags & AMVHIP_FLAG_FFMPEG)
        return {BackHalf::kYuv, flags, 0u, amvhip_yuv420_frame_bytes(g.width, g.height), keep || yuv_store_covers_planes(g)};
    return {BackHalf::kBgr, flags, 0u, g.frame_bytes, keep || g.stride == g.width * 3};
}

static int reconstruct_launch(amvhip_ctx* c, const SyncSinks& sinks, const uint32_t* d_nmcu_ok, uint32_t n, const FrameSel& sel,
                              uint32_t items, const FrameGeom& g, const BackHalf& bh, uint8_t* d_out, hipStream_t st) {
    Timed t(c, AMVHIP_K_RECON, st);
    switch (bh.kind) {
        case BackHalf::kYuvLowres: launch_reconstruct_yuv_lowres(sinks, d_nmcu_ok, n, sel, items, g, bh.lowres, d_out, st); break;
        case BackHalf::kYuv: launch_reconstruct_yuv(sinks, d_nmcu_ok, n, sel, items, g, bh.frame_bytes, d_out, st); break;
        case BackHalf::kBgr: launch_reconstruct(sinks, d_nmcu_ok, n, sel, items, g, bh.flags, d_out, st); break;
    }
    return check_launch(c, "reconstruct");
}

static int clear_unwritten(amvhip_ctx* c, uint32_t n, const BackHalf& bh, uint8_t* d_out, hipStream_t st) {
    if (!bh.covered) HIP_TRY(c, hipMemsetAsync(d_out, 0, bh.frame_bytes * n, st));
    return AMVHIP_OK;
}

// amvhip_reconstruct_dev and amvhip_reconstruct_lowres_dev (`who`) behind their own argument checks
static int reconstruct_dense(amvhip_ctx* c, const char* who, const int16_t* d_coef, const uint32_t* d_nmcu_ok, uint32_t n, uint32_t w,
                             uint32_t h, uint32_t flags, uint32_t lowres, uint8_t* d_out, void* stream) {
    if (!size_ok(w, h) || (n && (!d_coef || !d_nmcu_ok || !d_out))) return fail(c, AMVHIP_ERR_ARG, "%s: bad argument", who);
    if (((uintptr_t)d_out & 3u) || ((uintptr_t)d_coef & 15u)) return fail(c, AMVHIP_ERR_ARG, "%s: out must be 4-byte, coef 16-byte aligned", who);
    if (int r = use_device(c)) return r;
    if (n == 0) return AMVHIP_OK;
    const FrameGeom g = make_geom(w, h);
    const BackHalf bh = back_half(flags, lowres, g);
    SyncSinks sinks{};
    sinks.coef = const_cast<int16_t*>(d_coef);
    if (int r = clear_unwritten(c, n, bh, d_out, (hipStream_t)stream)) return r;
    return reconstruct_launch(c, sinks, d_nmcu_ok, n, kAllFrames, n, g, bh, d_out, (hipStream_t)stream);
}

extern "C" int amvhip_reconstruct_dev(amvhip_ctx* c, const int16_t* d_coef, const uint32_t* d_nmcu_ok, uint32_t n, uint32_t w, uint32_t h,
                                      uint32_t flags, uint8_t* d_out, void* stream) {
    if (!c) return AMVHIP_ERR_ARG;
    return reconstruct_dense(c, "reconstruct", d_coef, d_nmcu_ok, n, w, h, flags, 0u, d_out, stream);
}

int amv::decode_args_ok(amvhip_ctx* c, const uint8_t* d_blob, const uint64_t* d_offs, const uint32_t* d_lens, uint32_t n, uint32_t w,
                          uint32_t h, uint32_t flags, const uint8_t* d_out, const int32_t* d_status) {
    if (!size_ok(w, h)) return fail(c, AMVHIP_ERR_ARG, "decode: bad size %ux%u", w, h);
    if ((flags & AMVHIP_FLAG_FFMPEG_KEEP) && !(flags & AMVHIP_FLAG_FFMPEG))
        return fail(c, AMVHIP_ERR_ARG, "decode: AMVHIP_FLAG_FFMPEG_KEEP is a mode of AMVHIP_FLAG_FFMPEG");
    if (n == 0) return AMVHIP_OK;
    if (!d_blob || !d_offs || !d_lens || !d_out || !d_status) return fail(c, AMVHIP_ERR_ARG, "decode: null argument");
    if (((uintptr_t)d_blob & 3u) || ((uintptr_t)d_out & 3u)) return fail(c, AMVHIP_ERR_ARG, "decode: blob and out must be 4-byte aligned");
    return AMVHIP_OK;
}

// The entropy stage of a decode call into the hand-over set b: sizes the record space, the segment bounds, the lane table
// and the record counts, then runs entropy_front.  Statuses and nmcu_ok go to d_status / d_nmcu_ok (ok_in_blocks: nmcu_ok
// counts whole blocks, AMVHIP_FLAG_FFMPEG_KEEP).  sinks: where the records are; its coef is left null.
int amv::entropy_records(amvhip_ctx* c, const uint8_t* d_blob, uint64_t blob_bytes, const uint64_t* d_offs, const uint32_t* d_lens,
                         uint32_t n, const FrameGeom& g, bool ok_in_blocks, int32_t* d_status, uint32_t* d_nmcu_ok, DecodeSet& b,
                         hipStream_t st, SyncSinks& sinks, Fallback& fb) {
    const EntropyPlan p = entropy_plan(n, blob_bytes, g);   // the record space and the unstuffed scans' window (amv_host_plan.h)
    const uint32_t lanes = (uint32_t)huffman_sync_lanes(n, c->cus, c->sync_lanes, (uint64_t)g.width * g.height);
    // a batch that gets one lane per frame gives its heavy frames kHeavyLanes (entropy_front); AMVHIP_SPLIT=0: every frame one
    const uint32_t heavy_lanes = lanes == 1u && c->split_heavy ? c->heavy_lanes : 0u;
    const uint32_t tab_lanes = heavy_lanes ? heavy_lanes : lanes;       // a frame's row in lane_tab
    if (int r = ensure(c, b.rec, (size_t)p.cap_lines * 128 + 16)) return r;   // + what a 16-byte read of a frame's last records may overshoot
    if (int r = ensure(c, b.rec_line, ((size_t)n + 1) * 4)) return r;
    const LayoutSpec rec_layout{4u, p.add_rec, p.hi_rec, 5u, (uint32_t)p.cap_lines, (uint32_t*)b.rec_line.p};   // laid out by entropy_front's launch
    if (int r = ensure(c, b.seg_start, (size_t)n * (p.segs + 1) * 8)) return r;
    if (int r = ensure(c, b.lane_tab, (size_t)n * tab_lanes * 16)) return r;
    if (int r = ensure(c, b.rec_count, (size_t)n * 4)) return r;
    sinks = SyncSinks{};
    sinks.rec = (uint32_t*)b.rec.p;
    sinks.rec_line = (const uint32_t*)b.rec_line.p;
    sinks.seg_start = (uint32_t*)b.seg_start.p;
    sinks.lane_tab = (uint32_t*)b.lane_tab.p;
    sinks.lanes = tab_lanes;
    sinks.rec_count = (uint32_t*)b.rec_count.p;
    sinks.ok_in_blocks = ok_in_blocks ? 1u : 0u;
    c->last_decode_retry = &b.retry;
    return entropy_front(c, d_blob, blob_bytes, d_offs, d_lens, n, g, sinks, d_status, d_nmcu_ok, b.retry, st, fb, (int)lanes, (int)heavy_lanes,
                         p.ws_lines, rec_layout);
}

extern "C" int amvhip_huffman_decode_dev(amvhip_ctx* c, const uint8_t* d_blob, uint64_t blob_bytes, const uint64_t* d_offs,
                                         const uint32_t* d_lens, uint32_t n, uint32_t w, uint32_t h, int16_t* d_coef, int32_t* d_status,
                                         uint32_t* d_nmcu_ok, void* stream) {
    if (!c) return AMVHIP_ERR_ARG;
    if (!size_ok(w, h) || (n && (!d_blob || !d_offs || !d_lens || !d_coef || !d_status || !d_nmcu_ok)))
        return fail(c, AMVHIP_ERR_ARG, "huffman_decode: bad argument");
    if (((uintptr_t)d_blob & 3u) || ((uintptr_t)d_coef & 15u)) return fail(c, AMVHIP_ERR_ARG, "huffman_decode: blob must be 4-byte, coef 16-byte aligned");
    if (int r = use_device(c)) return r;
    if (n == 0) return AMVHIP_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    const FrameGeom g = make_geom(w, h);
    hipStream_t st = (hipStream_t)stream;
    // the entropy stage of amvhip_decode_batch_dev, into its hand-over set; the records become the caller's lines
    SyncSinks sinks;
    Fallback fb;
    if (int r = entropy_records(c, d_blob, blob_bytes, d_offs, d_lens, n, g, false, d_status, d_nmcu_ok, c->set[0], st, sinks, fb))
        return r;
    if (fb.list) {   // (without a list every frame is the serial kernel's)
        launch_expand_records(sinks, d_nmcu_ok, n, g, d_coef, st);
        if (int r = check_launch(c, "expand_records")) return r;
    }
    {   // the caller's array has a place for every frame: one launch, lines at the frames' own places
        Timed t(c, AMVHIP_K_HUFFMAN_SERIAL, st);
        launch_huffman(d_blob, blob_bytes, d_offs, d_lens, n, g, (const HuffDecodeImage*)c->d_dec.p, d_coef, d_status, d_nmcu_ok, fb.list,
                       fb.count, 0u, fb.items, false, false, st);
    }
    return check_launch(c, "huffman");
}

// The entropy stage goes to stream `front`, everything that writes d_out to `back` (the same stream, or two of the
// context's own with `back` waiting for `front`).  Caller holds the lock.
int amv::decode_core(amvhip_ctx* c, const uint8_t* d_blob, uint64_t blob_bytes, const uint64_t* d_offs, const uint32_t* d_lens,
                       uint32_t n, uint32_t w, uint32_t h, uint32_t flags, uint8_t* d_out, int32_t* d_status, DecodeSet& b,
                       hipStream_t front, hipStream_t back, uint32_t lowres) {
    const FrameGeom g = make_geom(w, h);
    const BackHalf bh = back_half(flags, lowres, g);
    // (rounds of up to 16 384 frames: every round is a pair of launches that usually find nothing to do, and a batch that
    // small is latency-bound -- three rounds cost the 10 000-frame stream 3 % of its step)
    const uint32_t round = fallback_round(n, g, 16384u, 4u);
    if (int r = ensure(c, c->coef, (size_t)round * g.blocks * 128)) return r;
    if (int r = ensure(c, b.nmcu, (size_t)n * 4)) return r;
    uint32_t* d_nmcu = (uint32_t*)b.nmcu.p;
    // AMVHIP_FLAG_FFMPEG_KEEP: b.nmcu is the context's own array, so it may count whole blocks, not whole MCUs
    SyncSinks sinks;
    Fallback fb;
    if (int r = entropy_records(c, d_blob, blob_bytes, d_offs, d_lens, n, g, (flags & AMVHIP_FLAG_FFMPEG_KEEP) != 0, d_status, d_nmcu, b, front,
                                sinks, fb))
        return r;
    sinks.coef = (int16_t*)c->coef.p;
    if (back != front) {
        HIP_TRY(c, hipEventRecord(c->ev_front, front));
        HIP_TRY(c, hipStreamWaitEvent(back, c->ev_front, 0));
    }
    hipStream_t st = back;
    if (int r = clear_unwritten(c, n, bh, d_out, st)) return r;
    if (fb.list)   // the frames in records form (a launch that skips the others)
        if (int r = reconstruct_launch(c, sinks, d_nmcu, n, kAllFrames, n, g, bh, d_out, st)) return r;
    // The others, a round of dense lines at a time.  With a list the count is on the device: the rounds past it find
    // nothing to do and leave at once (usually all of them: one pair of empty launches per round).
    for (uint32_t base = 0; base < fb.items; base += round) {
        const uint32_t items = fb.items - base < round ? fb.items - base : round;
        {
            Timed t(c, AMVHIP_K_HUFFMAN_SERIAL, st);
            launch_huffman(d_blob, blob_bytes, d_offs, d_lens, n, g, (const HuffDecodeImage*)c->d_dec.p, sinks.coef, d_status, d_nmcu, fb.list,
                           fb.count, base, items, true, sinks.ok_in_blocks != 0u, st);
        }
        if (int r = check_launch(c, "huffman")) return r;
        if (int r = reconstruct_launch(c, sinks, d_nmcu, n, FrameSel{fb.list, fb.count, base, items}, items, g, bh, d_out, st)) return r;
    }
    c->ws_bytes_per_frame = (double)(c->ws.cap + c->coef.cap + c->ws_bytes.cap + c->ws_line.cap + c->set[0].cap() + c->set[1].cap()) / n;
    return AMVHIP_OK;
}

extern "C" int amvhip_decode_batch_dev(amvhip_ctx* c, const uint8_t* d_blob, uint64_t blob_bytes, const uint64_t* d_offs, const uint32_t* d_lens,
                                       uint32_t n, uint32_t w, uint32_t h, uint32_t flags, uint8_t* d_out, int32_t* d_status, void* stream) {
    if (!c) return AMVHIP_ERR_ARG;
    if (int r = decode_args_ok(c, d_blob, d_offs, d_lens, n, w, h, flags, d_out, d_status)) return r;
    if (n == 0) return AMVHIP_OK;
    if (int r = use_device(c)) return r;
    std::lock_guard<std::mutex> lk(c->mu);
    return decode_core(c, d_blob, blob_bytes, d_offs, d_lens, n, w, h, flags, d_out, d_status, c->set[0], (hipStream_t)stream,
                       (hipStream_t)stream);
}

// ---- the same in two halves, for a caller with more than one batch in hand ---------------------------------------
// submit: the batch's inputs are ready where `stream` stands now (an event is recorded there); the entropy stage is
// queued on the context's `front` stream, the reconstruction on its `back` stream, and `stream` is NOT made to wait.
// collect: `stream` waits for the oldest batch submitted and not yet collected.  With submit(k+1) called before
// collect(k), the entropy stage of batch k+1 runs beside the reconstruction of batch k -- the two are limited by
// different things (amv_huffman_fast_kernel by memory latency and scattered stores, amv_reconstruct_kernel by VALU
// issue).  At most two batches between submit and collect: the hand-over buffers exist twice.
extern "C" int amvhip_decode_submit_dev(amvhip_ctx* c, const uint8_t* d_blob, uint64_t blob_bytes, const uint64_t* d_offs,
                                        const uint32_t* d_lens, uint32_t n, uint32_t w, uint32_t h, uint32_t flags, uint8_t* d_out,
                                        int32_t* d_status, void* stream) {
    if (!c) return AMVHIP_ERR_ARG;
    if (int r = decode_args_ok(c, d_blob, d_offs, d_lens, n, w, h, flags, d_out, d_status)) return r;
    if (int r = select_device(c)) return r;
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->submitted - c->collected >= 2) return fail(c, AMVHIP_ERR_ARG, "decode_submit: two batches are in flight, collect one first");
    if (!c->front) {
        // the entropy stage's few large workgroups (127 KB of LDS) ahead of the reconstruction's many small ones
        int least = 0, greatest = 0;
        HIP_TRY(c, hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIP_TRY(c, hipStreamCreateWithPriority(&c->front, hipStreamNonBlocking, greatest));
        HIP_TRY(c, hipStreamCreateWithPriority(&c->back, hipStreamNonBlocking, least));
        for (hipEvent_t* e : {&c->ev_in, &c->ev_front, &c->ev_done[0], &c->ev_done[1]})
            HIP_TRY(c, hipEventCreateWithFlags(e, hipEventDisableTiming));
    }
    const int which = (int)(c->submitted & 1u);
    HIP_TRY(c, hipEventRecord(c->ev_in, (hipStream_t)stream));
    HIP_TRY(c, hipStreamWaitEvent(c->front, c->ev_in, 0));
    // (the hand-over set this batch writes was last read by the reconstruction of the batch two before: on `back`,
    // ahead of the batch before this one -- whose entropy stage `front` has already gone through -- but not of `front`)
    if (c->submitted >= 2) HIP_TRY(c, hipStreamWaitEvent(c->front, c->ev_done[which], 0));
    if (n != 0) {
        if (int r = decode_core(c, d_blob, blob_bytes, d_offs, d_lens, n, w, h, flags, d_out, d_status, c->set[which], c->front, c->back))
            return r;
    } else {   // nothing to decode: `back` still has to pass the point where the inputs are ready
        HIP_TRY(c, hipEventRecord(c->ev_front, c->front));
        HIP_TRY(c, hipStreamWaitEvent(c->back, c->ev_front, 0));
    }
    HIP_TRY(c, hipEventRecord(c->ev_done[which], c->back));
    ++c->submitted;
    return AMVHIP_OK;
}

extern "C" int amvhip_decode_collect_dev(amvhip_ctx* c, void* stream) {
    if (!c) return AMVHIP_ERR_ARG;
    if (int r = select_device(c)) return r;
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->collected == c->submitted) return fail(c, AMVHIP_ERR_ARG, "decode_collect: nothing submitted");
    HIP_TRY(c, hipStreamWaitEvent((hipStream_t)stream, c->ev_done[c->collected & 1u], 0));
    ++c->collected;
    return AMVHIP_OK;
}

// device workspace the last amvhip_decode_batch_dev call held, in bytes per frame of that call (a diagnostic)
extern "C" double amvhip_decode_workspace_per_frame(const amvhip_ctx* c) { return c ? c->ws_bytes_per_frame : 0.0; }

extern "C" int amvhip_decode_batch_async(amvhip_ctx* c, const uint8_t* blob, uint64_t blob_bytes, const uint64_t* offs, const uint32_t* lens,
                                         uint32_t n, uint32_t w, uint32_t h, uint32_t flags, uint8_t* out, int32_t* status) {
    if (!c) return AMVHIP_ERR_ARG;
    if (!size_ok(w, h) || (n && (!blob || !offs || !lens || !out))) return fail(c, AMVHIP_ERR_ARG, "decode: bad argument");
    if (n == 0) return AMVHIP_OK;
    hipStream_t st;
    if (int r = host_stream(c, &st)) return r;
    const uint64_t fb = back_half(flags, 0u, make_geom(w, h)).frame_bytes;
    // the staging buffers belong to the context: one host-buffer call at a time grows and fills them (hmu orders the
    // host-buffer entry points among themselves; mu, taken inside the _dev calls, orders the kernels' workspace)
    std::lock_guard<std::mutex> hlk(c->hmu);
    if (!c->dstream) {
        HIP_TRY(c, hipStreamCreateWithFlags(&c->dstream, hipStreamNonBlocking));
        for (hipEvent_t* e : {&c->ev_decoded, &c->ev_copied[0], &c->ev_copied[1]}) HIP_TRY(c, hipEventCreateWithFlags(e, hipEventDisableTiming));
    }
    const uint32_t which = (uint32_t)(c->async_calls & 1u);
    DevBuf &d_frames = c->v_out[which], &d_st = c->v_status[which];
    if (int r = ensure(c, d_frames, fb * n)) return r;          // (growing one frees the old: hipFree waits for the device)
    if (int r = ensure(c, d_st, (size_t)n * 4)) return r;
    // the copy that last read this staging buffer (the call before the last one) must be done before the kernels write it
    if (c->async_calls >= 2) HIP_TRY(c, hipStreamWaitEvent(st, c->ev_copied[which], 0));
    if (int r = stage(c, c->h_in, blob_bytes + 16, blob, blob_bytes, st)) return r;
    if (int r = stage(c, c->h_offs, (size_t)n * 8, offs, (size_t)n * 8, st)) return r;
    if (int r = stage(c, c->h_lens, (size_t)n * 4, lens, (size_t)n * 4, st)) return r;
    // AMVHIP_FLAG_FFMPEG_KEEP: what no block covers stays as the CALLER had it -- the caller's frames go up first
    if (flags & AMVHIP_FLAG_FFMPEG_KEEP) HIP_TRY(c, hipMemcpyAsync(d_frames.p, out, fb * n, hipMemcpyHostToDevice, st));
    if (int r = amvhip_decode_batch_dev(c, (const uint8_t*)c->h_in.p, blob_bytes, (const uint64_t*)c->h_offs.p,
                                        (const uint32_t*)c->h_lens.p, n, w, h, flags, (uint8_t*)d_frames.p, (int32_t*)d_st.p, st))
        return r;
    HIP_TRY(c, hipEventRecord(c->ev_decoded, st));
    HIP_TRY(c, hipStreamWaitEvent(c->dstream, c->ev_decoded, 0));
    // From the first copy queued on dstream on, a failure must not leave this staging buffer with a copy in flight that
    // no event stands for: the call after the next would pick the buffer again, wait for an event recorded two calls
    // earlier, and let its kernels write under the orphaned copy.  So whatever fails below, dstream is drained before
    // the call returns, and the call counts (the buffers keep taking turns).
    hipError_t e = hipMemcpyAsync(out, d_frames.p, fb * n, hipMemcpyDeviceToHost, c->dstream);
    if (e == hipSuccess && status) e = hipMemcpyAsync(status, d_st.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->dstream);
    if (e == hipSuccess) e = hipEventRecord(c->ev_copied[which], c->dstream);
    ++c->async_calls;
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(c->dstream);
        (void)hipEventRecord(c->ev_copied[which], c->dstream);   // (what the call after the next will wait for: nothing pending)
        return fail(c, AMVHIP_ERR_DEVICE, "decode_batch_async: copy back: %s", hipGetErrorString(e));
    }
    return AMVHIP_OK;
}

extern "C" int amvhip_decode_batch(amvhip_ctx* c, const uint8_t* blob, uint64_t blob_bytes, const uint64_t* offs, const uint32_t* lens,
                                   uint32_t n, uint32_t w, uint32_t h, uint32_t flags, uint8_t* out, int32_t* status) {
    if (int r = amvhip_decode_batch_async(c, blob, blob_bytes, offs, lens, n, w, h, flags, out, status)) return r;
    return amvhip_sync(c);
}


// ---- reduced-size decode (lowres 1..3): include/amvhip.h states the rule ------------------------------------------------
extern "C" uint32_t amvhip_lowres_dim(uint32_t full, uint32_t lowres) { return lowres_dim(full, lowres); }

extern "C" uint64_t amvhip_lowres_frame_bytes(uint32_t w, uint32_t h, uint32_t lowres) { return lowres_frame_bytes(w, h, lowres); }

extern "C" int amvhip_reconstruct_lowres_dev(amvhip_ctx* c, const int16_t* d_coef, const uint32_t* d_nmcu_ok, uint32_t n, uint32_t w, uint32_t h,
                                             uint32_t lowres, uint8_t* d_out, void* stream) {
    if (!c) return AMVHIP_ERR_ARG;
    if (lowres < 1u || lowres > 3u) return fail(c, AMVHIP_ERR_ARG, "reconstruct_lowres: lowres must be 1, 2 or 3");
    return reconstruct_dense(c, "reconstruct_lowres", d_coef, d_nmcu_ok, n, w, h, AMVHIP_FLAG_FFMPEG, lowres, d_out, stream);
}

// what both decode entry points ask of the mode, the format and the row pitch (before anything touches a device)
static int lowres_args_ok(amvhip_ctx* c, uint32_t w, uint32_t flags, uint32_t lowres, int dst_fmt, uint32_t out_stride) {
    if (flags != AMVHIP_FLAG_FFMPEG)
        return fail(c, AMVHIP_ERR_ARG, "decode_lowres: flags must be exactly AMVHIP_FLAG_FFMPEG (the reduced planes are that decoder's)");
    if (lowres < 1u || lowres > 3u) return fail(c, AMVHIP_ERR_ARG, "decode_lowres: lowres must be 1, 2 or 3");
    const uint32_t wl = lowres_dim(w, lowres);
    if (dst_fmt == AMVHIP_PIX_YUVJ420P) {
        if (out_stride != wl) return fail(c, AMVHIP_ERR_ARG, "decode_lowres: the YUVJ420P planes are tight, out_stride must be %u", wl);
    } else {
        if (pix_route(AMVHIP_PIX_YUVJ420P, dst_fmt) == kRouteNone)
            return fail(c, AMVHIP_ERR_ARG, "decode_lowres: no one-step route from YUVJ420P to format %d", dst_fmt);
        if (out_stride < wl * pix_bpp(dst_fmt)) return fail(c, AMVHIP_ERR_ARG, "decode_lowres: out_stride below the row");
    }
    return AMVHIP_OK;
}

extern "C" int amvhip_decode_lowres_batch_dev(amvhip_ctx* c, const uint8_t* d_blob, uint64_t blob_bytes, const uint64_t* d_offs,
                                              const uint32_t* d_lens, uint32_t n, uint32_t w, uint32_t h, uint32_t flags, uint32_t lowres,
                                              int dst_fmt, uint8_t* d_out, uint32_t out_stride, int32_t* d_status, void* stream) {
    if (!c) return AMVHIP_ERR_ARG;
    if (int r = lowres_args_ok(c, w, flags, lowres, dst_fmt, out_stride)) return r;
    if (int r = decode_args_ok(c, d_blob, d_offs, d_lens, n, w, h, flags, d_out, d_status)) return r;
    if (n == 0) return AMVHIP_OK;
    if (int r = use_device(c)) return r;
    std::lock_guard<std::mutex> lk(c->mu);
    hipStream_t st = (hipStream_t)stream;
    if (dst_fmt == AMVHIP_PIX_YUVJ420P) return decode_core(c, d_blob, blob_bytes, d_offs, d_lens, n, w, h, flags, d_out, d_status, c->set[0], st, st, lowres);
    // the other formats: the planes in the context's workspace, then img_convert at the reduced size
    const uint32_t wl = lowres_dim(w, lowres), hl = lowres_dim(h, lowres);
    if (int r = ensure(c, c->pix_dec, lowres_frame_bytes(w, h, lowres) * n)) return r;
    if (int r = decode_core(c, d_blob, blob_bytes, d_offs, d_lens, n, w, h, flags, (uint8_t*)c->pix_dec.p, d_status, c->set[0], st, st, lowres))
        return r;
    const uint64_t out_frame = pix_frame_bytes(dst_fmt, out_stride, hl);
    PixPicture dst = make_picture(d_out, nullptr, nullptr, out_stride, (out_stride + 1) / 2, out_frame, out_frame);
    if (dst_fmt == AMVHIP_PIX_YUV420P) {
        dst.p[1] = d_out + (uint64_t)out_stride * hl;
        dst.p[2] = dst.p[1] + (uint64_t)dst.stride[1] * ((hl + 1) / 2);
    }
    return pix_convert_launch(c, AMVHIP_PIX_YUVJ420P, tight_420((uint8_t*)c->pix_dec.p, wl, hl), dst_fmt, dst, wl, hl, n, st);
}

extern "C" int amvhip_decode_lowres_batch(amvhip_ctx* c, const uint8_t* blob, uint64_t blob_bytes, const uint64_t* offs, const uint32_t* lens,
                                          uint32_t n, uint32_t w, uint32_t h, uint32_t flags, uint32_t lowres, int dst_fmt, uint8_t* out,
                                          uint32_t out_stride, int32_t* status) {
    if (!c) return AMVHIP_ERR_ARG;
    if (int r = lowres_args_ok(c, w, flags, lowres, dst_fmt, out_stride)) return r;
    if (!size_ok(w, h) || (n && (!blob || !offs || !lens || !out))) return fail(c, AMVHIP_ERR_ARG, "decode_lowres: bad argument");
    if (n == 0) return AMVHIP_OK;
    hipStream_t st;
    if (int r = host_stream(c, &st)) return r;
    const uint64_t fb = pix_frame_bytes(dst_fmt, out_stride, lowres_dim(h, lowres));
    std::lock_guard<std::mutex> hlk(c->hmu);
    if (int r = stage(c, c->h_in, blob_bytes + 16, blob, blob_bytes, st)) return r;
    if (int r = stage(c, c->h_offs, (size_t)n * 8, offs, (size_t)n * 8, st)) return r;
    if (int r = stage(c, c->h_lens, (size_t)n * 4, lens, (size_t)n * 4, st)) return r;
    // bytes between a row's end and out_stride stay as the CALLER had them: the caller's frames go up first
    if (int r = ensure(c, c->h_out, fb * n)) return r;
    if (dst_fmt != AMVHIP_PIX_YUVJ420P) HIP_TRY(c, hipMemcpyAsync(c->h_out.p, out, fb * n, hipMemcpyHostToDevice, st));
    if (int r = ensure(c, c->h_status, (size_t)n * 4)) return r;
    if (int r = amvhip_decode_lowres_batch_dev(c, (const uint8_t*)c->h_in.p, blob_bytes, (const uint64_t*)c->h_offs.p, (const uint32_t*)c->h_lens.p,
                                               n, w, h, flags, lowres, dst_fmt, (uint8_t*)c->h_out.p, out_stride, (int32_t*)c->h_status.p, st))
        return r;
    HIP_TRY(c, hipMemcpyAsync(out, c->h_out.p, fb * n, hipMemcpyDeviceToHost, st));
    if (status) HIP_TRY(c, hipMemcpyAsync(status, c->h_status.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    return AMVHIP_OK;
}
